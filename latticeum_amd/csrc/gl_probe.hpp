// gl_probe.hpp -- a test aid: one evaluation of each gl.hpp primitive (and, on the
// device, of the slot.hpp / ring.hpp products built on them) per element, so the
// arithmetic can be driven with directed inputs and compared with plain integers.
// gl_probe.hip wraps it in kernels (lf_dev_gl_probe); tests/test_gl_host.py compiles
// the same functions for the host. The op codes are oracle/gl_model.py's OPS.
#pragma once
#include <utility>

#include "gl.hpp"
#if defined(GL_PROBE_DEVICE)
#include "ring.hpp"
#include "slot.hpp"
#endif

namespace glp {

enum Op : int {
  OP_CANON = 0,
  OP_ADD = 1,
  OP_SUB = 2,
  OP_NEG = 3,
  OP_REDUCE128 = 4,         // a = lo, b = hi; weakly reduced out
  OP_MUL = 5,               // any u64 operands
  OP_MUL_POW2 = 6,          // s a template constant
  OP_MUL_POW2_RT = 7,       // s a run-time value (as fq3_mul's callers reach it)
  OP_SHL96 = 8,             // s a template constant, 0 .. 95
  OP_SHL192 = 9,            // s a template constant, 0 .. 191
  OP_SHL_SMALL_WEAK = 10,   // s a template constant, 1 .. 31; weakly reduced out
  OP_ADD_WEAK = 11,         // a any u64, b canonical; weakly reduced out
  OP_FROM_X_Y32 = 12,       // a, b the bit patterns of signed X, Y
  OP_ACC_REDUCE = 13,       // sum of m products through Acc
  OP_ACC_ADD = 14,          // sum of m (a b + a + b): acc_mad, then acc_add of both operands
  OP_CACC_REDUCE = 15,      // sum of m products through CAcc
  OP_CACC_REDUCE_WEAK = 16, // weakly reduced out
  OP_CACC_REDUCE_TERMS = 17,
  OP_FQ3_MUL = 18,          // 3-word elements from here on, except the two below
  OP_TO_MONT = 19,
  OP_FROM_MONT = 20,
  OP_S_MUL3 = 21,
  OP_S_MUL_W3 = 22,         // s_mul_w then s_canon
  OP_S_MAD2_3 = 23,         // m = 2: a0 b0 + a1 b1
  OP_SACC3 = 24,            // m sacc_mad, sacc_final
  OP_FQ3ACC = 25,           // m fq3acc_mad, fq3acc_final
  OP_COUNT = 26
};

constexpr int MAX_M = 4096;

LF_HD int words(int op) { return (op == OP_FQ3_MUL || op >= OP_S_MUL3) ? 3 : 1; }
LF_HD bool is_const_shift(int op) {
  return op == OP_MUL_POW2 || op == OP_SHL96 || op == OP_SHL192 || op == OP_SHL_SMALL_WEAK;
}
LF_HD bool takes_b(int op) {
  return !(op == OP_CANON || op == OP_NEG || op == OP_MUL_POW2 || op == OP_MUL_POW2_RT || op == OP_SHL96 ||
           op == OP_SHL192 || op == OP_SHL_SMALL_WEAK || op == OP_TO_MONT || op == OP_FROM_MONT);
}
// the shift amounts an op takes: [lo, hi)
LF_HD void shift_range(int op, int &lo, int &hi) {
  lo = 0;
  hi = 1;
  if (op == OP_MUL_POW2 || op == OP_MUL_POW2_RT || op == OP_SHL192) hi = 192;
  if (op == OP_SHL96) hi = 96;
  if (op == OP_SHL_SMALL_WEAK) lo = 1, hi = 32;
}
LF_HD bool m_ok(int op, int m) {
  if (op == OP_ACC_REDUCE || op == OP_ACC_ADD || op == OP_CACC_REDUCE || op == OP_CACC_REDUCE_WEAK ||
      op == OP_CACC_REDUCE_TERMS || op == OP_SACC3 || op == OP_FQ3ACC)
    return m >= 1 && m <= MAX_M;
  return m == (op == OP_S_MAD2_3 ? 2 : 1);
}

// the shifting primitives at a shift amount that folds to a constant, as the kernels reach them
template <int OP, int S>
LF_HD uint64_t shift_const(uint64_t x) {
  if constexpr (OP == OP_MUL_POW2)
    return gl::mul_pow2(x, S);
  else if constexpr (OP == OP_SHL96)
    return gl::shl96(x, S);
  else if constexpr (OP == OP_SHL192)
    return gl::shl192(x, S);
  else
    return gl::shl_small_weak(x, S);
}

// element i of every other op: a, b hold m words(op) operand words per element
LF_HD void elem(int op, const uint64_t *a, const uint64_t *b, int s, int m, size_t i, uint64_t *out) {
  switch (op) {
    case OP_CANON: out[i] = gl::canon(a[i]); break;
    case OP_ADD: out[i] = gl::add(a[i], b[i]); break;
    case OP_SUB: out[i] = gl::sub(a[i], b[i]); break;
    case OP_NEG: out[i] = gl::neg(a[i]); break;
    case OP_REDUCE128: out[i] = gl::reduce128(a[i], b[i]); break;
    case OP_MUL: out[i] = gl::mul(a[i], b[i]); break;
    case OP_MUL_POW2_RT: out[i] = gl::mul_pow2(a[i], s); break;
    case OP_ADD_WEAK: out[i] = gl::add_weak(a[i], b[i]); break;
    case OP_FROM_X_Y32: out[i] = gl::from_x_y32((int64_t)a[i], (int64_t)b[i]); break;
    case OP_TO_MONT: out[i] = gl::to_mont(a[i]); break;
    case OP_FROM_MONT: out[i] = gl::from_mont(a[i]); break;
    case OP_FQ3_MUL: gl::fq3_mul(a + 3 * i, b + 3 * i, out + 3 * i); break;
    case OP_ACC_REDUCE:
    case OP_ACC_ADD: {
      gl::Acc x;
      gl::acc_zero(x);
      for (int j = 0; j < m; j++) {
        const uint64_t u = a[i * m + j], v = b[i * m + j];
        gl::acc_mad(x, u, v);
        if (op == OP_ACC_ADD) {
          gl::acc_add(x, u);
          gl::acc_add(x, v);
        }
      }
      out[i] = gl::acc_reduce(x);
      break;
    }
    case OP_CACC_REDUCE:
    case OP_CACC_REDUCE_WEAK:
    case OP_CACC_REDUCE_TERMS: {
      gl::CAcc x;
      gl::cacc_zero(x);
      for (int j = 0; j < m; j++) gl::cacc_mad(x, a[i * m + j], b[i * m + j]);
      out[i] = op == OP_CACC_REDUCE        ? gl::cacc_reduce(x)
               : op == OP_CACC_REDUCE_WEAK ? gl::cacc_reduce_weak(x)
                                           : gl::cacc_reduce_terms(x);
      break;
    }
#if defined(GL_PROBE_DEVICE)
    case OP_S_MUL3:
      lfk::s_store<3>(out + 3 * i, lfk::s_mul(lfk::s_load<3>(a + 3 * i), lfk::s_load<3>(b + 3 * i)));
      break;
    case OP_S_MUL_W3:
      lfk::s_store<3>(out + 3 * i, lfk::s_canon(lfk::s_mul_w(lfk::s_load<3>(a + 3 * i), lfk::s_load<3>(b + 3 * i))));
      break;
    case OP_S_MAD2_3:
      lfk::s_store<3>(out + 3 * i, lfk::s_mad2(lfk::s_load<3>(a + 6 * i), lfk::s_load<3>(b + 6 * i),
                                               lfk::s_load<3>(a + 6 * i + 3), lfk::s_load<3>(b + 6 * i + 3)));
      break;
    case OP_SACC3: {
      lfk::SAcc<3> x;
      lfk::sacc_zero(x);
      for (int j = 0; j < m; j++)
        lfk::sacc_mad(x, lfk::s_load<3>(a + 3 * (i * m + j)), lfk::s_load<3>(b + 3 * (i * m + j)));
      lfk::s_store<3>(out + 3 * i, lfk::sacc_final(x));
      break;
    }
    case OP_FQ3ACC: {
      ring::Fq3Acc x;
      ring::fq3acc_zero(x);
      for (int j = 0; j < m; j++) {
        const uint64_t *u = a + 3 * (i * m + j), *v = b + 3 * (i * m + j);
        ring::fq3acc_mad(x, u[0], u[1], u[2], v[0], v[1], v[2]);
      }
      ring::fq3acc_final(x, out + 3 * i);
      break;
    }
#endif
    default: break;
  }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// host side of the constant shifts: s -> the instantiation shift_const<OP, s>
template <int OP, int BASE, int... I>
inline uint64_t shift_host(uint64_t x, int s, std::integer_sequence<int, I...>) {
  using F = uint64_t (*)(uint64_t);
  static const F tab[] = {&shift_const<OP, BASE + I>...};
  return tab[s - BASE](x);
}
inline uint64_t shift_host(int op, uint64_t x, int s) {
  switch (op) {
    case OP_MUL_POW2: return shift_host<OP_MUL_POW2, 0>(x, s, std::make_integer_sequence<int, 192>());
    case OP_SHL96: return shift_host<OP_SHL96, 0>(x, s, std::make_integer_sequence<int, 96>());
    case OP_SHL192: return shift_host<OP_SHL192, 0>(x, s, std::make_integer_sequence<int, 192>());
    default: return shift_host<OP_SHL_SMALL_WEAK, 1>(x, s, std::make_integer_sequence<int, 31>());
  }
}
#endif

}  // namespace glp
