// gl_probe.hip -- lf_dev_gl_probe: the device compile of the field arithmetic, one
// primitive per launch, elementwise over directed inputs (a test aid, gl_probe.hpp).
#define GL_PROBE_DEVICE 1
#include "gl_probe.hpp"

#include "api_internal.hpp"

namespace {

constexpr int BLOCK = 64;

template <int OP, int S>
__global__ void k_probe_shift(const uint64_t *a, uint64_t *out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK)
    out[i] = glp::shift_const<OP, S>(a[i]);
}
__global__ void k_probe_elem(int op, const uint64_t *a, const uint64_t *b, int s, int m, uint64_t *out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK)
    glp::elem(op, a, b, s, m, i, out);
}

using ShiftKernel = void (*)(const uint64_t *, uint64_t *, size_t);
template <int OP, int BASE, int... I>
ShiftKernel shift_kernel(int s, std::integer_sequence<int, I...>) {
  static const ShiftKernel tab[] = {&k_probe_shift<OP, BASE + I>...};
  return tab[s - BASE];
}
ShiftKernel shift_kernel(int op, int s) {
  switch (op) {
    case glp::OP_MUL_POW2: return shift_kernel<glp::OP_MUL_POW2, 0>(s, std::make_integer_sequence<int, 192>());
    case glp::OP_SHL96: return shift_kernel<glp::OP_SHL96, 0>(s, std::make_integer_sequence<int, 96>());
    case glp::OP_SHL192: return shift_kernel<glp::OP_SHL192, 0>(s, std::make_integer_sequence<int, 192>());
    default: return shift_kernel<glp::OP_SHL_SMALL_WEAK, 1>(s, std::make_integer_sequence<int, 31>());
  }
}

}  // namespace

int lf_dev_gl_probe(lf_ctx *c, int op, const uint64_t *a, const uint64_t *b, int s, int m, uint64_t *out, size_t n) {
  if (!c) return LF_ERR_INVALID_ARG;
  if (op < 0 || op >= glp::OP_COUNT) return fail(c, LF_ERR_INVALID_ARG, "gl_probe: unknown op");
  int slo, shi;
  glp::shift_range(op, slo, shi);
  if (s < slo || s >= shi) return fail(c, LF_ERR_INVALID_ARG, "gl_probe: shift out of the op's range");
  if (!glp::m_ok(op, m)) return fail(c, LF_ERR_INVALID_ARG, "gl_probe: m out of the op's range");
  if (n && (!a || !out || (glp::takes_b(op) && !b))) return fail(c, LF_ERR_INVALID_ARG, "gl_probe: null operand");
  if (!n) return LF_OK;
  DevGuard g(c);
  const size_t blocks = (n + BLOCK - 1) / BLOCK;
  const unsigned grid = (unsigned)(blocks < 65535 ? blocks : 65535);
  if (glp::is_const_shift(op))
    hipLaunchKernelGGL(shift_kernel(op, s), dim3(grid), dim3(BLOCK), 0, c->cur, a, out, n);
  else
    hipLaunchKernelGGL(k_probe_elem, dim3(grid), dim3(BLOCK), 0, c->cur, op, a, b, s, m, out, n);
  LF_HIP(c, hipGetLastError());
  return LF_OK;
}
