// witness_pack.hip -- Witness::from_f_coeff (LF/arith.rs:324-338: f = CRT(f_coeff),
// w_ccs = gadget_recompose(f, B, L)) at every ring, and the packed witness (lf.h,
// "witness wire format"): pack, the width probe's range count, and the decode that
// unpack runs inside the from_f_coeff kernels. Each from_f_coeff kernel takes its
// coefficients through a source (wsrc.hpp): canonical u64 words, or the payload's
// i16 / i32 / u64 words, decoded in registers; with fc_out it also writes f_coeff in
// canonical form, so unpack reads the payload once and no u64 f_coeff is read back.
//   d = 1024: kernels_n32.hip's k_from_fcoeff_n32 and its split form for plain u64 words,
//             k_from_fcoeff_src_n32 here for a payload;
//   d = 4096: k_from_fcoeff_n4k here, on the quarter transforms of kernels_n4k.hip;
//   d = 16 .. 512 and 2048: k_from_fcoeff_nega on ring::stockham4, one workgroup per group;
//   d = 24: k_from_fcoeff_phi72 on ring::phi72_crt, one thread per element.
#include "digits.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "ntt32.hpp"
#include "ring.hpp"
#include "wsrc.hpp"

namespace lfk {

using ring::NT;

// ============================================================ X^d + 1 on the LDS transform
// The mirror of k_from_f_nega (transform.hip): per limb, from the top one, twist ->
// forward Stockham -> f, with w_ccs's Horner step on the slots in registers.
template <int D, class S>
__global__ void __launch_bounds__(NT<D>::T) k_from_fcoeff_nega(const typename S::word *src, size_t W, int lb, int L,
                                                              uint64_t *fc_out, uint64_t *f, uint64_t *w_ccs,
                                                              ring::NegaTables fwd, int *err, const int *skip_if) {
  constexpr int T = NT<D>::T, PER = D / T;
  __shared__ uint64_t buf[2][D];
  if (skip_if && *skip_if) return;  // uniform: the coefficient-form fold wrote no f_coeff (its fallback runs)
  const int tid = threadIdx.x;
  bool bad = false;
  for (size_t j = blockIdx.x; j < W; j += gridDim.x) {
    uint64_t acc[PER];
    for (int l = L - 1; l >= 0; l--) {
      const size_t e = j * L + l;
      const typename S::word *g = src + e * D;
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const int i = tid + q * T;
        const uint64_t c = S::get(g[i], bad);
        if (fc_out) fc_out[e * D + i] = c;
        buf[0][i] = gl::mul(c, fwd.twist[i]);
      }
      __syncthreads();
      uint64_t *r = ring::stockham4<D, T, false>(buf[0], buf[1], fwd.roots, tid);
      uint64_t *of = f + e * D;
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const uint64_t v = r[tid + q * T];
        of[tid + q * T] = v;
        acc[q] = (l == L - 1) ? v : gl::add(gl::mul_pow2(acc[q], lb), v);
      }
      __syncthreads();
    }
    uint64_t *ow = w_ccs + j * D;
#pragma unroll
    for (int q = 0; q < PER; q++) ow[tid + q * T] = acc[q];
  }
  if (bad) raise(err, 1);
}

// ============================================================ Phi_72
// 24 words of an element as 16-B vector loads: 12 (u64), 6 (i32) or 3 (i16); an element
// starts on a 16-B boundary at every width (192, 96, 48 B) when the buffer does
template <class S>
__device__ __forceinline__ void ld24_src(const typename S::word *p, uint64_t *c, bool &bad) {
  constexpr int PER = 16 / (int)sizeof(typename S::word), NV = 24 / PER;
  union V {
    uint4 q;
    typename S::word w[PER];
  };
  const uint4 *src = reinterpret_cast<const uint4 *>(p);
  V v[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) v[i].q = src[i];
#pragma unroll
  for (int i = 0; i < NV; i++)
#pragma unroll
    for (int k = 0; k < PER; k++) c[i * PER + k] = S::get(v[i].w[k], bad);
}

// The mirror of k_from_f_phi72 (transform.hip): one thread per f element (j, l), a block
// holds G = blockDim / L whole groups; f = CRT(f_coeff) goes through LDS, where the
// block's threads run the Horner recompose over the G * 24 w_ccs coefficients.
template <class S>
__global__ void __launch_bounds__(256) k_from_fcoeff_phi72(const typename S::word *src, size_t W, int lb, int L,
                                                          uint64_t *fc_out, uint64_t *f, uint64_t *w_ccs, int *err) {
  extern __shared__ uint64_t lds[];  // [G * L][24]
  const int G = blockDim.x / L, t = threadIdx.x;
  const size_t j0 = (size_t)blockIdx.x * G;
  const size_t u = j0 * L + t;
  if (t < G * L && u < W * (size_t)L) {
    uint64_t c[24];
    bool bad = false;
    ld24_src<S>(src + u * 24, c, bad);
    if (bad) raise(err, 1);
    if (fc_out) ring::st24(fc_out + u * 24, c);
    ring::phi72_crt(c);
    ring::st24(f + u * 24, c);
#pragma unroll
    for (int i = 0; i < 24; i++) lds[t * 24 + i] = c[i];
  }
  __syncthreads();
  const size_t ng = W - j0 < (size_t)G ? W - j0 : (size_t)G;
  for (int o = t; o < (int)ng * 24; o += blockDim.x) {
    const int g = o / 24, i = o - g * 24;
    const uint64_t *row = lds + g * L * 24 + i;
    uint64_t acc = row[(L - 1) * 24];
    for (int l = L - 2; l >= 0; l--) acc = gl::add(gl::mul_pow2(acc, lb), row[l * 24]);
    w_ccs[j0 * 24 + o] = acc;
  }
}

// ============================================================ d = 1024 and d = 4096 on the 32 x 32 NTT
// The new kernels live in this file, not beside their mirrors in kernels_n32.hip and
// kernels_n4k.hip: those files' kernels stay the same code whatever is added here.
namespace {
constexpr int D1K = 1024, D4 = 4096, Q4 = 1024;
constexpr int WPB = 4;   // d = 1024: waves per block, as kernels_n32.hip
constexpr int WPB4 = 8;  // d = 4096: two group pairs x four quarters, as kernels_n4k.hip

// One coefficient row of a half-wave (lane r: x[r + 32 k], k < 32) through a source: a
// rolled loop of 8 loads at a time, decoded, stored to oc (the canonical f_coeff, may
// be null) and parked in the half-wave's own transpose tile, which is idle until the
// transform; then all 32 back into registers. Unrolled, the loads of the whole row are
// hoisted above the decode and the kernel spills.
template <class S>
__device__ __forceinline__ void load_row_src(const typename S::word *row, uint64_t *oc, bool store, uint64_t *tile,
                                             int r, uint64_t *v, bool &bad) {
#pragma unroll 1
  for (int k0 = 0; k0 < 32; k0 += 8) {
    typename S::word w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = row[32 * (k0 + k)];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint64_t c = S::get(w[k], bad);
      if (store) oc[32 * (k0 + k)] = c;
      tile[(k0 + k) * 32 + r] = c;
    }
  }
#pragma unroll
  for (int k = 0; k < 32; k++) v[k] = tile[k * 32 + r];
}
// w_ccs's Horner step (B = 2^lb) over the limbs, from the top one; weakly reduced at B = 2^15
__device__ __forceinline__ void horner_step(uint64_t *acc, const uint64_t *v, bool first, int lb, uint64_t b_pow) {
  if (first) {
#pragma unroll
    for (int i = 0; i < 32; i++) acc[i] = v[i];
  } else if (lb == 15) {  // GoldiLocksDP B = 2^15: a shift instead of a product
#pragma unroll
    for (int i = 0; i < 32; i++) acc[i] = gl::add_weak(gl::shl_small_weak(acc[i], 15), v[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 32; i++) acc[i] = gl::add(gl::mul(acc[i], b_pow), v[i]);
  }
}
}  // namespace

// d = 1024: k_from_fcoeff_n32's ungated loop (one half-wave per group, slot-form Horner),
// its rows read through a source. That kernel keeps its own body and instantiation (the
// coefficient-form fold's); this one serves the packed sources.
template <class S>
__global__ void __launch_bounds__(256, 2) k_from_fcoeff_src_n32(const typename S::word *src, size_t W, int lb, int L,
                                                               uint64_t *fc_out, uint64_t *f, uint64_t *w_ccs,
                                                               const uint64_t *mid_fg, int *err) {
  __shared__ uint64_t lds_all[WPB * n32::WAVE_U64];
  __shared__ uint64_t mid_f[n32::MID_U64];
  n32::stage_mid(mid_f, mid_fg);
  __syncthreads();
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  uint64_t *tile = lds_all + wib * n32::WAVE_U64 + h * n32::HALF_U64;
  const size_t stride = (size_t)gridDim.x * WPB * 2, Wp = (W + 1) & ~(size_t)1;  // both halves iterate together
  const uint64_t b_pow = gl::mul_pow2(1, lb);
  bool bad = false;
  for (size_t g = ((size_t)blockIdx.x * WPB + wib) * 2 + h; g < Wp; g += stride) {
    const bool ok = g < W;
    const size_t gg = ok ? g : 0;
    uint64_t acc[32];
    for (int l = L - 1; l >= 0; l--) {
      const size_t e = gg * L + l;
      uint64_t v[32];
      load_row_src<S>(src + e * D1K + r, fc_out + e * D1K + r, fc_out && ok, tile, r, v, bad);
      n32::forward(v, mid_f, tile, r);  // v[i] = X[r + 32 brv5(i)]
      horner_step(acc, v, l == L - 1, lb, b_pow);
      if (ok) {
        uint64_t *of = f + e * D1K + r;
#pragma unroll
        for (int i = 0; i < 32; i++) of[32 * n32::brv5(i)] = v[i];
      }
    }
    if (ok) {
      uint64_t *ow = w_ccs + g * D1K + r;
#pragma unroll
      for (int i = 0; i < 32; i++) ow[32 * n32::brv5(i)] = gl::canon(acc[i]);
    }
  }
  if (bad) raise(err, 1);
}

// d = 4096, the mirror of k_from_f_n4k without its exchange: with j = a + 1024 b and
// m = m0 + 4 m1 (kernels_n4k.hip's header),
//   X[m0 + 4 m1] = NTT1024(y_m0)[m1],  y_m0[a] = psi^((2 m0 - 3) a) sum_b x[a + 1024 b] w8^(b (2 m0 + 1)),
// so the forward direction needs no data of another quarter: a half-wave owns one
// (group, quarter m0) as in k_decompose_n4k. Per limb it reads the four coefficients
// a + 1024 b of its 32 a = r + 32 k (the four waves of a group read the same words: one
// pass over HBM, the rest from L2), keeps z_m0 of their radix-4 butterfly (w8 = 2^120:
// shifts), twists by tw4, and runs the 1024-point transform. The wave of quarter m0
// writes quarter b = m0 of fc_out (may be null) and slots m0 + 4 m1 of f.
namespace {
__device__ __forceinline__ uint64_t dft4_fwd_one(uint64_t d0, uint64_t d1, uint64_t d2, uint64_t d3, int m0) {
  // z_m = sum_b (w8^b d_b) w4^(b m), w8 = 2^120 = -2^24, w4 = 2^48 (kernels_n4k.hip dft4_fwd)
  const uint64_t e1 = gl::neg(gl::shl96(d1, 24)), e2 = gl::shl96(d2, 48), f3 = gl::neg(gl::shl96(d3, 72));  // w8^b d_b: w8^3 = -2^72
  const uint64_t t0 = gl::add(d0, e2), t1 = gl::sub(d0, e2), t2 = gl::add(e1, f3);
  const uint64_t t3 = gl::shl96(gl::sub(e1, f3), 48);
  return m0 == 0 ? gl::add(t0, t2) : m0 == 1 ? gl::add(t1, t3) : m0 == 2 ? gl::sub(t0, t2) : gl::sub(t1, t3);
}
}  // namespace
template <class S>
__global__ void __launch_bounds__(512, 1) k_from_fcoeff_n4k(const typename S::word *src, size_t W, int lb, int L,
                                                           uint64_t *fc_out, uint64_t *f, uint64_t *w_ccs,
                                                           const uint64_t *mid_fg, const uint64_t *twf, int *err) {
  __shared__ uint64_t lds_all[WPB4 * n32::WAVE_U64];
  __shared__ uint64_t mid_f[n32::MID_U64];
  n32::stage_mid(mid_f, mid_fg);
  __syncthreads();
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5, m0 = wib & 3, G = 2 * (wib >> 2) + h;
  uint64_t *T = lds_all + wib * n32::WAVE_U64 + h * n32::HALF_U64;
  const uint64_t *tw = twf + m0 * Q4 + r;
  const uint64_t b_pow = gl::mul_pow2(1, lb);
  bool bad = false;
  for (size_t g0 = (size_t)blockIdx.x * 4; g0 < W; g0 += (size_t)gridDim.x * 4) {
    const size_t g = g0 + G;
    const bool ok = g < W;
    const size_t gg = ok ? g : 0;
    uint64_t acc[32];
    for (int l = L - 1; l >= 0; l--) {
      const size_t e = gg * L + l;
      const typename S::word *row = src + e * D4 + r;
      uint64_t *oc = fc_out + e * D4 + m0 * Q4 + r;
      const bool store = fc_out && ok;
      // y_m0 of 8 a at a time into the half-wave's own (idle) tile, as load_row_src
#pragma unroll 1
      for (int k0 = 0; k0 < 32; k0 += 8) {
        typename S::word w[8][4];
        uint64_t t8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
#pragma unroll
          for (int b = 0; b < 4; b++) w[k][b] = row[32 * (k0 + k) + b * Q4];
          t8[k] = tw[32 * (k0 + k)];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
          uint64_t dg[4];
#pragma unroll
          for (int b = 0; b < 4; b++) dg[b] = S::get(w[k][b], bad);
          if (store) oc[32 * (k0 + k)] = m0 == 0 ? dg[0] : m0 == 1 ? dg[1] : m0 == 2 ? dg[2] : dg[3];
          T[(k0 + k) * 32 + r] = gl::mul(dft4_fwd_one(dg[0], dg[1], dg[2], dg[3], m0), t8[k]);
        }
      }
      uint64_t v[32];
#pragma unroll
      for (int k = 0; k < 32; k++) v[k] = T[k * 32 + r];
      n32::forward(v, mid_f, T, r);  // v[i] = slot m0 + 4 (r + 32 brv5(i))
      if (ok) {
        uint64_t *of = f + e * D4 + m0 + 4 * r;
#pragma unroll
        for (int i = 0; i < 32; i++) of[128 * n32::brv5(i)] = v[i];
      }
      horner_step(acc, v, l == L - 1, lb, b_pow);
    }
    if (ok) {
      uint64_t *ow = w_ccs + g * D4 + m0 + 4 * r;
#pragma unroll
      for (int i = 0; i < 32; i++) ow[128 * n32::brv5(i)] = gl::canon(acc[i]);
    }
  }
  if (bad) raise(err, 1);
}

hipError_t from_fcoeff_src_n32(const void *src, int kind, size_t W, int lb, int L, uint64_t *fc_out, uint64_t *f,
                               uint64_t *w_ccs, const ring::NegaTables &fwd, int *err, hipStream_t st) {
  if (!W) return hipSuccess;
  if (!fwd.mid) return hipErrorInvalidValue;
  size_t nb = (W + 2 * WPB - 1) / (2 * WPB);
  if (nb > 4096) nb = 4096;  // the kernel loops
  return witness_src(kind, [&](auto s) {
    using S = decltype(s);
    hipLaunchKernelGGL((k_from_fcoeff_src_n32<S>), dim3((unsigned)nb), dim3(64 * WPB), 0, st,
                       static_cast<const typename S::word *>(src), W, lb, L, fc_out, f, w_ccs, fwd.mid, err);
    return hipGetLastError();
  });
}
hipError_t from_fcoeff_n4k(const void *src, int kind, size_t W, int lb, int L, uint64_t *fc_out, uint64_t *f,
                           uint64_t *w_ccs, const ring::NegaTables &fwd, int *err, hipStream_t st) {
  if (!fwd.mid || !fwd.tw4) return hipErrorInvalidValue;
  if (!W) return hipSuccess;
  size_t nb = (W + 3) / 4;  // one block per 4 groups, capped (the kernel loops)
  if (nb > 4096) nb = 4096;
  return witness_src(kind, [&](auto s) {
    using S = decltype(s);
    hipLaunchKernelGGL((k_from_fcoeff_n4k<S>), dim3((unsigned)nb), dim3(64 * WPB4), 0, st,
                       static_cast<const typename S::word *>(src), W, lb, L, fc_out, f, w_ccs, fwd.mid, fwd.tw4, err);
    return hipGetLastError();
  });
}

// the LDS-transform degrees this file's kernel is built for (1024 and 4096 have their own files)
using WitnessNegaDegrees = std::integer_sequence<int, 16, 32, 64, 128, 256, 512, 2048>;

hipError_t from_fcoeff(const void *src, int kind, size_t N, int d, int lb, int L, uint64_t *fc_out, uint64_t *f,
                       uint64_t *w_ccs, const ring::NegaTables &fwd, int *err, hipStream_t st, const int *skip_if) {
  if (L < 1) return hipErrorInvalidValue;
  const size_t W = N / L;
  if (W == 0) return hipSuccess;
  if (skip_if && (d == 1024 || d == 4096 || d == 24)) return hipErrorInvalidValue;  // the LDS-transform kernel's gate
  if (d == 1024) {
    // canonical words and nothing else to write: the coefficient-form fold's launcher, ungated
    if (kind == WSRC_U64 && !fc_out)
      return from_fcoeff_n32(const_cast<uint64_t *>(static_cast<const uint64_t *>(src)), W, lb, L, f, w_ccs, fwd,
                             nullptr, st);
    return from_fcoeff_src_n32(src, kind, W, lb, L, fc_out, f, w_ccs, fwd, err, st);
  }
  if (d == 4096) return from_fcoeff_n4k(src, kind, W, lb, L, fc_out, f, w_ccs, fwd, err, st);
  if (d == 24) {
    if (L > 256) return hipErrorInvalidValue;
    const int G = 256 / L;
    return witness_src(kind, [&](auto s) {
      using S = decltype(s);
      hipLaunchKernelGGL((k_from_fcoeff_phi72<S>), dim3(blocks(W, G)), dim3(G * L), (size_t)G * L * 24 * 8, st,
                         static_cast<const typename S::word *>(src), W, lb, L, fc_out, f, w_ccs, err);
      return hipGetLastError();
    });
  }
  return nega_degree_in(
      d,
      [&](auto dd) {
        constexpr int D = decltype(dd)::value;
        return witness_src(kind, [&](auto s) {
          using S = decltype(s);
          hipLaunchKernelGGL((k_from_fcoeff_nega<D, S>), dim3(grid_cap(W)), dim3(NT<D>::T), 0, st,
                             static_cast<const typename S::word *>(src), W, lb, L, fc_out, f, w_ccs, fwd, err, skip_if);
          return hipGetLastError();
        });
      },
      WitnessNegaDegrees{});
}

// ============================================================ pack / decode
// eight coefficients per thread (d is a multiple of 8 at every ring): 16-B stores of the
// i16 words, two of the i32 words. A coefficient outside the width raises the flag.
template <class S>
__global__ void __launch_bounds__(256) k_witness_pack(const uint64_t *fc, size_t n8, typename S::word *out, int *err) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= n8) return;
  using Wd = typename S::word;
  union {
    uint4 q[sizeof(Wd) / 2];
    Wd w[8];
  } o;
  const ulonglong2 *in = reinterpret_cast<const ulonglong2 *>(fc) + 4 * t;
  uint64_t x[8];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const ulonglong2 v = in[i];
    x[2 * i] = v.x;
    x[2 * i + 1] = v.y;
  }
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if constexpr (S::bits == 64) {
      o.w[i] = (Wd)x[i];
    } else {
      const int64_t s = signed_rep(x[i]);
      const int64_t lim = (int64_t)1 << (S::bits - 1);
      bad |= s < -lim || s >= lim;
      o.w[i] = (Wd)s;
    }
  }
  if (bad) raise(err, 1);
  uint4 *dst = reinterpret_cast<uint4 *>(out) + (sizeof(Wd) / 2) * t;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(Wd) / 2); i++) dst[i] = o.q[i];
}

// payload -> f_coeff alone (unpack without f and w_ccs)
template <class S>
__global__ void __launch_bounds__(256) k_witness_decode(const typename S::word *in, size_t n8, uint64_t *fc, int *err) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= n8) return;
  using Wd = typename S::word;
  union {
    uint4 q[sizeof(Wd) / 2];
    Wd w[8];
  } v;
  const uint4 *src = reinterpret_cast<const uint4 *>(in) + (sizeof(Wd) / 2) * t;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(Wd) / 2); i++) v.q[i] = src[i];
  bool bad = false;
  ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(fc) + 4 * t;
#pragma unroll
  for (int i = 0; i < 4; i++) dst[i] = make_ulonglong2(S::get(v.w[2 * i], bad), S::get(v.w[2 * i + 1], bad));
  if (bad) raise(err, 1);
}

hipError_t witness_pack(const uint64_t *fc, size_t n, int bits, void *out, int *err, hipStream_t st) {
  if (n % 8) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  const int kind = bits == 16 ? WSRC_I16 : bits == 32 ? WSRC_I32 : bits == 64 ? WSRC_U64 : -1;
  return witness_src(kind, [&](auto s) {
    using S = decltype(s);
    hipLaunchKernelGGL((k_witness_pack<S>), dim3(blocks(n / 8, 256)), dim3(256), 0, st, fc, n / 8,
                       static_cast<typename S::word *>(out), err);
    return hipGetLastError();
  });
}
hipError_t witness_decode(const void *in, int kind, size_t n, uint64_t *fc, int *err, hipStream_t st) {
  if (n % 8) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  return witness_src(kind, [&](auto s) {
    using S = decltype(s);
    hipLaunchKernelGGL((k_witness_decode<S>), dim3(blocks(n / 8, 256)), dim3(256), 0, st,
                       static_cast<const typename S::word *>(in), n / 8, fc, err);
    return hipGetLastError();
  });
}

// ============================================================ the width probe
// out[0] += coefficients outside [-2^15, 2^15 - 1], out[1] += those outside [-2^31, 2^31 - 1]
// (the l_inf norm alone cannot tell -2^15 from 2^15)
__global__ void __launch_bounds__(256) k_witness_range(const uint64_t *fc, size_t n, unsigned long long *out) {
  unsigned int c16 = 0, c32 = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int64_t s = signed_rep(fc[i]);
    c16 += s < -32768 || s > 32767;
    c32 += s < -2147483648ll || s > 2147483647ll;
  }
  if (c16) atomicAdd(&out[0], (unsigned long long)c16);
  if (c32) atomicAdd(&out[1], (unsigned long long)c32);
}
hipError_t witness_range(const uint64_t *fc, size_t n, uint64_t *out, hipStream_t st) {
  hipError_t e = hipMemsetAsync(out, 0, 16, st);
  if (e != hipSuccess || !n) return e;
  hipLaunchKernelGGL(k_witness_range, dim3(grid_cap(blocks(n, 256))), dim3(256), 0, st, fc, n,
                     reinterpret_cast<unsigned long long *>(out));
  return hipGetLastError();
}

}  // namespace lfk
