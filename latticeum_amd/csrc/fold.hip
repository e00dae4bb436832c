// fold.hip -- the linear folds of a step: the commitments' (y_0 of both sides and
// cm_0), the witnesses' in NTT form, the Phi_72 witnesses' in coefficient form from the
// decomposition's digit masks (decompose_phi72.hip) with the expansion of those masks,
// and rot_lin_combination (v_0 of the folded LCCCS). One translation unit on purpose:
// compiled apart, the Phi_72 kernels here are scheduled differently.
#include "digitpack.hpp"
#include "digits.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "ring.hpp"

namespace lfk {

// ============================================================ commit_witnesses y_0
// LF/nifs/decomposition.rs:183-200: y_0 = cm - sum_{k>=1} b^k y_k (scalar b)
__global__ void k_commit_y0(const uint64_t *cm, uint64_t *y, size_t n, int lbs, int K) {
  size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (c >= n) return;
  uint64_t acc = 0;
  for (int k = K - 1; k >= 1; k--) acc = gl::mul_pow2(gl::add(acc, y[(size_t)k * n + c]), lbs);
  y[c] = gl::sub(cm[c], acc);
}

hipError_t commit_y0(const uint64_t *cm, uint64_t *y, size_t kappa, int d, int lbs, int K,
                     hipStream_t st) {
  size_t n = kappa * (size_t)d;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_commit_y0, dim3(blocks(n, 256)), dim3(256), 0, st, cm, y, n, lbs, K);
  return hipGetLastError();
}

// the other way round: cm = sum_{k>=0} b^k y_k from all K planes' commitments (lf_dev_commit_planes)
__global__ void k_cm_from_y(const uint64_t *y, size_t n, int lbs, int K, uint64_t *cm) {
  size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (c >= n) return;
  uint64_t acc = 0;
  for (int k = K - 1; k >= 1; k--) acc = gl::mul_pow2(gl::add(acc, y[(size_t)k * n + c]), lbs);
  cm[c] = gl::add(y[c], acc);
}

hipError_t cm_from_y(const uint64_t *y, size_t kappa, int d, int lbs, int K, uint64_t *cm, hipStream_t st) {
  size_t n = kappa * (size_t)d;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cm_from_y, dim3(blocks(n, 256)), dim3(256), 0, st, y, n, lbs, K, cm);
  return hipGetLastError();
}

// both sides' y_0 and the folded commitment in one pass (see kernels.hpp y0_cm0)
// one thread per commitment slot; K <= Y0_KMAX: every plane's y and rho of a side
// are loaded before the Horner chain, so the 2 (K - 1) loads of a thread are in
// flight together instead of one latency per plane (W = 464: 18.6 us per launch
// with the loads inside the chain)
constexpr int Y0_KMAX = 16;
// CM1: side 1's y_0 is the input (the step contracted the side's plane-0 operand
// row, api_step.hip) and its commitment the output, cm1 = y_1[0] + sum_{k>=1}
// 2^(k lbs) y_1[k]: the same loads and the same Horner chain, one sum the other way
template <bool CM1>
__global__ void k_y0_cm0(const uint64_t *cm0s, uint64_t *cm1s, uint64_t *y0, uint64_t *y1,
                         const uint64_t *rho, size_t n, int d, int lbs, int K, uint64_t *cm0) {
  const size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (c >= n) return;
  const int s = c % d;
  gl::CAcc a;
  gl::cacc_zero(a);
#pragma unroll
  for (int side = 0; side < 2; side++) {
    uint64_t *y = side ? y1 : y0;
    const uint64_t *rs = rho + (size_t)side * K * d + s;
    uint64_t yv[Y0_KMAX], rv[Y0_KMAX];
#pragma unroll
    for (int k = 1; k < Y0_KMAX; k++)
      if (k < K) {
        yv[k] = y[(size_t)k * n + c];
        rv[k] = rs[(size_t)k * d];
      }
    uint64_t acc = 0;
#pragma unroll
    for (int k = Y0_KMAX - 1; k >= 1; k--)
      if (k < K) {
        gl::cacc_mad(a, rv[k], yv[k]);
        acc = gl::mul_pow2(gl::add(acc, yv[k]), lbs);
      }
    uint64_t v0;
    if (CM1 && side) {
      v0 = y[c];
      cm1s[c] = gl::add(v0, acc);
    } else {
      v0 = gl::sub((side ? cm1s : cm0s)[c], acc);
      y[c] = v0;
    }
    gl::cacc_mad(a, rs[0], v0);
  }
  cm0[c] = gl::cacc_reduce(a);
}

// Phi_72: 16 slots x 16 k-lanes per block. Lane q of slot u takes the planes
// k = q, q + 16, ... (k >= 1) of both sides: y_k 2^(k lbs) (the Horner sum of
// y_0, unrolled) and rho_k (.) y_k (the Fq3 slot product of the fold); the
// lanes' sums meet in LDS, and lane 0 forms y_0 = cm - sum and adds rho_0 (.) y_0
__global__ void __launch_bounds__(256) k_y0_cm0_phi72(const uint64_t *cm0s, const uint64_t *cm1s, uint64_t *y0,
                                                     uint64_t *y1, const uint64_t *rho, size_t nslots, int lbs,
                                                     int K, uint64_t *cm0) {
  __shared__ uint64_t part[16][16][9];
  const int q = threadIdx.x & 15, ul = threadIdx.x >> 4;
  const size_t u = blockIdx.x * (size_t)16 + ul;
  const bool ok = u < nslots;
  const size_t n = nslots * 3;
  const int s = u % 8;
  ring::Fq3Acc a;
  ring::fq3acc_zero(a);
  uint64_t hs[2][3] = {{0, 0, 0}, {0, 0, 0}};
  if (ok)
    for (int side = 0; side < 2; side++) {
      const uint64_t *y = side ? y1 : y0;
      for (int k = q > 0 ? q : 16; k < K; k += 16) {
        const uint64_t *v = y + (size_t)k * n + 3 * u, *r = rho + ((size_t)side * K + k) * 24 + 3 * s;
        ring::fq3acc_mad(a, r[0], r[1], r[2], v[0], v[1], v[2]);
        const int e = (int)(((long long)k * lbs) % 192);
#pragma unroll
        for (int c = 0; c < 3; c++) hs[side][c] = gl::add(hs[side][c], gl::mul_pow2(v[c], e));
      }
    }
  uint64_t cc[3];
  ring::fq3acc_final(a, cc);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    part[ul][q][c] = cc[c];
    part[ul][q][3 + c] = hs[0][c];
    part[ul][q][6 + c] = hs[1][c];
  }
  __syncthreads();
  if (q != 0 || !ok) return;
  uint64_t t[9];
#pragma unroll
  for (int c = 0; c < 9; c++) t[c] = part[ul][0][c];
  for (int l = 1; l < 16; l++)
#pragma unroll
    for (int c = 0; c < 9; c++) t[c] = gl::add(t[c], part[ul][l][c]);
  ring::Fq3Acc a0;
  ring::fq3acc_zero(a0);
  for (int side = 0; side < 2; side++) {
    uint64_t *y = side ? y1 : y0;
    const uint64_t *cm = (side ? cm1s : cm0s) + 3 * u, *r = rho + (size_t)side * K * 24 + 3 * s;
    uint64_t v0[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      v0[c] = gl::sub(cm[c], t[3 + 3 * side + c]);
      y[3 * u + c] = v0[c];
    }
    ring::fq3acc_mad(a0, r[0], r[1], r[2], v0[0], v0[1], v0[2]);
  }
  ring::fq3acc_final(a0, cc);
#pragma unroll
  for (int c = 0; c < 3; c++) cm0[3 * u + c] = gl::add(cc[c], t[c]);
}

hipError_t y0_cm0(const uint64_t *cm0s, uint64_t *cm1s, uint64_t *y0, uint64_t *y1, const uint64_t *rho,
                  size_t kappa, int d, int lbs, int K, uint64_t *cm0, hipStream_t st, bool cm1_out) {
  const size_t n = kappa * (size_t)d;
  if (n == 0) return hipSuccess;
  if (K < 1 || K > Y0_KMAX || (cm1_out && d == 24)) return hipErrorInvalidValue;
  if (cm1_out) {
    hipLaunchKernelGGL(k_y0_cm0<true>, dim3(blocks(n, 256)), dim3(256), 0, st, cm0s, cm1s, y0, y1, rho, n, d, lbs, K,
                       cm0);
    return hipGetLastError();
  }
  if (d == 24) {
    hipLaunchKernelGGL(k_y0_cm0_phi72, dim3(blocks(kappa * 8, 16)), dim3(256), 0, st, cm0s, cm1s, y0, y1, rho,
                       kappa * 8, lbs, K, cm0);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_y0_cm0<false>, dim3(blocks(n, 256)), dim3(256), 0, st, cm0s, cm1s, y0, y1, rho, n, d, lbs, K,
                     cm0);
  return hipGetLastError();
}

// ============================================================ linear fold
// LF/nifs/folding.rs:258-268 (f_0) and folding/utils.rs:470-476 (cm_0):
//   out[j] = sum_i rho_i (.) x_i[j]
// two adjacent slots per thread (16-B streaming loads; d is even)
// run_if: when given, nothing to do unless *run_if != 0 (the fallback of the
// coefficient-form fold, fold_coeff.hip; its launch is then grid-capped and strides)
__global__ void __launch_bounds__(256) k_fold_nega(const uint64_t *rho, VecPtrs x, int nwit, size_t n,
                                                  int d, uint64_t *out, const int *run_if) {
  if (run_if && !*run_if) return;
  for (size_t c = 2 * (blockIdx.x * (size_t)blockDim.x + threadIdx.x); c < n * (size_t)d;
       c += 2 * (size_t)gridDim.x * blockDim.x) {
  const int s = c % d;
  gl::CAcc a0, a1;
  gl::cacc_zero(a0);
  gl::cacc_zero(a1);
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  // witnesses in batches of FB: the batch's loads are all in flight before its MACs
  constexpr int FB = 6;
  int i = 0;
  for (; i + FB <= nwit; i += FB) {
    u64x2 v[FB];
#pragma unroll
    for (int q = 0; q < FB; q++) v[q] = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(x.p[i + q] + c));
#pragma unroll
    for (int q = 0; q < FB; q++) {
      const ulonglong2 r = *reinterpret_cast<const ulonglong2 *>(rho + (i + q) * d + s);
      gl::cacc_mad(a0, r.x, v[q].x);
      gl::cacc_mad(a1, r.y, v[q].y);
    }
  }
  for (; i < nwit; i++) {
    const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(x.p[i] + c));
    const ulonglong2 r = *reinterpret_cast<const ulonglong2 *>(rho + i * d + s);
    gl::cacc_mad(a0, r.x, v.x);
    gl::cacc_mad(a1, r.y, v.y);
  }
  *reinterpret_cast<ulonglong2 *>(out + c) = make_ulonglong2(gl::cacc_reduce(a0), gl::cacc_reduce(a1));
  }
}
__global__ void __launch_bounds__(256) k_fold_phi72(const uint64_t *rho, VecPtrs x, int nwit, size_t n,
                                                   uint64_t *out, const int *run_if) {
  if (run_if && !*run_if) return;  // uniform: the coefficient-form fold produced f_0
  for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < n * 8; u += (size_t)gridDim.x * blockDim.x) {
  const int s = u % 8;  // Fq3 slot index u
  ring::Fq3Acc a;
  ring::fq3acc_zero(a);
  for (int i = 0; i < nwit; i++) {
    const uint64_t *r = rho + i * 24 + 3 * s, *p = x.p[i] + 3 * u;
    ring::fq3acc_mad(a, r[0], r[1], r[2], p[0], p[1], p[2]);
  }
  uint64_t c[3];
  ring::fq3acc_final(a, c);
  out[3 * u] = c[0];
  out[3 * u + 1] = c[1];
  out[3 * u + 2] = c[2];
  }
}

hipError_t fold(const uint64_t *rho, const VecPtrs &x, int nwit, size_t n, int d, uint64_t *out,
                hipStream_t st, const int *run_if) {
  if (n == 0) return hipSuccess;
  if (nwit <= 0 || nwit > LF_MAX_VECS) return hipErrorInvalidValue;
  if (d == 24) {
    unsigned nb = blocks(n * 8, 256);
    if (run_if && nb > 1024) nb = 1024;  // usually returns at once: do not launch a block per 256 slots
    hipLaunchKernelGGL(k_fold_phi72, dim3(nb), dim3(256), 0, st, rho, x, nwit, n, out, run_if);
  } else {
    unsigned nb = blocks(n * d / 2, 256);
    if (run_if && nb > 8192) nb = 8192;  // usually returns at once: do not launch a block per 512 slots
    hipLaunchKernelGGL(k_fold_nega, dim3(nb), dim3(256), 0, st, rho, x, nwit, n, d, out, run_if);
  }
  return hipGetLastError();
}

// ============================================================ rot_lin_combination
// v_0 of the folded LCCCS (CR/rotation.rs:84-101, rot_sum :45-63):
//   v0[j][c] = sum_i sum_r theta_i[r][c] coeff_j(X^r rho_i)
// theta_i flattened to d base-ring values of comp components (Fq3 for Phi_72).
// coeff_j(X^r a) in closed form: X^d + 1: a_(j-r), or -a_(d+j-r) when r > j;
// Phi_72: the terms a_k X^m, m = k + r < 48, folded back with X^24 = X^12 - 1
// (m in [24, 36): +X^(m-12) - X^(m-24)) and X^36 = -1 (m >= 36: -X^(m-36)).
__device__ __forceinline__ uint64_t rot_coeff(const uint64_t *a, int d, int j, int r) {
  if (d != 24) return j >= r ? a[j - r] : gl::sub(0, a[d + j - r]);
  uint64_t v = j >= r ? a[j - r] : 0;
  if (j >= 12 && r > j - 12) v = gl::add(v, a[j + 12 - r]);
  if (j < 12 && r > j) v = gl::sub(v, a[j + 24 - r]);
  if (j < 12 && r > j + 12) v = gl::sub(v, a[j + 36 - r]);
  return v;
}
// one block per output value (j, c); threads stride over (i, r)
__global__ void __launch_bounds__(256) k_rot_lin(const uint64_t *rho_coeff, const uint64_t *theta, int n, int d,
                                                int comp, uint64_t *v0) {
  __shared__ uint64_t red[256];
  const int j = blockIdx.x / comp, c = blockIdx.x % comp;
  gl::CAcc a;
  gl::cacc_zero(a);
  for (int t = threadIdx.x; t < n * d; t += blockDim.x) {
    const int i = t / d, r = t - i * d;
    gl::cacc_mad(a, gl::canon(theta[((size_t)i * d + r) * comp + c]), rot_coeff(rho_coeff + (size_t)i * d, d, j, r));
  }
  red[threadIdx.x] = gl::cacc_reduce(a);
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = gl::add(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) v0[(size_t)j * comp + c] = red[0];
}

hipError_t rot_lin(const uint64_t *rho_coeff, const uint64_t *theta, int n, int d, uint64_t *v0, hipStream_t st) {
  if (n < 1 || (d != 24 && (d < 2 || (d & (d - 1))))) return hipErrorInvalidValue;
  const int comp = d == 24 ? 3 : 1;
  hipLaunchKernelGGL(k_rot_lin, dim3((unsigned)(d * comp)), dim3(256), 0, st, rho_coeff, theta, n, d, comp, v0);
  return hipGetLastError();
}

// ============================================================ Phi_72 fold in coefficient form
// The 2K folded witnesses are digit planes, f_i = CRT(D_i) with D_i in {-1, 0, 1}^24,
// and get_rhos' challenges are short (coefficients in [-32, 31],
// rings/goldilocks.rs:41-67). CRT is a ring isomorphism, so f_0 = CRT(f0_coeff)
// with f0_coeff = sum_i rho_i * D_i, the product in Z[X]/(X^24 - X^12 + 1) of
// small integers. Before the reduction every coefficient of the degree-46 sum is
// at most 2K 24 32 = 23 040 in magnitude, so it runs on packed 16-bit lanes
// (v_pk_mad_i16: two coefficients per instruction). It replaces reading the 2K
// NTT-form planes (30 x 192 B per element) with 30 x 8 B of digit masks, and
// Witness::from_f's ICRT with a CRT.
constexpr int RHO24_BOUND = 32;
constexpr int RHO24_WORDS = 25;  // per witness: 12 pairs (rho_2b, rho_2b+1), 13 pairs (rho_2b-1, rho_2b)
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); }
__global__ void k_rho_phi72(const uint64_t *rho, int nw, uint32_t *rc, int *bad) {
  const int i = threadIdx.x;  // one block of >= nw threads: it also clears / sets the flag
  bool out = false;
  if (i < nw) {
  uint64_t c[24];
#pragma unroll
  for (int t = 0; t < 24; t++) c[t] = rho[(size_t)i * 24 + t];
  ring::phi72_icrt(c);
  int v[26];
  v[0] = v[25] = 0;  // rho_-1, rho_24
#pragma unroll
  for (int t = 0; t < 24; t++) {
    const int64_t x = signed_rep(c[t]);
    out |= x > RHO24_BOUND || x < -RHO24_BOUND;
    v[t + 1] = (int)(x > RHO24_BOUND ? 0 : x < -RHO24_BOUND ? 0 : x);
  }
#pragma unroll
  for (int b = 0; b < 12; b++) rc[i * RHO24_WORDS + b] = pack16(v[2 * b + 1], v[2 * b + 2]);
#pragma unroll
  for (int b = 0; b < 13; b++) rc[i * RHO24_WORDS + 12 + b] = pack16(v[2 * b], v[2 * b + 1]);
  }
  out = __syncthreads_or(out);
  if (i == 0) *bad = out ? 1 : 0;
}

hipError_t fold_phi72_rho(const uint64_t *rho, int nw, uint32_t *rc, int *bad, hipStream_t st) {
  if (nw < 1 || nw > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rho_phi72, dim3(1), dim3(64), 0, st, rho, nw, rc, bad);
  return hipGetLastError();
}

// one thread per element (blocks of whole groups, G = blockDim / L); the f0
// elements meet in LDS for w_ccs0 = sum_l B^l f0[gL + l], as in k_from_f_phi72.
// acc2[q] holds coefficients (2q, 2q + 1) of the degree-46 sum: digit j = 2a
// adds dg (rho_2b, rho_2b+1) to acc2[a + b], digit j = 2a + 1 adds
// dg (rho_2b-1, rho_2b) to acc2[a + b]
__global__ void __launch_bounds__(256) k_fold_coeff_phi72(const uint2 *masks0, const uint2 *masks1,
                                                          const uint32_t *rc, const int *bad, size_t N, int K, int L,
                                                          int lb, uint64_t *f0_coeff, uint64_t *f0,
                                                          uint64_t *w_ccs0) {
  if (*bad) return;  // uniform: a challenge is not short, the NTT-form fold runs instead
  extern __shared__ uint64_t lds[];  // [G L][24] f0 elements, then the 2K x 25 packed rho words
  // PW_SPLIT lanes per element (consecutive, one quad): lane h takes witnesses
  // h, h + PW_SPLIT, ..; their partial sums meet by two xor-shuffles
  constexpr int PW_SPLIT = 4;
  const int G = blockDim.x / (PW_SPLIT * L), t = threadIdx.x, nw = 2 * K, h = t & (PW_SPLIT - 1);
  uint32_t *rl = reinterpret_cast<uint32_t *>(lds + (size_t)G * L * 24);
  for (int q = t; q < nw * RHO24_WORDS; q += blockDim.x) rl[q] = rc[q];
  __syncthreads();
  const size_t W = N / L, j0 = (size_t)blockIdx.x * G;
  const int el = t / PW_SPLIT;  // element within the block
  const size_t e = j0 * L + el;
  const bool live = el < G * L && e < N;
  {
    s16x2 acc2[24];
#pragma unroll
    for (int q = 0; q < 24; q++) acc2[q] = (s16x2){0, 0};
    // the next witness's masks load while this one's products run
    auto mask_of = [&](int i) {
      return live ? (i < K ? masks0 : masks1)[mask24_index(i < K ? i : i - K, N, e)] : make_uint2(0u, 0u);
    };
    uint2 mn = mask_of(h);
    for (int i = h; i < nw; i += PW_SPLIT) {
      const uint2 m = mn;
      if (i + PW_SPLIT < nw) mn = mask_of(i + PW_SPLIT);
      s16x2 r[RHO24_WORDS];
#pragma unroll
      for (int u = 0; u < RHO24_WORDS; u++) r[u] = __builtin_bit_cast(s16x2, rl[i * RHO24_WORDS + u]);
#pragma unroll
      for (int jj = 0; jj < 24; jj++) {
        const short dv = (short)mask24_digit(m.x, m.y, jj);
        const s16x2 dg = {dv, dv};
        const int a = jj >> 1;
        if ((jj & 1) == 0) {
#pragma unroll
          for (int b2 = 0; b2 < 12; b2++) acc2[a + b2] += dg * r[b2];
        } else {
#pragma unroll
          for (int b2 = 0; b2 < 13; b2++)
            if (a + b2 < 24) acc2[a + b2] += dg * r[12 + b2];
        }
      }
    }
    // sum over the quad (exact in 16 bits: the total is the one bounded above)
#pragma unroll
    for (int q = 0; q < 24; q++) {
      uint32_t v = __builtin_bit_cast(uint32_t, acc2[q]);
      v = __builtin_bit_cast(uint32_t, acc2[q] + __builtin_bit_cast(s16x2, (uint32_t)__shfl_xor((int)v, 1)));
      acc2[q] = __builtin_bit_cast(s16x2, v) + __builtin_bit_cast(s16x2, (uint32_t)__shfl_xor((int)v, 2));
    }
    if (live && h == 0) {
    int32_t acc[48];
#pragma unroll
    for (int q = 0; q < 24; q++) {
      acc[2 * q] = acc2[q].x;
      acc[2 * q + 1] = acc2[q].y;
    }
    // X^24 = X^12 - 1:  X^s = X^(s-12) - X^(s-24) for 24 <= s < 36, X^s = -X^(s-36) for s >= 36
#pragma unroll
    for (int s2 = 46; s2 >= 36; s2--) acc[s2 - 36] -= acc[s2];
#pragma unroll
    for (int s2 = 35; s2 >= 24; s2--) {
      acc[s2 - 12] += acc[s2];
      acc[s2 - 24] -= acc[s2];
    }
    uint64_t c[24];
#pragma unroll
    for (int u = 0; u < 24; u++) c[u] = from_signed(acc[u]);
    ring::st24(f0_coeff + e * 24, c);
    ring::phi72_crt(c);
    ring::st24(f0 + e * 24, c);
#pragma unroll
    for (int u = 0; u < 24; u++) lds[el * 24 + u] = c[u];
    }
  }
  __syncthreads();
  const size_t ng = W - j0 < (size_t)G ? W - j0 : (size_t)G;
  for (int o = t; o < (int)ng * 24; o += blockDim.x) {
    const int g = o / 24, i = o - g * 24;
    const uint64_t *row = lds + g * L * 24 + i;
    uint64_t acc = row[(L - 1) * 24];
    for (int l = L - 2; l >= 0; l--) acc = gl::add(gl::mul_pow2(acc, lb), row[l * 24]);
    w_ccs0[j0 * 24 + o] = acc;
  }
}

hipError_t fold_phi72_coeff(const uint2 *masks0, const uint2 *masks1, const uint32_t *rc, const int *bad, size_t N,
                            int K, int L, int lb, uint64_t *f0_coeff, uint64_t *f0, uint64_t *w_ccs0, hipStream_t st) {
  const size_t W = N / L;
  if (W == 0) return hipSuccess;
  if (L < 1 || L > 64 || K < 1 || 2 * K > 64) return hipErrorInvalidValue;
  const int G = 256 / (4 * L);  // 4 lanes per element (k_fold_coeff_phi72's PW_SPLIT)
  if (G < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)G * L * 24 * 8 + (size_t)2 * K * RHO24_WORDS * 4;
  hipLaunchKernelGGL(k_fold_coeff_phi72, dim3(blocks(W, G)), dim3(4 * G * L), lds, st, masks0, masks1, rc, bad, N, K,
                     L, lb, f0_coeff, f0, w_ccs0);
  return hipGetLastError();
}

// f_0 from the digit masks for any rho (the fallback of k_fold_coeff_phi72 when
// the planes are kept packed, lf_fold_step_bufs.fk == NULL): the same ring
// product in coefficient form, f0_coeff = sum_i ICRT(rho_i) * D_i mod p, one
// thread per element, then f_0 = CRT(f0_coeff). Every block takes the 2K
// inverse transforms of rho (and their negatives) into LDS itself.
__global__ void __launch_bounds__(256) k_fold_phi72_masks(const uint2 *masks0, const uint2 *masks1, const uint64_t *rho,
                                                          int K, size_t N, uint64_t *f0, const int *run_if) {
  if (run_if && !*run_if) return;  // uniform: the short-challenge fold produced f_0
  __shared__ uint64_t rc[2][64 * 24];  // [sign][witness][coefficient]
  const int nw = 2 * K;
  for (int i = threadIdx.x; i < nw; i += blockDim.x) {
    uint64_t c[24];
#pragma unroll
    for (int t = 0; t < 24; t++) c[t] = rho[(size_t)i * 24 + t];
    ring::phi72_icrt(c);
#pragma unroll
    for (int t = 0; t < 24; t++) {
      rc[0][i * 24 + t] = c[t];
      rc[1][i * 24 + t] = gl::sub(0, c[t]);
    }
  }
  __syncthreads();
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < N; e += (size_t)gridDim.x * blockDim.x) {
    uint64_t acc[47];
#pragma unroll
    for (int t = 0; t < 47; t++) acc[t] = 0;
    for (int i = 0; i < nw; i++) {
      const uint2 m = (i < K ? masks0 : masks1)[mask24_index(i < K ? i : i - K, N, e)];
#pragma unroll
      for (int j = 0; j < 24; j++) {
        if (!(m.x >> j & 1)) continue;
        const uint64_t *r = rc[m.y >> j & 1] + i * 24;
#pragma unroll
        for (int t = 0; t < 24; t++) acc[j + t] = gl::add(acc[j + t], r[t]);
      }
    }
    // X^24 = X^12 - 1 (as in k_fold_coeff_phi72)
#pragma unroll
    for (int s2 = 46; s2 >= 36; s2--) acc[s2 - 36] = gl::sub(acc[s2 - 36], acc[s2]);
#pragma unroll
    for (int s2 = 35; s2 >= 24; s2--) {
      acc[s2 - 12] = gl::add(acc[s2 - 12], acc[s2]);
      acc[s2 - 24] = gl::sub(acc[s2 - 24], acc[s2]);
    }
    ring::phi72_crt(acc);
    ring::st24(f0 + e * 24, acc);
  }
}

hipError_t fold_phi72_masks(const uint2 *masks0, const uint2 *masks1, const uint64_t *rho, int K, size_t N,
                            uint64_t *f0, const int *run_if, hipStream_t st) {
  if (N == 0) return hipSuccess;
  if (K < 1 || 2 * K > 64) return hipErrorInvalidValue;
  unsigned nb = blocks(N, 256);
  if (run_if && nb > 1024) nb = 1024;  // usually returns at once
  hipLaunchKernelGGL(k_fold_phi72_masks, dim3(nb), dim3(256), 0, st, masks0, masks1, rho, K, N, f0, run_if);
  return hipGetLastError();
}

// packed Phi_72 digit planes (digitpack.hpp, the d = 24 masks) -> the u64
// witness forms f_coeff (the digits mod p) and f = CRT(f_coeff); either may be null
__global__ void __launch_bounds__(256) k_expand_phi72(const uint2 *planes, size_t n, uint64_t *fc, uint64_t *f) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const uint2 m = planes[e];
    uint64_t c[24];
#pragma unroll
    for (int i = 0; i < 24; i++) c[i] = pw_digit(m.x, m.y, i);
    if (fc) ring::st24(fc + e * 24, c);
    if (f) {
      ring::phi72_crt(c);
      ring::st24(f + e * 24, c);
    }
  }
}

hipError_t expand_phi72(const uint2 *planes, size_t n, uint64_t *fc, uint64_t *f, hipStream_t st) {
  if (n == 0 || (!fc && !f)) return hipSuccess;
  hipLaunchKernelGGL(k_expand_phi72, dim3(grid_cap(blocks(n, 256))), dim3(256), 0, st, planes, n, fc, f);
  return hipGetLastError();
}

}  // namespace lfk
