// transform.hip -- the ring transforms of whole vectors, the slot-wise product, the
// Montgomery edge, and the witness conversions in their generic forms (from_w_ccs,
// from_f, decompose_witness: Phi_72, and one workgroup per element on the LDS
// transform for every X^d + 1), whose launchers also dispatch to the d = 1024
// (kernels_n32.hip) and d = 4096 (kernels_n4k.hip) forms. The users of
// ring::stockham4 share this one translation unit on purpose: compiled apart, the
// transform kernels come out with different address arithmetic.
// (decompose_pow2.hip instantiates stockham4 only for its own kernel, 16 elements per block.)
// Data layout in HBM (every kernel file): AoS ring elements, d u64 each (d = 24 for
// Phi_72 in the reference's in-place CRT layout [s0.c0, s0.c1, s0.c2, s1.c0, ..]
// (stark-rings crt.rs:53-77), d = 2^k, 16 <= d <= 4096, for the negacyclic rings),
// canonical values. Every launcher returns hipError_t and takes the stream explicitly.
#include "digits.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "ring.hpp"

namespace lfk {

using ring::NT;

// ============================================================ Phi_72 transforms
// one thread per ring element; 16-B vector loads of the 192-B element
template <bool FWD>
__global__ void __launch_bounds__(256) k_phi72_transform(uint64_t *data, size_t n) {
  size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e >= n) return;
  uint64_t c[24];
  ring::ld24(data + e * 24, c);
  if (FWD)
    ring::phi72_crt(c);
  else
    ring::phi72_icrt(c);
  ring::st24(data + e * 24, c);
}

// ============================================================ negacyclic transforms
template <int D, bool FWD>
__global__ void __launch_bounds__(NT<D>::T) k_nega_transform(uint64_t *data, size_t n,
                                                            ring::NegaTables tb) {
  constexpr int T = NT<D>::T;
  __shared__ uint64_t buf[2][D];
  const int tid = threadIdx.x;
  for (size_t e = blockIdx.x; e < n; e += gridDim.x) {
    uint64_t *g = data + e * D;
#pragma unroll
    for (int i = tid; i < D; i += T) {
      uint64_t v = g[i];
      buf[0][i] = FWD ? gl::mul(v, tb.twist[i]) : v;
    }
    __syncthreads();
    uint64_t *r = ring::stockham4<D, T, !FWD>(buf[0], buf[1], tb.roots, tid);
#pragma unroll
    for (int i = tid; i < D; i += T) g[i] = FWD ? r[i] : gl::mul(r[i], tb.twist[i]);
    __syncthreads();
  }
}

hipError_t transform(uint64_t *data, size_t n, int d, bool fwd, const ring::NegaTables &tb,
                     hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (d == 1024 && tb.mid) return transform_n32(data, n, fwd, tb, st);
  if (d == 24) {
    if (fwd)
      hipLaunchKernelGGL(k_phi72_transform<true>, dim3(blocks(n, 256)), dim3(256), 0, st, data, n);
    else
      hipLaunchKernelGGL(k_phi72_transform<false>, dim3(blocks(n, 256)), dim3(256), 0, st, data, n);
    return hipGetLastError();
  }
  return nega_degree(d, [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    if (fwd)
      hipLaunchKernelGGL((k_nega_transform<D, true>), dim3(grid_cap(n)), dim3(NT<D>::T), 0, st, data, n, tb);
    else
      hipLaunchKernelGGL((k_nega_transform<D, false>), dim3(grid_cap(n)), dim3(NT<D>::T), 0, st, data, n, tb);
    return hipGetLastError();
  });
}

// ============================================================ slot-wise ring product
__global__ void k_slot_mul_phi72(const uint64_t *a, const uint64_t *b, uint64_t *out, size_t nslots) {
  size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  uint64_t x[3] = {a[3 * s], a[3 * s + 1], a[3 * s + 2]};
  uint64_t y[3] = {b[3 * s], b[3 * s + 1], b[3 * s + 2]};
  uint64_t z[3];
  gl::fq3_mul(x, y, z);
  out[3 * s] = z[0];
  out[3 * s + 1] = z[1];
  out[3 * s + 2] = z[2];
}
__global__ void k_slot_mul_nega(const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = gl::mul(a[i], b[i]);
}

hipError_t slot_mul(const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n, int d,
                    hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (d == 24)
    hipLaunchKernelGGL(k_slot_mul_phi72, dim3(blocks(n * 8, 256)), dim3(256), 0, st, a, b, out, n * 8);
  else
    hipLaunchKernelGGL(k_slot_mul_nega, dim3(blocks(n * d, 256)), dim3(256), 0, st, a, b, out, n * d);
  return hipGetLastError();
}

// ============================================================ Montgomery edge
__global__ void k_mont(uint64_t *x, size_t n, int to) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) x[i] = to ? gl::to_mont(gl::canon(x[i])) : gl::from_mont(x[i]);
}

hipError_t mont(uint64_t *x, size_t n, bool to, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mont, dim3(blocks(n, 256)), dim3(256), 0, st, x, n, to ? 1 : 0);
  return hipGetLastError();
}

// ============================================================ Witness::from_w_ccs
// LF/arith.rs:230-248: ICRT -> gadget_decompose(B, L) -> CRT.
// Phi_72: one thread per (w_ccs element j, digit l), so a launch has W * L
// threads (about 1,500 waves at the real zkvm shape instead of 310). Each
// thread redoes the ICRT of its element and the digit steps up to l; the last
// digit's thread checks that the carry ran out. Neighbouring threads write
// neighbouring 192-B outputs.
__global__ void __launch_bounds__(128) k_from_w_ccs_phi72(const uint64_t *w_ccs, size_t W, int lb,
                                                         int L, uint64_t *f_coeff, uint64_t *f,
                                                         int *err) {
  const size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (u >= W * (size_t)L) return;
  const size_t j = u / L;
  const int l = (int)(u - j * L);
  uint64_t c[24];
  ring::ld24(w_ccs + j * 24, c);
  ring::phi72_icrt(c);
  int64_t cur[24], dg[24];
#pragma unroll
  for (int i = 0; i < 24; i++) cur[i] = signed_rep(c[i]);
  for (int s = 0; s <= l; s++) {
#pragma unroll
    for (int i = 0; i < 24; i++) dg[i] = bal_digit(cur[i], lb);
  }
#pragma unroll
  for (int i = 0; i < 24; i++) c[i] = from_signed(dg[i]);
  ring::st24(f_coeff + u * 24, c);
  ring::phi72_crt(c);
  ring::st24(f + u * 24, c);
  if (l == L - 1) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 24; i++) bad |= cur[i] != 0;
    if (bad) raise(err, 1);
  }
}

// negacyclic: one workgroup per w_ccs element.
template <int D>
__global__ void __launch_bounds__(NT<D>::T) k_from_w_ccs_nega(const uint64_t *w_ccs, size_t W,
                                                             int lb, int L, uint64_t *f_coeff,
                                                             uint64_t *f, ring::NegaTables fwd,
                                                             ring::NegaTables inv, int *err) {
  constexpr int T = NT<D>::T, PER = D / T;
  __shared__ uint64_t buf[2][D];
  const int tid = threadIdx.x;
  for (size_t j = blockIdx.x; j < W; j += gridDim.x) {
    const uint64_t *g = w_ccs + j * D;
#pragma unroll
    for (int i = tid; i < D; i += T) buf[0][i] = g[i];
    __syncthreads();
    uint64_t *r = ring::stockham4<D, T, true>(buf[0], buf[1], inv.roots, tid);
    int64_t cur[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) cur[q] = signed_rep(gl::mul(r[tid + q * T], inv.twist[tid + q * T]));
    __syncthreads();
    for (int l = 0; l < L; l++) {
      uint64_t *oc = f_coeff + (j * L + l) * D;
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const int i = tid + q * T;
        uint64_t dgt = from_signed(bal_digit(cur[q], lb));
        oc[i] = dgt;
        buf[0][i] = gl::mul(dgt, fwd.twist[i]);
      }
      __syncthreads();
      uint64_t *rr = ring::stockham4<D, T, false>(buf[0], buf[1], fwd.roots, tid);
      uint64_t *of = f + (j * L + l) * D;
#pragma unroll
      for (int q = 0; q < PER; q++) of[tid + q * T] = rr[tid + q * T];
      __syncthreads();
    }
    bool bad = false;
#pragma unroll
    for (int q = 0; q < PER; q++) bad |= cur[q] != 0;
    if (bad) raise(err, 1);
  }
}

hipError_t from_w_ccs(const uint64_t *w_ccs, size_t W, int d, int lb, int L, uint64_t *f_coeff,
                      uint64_t *f, const ring::NegaTables &fwd, const ring::NegaTables &inv, int *err,
                      hipStream_t st, uint32_t *smg) {
  if (W == 0) return hipSuccess;
  if (smg && (d != 1024 || lb > 15 || !fwd.mid || !inv.mid)) return hipErrorInvalidValue;
  if (d == 1024 && fwd.mid && inv.mid) return from_w_ccs_n32(w_ccs, W, lb, L, f_coeff, f, fwd, inv, err, st, smg);
  if (d == 4096 && fwd.tw4 && inv.tw4) return from_w_ccs_n4k(w_ccs, W, lb, L, f_coeff, f, fwd, inv, err, st);
  if (d == 24) {
    hipLaunchKernelGGL(k_from_w_ccs_phi72, dim3(blocks(W * L, 128)), dim3(128), 0, st, w_ccs, W, lb,
                       L, f_coeff, f, err);
    return hipGetLastError();
  }
  return nega_degree(d, [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    hipLaunchKernelGGL((k_from_w_ccs_nega<D>), dim3(grid_cap(W)), dim3(NT<D>::T), 0, st, w_ccs, W, lb, L, f_coeff, f,
                       fwd, inv, err);
    return hipGetLastError();
  });
}

// ============================================================ Witness::from_f
// LF/arith.rs:299-313: f_coeff = ICRT(f); w_ccs = gadget_recompose(f, B, L).
// Phi_72: one thread per f element (j, l); a block holds G = blockDim / L whole
// groups. The raw elements go through LDS, where the block's threads run the
// Horner recompose (balanced_decomposition/mod.rs:105-117) over the G * 24
// w_ccs coefficients and store them contiguously.
__global__ void __launch_bounds__(256) k_from_f_phi72(const uint64_t *f, size_t W, int lb, int L,
                                                     uint64_t *f_coeff, uint64_t *w_ccs, const int *run_if) {
  if (run_if && !*run_if) return;    // uniform: the coefficient-form fold produced f_coeff and w_ccs
  extern __shared__ uint64_t lds[];  // [G * L][24]
  const int G = blockDim.x / L, t = threadIdx.x;
  const size_t j0 = (size_t)blockIdx.x * G;
  const size_t u = j0 * L + t;
  if (t < G * L && u < W * (size_t)L) {
    uint64_t c[24];
    ring::ld24(f + u * 24, c);
#pragma unroll
    for (int i = 0; i < 24; i++) lds[t * 24 + i] = c[i];
    ring::phi72_icrt(c);
    ring::st24(f_coeff + u * 24, c);
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

template <int D>
__global__ void __launch_bounds__(NT<D>::T) k_from_f_nega(const uint64_t *f, size_t W, int lb, int L,
                                                         uint64_t *f_coeff, uint64_t *w_ccs,
                                                         ring::NegaTables inv, const int *run_if) {
  constexpr int T = NT<D>::T, PER = D / T;
  __shared__ uint64_t buf[2][D];
  if (run_if && !*run_if) return;  // uniform: the coefficient-form fold produced f_coeff and w_ccs
  const int tid = threadIdx.x;
  for (size_t j = blockIdx.x; j < W; j += gridDim.x) {
    uint64_t acc[PER];
    for (int l = L - 1; l >= 0; l--) {
      const uint64_t *g = f + (j * L + l) * D;
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const int i = tid + q * T;
        uint64_t v = g[i];
        buf[0][i] = v;
        acc[q] = (l == L - 1) ? v : gl::add(gl::mul_pow2(acc[q], lb), v);
      }
      __syncthreads();
      uint64_t *r = ring::stockham4<D, T, true>(buf[0], buf[1], inv.roots, tid);
      uint64_t *oc = f_coeff + (j * L + l) * D;
#pragma unroll
      for (int q = 0; q < PER; q++) oc[tid + q * T] = gl::mul(r[tid + q * T], inv.twist[tid + q * T]);
      __syncthreads();
    }
    uint64_t *ow = w_ccs + j * D;
#pragma unroll
    for (int q = 0; q < PER; q++) ow[tid + q * T] = acc[q];
  }
}

hipError_t from_f(const uint64_t *f, size_t N, int d, int lb, int L, uint64_t *f_coeff,
                  uint64_t *w_ccs, const ring::NegaTables &inv, hipStream_t st, const int *run_if) {
  const size_t W = N / L;
  if (W == 0) return hipSuccess;
  if (d == 1024 && inv.mid) return from_f_n32(f, W, lb, L, f_coeff, w_ccs, inv, st, run_if);
  if (d == 24) {
    if (L < 1 || L > 256) return hipErrorInvalidValue;
    const int G = 256 / L;
    hipLaunchKernelGGL(k_from_f_phi72, dim3(blocks(W, G)), dim3(G * L), (size_t)G * L * 24 * 8, st, f,
                       W, lb, L, f_coeff, w_ccs, run_if);
    return hipGetLastError();
  }
  if (d == 4096 && inv.tw4) return run_if ? hipErrorInvalidValue : from_f_n4k(f, W, lb, L, f_coeff, w_ccs, inv, st);
  return nega_degree(d, [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    hipLaunchKernelGGL((k_from_f_nega<D>), dim3(grid_cap(W)), dim3(NT<D>::T), 0, st, f, W, lb, L, f_coeff, w_ccs,
                       inv, run_if);
    return hipGetLastError();
  });
}

// ============================================================ decompose_witness
// LF/nifs/decomposition.rs:162-167 + decomposition/utils.rs:45-49 + arith.rs:324-338:
// K balanced base-b_small digit vectors of f_coeff; per digit vector:
// f_k = CRT(f_coeff_k), w_ccs_k = recompose(f_k, B, L). Phi_72: decompose_phi72.hip.
// negacyclic: one workgroup per group of L elements; coefficients of the
// group kept in registers as int64 "cur" (|v| < 2^K for a valid witness).
template <int D>
__global__ void __launch_bounds__(NT<D>::T) k_decompose_nega(const uint64_t *f_coeff, size_t N, int lb,
                                                            int L, int lbs, int K, uint64_t *f_coeff_k,
                                                            uint64_t *f_k, uint64_t *w_ccs_k,
                                                            ring::NegaTables fwd, int *err) {
  constexpr int T = NT<D>::T, PER = D / T, LMAX = 8;
  __shared__ uint64_t buf[2][D];
  const int tid = threadIdx.x;
  const size_t W = N / L;
  for (size_t g = blockIdx.x; g < W; g += gridDim.x) {
    int64_t cur[LMAX][PER];
#pragma unroll
    for (int l = 0; l < LMAX; l++)
      if (l < L)
#pragma unroll
        for (int q = 0; q < PER; q++) cur[l][q] = signed_rep(f_coeff[(g * L + l) * D + tid + q * T]);
    for (int k = 0; k < K; k++) {
      uint64_t acc[PER];
#pragma unroll
      for (int l = LMAX - 1; l >= 0; l--) {
        if (l >= L) continue;
        const size_t e = (size_t)k * N + g * L + l;
#pragma unroll
        for (int q = 0; q < PER; q++) {
          const int i = tid + q * T;
          int64_t dg = bal_digit(cur[l][q], lbs);
          f_coeff_k[e * D + i] = from_signed(dg);
          uint64_t tw = fwd.twist[i];
          buf[0][i] = dg == 0 ? 0 : (dg == 1 ? tw : (dg == -1 ? gl::neg(tw) : gl::mul(from_signed(dg), tw)));
        }
        __syncthreads();
        uint64_t *r = ring::stockham4<D, T, false>(buf[0], buf[1], fwd.roots, tid);
#pragma unroll
        for (int q = 0; q < PER; q++) {
          uint64_t v = r[tid + q * T];
          f_k[e * D + tid + q * T] = v;
          acc[q] = (l == L - 1) ? v : gl::add(gl::mul_pow2(acc[q], lb), v);
        }
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < PER; q++) w_ccs_k[((size_t)k * W + g) * D + tid + q * T] = acc[q];
    }
    bool bad = false;
#pragma unroll
    for (int l = 0; l < LMAX; l++)
      if (l < L)
#pragma unroll
        for (int q = 0; q < PER; q++) bad |= cur[l][q] != 0;
    if (bad) raise(err, 1);
  }
}

hipError_t decompose_witness(const uint64_t *f_coeff, size_t N, int d, int lb, int L, int lbs, int K,
                             uint64_t *f_coeff_k, uint64_t *f_k, uint64_t *w_ccs_k,
                             const ring::NegaTables &fwd, int *err, hipStream_t st, uint4 *frag, int nch,
                             int row0) {
  const size_t W = N / L;
  if (W == 0) return hipSuccess;
  if (d == 1024 && fwd.mid && lbs == 1 && K <= 15 && L <= 5)
    return decompose_n32(f_coeff, N, lb, L, K, f_coeff_k, f_k, w_ccs_k, fwd, err, st);
  if (d == 24) {
    FusedSides sd{};
    sd.nside = 1;
    sd.f_coeff[0] = f_coeff;
    sd.f_coeff_k[0] = f_coeff_k;
    sd.f_k[0] = f_k;
    sd.w_ccs_k[0] = w_ccs_k;
    sd.row0[0] = row0;
    return decompose_phi72_sides(sd, N, lb, L, lbs, K, err, frag, nch, st);
  }
  if (L > 8) return hipErrorInvalidValue;
  return nega_degree(d, [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    hipLaunchKernelGGL((k_decompose_nega<D>), dim3(grid_cap(W)), dim3(NT<D>::T), 0, st, f_coeff, N, lb, L, lbs, K,
                       f_coeff_k, f_k, w_ccs_k, fwd, err);
    return hipGetLastError();
  });
}

}  // namespace lfk
