// ajtai.hip -- the VALU Ajtai commitment (the matrix-core one is ajtai_mfma.hip) and the
// sums over its column splits.
#include "kernels.hpp"
#include "launch.hpp"
#include "ring.hpp"

namespace lfk {

using gl::Acc;

// ============================================================ Ajtai commitment
// LF/commitment/commitment_scheme.rs:37-54 -> LA/matrix.rs:168-178:
//   cm[v][i] = sum_j A[i][j] (.) f_v[j]    (slot-wise products)
// Work units: (slot chunk, row tile, column split) x vector tile. Each thread
// owns one slot position and an R x V tile of column accumulators (gl::CAcc,
// 8 VALU ops per 64x64 MAC). Units that read the same A tile (same slot
// chunk / row tile / column split, different vector tiles) get block ids
// that are congruent mod 8, i.e. land on one XCD under round-robin dispatch,
// so A is re-read from that XCD's L2 rather than HBM (speed only). Loads of
// column j+1 are issued before the MACs of column j.
struct AjtaiGrid {
  int nsc, nrt, nsplit, nvt;  // slot chunks, row tiles, column splits, vector tiles
  __host__ __device__ int others() const { return nsc * nrt * nsplit; }
  __host__ __device__ unsigned blocks() const { return (unsigned)(((others() + 7) / 8) * nvt * 8); }
};
__device__ __forceinline__ bool ajtai_unit(const AjtaiGrid &g, int &sc, int &rt, int &js, int &vt) {
  const int L = blockIdx.x;
  const int lo = L % 8, hi = L / 8;
  vt = hi % g.nvt;
  const int other = (hi / g.nvt) * 8 + lo;
  if (other >= g.others()) return false;
  sc = other % g.nsc;
  rt = (other / g.nsc) % g.nrt;
  js = other / (g.nsc * g.nrt);
  return true;
}

template <int R, int V>
__global__ void __launch_bounds__(256) k_ajtai_nega(const uint64_t *A, size_t kappa, size_t ncols,
                                                   int d, VecPtrs fv, int nvec, size_t jchunk,
                                                   AjtaiGrid g, uint64_t *partial) {
  int sc, rt, js, vt;
  if (!ajtai_unit(g, sc, rt, js, vt)) return;
  const int s = sc * 256 + threadIdx.x;  // slot
  if (s >= d) return;
  const int i0 = rt * R, v0 = vt * V;
  const size_t j0 = (size_t)js * jchunk, j1 = min(ncols, j0 + jchunk);
  const uint64_t *pa[R];
  const uint64_t *pb[V];
#pragma unroll
  for (int r = 0; r < R; r++) pa[r] = A + ((size_t)min(i0 + r, (int)kappa - 1) * ncols) * d + s;
#pragma unroll
  for (int v = 0; v < V; v++) pb[v] = fv.p[min(v0 + v, nvec - 1)] + s;
  gl::CAcc acc[R][V];
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int v = 0; v < V; v++) gl::cacc_zero(acc[r][v]);
  uint64_t a[R], b[V];
  if (j0 < j1) {
#pragma unroll
    for (int r = 0; r < R; r++) a[r] = pa[r][j0 * d];
#pragma unroll
    for (int v = 0; v < V; v++) b[v] = pb[v][j0 * d];
  }
  for (size_t j = j0; j < j1; j++) {
    uint64_t an[R], bn[V];
    const size_t jn = (j + 1 < j1 ? j + 1 : j) * d;
#pragma unroll
    for (int r = 0; r < R; r++) an[r] = pa[r][jn];
#pragma unroll
    for (int v = 0; v < V; v++) bn[v] = pb[v][jn];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int v = 0; v < V; v++) gl::cacc_mad(acc[r][v], a[r], b[v]);
#pragma unroll
    for (int r = 0; r < R; r++) a[r] = an[r];
#pragma unroll
    for (int v = 0; v < V; v++) b[v] = bn[v];
  }
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int v = 0; v < V; v++)
      if (i0 + r < (int)kappa && v0 + v < nvec)
        partial[(((size_t)js * nvec + v0 + v) * kappa + i0 + r) * d + s] = gl::cacc_reduce(acc[r][v]);
}

// Phi_72: lanes = 8 Fq3 slots x 8 column phases; R x V tile of Fq3 accumulators
// (9 column-accumulated products per Fq3 MAC into 5 sums, ring::fq3acc layout).
struct Fq3CAcc {
  gl::CAcc s00, s0n, s1, s1n, s2;
};
template <int R, int V>
__global__ void __launch_bounds__(256) k_ajtai_phi72(const uint64_t *A, size_t kappa, size_t ncols,
                                                    VecPtrs fv, int nvec, size_t jchunk,
                                                    uint64_t *partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane & 7, ph = lane >> 3;  // column phase 0..7
  const int i0 = blockIdx.y * R;
  const int nvt = (nvec + V - 1) / V;
  const int v0 = (blockIdx.z % nvt) * V;
  const int js = blockIdx.x * 4 + wave;  // column split index
  const size_t j0 = (size_t)js * jchunk, j1 = min(ncols, j0 + jchunk);
  Fq3CAcc acc[R][V];
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int v = 0; v < V; v++) {
      gl::cacc_zero(acc[r][v].s00);
      gl::cacc_zero(acc[r][v].s0n);
      gl::cacc_zero(acc[r][v].s1);
      gl::cacc_zero(acc[r][v].s1n);
      gl::cacc_zero(acc[r][v].s2);
    }
  for (size_t j = j0 + ph; j < j1; j += 8) {
    uint64_t a[R][3], b[V][3];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint64_t *p = A + ((size_t)min(i0 + r, (int)kappa - 1) * ncols + j) * 24 + 3 * slot;
      a[r][0] = p[0];
      a[r][1] = p[1];
      a[r][2] = p[2];
    }
#pragma unroll
    for (int v = 0; v < V; v++) {
      const uint64_t *p = fv.p[min(v0 + v, nvec - 1)] + j * 24 + 3 * slot;
      b[v][0] = p[0];
      b[v][1] = p[1];
      b[v][2] = p[2];
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int v = 0; v < V; v++) {
        Fq3CAcc &q = acc[r][v];
        gl::cacc_mad(q.s00, a[r][0], b[v][0]);
        gl::cacc_mad(q.s0n, a[r][1], b[v][2]);
        gl::cacc_mad(q.s0n, a[r][2], b[v][1]);
        gl::cacc_mad(q.s1, a[r][0], b[v][1]);
        gl::cacc_mad(q.s1, a[r][1], b[v][0]);
        gl::cacc_mad(q.s1n, a[r][2], b[v][2]);
        gl::cacc_mad(q.s2, a[r][0], b[v][2]);
        gl::cacc_mad(q.s2, a[r][1], b[v][1]);
        gl::cacc_mad(q.s2, a[r][2], b[v][0]);
      }
  }
  // c0 = s00 + 2^40 s0n, c1 = s1 + 2^40 s1n, c2 = s2; then sum the 8 column phases
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int v = 0; v < V; v++) {
      const Fq3CAcc &q = acc[r][v];
      uint64_t c[3];
      c[0] = gl::add(gl::cacc_reduce(q.s00), gl::mul_pow2(gl::cacc_reduce(q.s0n), 40));
      c[1] = gl::add(gl::cacc_reduce(q.s1), gl::mul_pow2(gl::cacc_reduce(q.s1n), 40));
      c[2] = gl::cacc_reduce(q.s2);
#pragma unroll
      for (int off = 8; off < 64; off <<= 1)
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = gl::add(c[k], __shfl_xor(c[k], off));
      if (ph == 0 && i0 + r < (int)kappa && v0 + v < nvec) {  // empty splits write zeros
        uint64_t *o = partial + (((size_t)js * nvec + v0 + v) * kappa + i0 + r) * 24 + 3 * slot;
        o[0] = c[0];
        o[1] = c[1];
        o[2] = c[2];
      }
    }
}

// sum nsplit partial planes of len u64 each (mod p)
__global__ void k_sum_planes(const uint64_t *partial, int nsplit, size_t len, uint64_t *out,
                             size_t out_stride_vec, size_t per_vec) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= len) return;
  Acc a;
  gl::acc_zero(a);
  for (int s = 0; s < nsplit; s++) gl::acc_add(a, partial[(size_t)s * len + i]);
  size_t v = i / per_vec, r = i % per_vec;
  out[v * out_stride_vec + r] = gl::acc_reduce(a);
}

int ajtai_nsplit(size_t ncols, int d, int nvec) {
  if (d == 24) {
    // one wave per column split; ~64 columns per lane phase minimum
    size_t want = (ncols + 511) / 512;
    if (want > 1024) want = 1024;
    return (int)((want + 3) / 4 * 4);
  }
  // enough units to fill 256 CUs: (d/256) slot chunks x (kappa/R) row tiles x nsplit x nvt
  size_t want = (ncols + 127) / 128;
  if (want > 40) want = 40;
  if (want < 1) want = 1;
  return (int)want;
}
size_t ajtai_partial_elems(size_t kappa, size_t ncols, int d, int nvec) {
  size_t nsplit = ajtai_nsplit(ncols, d, nvec);
  return nsplit * (size_t)nvec * kappa * (size_t)d;
}

hipError_t ajtai_commit(const uint64_t *A, size_t kappa, size_t ncols, int d, const VecPtrs &fv,
                        int nvec, uint64_t *partial, uint64_t *cm, hipStream_t st, hipEvent_t ev0,
                        hipEvent_t ev1) {
  if (nvec <= 0 || nvec > LF_MAX_VECS) return hipErrorInvalidValue;
  const int nsplit = ajtai_nsplit(ncols, d, nvec);
  const size_t jchunk = (ncols + nsplit - 1) / nsplit;
  if (ev0) (void)hipEventRecord(ev0, st);
  if (d == 24) {
    constexpr int R = 2, V = 2;
    const int nvt = (nvec + V - 1) / V;
    dim3 grid(nsplit / 4, (unsigned)((kappa + R - 1) / R), nvt);
    hipLaunchKernelGGL((k_ajtai_phi72<R, V>), grid, dim3(256), 0, st, A, kappa, ncols, fv, nvec, jchunk,
                       partial);
  } else if (nvec == 1) {
    constexpr int R = 8, V = 1;
    AjtaiGrid g{(d + 255) / 256, (int)((kappa + R - 1) / R), nsplit, 1};
    hipLaunchKernelGGL((k_ajtai_nega<R, V>), dim3(g.blocks()), dim3(256), 0, st, A, kappa, ncols, d, fv,
                       nvec, jchunk, g, partial);
  } else {
    constexpr int R = 4, V = 4;
    AjtaiGrid g{(d + 255) / 256, (int)((kappa + R - 1) / R), nsplit, (nvec + V - 1) / V};
    hipLaunchKernelGGL((k_ajtai_nega<R, V>), dim3(g.blocks()), dim3(256), 0, st, A, kappa, ncols, d, fv,
                       nvec, jchunk, g, partial);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (ev1) (void)hipEventRecord(ev1, st);
  const size_t len = (size_t)nvec * kappa * d;
  hipLaunchKernelGGL(k_sum_planes, dim3(blocks(len, 256)), dim3(256), 0, st, partial, nsplit, len, cm,
                     kappa * (size_t)d, kappa * (size_t)d);
  return hipGetLastError();
}

hipError_t sum_planes(const uint64_t *partial, int nsplit, size_t len, uint64_t *out, hipStream_t st) {
  if (len == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sum_planes, dim3(blocks(len, 256)), dim3(256), 0, st, partial, nsplit, len, out, len, len);
  return hipGetLastError();
}

// 64 outputs x 4 split groups per block: wave g sums splits g, g + 4, ... of
// its 64 outputs (coalesced), and the 4 partial sums meet in LDS
__global__ void __launch_bounds__(256) k_sum_planes_to(const uint64_t *partial, int nsplit, size_t len, int nvec,
                                                      OutPtrs out) {
  __shared__ uint64_t part[3][64];
  const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
  const size_t i = blockIdx.x * (size_t)64 + o;
  const bool ok = i < len * nvec;
  Acc a;
  gl::acc_zero(a);
  if (ok)
    for (int s = g; s < nsplit; s += 4) gl::acc_add(a, partial[(size_t)s * len * nvec + i]);
  const uint64_t v = gl::acc_reduce(a);
  if (g > 0) part[g - 1][o] = v;
  __syncthreads();
  if (g == 0 && ok) out.p[i / len][i % len] = gl::add(gl::add(v, part[0][o]), gl::add(part[1][o], part[2][o]));
}

hipError_t sum_planes_to(const uint64_t *partial, int nsplit, size_t len, int nvec, const OutPtrs &out,
                         hipStream_t st) {
  if (len == 0 || nvec < 1) return hipSuccess;
  hipLaunchKernelGGL(k_sum_planes_to, dim3(blocks(len * nvec, 64)), dim3(256), 0, st, partial, nsplit, len, nvec,
                     out);
  return hipGetLastError();
}

}  // namespace lfk
