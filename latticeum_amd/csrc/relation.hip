// relation.hip -- the proving loop's self-checks on the device: CCS::check_relation
// (latticefold/src/arith.rs:78-105; check_relation_debug, zkvm/src/constraints.rs:1833-1871),
// the row values its failure report prints, the witness's linf norm on signed
// representatives (stark-rings ring/src/traits.rs:23-34, balanced_decomposition/
// convertible_ring.rs:59-66) and a first-difference compare of two device buffers
// (the witness-consistency checks of lf_lcccs_check / lf_cccs_check).
//
// The relation is sum_i c_i (.) prod_(j in S_i) (M_j z) = 0 on every row. It is
// slot-wise, so it runs as mz.hip's mat_vec_mul does -- one thread per (row, NTT slot)
// -- with the Hadamard products and the c-weighted sum taken on the row sums in
// registers: no M_j z vector is written, and the answer is one word per z.
#include "kernels.hpp"
#include "launch.hpp"
#include "slot.hpp"

namespace lfk {

namespace {

constexpr int RT = 256;
constexpr uint64_t NONE = ~0ull;

// the block's minimum (MAX: maximum) of v, in thread 0; every thread of the block calls it
template <bool MAX>
__device__ __forceinline__ uint64_t block_reduce(uint64_t v, uint64_t *red) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint64_t w = (uint64_t)__shfl_xor((unsigned)(v >> 32), o) << 32 | __shfl_xor((unsigned)v, o);
    v = (MAX ? w > v : w < v) ? w : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (unsigned i = 1; i < (blockDim.x + 63) / 64; i++) v = (MAX ? red[i] > v : red[i] < v) ? red[i] : v;
  return v;
}

// row r of M z at one slot: sum_k val[k] (.) z[col[k]], k in [k, e) -- k_csr's row sum
// (four entries' index loads, then their value and z loads, issued together)
template <int TB, bool SC>
__device__ __forceinline__ Sv<TB> row_sum(uint64_t k, uint64_t e, const uint32_t *col, const uint64_t *val, int d,
                                          int slot, const uint64_t *zb) {
  SAcc<TB> acc;
  sacc_zero(acc);
  auto term = [&](uint64_t vi, uint32_t c) {
    if (SC)
      sacc_smad(acc, val[vi], s_load<TB>(zb + (size_t)c * d));
    else
      sacc_mad(acc, s_load<TB>(val + vi * d + slot * TB), s_load<TB>(zb + (size_t)c * d));
  };
  for (; k + 4 <= e; k += 4) {
    uint32_t c[4];
#pragma unroll
    for (int u = 0; u < 4; u++) c[u] = col[k + u];
#pragma unroll
    for (int u = 0; u < 4; u++) term(k + u, c[u]);
  }
  for (; k < e; k++) term(k, col[k]);
  return sacc_final(acc);
}

// resid[b][r] = sum_i c_i (.) prod_(j in S_i) (M_j z_b)[r] (b = blockIdx.y; resid may be
// null) and first_bad[b] = min(first_bad[b], the block's smallest row with a nonzero word).
// An empty multiset's product is ONE; an index repeated in a multiset multiplies the row
// sum in again (computed once when the repeats are adjacent). A matrix named by several
// multisets has its row summed once per multiset. One atomic per block, from blocks
// that hold an unsatisfied row only; with slot tiling (blockIdx.z) each tile's block
// reports for its own slots, and the minimum over them is the OR over the slots.
template <int TB, bool SC>
__global__ void __launch_bounds__(RT) k_ccs_relation(const uint64_t *rp, size_t rp_stride, const uint32_t *col,
                                                    const uint64_t *val, size_t nrows, int d, const uint64_t *z,
                                                    size_t z_stride, const uint64_t *c, int q, const int *S_off,
                                                    const int *S_idx, uint64_t *resid, unsigned long long *first_bad,
                                                    int spb) {
  __shared__ uint64_t red[RT / 64];
  const int slot_l = threadIdx.x % spb, lane_r = threadIdx.x / spb, rpb = RT / spb;
  const int slot = blockIdx.z * spb + slot_l;
  const size_t r = (size_t)blockIdx.x * rpb + lane_r;
  uint64_t bad = NONE;
  if (r < nrows) {  // no return: the block reduction below is block-wide
    const uint64_t *zb = z + blockIdx.y * z_stride + slot * TB;
    SAcc<TB> tot;
    sacc_zero(tot);
    for (int i = 0; i < q; i++) {
      Sv<TB> prod = s_one<TB>(), rs = s_zero<TB>();
      int prev = -1;
      for (int k = S_off[i]; k < S_off[i + 1]; k++) {
        const int j = S_idx[k];
        if (j != prev) {
          const uint64_t *rpa = rp + (size_t)j * rp_stride;
          rs = row_sum<TB, SC>(rpa[r], rpa[r + 1], col, val, d, slot, zb);
        }
        prod = prev < 0 ? rs : s_mul(prod, rs);
        prev = j;
      }
      sacc_mad(tot, s_load<TB>(c + (size_t)i * d + slot * TB), prod);
    }
    const Sv<TB> v = sacc_final(tot);
    if (resid) s_store(resid + (blockIdx.y * nrows + r) * d + slot * TB, v);
    if (!s_is_zero(v)) bad = r;
  }
  bad = block_reduce<false>(bad, red);
  if (threadIdx.x == 0 && bad != NONE) atomicMin(first_bad + blockIdx.y, (unsigned long long)bad);
}

// out[j] = (M_j z)[row]: one block per matrix, its threads over the slots
template <int TB, bool SC>
__global__ void __launch_bounds__(RT) k_ccs_row_evals(const uint64_t *rp, size_t rp_stride, const uint32_t *col,
                                                     const uint64_t *val, size_t row, int d, const uint64_t *z,
                                                     uint64_t *out) {
  const uint64_t *rpa = rp + (size_t)blockIdx.x * rp_stride;
  const uint64_t k = rpa[row], e = rpa[row + 1];
  for (int slot = threadIdx.x; slot < d / TB; slot += RT)
    s_store(out + (size_t)blockIdx.x * d + slot * TB, row_sum<TB, SC>(k, e, col, val, d, slot, z + slot * TB));
}

// the 16-byte pieces of n words at x (8-byte aligned): `head` (0 or 1) words before the
// first aligned piece, then `pairs` pieces, then `tail` (0 or 1) words
struct Pieces {
  size_t head, pairs, tail;
};
__device__ __forceinline__ Pieces pieces(const uint64_t *x, size_t n) {
  Pieces p;
  p.head = n && ((uintptr_t)x & 8) ? 1 : 0;
  p.pairs = (n - p.head) / 2;
  p.tail = n - p.head - 2 * p.pairs;
  return p;
}

__device__ __forceinline__ uint64_t absval(uint64_t x) { return x < gl::P - x ? x : gl::P - x; }

// *out = max(*out, max_i min(x_i, p - x_i)): linf_norm of canonical words on their signed
// representatives. 16-byte loads, a wave then a block reduction, one atomic per block
// (none from a block of zeros: *out starts at 0). A maximum: no order dependence
__global__ void __launch_bounds__(RT) k_linf_norm(const uint64_t *x, size_t n, unsigned long long *out) {
  __shared__ uint64_t red[RT / 64];
  const Pieces p = pieces(x, n);
  const ulonglong2 *xp = reinterpret_cast<const ulonglong2 *>(x + p.head);
  uint64_t m = 0;
  for (size_t i = blockIdx.x * (size_t)RT + threadIdx.x; i < p.pairs; i += (size_t)gridDim.x * RT) {
    const ulonglong2 v = xp[i];
    const uint64_t a = absval(v.x), b = absval(v.y);
    m = a > m ? a : m;
    m = b > m ? b : m;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (p.head) m = absval(x[0]) > m ? absval(x[0]) : m;
    if (p.tail) m = absval(x[n - 1]) > m ? absval(x[n - 1]) : m;
  }
  m = block_reduce<true>(m, red);
  if (threadIdx.x == 0 && m) atomicMax(out, (unsigned long long)m);
}

// *out = min(*out, the smallest i with a[i] != b[i]) (*out starts at all-ones: none);
// 16-byte loads when both buffers are 16-byte aligned and n is even (whole ring elements
// from an allocation's start), else word loads. The first difference a thread meets is
// its smallest: its indices only grow
__global__ void __launch_bounds__(RT) k_first_diff(const uint64_t *a, const uint64_t *b, size_t n,
                                                  unsigned long long *out) {
  __shared__ uint64_t red[RT / 64];
  uint64_t bad = NONE;
  const size_t t0 = blockIdx.x * (size_t)RT + threadIdx.x, step = (size_t)gridDim.x * RT;
  if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0 && n % 2 == 0) {
    const ulonglong2 *ap = reinterpret_cast<const ulonglong2 *>(a);
    const ulonglong2 *bp = reinterpret_cast<const ulonglong2 *>(b);
    for (size_t i = t0; i < n / 2 && bad == NONE; i += step) {
      const ulonglong2 u = ap[i], v = bp[i];
      if (u.x != v.x)
        bad = 2 * i;
      else if (u.y != v.y)
        bad = 2 * i + 1;
    }
  } else {
    for (size_t i = t0; i < n && bad == NONE; i += step)
      if (a[i] != b[i]) bad = i;
  }
  bad = block_reduce<false>(bad, red);
  if (threadIdx.x == 0 && bad != NONE) atomicMin(out, (unsigned long long)bad);
}

// blocks of a grid-stride pass over n items: one item per thread up to a few waves per CU
unsigned stride_blocks(size_t n) {
  const size_t b = blocks(n, RT);
  return (unsigned)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

}  // namespace

hipError_t ccs_relation(const CcsDev &M, const uint64_t *z, int nz, const uint64_t *c, int q, const int *S_off,
                        const int *S_idx, uint64_t *resid, uint64_t *first_bad, hipStream_t st) {
  if (nz < 1 || nz > 65535 || q < 1) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(first_bad, 0xFF, (size_t)nz * 8, st);
  if (e != hipSuccess || !M.m) return e;
  const int d = M.d, tb = slot_words(d), ns = d / tb, spb = ns < RT ? ns : RT;
  const dim3 grid(blocks(M.m, RT / spb), (unsigned)nz, (unsigned)(ns / spb));
  unsigned long long *fb = reinterpret_cast<unsigned long long *>(first_bad);
#define LF_REL(TB, SC, VAL)                                                                                          \
  hipLaunchKernelGGL((k_ccs_relation<TB, SC>), grid, dim3(RT), 0, st, M.rp, M.m + 1, M.col, VAL, M.m, d, z, M.n * d, \
                     c, q, S_off, S_idx, resid, fb, spb)
  if (tb == 3) {
    if (M.sval)
      LF_REL(3, true, M.sval);
    else
      LF_REL(3, false, M.val);
  } else {
    if (M.sval)
      LF_REL(1, true, M.sval);
    else
      LF_REL(1, false, M.val);
  }
#undef LF_REL
  return hipGetLastError();
}

hipError_t ccs_row_evals(const CcsDev &M, const uint64_t *z, size_t row, uint64_t *out, hipStream_t st) {
  if (row >= M.m) return hipErrorInvalidValue;
  const int tb = slot_words(M.d);
#define LF_ROW(TB, SC, VAL)                                                                                     \
  hipLaunchKernelGGL((k_ccs_row_evals<TB, SC>), dim3((unsigned)M.t), dim3(RT), 0, st, M.rp, M.m + 1, M.col, VAL, row, \
                     M.d, z, out)
  if (tb == 3) {
    if (M.sval)
      LF_ROW(3, true, M.sval);
    else
      LF_ROW(3, false, M.val);
  } else {
    if (M.sval)
      LF_ROW(1, true, M.sval);
    else
      LF_ROW(1, false, M.val);
  }
#undef LF_ROW
  return hipGetLastError();
}

hipError_t linf_norm(const uint64_t *x, size_t n, uint64_t *out, hipStream_t st) {
  hipError_t e = hipMemsetAsync(out, 0, 8, st);
  if (e != hipSuccess || !n) return e;
  hipLaunchKernelGGL(k_linf_norm, dim3(stride_blocks(n / 2)), dim3(RT), 0, st, x, n,
                     reinterpret_cast<unsigned long long *>(out));
  return hipGetLastError();
}

hipError_t first_diff(const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out, hipStream_t st) {
  hipError_t e = hipMemsetAsync(out, 0xFF, 8, st);
  if (e != hipSuccess || !n) return e;
  hipLaunchKernelGGL(k_first_diff, dim3(stride_blocks(n / 2)), dim3(RT), 0, st, a, b, n,
                     reinterpret_cast<unsigned long long *>(out));
  return hipGetLastError();
}

}  // namespace lfk
