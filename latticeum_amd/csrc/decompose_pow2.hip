// decompose_pow2.hip -- the fused decomposition of the commit+fold step at X^d + 1,
// d = 2^k, 16 <= d <= 512, b_small = 2, and the expander of
// its packed planes.
//
// A block owns 16 consecutive groups of one side (unit G of fragpos.hpp), so for
// every (plane k, limb l) it makes exactly one 16-column unit of the contraction
// order (Lp = L). Element j of the 16 is transformed by the T threads
// [j T, j T + T) with ring::stockham4<D, T, false> on its own pair of LDS rows; the
// 16 results then lie side by side in one of the two ping-pong halves, which is the
// tile of the byte transpose: thread s reads slot s of the 16 rows (consecutive
// lanes, consecutive words) and writes the eight 16-byte pieces of that slot to
// fv_index(s, nch, chunk, row, half) + 4 digit. The pieces of four neighbouring
// threads form one 64-B run.
//
// The coefficients are read once per unit, range-checked and kept as sign|magnitude
// words in registers (the same words go to sd.smg: the packed planes, digitpack.hpp
// smp2_*); digit k of a word is a bit test, and its twisted value a select and a
// negation of the twist. The OR of the 16 elements' magnitudes per limb says which
// planes of which limb are zero: such a unit is dead (its pieces are not written,
// its flag is 1) and skips its transform.
#include <algorithm>

#include "digits.hpp"
#include "frag.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "ring.hpp"

namespace lfk {

namespace {

constexpr int P2_LMAX = 8;  // limbs held in registers

template <int D>
struct P2 {
  static constexpr int T = D / 4 < 64 ? D / 4 : 64;  // threads per element's transform
  static constexpr int NTH = 16 * T;                 // threads per block: 16 elements at once
  static constexpr int PER = D / T;                  // coefficients per thread
  static constexpr int LDS_U64 = 2 * 16 * D;         // the two Stockham halves of 16 elements
};

using P2Degrees = std::integer_sequence<int, 16, 32, 64, 128, 256, 512>;

// PL (lf_dev_commit_planes): the words are loaded from sd.smg (the caller's packed planes)
// instead of made from f_coeff -- nothing to range-check, nothing to write back
template <int D, bool NT, bool PL>
__global__ void __launch_bounds__(P2<D>::NTH) k_decompose_pow2(size_t N, int L, int lb, int K, FusedSides sd,
                                                              ring::NegaTables fwd, uint4 *frag, int nch,
                                                              int *err) {
  constexpr int T = P2<D>::T, NTH = P2<D>::NTH, PER = P2<D>::PER, H = D / 2, PH = PER / 2;
  __shared__ uint64_t buf[P2<D>::LDS_U64];
  __shared__ uint32_t mags[P2_LMAX];  // per limb: the OR of the 16 elements' magnitudes
  const int tid = threadIdx.x, j = tid / T, t = tid % T;
  uint64_t *x = buf + j * D, *y = buf + 16 * D + j * D;
  const size_t W = N / L, nG = frag_groups(W), ptop = frag_ptop(nG, L);
  for (size_t unit = blockIdx.x; unit < sd.nside * nG; unit += gridDim.x) {
    const int side = unit >= nG;
    const size_t G = unit - side * nG, g = 16 * G + j;
    const bool ok = g < W;  // a group past W: zero digits, nothing stored but its operand bytes
    const size_t e0 = ok ? g * L : 0;
    if (tid < P2_LMAX) mags[tid] = 0;
    __syncthreads();
    // word q of limb l: coefficients t + q T (low half) and t + q T + D / 2 (high half)
    uint32_t sm[P2_LMAX][PH];
    bool bad = false;
#pragma unroll
    for (int l = 0; l < P2_LMAX; l++) {
      if (l >= L) continue;
      uint32_t m = 0;
      if constexpr (PL) {
#pragma unroll
        for (int q = 0; q < PH; q++) {
          sm[l][q] = ok ? sd.smg[side][smp2_word(e0 + l, D, t + q * T)] : 0;
          m |= sm[l][q];
        }
      } else {
      const uint64_t *src = sd.f_coeff[side] + (e0 + l) * D;
#pragma unroll
      for (int q = 0; q < PH; q++) {
        const int i = t + q * T;
        int64_t lo = 0, hi = 0;
        if (ok) {
          lo = signed_rep(src[i]);
          hi = signed_rep(src[i + H]);
          bad = bad || sm16_overflow(lo, K) || sm16_overflow(hi, K);
        }
        sm[l][q] = smp2_make(lo, hi);
        if (ok) sd.smg[side][smp2_word(e0 + l, D, i)] = sm[l][q];
        m |= sm[l][q];
      }
      }
      m = (m | (m >> 16)) & SM16_MAG;
      if (m) atomicOr(&mags[l], m);
    }
    if (bad) raise(err, 1);
    __syncthreads();
    uint64_t *fck = sd.f_coeff_k[side], *fk = sd.f_k[side];
    // the (plane, limb) loops stay rolled: one copy of the transform and the transpose
#pragma unroll 1
    for (int k = 0; k < K; k++) {
      const int row = k > 0 ? sd.row0[side] + k - 1 : sd.row_p0[side];
      uint64_t acc[PER];
#pragma unroll 1
      for (int l = L - 1; l >= 0; l--) {
        // limb l's words, by selects over the register copy (l is block-uniform)
        uint32_t cur[PH];
#pragma unroll
        for (int q = 0; q < PH; q++) cur[q] = 0;
#pragma unroll
        for (int ll = 0; ll < P2_LMAX; ll++)
#pragma unroll
          for (int q = 0; q < PH; q++) cur[q] = ll == l ? sm[ll][q] : cur[q];
        // block-uniform; without flags every unit is written
        const bool live = !sd.dead || ((mags[l] >> k) & 1u);
        const size_t e = (size_t)k * N + e0 + l;
        uint64_t v[PER];
        const uint64_t *r = x;
        if (live) {
#pragma unroll
          for (int q = 0; q < PER; q++) {
            const uint32_t w = cur[q % PH] >> (16 * (q / PH));
            const bool bit = (w >> k) & 1u, neg = (w >> 15) & 1u;
            const int i = t + q * T;
            const uint64_t tw = fwd.twist[i];  // d words: cache-resident
            x[i] = bit ? (neg ? gl::neg(tw) : tw) : 0;
            if (fck && ok) out_store<NT>(&fck[e * D + i], (uint64_t)(bit ? (neg ? gl::P - 1 : 1) : 0));
          }
          __syncthreads();
          r = ring::stockham4<D, T, false>(x, y, fwd.roots, t);
#pragma unroll
          for (int q = 0; q < PER; q++) v[q] = r[t + q * T];
        } else {
#pragma unroll
          for (int q = 0; q < PER; q++) {
            v[q] = 0;
            if (fck && ok) out_store<NT>(&fck[e * D + t + q * T], (uint64_t)0);
          }
        }
        if (fk && ok) {
#pragma unroll
          for (int q = 0; q < PER; q++) out_store<NT>(&fk[e * D + t + q * T], v[q]);
        }
#pragma unroll
        for (int q = 0; q < PER; q++) acc[q] = l == L - 1 ? v[q] : gl::add(gl::mul_pow2(acc[q], lb), v[q]);
        if (row >= 0) {
          const size_t pos = frag_pos(G, l, L, ptop);
          if (sd.dead && tid == 0) sd.dead[pos * 32 + row] = live ? 0 : 1;
          if (live) {
            const uint64_t *tile = r - j * D;  // the half that holds the 16 results
            for (int s = tid; s < D; s += NTH) {
              uint64_t xs[16];
#pragma unroll
              for (int jj = 0; jj < 16; jj++) xs[jj] = fenc(tile[jj * D + s]);
              uint4 pu[8];
              d8_transpose16(xs, pu);
              uint4 *out = frag + fv_index((size_t)s, nch, (int)(pos >> 1), row, (int)(pos & 1));
#pragma unroll
              for (int b = 0; b < 8; b++) out_store<NT>(&out[4 * b], pu[b]);
            }
          }
        }
        if (live) __syncthreads();  // the tile is read before the next unit's digits overwrite it
      }
      if (ok && (!PL || sd.w_ccs_k[side])) {  // from planes: w_ccs_k may be null
        uint64_t *ow = sd.w_ccs_k[side] + ((size_t)k * W + g) * D;
#pragma unroll
        for (int q = 0; q < PER; q++) ow[t + q * T] = acc[q];
      }
    }
    __syncthreads();  // mags is read to the end of the unit
  }
}

// the packed words -> the K digit planes in coefficient form, one thread per output
__global__ void k_expand_smp2(const uint32_t *smg, size_t N, int d, int K, uint64_t *fck) {
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < (size_t)K * N * d;
       t += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(t % d), k = (int)(t / (N * d));
    const size_t e = (t / d) % N;
    const int dg = smp2_digit(smg, e, d, i, k);
    fck[t] = dg ? (dg < 0 ? gl::P - 1 : 1) : 0;
  }
}

}  // namespace

hipError_t decompose_pow2(const FusedSides &sd, size_t N, int d, int lb, int L, int K, const ring::NegaTables &fwd,
                          uint4 *frag, int nch, int *err, hipStream_t st) {
  if (!smp2_degree(d) || K < 1 || K > 15 || L < 1 || L > P2_LMAX || N % L || sd.nside < 1 || sd.nside > 2 || !frag ||
      !fwd.twist || !fwd.roots)
    return hipErrorInvalidValue;
  int nrows = 1;  // the operand rows, plus the u64 rows the caller keeps
  for (int s = 0; s < sd.nside; s++) {
    if (!sd.smg[s] || (!sd.planes_in() && (!sd.f_coeff[s] || !sd.w_ccs_k[s]))) return hipErrorInvalidValue;
    if (sd.row0[s] < 0 || sd.row0[s] + K - 1 > 32 || sd.row_p0[s] >= 32) return hipErrorInvalidValue;
    nrows = std::max(nrows, 1 + (sd.f_k[s] ? 1 : 0) + (sd.f_coeff_k[s] ? 1 : 0));
  }
  if (N == 0) return hipSuccess;
  const size_t units = sd.nside * frag_groups(N / L);
  // the fold re-reads the operand rows (or f_k): cached stores below the streaming threshold
  const bool nt = dec_streaming(sd.nside * (size_t)K * N * d * 8 * nrows, /*refold=*/true);
  return nega_degree_in(d, [&](auto dd) {
    constexpr int D = decltype(dd)::value;
#define LF_P2(NT_, PL_)                                                                                             \
  hipLaunchKernelGGL((k_decompose_pow2<D, NT_, PL_>), dim3(grid_cap(units)), dim3(P2<D>::NTH), 0, st, N, L, lb, K, sd, \
                     fwd, frag, nch, err)
    if (sd.planes_in()) {
      if (nt) LF_P2(true, true); else LF_P2(false, true);
    } else {
      if (nt) LF_P2(true, false); else LF_P2(false, false);
    }
#undef LF_P2
    return hipGetLastError();
  }, P2Degrees{});
}

hipError_t expand_smp2(const uint32_t *smg, size_t N, int d, int K, uint64_t *fck, hipStream_t st) {
  if (!N) return hipSuccess;
  if (!smp2_degree(d) || K < 1 || K > 15) return hipErrorInvalidValue;
  const size_t n = (size_t)K * N * d;
  hipLaunchKernelGGL(k_expand_smp2, dim3(grid_cap(blocks(n, 256))), dim3(256), 0, st, smg, N, d, K, fck);
  return hipGetLastError();
}

}  // namespace lfk
