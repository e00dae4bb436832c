// ajtai_seeded.hip -- the Ajtai matrix derived on the device from a seed
// (include/lf.h, lf_ajtai_create_seeded): the u64 matrix never exists, the
// generator's words go straight into the i8-MFMA operand order of ajtai_mfma.hip.
//
// Both kinds produce an element in blocks of 8 words (seed_block8): one width-16
// Poseidon2 permutation per block (LF_AJTAI_SEED_POSEIDON2, state layout in lf.h
// and ajtai_seed.hpp), or 8 words of the SplitMix stream (LF_AJTAI_SEED_SPLITMIX).
//  * k_seed_frag: k_to_frag's block (16 slots x 8 rows x one 32-column chunk, the
//    same tile, d8, d8_transpose16, op_slot and A-side index) whose load phase
//    computes the words. One thread fills 8 tile words per pass (two passes: a
//    16-slot block of one (row, column) is two generator blocks); Phi_72 runs an
//    element's three blocks in one thread and evaluates the Toom-3 virtual slots of
//    its slot block from them. A block walks the chunks blockIdx.y, + gridDim.y, ..
//    and its emit threads, which hold the raw words of one (row, slot, 16-column
//    unit) before they are digit-encoded, keep that (row, slot)'s sum per chunk
//    class as two 64-bit sums of 32-bit halves (exact: < 2^32 columns). The sums go
//    to a scratch of gridDim.y x 4 x kappa x dv words, whose size does not depend
//    on the width, and k_seed_kr folds them into the `kr` tables (for Phi_72 the
//    virtual-slot sums directly: the evaluation is linear).
//  * k_seed_expand: the plain u64 window [nrows][ncols][d].
#include "ajtai_seed.hpp"
#include "frag.hpp"
#include "kernels.hpp"
#include "launch.hpp"

namespace lfk {

namespace seeded {
#include "p2_perm.inc"
}  // namespace seeded

// words 8 j .. 8 j + 7 of element (row, col), col the global column
template <int KIND>
__device__ __forceinline__ void seed_block8(const SeedGen &g, size_t row, size_t col, int j, uint64_t *o) {
  if (KIND == LF_AJTAI_SEED_POSEIDON2) {
    uint64_t s[16];
    seed_p2_state(g, row, col, j, s);
    {
      using namespace seeded;
      LF_P2_ROUNDS(s, 30);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = s[i];
  } else {
    const uint64_t base = ((uint64_t)row * g.ncols_total + col) * (uint64_t)g.d + 8 * (uint64_t)j;
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = seed_splitmix_word(g.seed[0], base + i);
  }
}

// ---------------------------------------------------------------- the fragment writer
// grid = (slot blocks, chunk walkers gy, row groups of 8 over all kappa rows);
// row i is row i % 32 of A's tile i / 32 (tile_u4 uint4 apart). ctop: the first
// chunk of the top region (nch when the geometry has none). Rows past kappa are
// not written, columns past the width hold zero, as k_to_frag leaves them.
template <int KIND, bool PHI72>
__global__ void __launch_bounds__(256) k_seed_frag(SeedGen g, int kappa, size_t col0, int dv, int nch, int Lp,
                                                   size_t Wp, uint4 *Af, size_t tile_u4, int qd, int ctop,
                                                   uint64_t *part) {
  __shared__ uint64_t tile[TF_R * TF_S * TF_J];
  const int sb = blockIdx.x, tid = threadIdx.x, r0 = blockIdx.z * TF_R;
  // emit: thread = (slot sl, half h, row r), as in k_to_frag
  const int er = tid & 7, eh = (tid >> 3) & 1, esl = tid >> 4;
  const int erow = r0 + er;
  const bool emit = erow < kappa && sb * TF_S + esl < dv;
  uint64_t flo = 0, fhi = 0, tlo = 0, thi = 0;  // this (row, slot)'s sums below the top region and in it
  for (int c = blockIdx.y; c < nch; c += gridDim.y) {
    if (PHI72) {
      // one thread per (row, column): the element's 24 words, then the virtual slots of this slot block
      const int r = tid >> 5, j = tid & 31;
      bool ok;
      const size_t col = frag_column(c, j, Lp, Wp, ok);
      uint64_t ev[TF_S];
#pragma unroll
      for (int i = 0; i < TF_S; i++) ev[i] = 0;
      if (r0 + r < kappa && ok) {
        uint64_t e[24];
        // (three calls, not a loop: the compiler keeps a loop rolled and e[] in scratch)
        seed_block8<KIND>(g, (size_t)(r0 + r), col0 + col, 0, e);
        seed_block8<KIND>(g, (size_t)(r0 + r), col0 + col, 1, e + 8);
        seed_block8<KIND>(g, (size_t)(r0 + r), col0 + col, 2, e + 16);
        if (sb == 0)
          phi72_evals<0>(e, ev);
        else if (sb == 1)
          phi72_evals<1>(e, ev);
        else
          phi72_evals<2>(e, ev);
      }
#pragma unroll
      for (int i = 0; i < TF_S; i++) tile[(r * TF_S + i) * TF_J + j] = ev[i];
    } else {
      // 8 rows x 32 columns x 2 generator blocks = two passes of 256
#pragma unroll 1
      for (int it = 0; it < 2; it++) {
        const int p = it * 256 + tid;
        const int r = p >> 6, j = (p >> 1) & 31, hb = p & 1;
        bool ok;
        const size_t col = frag_column(c, j, Lp, Wp, ok);
        uint64_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = 0;
        if (r0 + r < kappa && ok) seed_block8<KIND>(g, (size_t)(r0 + r), col0 + col, 2 * sb + hb, w);
#pragma unroll
        for (int i = 0; i < 8; i++) tile[(r * TF_S + 8 * hb + i) * TF_J + j] = w[i];
      }
    }
    __syncthreads();
    if (emit) {
      const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(tile + (er * TF_S + esl) * TF_J + 16 * eh);
      uint64_t x[16];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const ulonglong2 t = src[q];
        x[2 * q] = t.x;
        x[2 * q + 1] = t.y;
      }
      uint64_t lo = 0, hi = 0;
#pragma unroll
      for (int q = 0; q < 16; q++) {
        lo += (uint32_t)x[q];
        hi += x[q] >> 32;
        x[q] = d8(x[q]);
      }
      if (c >= ctop)  // uniform
        tlo += lo, thi += hi;
      else
        flo += lo, fhi += hi;
      uint4 u[8];
      d8_transpose16(x, u);
      const size_t s = op_slot((size_t)sb * TF_S + esl, qd);
      uint4 *out = Af + (size_t)(erow >> 5) * tile_u4 + ((s * nch + c) * 8) * 64 + (erow & 31) + 32 * eh;
#pragma unroll
      for (int b = 0; b < 8; b++) out[b * 64] = u[b];
    }
    __syncthreads();  // the tile is free for the next chunk
  }
  if (emit) {
    // both halves' threads of a (row, slot) hold a part of its sums: [walker][class][half]
    const size_t m = (size_t)kappa * dv, t = (size_t)erow * dv + sb * TF_S + esl;
    uint64_t *p = part + ((size_t)blockIdx.y * 4 + eh) * m + t;
    p[0] = gl::add(gl::canon(flo), gl::mul_pow2(fhi, 32));
    p[2 * m] = gl::add(gl::canon(tlo), gl::mul_pow2(thi, 32));
  }
}

// kr from the walkers' sums: part [gy][class][half][kappa dv]. three: the geometry
// has a top region, and kr holds the tables over every column, below the top limb
// and over the top-limb columns, m = kappa dv apart (ajtai_rowsums)
__global__ void k_seed_kr(const uint64_t *part, int gy, size_t m, int three, uint64_t *kr) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= m) return;
  uint64_t f = 0, tp = 0;
  for (int y = 0; y < gy; y++) {
    const uint64_t *p = part + (size_t)y * 4 * m + t;
    f = gl::add(f, gl::add(p[0], p[m]));
    tp = gl::add(tp, gl::add(p[2 * m], p[3 * m]));
  }
  const uint64_t all = gl::mul(FOFF, gl::add(f, tp));
  kr[t] = all;
  if (three) {
    const uint64_t top = gl::mul(FOFF, tp);
    kr[2 * m + t] = top;
    kr[m + t] = gl::sub(all, top);
  }
}

// chunk walkers of the writer: enough blocks at every degree, and a scratch whose
// size depends on kappa alone (at most 4 kappa 2^16 words)
static int seed_walkers(int dv, int nch) {
  const int want = 65536 / dv;
  return nch < want ? nch : want;
}
size_t seeded_frag_scratch_elems(size_t kappa, int d, const FragGeom &g) {
  const int dv = mfma_dim(d);
  return (size_t)seed_walkers(dv, g.nch) * 4 * kappa * dv;
}

hipError_t seeded_to_frag(const SeedGen &sg, size_t kappa, size_t col0, const FragGeom &g, uint4 *Af, uint64_t *kr,
                          uint64_t *part, hipStream_t st) {
  const int d = sg.d, dv = mfma_dim(d);
  if ((d != 24 && d % TF_S) || kappa < 1 || mfma_ktiles(kappa) > LF_MAX_KTILES || g.nch < 1)
    return hipErrorInvalidValue;
  const int gy = seed_walkers(dv, g.nch), qd = g.qperm ? d / 4 : 0;
  const int ctop = g.ptop ? g.ptop / 2 : g.nch;
  const dim3 grid((dv + TF_S - 1) / TF_S, gy, (unsigned)((kappa + TF_R - 1) / TF_R));
  const size_t tile_u4 = frag_elems(g, d);
#define LF_SF(KIND, PH)                                                                                          \
  hipLaunchKernelGGL((k_seed_frag<KIND, PH>), grid, dim3(256), 0, st, sg, (int)kappa, col0, dv, g.nch, g.Lp, g.Wp, \
                     Af, tile_u4, qd, ctop, part)
  if (sg.kind == LF_AJTAI_SEED_POSEIDON2) {
    if (d == 24)
      LF_SF(LF_AJTAI_SEED_POSEIDON2, true);
    else
      LF_SF(LF_AJTAI_SEED_POSEIDON2, false);
  } else if (sg.kind == LF_AJTAI_SEED_SPLITMIX) {
    if (d == 24)
      LF_SF(LF_AJTAI_SEED_SPLITMIX, true);
    else
      LF_SF(LF_AJTAI_SEED_SPLITMIX, false);
  } else {
    return hipErrorInvalidValue;
  }
#undef LF_SF
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t m = kappa * (size_t)dv;
  hipLaunchKernelGGL(k_seed_kr, dim3(blocks(m, 256)), dim3(256), 0, st, part, gy, m, g.Lp > 1 ? 1 : 0, kr);
  return hipGetLastError();
}

// ---------------------------------------------------------------- the plain window
// out [nrows][ncols][d] <- rows row0 .., columns col0 .. of the seeded matrix; thread per generator block
template <int KIND>
__global__ void __launch_bounds__(256) k_seed_expand(SeedGen g, size_t row0, size_t col0, size_t ncols, size_t n,
                                                     uint64_t *out) {
  const int nb = g.d >> 3;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
    const size_t rc = t / nb, row = rc / ncols, col = rc - row * ncols;
    const int j = (int)(t - rc * nb);
    uint64_t w[8];
    seed_block8<KIND>(g, row0 + row, col0 + col, j, w);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(out + rc * g.d + 8 * j);
#pragma unroll
    for (int i = 0; i < 4; i++) dst[i] = make_ulonglong2(w[2 * i], w[2 * i + 1]);
  }
}

hipError_t seeded_expand(const SeedGen &sg, size_t row0, size_t nrows, size_t col0, size_t ncols, uint64_t *out,
                         hipStream_t st) {
  if (sg.d < 8 || sg.d % 8) return hipErrorInvalidValue;
  const size_t n = nrows * ncols * (size_t)(sg.d >> 3);
  if (n == 0) return hipSuccess;
  const dim3 grid(grid_cap((n + 255) / 256));
  if (sg.kind == LF_AJTAI_SEED_POSEIDON2)
    hipLaunchKernelGGL((k_seed_expand<LF_AJTAI_SEED_POSEIDON2>), grid, dim3(256), 0, st, sg, row0, col0, ncols, n, out);
  else if (sg.kind == LF_AJTAI_SEED_SPLITMIX)
    hipLaunchKernelGGL((k_seed_expand<LF_AJTAI_SEED_SPLITMIX>), grid, dim3(256), 0, st, sg, row0, col0, ncols, n, out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace lfk
