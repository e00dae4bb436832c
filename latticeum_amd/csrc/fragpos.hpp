// fragpos.hpp -- where a 16-column operand unit sits in the contraction order, and
// the compacted (step, row) list of the contraction's top-limb class
// (ajtai_mfma.hip). Plain integer code that also compiles for the host alone
// (tests/test_frag_order.py runs it under the address and UB sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LF_HD __host__ __device__ __forceinline__
#else
#define LF_HD inline
#endif

namespace lfk {

// Unit (G, l) = limb l of the groups 16G .. 16G + 15 (column g Lp + l); nG units
// of 16 groups. Position p is half p & 1 of chunk p >> 1. Lp == 1: p = G. Lp > 1:
// the limbs below the top one keep the group-major order, p = G (Lp - 1) + l, and
// the top limbs (l = Lp - 1) follow from the first chunk boundary on, p = ptop + G:
// a chunk of the top region holds nothing but top limbs, whose digit planes are
// mostly zero (DeadUnits), so the contraction can treat those chunks as a class
// of their own. The one or two positions that hold no unit (the end of either
// region when its unit count is odd) are padding: they map to group nG, which
// is past Wp, so A is zero there.
LF_HD size_t frag_groups(size_t Wp) { return (Wp + 15) / 16; }
// the first top position (even), or 0 when there is no top region
LF_HD size_t frag_ptop(size_t nG, int Lp) { return Lp > 1 ? 2 * ((nG * (size_t)(Lp - 1) + 1) / 2) : 0; }
// positions in all, padding included: twice the chunk count
LF_HD size_t frag_npos(size_t nG, int Lp) { return frag_ptop(nG, Lp) + 2 * ((nG + 1) / 2); }
LF_HD size_t frag_pos(size_t G, int l, int Lp, size_t ptop) {
  return Lp == 1 ? G : l < Lp - 1 ? G * (size_t)(Lp - 1) + l : ptop + G;
}
// the inverse; a padding position gives G = nG
LF_HD void frag_unit(size_t p, int Lp, size_t ptop, size_t &G, int &l) {
  if (Lp == 1) {
    G = p, l = 0;
  } else if (p >= ptop) {
    G = p - ptop, l = Lp - 1;
  } else {
    G = p / (size_t)(Lp - 1), l = (int)(p % (size_t)(Lp - 1));
  }
}

// The top class's tiles: the operand rows with a live top-limb unit, over all the
// steps of a launch, packed 32 to a tile in (step, row) order. live[s] bit r: row r
// of step s is live. An entry is (step << 8) | row; the last tile is padded with
// entry (0, 0), a valid row that the consumer's counts exclude. tbl[0] = entries,
// tbl[1 ..] = the entries; returns the entry count (<= 32 nsteps).
constexpr int TOP_TBL_WORDS = 1 + 32 * 8;  // LF_MAX_STEPS = 8
LF_HD int top_compact(const uint32_t *live, int nsteps, int nvec, uint32_t *tbl) {
  int n = 0;
  for (int s = 0; s < nsteps; s++)
    for (int r = 0; r < nvec && r < 32; r++)
      if ((live[s] >> r) & 1u) tbl[1 + n++] = ((uint32_t)s << 8) | (uint32_t)r;
  for (int i = n; i < (n + 31) / 32 * 32; i++) tbl[1 + i] = 0;
  tbl[0] = (uint32_t)n;
  return n;
}
// an entry's step and row, clamped: never an address out of the launch's buffers
LF_HD int top_step(uint32_t e, int nsteps) { return (int)(e >> 8) < nsteps ? (int)(e >> 8) : nsteps - 1; }
LF_HD int top_row(uint32_t e) { return (int)(e & 31u); }
// entries of tile t
LF_HD int top_tile_entries(uint32_t n, int t, int nsteps) {
  const int m = (int)(n < 32u * (uint32_t)nsteps ? n : 32u * (uint32_t)nsteps) - 32 * t;
  return m < 0 ? 0 : m > 32 ? 32 : m;
}

}  // namespace lfk
