// ajtai_seed.hpp -- the Ajtai matrix as a function of a seed (include/lf.h,
// lf_ajtai_create_seeded): what the host expansion (transcript.cpp) and the device
// generators (ajtai_seeded.hip) share -- the domain tag, the generator's
// parameters, the argument checks and the SplitMix word.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lf.h"
#include "gl.hpp"

namespace lfk {

constexpr uint64_t AJTAI_SEED_TAG = 0x4C46414A54414931ull;  // "LFAJTAI1"

// A[row][col][.] of the kappa x ncols_total matrix of degree-d elements
struct SeedGen {
  uint64_t seed[4];
  int kind;  // LF_AJTAI_SEED_*
  int d;
  size_t ncols_total;
};

// LF_AJTAI_SEED_POSEIDON2: the permutation's input for block j (words 8 j .. 8 j + 7) of element (row, col)
LF_HD void seed_p2_state(const SeedGen &g, size_t row, size_t col, int j, uint64_t *s) {
  s[0] = g.seed[0], s[1] = g.seed[1], s[2] = g.seed[2], s[3] = g.seed[3];
  s[4] = AJTAI_SEED_TAG, s[5] = (uint64_t)g.d, s[6] = row, s[7] = col, s[8] = (uint64_t)j;
  for (int i = 9; i < 16; i++) s[i] = 0;
}

// LF_AJTAI_SEED_SPLITMIX: word i of fill_uniform(., seed) (util.hip k_fill_uniform, oracle lfo_fill_uniform)
LF_HD uint64_t seed_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
LF_HD uint64_t seed_splitmix_word(uint64_t seed, uint64_t i) {
  const uint64_t G = 0x9e3779b97f4a7c15ull;
  uint64_t x = seed_mix64(seed + (i + 1) * G);
  while (x >= gl::P) x = seed_mix64(x + G);
  return x;
}

// the refusals every seeded entry shares: LF_OK, or the status and what was wrong
inline int seed_check(const uint64_t *seed, int kind, size_t kappa, size_t ncols_total, int d, size_t col0,
                      size_t ncols, const char **why) {
  *why = "";
  if (!seed || !kappa || !ncols || !ncols_total) return *why = "null seed or a zero size", LF_ERR_INVALID_ARG;
  if (kind != LF_AJTAI_SEED_POSEIDON2 && kind != LF_AJTAI_SEED_SPLITMIX)
    return *why = "kind must be LF_AJTAI_SEED_POSEIDON2 or LF_AJTAI_SEED_SPLITMIX", LF_ERR_INVALID_ARG;
  if (!lf_ring_supported(d)) return *why = "unsupported ring degree", LF_ERR_UNSUPPORTED_RING;
  if (col0 > ncols_total || ncols > ncols_total - col0)
    return *why = "col0 + ncols exceeds ncols_total", LF_ERR_INVALID_ARG;
  if (kind == LF_AJTAI_SEED_POSEIDON2) {
    for (int i = 0; i < 4; i++)
      if (seed[i] >= gl::P) return *why = "seed words must be canonical (< p)", LF_ERR_INVALID_ARG;
    if ((uint64_t)kappa > (1ull << 32) || (uint64_t)ncols_total > (1ull << 32))
      return *why = "kappa and ncols_total must be at most 2^32", LF_ERR_INVALID_ARG;
  } else {
    if (seed[1] || seed[2] || seed[3]) return *why = "SplitMix kind: seed[1..3] must be 0", LF_ERR_INVALID_ARG;
  }
  // the matrix's bytes fit 64 bits (so do every window's, and the SplitMix word index)
  unsigned long long n;
  if (__builtin_umulll_overflow(kappa, ncols_total, &n) || __builtin_umulll_overflow(n, (unsigned long long)d, &n) ||
      __builtin_umulll_overflow(n, 8ull, &n))
    return *why = "kappa ncols_total d 8 bytes overflow 64 bits", LF_ERR_INVALID_ARG;
  return LF_OK;
}

}  // namespace lfk
