// digitpack.hpp -- the packed digit formats of the b_small = 2 decompositions: the
// one commented home of each layout. Writers (the pack kernels, from_w_ccs), readers
// (the fused decompositions, the coefficient-form folds), the expanders
// (lf_dev_expand_planes) and the host's buffer sizing all take the sizes, indices,
// encode and decode from here. Four of the formats are public: callers keep them in
// lf_fold_step_bufs.planes between steps (include/lf.h). Plain integer code that also
// compiles for the host alone (tests/test_digit_pack.py runs it under the address and
// UB sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fragpos.hpp"  // LF_HD

namespace lfk {

// ---------------------------------------------------------------- 16-bit sign|magnitude word
// A coefficient x with |x| < 2^K, K <= 15: bits 0..14 = |x|, bit 15 = 1 when x < 0.
// With b_small = 2 the balanced digit k of x is sign(x) bit_k(|x|), so every digit
// plane is read straight off the word.
constexpr uint32_t SM16_MAG = 0x7FFFu, SM16_SIGN = 0x8000u;
LF_HD uint32_t sign_mag16(int64_t x) {
  const uint64_t m = x < 0 ? (uint64_t)(-x) : (uint64_t)x;
  return (uint32_t)(m & SM16_MAG) | (x < 0 ? SM16_SIGN : 0u);
}
// |x| >= 2^K: the K planes do not hold x (the decomposition's range error)
LF_HD bool sm16_overflow(int64_t x, int K) {
  const uint64_t m = x < 0 ? (uint64_t)(-x) : (uint64_t)x;
  return (m >> K) != 0;
}
// digit k in {-1, 0, 1} of a word (bits above 15 are ignored)
LF_HD int sm16_digit(uint32_t w, int k) {
  const int bit = (int)((w >> k) & 1u);
  return (w & SM16_SIGN) ? -bit : bit;
}

// ---------------------------------------------------------------- d = 1024: sm16 words (public)
// 512 u32 (2 KiB) per ring element, all K planes in one. Word (q, r), q < 16,
// r < 32, of element col sits at (col 16 + q) 32 + r and holds
// sm(x[r + 64 q]) | sm(x[r + 64 q + 32]) << 16: coefficient j is half (j >> 5) & 1
// of word (q = j >> 6, r = j & 31). A half-wave lane r reads its 16 words 128 B apart.
constexpr size_t SM1024_WORDS = 512;
LF_HD size_t sm1024_word(size_t col, int q, int r) { return (col * 16 + (size_t)q) * 32 + (size_t)r; }
LF_HD size_t sm1024_word_of(size_t col, int j) { return sm1024_word(col, j >> 6, j & 31); }
LF_HD int sm1024_half_of(int j) { return (j >> 5) & 1; }
LF_HD int sm1024_digit(const uint32_t *words, size_t col, int j, int k) {
  return sm16_digit(words[sm1024_word_of(col, j)] >> (16 * sm1024_half_of(j)), k);
}

// ---------------------------------------------------------------- d = 2^k, 16 <= d <= 512: sm16 words (public)
// d / 2 u32 per ring element, all K planes in one; one format for the six degrees.
// Word j < d / 2 of element e sits at e d / 2 + j and holds
// sm(x[j]) | sm(x[j + d / 2]) << 16: coefficient i is half i / (d / 2) of word
// i mod (d / 2). A thread of the fused decomposition (decompose_pow2.hip) that owns
// the coefficients i = t, t + T, .. of its element owns both halves of each of its
// words, and neighbouring threads write neighbouring words.
LF_HD bool smp2_degree(int d) { return d >= 16 && d <= 512 && (d & (d - 1)) == 0; }
LF_HD size_t smp2_words(int d) { return (size_t)d / 2; }  // u32 per element
LF_HD size_t smp2_word(size_t e, int d, int j) { return e * smp2_words(d) + (size_t)j; }
LF_HD size_t smp2_word_of(size_t e, int d, int i) { return smp2_word(e, d, i & (d / 2 - 1)); }
LF_HD int smp2_half_of(int d, int i) { return i >= d / 2 ? 1 : 0; }
LF_HD uint32_t smp2_make(int64_t lo, int64_t hi) { return sign_mag16(lo) | sign_mag16(hi) << 16; }
LF_HD int smp2_digit(const uint32_t *words, size_t e, int d, int i, int k) {
  return sm16_digit(words[smp2_word_of(e, d, i)] >> (16 * smp2_half_of(d, i)), k);
}

// ---------------------------------------------------------------- d = 24: sm16 words (scratch)
// 12 u32 per element: word p of element e at e 12 + p = sm(x[2p]) | sm(x[2p + 1]) << 16.
constexpr size_t SM24_WORDS = 12;
LF_HD size_t sm24_word(size_t e, int p) { return e * SM24_WORDS + (size_t)p; }
LF_HD int sm24_digit(const uint32_t *words, size_t e, int i, int k) {
  return sm16_digit(words[sm24_word(e, i >> 1)] >> (16 * (i & 1)), k);
}

// ---------------------------------------------------------------- d = 24: digit masks (public)
// [K][N] pairs of u32 (one u64 per element and plane): plane k of element e at
// k N + e; bit i of the low word = coefficient i's digit is nonzero, bit i of the
// high word = it is -1. Bits 24..31 of both are zero.
LF_HD size_t mask24_index(int k, size_t N, size_t e) { return (size_t)k * N + e; }
LF_HD size_t mask24_elems(int K, size_t N) { return (size_t)K * N; }  // u64 (uint2) per side
LF_HD int mask24_digit(uint32_t nz, uint32_t ng, int i) { return (nz >> i & 1u) ? ((ng >> i & 1u) ? -1 : 1) : 0; }
// the two mask bits of coefficient i from its sm16 word, at plane k
LF_HD void mask24_put(uint32_t w, int k, int i, uint32_t &nz, uint32_t &ng) {
  const uint32_t bit = (w >> k) & 1u;
  nz |= bit << i;
  ng |= (bit & (w >> 15)) << i;  // bit is 0 or 1: bits above the sign drop out
}

// ---------------------------------------------------------------- d = 4096: Morton words (scratch)
// 1024 u64 per element: word a < 1024 of element e at e 1024 + a holds the four
// coefficients a + 1024 b, b < 4: magnitude bit t of quarter b at bit 4 t + b
// (t < 15), the sign of quarter b at bit 60 + b. Plane k of all four is the nibble at
// 4 k; the signs are the top nibble.
constexpr size_t SM4_WORDS = 1024;
LF_HD size_t sm4_word(size_t e, int a) { return e * SM4_WORDS + (size_t)a; }
// bit t of a 16-bit value -> bit 4 t
LF_HD uint64_t spread4(uint32_t v) {
  uint64_t x = v & 0xFFFFu;
  x = (x | (x << 24)) & 0x000000FF000000FFull;
  x = (x | (x << 12)) & 0x000F000F000F000Full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}
LF_HD uint64_t sm4_put(uint32_t sm16, int b) { return spread4(sm16) << b; }
LF_HD uint32_t sm4_nibble(uint64_t w, int k) { return (uint32_t)(w >> (4 * k)) & 15u; }
LF_HD uint32_t sm4_signs(uint64_t w) { return (uint32_t)(w >> 60); }
LF_HD int sm4_digit(uint64_t w, int b, int k) {
  const int bit = (int)((sm4_nibble(w, k) >> b) & 1u);
  return ((sm4_signs(w) >> b) & 1u) ? -bit : bit;
}

// ---------------------------------------------------------------- d = 4096: digit bytes (public)
// K 1024 bytes (K 256 u32) per element: one byte per coefficient quad and plane.
// Byte ((e K + k) 32 + r) 32 + j, r < 32, j < 32, holds the quad a = r + 32 j (the
// coefficients a + 1024 b): bit b = digit k of coefficient a + 1024 b is nonzero,
// bit 4 + b = that coefficient is negative (set whether or not the digit is zero).
constexpr size_t SM8_PLANE_WORDS = 256;                                 // u32 of one plane of an element
LF_HD size_t sm8_words(int K) { return (size_t)K * SM8_PLANE_WORDS; }  // u32 per element
LF_HD size_t sm8_byte(size_t e, int K, int k, int r, int j) {
  return (((e * (size_t)K + (size_t)k) * 32 + (size_t)r) * 32) + (size_t)j;
}
// the u32 that holds bytes j = 4 j4 .. 4 j4 + 3 of lane r (j4 < 8): sm8_byte(e, K, k, r, 4 j4) / 4
LF_HD size_t sm8_word(size_t e, int K, int k, int r, int j4) {
  return ((e * (size_t)K + (size_t)k) * 32 + (size_t)r) * 8 + (size_t)j4;
}
LF_HD size_t sm8_byte_of(size_t e, int K, int k, int a) { return sm8_byte(e, K, k, a & 31, a >> 5); }
LF_HD uint32_t sm8_make(uint32_t nibble, uint32_t signs) { return (nibble & 15u) | (signs << 4); }
LF_HD int sm8_digit(uint32_t byte, int b) {
  const int bit = (int)((byte >> b) & 1u);
  return ((byte >> (4 + b)) & 1u) ? -bit : bit;
}

// ---------------------------------------------------------------- launches that start from the public planes
// A fused decomposition whose every side (nside = 1 or 2) is already packed -- one bit per
// side in FusedSides::prepacked -- reads the caller's planes and no coefficients
// (lf_dev_commit_planes). All K planes of side s are then operand rows of their own, plane 0
// first: row s K + k, so plane 0's row is the one before plane 1's and 2 K <= 30 rows are used.
LF_HD bool planes_all_packed(int prepacked, int nside) {
  return nside >= 1 && nside <= 2 && prepacked == (1 << nside) - 1;
}
LF_HD int planes_row(int side, int K, int k) { return side * K + k; }

}  // namespace lfk
