// planes_witness.hpp -- the packed digit planes (digitpack.hpp, the four public formats) from a
// witness's f_coeff and back: which words a thread of planes_witness.hip's kernels owns, the
// value sum_k 2^k digit_k a reader's digits add up to, and the test that a packer wrote the
// bytes. Every index and every digit comes from digitpack.hpp. Plain integer code that also
// compiles for the host alone (tests/test_planes_witness_host.py runs it under the address
// and UB sanitizers).
//
// Canonical planes are a fixed point: pack(value(planes)) == planes byte for byte. A packer
// writes the digits sign(x) bit_k(|x|) of one number |x| < 2^K, so per format:
//   sm16 halves: magnitude bits K .. 14 are zero, and the half is not 0x8000 (a negative zero);
//   mask24: bits 24 .. 31 of both words are zero, and a coefficient's sign bit is set on none of
//           its planes or on exactly the planes whose digit is nonzero;
//   sm8: a quad's sign nibble is the same on all K planes, and a set sign of quarter b has a
//        plane with digit bit b set.
#pragma once
#include "digitpack.hpp"

namespace lfk {

// ---------------------------------------------------------------- sm16 halves (d = 16 .. 512, 1024)
// sum_(k < K) 2^k sm16_digit(half, k): the low K magnitude bits under the sign
LF_HD int32_t sm16_value(uint32_t half, int K) {
  const int32_t m = (int32_t)(half & ((1u << K) - 1u));
  return (half & SM16_SIGN) ? -m : m;
}
LF_HD bool sm16_canonical(uint32_t half, int K) {
  half &= 0xFFFFu;
  return ((half & SM16_MAG) >> K) == 0 && half != SM16_SIGN;
}
// A unit is four consecutive words of one element (one 16-byte access): their low halves are
// the coefficients lo .. lo + 3 of element e, their high halves lo + hoff .. lo + hoff + 3
// (two 32-byte runs of f_coeff). Neighbouring units are neighbouring words.
struct Sm16Unit {
  size_t e, word;
  int lo, hoff;
};
LF_HD size_t sm16_elem_words(int d) { return d == 1024 ? SM1024_WORDS : smp2_words(d); }
LF_HD size_t sm16_units(int d, size_t N) { return N * sm16_elem_words(d) / 4; }
LF_HD Sm16Unit sm16_unit(int d, size_t u) {
  const size_t wpe = sm16_elem_words(d), e = 4 * u / wpe;
  const int j = (int)(4 * u % wpe);
  if (d == 1024) return {e, sm1024_word(e, j >> 5, j & 31), (j & 31) + 64 * (j >> 5), 32};
  return {e, smp2_word(e, d, j), j, d / 2};
}

// ---------------------------------------------------------------- mask24 (d = 24)
// The pack kernel's block takes PK24_ELEMS consecutive elements. Their PK24_ELEMS 24 words go
// through an LDS tile of 16-bit entries (sm16 halves on the way in, the values on the way
// back), so that both the f_coeff side (thread t: words t, t + PK24_ELEMS, ..) and the plane
// side (thread t: element t's K masks, plane by plane) are runs over neighbouring lanes. An
// element's 24 entries are 12 u32 (digitpack.hpp's sm24 word: entries 2 p and 2 p + 1) and
// one u32 of padding: an odd word stride, so the element-per-thread reads hit 32 banks.
constexpr int PK24_ELEMS = 256, PK24_STRIDE = 26;  // entries of the tile per element
LF_HD int pk24_slot(int el, int i) { return el * PK24_STRIDE + i; }
LF_HD int pk24_word(int el, int p) { return el * (PK24_STRIDE / 2) + p; }
// plane k of an element from its 12 sm24 words
LF_HD uint64_t mask24_make(const uint32_t *w12, int k) {
  uint32_t nz = 0, ng = 0;
#pragma unroll
  for (int i = 0; i < 24; i++) mask24_put(w12[i >> 1] >> (16 * (i & 1)), k, i, nz, ng);
  return nz | (uint64_t)ng << 32;
}
// an element's planes, one at a time: the values and what the canonical test needs
struct Mask24Acc {
  int32_t x[24];
  uint32_t diff, ng_any, high;
  LF_HD void init() {
#pragma unroll
    for (int i = 0; i < 24; i++) x[i] = 0;
    diff = ng_any = high = 0;
  }
  LF_HD void plane(uint64_t m, int k) {
    const uint32_t nz = (uint32_t)m, ng = (uint32_t)(m >> 32);
#pragma unroll
    for (int i = 0; i < 24; i++) x[i] += mask24_digit(nz, ng, i) * (1 << k);
    diff |= nz ^ ng;  // planes where the sign bit and the digit bit differ
    ng_any |= ng;
    high |= (nz | ng) & 0xFF000000u;
  }
  LF_HD bool canonical() const { return !high && !(diff & ng_any); }
};

// ---------------------------------------------------------------- sm8 (d = 4096)
// A unit is the word (r, j4) of an element's planes (k_pack_sm8's thread): K u32, one per
// plane, each the bytes of the quads a = r + 32 (4 j4 + jj), jj < 4; 16 coefficients.
LF_HD size_t sm8_units(size_t N) { return N * SM8_PLANE_WORDS; }
LF_HD size_t sm8_unit_elem(size_t u) { return u / SM8_PLANE_WORDS; }
LF_HD int sm8_unit_r(size_t u) { return (int)((u >> 3) & 31); }
LF_HD int sm8_unit_j4(size_t u) { return (int)(u & 7); }
LF_HD int sm8_unit_coeff(int r, int j4, int jj, int b) { return r + 32 * (4 * j4 + jj) + 1024 * b; }
struct Sm8Acc {
  int32_t x[16];  // [jj][b]
  uint32_t s0, sdiff, nz_any;
  LF_HD void init() {
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = 0;
    s0 = sdiff = nz_any = 0;
  }
  LF_HD void plane(uint32_t w, int k) {
#pragma unroll
    for (int jj = 0; jj < 4; jj++)
#pragma unroll
      for (int b = 0; b < 4; b++) x[4 * jj + b] += sm8_digit((w >> (8 * jj)) & 0xFFu, b) * (1 << k);
    if (k == 0) s0 = w & 0xF0F0F0F0u;
    sdiff |= (w & 0xF0F0F0F0u) ^ s0;
    nz_any |= w & 0x0F0F0F0Fu;
  }
  LF_HD bool canonical() const { return !sdiff && !((s0 >> 4) & ~nz_any); }
};

}  // namespace lfk
