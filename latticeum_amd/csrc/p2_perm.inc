// p2_perm.inc -- the width-16 Poseidon2 permutation's device code: the round
// constants and the round loop. Included inside a namespace by each kernel file
// that permutes (poseidon2.hip in lfk, ajtai_seeded.hip in lfk::seeded), so each
// has its own copy of the __constant__ tables and no symbol is defined twice.
// zkvm/src/poseidon2.rs:100-173 (+ Plonky3 add_rc_and_sbox_generic, matmul_internal)
#include "p2_consts.inc"
__constant__ uint64_t P2_EXT_INIT[64] = LF_P2_EXT_INIT;
__constant__ uint64_t P2_EXT_TERM[64] = LF_P2_EXT_TERM;
__constant__ uint64_t P2_INTERNAL[22] = LF_P2_INTERNAL;
__constant__ uint64_t P2_DIAG_M1[16] = LF_P2_DIAG_M1;

__device__ __forceinline__ uint64_t sbox7(uint64_t x) {
  uint64_t x2 = gl::mul(x, x), x4 = gl::mul(x2, x2);
  return gl::mul(gl::mul(x4, x2), x);
}
__device__ __forceinline__ void mds16(uint64_t *s) {  // poseidon2.rs:243-268
#pragma unroll
  for (int c = 0; c < 16; c += 4) {
    uint64_t x0 = s[c], x1 = s[c + 1], x2 = s[c + 2], x3 = s[c + 3];
    uint64_t t = gl::add(gl::add(x0, x1), gl::add(x2, x3));
    s[c] = gl::add(t, gl::add(x0, gl::add(x1, x1)));
    s[c + 1] = gl::add(t, gl::add(x1, gl::add(x2, x2)));
    s[c + 2] = gl::add(t, gl::add(x2, gl::add(x3, x3)));
    s[c + 3] = gl::add(t, gl::add(x3, gl::add(x0, x0)));
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint64_t sum = gl::add(gl::add(s[k], s[4 + k]), gl::add(s[8 + k], s[12 + k]));
#pragma unroll
    for (int j = k; j < 16; j += 4) s[j] = gl::add(s[j], sum);
  }
}
// The permutation of the 16 canonical words s[], in place: the initial MDS, then the
// first `rounds` of the 4 + 22 + 4 rounds (30: all of it). A macro, so that
// k_p2_permute keeps the exact code it had when the loop stood in its body (as an
// inlined function the same loop came out with operands of a multiply swapped).
// Its locals carry a p2_ prefix so that they cannot shadow the caller's names.
#define LF_P2_ROUNDS(s, rounds)                                                                                       \
  do {                                                                                                                \
    mds16(s);                                                                                                         \
    const int p2_ri_ = (rounds) < 4 ? (rounds) : 4, p2_rp_ = (rounds) - 4 < 0 ? 0 : (rounds) - 4 > 22 ? 22 : (rounds) - 4; \
    const int p2_rt_ = (rounds) - 26 < 0 ? 0 : (rounds) - 26 > 4 ? 4 : (rounds) - 26;                                 \
    _Pragma("unroll 1") for (int p2_r_ = 0; p2_r_ < p2_ri_; p2_r_++) {                                                \
      _Pragma("unroll") for (int p2_i_ = 0; p2_i_ < 16; p2_i_++) (s)[p2_i_] = sbox7(gl::add((s)[p2_i_], P2_EXT_INIT[16 * p2_r_ + p2_i_])); \
      mds16(s);                                                                                                       \
    }                                                                                                                 \
    _Pragma("unroll 1") for (int p2_r_ = 0; p2_r_ < p2_rp_; p2_r_++) {                                                \
      (s)[0] = sbox7(gl::add((s)[0], P2_INTERNAL[p2_r_]));                                                            \
      uint64_t p2_sum_ = 0;                                                                                           \
      _Pragma("unroll") for (int p2_i_ = 0; p2_i_ < 16; p2_i_++) p2_sum_ = gl::add(p2_sum_, (s)[p2_i_]);              \
      _Pragma("unroll") for (int p2_i_ = 0; p2_i_ < 16; p2_i_++) (s)[p2_i_] = gl::add(gl::mul((s)[p2_i_], P2_DIAG_M1[p2_i_]), p2_sum_); \
    }                                                                                                                 \
    _Pragma("unroll 1") for (int p2_r_ = 0; p2_r_ < p2_rt_; p2_r_++) {                                                \
      _Pragma("unroll") for (int p2_i_ = 0; p2_i_ < 16; p2_i_++) (s)[p2_i_] = sbox7(gl::add((s)[p2_i_], P2_EXT_TERM[16 * p2_r_ + p2_i_])); \
      mds16(s);                                                                                                       \
    }                                                                                                                 \
  } while (0)
