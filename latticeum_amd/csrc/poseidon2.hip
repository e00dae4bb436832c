// poseidon2.hip -- the width-16 Poseidon2 permutation over Goldilocks (the width-8
// one of the Merkle trees is in merkle.hip).
#include "kernels.hpp"
#include "launch.hpp"

namespace lfk {

// ============================================================ Poseidon2-16
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
// rounds < 30 stops after the initial MDS and that many rounds (a debug entry
// that lets the reference's round-0 vector, sages/inverse_mds.sage, pin the device)
__global__ void __launch_bounds__(256) k_p2_permute(uint64_t *states, size_t n, int rounds) {
  size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e >= n) return;
  uint64_t s[16];
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(states + e * 16);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    ulonglong2 v = src[i];
    s[2 * i] = gl::canon(v.x);
    s[2 * i + 1] = gl::canon(v.y);
  }
  mds16(s);
  const int ri = rounds < 4 ? rounds : 4, rp = rounds - 4 < 0 ? 0 : rounds - 4 > 22 ? 22 : rounds - 4;
  const int rt = rounds - 26 < 0 ? 0 : rounds - 26 > 4 ? 4 : rounds - 26;
#pragma unroll 1
  for (int r = 0; r < ri; r++) {
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = sbox7(gl::add(s[i], P2_EXT_INIT[16 * r + i]));
    mds16(s);
  }
#pragma unroll 1
  for (int r = 0; r < rp; r++) {
    s[0] = sbox7(gl::add(s[0], P2_INTERNAL[r]));
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) sum = gl::add(sum, s[i]);
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = gl::add(gl::mul(s[i], P2_DIAG_M1[i]), sum);
  }
#pragma unroll 1
  for (int r = 0; r < rt; r++) {
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = sbox7(gl::add(s[i], P2_EXT_TERM[16 * r + i]));
    mds16(s);
  }
  ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(states + e * 16);
#pragma unroll
  for (int i = 0; i < 8; i++) dst[i] = make_ulonglong2(s[2 * i], s[2 * i + 1]);
}

hipError_t p2_permute(uint64_t *states, size_t n, hipStream_t st, int rounds) {
  if (n == 0) return hipSuccess;
  if (rounds < 0 || rounds > 30) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_p2_permute, dim3(blocks(n, 256)), dim3(256), 0, st, states, n, rounds);
  return hipGetLastError();
}

}  // namespace lfk
