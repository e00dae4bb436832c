// poseidon2.hip -- the width-16 Poseidon2 permutation over Goldilocks (the width-8
// one of the Merkle trees is in merkle.hip).
#include "kernels.hpp"
#include "launch.hpp"

namespace lfk {

// ============================================================ Poseidon2-16
// the constants, sbox7, mds16 and the round loop LF_P2_ROUNDS
#include "p2_perm.inc"

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
  LF_P2_ROUNDS(s, rounds);
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
