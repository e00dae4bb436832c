// util.hip -- synthetic inputs, the cross-rank reduction and the RCCL limb transport.
#include "kernels.hpp"
#include "launch.hpp"

namespace lfk {

using gl::Acc;

// ============================================================ synthetic inputs / reductions
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// element i = SplitMix64(counter i) re-mixed until < p (oracle lfo_fill_uniform)
__global__ void k_fill_uniform(uint64_t *out, size_t n, uint64_t seed) {
  const uint64_t G = 0x9e3779b97f4a7c15ull;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint64_t x = mix64(seed + (uint64_t)(i + 1) * G);
    while (x >= gl::P) x = mix64(x + G);
    out[i] = x;
  }
}

hipError_t fill_uniform(uint64_t *out, size_t n, uint64_t seed, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fill_uniform, dim3(grid_cap(blocks(n, 256))), dim3(256), 0, st, out, n, seed);
  return hipGetLastError();
}

// out[c] = sum_r in[r*len + c] mod p  (cross-rank accumulator reduce)
__global__ void k_modp_sum(const uint64_t *in, int nparts, size_t len, uint64_t *out) {
  size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (c >= len) return;
  Acc a;
  gl::acc_zero(a);
  for (int r = 0; r < nparts; r++) gl::acc_add(a, gl::canon(in[(size_t)r * len + c]));
  out[c] = gl::acc_reduce(a);
}

hipError_t modp_sum(const uint64_t *in, int nparts, size_t len, uint64_t *out, hipStream_t st) {
  if (len == 0) return hipSuccess;
  hipLaunchKernelGGL(k_modp_sum, dim3(blocks(len, 256)), dim3(256), 0, st, in, nparts, len, out);
  return hipGetLastError();
}

// ============================================================ RCCL limb transport
// RCCL sums u64 mod 2^64, not mod p: ship 32-bit limbs (sums of <= 2^8 ranks
// stay < 2^40) and fold the limb sums back into the field afterwards.
__global__ void k_limb_split(const uint64_t *x, size_t n, uint64_t *lo, uint64_t *hi) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t v = x[i];
  lo[i] = v & 0xFFFFFFFFull;
  hi[i] = v >> 32;
}
__global__ void k_limb_join(const uint64_t *lo, const uint64_t *hi, size_t n, uint64_t *out) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t h = hi[i], wl = h << 32, wh = h >> 32;  // h * 2^32 as 128 bits
  uint64_t s = wl + lo[i];
  wh += s < wl ? 1 : 0;
  out[i] = gl::canon(gl::reduce128(s, wh));
}

hipError_t limb_split(const uint64_t *x, size_t n, uint64_t *lo, uint64_t *hi, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_limb_split, dim3(blocks(n, 256)), dim3(256), 0, st, x, n, lo, hi);
  return hipGetLastError();
}
hipError_t limb_join(const uint64_t *lo, const uint64_t *hi, size_t n, uint64_t *out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_limb_join, dim3(blocks(n, 256)), dim3(256), 0, st, lo, hi, n, out);
  return hipGetLastError();
}

}  // namespace lfk
