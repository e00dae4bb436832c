// planes_witness.hip -- the packed digit planes (lf_fold_step_bufs.planes) from a witness's
// f_coeff and back, without a step: the pack kernels of d = 24 (digit masks) and d = 16 .. 512
// (sm16 words) -- d = 1024 and d = 4096 launch kernels_n32.hip's k_pack_sm and
// kernels_n4k.hip's k_pack_sm8 as they are --, the recompose kernels planes -> f_coeff
// (sum_k 2^k digit_k, decoded as lf_dev_expand_planes decodes) and the scan that
// lf_dev_planes_check runs: the l_inf norm of those values and the lowest element that no
// packer wrote. One pass over the planes each; the thread-to-word maps, the values and the
// canonical test are planes_witness.hpp's.
#include "digits.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "planes_witness.hpp"

namespace lfk {

namespace {

// ============================================================ pack
// d = 16 .. 512: one unit (four words, eight coefficients) per thread: 2 x 32 contiguous
// bytes in, one 16-byte store out, as k_pack_sm at d = 1024
__device__ __forceinline__ uint32_t pack_half(uint64_t x, int K, bool &bad) {
  const int64_t a = signed_rep(x);
  bad |= sm16_overflow(a, K);
  return sign_mag16(a);
}
__global__ void __launch_bounds__(256) k_pack_smp2(const uint64_t *fc, int d, size_t N, int K, uint32_t *words,
                                                   int *err) {
  const size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (u >= sm16_units(d, N)) return;
  const Sm16Unit un = sm16_unit(d, u);
  const ulonglong2 *x = reinterpret_cast<const ulonglong2 *>(fc + un.e * d + un.lo);
  const ulonglong2 *y = reinterpret_cast<const ulonglong2 *>(fc + un.e * d + un.lo + un.hoff);
  const ulonglong2 a0 = x[0], a1 = x[1], c0 = y[0], c1 = y[1];
  bool bad = false;
  uint4 o;
  o.x = pack_half(a0.x, K, bad) | (pack_half(c0.x, K, bad) << 16);
  o.y = pack_half(a0.y, K, bad) | (pack_half(c0.y, K, bad) << 16);
  o.z = pack_half(a1.x, K, bad) | (pack_half(c1.x, K, bad) << 16);
  o.w = pack_half(a1.y, K, bad) | (pack_half(c1.y, K, bad) << 16);
  if (bad) raise(err, 1);
  *reinterpret_cast<uint4 *>(words + un.word) = o;
}

// d = 24: a block packs PK24_ELEMS elements through the tile of planes_witness.hpp: every
// thread brings 24 words of the block's contiguous f_coeff run in as sm16 halves, then takes
// one element and writes its K masks, plane by plane: a wave stores 64 neighbouring u64 of a plane
__global__ void __launch_bounds__(PK24_ELEMS) k_pack_mask24(const uint64_t *fc, size_t N, int K, uint64_t *planes,
                                                            int *err) {
  __shared__ uint32_t tile[PK24_ELEMS * PK24_STRIDE / 2];
  uint16_t *half = reinterpret_cast<uint16_t *>(tile);
  const int t = threadIdx.x;
  const size_t e0 = (size_t)blockIdx.x * PK24_ELEMS, n = N * 24;
  bool bad = false;
#pragma unroll 4
  for (int q = 0; q < 24; q++) {
    const int o = t + q * PK24_ELEMS;
    const size_t g = e0 * 24 + o;
    if (g < n) {
      const int64_t a = signed_rep(fc[g]);
      bad |= sm16_overflow(a, K);
      half[pk24_slot(o / 24, o % 24)] = (uint16_t)sign_mag16(a);
    }
  }
  if (bad) raise(err, 1);
  __syncthreads();
  const size_t e = e0 + t;
  if (e >= N) return;
  uint32_t w[SM24_WORDS];
#pragma unroll
  for (int p = 0; p < (int)SM24_WORDS; p++) w[p] = tile[pk24_word(t, p)];
  for (int k = 0; k < K; k++) planes[mask24_index(k, N, e)] = mask24_make(w, k);
}

// ============================================================ planes -> values, and the scan
// what a thread of the scan has seen: the largest |value|, the lowest element with a
// non-canonical entry and the lowest with a value above the bound (all-ones: none)
struct Scan {
  uint32_t mx = 0;
  unsigned long long enc = ~0ull, bnd = ~0ull;
  __device__ __forceinline__ void elem(size_t e, uint32_t m, bool canonical, uint64_t bound) {
    mx = m > mx ? m : mx;
    if (!canonical && e < enc) enc = e;
    if (bound && m > bound && e < bnd) bnd = e;
  }
  // res = {norm, lowest non-canonical element, lowest element above the bound}; every lane of the wave calls it
  __device__ __forceinline__ void flush(unsigned long long *res) {
    uint32_t m = mx;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)m, s);
      m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&res[0], (unsigned long long)m);
    if (enc != ~0ull) atomicMin(&res[1], enc);
    if (bnd != ~0ull) atomicMin(&res[2], bnd);
  }
};
__device__ __forceinline__ uint32_t abs32(int32_t v) { return (uint32_t)(v < 0 ? -v : v); }

// CHK = false: fc gets the values in canonical form; CHK = true: res gets the scan, nothing else is written
template <bool CHK>
__global__ void __launch_bounds__(256) k_planes_sm16(const uint32_t *words, int d, size_t N, int K, uint64_t *fc,
                                                     uint64_t bound, unsigned long long *res) {
  const size_t nu = sm16_units(d, N);
  Scan sc;
  for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < nu; u += (size_t)gridDim.x * blockDim.x) {
    const Sm16Unit un = sm16_unit(d, u);
    const uint4 q = *reinterpret_cast<const uint4 *>(words + un.word);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    int32_t lo[4], hi[4];
#pragma unroll
    for (int i = 0; i < 4; i++) lo[i] = sm16_value(w[i] & 0xFFFFu, K), hi[i] = sm16_value(w[i] >> 16, K);
    if constexpr (CHK) {
      bool ok = true;
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        ok = ok && sm16_canonical(w[i] & 0xFFFFu, K) && sm16_canonical(w[i] >> 16, K);
        const uint32_t a = abs32(lo[i]), b = abs32(hi[i]);
        m = a > m ? a : m;
        m = b > m ? b : m;
      }
      sc.elem(un.e, m, ok, bound);
    } else {
      ulonglong2 *ol = reinterpret_cast<ulonglong2 *>(fc + un.e * d + un.lo);
      ulonglong2 *oh = reinterpret_cast<ulonglong2 *>(fc + un.e * d + un.lo + un.hoff);
      ol[0] = make_ulonglong2(from_signed(lo[0]), from_signed(lo[1]));
      ol[1] = make_ulonglong2(from_signed(lo[2]), from_signed(lo[3]));
      oh[0] = make_ulonglong2(from_signed(hi[0]), from_signed(hi[1]));
      oh[1] = make_ulonglong2(from_signed(hi[2]), from_signed(hi[3]));
    }
  }
  if constexpr (CHK) sc.flush(res);
}

// d = 24: one element per thread, its K masks read plane by plane (a wave: 64 neighbouring u64);
// the values leave through the pack kernel's tile, as runs of the block's contiguous f_coeff
template <bool CHK>
__global__ void __launch_bounds__(PK24_ELEMS) k_planes_mask24(const uint64_t *planes, size_t N, int K, uint64_t *fc,
                                                              uint64_t bound, unsigned long long *res) {
  __shared__ uint32_t tile[CHK ? 1 : PK24_ELEMS * PK24_STRIDE / 2];
  const int t = threadIdx.x;
  const size_t e0 = (size_t)blockIdx.x * PK24_ELEMS, e = e0 + t;
  Scan sc;
  if (e < N) {
    Mask24Acc acc;
    acc.init();
    for (int k = 0; k < K; k++) acc.plane(planes[mask24_index(k, N, e)], k);
    if constexpr (CHK) {
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 24; i++) m = abs32(acc.x[i]) > m ? abs32(acc.x[i]) : m;
      sc.elem(e, m, acc.canonical(), bound);
    } else {
#pragma unroll
      for (int p = 0; p < (int)SM24_WORDS; p++)
        tile[pk24_word(t, p)] = ((uint32_t)acc.x[2 * p] & 0xFFFFu) | ((uint32_t)acc.x[2 * p + 1] << 16);
    }
  }
  if constexpr (CHK) {
    sc.flush(res);
  } else {
    __syncthreads();
    const int16_t *val = reinterpret_cast<const int16_t *>(tile);
    const size_t n = N * 24;
#pragma unroll 4
    for (int q = 0; q < 24; q++) {
      const int o = t + q * PK24_ELEMS;
      const size_t g = e0 * 24 + o;
      if (g < n) fc[g] = from_signed((int64_t)val[pk24_slot(o / 24, o % 24)]);
    }
  }
}

// d = 4096: one word (r, j4) of an element's planes per thread, K u32 4 K bytes apart
// (neighbouring threads: neighbouring words), 16 coefficients out, the mirror of k_pack_sm8's reads
template <bool CHK>
__global__ void __launch_bounds__(256) k_planes_sm8(const uint32_t *sm8, size_t N, int K, uint64_t *fc,
                                                    uint64_t bound, unsigned long long *res) {
  const size_t nu = sm8_units(N);
  Scan sc;
  for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < nu; u += (size_t)gridDim.x * blockDim.x) {
    const size_t e = sm8_unit_elem(u);
    const int r = sm8_unit_r(u), j4 = sm8_unit_j4(u);
    Sm8Acc acc;
    acc.init();
    for (int k = 0; k < K; k++) acc.plane(sm8[sm8_word(e, K, k, r, j4)], k);
    if constexpr (CHK) {
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 16; i++) m = abs32(acc.x[i]) > m ? abs32(acc.x[i]) : m;
      sc.elem(e, m, acc.canonical(), bound);
    } else {
      uint64_t *o = fc + e * 4096;
#pragma unroll
      for (int jj = 0; jj < 4; jj++)
#pragma unroll
        for (int b = 0; b < 4; b++) o[sm8_unit_coeff(r, j4, jj, b)] = from_signed(acc.x[4 * jj + b]);
    }
  }
  if constexpr (CHK) sc.flush(res);
}

bool packed_ok(int d, int K) { return K >= 1 && K <= 15 && (d == 24 || d == 1024 || d == 4096 || smp2_degree(d)); }

template <bool CHK>
hipError_t planes_launch(const uint64_t *planes, size_t N, int d, int K, uint64_t *fc, uint64_t bound, uint64_t *res,
                         hipStream_t st) {
  unsigned long long *r = reinterpret_cast<unsigned long long *>(res);
  const uint32_t *w = reinterpret_cast<const uint32_t *>(planes);
  if (d == 24)
    hipLaunchKernelGGL((k_planes_mask24<CHK>), dim3(blocks(N, PK24_ELEMS)), dim3(PK24_ELEMS), 0, st, planes, N, K, fc,
                       bound, r);
  else if (d == 4096)
    hipLaunchKernelGGL((k_planes_sm8<CHK>), dim3(grid_cap(blocks(sm8_units(N), 256))), dim3(256), 0, st, w, N, K, fc,
                       bound, r);
  else
    hipLaunchKernelGGL((k_planes_sm16<CHK>), dim3(grid_cap(blocks(sm16_units(d, N), 256))), dim3(256), 0, st, w, d, N,
                       K, fc, bound, r);
  return hipGetLastError();
}

}  // namespace

hipError_t planes_pack(const uint64_t *fc, size_t N, int d, int K, uint64_t *planes, int *err, hipStream_t st) {
  if (!packed_ok(d, K)) return hipErrorInvalidValue;
  if (!N) return hipSuccess;
  uint32_t *w = reinterpret_cast<uint32_t *>(planes);
  if (d == 1024) return pack_sm(fc, N, K, w, err, st);
  if (d == 4096) return pack_sm8(fc, N, K, w, err, st);
  if (d == 24)
    hipLaunchKernelGGL(k_pack_mask24, dim3(blocks(N, PK24_ELEMS)), dim3(PK24_ELEMS), 0, st, fc, N, K, planes, err);
  else
    hipLaunchKernelGGL(k_pack_smp2, dim3(blocks(sm16_units(d, N), 256)), dim3(256), 0, st, fc, d, N, K, w, err);
  return hipGetLastError();
}

hipError_t planes_recompose(const uint64_t *planes, size_t N, int d, int K, uint64_t *fc, hipStream_t st) {
  if (!packed_ok(d, K)) return hipErrorInvalidValue;
  if (!N) return hipSuccess;
  return planes_launch<false>(planes, N, d, K, fc, 0, nullptr, st);
}

hipError_t planes_scan(const uint64_t *planes, size_t N, int d, int K, uint64_t bound, uint64_t *res, hipStream_t st) {
  if (!packed_ok(d, K)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(res, 0, 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(res + 1, 0xFF, 16, st);
  if (e != hipSuccess || !N) return e;
  return planes_launch<true>(planes, N, d, K, nullptr, bound, res, st);
}

}  // namespace lfk
