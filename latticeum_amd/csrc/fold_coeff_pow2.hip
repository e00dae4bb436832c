// fold_coeff_pow2.hip -- f_0 = sum_i rho_i f_i (LF/nifs/folding.rs:258-268) for X^d + 1,
// d = 16 .. 512, in coefficient form on the i8 matrix cores, from the packed digit
// planes of both sides (digitpack.hpp smp2_*) and the 2K challenges alone.
//
// The 2K folded witnesses are the balanced digit planes of the two decomposed sides,
// f_i = NTT(D_i) with D_i in {-1, 0, 1}^d (b_small = 2: the digits are sign-magnitude
// binary), i = s K + k. The NTT is a ring isomorphism, so
// f_0 = NTT(sum_i rho_i * D_i), * the negacyclic product, and
//   f0_coeff[c][e] = sum_i sum_j R_i[c][j] D_i[j][e],
//   R_i[c][j] = rho_i[c - j] (c >= j),  -rho_i[c - j + d] (c < j),
// an exact integer product of i8 operands into i32.
//
// Range. With |rho coefficient| <= 127, |f0_coeff| <= 2K d 127. What can be reached is
// less: the K digits of one coefficient x are sign(x) bit_k(|x|), all of one sign, and a
// witness coefficient is a balanced base-B digit, |x| <= B / 2 = 2^14, so at most 14 of
// its 15 planes are nonzero at once: 2 14 d 127 = 1,820,672 at d = 512, far inside i32.
// No Karatsuba split is needed (and its sum tables would not fit i8 for challenges
// beyond [-63, 63]: these tables take the full [-127, 127]). Canonicalised
// mod p the result is Witness::from_f's f_coeff itself; f_0 and w_ccs_0 follow from one
// forward transform per element (witness_pack.hip from_fcoeff).
//
// The product (foldpow2.hpp has the index arithmetic). R_i is Toeplitz: the 32 x 32 A
// tile of rows 32 t .. and columns 32 q .. depends only on t - q and is 16 bytes per lane
// at a lane-dependent byte offset of the challenge's reversed table in LDS (5 dwords,
// v_alignbyte). The B tile is 16 digits per lane: the lane reads the 16 packed words
// that hold them once per (side, q) and cuts every plane's bytes from those registers,
// so the planes are read once per row group, not once per plane. Loop order: side, q,
// plane, row tile; every product re-reads its A tile from LDS (what that leaves on the
// table: DESIGN.md section 30). d = 16 has a single 16 x 16 block per witness: one
// 32 x 32 x 32 product takes two witnesses along k and leaves rows 16 .. 31 zero.
//
// Used only when every rho_i has coefficients in [-127, 127] (k_rho_prep_pow2 checks on
// the device); otherwise the flag it raises makes these kernels return at once, and the
// step's gated fallback (the fold from the operand rows, Witness::from_f) runs instead,
// with no host synchronisation.
#include "digits.hpp"
#include "foldpow2.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "ring.hpp"

namespace lfk {

namespace {
using ring::NT;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// rho_i (NTT form) -> its coefficients (inverse Stockham, ring.hpp) -> the reversed byte
// table (foldpow2.hpp), one block per challenge. The blocks' ORs of "a coefficient is
// outside [-127, 127]" meet in sync[0]; the last block to finish (ticket sync[1])
// publishes it to *bad and resets both, so sync is zero again for the next launch: no
// memset per step and no host synchronisation (as k_rho_prep, fold_coeff.hip).
template <int D>
__global__ void __launch_bounds__(NT<D>::T) k_rho_prep_pow2(const uint64_t *rho, uint8_t *tab, int *bad,
                                                           ring::NegaTables inv, int *sync) {
  constexpr int T = NT<D>::T, PER = D / T, TB = 2 * D + 32;
  __shared__ uint64_t buf[2][D];
  __shared__ int any;
  const int tid = threadIdx.x, i = blockIdx.x;
  if (tid == 0) any = 0;
#pragma unroll
  for (int q = 0; q < PER; q++) buf[0][tid + q * T] = rho[(size_t)i * D + tid + q * T];
  __syncthreads();
  const uint64_t *r = ring::stockham4<D, T, true>(buf[0], buf[1], inv.roots, tid);
  uint8_t *ti = tab + (size_t)i * TB;
  bool out = false;
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int c = tid + q * T;
    const int64_t sv = signed_rep(gl::mul(r[c], inv.twist[c]));
    out |= sv > 127 || sv < -127;
    ti[fp2_tab_pos_plus(D, c)] = (uint8_t)(int8_t)sv;
    if (c > 0) ti[fp2_tab_pos_minus(D, c)] = (uint8_t)(int8_t)(-sv);
  }
  for (int o = tid; o < 32; o += T) ti[2 * D + o] = 0;
  if (tid == 0) ti[0] = 0;
  if (out) atomicOr(&any, 1);
  __syncthreads();
  if (tid == 0) {
    if (any) atomicOr(&sync[0], 1);
    __threadfence();
    if (atomicAdd(&sync[1], 1) == (int)gridDim.x - 1) {  // the last block: every block's flag is in
      *bad = atomicExch(&sync[0], 0) ? 1 : 0;
      atomicExch(&sync[1], 0);
    }
  }
}

// 16 bytes of a table at byte offset o (any alignment): 5 dwords, v_alignbyte
__device__ __forceinline__ v4i tile_a(const uint8_t *ri, int o, int sh) {
  const uint32_t *p = reinterpret_cast<const uint32_t *>(ri + (o & ~3));
  const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4];
  v4i a;
  a[0] = (int)__builtin_amdgcn_alignbyte(d1, d0, sh);
  a[1] = (int)__builtin_amdgcn_alignbyte(d2, d1, sh);
  a[2] = (int)__builtin_amdgcn_alignbyte(d3, d2, sh);
  a[3] = (int)__builtin_amdgcn_alignbyte(d4, d3, sh);
  return a;
}

// The 16 half words of a lane, transposed once per (side, q) so that a plane's digit bytes
// cost four instructions a dword: per dword g of four half words, lo[g] holds their low
// bytes (magnitude bits 0 .. 7, one coefficient a byte), hi[g] their high bytes (bits
// 8 .. 14) and sx[g] the byte 0xFF where the coefficient is negative, else 0x01. Bits of a
// half word above 15 are ignored.
struct DigitSrc {
  uint32_t lo[4], hi[4], sx[4];
};
__device__ __forceinline__ DigitSrc digit_src(const uint32_t (&hw)[16]) {
  DigitSrc s;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    // v_perm_b32: byte i of the result = byte sel_i of {first : second} (second = bytes 0 .. 3)
    const uint32_t t0 = __builtin_amdgcn_perm(hw[4 * g + 1], hw[4 * g], 0x05010400u);      // a0 b0 a1 b1
    const uint32_t t1 = __builtin_amdgcn_perm(hw[4 * g + 3], hw[4 * g + 2], 0x05010400u);  // c0 d0 c1 d1
    s.lo[g] = __builtin_amdgcn_perm(t1, t0, 0x05040100u);                                  // a0 b0 c0 d0
    s.hi[g] = __builtin_amdgcn_perm(t1, t0, 0x07060302u);                                  // a1 b1 c1 d1
    s.sx[g] = ((s.hi[g] >> 7) & 0x01010101u) * 0xFEu + 0x01010101u;  // bytes 0xFF / 0x01: no carry between bytes
  }
  return s;
}
// the 16 digit bytes (fp2_digit_byte) of the plane whose bit is bit `sh` of every byte of src
__device__ __forceinline__ v4i digit_bytes(const uint32_t (&src)[4], const uint32_t (&sx)[4], int sh) {
  v4i b;
#pragma unroll
  for (int g = 0; g < 4; g++) b[g] = (int)((((src[g] >> sh) & 0x01010101u) * 0xFFu) & sx[g]);  // 0x00 / 0xFF, then the sign
  return b;
}
__device__ __forceinline__ void load16(const uint32_t *p, uint32_t (&w)[16]) {
  const uint4 *src = reinterpret_cast<const uint4 *>(p);
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const uint4 x = src[v];
    w[4 * v] = x.x, w[4 * v + 1] = x.y, w[4 * v + 2] = x.z, w[4 * v + 3] = x.w;
  }
}

__device__ __forceinline__ uint64_t fe32(int x) { return x < 0 ? (uint64_t)(int64_t)x + gl::P : (uint64_t)x; }

// A block (4 waves) owns fp2_tiles_per_block element tiles of 32 elements at a time,
// fp2_waves_per_tile waves a tile, each its RT row tiles; grid-stride over (tile group,
// split). ks_n > 1 (few elements): task (group, ks) sums only the witnesses
// [ks nw / ks_n, (ks + 1) nw / ks_n) and writes exact int32 partials to part[ks][e][d],
// which k_fold_pow2_sum adds up. *bad (a rho that is not short): returns at once.
template <int D>
__global__ void __launch_bounds__(256, 2) k_fold_coeff_pow2(const uint32_t *sm0, const uint32_t *sm1,
                                                           const uint8_t *tab_g, const int *bad, size_t N, int K,
                                                           uint64_t *f0c, int ks_n, int32_t *part) {
  constexpr int TB = 2 * D + 32, NQ = D >= 32 ? D / 32 : 1, RT = NQ < 8 ? NQ : 8, WPT = NQ / RT, TPB = 4 / WPT;
  constexpr int HW = D / 2;  // packed words per element
  __shared__ __attribute__((aligned(16))) uint8_t rt[FP2_MAXW * TB];
  if (*bad) return;
  const int nw = 2 * K, tid = threadIdx.x;
  for (int x = tid; x < nw * TB / 16; x += blockDim.x)
    reinterpret_cast<uint4 *>(rt)[x] = reinterpret_cast<const uint4 *>(tab_g)[x];
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6, col = lane & 31, h = lane >> 5;
  const int sh = (-col) & 3, t0 = (wv % WPT) * RT;
  const size_t ntile = (N + 31) / 32, ngrp = (ntile + TPB - 1) / TPB;
  for (size_t task = blockIdx.x; task < ngrp * ks_n; task += gridDim.x) {
    const size_t tile = (task / ks_n) * TPB + wv / WPT;
    if (tile >= ntile) continue;  // wave-uniform; no barrier below
    const int ks = (int)(task % ks_n), i0 = fp2_split_begin(nw, ks, ks_n), i1 = fp2_split_begin(nw, ks + 1, ks_n);
    const size_t e = tile * 32 + col;
    const bool valid = e < N;
    const size_t ee = valid ? e : 0;
    v16i acc[RT];
#pragma unroll
    for (int tt = 0; tt < RT; tt++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[tt][i] = 0;
    if constexpr (D == 16) {
      // two witnesses a product: lane half h takes witness 2 m + h
      const int o = fp2_a_offset16(lane);
      for (int m = i0 / 2; m < i1 / 2; m++) {
        const int i = 2 * m + h, s = i >= K, k = i - s * K;
        const uint32_t *p = (s ? sm1 : sm0) + smp2_word(ee, D, 0);
        const uint4 lo = reinterpret_cast<const uint4 *>(p)[0], hi = reinterpret_cast<const uint4 *>(p)[1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t hw[16];
#pragma unroll
        for (int x = 0; x < 8; x++) hw[x] = w[x], hw[8 + x] = w[x] >> 16;
        const DigitSrc ds = digit_src(hw);
        const v4i b = k < 8 ? digit_bytes(ds.lo, ds.sx, k) : digit_bytes(ds.hi, ds.sx, k - 8);  // k varies by lane half
        v4i a = tile_a(rt + i * TB, o, sh);
        if (col >= 16) a = (v4i){0, 0, 0, 0};
        acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[0], 0, 0, 0);
      }
    } else {
      // the lane's A bytes of (row tile t, q): offset obase - 32 (t - q) of witness i's table
      const int obase = D + 16 * h - col;
      for (int s = 0; s < 2; s++) {
        const int ka = (i0 > s * K ? i0 : s * K) - s * K, kb = (i1 < (s + 1) * K ? i1 : (s + 1) * K) - s * K;
        if (ka >= kb) continue;
        const uint32_t *pe = (s ? sm1 : sm0) + smp2_word(ee, D, 0);
        for (int q = 0; q < NQ; q++) {
          const int j0 = 32 * q + 16 * h;  // the lane's 16 coefficients j0 .. j0 + 15 of its element
          uint32_t hw[16];
          load16(pe + (j0 & (HW - 1)), hw);
          if (j0 >= HW) {
#pragma unroll
            for (int x = 0; x < 16; x++) hw[x] >>= 16;
          }
          const DigitSrc ds = digit_src(hw);
          // planes [k0, k1) of this side, their bits in the bytes of src from bit k0 - kbit on
          auto planes = [&](const uint32_t (&src)[4], int k0, int k1, int kbit) {
            for (int k = k0; k < k1; k++) {
              const v4i b = digit_bytes(src, ds.sx, k - kbit);
              const uint8_t *ri = rt + (s * K + k) * TB;
#pragma unroll
              for (int tt = 0; tt < RT; tt++)
                acc[tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(tile_a(ri, obase - 32 * (t0 + tt - q), sh), b,
                                                                 acc[tt], 0, 0, 0);
            }
          };
          planes(ds.lo, ka, kb < 8 ? kb : 8, 0);
          planes(ds.hi, ka > 8 ? ka : 8, kb, 8);
        }
      }
    }
    if (!valid) continue;
    // lane (col, h), acc[tt][4 g + r]: row 32 (t0 + tt) + 8 g + 4 h + r of element e
    constexpr int NG = D == 16 ? 2 : 4;
    if (ks_n > 1) {
      int32_t *out = part + ((size_t)ks * N + e) * D + 32 * t0 + 4 * h;
#pragma unroll
      for (int tt = 0; tt < RT; tt++)
#pragma unroll
        for (int g = 0; g < NG; g++)
          *reinterpret_cast<v4i *>(out + 32 * tt + 8 * g) =
              (v4i){acc[tt][4 * g], acc[tt][4 * g + 1], acc[tt][4 * g + 2], acc[tt][4 * g + 3]};
    } else {
      uint64_t *out = f0c + e * D + 32 * t0 + 4 * h;
#pragma unroll
      for (int tt = 0; tt < RT; tt++)
#pragma unroll
        for (int g = 0; g < NG; g++) {
          ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + 32 * tt + 8 * g);
          o[0] = make_ulonglong2(fe32(acc[tt][4 * g]), fe32(acc[tt][4 * g + 1]));
          o[1] = make_ulonglong2(fe32(acc[tt][4 * g + 2]), fe32(acc[tt][4 * g + 3]));
        }
    }
  }
}

// f0c[e][c] = sum_ks part[ks][e][c] (exact: the full sum is the bounded one), canonical
__global__ void k_fold_pow2_sum(const int32_t *part, int ks_n, size_t n, const int *bad, uint64_t *f0c) {
  if (*bad) return;
  const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;  // 4 coefficients
  if (q >= n / 4) return;
  v4i s = *reinterpret_cast<const v4i *>(part + 4 * q);
  for (int k = 1; k < ks_n; k++) s += *reinterpret_cast<const v4i *>(part + (size_t)k * n + 4 * q);
  ulonglong2 *o = reinterpret_cast<ulonglong2 *>(f0c + 4 * q);
  o[0] = make_ulonglong2(fe32(s[0]), fe32(s[1]));
  o[1] = make_ulonglong2(fe32(s[2]), fe32(s[3]));
}

// *err |= bit when *flag is set (lf_dev_fold_planes: a rho that is not short is the caller's error)
__global__ void k_flag_to_err(const int *flag, int *err, int bit) {
  if (*flag) atomicOr(err, bit);
}

using Pow2Degrees = std::integer_sequence<int, 16, 32, 64, 128, 256, 512>;
}  // namespace

int fold_pow2_splits(size_t N, int d, int K, int ncu) {
  if (d == 16) return 1;  // 15 products a tile: nothing to split
  const size_t ntile = (N + 31) / 32, tpb = (size_t)fp2_tiles_per_block(d), ngrp = (ntile + tpb - 1) / tpb;
  const size_t cap = 2 * (size_t)ncu;
  int best = 1;
  for (int ks = 2; ks <= 2 * K; ks++)
    if ((2 * K) % ks == 0 && ngrp * ks <= cap) best = ks;
  return best;
}

hipError_t fold_pow2_rho_tables(const uint64_t *rho, int nw, int d, uint8_t *tab, int *bad,
                                const ring::NegaTables &inv, int *sync, hipStream_t st) {
  if (nw < 1 || nw > FP2_MAXW || !sync || !smp2_degree(d)) return hipErrorInvalidValue;
  return nega_degree_in(
      d,
      [&](auto dd) {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_rho_prep_pow2<D>), dim3(nw), dim3(NT<D>::T), 0, st, rho, tab, bad, inv, sync);
        return hipGetLastError();
      },
      Pow2Degrees{});
}

hipError_t fold_coeff_pow2(const uint32_t *sm0, const uint32_t *sm1, const uint8_t *tab, const int *bad, size_t N,
                           int d, int K, uint64_t *f0c, int ncu, hipStream_t st, int32_t *part) {
  if (K < 1 || 2 * K > FP2_MAXW || ncu < 1 || !smp2_degree(d)) return hipErrorInvalidValue;
  if (!N) return hipSuccess;
  const int ks_n = part ? fold_pow2_splits(N, d, K, ncu) : 1;
  const size_t ntile = (N + 31) / 32, tpb = (size_t)fp2_tiles_per_block(d), ngrp = (ntile + tpb - 1) / tpb;
  const size_t ntask = ngrp * ks_n, cap = 2 * (size_t)ncu;  // two blocks per CU
  hipError_t e = nega_degree_in(
      d,
      [&](auto dd) {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_fold_coeff_pow2<D>), dim3((unsigned)(ntask < cap ? ntask : cap)), dim3(256), 0, st, sm0,
                           sm1, tab, bad, N, K, f0c, ks_n, part);
        return hipGetLastError();
      },
      Pow2Degrees{});
  if (e != hipSuccess) return e;
  if (ks_n > 1) {
    const size_t n = N * (size_t)d;
    hipLaunchKernelGGL(k_fold_pow2_sum, dim3(blocks(n / 4, 256)), dim3(256), 0, st, part, ks_n, n, bad, f0c);
  }
  return hipGetLastError();
}

hipError_t flag_to_err(const int *flag, int *err, int bit, hipStream_t st) {
  hipLaunchKernelGGL(k_flag_to_err, dim3(1), dim3(1), 0, st, flag, err, bit);
  return hipGetLastError();
}

}  // namespace lfk
