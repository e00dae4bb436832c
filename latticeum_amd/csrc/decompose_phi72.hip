// decompose_phi72.hip -- decompose_witness for Phi_72 (d = 24): the block kernel for
// any b_small, and the wave-local b_small = 2 kernel on the packed sign|magnitude
// words, both of which can also write the digit planes as i8-MFMA operand rows.
#include "digitpack.hpp"
#include "digits.hpp"
#include "frag.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "ring.hpp"

namespace lfk {

// LF/nifs/decomposition.rs:162-167 + decomposition/utils.rs:45-49 + arith.rs:324-338:
// K balanced base-b_small digit vectors of f_coeff; per digit vector:
// f_k = CRT(f_coeff_k), w_ccs_k = recompose(f_k, B, L).
// Phi_72: one thread per element, 64 groups of L elements per block; the
// recompose across the L elements of a group goes through LDS.
constexpr int DEC_GROUPS = 48;  // 3 units of 16 groups: 240 of the 256 threads own an element
constexpr int DEC_SROW = 41;  // operand staging row (40 virtual slots + pad) of the fused d = 24 decomposition
// With frag != nullptr, planes k >= 1 are also written as i8-MFMA operand rows
// row0 + k - 1 (ajtai_mfma.hip, vector-major, Lp = L column order): the block's
// 48 groups are the 16-group units (G, l), G = 3 blockIdx.x + {0, 1, 2}, and each
// (unit, virtual slot) piece is assembled from the plane's NTT values in LDS.
// Every HBM access of the block is a run of whole 16-B pieces over contiguous
// rows: f_coeff comes in and f_coeff_k / f_k go out through LDS (the element
// rows [e][SROW] and a byte copy of the digits), not as one 192-B row per thread.
// blockIdx.z selects the side (both sides of a fold step in one launch)
__global__ void __launch_bounds__(256) k_decompose_phi72(FusedSides sd, size_t N, int lb, int L, int lbs, int K,
                                                        int *err, uint4 *frag, int nch, int srow) {
  extern __shared__ uint64_t lds[];  // [DEC_GROUPS * L][srow] u64; a row's words 25..27 hold the digit bytes
  const int side = blockIdx.z;
  const uint64_t *f_coeff = sd.f_coeff[side];
  uint64_t *f_coeff_k = sd.f_coeff_k[side], *f_k = sd.f_k[side], *w_ccs_k = sd.w_ccs_k[side];
  const int row0 = sd.row0[side];
  const int t = threadIdx.x, ne = DEC_GROUPS * L;
  int8_t *dgl = reinterpret_cast<int8_t *>(lds + 25);  // element e's digits at dgl[e * 8 srow + i]
  const size_t W = N / L;
  const size_t j0 = (size_t)blockIdx.x * ne, j = j0 + t;  // element index
  const int nv = (int)(N - j0 < (size_t)ne ? N - j0 : (size_t)ne);  // valid elements of the block
  const bool act = t < nv;
  // the block's f_coeff rows, 16 B per thread per step
  for (int q = t; q < nv * 12; q += blockDim.x) {
    const int e = q / 12, pr = q - 12 * e;
    const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(f_coeff + j0 * 24)[q];
    lds[e * srow + 2 * pr] = v.x;
    lds[e * srow + 2 * pr + 1] = v.y;
  }
  __syncthreads();
  int64_t cur[24];
  if (act) {
#pragma unroll
    for (int i = 0; i < 24; i++) cur[i] = signed_rep(lds[t * srow + i]);
  }
  // b = 2 (lbs = 1): the balanced digits are sign(v) bit_k(|v|) (bal_digit's
  // remainder is never rounded), so the planes are independent and
  // blockIdx.y takes a range of them; otherwise gridDim.y = 1 and the planes
  // run in order on the residual
  const int KP = (K + (int)gridDim.y - 1) / (int)gridDim.y;
  const int k0 = (int)blockIdx.y * KP, k1 = k0 + KP < K ? k0 + KP : K;
  for (int k = k0; k < k1; k++) {
    uint64_t c[24];
    if (act) {
#pragma unroll
      for (int i = 0; i < 24; i++) {
        int64_t dg;
        if (lbs == 1) {
          const int64_t m = cur[i] < 0 ? -cur[i] : cur[i], bit = (m >> k) & 1;
          dg = cur[i] < 0 ? -bit : bit;
        } else {
          dg = bal_digit(cur[i], lbs);
        }
        c[i] = from_signed(dg);
        // |digit| <= b/2 fits a byte for b_small <= 2^8; larger b_small keeps the u64 path below
        if (lbs <= 8) dgl[t * 8 * srow + i] = (int8_t)dg;
      }
      if (lbs > 8) ring::st24(f_coeff_k + ((size_t)k * N + j) * 24, c);
      ring::phi72_crt(c);
    }
    __syncthreads();  // the f_coeff rows (first plane) or the previous plane's rows are consumed
    if (act) {
#pragma unroll
      for (int i = 0; i < 24; i++) lds[t * srow + i] = c[i];
    }
    __syncthreads();
    // f_coeff_k and f_k rows of the block, and the recompose: one thread per (group, coefficient)
    {
      uint64_t *fck = f_coeff_k + ((size_t)k * N + j0) * 24, *fk = f_k + ((size_t)k * N + j0) * 24;
      for (int q = t; q < nv * 12; q += blockDim.x) {
        const int e = q / 12, pr = q - 12 * e;
        if (lbs <= 8)
          reinterpret_cast<ulonglong2 *>(fck)[q] =
              make_ulonglong2(from_signed(dgl[e * 8 * srow + 2 * pr]), from_signed(dgl[e * 8 * srow + 2 * pr + 1]));
        reinterpret_cast<ulonglong2 *>(fk)[q] = make_ulonglong2(lds[e * srow + 2 * pr], lds[e * srow + 2 * pr + 1]);
      }
    }
    for (int u = t; u < DEC_GROUPS * 24; u += blockDim.x) {
      const int g = u / 24, i = u % 24;
      const size_t wj = (size_t)blockIdx.x * DEC_GROUPS + g;
      if (wj < W) {
        uint64_t a = lds[(g * L + L - 1) * srow + i];
        for (int l = L - 2; l >= 0; l--) a = gl::add(gl::mul_pow2(a, lb), lds[(g * L + l) * srow + i]);
        w_ccs_k[((size_t)k * W + wj) * 24 + i] = a;
      }
    }
    if (frag && k > 0) {
      // each element's 40 virtual slots (Toom-3 evaluations, ring::phi72_eval) as
      // D8 words into LDS rows of srow, then one thread per (unit, virtual
      // slot) gathers the unit's 16 columns into the 8 operand pieces
      __syncthreads();  // the copy-out and recompose reads of lds are done
      if (act) {
#pragma unroll
        for (int vs = 0; vs < 40; vs++) lds[t * srow + vs] = fenc(ring::phi72_eval(c, vs));
      }
      __syncthreads();
      for (int tk = t; tk < DEC_GROUPS / 16 * L * 40; tk += blockDim.x) {
        const int vs = tk % 40, ul = tk / 40, gh = ul / L, l = ul - gh * L;
        const size_t Gu = (size_t)blockIdx.x * (DEC_GROUPS / 16) + gh, nG = frag_groups(W);
        if (Gu >= nG) continue;
        const size_t u = frag_pos(Gu, l, L, frag_ptop(nG, L));  // the unit's position in the contraction order
        uint64_t x[16];
#pragma unroll
        for (int jj = 0; jj < 16; jj++) {
          const int g = gh * 16 + jj;
          x[jj] = (size_t)blockIdx.x * DEC_GROUPS + g < W ? lds[(g * L + l) * srow + vs] : 0;
        }
        uint4 pu[8];
        d8_transpose16(x, pu);
        uint4 *out = frag + fv_index(vs, nch, (int)(u >> 1), row0 + k - 1, (int)(u & 1));
#pragma unroll
        for (int b = 0; b < 8; b++) out[4 * b] = pu[b];
      }
    }
    if (k + 1 < k1) __syncthreads();  // this plane's reads of the digit bytes and rows are done
  }
  if (act && blockIdx.y == 0) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 24; i++) bad |= lbs == 1 ? ((cur[i] < 0 ? -cur[i] : cur[i]) >> K) != 0 : cur[i] != 0;
    if (bad) raise(err, 1);
  }
}

// Phi_72 with b_small = 2, wave-local (the default d = 24 decomposition): a wave
// owns 16 groups -- one 16-column contraction unit per limb -- at 4 digit
// planes; lane 16 kq + gi owns group 16 G + gi at plane 4 pass + kq and walks
// the group's L limbs. The plane's digits of a limb are kept as two bit masks,
// so w_ccs_k = sum_l B^l f_k[gL + l] = CRT(sum_l B^l D_l) (linearity; an exact
// integer for (L - 1) lb < 62) is one more CRT per group, not a 24-value
// accumulator in registers. Every store instruction writes whole 192-B rows:
// lane t stores piece t % 12 of row t / 12 (64 lanes = 5.3 rows), the rows
// coming from the owning lane's masks (f_coeff_k, by ds_bpermute) or from a
// wave-private LDS tile (f_k, w_ccs_k) -- one request per line instead of one
// per 16-B piece, which is what bounds a store stream scattered over 192-B
// rows. The operand pieces of a (unit, plane) are a byte transpose over the 16
// lanes of a quarter, 8 virtual slots at a time through the same tile; each
// lane then emits the 4 pieces of one (plane, virtual slot, digit half). The
// waves of a block never synchronise with each other.
constexpr int PW_VS = 8;     // virtual slots per staging round (4 kq x 8 vs x 2 halves = one task per lane)
constexpr int PW_ROW = 17;   // u64 per operand staging row: 16 columns + pad
constexpr int PW_RROW = 25;  // u64 per element row in the tile: 24 + pad
constexpr int PW_WAVE_U64 = 64 * PW_RROW;  // 12.8 KB per wave (>= 4 PW_VS PW_ROW)
template <int NT>
__device__ __forceinline__ void st16(ulonglong2 *p, ulonglong2 v) {
  if (NT)
    nt_store(reinterpret_cast<uint4 *>(p), make_uint4((uint32_t)v.x, (uint32_t)(v.x >> 32), (uint32_t)v.y, (uint32_t)(v.y >> 32)));
  else
    *p = v;
}
// the coefficients of every (element, limb) of both sides as sign|magnitude words
// (digitpack.hpp, d = 24) once, so the K planes' waves read 48 B and take a bit
// instead of 24 u64 and a signed magnitude each (the range check |x| < 2^K is here
// too); thread = (side, element, pair)
__global__ void k_pack_sm24(FusedSides sd, size_t N, int K, int *err) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= (size_t)sd.nside * N * SM24_WORDS) return;
  const int side = t >= N * SM24_WORDS;
  const size_t q = t - side * N * SM24_WORDS;  // (element, pair): sm24_word
  const ulonglong2 v2 = reinterpret_cast<const ulonglong2 *>(sd.f_coeff[side])[q];
  bool bad = false;
  uint32_t o = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int64_t v = signed_rep(h ? v2.y : v2.x);
    bad |= sm16_overflow(v, K);
    o |= sign_mag16(v) << (16 * h);
  }
  if (bad) raise(err, 1);
  sd.smg[side][q] = o;
}

// NTM: streaming stores, bit 0 f_coeff_k, bit 1 f_k, bit 2 operand pieces; bit 3:
// packed planes only -- no u64 f_coeff_k / f_k rows, the decomposed witnesses
// stay as the digit masks (lf_fold_step_bufs.planes, lf_dev_expand_planes); bit 4
// (with bit 3): the masks are the input (sd.masks, read as mask24_digit reads them)
// instead of made from the packed words, and plane 0 is an operand row too: row0 - 1,
// which the launcher requires row_p0 to be (the row arithmetic of the other variants as it is)
template <int NTM>
__global__ void __launch_bounds__(256) k_decompose_phi72_w(FusedSides sd, size_t N, int lb, int L, int K, int *err,
                                                          uint4 *frag, int nch, size_t nblk) {
  constexpr bool ROWS = !(NTM & 8), PL = (NTM & 16) != 0;
  constexpr int KMIN = PL ? 0 : 1;  // the first plane with an operand row
  __shared__ uint64_t lds_all[4 * PW_WAVE_U64];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  uint64_t *S = lds_all + wib * PW_WAVE_U64;
  const int npass = (K + 3) / 4;
  const size_t task = (size_t)blockIdx.x * 4 + wib;  // (side, G, pass), pass fastest
  if (task >= (size_t)sd.nside * nblk * npass) return;  // wave-uniform; the kernel has no block barrier
  const int pass = (int)(task % npass);
  const size_t rest = task / npass;
  const int side = rest >= nblk ? 1 : 0;
  const size_t G = rest - side * nblk;
  const int kq = lane >> 4, gi = lane & 15, k = 4 * pass + kq;
  const bool kok = k < K;
  const size_t W = N / L, g = 16 * G + gi;
  const bool ok = g < W;
  uint64_t *f_coeff_k = sd.f_coeff_k[side], *f_k = sd.f_k[side], *w_ccs_k = sd.w_ccs_k[side];
  const int row0 = sd.row0[side];
  // this lane's operand task: plane kq_t, virtual slot PW_VS r + vl_t, digit half hf_t
  const int kq_t = lane >> 4, vl_t = (lane & 3) | ((lane >> 3 & 1) << 2), hf_t = lane >> 2 & 1;
  const int k_t = 4 * pass + kq_t;
  const bool emit = frag && k_t >= KMIN && k_t < K;
  // this lane's row pieces: piece (64 it + lane) % 12 of the row of source lane
  // (64 it + lane) / 12, it < 12. The lane index goes through an empty asm at
  // each use, so these per-piece offsets are recomputed (a few integer
  // operations) instead of being hoisted out of the limb loop into 100+ VGPRs
  auto opaque_lane = [&]() {
    int x = lane;
    asm volatile("" : "+v"(x));
    return x;
  };
  auto row_live = [&](int j) { return 16 * G + (j & 15) < W && 4 * pass + (j >> 4) < K; };
  uint32_t nzm[8], ngm[8];
  for (int l = L - 1; l >= 0; l--) {
    uint32_t nz = 0, ng = 0;
    if constexpr (PL) {
      if (ok && kok) {  // the caller's masks: bits 24..31 dropped, a sign without a digit dropped (mask24_digit)
        const uint2 m = sd.masks[side][mask24_index(k, N, g * L + l)];
        nz = m.x & 0xFFFFFFu;
        ng = m.y & nz;
      }
    } else if (ok && kok) {  // plane k of the 24 packed sign|magnitude coefficients (k_pack_sm24)
      const uint4 *src = reinterpret_cast<const uint4 *>(sd.smg[side] + sm24_word(g * L + l, 0));
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const uint4 w4 = src[q];
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 8; i++) {
          mask24_put(w[i >> 1] >> (16 * (i & 1)), k, 8 * q + i, nz, ng);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 8; q++)
      if (q == l) {
        nzm[q] = nz;
        ngm[q] = ng;
      }
    if (!PL && sd.masks[side] && ok && kok) sd.masks[side][mask24_index(k, N, g * L + l)] = make_uint2(nz, ng);
    // f_coeff_k rows from the owners' masks
    if constexpr (ROWS) {
    const int ln0 = opaque_lane();
#pragma unroll
    for (int it = 0; it < 12; it++) {
      const int j = (64 * it + ln0) / 12, pq = (64 * it + ln0) % 12;
      const uint32_t nzj = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * j, (int)nz);
      const uint32_t ngj = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * j, (int)ng);
      if (row_live(j)) {
        const size_t ej = (16 * G + (j & 15)) * L + l;
        st16<NTM & 1>(reinterpret_cast<ulonglong2 *>(f_coeff_k + ((size_t)(4 * pass + (j >> 4)) * N + ej) * 24) + pq,
                      make_ulonglong2(pw_digit(nzj, ngj, 2 * pq), pw_digit(nzj, ngj, 2 * pq + 1)));
      }
    }
    }
    // Planes that are zero on all 16 groups of this unit (the top limb's planes 4..K-1
    // of a balanced decomposition of a field element; fused d = 1024 / 4096 do the
    // same): bit 16 kq + gi of bal = lane's digits nonzero. A wave whose 4 planes are
    // all zero skips the transform and the operand rounds; a zero plane's operand
    // rows are left unwritten and flagged (lfk::DeadUnits)
    const uint64_t bal = __ballot(nz != 0);
    uint64_t c[24];
    if (bal) {
      ring::phi72_crt_ternary(nz, ng, c);
    } else {
#pragma unroll
      for (int i = 0; i < 24; i++) c[i] = 0;
    }
    // f_k rows through the tile
    if constexpr (ROWS) {
#pragma unroll
    for (int i = 0; i < 12; i++)
      *reinterpret_cast<ulonglong2 *>(S + lane * PW_RROW + 2 * i) = make_ulonglong2(c[2 * i], c[2 * i + 1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int ln1 = opaque_lane();
#pragma unroll
    for (int it = 0; it < 12; it++) {
      const int j = (64 * it + ln1) / 12, pq = (64 * it + ln1) % 12;
      const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(S + j * PW_RROW + 2 * pq);
      if (row_live(j)) {
        const size_t ej = (16 * G + (j & 15)) * L + l;
        st16<NTM & 2>(reinterpret_cast<ulonglong2 *>(f_k + ((size_t)(4 * pass + (j >> 4)) * N + ej) * 24) + pq, v);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the tile is read before the operand rounds reuse it
    }
    const size_t u = frag_pos(G, l, L, frag_ptop(frag_groups(W), L));  // position of these 16 columns' unit
    if (frag && sd.dead && gi == 0 && k >= KMIN && k < K)  // one lane per plane writes its flag
      sd.dead[u * 32 + row0 + k - 1] = ((bal >> (16 * kq)) & 0xFFFFull) ? 0 : 1;
    if (frag && (bal || !sd.dead)) {
      const int ch = (int)(u >> 1), uh = (int)(u & 1);
      const bool live_t = !sd.dead || ((bal >> (16 * kq_t)) & 0xFFFFull) != 0;  // this lane's task's plane
#pragma unroll
      for (int r = 0; r < 40 / PW_VS; r++) {
        // keep the rounds in order (the compiler would otherwise evaluate all
        // 40 virtual slots up front)
#pragma unroll
        for (int i = 0; i < 24; i += 4) asm volatile("" : "+v"(c[i]), "+v"(c[i + 1]), "+v"(c[i + 2]), "+v"(c[i + 3]));
#pragma unroll
        for (int v = 0; v < PW_VS; v++) S[(kq * PW_VS + v) * PW_ROW + gi] = fenc(ring::phi72_eval(c, PW_VS * r + v));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's tile writes landed
        const uint32_t *row = reinterpret_cast<const uint32_t *>(S + (kq_t * PW_VS + vl_t) * PW_ROW) + hf_t;
        uint32_t w[16];
#pragma unroll
        for (int jj = 0; jj < 16; jj++) w[jj] = row[2 * jj];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read before the next round overwrites the tile
        if (emit && live_t) {
          // 4 pieces: digit 4 hf_t + b of the 16 columns (byte jj = column jj)
          uint32_t o[4][4];
#pragma unroll
          for (int q = 0; q < 4; q++) byte_tr4(w + 4 * q, o[q]);
          const int vs = PW_VS * r + vl_t;
          uint4 *out = frag + fv_index(vs, nch, ch, row0 + k_t - 1, uh) + 16 * hf_t;
#pragma unroll
          for (int b = 0; b < 4; b++) out_store<(NTM & 4) != 0>(&out[4 * b], make_uint4(o[0][b], o[1][b], o[2][b], o[3][b]));
        }
      }
    }
  }
  if (!PL || w_ccs_k) {  // w_ccs_k = CRT(sum_l B^l D_l), rows w_ccs_k[k][16 G ..] through the tile (PL: may be null)
    uint64_t c[24];
#pragma unroll
    for (int i = 0; i < 24; i++) {
      int64_t a = 0;
      for (int l = L - 1; l >= 0; l--) {
        uint32_t nz = 0, ng = 0;
#pragma unroll
        for (int q = 0; q < 8; q++)
          if (q == l) {
            nz = nzm[q];
            ng = ngm[q];
          }
        a = a * ((int64_t)1 << lb) + mask24_digit(nz, ng, i);
      }
      c[i] = from_signed(a);
    }
    ring::phi72_crt(c);
#pragma unroll
    for (int i = 0; i < 12; i++)
      *reinterpret_cast<ulonglong2 *>(S + lane * PW_RROW + 2 * i) = make_ulonglong2(c[2 * i], c[2 * i + 1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 12; it++) {
      const int j = (64 * it + lane) / 12, pq = (64 * it + lane) % 12;
      const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(S + j * PW_RROW + 2 * pq);
      if (row_live(j))
        reinterpret_cast<ulonglong2 *>(w_ccs_k + ((size_t)(4 * pass + (j >> 4)) * W + 16 * G + (j & 15)) * 24)[pq] = v;
    }
  }
}

hipError_t decompose_phi72_sides(const FusedSides &sd, size_t N, int lb, int L, int lbs, int K, int *err,
                                 uint4 *frag, int nch, hipStream_t st, bool *masks_written, bool *dead_written) {
  const size_t W = N / L;
  if (masks_written) *masks_written = false;
  if (dead_written) *dead_written = false;
  if (W == 0) return hipSuccess;
  if (DEC_GROUPS * L > 256 || sd.nside < 1 || sd.nside > 2) return hipErrorInvalidValue;
  if (frag) {
    if (L > 5) return hipErrorInvalidValue;
    for (int s = 0; s < sd.nside; s++)
      if (sd.row0[s] < 0 || sd.row0[s] + K - 1 > 32) return hipErrorInvalidValue;
  }
  bool packed_sm = K <= 15;  // the wave kernel reads k_pack_sm24's 16-bit words
  for (int s = 0; s < sd.nside; s++) packed_sm &= sd.smg[s] != nullptr;
  // from the caller's masks (lf_dev_commit_planes): the wave-local kernel or nothing
  const bool pl = sd.planes_in();
  if (pl) {
    if (lbs != 1 || L > 8 || (L - 1) * lb >= 62 || K > 15 || !frag) return hipErrorInvalidValue;
    for (int s = 0; s < sd.nside; s++)
      if (!sd.masks[s] || sd.f_k[s] || sd.f_coeff_k[s] || sd.row_p0[s] < 0 || sd.row_p0[s] != sd.row0[s] - 1)
        return hipErrorInvalidValue;
  }
  if (lbs == 1 && L <= 8 && (L - 1) * lb < 62 && (packed_sm || pl)) {
    const size_t nblk = (W + 15) / 16, waves = (size_t)sd.nside * nblk * ((K + 3) / 4);
    if (!pl) {
      const size_t np = (size_t)sd.nside * N * SM24_WORDS;
      hipLaunchKernelGGL(k_pack_sm24, dim3(blocks(np, 256)), dim3(256), 0, st, sd, N, K, err);
    }
    // streaming stores for the f_coeff_k, f_k and operand rows (mask 7):
    // nothing in the step re-reads f_coeff_k or f_k (the fold reads the digit
    // masks), and the contraction's one pass over the operand rows does not gain
    // from them sitting in the caches either (W = 19 763, 4 streams: cached 0.65
    // ms per launch, 900 steps/s; mask 3 0.50-0.53 ms; mask 7 0.47-0.49 ms with
    // the contraction 0.385 -> 0.36 ms, 1,133-1,138 -> 1,141-1,150 steps/s)
    int ntm = 7;
    // no f_coeff_k / f_k buffers: the planes stay packed (the masks must be kept)
    bool all = true, none = true;  // every side has its u64 rows / no side has
    for (int s = 0; s < sd.nside; s++) {
      all &= sd.f_k[s] != nullptr && sd.f_coeff_k[s] != nullptr;
      none &= sd.f_k[s] == nullptr && sd.f_coeff_k[s] == nullptr;
    }
    if (!all && !none) return hipErrorInvalidValue;
    if (none) {
      for (int s = 0; s < sd.nside; s++)
        if (!sd.masks[s]) return hipErrorInvalidValue;
      ntm = pl ? 28 : 12;  // packed only (bit 3), the operand rows still streamed; bit 4: from the masks
    }
    const dim3 grid(blocks(waves, 4));
#define LF_PW(M)                                                                                          \
  case M:                                                                                                \
    hipLaunchKernelGGL(k_decompose_phi72_w<M>, grid, dim3(256), 0, st, sd, N, lb, L, K, err, frag, nch, nblk); \
    break;
    switch (ntm) { LF_PW(7) LF_PW(12) LF_PW(28) default: return hipErrorInvalidValue; }
#undef LF_PW
    if (masks_written) *masks_written = !pl && sd.masks[0] != nullptr && (sd.nside < 2 || sd.masks[1] != nullptr);
    if (dead_written) *dead_written = frag && sd.dead;  // the wave-local kernel flags its zero units
    return hipGetLastError();
  }
  const int srow = frag ? DEC_SROW : 28;
  const size_t lds = (size_t)DEC_GROUPS * L * srow * sizeof(uint64_t);
  // with independent planes (b = 2), split them over blockIdx.y until about
  // 1024 blocks run per side: the real zkvm shape (W = 19 763) has only 412
  // element blocks (one plane per block is no faster there: 0.30 against 0.29 ms)
  const unsigned nb = blocks(W, DEC_GROUPS);
  unsigned ys = lbs == 1 ? (1024 + nb - 1) / nb : 1;
  if (ys > (unsigned)K) ys = K;
  if (ys < 1) ys = 1;
  hipLaunchKernelGGL(k_decompose_phi72, dim3(nb, ys, (unsigned)sd.nside), dim3(256), lds, st, sd, N, lb, L, lbs, K,
                     err, frag, nch, srow);
  return hipGetLastError();
}

}  // namespace lfk
