// fold_coeff.hip -- f_0 = sum_i rho_i f_i (LF/nifs/folding.rs:258-268) for X^1024 + 1,
// in coefficient form on the i8 matrix cores.
//
// The 2K folded witnesses are the balanced digit planes of the two decomposed
// sides, f_i = NTT(D_i) with D_i in {-1, 0, 1}^1024 (b_small = 2), and the
// folding challenges are short: rho_i has coefficients in [-32, 32)
// (cyclotomic-rings rings/goldilocks.rs:41-67, get_rhos in folding/utils.rs:116-127).
// The NTT is a ring isomorphism, so f_0 = NTT(sum_i rho_i * D_i), * the
// negacyclic product, and
//   f0_coeff[c][e] = sum_i sum_j R_i[c][j] D_i[j][e],
//   R_i[c][j] = rho_i[c - j] (c >= j),  -rho_i[c - j + 1024] (c < j),
// an exact integer GEMM of i8 operands (|f0_coeff| <= 2K 1024 32 < 2^31):
// M = 1024 coefficients, N = elements, K = 2K x 1024. Canonicalised, it is
// Witness::from_f's f_coeff itself; f_0 and w_ccs follow from one forward
// transform per element (k_from_fcoeff_n32). Instead of the 2K NTT-form planes
// (E 2K N = 20 GB at W = 2^14) the fold reads one key byte per coefficient quad
// and plane (0.6 GB).
//
// R_i is Toeplitz: the 32 x 32 A tile of rows 32t.. and columns 32q.. depends
// only on t - q. A wave owns 8 row tiles; stepping q by one shifts its 8 tiles
// one diagonal, so it keeps them in an 8-slot register window and loads one new
// tile per 32-column step (16 bytes at a lane-dependent byte offset of the
// reversed table, assembled from 5 LDS dwords with v_alignbyte). The B operand
// (16 digits of one element) comes from 4 key bytes through a 256-entry LDS
// table: key = 4 magnitude bits | 4 sign bits -> the quad's 4 digit bytes.
//
// Used only when every rho_i has coefficients in [-127, 127] (k_rho_prep checks
// on the device); otherwise the flag it raises makes these kernels return at
// once and the NTT-form fold and Witness::from_f run instead (the same flag,
// the other way round), with no host synchronisation.
//
// The Karatsuba split (level 1, k_fold_coeff_kara1). With the signed generator
// g[delta] = rho[delta] (delta >= 0), -rho[delta + 1024] (delta < 0), R[c][j] =
// g[c - j], and the 512 x 512 Toeplitz blocks T1 (generator g[delta]) and T2
// (g[512 + delta]), R = [T1 -T2; T2 T1] and
//   R [V0; V1] = [P_a - P_c; P_a + P_b],
//   P_a = T1 (V0 + V1),  P_b = (T2 - T1) V0,  P_c = (T1 + T2) V1:
// three products of 16 x 16 tiles, 768 matrix instructions per plane and
// 32-element tile instead of 1024, and the same integers. The three generators are
// sums of two g values and the digit sums lie in [-2, 2], so for challenges in
// [-63, 63] (short ones lie in [-32, 32)) every operand is an i8; k_rho_prep builds
// their reversed byte tables beside the dense ones, checks every entry against
// [-128, 127] and publishes the level that runs (0: the dense product) in the word
// after the flag. k_fold_coeff and k_fold_coeff_kara1 are both launched and gated on
// that word, so the choice costs one empty launch and no host round trip;
// LATTICEUM_AMD_FOLD_KARA=0 caps the level (fold_kara_cap). A second level (nine
// 256 x 256 products, 576 instructions; its entries also fit i8 for every short
// challenge) is not built: DESIGN.md section 27.
#include "digitpack.hpp"
#include "digits.hpp"
#include "frag.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "ntt32.hpp"

namespace lfk {

namespace {
constexpr int FD = 1024;
constexpr int FC_KEYROW = 64;  // u32 per (element, plane): 256 key bytes

// bit b of x (b < 8) -> bit 4b
__device__ __forceinline__ uint32_t spread8(uint32_t x) {
  x &= 0xFFu;
  x = (x | (x << 12)) & 0x000F000Fu;
  x = (x | (x << 6)) & 0x03030303u;
  x = (x | (x << 3)) & 0x11111111u;
  return x;
}

// keys[(col K + k) 64 + h 32 + q] byte i = key of quad p = 8q + 4h + i (its
// coefficients 4p .. 4p + 3) in plane k: bit m = bit k of |x_(4p+m)|, bit 4 + m
// = its sign. From the fused decomposition's packed coefficients
// (digitpack.hpp, d = 1024). One thread per (col, h, 4 consecutive q):
// 128 B in, one 16-B row piece per plane out.
// nz[col] (when given): bit k = plane k of the column has a nonzero digit (the 16
// threads of a column are 16 consecutive lanes of one wave: OR by shuffles)
__global__ void __launch_bounds__(256) k_pack_keys(const uint32_t *smg, size_t ncol, int K, uint32_t *keys,
                                                   uint32_t *nz) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= (ncol * 16 + 63) / 64 * 64) return;  // whole waves stay (the shuffles below)
  const bool live_t = t < ncol * 16;
  const size_t col = live_t ? t >> 4 : 0;
  const int h = (int)(t >> 3) & 1, q0 = 4 * (int)(t & 7);
  // coefficient j = 32 q + 16 h + 4 i + m sits in word (qq = q / 2, rr = 16 h + 4 i + m), half q & 1
  uint32_t w[2][16];
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const uint4 *src = reinterpret_cast<const uint4 *>(smg + sm1024_word(col, q0 / 2 + a, 16 * h));
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const uint4 x = src[v];
      w[a][4 * v] = x.x;
      w[a][4 * v + 1] = x.y;
      w[a][4 * v + 2] = x.z;
      w[a][4 * v + 3] = x.w;
    }
  }
  if (nz) {
    uint32_t m = 0;  // magnitude bits of every coefficient this thread holds
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int i = 0; i < 16; i++) m |= w[a][i] | (w[a][i] >> 16);
    m &= SM16_MAG;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m |= __shfl_xor(m, o);
    if (live_t && (t & 15) == 0) nz[col] = m;
  }
  if (!live_t) return;
  // per quad: planes 0..7 (lo) and 8..15 (hi, plane 15 = the sign) bit-sliced, bit 4 (k % 8) + m
  uint32_t lo[16], hi[16];
#pragma unroll
  for (int qd = 0; qd < 4; qd++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t L = 0, H = 0;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const uint32_t v = w[qd >> 1][4 * i + m] >> (16 * (qd & 1));
        L |= spread8(v) << m;
        H |= spread8(v >> 8) << m;
      }
      lo[4 * qd + i] = L;
      hi[4 * qd + i] = H;
    }
  uint4 *dst = reinterpret_cast<uint4 *>(keys + col * K * FC_KEYROW + 32 * h + q0);
  for (int k = 0; k < K; k++) {
    uint32_t o[4];
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
      uint32_t x = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int u = 4 * qd + i;
        const uint32_t nib = (k < 8 ? lo[u] >> (4 * k) : hi[u] >> (4 * (k - 8))) & 0xFu;
        x |= (nib | ((hi[u] >> 28) << 4)) << (8 * i);
      }
      o[qd] = x;
    }
    dst[k * (FC_KEYROW / 4)] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// rho (2K NTT elements) -> coefficients (rc), reversed byte tables and the range
// flag in ONE launch: half-wave i inverts rho_i on the register 32 x 32 NTT
// (ntt32.hpp), then writes its coefficients and
//   tab[i][u + 1024] = rho_i[-u] (-1023 <= u <= 0), -rho_i[1024 - u] (1 <= u <= 1023), else 0.
// The blocks' ORs of "a coefficient is outside [-127, 127]" meet in sync[0]; the
// last block to finish (ticket sync[1]) publishes it to *bad and resets both, so
// sync is zero again for the next launch (no memset). It replaces a device copy,
// a memset, the 2K-element inverse transform and the table kernel (about 35 us
// of serialised launches per step at W = 464).
// kara_cap >= 1: after the nw dense tables it also writes the level-1 tables
//   tab1[i][p][u + 512] = G_p[-u] (|u| <= 511), else 0, G_0 = T1, G_1 = T2 - T1, G_2 = T1 + T2
// (FOLD_RT1 bytes each), ORs "an entry is outside [-128, 127]" into bit 1 of sync[0],
// and the last block publishes bad[1] = the level that runs: kara_cap if neither bit
// is set, else 0.
constexpr int RP_WAVES = 2;  // 4 rho per block: 2K = 30 is 8 blocks of one round each
__global__ void __launch_bounds__(64 * RP_WAVES) k_rho_prep(const uint64_t *rho, int nw, uint64_t *rc, uint8_t *tab,
                                                           int *bad, const uint64_t *mid_ig, int *sync, int kara_cap) {
  __shared__ uint64_t lds_all[RP_WAVES * n32::WAVE_U64];
  __shared__ uint64_t mid[n32::MID_U64];
  __shared__ int any;
  n32::stage_mid(mid, mid_ig);
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  uint64_t *T = lds_all + wib * n32::WAVE_U64 + h * n32::HALF_U64;
  bool out = false;
  int64_t hi1 = 0, lo1 = 0;  // the extremes of the level-1 entries
  uint8_t *tab1 = tab + (size_t)nw * FOLD_RT;
  // every wave runs every round (wave-uniform)
  for (int i0 = 2 * RP_WAVES * blockIdx.x; i0 < nw; i0 += 2 * RP_WAVES * gridDim.x) {
    const int i = i0 + 2 * wib + h;
    const bool ok = i < nw;
    uint64_t v[32];
    n32::load_row32(rho + (size_t)(ok ? i : 0) * FD + r, v);  // slot input layout v[m2] = X[r + 32 m2]
    n32::inverse(v, mid, T, r);                                 // coefficient layout v[k] = x[r + 32 k]
    if (ok) {
      uint64_t *rci = rc + (size_t)i * FD + r;
      uint8_t *ti = tab + (size_t)i * FOLD_RT;
#pragma unroll
      for (int k = 0; k < 32; k++) {
        const int c = r + 32 * k;
        const int64_t sv = signed_rep(v[k]);
        out |= sv > 127 || sv < -127;
        rci[32 * k] = v[k];
        ti[1024 - c] = (uint8_t)(int8_t)sv;                      // u = -c
        if (c > 0) ti[2048 - c] = (uint8_t)(int8_t)(-sv);        // u = 1024 - c
      }
      // u = -1024 and u >= 1024: zero (positions 0 and 2048 .. FOLD_RT - 1)
      for (int o = 2048 + r; o < FOLD_RT; o += 32) ti[o] = 0;
      if (r == 0) ti[0] = 0;
      if (kara_cap >= 1) {
        // level 1: a = rho[c], b = rho[c + 512] (c < 512) give the three generators at
        // delta = c (T1: a, T2: b) and at delta = c - 512 (T1: -b, T2: a)
        uint8_t *t1 = tab1 + (size_t)i * 3 * FOLD_RT1;
#pragma unroll
        for (int k = 0; k < 16; k++) {
          const int c = r + 32 * k;
          const int64_t a = signed_rep(v[k]), b = signed_rep(v[k + 16]);
          const int64_t g[2][3] = {{a, b - a, a + b}, {-b, a + b, a - b}};
#pragma unroll
          for (int p = 0; p < 3; p++) {
            const int64_t g1 = c > 0 ? g[1][p] : 0;  // c = 0: delta = -512 is not an entry
            hi1 = max(hi1, max(g[0][p], g1));
            lo1 = min(lo1, min(g[0][p], g1));
            t1[p * FOLD_RT1 + 512 - c] = (uint8_t)(int8_t)g[0][p];
            if (c > 0) t1[p * FOLD_RT1 + 1024 - c] = (uint8_t)(int8_t)g[1][p];
          }
        }
        // u = -512 and u >= 512: zero (positions 0 and 1024 .. FOLD_RT1 - 1)
        if (r < FOLD_RT1 - 1024 + 1)
#pragma unroll
          for (int p = 0; p < 3; p++) t1[p * FOLD_RT1 + (r ? 1023 + r : 0)] = 0;
      }
    }
  }
  const bool out1 = hi1 > 127 || lo1 < -128;
  if (out || out1) atomicOr(&any, (out ? 1 : 0) | (out1 ? 2 : 0));
  __syncthreads();
  if (threadIdx.x == 0) {
    if (any) atomicOr(&sync[0], any);
    __threadfence();
    if (atomicAdd(&sync[1], 1) == (int)gridDim.x - 1) {  // the last block: every block's flags are in
      const int f = atomicExch(&sync[0], 0);
      bad[0] = f & 1;
      bad[1] = f ? 0 : kara_cap;  // the level that runs (one level is built: f & 2 rules it out)
      atomicExch(&sync[1], 0);
    }
  }
}

// 16 bytes of a rho table at byte offset o (any alignment): 5 dwords, v_alignbyte
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

constexpr int FC_MAXW = 30;  // 2K <= 30
// A block (4 waves) owns 32 elements (MFMA columns) at a time; wave w the rows
// 256 w .. 256 w + 255 (row tiles t = 8 w + tt). Grid-stride over element tiles.
// ks_n > 1 (few elements: fewer 32-element tiles than the chip has block
// slots): task (tile, ks) sums only witnesses [ks nw / ks_n, (ks + 1) nw / ks_n)
// and writes its exact int32 partials to part[ks][e][1024]; k_fold_coeff_sum
// adds them up
// *bad (rho not short): with fb.frag the launch folds f_0 in NTT form from the
// operand rows instead (fold_frag_block, grid-stride; a separate gated launch of
// its (d / 16) nch blocks would wait for CU resources behind other streams' work
// even when it has nothing to do), else it returns and the NTT-form fold runs
__global__ void __launch_bounds__(256, 2) k_fold_coeff(const uint32_t *keys, const uint8_t *tab_g, const int *bad,
                                                      size_t N, int K, uint64_t *f0c, int ks_n, int32_t *part,
                                                      FoldFallback fb, int L, const uint32_t *nz) {
  __shared__ __attribute__((aligned(16))) uint8_t rt[FC_MAXW * FOLD_RT];
  __shared__ uint32_t lut[256];
  static_assert(FC_MAXW * FOLD_RT >= 512 * 9 * 8, "fold_frag_block's LDS fits the rho tables'");
  if (*bad) {
    if (fb.frag) {
      const size_t nvb = (size_t)(FD / 16) * fb.nch;
      for (size_t vb = blockIdx.x; vb < nvb; vb += gridDim.x)
        fold_frag_block(vb, fb.frag, fb.nch, fb.Lp, fb.Wp, fb.fr, fb.rho, FD, N, fb.f0,
                        reinterpret_cast<uint64_t *>(rt));
    }
    return;
  }
  if (bad[1] != 0) return;  // a Karatsuba level runs (k_fold_coeff_kara1)
  const int nw = 2 * K, tid = threadIdx.x;
  for (int x = tid; x < nw * FOLD_RT / 16; x += blockDim.x)
    reinterpret_cast<uint4 *>(rt)[x] = reinterpret_cast<const uint4 *>(tab_g)[x];
  {
    const uint32_t m = tid & 15, s = tid >> 4;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if ((m >> i) & 1) v |= ((s >> i) & 1 ? 0xFFu : 0x01u) << (8 * i);
    lut[tid] = v;
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6, col = lane & 31, h = lane >> 5;
  const int sh = (-col) & 3;
  // A tile of diagonal dl = t - q for this lane: bytes o .. o + 15, o = obase - 32 dl
  const int obase = 1024 + 16 * h - col;
  // Tiles are limb-pure: tile (l, gt) holds elements (32 gt + col) L + l, so a
  // tile of the top limb (whose planes 4.. are zero for any balanced
  // decomposition of a field element) skips those planes' products; a plane is
  // skipped only when it is zero on all 32 of the tile's elements (nz: the
  // per-column plane masks of k_pack_keys), so any input stays exact.
  const size_t W = N / L, ntl = (W + 31) / 32, ntile = ntl * L;
  for (size_t task = blockIdx.x; task < ntile * ks_n; task += gridDim.x) {
    const size_t tile = task / ks_n;
    const int ks = (int)(task % ks_n), iq0 = 4 * (ks * nw / ks_n), iq1 = 4 * ((ks + 1) * nw / ks_n);
    const size_t grp = (tile % ntl) * 32 + col;
    const bool valid = grp < W;
    const size_t e = grp * L + tile / ntl, ee = valid ? e : 0;
    uint32_t live = nz ? (valid ? nz[ee] | (nz[N + ee] << K) : 0u) : 0xFFFFFFFFu;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) live |= __shfl_xor(live, o);  // the tile's 32 columns (both halves agree)
    live = __builtin_amdgcn_readfirstlane(live);
    // the next iq at or after iq whose plane is live (whole planes are skipped)
    auto next_live = [&](int iq) {
      while (iq < iq1 && !((live >> (iq >> 2)) & 1u)) iq = (iq & ~3) + 4;
      return iq;
    };
    const uint32_t *kb0 = keys + ee * K * FC_KEYROW + 32 * h, *kb1 = keys + (N + ee) * K * FC_KEYROW + 32 * h;
    v16i acc[8];
#pragma unroll
    for (int tt = 0; tt < 8; tt++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[tt][i] = 0;
    v4i A[8];
    // the key words of (plane i, q block qb): 8 dwords, one block ahead
    auto kaddr = [&](int iq) {
      const int i = iq >> 2, s = i >= K;
      return (s ? kb1 : kb0) + (i - s * K) * FC_KEYROW + 8 * (iq & 3);
    };
    uint4 kn0 = make_uint4(0, 0, 0, 0), kn1 = kn0;
    const int iqs = next_live(iq0);
    if (iqs < iq1) {
      const uint4 *p = reinterpret_cast<const uint4 *>(kaddr(iqs));
      kn0 = p[0];
      kn1 = p[1];
    }
    for (int iq = iqs; iq < iq1; iq = next_live(iq + 1)) {
      const int i = iq >> 2;
      const uint8_t *ri = rt + i * FOLD_RT;
      if ((iq & 3) == 0) {  // a new plane: slots 1..7 take diagonals 8 w + 1 .. 8 w + 7
#pragma unroll
        for (int tt = 1; tt < 8; tt++) A[tt] = tile_a(ri, obase - 32 * (8 * wv + tt), sh);
      }
      const uint32_t kw[8] = {kn0.x, kn0.y, kn0.z, kn0.w, kn1.x, kn1.y, kn1.z, kn1.w};
      {
        const int nx = next_live(iq + 1);
        const uint4 *p = reinterpret_cast<const uint4 *>(kaddr(nx < iq1 ? nx : iq));
        kn0 = p[0];
        kn1 = p[1];
      }
      const int q0 = 8 * (iq & 3);
#pragma unroll
      for (int qi = 0; qi < 8; qi++) {
        // slot (tt - q) & 7 holds diagonal 8 w + tt - q; the new one (tt = 0) goes to slot (-q) & 7
        A[(8 - qi) & 7] = tile_a(ri, obase - 32 * (8 * wv - (q0 + qi)), sh);
        v4i b;
        b[0] = (int)lut[kw[qi] & 0xFF];
        b[1] = (int)lut[(kw[qi] >> 8) & 0xFF];
        b[2] = (int)lut[(kw[qi] >> 16) & 0xFF];
        b[3] = (int)lut[kw[qi] >> 24];
#pragma unroll
        for (int tt = 0; tt < 8; tt++)
          acc[tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[(tt - qi) & 7], b, acc[tt], 0, 0, 0);
      }
    }
    if (valid && ks_n > 1) {
      int32_t *out = part + ((size_t)ks * N + e) * FD + 256 * wv + 4 * h;
#pragma unroll
      for (int tt = 0; tt < 8; tt++)
#pragma unroll
        for (int g = 0; g < 4; g++)
          *reinterpret_cast<v4i *>(out + 32 * tt + 8 * g) =
              (v4i){acc[tt][4 * g], acc[tt][4 * g + 1], acc[tt][4 * g + 2], acc[tt][4 * g + 3]};
    } else if (valid) {
      // lane (col, h), acc[tt][4 g + r]: row 32 (8 w + tt) + 8 g + 4 h + r of element e
      uint64_t *out = f0c + e * FD + 256 * wv + 4 * h;
      auto fe = [](int x) { return x < 0 ? (uint64_t)(int64_t)x + gl::P : (uint64_t)x; };
#pragma unroll
      for (int tt = 0; tt < 8; tt++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + 32 * tt + 8 * g);
          o[0] = make_ulonglong2(fe(acc[tt][4 * g]), fe(acc[tt][4 * g + 1]));
          o[1] = make_ulonglong2(fe(acc[tt][4 * g + 2]), fe(acc[tt][4 * g + 3]));
        }
    }
  }
}
// ---------------------------------------------------------------- level 1 of the Karatsuba split
constexpr int FC1_TAB = 3 * FOLD_RT1;  // bytes per witness: the generators of T1, T2 - T1, T1 + T2

// byte-wise a + b of two digit words (every byte sum is in [-2, 2]; a plain add would
// carry out of a byte that holds -1)
__device__ __forceinline__ uint32_t add_bytes(uint32_t a, uint32_t b) {
  return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}

// acc += T (V0 + V1) (MODE 0), T V0 (1) or T V1 (2) over the live planes [i0, i1) for
// one wave's 8 row tiles (rows 256 rh .. of the 512) and 32 elements: the register
// window of k_fold_coeff on a 16 x 16-tile Toeplitz matrix whose reversed generator
// of plane i is tp + i FC1_TAB.
//
// One wave per SIMD: no other wave hides the LDS latency of a step's operands, and
// left alone the scheduler gathers a plane's reads in front of its 128 products. So
// the operand work is one software pipeline over the steps (plane, q), cut in slices
// that sched_barrier pins between the products. Step q issues the products of row
// tiles 1..7, then 0 (the step's new diagonal, whose slot tile 7 of step q - 1 has
// just left); after its product
//   0      the new A tile is assembled (v_alignbyte) from what step q - 1 read,
//   1, 2   step q + 1's B words are assembled (digit sums) from step q - 1's reads,
//   3      step q + 1's A dwords are read,
//   4, 5   step q + 2's digit words are looked up,
//   6      one tile of the next live plane's starting window is read / assembled,
//   7      four steps' key words are reloaded in place for the next live plane, once
//          their last reader (the lookup of two steps ahead) is past.
// The pipeline runs across planes: steps 14 and 15 look up and read for the next
// plane's steps 0 and 1.
template <int MODE>
__device__ __forceinline__ void kara1_pass(v16i (&acc)[8], const uint8_t *tp, const uint32_t *lut,
                                           const uint32_t *kb0, size_t side1, int K, uint32_t live, int i0,
                                           int i1, int rh, int obase, int sh) {
  constexpr int NV = MODE == 0 ? 2 : 1;  // key words per step: V0 and V1, or one of them
  auto next_live = [&](int i) {
    while (i < i1 && !((live >> i) & 1u)) i++;
    return i;
  };
  auto krow = [&](int i) {
    const int s = i >= K;
    return reinterpret_cast<const uint4 *>(kb0 + ((s ? side1 : 0) + (i - s * K) * FC_KEYROW + (MODE == 2 ? 16 : 0)));
  };
  int i = next_live(i0);
  if (i >= i1) return;
  uint4 kq[NV][4];  // kq[v][m]: the key words of steps 4 m .. 4 m + 3
  auto load_keys = [&](int pl, int m) {
    const uint4 *p = krow(pl);
#pragma unroll
    for (int v = 0; v < NV; v++) kq[v][m] = p[4 * v + m];
  };
  auto key = [&](int v, int q) {
    const uint4 &u = kq[v][q >> 2];
    return (q & 3) == 0 ? u.x : (q & 3) == 1 ? u.y : (q & 3) == 2 ? u.z : u.w;
  };
  // the A tile of diagonal dl of the table at r: 5 dwords, then 4 v_alignbyte
  auto fetch_a = [&](const uint8_t *r, int dl, uint32_t (&d)[5]) {
    const int o = obase - 32 * dl;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(r + (o & ~3));
#pragma unroll
    for (int x = 0; x < 5; x++) d[x] = p[x];
  };
  auto asm_a = [&](const uint32_t (&d)[5], v4i &a) {
#pragma unroll
    for (int x = 0; x < 4; x++) a[x] = (int)__builtin_amdgcn_alignbyte(d[x + 1], d[x], sh);
  };
  // digit words j0, j0 + 1 of step q's key word(s)
  uint32_t rl[NV][4];
  auto fetch_b = [&](int q, int j0) {
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
      for (int j = j0; j < j0 + 2; j++) rl[v][j] = lut[(key(v, q) >> (8 * j)) & 0xFF];
  };
  auto asm_b = [&](int x0, v4i &b) {
#pragma unroll
    for (int x = x0; x < x0 + 2; x++) b[x] = (int)(MODE == 0 ? add_bytes(rl[0][x], rl[NV - 1][x]) : rl[0][x]);
  };
#pragma unroll
  for (int m = 0; m < 4; m++) load_keys(i, m);
  int nx = next_live(i + 1);
  const uint8_t *ri = tp + i * FC1_TAB;
  v4i A[8], An[8], bb[2];
  uint32_t rd[5], wd[5];
  // the first plane's window (slots 1..7: diagonals 8 rh + 1 .. 8 rh + 7), step 0's B
  // words and A dwords, step 1's digit words
  {
    uint32_t d[7][5];
#pragma unroll
    for (int tt = 1; tt < 8; tt++) fetch_a(ri, 8 * rh + tt, d[tt - 1]);
#pragma unroll
    for (int tt = 1; tt < 8; tt++) asm_a(d[tt - 1], A[tt]);
  }
  fetch_b(0, 0);
  fetch_b(0, 2);
  asm_b(0, bb[0]);
  asm_b(2, bb[0]);
  fetch_a(ri, 8 * rh, rd);
  fetch_b(1, 0);
  fetch_b(1, 2);
  for (;;) {
    const bool more = nx < i1;
    const int pn = more ? nx : i;  // the last plane reads itself again (unused)
    const uint8_t *rin = tp + pn * FC1_TAB;
#pragma unroll
    for (int q = 0; q < 16; q++) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int tt = (k + 1) & 7;
        __builtin_amdgcn_sched_barrier(0);
        acc[tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[(tt - q) & 7], bb[q & 1], acc[tt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (k == 0) asm_a(rd, A[(16 - q) & 7]);
        if (k == 1) asm_b(0, bb[(q + 1) & 1]);
        if (k == 2) asm_b(2, bb[(q + 1) & 1]);
        if (k == 3) fetch_a(q < 15 ? ri : rin, 8 * rh - ((q + 1) & 15), rd);
        if (k == 4) fetch_b((q + 2) & 15, 0);
        if (k == 5) fetch_b((q + 2) & 15, 2);
        if (k == 6) {  // the next plane's window: tile q - 6 read at steps 7..13, assembled a step later
          if (q >= 8 && q <= 14) asm_a(wd, An[q - 7]);
          if (q >= 7 && q <= 13) fetch_a(rin, 8 * rh + q - 6, wd);
        }
        if (k == 7 && (q & 3) == 2) load_keys(pn, q >> 2);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (!more) break;
#pragma unroll
    for (int tt = 1; tt < 8; tt++) A[tt] = An[tt];
    i = nx;
    ri = rin;
    nx = next_live(i + 1);
  }
}

// One level of the Karatsuba split (the header): a block owns two 32-element tiles,
// wave (s, rh) = (wv / 2, wv % 2) the row half rh of the three 512 x 512 products of
// tile s, one after the other on two accumulator sets:
//   a0 = P_a;  a1 = a0;  a0 = -a0 + P_c = -R0;  a1 += P_b = R1
// so the partial products meet in registers. 512 registers per wave, one block per
// CU, all three generators of every witness in LDS (94 KB). Runs only when
// bad[1] == 1 (k_rho_prep); tasks, plane skips and the witness splits as k_fold_coeff.
__global__ void __launch_bounds__(256, 1) k_fold_coeff_kara1(const uint32_t *keys, const uint8_t *tab1_g,
                                                            const int *bad, size_t N, int K, uint64_t *f0c, int ks_n,
                                                            int32_t *part, int L, const uint32_t *nz) {
  __shared__ __attribute__((aligned(16))) uint8_t rt[FC_MAXW * FC1_TAB];
  __shared__ uint32_t lut[256];
  if (bad[1] != 1) return;
  const int nw = 2 * K, tid = threadIdx.x;
  for (int x = tid; x < nw * FC1_TAB / 16; x += blockDim.x)
    reinterpret_cast<uint4 *>(rt)[x] = reinterpret_cast<const uint4 *>(tab1_g)[x];
  {
    const uint32_t m = tid & 15, s = tid >> 4;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if ((m >> i) & 1) v |= ((s >> i) & 1 ? 0xFFu : 0x01u) << (8 * i);
    lut[tid] = v;
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6, col = lane & 31, h = lane >> 5;
  const int sh = (-col) & 3, rh = wv & 1;
  const int obase = 512 + 16 * h - col;
  const size_t W = N / L, ntl = (W + 31) / 32, ntile = ntl * L, npair = (ntile + 1) / 2;
  for (size_t task = blockIdx.x; task < npair * ks_n; task += gridDim.x) {
    const size_t tile = 2 * (task / ks_n) + (wv >> 1);
    if (tile >= ntile) continue;  // wave-uniform; no barrier below
    const int ks = (int)(task % ks_n), i0 = ks * nw / ks_n, i1 = (ks + 1) * nw / ks_n;
    const size_t grp = (tile % ntl) * 32 + col;
    const bool valid = grp < W;
    const size_t e = grp * L + tile / ntl, ee = valid ? e : 0;
    uint32_t live = nz ? (valid ? nz[ee] | (nz[N + ee] << K) : 0u) : 0xFFFFFFFFu;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) live |= __shfl_xor(live, o);
    live = __builtin_amdgcn_readfirstlane(live);
    const uint32_t *kb0 = keys + ee * K * FC_KEYROW + 32 * h;
    const size_t side1 = N * K * FC_KEYROW;  // side 1's keys of the same element (uniform)
    v16i a0[8], a1[8];
#pragma unroll
    for (int tt = 0; tt < 8; tt++)
#pragma unroll
      for (int i = 0; i < 16; i++) a0[tt][i] = 0;
    kara1_pass<0>(a0, rt, lut, kb0, side1, K, live, i0, i1, rh, obase, sh);
#pragma unroll
    for (int tt = 0; tt < 8; tt++) {
      a1[tt] = a0[tt];
      a0[tt] = -a0[tt];
    }
    // lane (col, h), a[tt][4 g + r]: row 256 rh + 32 tt + 8 g + 4 h + r of R0 (-a0) and of R1 (a1)
    auto store = [&](const v16i (&a)[8], int row) {
      if (!valid) return;
      if (ks_n > 1) {
        int32_t *out = part + ((size_t)ks * N + e) * FD + row;
#pragma unroll
        for (int tt = 0; tt < 8; tt++)
#pragma unroll
          for (int g = 0; g < 4; g++)
            *reinterpret_cast<v4i *>(out + 32 * tt + 8 * g) =
                (v4i){a[tt][4 * g], a[tt][4 * g + 1], a[tt][4 * g + 2], a[tt][4 * g + 3]};
      } else {
        uint64_t *out = f0c + e * FD + row;
        auto fe = [](int x) { return x < 0 ? (uint64_t)(int64_t)x + gl::P : (uint64_t)x; };
#pragma unroll
        for (int tt = 0; tt < 8; tt++)
#pragma unroll
          for (int g = 0; g < 4; g++) {
            ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + 32 * tt + 8 * g);
            o[0] = make_ulonglong2(fe(a[tt][4 * g]), fe(a[tt][4 * g + 1]));
            o[1] = make_ulonglong2(fe(a[tt][4 * g + 2]), fe(a[tt][4 * g + 3]));
          }
      }
    };
    kara1_pass<2>(a0, rt + 2 * FOLD_RT1, lut, kb0, side1, K, live, i0, i1, rh, obase, sh);
#pragma unroll
    for (int tt = 0; tt < 8; tt++) a0[tt] = -a0[tt];
    store(a0, 256 * rh + 4 * h);
    kara1_pass<1>(a1, rt + FOLD_RT1, lut, kb0, side1, K, live, i0, i1, rh, obase, sh);
    store(a1, 512 + 256 * rh + 4 * h);
  }
}

// f0c[e][c] = sum_ks part[ks][e][c] (exact: the full sum is the bounded one), canonical
__global__ void k_fold_coeff_sum(const int32_t *part, int ks_n, size_t n, const int *bad, uint64_t *f0c) {
  if (*bad) return;
  const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;  // 4 coefficients
  if (q >= n / 4) return;
  v4i s = *reinterpret_cast<const v4i *>(part + 4 * q);
  for (int k = 1; k < ks_n; k++) s += *reinterpret_cast<const v4i *>(part + (size_t)k * n + 4 * q);
  auto fe = [](int x) { return x < 0 ? (uint64_t)(int64_t)x + gl::P : (uint64_t)x; };
  ulonglong2 *o = reinterpret_cast<ulonglong2 *>(f0c + 4 * q);
  o[0] = make_ulonglong2(fe(s[0]), fe(s[1]));
  o[1] = make_ulonglong2(fe(s[2]), fe(s[3]));
}
}  // namespace

// witness splits for N elements: enough (tile, split) tasks for two blocks per
// CU, the splits dividing the 2K witnesses evenly (1 at the bench's W = 2^14)
int fold_coeff_splits(size_t N, int K, int ncu) {
  const size_t ntile = (N + 31) / 32, cap = 2 * (size_t)ncu;
  int best = 1;
  for (int ks = 2; ks <= 2 * K; ks++)
    if ((2 * K) % ks == 0 && ntile * ks <= cap) best = ks;
  return best;
}

int fold_kara_cap() {
  const char *e = getenv("LATTICEUM_AMD_FOLD_KARA");
  if (!e || e[0] < '0' || e[0] > '0' + FOLD_KARA_MAX || e[1]) return FOLD_KARA_MAX;
  return e[0] - '0';
}

hipError_t fold_keys(const uint32_t *smg, size_t ncol, int K, uint32_t *keys, hipStream_t st, uint32_t *nz) {
  if (K < 1 || K > 15) return hipErrorInvalidValue;
  if (!ncol) return hipSuccess;
  hipLaunchKernelGGL(k_pack_keys, dim3(blocks(ncol * 16, 256)), dim3(256), 0, st, smg, ncol, K, keys,
                     nz);
  return hipGetLastError();
}

hipError_t fold_rho_tables(const uint64_t *rho, int nw, uint64_t *rc, uint8_t *tab, int *bad,
                           const ring::NegaTables &inv, int *sync, hipStream_t st, int kara_cap) {
  if (nw < 1 || nw > FC_MAXW || !inv.mid || !sync || kara_cap < 0 || kara_cap > FOLD_KARA_MAX)
    return hipErrorInvalidValue;
  const int per = 2 * RP_WAVES;
  hipLaunchKernelGGL(k_rho_prep, dim3((nw + per - 1) / per), dim3(64 * RP_WAVES), 0, st, rho, nw, rc, tab, bad,
                     inv.mid, sync, kara_cap);
  return hipGetLastError();
}

hipError_t fold_coeff(const uint32_t *keys, const uint8_t *tab, const int *bad, size_t N, int K, uint64_t *f0c,
                      int ncu, hipStream_t st, int32_t *part, const FoldFallback *fb, int L, const uint32_t *nz,
                      int kara_cap) {
  FoldFallback fbv{};
  if (fb) fbv = *fb;
  if (K < 1 || 2 * K > FC_MAXW || ncu < 1 || L < 1 || N % L) return hipErrorInvalidValue;
  if (!N) return hipSuccess;
  const int ks_n = part ? fold_coeff_splits(N, K, ncu) : 1;
  const size_t ntile = (N / L + 31) / 32 * L;
  const size_t ntask = ntile * ks_n, cap = 2 * (size_t)ncu;  // two blocks per CU (LDS 63 KB, 256 registers)
  hipLaunchKernelGGL(k_fold_coeff, dim3((unsigned)(ntask < cap ? ntask : cap)), dim3(256), 0, st, keys, tab, bad, N,
                     K, f0c, ks_n, part, fbv, L, nz);
  if (kara_cap >= 1) {  // gated on bad[1] like the launch above: one of the two returns at once
    const size_t ntask1 = (ntile + 1) / 2 * ks_n;  // one block per CU (LDS 94 KB, 512 registers)
    hipLaunchKernelGGL(k_fold_coeff_kara1, dim3((unsigned)(ntask1 < (size_t)ncu ? ntask1 : (size_t)ncu)), dim3(256),
                       0, st, keys, tab + (size_t)2 * K * FOLD_RT, bad, N, K, f0c, ks_n, part, L, nz);
  }
  if (ks_n > 1) {
    const size_t n = N * FD;
    hipLaunchKernelGGL(k_fold_coeff_sum, dim3(blocks(n / 4, 256)), dim3(256), 0, st, part, ks_n, n, bad,
                       f0c);
  }
  return hipGetLastError();
}

}  // namespace lfk
