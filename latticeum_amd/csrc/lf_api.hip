// lf_api.hip -- the extern "C" boundary (include/lf.h): the context, the twiddle
// tables, the host-buffer wrappers, the thin lf_dev_* wrappers and the RCCL
// communicators. The commit+fold step is in api_step.hip, the sumcheck provers in
// api_sumcheck.hip, the CCS matrices in api_ccs.hip, the persistent memory tree in
// api_memtree.hip; api_internal.hpp holds what they share. No CPU compute fallback
// exists: every ring/commit/fold operation runs on the GPU, and creating a context
// fails loudly without one.
#include <dlfcn.h>

#include <cstdio>
#include <algorithm>
#include <memory>

#include "ajtai_seed.hpp"
#include "api_internal.hpp"

// negacyclic twiddle tables for degree d (built on the host once per context)
int get_tables(lf_ctx *c, int d, Tables *&out) {
  auto it = c->tables.find(d);
  if (it != c->tables.end()) {
    out = &it->second;
    return LF_OK;
  }
  Tables t;
  if (d != 24) {
    // d = 1024: the 32 x 32 NTT middle factors (fwd, inv); d = 4096: those of its
    // 1024-point sub-transforms, then the radix-4 twists (fwd, inv) and the digit
    // butterfly table (kernels_n4k.hip)
    const size_t extra = d == 1024 ? 2048 : d == 4096 ? 2048 + 2 * 4096 + 1024 : 0;
    // d = 1024: then the D8 byte planes of zeta^((2 m1 + 1) j2) for the matrix-core stage 1 (1024 u64);
    // d = 4096: the quarters' stage-1 planes Z''_m0 (4 x 4096 u64) and middle factors (4 x 1024)
    const size_t az_off = 4 * (size_t)d + extra;
    // d = 1024: after the planes, the forward middle factors' limb tables (ring::MID3_U64)
    std::vector<uint64_t> h(az_off + (d == 1024 ? 1024 + ring::MID3_U64 : d == 4096 ? 4 * 4096 + 4 * 1024 : 0));
    const uint64_t psi = gl::pow(7, (gl::P - 1) / (2 * (uint64_t)d));
    const uint64_t psi_inv = gl::inv(psi), w = gl::mul(psi, psi), w_inv = gl::mul(psi_inv, psi_inv);
    const uint64_t dinv = gl::inv((uint64_t)d);
    uint64_t a = 1, b = 1, x = dinv, y = 1;
    for (int j = 0; j < d; j++) {
      h[j] = a;                // psi^j
      h[d + j] = b;            // w^j
      h[2 * d + j] = x;        // d^-1 psi^-j
      h[3 * d + j] = y;        // w^-j
      a = gl::mul(a, psi);
      b = gl::mul(b, w);
      x = gl::mul(x, psi_inv);
      y = gl::mul(y, w_inv);
    }
    // ring.hpp stockham4: omega^(d/4) is the shift 2^48
    if (h[d + d / 4] != gl::mul_pow2(1, 48) || h[3 * d + d / 4] != gl::mul_pow2(1, 144))
      return fail(c, LF_ERR_DEVICE, "unexpected 4th root of unity");
    if (extra) {
      // the 1024-point transform's root: psi itself (d = 1024) or psi^4 (d = 4096)
      const uint64_t p1 = d == 1024 ? psi : gl::pow(psi, 4), p1_inv = gl::inv(p1), q1inv = gl::inv(1024);
      // ntt32.hpp relies on p1^32 = 2^39 and p1^64 = 2^78 (shift-only 32-point stages)
      if (gl::pow(p1, 32) != gl::mul_pow2(1, 39) || gl::pow(p1, 64) != gl::mul_pow2(1, 78))
        return fail(c, LF_ERR_DEVICE, "unexpected root of unity for the 32 x 32 NTT");
      auto brv5 = [](int i) { return ((i & 1) << 4) | ((i & 2) << 2) | (i & 4) | ((i & 8) >> 2) | ((i & 16) >> 4); };
      for (int r = 0; r < 32; r++)
        for (int i = 0; i < 32; i++) {
          // forward: p1^((2 brv5(i) + 1) r);  inverse: 1024^-1 p1^-((2r + 1) brv5(i))
          h[4 * d + r * 32 + i] = gl::pow(p1, (uint64_t)(2 * brv5(i) + 1) * r);
          h[4 * d + 1024 + r * 32 + i] = gl::mul(q1inv, gl::pow(p1_inv, (uint64_t)(2 * r + 1) * brv5(i)));
        }
      if (d == 1024) {
        // az[t][m1][j2] = signed byte t of D8(zeta^((2 m1 + 1) j2)), zeta = p1^32 (frag.hpp d8)
        int8_t *az = reinterpret_cast<int8_t *>(h.data() + az_off);
        const uint64_t zeta = gl::pow(p1, 32);
        for (int m1 = 0; m1 < 32; m1++)
          for (int j2 = 0; j2 < 32; j2++) {
            const uint64_t x = gl::pow(zeta, (uint64_t)(2 * m1 + 1) * j2);
            const uint64_t tt = x <= 0x7F7F7F7F7F7F7F7Full ? x : x + 0xFFFFFFFFull;
            const uint64_t dd = (tt + 0x8080808080808080ull) ^ 0x8080808080808080ull;
            for (int b = 0; b < 8; b++) az[(b * 32 + m1) * 32 + j2] = (int8_t)(uint8_t)(dd >> (8 * b));
          }
        // mid3[g][j1 - 1][m1] = the signed 32-bit limbs (lo | hi << 32) of 2^(24g) p1^((2 m1 + 1) j1), j1 >= 1
        // (gl::mid_limbs; row j1 = 0 is the constant 2^(24g)): the middle factors as k_decompose_fused
        // multiplies them into the grouped byte sums of its matrix-core stage 1
        uint64_t *m3 = h.data() + az_off + 1024;
        for (int g = 0; g < 3; g++)
          for (int j1 = 1; j1 < 32; j1++)
            for (int m1 = 0; m1 < 32; m1++) {
              int32_t lo, hi;
              gl::mid_limbs(h[4 * d + j1 * 32 + brv5(m1)], g, lo, hi);
              m3[(g * 31 + j1 - 1) * 32 + m1] = (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32);
            }
      }
      if (d == 4096) {
        // kernels_n4k.hip relies on psi^1024 = 2^120 (the radix-4 butterflies are shifts)
        if (gl::pow(psi, 1024) != gl::mul_pow2(1, 120)) return fail(c, LF_ERR_DEVICE, "unexpected 8th root of unity");
        uint64_t *tf = h.data() + 4 * d + 2048, *ti = tf + 4096, *zt = ti + 4096;
        const uint64_t inv4 = gl::inv(4);
        for (int m0 = 0; m0 < 4; m0++) {
          const uint64_t s = gl::pow(psi, (uint64_t)((2 * m0 - 3 + 8192) % 8192));  // psi^(2 m0 - 3)
          const uint64_t s_inv = gl::inv(s);
          uint64_t f = 1, g = inv4;
          for (int ai = 0; ai < 1024; ai++) {
            tf[m0 * 1024 + ai] = f;  // psi^((2 m0 - 3) a)
            ti[m0 * 1024 + ai] = g;  // 4^-1 psi^-((2 m0 - 3) a)
            f = gl::mul(f, s);
            g = gl::mul(g, s_inv);
          }
          for (int idx = 0; idx < 256; idx++) {  // sum_b d_b 2^(120 b (2 m0 + 1)), d_b = +-bit_b
            uint64_t z = 0;
            for (int bb = 0; bb < 4; bb++) {
              if (!((idx >> bb) & 1)) continue;
              const uint64_t cb = gl::mul_pow2(1, (120 * bb * (2 * m0 + 1)) % 192);
              z = (idx >> (4 + bb)) & 1 ? gl::sub(z, cb) : gl::add(z, cb);
            }
            zt[m0 * 256 + idx] = z;
          }
        }
        // stage 1 of quarter m0 as one ternary i8 product (tools/ntt4096_mx_model.py): with
        // a = j1 + 32 j2 the twist psi^((2 m0 - 3) a) = s^j1 s^(32 j2), so
        //   Z''_m0[m1][32 b + j2] = zeta^((2 m1 + 1) j2) s^(32 j2) 2^(120 b (2 m0 + 1))
        //   midq[m0][j1][i] = p1^((2 brv5(i) + 1) j1) s^j1
        int8_t *zq = reinterpret_cast<int8_t *>(h.data() + az_off);
        uint64_t *mq = h.data() + az_off + 4 * 4096;
        const uint64_t zeta = gl::pow(p1, 32);
        for (int m0 = 0; m0 < 4; m0++) {
          const uint64_t s = gl::pow(psi, (uint64_t)((2 * m0 - 3 + 8192) % 8192));
          const uint64_t s32 = gl::pow(s, 32);
          for (int m1 = 0; m1 < 32; m1++)
            for (int b = 0; b < 4; b++)
              for (int j2 = 0; j2 < 32; j2++) {
                const uint64_t cb = gl::mul_pow2(1, (120 * b * (2 * m0 + 1)) % 192);
                const uint64_t x = gl::mul(gl::mul(gl::pow(zeta, (uint64_t)(2 * m1 + 1) * j2), gl::pow(s32, j2)), cb);
                const uint64_t tt = x <= 0x7F7F7F7F7F7F7F7Full ? x : x + 0xFFFFFFFFull;
                const uint64_t dd = (tt + 0x8080808080808080ull) ^ 0x8080808080808080ull;
                for (int t = 0; t < 8; t++)
                  zq[(((size_t)m0 * 8 + t) * 32 + m1) * 128 + 32 * b + j2] = (int8_t)(uint8_t)(dd >> (8 * t));
              }
          for (int j1 = 0; j1 < 32; j1++) {
            const uint64_t sj = gl::pow(s, j1);
            for (int i = 0; i < 32; i++) mq[(size_t)m0 * 1024 + j1 * 32 + i] = gl::mul(h[4 * d + j1 * 32 + i], sj);
          }
        }
      }
    }
    LF_HIP(c, hipMalloc(&t.mem, h.size() * 8));
    LF_HIP(c, hipMemcpy(t.mem, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    // d = 1024 / 4096 run the register-resident 32 x 32 NTT kernels (kernels_n32.hip, kernels_n4k.hip)
    const bool n32 = extra != 0;
    t.fwd = {t.mem, t.mem + d, n32 ? t.mem + 4 * d : nullptr};
    if (d == 1024) t.fwd.az = t.mem + az_off;
    t.inv = {t.mem + 2 * d, t.mem + 3 * d, n32 ? t.mem + 4 * d + 1024 : nullptr};
    if (n32 && d == 4096) {
      t.fwd.tw4 = t.mem + 4 * d + 2048;
      t.inv.tw4 = t.fwd.tw4 + 4096;
      t.fwd.ztab = t.inv.tw4 + 4096;
      t.fwd.zq = t.mem + az_off;
      t.fwd.midq = t.mem + az_off + 4 * 4096;
    }
  }
  out = &(c->tables[d] = t);
  return LF_OK;
}

namespace {

bool use_mfma(int d, size_t kappa) {
  // kappa > 32 LF_MAX_KTILES (A tiles of 32 rows): the VALU contraction (k_ajtai_phi72 / k_ajtai_nega)
  return (d == 24 || d % 16 == 0) && lfk::mfma_ktiles(kappa) <= LF_MAX_KTILES;
}
// fragment column order: units of 16 groups at one limb for the GoldiLocksDP
// gadget length L = 5 (what the fused decomposition emits), else natural order
lfk::FragGeom ajtai_geom(size_t ncols) { return lfk::frag_geom(ncols, ncols % 5 == 0 ? 5 : 1); }

// build the MFMA fragment copy of A (scheme creation): 32-row tiles
int ajtai_prepare(lf_ctx *c, lf_ajtai *aj) {
  if (!use_mfma(aj->d, aj->kappa)) return LF_OK;
  aj->geom = ajtai_geom(aj->ncols);
  aj->geom.qperm = aj->d == 4096;  // the slot order kernels_n4k.hip produces
  const size_t n = lfk::frag_elems(aj->geom, aj->d);
  const int ktiles = lfk::mfma_ktiles(aj->kappa);
  LF_HIP(c, hipMalloc((void **)&aj->Af, n * ktiles * sizeof(uint4)));
  for (int t = 0; t < ktiles; t++) {
    lfk::VecPtrs rows{};
    const int r0 = 32 * t, nr = (int)std::min<size_t>(32, aj->kappa - r0);
    for (int i = 0; i < nr; i++) rows.p[i] = aj->A + (size_t)(r0 + i) * aj->ncols * aj->d;
    LF_HIP(c, lfk::to_frag(rows, nr, 0, aj->geom, aj->d, false, aj->Af + n * t, c->cur));
  }
  // the offset form's correction per (row, output slot)
  uint64_t *tmp = nullptr;
  LF_HIP(c, hipMalloc((void **)&aj->kr, lfk::ajtai_rowsums_elems(aj->kappa, aj->d, aj->geom.Lp) * sizeof(uint64_t)));
  LF_HIP(c, hipMalloc((void **)&tmp, aj->kappa * (size_t)aj->d * sizeof(uint64_t)));
  const hipError_t e = lfk::ajtai_rowsums(aj->A, aj->kappa, aj->ncols, aj->d, aj->kr, tmp, c->cur, aj->geom.Lp);
  const hipError_t e2 = hipStreamSynchronize(c->cur);
  (void)hipFree(tmp);
  LF_HIP(c, e);
  LF_HIP(c, e2);
  return LF_OK;
}

int drain_timing(lf_ctx *c) {
  if (c->pending.empty()) return LF_OK;
  LF_HIP(c, hipStreamSynchronize(c->cur));
  for (auto &t : c->pending) {
    float ms = 0;
    LF_HIP(c, hipEventElapsedTime(&ms, t.a, t.b));
    auto &s = c->stats[t.nvec];  // nvec < 0: a phase
    s.first += ms;
    s.second += t.count;
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  c->pending.clear();
  return LF_OK;
}

// ---------------------------------------------------------------- RCCL (resolved at run time)
// The library does not link RCCL: the entry points are looked up in the RCCL
// already loaded into the process (torch's, whose communicators a caller may
// hand over through lf_comm_wrap) or else in librccl.so.1.
struct Rccl {
  bool ok = false;
  std::string err;
  ncclResult_t (*getUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*commInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*commCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*commUserRank)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*allReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                            hipStream_t) = nullptr;
  const char *(*errorString)(ncclResult_t) = nullptr;
};
const Rccl &rccl() {
  static const Rccl r = [] {
    Rccl x;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    for (const char *name : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      x.err = "RCCL (librccl.so.1) not found";
      return x;
    }
    x.getUniqueId = (decltype(x.getUniqueId))dlsym(h, "ncclGetUniqueId");
    x.commInitRank = (decltype(x.commInitRank))dlsym(h, "ncclCommInitRank");
    x.commDestroy = (decltype(x.commDestroy))dlsym(h, "ncclCommDestroy");
    x.commCount = (decltype(x.commCount))dlsym(h, "ncclCommCount");
    x.commUserRank = (decltype(x.commUserRank))dlsym(h, "ncclCommUserRank");
    x.allReduce = (decltype(x.allReduce))dlsym(h, "ncclAllReduce");
    x.errorString = (decltype(x.errorString))dlsym(h, "ncclGetErrorString");
    x.ok = x.getUniqueId && x.commInitRank && x.commDestroy && x.commCount && x.commUserRank && x.allReduce &&
           x.errorString;
    if (!x.ok) x.err = "RCCL entry points missing";
    return x;
  }();
  return r;
}
#define LF_NCCL(ctx, call)                                                                       \
  do {                                                                                          \
    ncclResult_t r_ = (call);                                                                    \
    if (r_ != ncclSuccess)                                                                       \
      return fail((ctx), LF_ERR_COMM, std::string(#call) + ": " + rccl().errorString(r_));       \
  } while (0)
}  // namespace

size_t partial_elems(const lf_ajtai *aj, int nvec) {
  if (aj->Af) return lfk::mfma_scratch_elems(aj->geom, aj->d, aj->kappa, nvec);
  return lfk::ajtai_partial_elems(aj->kappa, aj->ncols, aj->d, nvec);
}

// cm[v] = A f_v for nvec vectors, on the matrix cores when the scheme has fragments
int ajtai_launch(lf_ctx *c, const lf_ajtai *aj, const uint64_t *const *vecs, int nvec, uint64_t *cm) {
  if (nvec < 1 || nvec > LF_MAX_VECS) return fail(c, LF_ERR_INVALID_ARG, "nvec must be in [1, 32]");
  lfk::VecPtrs vp{};
  for (int v = 0; v < nvec; v++) vp.p[v] = vecs[v];
  LF_TRY(grow(c, c->scratch, c->scratch_elems, partial_elems(aj, nvec)));
  if (aj->Af)
    LF_TRY(grow(c, c->frag, c->frag_elems, lfk::frag_elems(aj->geom, aj->d)));
  hipEvent_t a = nullptr, b = nullptr;
  if (c->timing) {
    LF_HIP(c, hipEventCreate(&a));
    LF_HIP(c, hipEventCreate(&b));
  }
  if (aj->Af)
    LF_HIP(c, lfk::ajtai_mfma(aj->Af, aj->kr, aj->kappa, aj->geom, aj->d, vp, nvec, false, c->frag, c->scratch, cm,
                              c->cur, a, b, nullptr, nullptr, c->zero80));
  else
    LF_HIP(c, lfk::ajtai_commit(aj->A, aj->kappa, aj->ncols, aj->d, vp, nvec, c->scratch, cm, c->cur, a, b));
  if (c->timing) c->pending.push_back({a, b, nvec});
  return LF_OK;
}

// x <- sum over the communicator's ranks of x, mod p, on the context stream:
// RCCL's integer sum is mod 2^64, so the vector travels as 32-bit limbs
// (exact for < 2^32 ranks) and is folded back into the field afterwards
int allreduce_modp(lf_ctx *c, lf_comm *cm, uint64_t *x, size_t n) {
  if (!cm || !cm->comm || !n) return LF_OK;  // one rank without a communicator: the sum is x
  if (!rccl().ok) return fail(c, LF_ERR_COMM, rccl().err);
  LF_TRY(grow(c, c->limb, c->limb_elems, 2 * n));
  LF_HIP(c, lfk::limb_split(x, n, c->limb, c->limb + n, c->cur));
  LF_NCCL(c, rccl().allReduce(c->limb, c->limb, 2 * n, ncclUint64, ncclSum, cm->comm, c->cur));
  LF_HIP(c, lfk::limb_join(c->limb, c->limb + n, n, x, c->cur));
  return LF_OK;
}

extern "C" {

lf_params lf_goldilocks_dp(int d) {
  lf_params p;
  p.d = d;
  p.B = 1ull << 15;
  p.L = 5;
  p.b_small = 2;
  p.K = 15;
  return p;
}

int lf_ring_supported(int d) { return ring_ok(d) ? 1 : 0; }

const char *lf_status_string(int s) {
  switch (s) {
    case LF_OK: return "ok";
    case LF_ERR_INVALID_ARG: return "invalid argument";
    case LF_ERR_UNSUPPORTED_RING: return "unsupported ring degree";
    case LF_ERR_WRONG_WITNESS_LENGTH: return "wrong length of the witness";
    case LF_ERR_WRONG_COMMITMENT_LENGTH: return "wrong length of the commitment";
    case LF_ERR_WRONG_AJTAI_DIMENSIONS: return "Ajtai matrix has wrong dimensions";
    case LF_ERR_DECOMPOSITION_OVERFLOW: return "balanced decomposition ran out of digits";
    case LF_ERR_INCORRECT_LENGTH: return "incorrect length";
    case LF_ERR_CHALLENGE_BYTES: return "wrong number of challenge bytes";
    case LF_ERR_DEVICE: return "HIP device error";
    case LF_ERR_OUT_OF_MEMORY: return "out of device memory";
    case LF_ERR_COMM: return "RCCL communicator error";
    case LF_ERR_VERIFICATION: return "the folding proof does not verify";
    case LF_ERR_UNSUPPORTED_CCS: return "unsupported CCS structure";
    case LF_ERR_NOT_SATISFIED: return "the CCS relation is not satisfied";
  }
  return "unknown status";
}

int lf_ctx_create(int device, lf_ctx **out) {
  if (!out) return LF_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
    fprintf(stderr, "latticeum_amd: no HIP device %d available (count=%d)\n", device, n);
    return LF_ERR_DEVICE;
  }
  auto c = std::make_unique<lf_ctx>();
  c->device = device;
  DevGuard g(device);
  if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) return LF_ERR_DEVICE;
  c->cur = c->own;
  if (hipMalloc(&c->d_err, sizeof(int)) != hipSuccess) return LF_ERR_OUT_OF_MEMORY;
  if (hipMemset(c->d_err, 0, sizeof(int)) != hipSuccess) return LF_ERR_DEVICE;
  if (hipMalloc(&c->d_sync, 2 * sizeof(int)) != hipSuccess) return LF_ERR_OUT_OF_MEMORY;
  if (hipMemset(c->d_sync, 0, 2 * sizeof(int)) != hipSuccess) return LF_ERR_DEVICE;
  if (hipMalloc(&c->sink, 4096 * sizeof(uint64_t)) != hipSuccess) return LF_ERR_OUT_OF_MEMORY;
  if (hipMalloc(&c->zero80, 32 * sizeof(uint4)) != hipSuccess) return LF_ERR_OUT_OF_MEMORY;
  if (hipMemset(c->zero80, 0x80, 32 * sizeof(uint4)) != hipSuccess) return LF_ERR_DEVICE;
  if (hipMalloc(&c->toptbl, lfk::TOP_TBL_WORDS * sizeof(uint32_t)) != hipSuccess) return LF_ERR_OUT_OF_MEMORY;
  if (hipMemset(c->toptbl, 0, lfk::TOP_TBL_WORDS * sizeof(uint32_t)) != hipSuccess) return LF_ERR_DEVICE;
  if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->ncu < 1)
    return LF_ERR_DEVICE;
  *out = c.release();
  return LF_OK;
}

// also what a failed lf_ctx_create leaves behind
lf_ctx::~lf_ctx() {
  lf_ctx *c = this;
  DevGuard g(c);
  (void)hipStreamSynchronize(c->cur);
  // a batched contraction this context led on the caller's contract stream reads its buffers
  if (c->contract) (void)hipStreamSynchronize(c->contract);
  c->contract = nullptr;
  for (auto &t : c->pending) {
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  for (auto &kv : c->tables)
    if (kv.second.mem) (void)hipFree(kv.second.mem);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->ybuf) (void)hipFree(c->ybuf);
  if (c->frag) (void)hipFree(c->frag);
  if (c->smg) (void)hipFree(c->smg);
  if (c->fkeys) (void)hipFree(c->fkeys);
  if (c->faux) (void)hipFree(c->faux);
  if (c->fpart) (void)hipFree(c->fpart);
  if (c->sink) (void)hipFree(c->sink);
  if (c->dead) (void)hipFree(c->dead);
  if (c->zero80) (void)hipFree(c->zero80);
  if (c->toptbl) (void)hipFree(c->toptbl);
  if (c->stage) (void)hipFree(c->stage);
  if (c->limb) (void)hipFree(c->limb);
  if (c->tmp) (void)hipFree(c->tmp);
  if (c->sc) (void)hipFree(c->sc);
  if (c->ptrs) (void)hipFree(c->ptrs);
  if (c->sel) (void)hipFree(c->sel);
  if (c->rel) (void)hipFree(c->rel);
  if (c->pwit) (void)hipFree(c->pwit);
  if (c->hmsg) (void)hipHostFree(c->hmsg);
  if (c->mv_host) (void)hipHostFree(c->mv_host);
  if (c->mv_dev) (void)hipFree(c->mv_dev);
  if (c->join) (void)hipEventDestroy(c->join);
  if (c->cjoin) (void)hipEventDestroy(c->cjoin);
  if (c->d_err) (void)hipFree(c->d_err);
  if (c->d_sync) (void)hipFree(c->d_sync);
  if (c->own) (void)hipStreamDestroy(c->own);
}

void lf_ctx_destroy(lf_ctx *c) { delete c; }

const char *lf_ctx_last_error(const lf_ctx *c) { return c ? c->last_error.c_str() : ""; }
void lf_ctx_set_error(lf_ctx *c, const char *msg) {
  if (c) c->last_error = msg ? msg : "";
}

size_t lf_witness_split_w(void) { return lfk::witness_split_w(); }

int lf_ctx_device(const lf_ctx *c) { return c ? c->device : -1; }

int lf_ctx_set_stream(lf_ctx *c, void *s) {
  if (!c) return LF_ERR_INVALID_ARG;
  c->cur = (hipStream_t)s;  // NULL = the HIP default (null) stream, e.g. torch's default stream
  return LF_OK;
}
void *lf_ctx_get_stream(const lf_ctx *c) { return c ? (void *)c->cur : nullptr; }

int lf_stream_create_cu_mask(int device, const uint32_t *mask, int nwords, void **stream) {
  if (!mask || nwords < 1 || !stream) return LF_ERR_INVALID_ARG;
  *stream = nullptr;
  DevGuard g(device);
  hipStream_t s = nullptr;
  if (hipExtStreamCreateWithCUMask(&s, (uint32_t)nwords, mask) != hipSuccess) return LF_ERR_DEVICE;
  *stream = (void *)s;
  return LF_OK;
}
int lf_ctx_set_contract_stream(lf_ctx *c, void *s) {
  if (!c) return LF_ERR_INVALID_ARG;
  if (s) {  // the caller keeps ownership; it must be a stream of this context's device
    hipDevice_t dev = -1;
    if (hipStreamGetDevice((hipStream_t)s, &dev) != hipSuccess)
      return fail(c, LF_ERR_INVALID_ARG, "contract stream: not a valid stream");
    if (dev != c->device) return fail(c, LF_ERR_INVALID_ARG, "contract stream is on another device");
  }
  c->contract = (hipStream_t)s;
  return LF_OK;
}
int lf_ctx_set_cu_count(lf_ctx *c, int ncu) {
  if (!c || ncu < 1) return LF_ERR_INVALID_ARG;
  c->ncu = ncu;
  return LF_OK;
}
int lf_stream_destroy(void *stream) {
  if (!stream) return LF_ERR_INVALID_ARG;
  return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? LF_OK : LF_ERR_DEVICE;
}

int lf_ctx_sync(lf_ctx *c) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_HIP(c, hipStreamSynchronize(c->cur));
  int e = 0;
  LF_HIP(c, hipMemcpy(&e, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
  if (e) {
    LF_HIP(c, hipMemset(c->d_err, 0, sizeof(int)));
    if (e & ~LF_DERR_RHO)
      return fail(c, LF_ERR_DECOMPOSITION_OVERFLOW, "a coefficient needed more digits than padding_size");
    return fail(c, LF_ERR_INVALID_ARG, "lf_dev_fold_planes: a coefficient of rho is outside the short range");
  }
  return LF_OK;
}

// test aid: the not-short flag the last fold_finish left at the tail of faux (it only
// waits and reads; the decomposition-overflow state stays for lf_ctx_sync)
int lf_ctx_fold_flag(lf_ctx *c, int *out) {
  DevGuard g(c);
  if (!c || !out) return LF_ERR_INVALID_ARG;
  LF_HIP(c, hipStreamSynchronize(c->cur));
  *out = -1;
  if (c->fold_flag_at < 0 || !c->faux || (size_t)c->fold_flag_at >= c->faux_elems) return LF_OK;
  int bad = 0;
  LF_HIP(c, hipMemcpy(&bad, c->faux + c->fold_flag_at, sizeof(int), hipMemcpyDeviceToHost));
  *out = bad ? 1 : 0;
  return LF_OK;
}

// test aid: the Karatsuba level the last fold_finish's d = 1024 coefficient-form fold ran
// at (the int beside the not-short flag; 0 when that flag is set); -1 on the paths without one
int lf_ctx_fold_level(lf_ctx *c, int *out) {
  DevGuard g(c);
  if (!c || !out) return LF_ERR_INVALID_ARG;
  LF_HIP(c, hipStreamSynchronize(c->cur));
  *out = -1;
  if (!c->fold_has_level || c->fold_flag_at < 0 || !c->faux || (size_t)c->fold_flag_at >= c->faux_elems) return LF_OK;
  int w[2] = {0, 0};
  LF_HIP(c, hipMemcpy(w, c->faux + c->fold_flag_at, sizeof w, hipMemcpyDeviceToHost));
  *out = w[1];  // 0 when the flag is set
  return LF_OK;
}

int lf_ctx_reserve(lf_ctx *c, size_t kappa, size_t ncols, int d, int nvec) {
  DevGuard g(c);
  if (!c || !ring_ok(d) || nvec < 1 || nvec > LF_MAX_VECS) return LF_ERR_INVALID_ARG;
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  lf_ajtai probe;
  probe.kappa = kappa;
  probe.ncols = ncols;
  probe.d = d;
  if (use_mfma(d, kappa)) {
    probe.Af = reinterpret_cast<uint4 *>(1);  // sizing only
    probe.geom = ajtai_geom(ncols);
    probe.geom.qperm = d == 4096;
    LF_TRY(grow(c, c->frag, c->frag_elems, lfk::frag_elems(probe.geom, d)));
  }
  LF_TRY(grow(c, c->scratch, c->scratch_elems, partial_elems(&probe, nvec)));
  return grow(c, c->ybuf, c->ybuf_elems, (size_t)nvec * kappa * d);
}

int lf_ctx_kernel_timing(lf_ctx *c, int enable) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_TRY(drain_timing(c));
  c->timing = enable != 0;
  c->stats.clear();
  return LF_OK;
}

int lf_ctx_phase_stats(lf_ctx *c, int phase, double *ms, long *count) {
  DevGuard g(c);
  if (!c || !ms || !count || phase < 0 || phase >= LF_PHASE_COUNT) return LF_ERR_INVALID_ARG;
  LF_TRY(drain_timing(c));
  auto it = c->stats.find(-1 - phase);
  *ms = it == c->stats.end() ? 0.0 : it->second.first;
  *count = it == c->stats.end() ? 0 : it->second.second;
  return LF_OK;
}

int lf_ctx_kernel_stats(lf_ctx *c, int nvec, double *ms, long *count) {
  DevGuard g(c);
  if (!c || !ms || !count) return LF_ERR_INVALID_ARG;
  LF_TRY(drain_timing(c));
  *ms = 0;
  *count = 0;
  for (auto &kv : c->stats)
    if (kv.first > 0 && (nvec == 0 || kv.first == nvec)) {
      *ms += kv.second.first;
      *count += kv.second.second;
    }
  return LF_OK;
}

// ---------------------------------------------------------------- host-buffer API
static int xform_host(lf_ctx *c, uint64_t *e, size_t n, int d, int repr, bool fwd) {
  DevGuard g(c);
  if (!c || (!e && n)) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  DevBuf b;
  LF_TRY(upload(c, b, e, n * d, repr));
  LF_HIP(c, lfk::transform(b.p, n, d, fwd, fwd ? t->fwd : t->inv, c->cur));
  LF_TRY(download(c, e, b, n * d, repr));
  return lf_ctx_sync(c);
}
int lf_crt(lf_ctx *c, uint64_t *e, size_t n, int d, int repr) { return xform_host(c, e, n, d, repr, true); }
int lf_icrt(lf_ctx *c, uint64_t *e, size_t n, int d, int repr) { return xform_host(c, e, n, d, repr, false); }

int lf_ring_mul(lf_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n, int d, int repr) {
  DevGuard g(c);
  if (!c || ((!a || !b || !out) && n)) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  DevBuf da, db, dout;
  LF_TRY(upload(c, da, a, n * d, repr));
  LF_TRY(upload(c, db, b, n * d, repr));
  LF_TRY(dev_alloc(c, dout, n * d));
  LF_HIP(c, lfk::slot_mul(da.p, db.p, dout.p, n, d, c->cur));
  LF_TRY(download(c, out, dout, n * d, repr));
  return lf_ctx_sync(c);
}

int lf_ajtai_create(lf_ctx *c, const uint64_t *A, size_t kappa, size_t ncols, int d, int repr,
                    lf_ajtai **out) {
  DevGuard g(c);
  if (!c || !A || !out || !kappa || !ncols) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  DevBuf b;
  LF_TRY(upload(c, b, A, kappa * ncols * d, repr));
  LF_TRY(lf_ctx_sync(c));
  auto *aj = new lf_ajtai;
  aj->device = c->device;
  aj->A = b.p;
  b.p = nullptr;
  aj->owned = true;
  aj->kappa = kappa;
  aj->ncols = ncols;
  aj->d = d;
  int rc = ajtai_prepare(c, aj);
  if (rc != LF_OK) {
    lf_ajtai_destroy(aj);
    return rc;
  }
  *out = aj;
  return LF_OK;
}

int lf_ajtai_create_device(lf_ctx *c, const uint64_t *A_dev, size_t kappa, size_t ncols, int d,
                           lf_ajtai **out) {
  DevGuard g(c);
  if (!c || !A_dev || !out || !kappa || !ncols) return LF_ERR_INVALID_ARG;
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  auto *aj = new lf_ajtai;
  aj->device = c->device;
  aj->A = A_dev;
  aj->kappa = kappa;
  aj->ncols = ncols;
  aj->d = d;
  int rc = ajtai_prepare(c, aj);
  if (rc != LF_OK) {
    lf_ajtai_destroy(aj);
    return rc;
  }
  *out = aj;
  return LF_OK;
}

// A from a seed (lf.h): with the fragment form the generator writes Af and kr
// directly (ajtai_seeded.hip) and aj->A stays null -- nothing reads it on such a
// scheme; without it the u64 window is generated, owned, and the scheme is what
// lf_ajtai_create makes
int lf_ajtai_create_seeded(lf_ctx *c, const uint64_t seed[4], int kind, size_t kappa, size_t ncols_total,
                           size_t col0, size_t ncols, int d, lf_ajtai **out) {
  DevGuard g(c);
  if (!c || !out) return LF_ERR_INVALID_ARG;
  const char *why;
  const int rc0 = lfk::seed_check(seed, kind, kappa, ncols_total, d, col0, ncols, &why);
  if (rc0 != LF_OK) return fail(c, rc0, why);
  const lfk::SeedGen sg{{seed[0], seed[1], seed[2], seed[3]}, kind, d, ncols_total};
  std::unique_ptr<lf_ajtai, void (*)(lf_ajtai *)> aj(new lf_ajtai, lf_ajtai_destroy);
  aj->device = c->device;
  aj->kappa = kappa;
  aj->ncols = ncols;
  aj->d = d;
  if (use_mfma(d, kappa)) {
    aj->geom = ajtai_geom(ncols);
    aj->geom.qperm = d == 4096;
    const size_t n = lfk::frag_elems(aj->geom, d);
    LF_HIP(c, hipMalloc((void **)&aj->Af, n * lfk::mfma_ktiles(kappa) * sizeof(uint4)));
    LF_HIP(c, hipMalloc((void **)&aj->kr, lfk::ajtai_rowsums_elems(kappa, d, aj->geom.Lp) * sizeof(uint64_t)));
    DevBuf part;
    LF_TRY(dev_alloc(c, part, lfk::seeded_frag_scratch_elems(kappa, d, aj->geom)));
    LF_HIP(c, lfk::seeded_to_frag(sg, kappa, col0, aj->geom, aj->Af, aj->kr, part.p, c->cur));
    LF_HIP(c, hipStreamSynchronize(c->cur));
  } else {
    uint64_t *A = nullptr;
    LF_HIP(c, hipMalloc((void **)&A, kappa * ncols * (size_t)d * sizeof(uint64_t)));
    aj->A = A;
    aj->owned = true;
    LF_HIP(c, lfk::seeded_expand(sg, 0, kappa, col0, ncols, A, c->cur));
    LF_HIP(c, hipStreamSynchronize(c->cur));
  }
  *out = aj.release();
  return LF_OK;
}

int lf_dev_ajtai_seeded_expand(lf_ctx *c, const uint64_t seed[4], int kind, size_t kappa, size_t ncols_total, int d,
                               size_t row0, size_t nrows, size_t col0, size_t ncols, uint64_t *out_dev) {
  DevGuard g(c);
  if (!c || !out_dev) return LF_ERR_INVALID_ARG;
  const char *why;
  const int rc0 = lfk::seed_check(seed, kind, kappa, ncols_total, d, col0, ncols, &why);
  if (rc0 != LF_OK) return fail(c, rc0, why);
  if (!nrows || row0 > kappa || nrows > kappa - row0) return fail(c, LF_ERR_INVALID_ARG, "row0 + nrows exceeds kappa");
  if ((uintptr_t)out_dev % 16) return fail(c, LF_ERR_INVALID_ARG, "out_dev must be 16-byte aligned");
  const lfk::SeedGen sg{{seed[0], seed[1], seed[2], seed[3]}, kind, d, ncols_total};
  LF_HIP(c, lfk::seeded_expand(sg, row0, nrows, col0, ncols, out_dev, c->cur));
  return LF_OK;
}

size_t lf_ajtai_device_bytes(const lf_ajtai *aj) {
  if (!aj) return 0;
  size_t b = aj->owned && aj->A ? aj->kappa * aj->ncols * (size_t)aj->d * sizeof(uint64_t) : 0;
  if (aj->Af) b += lfk::frag_elems(aj->geom, aj->d) * lfk::mfma_ktiles(aj->kappa) * sizeof(uint4);
  if (aj->kr) b += lfk::ajtai_rowsums_elems(aj->kappa, aj->d, aj->geom.Lp) * sizeof(uint64_t);
  return b;
}

void lf_ajtai_destroy(lf_ajtai *aj) {
  if (!aj) return;
  DevGuard g(aj->device);
  if (aj->owned) (void)hipFree((void *)aj->A);
  if (aj->Af) (void)hipFree(aj->Af);
  if (aj->kr) (void)hipFree(aj->kr);
  delete aj;
}
size_t lf_ajtai_kappa(const lf_ajtai *aj) { return aj ? aj->kappa : 0; }
size_t lf_ajtai_width(const lf_ajtai *aj) { return aj ? aj->ncols : 0; }
int lf_ajtai_d(const lf_ajtai *aj) { return aj ? aj->d : 0; }
int lf_ajtai_layout(const lf_ajtai *aj) { return aj && aj->Af ? 1 : 0; }

int lf_ajtai_commit(lf_ctx *c, const lf_ajtai *aj, const uint64_t *f, size_t f_len, uint64_t *cm, int repr) {
  DevGuard g(c);
  if (!c || !aj || !f || !cm) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  if (f_len != aj->ncols)  // commitment_scheme.rs:38-43
    return fail(c, LF_ERR_WRONG_WITNESS_LENGTH, "Wrong length of the witness");
  DevBuf df, dcm;
  LF_TRY(upload(c, df, f, f_len * aj->d, repr));
  LF_TRY(dev_alloc(c, dcm, aj->kappa * aj->d));
  const uint64_t *v = df.p;
  LF_TRY(ajtai_launch(c, aj, &v, 1, dcm.p));
  LF_TRY(download(c, cm, dcm, aj->kappa * aj->d, repr));
  return lf_ctx_sync(c);
}

int lf_witness_from_w_ccs(lf_ctx *c, const lf_params *pr, const uint64_t *w, size_t W, uint64_t *fc,
                          uint64_t *f, int repr) {
  DevGuard g(c);
  if (!c || (!w && W) || !fc || !f) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  const int d = pr->d;
  const size_t N = W * pr->L;
  DevBuf dw, dfc, df;
  LF_TRY(upload(c, dw, w, W * d, repr));
  LF_TRY(dev_alloc(c, dfc, N * d));
  LF_TRY(dev_alloc(c, df, N * d));
  LF_TRY(lf_dev_witness_from_w_ccs(c, pr, dw.p, W, dfc.p, df.p));
  LF_TRY(download(c, fc, dfc, N * d, repr));
  LF_TRY(download(c, f, df, N * d, repr));
  return lf_ctx_sync(c);
}

int lf_witness_from_f(lf_ctx *c, const lf_params *pr, const uint64_t *f, size_t N, uint64_t *fc,
                      uint64_t *w, int repr) {
  DevGuard g(c);
  if (!c || (!f && N) || !fc || !w) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  const int d = pr->d;
  DevBuf df, dfc, dw;
  LF_TRY(upload(c, df, f, N * d, repr));
  LF_TRY(dev_alloc(c, dfc, N * d));
  LF_TRY(dev_alloc(c, dw, N / pr->L * d));
  LF_TRY(lf_dev_witness_from_f(c, pr, df.p, N, dfc.p, dw.p));
  LF_TRY(download(c, fc, dfc, N * d, repr));
  LF_TRY(download(c, w, dw, N / pr->L * d, repr));
  return lf_ctx_sync(c);
}

int lf_decompose_witness(lf_ctx *c, const lf_params *pr, const uint64_t *fc, size_t N, uint64_t *fck,
                         uint64_t *fk, uint64_t *wk, int repr) {
  DevGuard g(c);
  if (!c || (!fc && N) || !fck || !fk || !wk) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  const int d = pr->d, K = pr->K;
  DevBuf dfc, dfck, dfk, dwk;
  LF_TRY(upload(c, dfc, fc, N * d, repr));
  LF_TRY(dev_alloc(c, dfck, K * N * d));
  LF_TRY(dev_alloc(c, dfk, K * N * d));
  LF_TRY(dev_alloc(c, dwk, K * (N / pr->L) * d));
  LF_TRY(lf_dev_decompose_witness(c, pr, dfc.p, N, dfck.p, dfk.p, dwk.p));
  LF_TRY(download(c, fck, dfck, K * N * d, repr));
  LF_TRY(download(c, fk, dfk, K * N * d, repr));
  LF_TRY(download(c, wk, dwk, K * (N / pr->L) * d, repr));
  return lf_ctx_sync(c);
}
int lf_short_challenge(const uint8_t *bs, size_t nbytes, int d, uint64_t *coeffs) {
  // cyclotomic-rings rings/goldilocks.rs:41-67 (3 bytes -> 4 six-bit coefficients - 32)
  if (!bs || !coeffs || d % 4) return LF_ERR_INVALID_ARG;
  if (nbytes != (size_t)(3 * d / 4)) return LF_ERR_CHALLENGE_BYTES;
  for (int i = 0; i < d / 4; i++) {
    int x[4];
    x[0] = (bs[3 * i] & 0x3f) - 32;
    x[1] = (((bs[3 * i] & 0xc0) >> 6) | ((bs[3 * i + 1] & 0x0f) << 2)) - 32;
    x[2] = (((bs[3 * i + 1] & 0xf0) >> 4) | ((bs[3 * i + 2] & 0x03) << 4)) - 32;
    x[3] = ((bs[3 * i + 2] & 0xfc) >> 2) - 32;
    for (int k = 0; k < 4; k++) coeffs[4 * i + k] = x[k] < 0 ? gl::P - (uint64_t)(-x[k]) : (uint64_t)x[k];
  }
  return LF_OK;
}

int lf_poseidon2_permute(lf_ctx *c, uint64_t *states, size_t n) {
  DevGuard g(c);
  if (!c || (!states && n)) return LF_ERR_INVALID_ARG;
  DevBuf b;
  LF_TRY(upload(c, b, states, 16 * n, LF_REPR_CANONICAL));
  LF_HIP(c, lfk::p2_permute(b.p, n, c->cur));
  LF_TRY(download(c, states, b, 16 * n, LF_REPR_CANONICAL));
  return lf_ctx_sync(c);
}

// ---------------------------------------------------------------- device API
int lf_dev_crt(lf_ctx *c, uint64_t *e, size_t n, int d) {
  DevGuard g(c);
  if (!c || (!e && n)) return LF_ERR_INVALID_ARG;
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  LF_HIP(c, lfk::transform(e, n, d, true, t->fwd, c->cur));
  return LF_OK;
}
int lf_dev_icrt(lf_ctx *c, uint64_t *e, size_t n, int d) {
  DevGuard g(c);
  if (!c || (!e && n)) return LF_ERR_INVALID_ARG;
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  LF_HIP(c, lfk::transform(e, n, d, false, t->inv, c->cur));
  return LF_OK;
}
int lf_dev_ring_mul(lf_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n, int d) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  LF_HIP(c, lfk::slot_mul(a, b, out, n, d, c->cur));
  return LF_OK;
}
int lf_dev_to_montgomery(lf_ctx *c, uint64_t *x, size_t n) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_HIP(c, lfk::mont(x, n, true, c->cur));
  return LF_OK;
}
int lf_dev_from_montgomery(lf_ctx *c, uint64_t *x, size_t n) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_HIP(c, lfk::mont(x, n, false, c->cur));
  return LF_OK;
}
int lf_dev_witness_from_w_ccs(lf_ctx *c, const lf_params *pr, const uint64_t *w, size_t W, uint64_t *fc,
                              uint64_t *f) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  Tables *t;
  LF_TRY(get_tables(c, pr->d, t));
  LF_HIP(c, lfk::from_w_ccs(w, W, pr->d, lb, pr->L, fc, f, t->fwd, t->inv, c->d_err, c->cur));
  return LF_OK;
}
int lf_dev_witness_from_f(lf_ctx *c, const lf_params *pr, const uint64_t *f, size_t N, uint64_t *fc,
                          uint64_t *w) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  Tables *t;
  LF_TRY(get_tables(c, pr->d, t));
  LF_HIP(c, lfk::from_f(f, N, pr->d, lb, pr->L, fc, w, t->inv, c->cur));
  return LF_OK;
}
int lf_dev_ajtai_commit(lf_ctx *c, const lf_ajtai *aj, const uint64_t *const *vecs, int nvec, uint64_t *cm) {
  DevGuard g(c);
  if (!c || !aj || !vecs || !cm) return LF_ERR_INVALID_ARG;
  return ajtai_launch(c, aj, vecs, nvec, cm);
}
int lf_dev_commit_y0(lf_ctx *c, const lf_params *pr, const uint64_t *cm, uint64_t *y, size_t kappa) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  LF_HIP(c, lfk::commit_y0(cm, y, kappa, pr->d, lbs, pr->K, c->cur));
  return LF_OK;
}
int lf_dev_fold(lf_ctx *c, int d, const uint64_t *rho, const uint64_t *const *x, int nwit, size_t n,
                uint64_t *out) {
  DevGuard g(c);
  if (!c || !rho || !x || !out || nwit < 1 || nwit > LF_MAX_VECS) return LF_ERR_INVALID_ARG;
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  lfk::VecPtrs vp{};
  for (int i = 0; i < nwit; i++) vp.p[i] = x[i];
  LF_HIP(c, lfk::fold(rho, vp, nwit, n, d, out, c->cur));
  return LF_OK;
}
int lf_dev_fold_lcccs(lf_ctx *c, int d, int nwit, const uint64_t *rho, const uint64_t *rho_coeff, const uint64_t *eta,
                      size_t t, const uint64_t *xwh, size_t l1, const uint64_t *theta, uint64_t *u0, uint64_t *x0,
                      uint64_t *v0) {
  if (!c || nwit < 1 || nwit > LF_MAX_VECS || !rho) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  if ((t && (!eta || !u0)) || (l1 && (!xwh || !x0)) || (!rho_coeff != !theta) || (theta && !v0))
    return fail(c, LF_ERR_INVALID_ARG, "missing buffer");
  lfk::VecPtrs ve{}, vx{};
  for (int i = 0; i < nwit; i++) {
    ve.p[i] = eta + (size_t)i * t * d;
    vx.p[i] = xwh + (size_t)i * l1 * d;
  }
  // u_0 = sum rho_i eta_i (folding/utils.rs:478-496), x_0 = sum rho_i (x_w || h)_i (:498-514)
  if (t) LF_HIP(c, lfk::fold(rho, ve, nwit, t, d, u0, c->cur));
  if (l1) LF_HIP(c, lfk::fold(rho, vx, nwit, l1, d, x0, c->cur));
  // v_0 = rot_lin_combination(rho_s_coeff, theta_s) (:466)
  if (theta) LF_HIP(c, lfk::rot_lin(rho_coeff, theta, nwit, d, v0, c->cur));
  return LF_OK;
}

int lf_fold_lcccs(lf_ctx *c, int d, int nwit, const uint64_t *rho, const uint64_t *rho_coeff, const uint64_t *eta,
                  size_t t, const uint64_t *xwh, size_t l1, const uint64_t *theta, uint64_t *u0, uint64_t *x0,
                  uint64_t *v0, int repr) {
  if (!c || nwit < 1 || nwit > LF_MAX_VECS || !rho) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(check_repr(c, repr));
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  const size_t tau = d == 24 ? 3 : 1, n = (size_t)nwit;
  DevBuf drho, drc, deta, dx, dth, du, dx0, dv;
  LF_TRY(upload(c, drho, rho, n * d, repr));
  if (t) {
    LF_TRY(upload(c, deta, eta, n * t * d, repr));
    LF_TRY(dev_alloc(c, du, t * d));
  }
  if (l1) {
    LF_TRY(upload(c, dx, xwh, n * l1 * d, repr));
    LF_TRY(dev_alloc(c, dx0, l1 * d));
  }
  if (theta) {
    LF_TRY(upload(c, drc, rho_coeff, n * d, repr));
    LF_TRY(upload(c, dth, theta, n * tau * d, repr));
    LF_TRY(dev_alloc(c, dv, tau * d));
  }
  LF_TRY(lf_dev_fold_lcccs(c, d, nwit, drho.p, drc.p, deta.p, t, dx.p, l1, dth.p, du.p, dx0.p, dv.p));
  if (t) LF_TRY(download(c, u0, du, t * d, repr));
  if (l1) LF_TRY(download(c, x0, dx0, l1 * d, repr));
  if (theta) LF_TRY(download(c, v0, dv, tau * d, repr));
  return lf_ctx_sync(c);
}

// compute_x_s = w_ccs_k of decompose_witness(Witness::from_w_ccs(x).f_coeff):
// gadget_decompose(ICRT(x)), its b_small digit planes, each plane recomposed
// over the L limbs with B and CRT'd -- decompose_big_vec_into_k_vec_and_compose_back
// (decomposition/utils.rs:12-42), the same arithmetic (CRT is linear)
int lf_dev_compute_x_s(lf_ctx *c, const lf_params *pr, const uint64_t *x, size_t m, uint64_t *x_s) {
  if (!c || (!x && m) || (!x_s && m)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (!m) return LF_OK;
  const int d = pr->d, L = pr->L, K = pr->K;
  const size_t N = m * L;
  LF_TRY(grow(c, c->tmp, c->tmp_elems, (2 + 2 * (size_t)K) * N * d));
  uint64_t *fc = c->tmp, *f = fc + N * d, *fck = f + N * d, *fk = fck + (size_t)K * N * d;
  LF_TRY(lf_dev_witness_from_w_ccs(c, pr, x, m, fc, f));
  return lf_dev_decompose_witness(c, pr, fc, N, fck, fk, x_s);
}

int lf_compute_x_s(lf_ctx *c, const lf_params *pr, const uint64_t *x, size_t m, uint64_t *x_s, int repr) {
  if (!c || (!x && m) || (!x_s && m)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(check_repr(c, repr));
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  DevBuf dx, ds;
  LF_TRY(upload(c, dx, x, m * pr->d, repr));
  LF_TRY(dev_alloc(c, ds, (size_t)pr->K * m * pr->d));
  LF_TRY(lf_dev_compute_x_s(c, pr, dx.p, m, ds.p));
  LF_TRY(download(c, x_s, ds, (size_t)pr->K * m * pr->d, repr));
  return lf_ctx_sync(c);
}
// ---------------------------------------------------------------- width-8 Poseidon2 Merkle trees
int lf_dev_poseidon2_w8_permute(lf_ctx *c, uint64_t *states, size_t n) {
  if (!c || (!states && n)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_HIP(c, lfk::p2w8_permute(states, n, c->cur));
  return LF_OK;
}

size_t lf_merkle_nodes_len(size_t nrows) { return nrows ? lfk::merkle_nodes(nrows) : 0; }

int lf_dev_merkle_tree(lf_ctx *c, const uint64_t *rows, size_t nrows, size_t width, uint64_t *nodes) {
  if (!c || !rows || !nodes || !width || !nrows)
    return c ? fail(c, LF_ERR_INVALID_ARG, "Merkle tree: at least one row of width >= 1") : LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_HIP(c, lfk::merkle_tree(rows, nrows, width, nodes, c->cur));
  return LF_OK;
}

int lf_dev_hash_w8_rows(lf_ctx *c, const uint64_t *rows, size_t nrows, size_t width, uint64_t *out) {
  if (!c || (nrows && (!out || (width && !rows)))) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_HIP(c, lfk::hash_w8_rows(rows, nrows, width, out, c->cur));
  return LF_OK;
}

int lf_merkle_open(lf_ctx *c, const uint64_t *nodes, size_t nrows, size_t index, uint64_t *path) {
  if (!c || !nodes || !path || !nrows || index >= nrows) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  // the sibling of the node on the path in every padded layer below the root,
  // leaves first (open_batch's opening_proof; a zero digest where the layer was padded)
  size_t off = 0, n = nrows <= 1 ? 1 : nrows + nrows % 2, i = index, k = 0;
  while (n > 1) {
    LF_HIP(c, hipMemcpyAsync(path + 4 * k, nodes + 4 * (off + (i ^ 1)), 32, hipMemcpyDeviceToHost, c->cur));
    off += n;
    n = n == 2 ? 1 : ((n / 2 + 1) & ~(size_t)1);
    i /= 2;
    k++;
  }
  LF_HIP(c, hipStreamSynchronize(c->cur));
  return LF_OK;
}

size_t lf_merkle_path_len(size_t nrows) { return (size_t)lfk::merkle_depth(nrows); }

int lf_dev_merkle_verify(lf_ctx *c, const uint64_t *rows, size_t k, size_t width, size_t nrows, const uint32_t *index,
                         const uint64_t *paths, const uint64_t *roots, int one_root, uint8_t *ok) {
  if (!c) return LF_ERR_INVALID_ARG;
  if (!k) return LF_OK;
  if (!rows || !index || !roots || !ok || !width || !nrows || (nrows > 1 && !paths) || k > ((size_t)1 << 28))
    return fail(c, LF_ERR_INVALID_ARG,
                "Merkle verify: at most 2^28 rows of width >= 1 from a tree of at least one row");
  DevGuard g(c);
  LF_HIP(c, lfk::merkle_verify(rows, k, k, width, nrows, index, paths, roots, one_root != 0, ok, c->cur));
  return LF_OK;
}

int lf_vm_code_comm(lf_ctx *c, const uint8_t *code, size_t len, uint64_t out4[4]) {
  if (!c || !out4 || (len && !code)) return LF_ERR_INVALID_ARG;
  if (!len) return fail(c, LF_ERR_INVALID_ARG, "vm_code_comm: empty code (the reference asserts)");
  DevGuard g(c);
  // little-endian 16-bit half-words, an odd last byte padded with zero (commitments.rs:316-328)
  const size_t nh = (len + 1) / 2;
  std::vector<uint64_t> hw(nh);
  for (size_t i = 0; i < nh; i++) hw[i] = code[2 * i] | (2 * i + 1 < len ? (uint64_t)code[2 * i + 1] << 8 : 0);
  DevBuf dr, dn;
  LF_TRY(upload(c, dr, hw.data(), nh, LF_REPR_CANONICAL));
  const size_t nn = lfk::merkle_nodes(nh);
  LF_TRY(dev_alloc(c, dn, 4 * nn));
  LF_HIP(c, lfk::merkle_tree(dr.p, nh, 1, dn.p, c->cur));
  LF_HIP(c, hipMemcpyAsync(out4, dn.p + 4 * (nn - 1), 32, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  return LF_OK;
}
// ---------------------------------------------------------------- communicators
int lf_comm_unique_id(uint8_t *id, size_t len) {
  if (!id || len != NCCL_UNIQUE_ID_BYTES) return LF_ERR_INVALID_ARG;
  if (!rccl().ok) return LF_ERR_COMM;
  ncclUniqueId u;
  if (rccl().getUniqueId(&u) != ncclSuccess) return LF_ERR_COMM;
  memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return LF_OK;
}

int lf_comm_init(lf_ctx *c, int nranks, int rank, const uint8_t *id, size_t len, lf_comm **out) {
  if (!c || !out || nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !id) ||
      (id && len != NCCL_UNIQUE_ID_BYTES))
    return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  *out = nullptr;
  auto cm = std::make_unique<lf_comm>();
  cm->nranks = nranks;
  cm->rank = rank;
  if (id) {  // one rank with an id still makes a (trivial) RCCL communicator
    if (!rccl().ok) return fail(c, LF_ERR_COMM, rccl().err);
    ncclUniqueId u;
    memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    LF_NCCL(c, rccl().commInitRank(&cm->comm, nranks, u, rank));
    cm->owned = true;
  }
  *out = cm.release();
  return LF_OK;
}

int lf_comm_wrap(lf_ctx *c, void *nccl_comm, lf_comm **out) {
  if (!c || !nccl_comm || !out) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!rccl().ok) return fail(c, LF_ERR_COMM, rccl().err);
  auto cm = std::make_unique<lf_comm>();
  cm->comm = (ncclComm_t)nccl_comm;
  LF_NCCL(c, rccl().commCount(cm->comm, &cm->nranks));
  LF_NCCL(c, rccl().commUserRank(cm->comm, &cm->rank));
  *out = cm.release();
  return LF_OK;
}

void lf_comm_destroy(lf_comm *cm) {
  if (!cm) return;
  if (cm->owned && cm->comm && rccl().ok) (void)rccl().commDestroy(cm->comm);
  delete cm;
}
int lf_comm_size(const lf_comm *cm) { return cm ? cm->nranks : 0; }
int lf_comm_rank(const lf_comm *cm) { return cm ? cm->rank : -1; }

int lf_comm_allreduce_modp(lf_ctx *c, lf_comm *cm, uint64_t *x, size_t n) {
  if (!c || !cm || (!x && n)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  return allreduce_modp(c, cm, x, n);
}

int lf_fold_reduce_allranks(lf_ctx *c, lf_comm *cm, uint64_t *cm0, size_t cm0_len, uint64_t *f0, size_t f0_len) {
  if (!c || !cm) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(allreduce_modp(c, cm, cm0, cm0_len));
  return allreduce_modp(c, cm, f0, f0_len);
}

int lf_dev_poseidon2_permute(lf_ctx *c, uint64_t *states, size_t n) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_HIP(c, lfk::p2_permute(states, n, c->cur));
  return LF_OK;
}

int lf_dev_poseidon2_permute_rounds(lf_ctx *c, uint64_t *states, size_t n, int rounds) {
  if (!c || (!states && n) || rounds < 0 || rounds > 30) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_HIP(c, lfk::p2_permute(states, n, c->cur, rounds));
  return LF_OK;
}
int lf_dev_fill_uniform(lf_ctx *c, uint64_t *out, size_t n, uint64_t seed) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_HIP(c, lfk::fill_uniform(out, n, seed, c->cur));
  return LF_OK;
}
int lf_dev_modp_sum(lf_ctx *c, const uint64_t *in, int nparts, size_t len, uint64_t *out) {
  DevGuard g(c);
  if (!c || nparts < 1) return LF_ERR_INVALID_ARG;
  LF_HIP(c, lfk::modp_sum(in, nparts, len, out, c->cur));
  return LF_OK;
}

int lf_dev_limb_split(lf_ctx *c, const uint64_t *x, size_t n, uint64_t *lo, uint64_t *hi) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_HIP(c, lfk::limb_split(x, n, lo, hi, c->cur));
  return LF_OK;
}
int lf_dev_limb_join(lf_ctx *c, const uint64_t *lo, const uint64_t *hi, size_t n, uint64_t *out) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  LF_HIP(c, lfk::limb_join(lo, hi, n, out, c->cur));
  return LF_OK;
}

}  // extern "C"
