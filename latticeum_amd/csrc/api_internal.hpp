// api_internal.hpp -- what the files behind the extern "C" boundary share
// (lf_api.hip, api_step.hip, api_sumcheck.hip, api_ccs.hip, api_memtree.hip, fold_prove.hip): the
// context and the other handles, the error / scratch / host-buffer helpers, and
// the two transcript steps every Fiat-Shamir loop is made of.
// The device error word (lf_ctx::d_err): bit 0 = a decomposition overflowed (digits.hpp
// raise), bit 1 = lf_dev_fold_planes was given a rho that is not short (LF_DERR_RHO).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the RCCL entry points are resolved at run time (lf_api.hip rccl())

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/lf.h"
#include "gl.hpp"
#include "kernels.hpp"
#include "launch.hpp"

constexpr int LF_DERR_RHO = 2;

struct Tables {
  uint64_t *mem = nullptr;  // 4*d u64: fwd twist | fwd roots | inv twist | inv roots
  ring::NegaTables fwd{}, inv{};
};

struct TimedLaunch {
  hipEvent_t a, b;
  int nvec;       // Ajtai launches: vectors per launch; phases: -1 - LF_PHASE_*
  int count = 1;  // steps the launch covers (a batched contraction: every step's share)
};

// How fold_finish makes f_0. fold_commit decides it once per step (api_step.hip
// step_plan, then what the decomposition reports) and leaves it in the context,
// where it survives between API calls: lf_dev_fold_step_partial -> _finish,
// lf_dev_decompose_commit -> lf_dev_fold_combine, the batch's commit loop -> finish loop.
enum class FoldPath {
  Ntt,            // NTT-form fold from the f_k rows
  Rows,           // NTT-form fold from the operand rows (a step without f_k buffers)
  Coeff1024,      // d = 1024: coefficient-form fold from the packed digits
  Coeff1024Rows,  // the same on packed planes: a rho that is not short folds from the operand rows in that launch
  CoeffPow2,      // d = 16 .. 512 without f_k: coefficient-form fold from the packed words, the operand rows for such a rho
  Masks24,        // Phi_72: coefficient-form fold from the digit masks, f_k rows for a rho that is not short
  Masks24Packed,  // the same on packed planes: such a rho folds from the masks in Z_p
};
struct StepState {
  FoldPath path = FoldPath::Ntt;
  size_t N = 0;                                // the witness length the state was made for
  uint32_t *smg_side[2] = {nullptr, nullptr};  // Coeff1024*, CoeffPow2: both sides' packed words (the caller's planes, or smg)
  const uint2 *masks24[2] = {nullptr, nullptr};  // Masks24*: both sides' digit masks (fkeys or the caller's planes)
  lfk::FoldRows fold_rows{};    // Rows, Coeff1024Rows, CoeffPow2: where the 2K planes sit in the operand rows
  lfk::DeadUnits dead_units{};  // the fused decomposition's flags (what the readers of c->frag honour)
};

struct lf_ctx {
  int device = 0;
  hipStream_t own = nullptr, cur = nullptr;
  int *d_err = nullptr;
  int *d_sync = nullptr;        // two ints, zero between launches (k_rho_prep's cross-block flag)
  std::string last_error;
  std::map<int, Tables> tables;
  uint64_t *scratch = nullptr;  // Ajtai split partial sums
  size_t scratch_elems = 0;
  uint64_t *ybuf = nullptr;     // batched commitments before they are scattered to y / cm
  size_t ybuf_elems = 0;
  uint4 *frag = nullptr;        // vectors in MFMA fragment order (ajtai_mfma.hip)
  size_t frag_elems = 0;
  uint32_t *smg = nullptr;      // packed coefficients for the fused decomposition
  size_t smg_elems = 0;
  uint32_t *fkeys = nullptr;    // coefficient-form fold: digit keys [2 N][K][64] (fold_coeff.hip)
  size_t fkeys_elems = 0;
  uint64_t *faux = nullptr;     // coefficient-form fold: rho coefficients, byte tables, the not-short flag
  int32_t *fpart = nullptr;     // coefficient-form fold with few elements: per witness-split partial sums
  size_t fpart_elems = 0;
  size_t faux_elems = 0;
  long fold_flag_at = -1;       // the last fold_finish's not-short flag: its u64 index in faux, -1 = a path without one
  bool fold_has_level = false;  // that u64's second int is the Karatsuba level that ran (lf_ctx_fold_level)
  uint64_t *sink = nullptr;     // 32 KiB row the fused decompositions store work past the end into
  uint8_t *dead = nullptr;      // dead-unit flags of the operand rows (lfk::DeadUnits) [2 nch][32]
  size_t dead_elems = 0;
  uint4 *zero80 = nullptr;      // 32 operand pieces of 0x80 bytes: the offset form of 0 (dead units)
  uint32_t *toptbl = nullptr;   // the batched contraction's top-class (step, row) list (lfk::TOP_TBL_WORDS)
  StepState step{};             // the last fold_commit's fold path and what it reads
  int ncu = 0;                  // compute units of `device`
  uint64_t *stage = nullptr;    // sharded step: the partial commitments [nvec][kappa d]
  size_t stage_elems = 0;
  uint64_t *limb = nullptr;     // RCCL transport: [lo | hi] 32-bit limbs of a field vector
  size_t limb_elems = 0;
  uint64_t *tmp = nullptr;      // small intermediates (compute_x_s)
  size_t tmp_elems = 0;
  uint64_t *sc = nullptr;       // sumcheck: fixed MLEs of the next round, round partial sums, weights
  size_t sc_elems = 0;
  uint64_t *ptrs = nullptr;     // lf_sumcheck_prove_ptrs: the MLE pointer table
  size_t ptrs_elems = 0;
  int *sel = nullptr;           // lf_dev_mz_mles_sel: the selected matrices
  size_t sel_elems = 0;
  uint64_t *rel = nullptr;      // relation checks: the first unsatisfied row per z, the norm
  size_t rel_elems = 0;
  uint64_t *pwit = nullptr;     // lf_dev_planes_witness: the outputs the caller does not take ([N][d] words each)
  size_t pwit_elems = 0;
  uint64_t *hmsg = nullptr;     // pinned host staging of the sumcheck round messages
  size_t hmsg_elems = 0;
  uint8_t *mv_host = nullptr;   // lf_memtree_verify / lf_memtree_audit: one chunk's pinned staging
  uint8_t *mv_dev = nullptr;    // and its device copy, status bytes included
  size_t mv_bytes = 0;
  bool timing = false;
  hipEvent_t join = nullptr;    // lf_dev_fold_step_batch: this stream's point to wait for / be waited on
  hipStream_t contract = nullptr;  // lf_ctx_set_contract_stream: where batched contractions led by this context run
  hipEvent_t cjoin = nullptr;   // the end of the last such contraction
  std::vector<TimedLaunch> pending;
  std::map<int, std::pair<double, long>> stats;  // nvec -> (ms, count)
  ~lf_ctx();  // lf_api.hip: everything above, on `device`
};

// Every entry point runs on its context's device and restores the caller's
// current device afterwards (also from destructors), so contexts on different
// GPUs can be used from one thread (lf.h threading contract).
struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    int cur = -1;
    if (dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
  }
  explicit DevGuard(const lf_ctx *c) : DevGuard(c ? c->device : -1) {}
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

struct lf_ajtai {
  int device = 0;
  const uint64_t *A = nullptr;
  uint4 *Af = nullptr;  // A in i8-MFMA fragment order, mfma_ktiles(kappa) tiles of 32 rows
  uint64_t *kr = nullptr;  // FOFF x row sums of A per (row, output slot): lfk::ajtai_rowsums
  lfk::FragGeom geom{};  // contraction order of the fragments (ajtai_mfma.hip)
  bool owned = false;
  size_t kappa = 0, ncols = 0;
  int d = 0;
};

// the CCS matrices on the device (lf_ccs_create), plus the structure the
// linearization needs (lf_ccs_set_structure): l, the degree, c and S
struct lf_ccs {
  int device = 0;
  lfk::CcsDev dev{};
  std::vector<void *> bufs;
  bool structured = false;
  size_t l = 0;
  int degree = 0;
  std::vector<uint64_t> c;     // q NTT elements, canonical
  std::vector<int> S_off, S_idx;
  std::vector<uint8_t> live;   // [t][m]: row r of M_j holds an entry
  uint64_t *c_dev = nullptr;   // in bufs
  size_t c_dev_elems = 0;
  int *S_dev = nullptr;        // S_off [q + 1] then S_idx (the relation kernel's copy), in bufs
  size_t S_dev_elems = 0;
  ~lf_ccs() {  // every device buffer, also on a failed lf_ccs_create
    DevGuard g(device);
    for (void *p : bufs) (void)hipFree(p);
  }
};

// a communicator for the accumulator exchange (RCCL over xGMI)
struct lf_comm {
  ncclComm_t comm = nullptr;
  bool owned = false;
  int nranks = 1, rank = 0;
};

inline int fail(lf_ctx *c, int code, const std::string &msg) {
  if (c) c->last_error = msg;
  return code;
}

#define LF_HIP(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail((ctx), e_ == hipErrorOutOfMemory ? LF_ERR_OUT_OF_MEMORY : LF_ERR_DEVICE,        \
                  std::string(#call) + ": " + hipGetErrorString(e_));                            \
  } while (0)

#define LF_TRY(expr)          \
  do {                        \
    int r_ = (expr);          \
    if (r_ != LF_OK) return r_; \
  } while (0)

// 24 (Phi_72), and X^d + 1 for the degrees the kernels are built for (launch.hpp
// NegaDegrees: every power of two from 16 to 4096; lf_ring_supported)
inline bool ring_ok(int d) { return d == 24 || lfk::nega_degree_ok(d); }

inline int log2_exact(uint64_t v) {
  if (v < 2 || (v & (v - 1))) return -1;
  int l = 0;
  while ((1ull << l) != v) l++;
  return l;
}

inline int check_params(lf_ctx *c, const lf_params *pr, int &lb, int &lbs) {
  if (!pr) return fail(c, LF_ERR_INVALID_ARG, "null params");
  if (!ring_ok(pr->d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  lb = log2_exact(pr->B);
  lbs = log2_exact(pr->b_small);
  if (lb < 1 || lb > 62 || lbs < 1 || lbs > 62 || pr->L < 1 || pr->K < 1 || pr->L > 8 || pr->K > 64)
    return fail(c, LF_ERR_INVALID_ARG, "device path needs power-of-two B, b_small and L<=8, K<=64");
  return LF_OK;
}
inline int check_repr(lf_ctx *c, int repr) {
  if (repr != LF_REPR_CANONICAL && repr != LF_REPR_MONTGOMERY)
    return fail(c, LF_ERR_INVALID_ARG, "repr must be LF_REPR_CANONICAL or LF_REPR_MONTGOMERY");
  return LF_OK;
}

template <class T>
int grow(lf_ctx *c, T *&buf, size_t &have, size_t need) {
  if (need <= have) return LF_OK;
  if (buf) {
    LF_HIP(c, hipStreamSynchronize(c->cur));
    LF_HIP(c, hipFree(buf));
    buf = nullptr;
    have = 0;
  }
  LF_HIP(c, hipMalloc((void **)&buf, need * sizeof(T)));
  have = need;
  return LF_OK;
}
// a round message back through pinned memory (a pageable destination costs an extra
// staging copy per round)
inline int pinned(lf_ctx *c, size_t elems) {
  if (elems > c->hmsg_elems) {
    if (c->hmsg) LF_HIP(c, hipHostFree(c->hmsg));
    c->hmsg = nullptr;
    c->hmsg_elems = 0;
    LF_HIP(c, hipHostMalloc((void **)&c->hmsg, elems * 8, hipHostMallocDefault));
    c->hmsg_elems = elems;
  }
  return LF_OK;
}
inline int download_msg(lf_ctx *c, uint64_t *dst, const uint64_t *src, size_t elems) {
  LF_TRY(pinned(c, elems));
  LF_HIP(c, hipMemcpyAsync(c->hmsg, src, elems * 8, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  memcpy(dst, c->hmsg, elems * 8);
  return LF_OK;
}

// RAII device buffer for the synchronous host API
struct DevBuf {
  uint64_t *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};
inline int dev_alloc(lf_ctx *c, DevBuf &b, size_t elems) {
  LF_HIP(c, hipMalloc(&b.p, (elems ? elems : 1) * 8));
  return LF_OK;
}
inline int upload(lf_ctx *c, DevBuf &b, const uint64_t *h, size_t elems, int repr) {
  LF_TRY(dev_alloc(c, b, elems));
  if (elems) {
    LF_HIP(c, hipMemcpyAsync(b.p, h, elems * 8, hipMemcpyHostToDevice, c->cur));
    if (repr == LF_REPR_MONTGOMERY) LF_HIP(c, lfk::mont(b.p, elems, false, c->cur));
  }
  return LF_OK;
}
inline int download(lf_ctx *c, uint64_t *h, DevBuf &b, size_t elems, int repr) {
  if (!elems) return LF_OK;
  if (repr == LF_REPR_MONTGOMERY) LF_HIP(c, lfk::mont(b.p, elems, true, c->cur));
  LF_HIP(c, hipMemcpyAsync(h, b.p, elems * 8, hipMemcpyDeviceToHost, c->cur));
  return LF_OK;
}

// lf_api.hip
int get_tables(lf_ctx *c, int d, Tables *&out);  // negacyclic twiddle tables for degree d (built once per context)
size_t partial_elems(const lf_ajtai *aj, int nvec);
int ajtai_launch(lf_ctx *c, const lf_ajtai *aj, const uint64_t *const *vecs, int nvec, uint64_t *cm);
int allreduce_modp(lf_ctx *c, lf_comm *cm, uint64_t *x, size_t n);
// api_step.hip: can the step keep the decomposed witnesses as packed planes only? (lf_prover_create_lean)
int step_packed_form(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr);

// absorb R::from(value): the scalar in every NTT slot's base-ring word 0
inline void absorb_scalar(lf_transcript *t, uint64_t value, int d) {
  std::vector<uint64_t> e(d, 0);
  const int tb = lfk::slot_words(d);
  for (int i = 0; i < d; i += tb) e[i] = value;
  lf_transcript_absorb_ring(t, e.data(), 1, d, LF_REPR_CANONICAL);
}
// get_challenge (fiat_shamir.rs:69-86): three samples re-observed for Fq3 (tb = 3);
// one sample re-observed for Fq (this project's convention for X^d + 1)
inline void sample_challenge(lf_transcript *t, int tb, uint64_t *ch) {
  if (tb == 3) {
    lf_transcript_get_challenge(t, ch);
  } else {
    ch[0] = lf_transcript_sample(t);
    lf_transcript_observe(t, ch[0]);
  }
}
