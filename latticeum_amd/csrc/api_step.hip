// api_step.hip -- the device-resident commit+fold step behind include/lf.h:
// fold_commit / fold_finish, the step's path (api_internal.hpp StepState), the
// lf_dev_fold_step* entry points and the host-buffer lf_commit / lf_fold_hot.
#include <algorithm>

#include "api_internal.hpp"
#include "foldpow2.hpp"
#include "wsrc.hpp"

namespace {

// events around one step phase (lf_ctx_phase_stats); no-op unless timing is on
struct PhaseTimer {
  lf_ctx *c;
  int phase;
  hipEvent_t a = nullptr;
  PhaseTimer(lf_ctx *ctx, int ph) : c(ctx), phase(ph) {
    if (c->timing && hipEventCreate(&a) == hipSuccess) (void)hipEventRecord(a, c->cur);
  }
  ~PhaseTimer() {
    hipEvent_t b = nullptr;
    if (a && hipEventCreate(&b) == hipSuccess) {
      (void)hipEventRecord(b, c->cur);
      c->pending.push_back({a, b, -1 - phase});
    }
  }
};

// The commit+fold arithmetic of fold() on device buffers, in two halves so a
// column-sharded step can all-reduce the commitments between them:
//  fold_commit: decompose_witness of both sides (decomposition.rs:162-167) and
//    the 2(K-1) commitments of commit_witnesses (:178-201), plus -- when
//    `commit_f` is given (the device step) -- commit(z)'s A.f in the same pass
//    over A (29 vectors, one read of A). Result v goes to dst[v]: commit(z)'s
//    cm first, then y_s[k], s = 0, 1, k = 1 .. K-1. On the fused X^d + 1
//    decompositions (d = 16 .. 512, 1024, 4096) vector 0 is side 1's plane-0 operand row instead
//    (z_plane0 below) and its result y_1[0]: no pass converts f.
//  fold_finish: y_0 = cm - sum b^k y_k of both sides (cm1_out: side 1's y_0 is
//    given and cm = sum b^k y_k is made instead), cm_0 = sum rho_i y_i,
//    f_0 = sum rho_i f_i (folding.rs:258-268, folding/utils.rs:470-476) and
//    Witness::from_f(f_0) (arith.rs:299-313).
// d = 4096 with b_small = 2 has the register-transform decomposition (kernels_n4k.hip)
bool n4k_ok(const Tables *t, int d, int lbs, int K) { return d == 4096 && lbs == 1 && K <= 15 && t->fwd.tw4; }

// Which decomposition fold_commit runs and how fold_finish then makes f_0. The fused
// decompositions write their digit planes straight into the MFMA operand buffer; they
// need a scheme with fragments in the column order grouped by this L (d = 4096: in
// the quarter-major operand slots). FusedPow2 (d = 16 .. 512, decompose_pow2.hip) is
// the one a caller opts into: with f_k buffers and no planes those degrees stay Plain.
enum class Decomp { Plain, Fused1024, Fused24, Fused4k, FusedPow2 };
struct StepPlan {
  Decomp dec = Decomp::Plain;
  FoldPath path = FoldPath::Ntt;  // Masks24*: when the decomposition then reports its masks
};
StepPlan step_plan(const lf_ajtai *aj, const lf_params *pr, int lbs, const Tables *t, const lf_fold_step_bufs *b) {
  const int d = pr->d, L = pr->L, K = pr->K;
  const bool grouped = aj->Af && aj->geom.Lp == L;
  // without f_k buffers the planes exist only as operand rows (or stay packed)
  const bool no_fk = !b->fk[0] && !b->fk[1], no_fck = !b->fk_coeff[0] && !b->fk_coeff[1];
  StepPlan p;
  if (grouped && d == 1024 && lbs == 1 && K <= 15 && t->fwd.mid) {
    // the coefficient-form fold also needs t->inv.mid, which get_tables makes whenever it makes fwd.mid
    p.dec = Decomp::Fused1024;
    p.path = !no_fk ? FoldPath::Coeff1024 : no_fck ? FoldPath::Coeff1024Rows : FoldPath::Rows;
  } else if (grouped && d == 24 && L <= 5) {
    p.dec = Decomp::Fused24;
    p.path = lbs != 1 ? FoldPath::Ntt : no_fk ? FoldPath::Masks24Packed : FoldPath::Masks24;
  } else if (grouped && aj->geom.qperm && n4k_ok(t, d, lbs, K)) {
    p.dec = Decomp::Fused4k;
    p.path = no_fk ? FoldPath::Rows : FoldPath::Ntt;
  } else if (grouped && lfk::smp2_degree(d) && lbs == 1 && K <= 15 && ((b->planes[0] && b->planes[1]) || no_fk)) {
    // d = 16 .. 512 (decompose_pow2.hip): only for a caller who opted in, with planes
    // or without f_k buffers; with f_k and no planes the step stays Plain
    p.dec = Decomp::FusedPow2;
    // f_0 from the packed words: faster than from the operand rows at every degree measured
    p.path = no_fk ? FoldPath::CoeffPow2 : FoldPath::Ntt;
  }
  return p;
}

// commit(z) from the decomposition's own rows. The decomposition is exact (f_coeff =
// sum_k 2^(k lbs) D_k, or the step's error flag is raised) and the NTT is linear, so
// A f = sum_k 2^(k lbs) A NTT(D_(1,k)): cm = sum_k 2^(k lbs) y_1[k]. A step that
// commits z on the fused X^1024 + 1 / X^4096 + 1 / d = 16 .. 512 decompositions therefore has side
// 1's plane 0 written as operand row 0, contracts it as vector 0 into y_1[0], and
// fold_finish forms cm from the y_1[k] (y0_cm0's cm1_out). A function of (scheme,
// params, buffers) alone, never context state: fold_commit, fold_dst and fold_finish
// each evaluate it, so the split calls (partial / finish) and a failed step cannot
// disagree.
bool z_plane0(const lf_ajtai *aj, const lf_params *pr, int lbs, const Tables *t, const lf_fold_step_bufs *b) {
  const Decomp dec = step_plan(aj, pr, lbs, t, b).dec;
  return dec == Decomp::Fused1024 || dec == Decomp::Fused4k || dec == Decomp::FusedPow2;
}
int z_plane0(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, int lbs, const lf_fold_step_bufs *b, bool &z0) {
  Tables *t;
  LF_TRY(get_tables(c, pr->d, t));
  z0 = z_plane0(aj, pr, lbs, t, b);
  return LF_OK;
}

// both sides of a step for a fused decomposition: the step buffers and the operand
// rows, planes 1 .. K-1 of side s from row extra + s (K-1) on and (p0: a step
// without f_k) plane 0 in row extra + 2 (K-1) + s, or (z0: z_plane0) side 1's
// plane 0 in row 0; returns the mask of those rows
uint32_t step_sides(lfk::FusedSides &sd, const uint64_t *const *fc, const lf_fold_step_bufs *b, int extra, int K,
                    bool p0, bool z0 = false) {
  uint32_t rows = 0;
  sd.nside = 2;
  for (int s = 0; s < 2; s++) {
    sd.f_coeff[s] = fc[s];
    sd.f_coeff_k[s] = b->fk_coeff[s];
    sd.f_k[s] = b->fk[s];
    sd.w_ccs_k[s] = b->wk[s];
    sd.row0[s] = extra + s * (K - 1);
    sd.row_p0[s] = z0 && s == 1 ? 0 : p0 ? extra + 2 * (K - 1) + s : -1;
    for (int k = 1; k < K; k++) rows |= 1u << (sd.row0[s] + k - 1);
    if (sd.row_p0[s] >= 0) rows |= 1u << sd.row_p0[s];
  }
  return rows;
}

// d = 4096 with b_small = 2: the register-transform decomposition (kernels_n4k.hip),
// all sides in one launch. The packed digits -- one u64 per 4 coefficients, or
// (fused: frag given) one byte per 4 coefficients and plane -- go to sd.smg when
// the caller set it (the packed step's planes), else to the smg scratch
int decompose_n4k_sides(lf_ctx *c, const Tables *t, lfk::FusedSides &sd, size_t N, int lb, int L, int K,
                        uint4 *frag = nullptr, int nch = 0) {
  const bool own = !(frag && sd.smg[0]);
  // the smg scratch a d = 1024 step's coefficient fold would read may be overwritten here
  if (c->step.path == FoldPath::Coeff1024 || c->step.path == FoldPath::Coeff1024Rows ||
      c->step.path == FoldPath::CoeffPow2)
    c->step = {};
  if (own) LF_TRY(grow(c, c->smg, c->smg_elems, (size_t)sd.nside * N * (frag ? lfk::sm8_words(K) : 2 * lfk::SM4_WORDS)));
  LF_HIP(c, lfk::decompose_n4k(sd, N, lb, L, K, own ? reinterpret_cast<uint64_t *>(c->smg) : nullptr, t->fwd, c->d_err,
                               c->sink, c->ncu, c->cur, frag, nch));
  return LF_OK;
}

int fold_nvec(const lf_params *pr, bool commit_f) { return (commit_f ? 1 : 0) + 2 * (pr->K - 1); }

// a fused step's contraction left for lf_dev_fold_step_batch to launch with other steps'
struct Deferred {
  const uint4 *Ff = nullptr;
  uint64_t *partial = nullptr;
  lfk::OutPtrs dst{};
  lfk::DeadUnits dead{};
  const uint4 *zero80 = nullptr;
  int nvec = 0;
  bool set = false;
};
// the dead-unit flags: zeroed when (re)allocated, so a padding unit that no
// decomposition writes (unit 2c + 1 when nblk L is odd) reads as live, never as
// uninitialised memory
int grow_dead(lf_ctx *c, size_t need) {
  if (need <= c->dead_elems) return LF_OK;
  LF_TRY(grow(c, c->dead, c->dead_elems, need));
  LF_HIP(c, hipMemsetAsync(c->dead, 0, need, c->cur));
  return LF_OK;
}

int fold_commit(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, int lb, int lbs, size_t W,
                const lf_fold_step_bufs *b, const uint64_t *wi_f_coeff, const uint64_t *commit_f,
                const lfk::OutPtrs &dst, Deferred *defer = nullptr, const uint32_t *prepacked1 = nullptr) {
  // prepacked1: the buffer into which step_commit's from_w_ccs has just written
  // side 1's sign|magnitude words (fused d = 1024 path), or null. It is an
  // argument, not context state, so a failed step cannot leave it set for a
  // later call.
  const int d = pr->d, L = pr->L, K = pr->K;
  const size_t N = W * (size_t)L, kappa = aj->kappa;
  const int extra = commit_f ? 1 : 0, nvec = fold_nvec(pr, commit_f != nullptr);
  c->step = {};  // a step that fails leaves no path behind
  if (2 * K > LF_MAX_VECS || nvec > LF_MAX_VECS) return fail(c, LF_ERR_INVALID_ARG, "2K must be <= 32");
  if (aj->ncols != N) return fail(c, LF_ERR_WRONG_WITNESS_LENGTH, "witness length != Ajtai width");
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  const uint64_t *fc_side[2] = {b->acc_f_coeff, wi_f_coeff};
  const size_t kd = kappa * (size_t)d;
  // the fused decompositions write their digit planes straight into the MFMA operand
  // buffer: X^1024 + 1 (kernels_n32.hip), Phi_72 (decompose_phi72.hip), X^4096 + 1 (kernels_n4k.hip)
  // and d = 16 .. 512 (decompose_pow2.hip)
  StepPlan plan = step_plan(aj, pr, lbs, t, b);
  const bool fused = plan.dec == Decomp::Fused1024, fused24 = plan.dec == Decomp::Fused24,
             fused4k = plan.dec == Decomp::Fused4k, fusedp2 = plan.dec == Decomp::FusedPow2;
  // without f_k buffers the planes exist only as operand rows (step_sides), where
  // fold_finish reads f_0's inputs (k_fold_frag), or stay packed
  const bool no_fk = !b->fk[0] && !b->fk[1];
  // commit(z) rides as side 1's plane-0 row (row 0, extra = 1) instead of a row made from f
  const bool z0 = commit_f && z_plane0(aj, pr, lbs, t, b);
  if (b->planes[0] || b->planes[1]) {
    if (!(fused24 || fused || fused4k || fusedp2) || lbs != 1 || !b->planes[0] || !b->planes[1])
      return fail(c, LF_ERR_INVALID_ARG,
                  "packed planes: d = 24 or the fused d = 16 .. 512 / 1024 / 4096 paths, b_small = 2, both sides");
  }
  // X^1024 + 1 without f_k / f_coeff_k: the planes stay packed (the fused
  // decomposition's sign|magnitude words), f_0 comes from the coefficient-form
  // fold, whose fallback for a rho that is not short reads the operand rows
  const bool packed1024 = plan.path == FoldPath::Coeff1024Rows;
  // Phi_72 without f_k / f_coeff_k: the decomposed witnesses stay packed (digit masks)
  const bool packed24 = no_fk && fused24;
  StepState st{};
  st.N = N;
  if (packed24) {
    if (lbs != 1) return fail(c, LF_ERR_INVALID_ARG, "packed Phi_72 planes need b_small = 2");
    if (b->fk_coeff[0] || b->fk_coeff[1])
      return fail(c, LF_ERR_INVALID_ARG, "Phi_72: f_k and f_coeff_k are both given or both NULL");
  } else if (no_fk) {
    if (!fused && !fused4k && !fusedp2)
      return fail(c, LF_ERR_INVALID_ARG,
                  "f_k buffers may be omitted only on the fused X^d+1 paths (d = 16 .. 512, 1024, 4096)");
    if ((fused4k || fusedp2) && (b->fk_coeff[0] || b->fk_coeff[1]) && !(b->fk_coeff[0] && b->fk_coeff[1]))
      return fail(c, LF_ERR_INVALID_ARG, "f_coeff_k: both sides or neither");
    if (fused && !packed1024 && (!b->fk_coeff[0] || !b->fk_coeff[1]))
      return fail(c, LF_ERR_INVALID_ARG, "f_coeff_k: both sides or neither");
    if (extra + 2 * (K - 1) + 2 > LF_MAX_VECS) return fail(c, LF_ERR_INVALID_ARG, "too many operand rows");
    st.fold_rows.n = 2 * K;
    for (int s2 = 0; s2 < 2; s2++)
      for (int k = 0; k < K; k++) {
        const int row_p0 = z0 && s2 == 1 ? 0 : extra + 2 * (K - 1) + s2;  // as step_sides
        st.fold_rows.row[s2 * K + k] = k > 0 ? extra + s2 * (K - 1) + k - 1 : row_p0;
        st.fold_rows.rho[s2 * K + k] = s2 * K + k;
      }
  } else if (!b->fk[0] || !b->fk[1]) {
    return fail(c, LF_ERR_INVALID_ARG, "f_k: both sides or neither");
  }
  if (plan.dec == Decomp::Plain) {
    if (n4k_ok(t, d, lbs, K)) {
      lfk::FusedSides sd{};
      step_sides(sd, fc_side, b, 0, K, false);
      PhaseTimer pt(c, LF_PHASE_DECOMPOSE);  // both sides in one launch
      LF_TRY(decompose_n4k_sides(c, t, sd, N, lb, L, K));
    } else {
      for (int s = 0; s < 2; s++) {
        PhaseTimer pt(c, LF_PHASE_DECOMPOSE);
        LF_HIP(c, lfk::decompose_witness(fc_side[s], N, d, lb, L, lbs, K, b->fk_coeff[s], b->fk[s], b->wk[s], t->fwd,
                                         c->d_err, c->cur));
      }
    }
    // commit_witnesses: 2(K-1) commitments sharing one pass over A (decomposition.rs:185-188)
    std::vector<const uint64_t *> vecs;
    if (commit_f) vecs.push_back(commit_f);
    for (int s = 0; s < 2; s++)
      for (int k = 1; k < K; k++) vecs.push_back(b->fk[s] + (size_t)k * N * d);
    LF_TRY(grow(c, c->ybuf, c->ybuf_elems, (size_t)nvec * kd));
    LF_TRY(ajtai_launch(c, aj, vecs.data(), nvec, c->ybuf));
    for (int v = 0; v < nvec; v++)
      if (dst.p[v] != c->ybuf + v * kd)
        LF_HIP(c, hipMemcpyAsync(dst.p[v], c->ybuf + v * kd, kd * 8, hipMemcpyDeviceToDevice, c->cur));
    c->step = st;
    return LF_OK;
  }
  LF_TRY(grow(c, c->frag, c->frag_elems, lfk::frag_elems(aj->geom, d)));
  // dead units: the planes' operand rows are left unwritten where a unit's plane is zero
  LF_TRY(grow_dead(c, (size_t)aj->geom.nch * 64));
  lfk::FusedSides sd{};
  // without f_k, plane 0 of each side gets an operand row too (every X^d + 1 path);
  // z0: side 1's is row 0, with or without f_k, and row 0's dead units read as zero80
  const uint32_t rows = step_sides(sd, fc_side, b, extra, K, no_fk && !fused24, z0);
  sd.dead = c->dead;
  st.dead_units = {c->dead, rows};
  if (fused4k) {
    // the packed bytes go straight into the caller's planes when given
    for (int s = 0; s < 2 && b->planes[0]; s++) sd.smg[s] = reinterpret_cast<uint32_t *>(b->planes[s]);
    PhaseTimer pt(c, LF_PHASE_DECOMPOSE);  // both sides in one launch
    LF_TRY(decompose_n4k_sides(c, t, sd, N, lb, L, K, c->frag, aj->geom.nch));
  } else if (fusedp2) {
    // the packed words go into the caller's planes when given, else the context's scratch
    const size_t words = N * lfk::smp2_words(d);
    if (!b->planes[0]) LF_TRY(grow(c, c->smg, c->smg_elems, 2 * words));
    for (int s = 0; s < 2; s++)
      st.smg_side[s] = sd.smg[s] =
          b->planes[0] ? reinterpret_cast<uint32_t *>(b->planes[s]) : c->smg + (size_t)s * words;
    PhaseTimer pt(c, LF_PHASE_DECOMPOSE);  // both sides in one launch
    LF_HIP(c, lfk::decompose_pow2(sd, N, d, lb, L, K, t->fwd, c->frag, aj->geom.nch, c->d_err, c->cur));
  } else if (fused) {
    // the packed words go straight into the caller's planes when given; fold_finish's
    // coefficient-form fold reads the digits from them
    if (!b->planes[0]) LF_TRY(grow(c, c->smg, c->smg_elems, 2 * N * lfk::SM1024_WORDS));
    for (int s = 0; s < 2; s++)
      st.smg_side[s] = sd.smg[s] =
          b->planes[0] ? reinterpret_cast<uint32_t *>(b->planes[s]) : c->smg + (size_t)s * N * lfk::SM1024_WORDS;
    // side 1's words, when step_commit's from_w_ccs wrote them into this very buffer
    sd.prepacked = prepacked1 && prepacked1 == sd.smg[1] && wi_f_coeff == b->f_coeff ? 2 : 0;
    PhaseTimer pt(c, LF_PHASE_DECOMPOSE);  // both sides in one launch
    LF_HIP(c, lfk::decompose_fused(sd, N, lb, L, K, t->fwd, c->frag, aj->geom.nch, c->d_err,
                                   c->sink, c->ncu, c->cur));
  } else {
    // b_small = 2: the digit masks for fold_finish's coefficient-form fold,
    // into the caller's planes if given, else the context's scratch
    const bool want_masks = lbs == 1;
    if (want_masks && !b->planes[0]) LF_TRY(grow(c, c->fkeys, c->fkeys_elems, 2 * 2 * lfk::mask24_elems(K, N)));
    LF_TRY(grow(c, c->smg, c->smg_elems, 2 * N * lfk::SM24_WORDS));  // the coefficients as 16-bit sign|magnitude
    if (lbs != 1) sd.dead = nullptr;  // only the wave-local b_small = 2 kernel flags the zero planes' rows
    for (int s = 0; s < 2; s++) {
      sd.smg[s] = c->smg + (size_t)s * N * lfk::SM24_WORDS;
      if (want_masks)
        sd.masks[s] = b->planes[s] ? reinterpret_cast<uint2 *>(b->planes[s])
                                   : reinterpret_cast<uint2 *>(c->fkeys) + (size_t)s * lfk::mask24_elems(K, N);
      st.masks24[s] = sd.masks[s];
    }
    PhaseTimer pt(c, LF_PHASE_DECOMPOSE);  // both sides in one launch
    bool masks = false, dead = false;
    LF_HIP(c, lfk::decompose_phi72_sides(sd, N, lb, L, lbs, K, c->d_err, c->frag, aj->geom.nch, c->cur, &masks,
                                         &dead));
    if (packed24 && !masks) return fail(c, LF_ERR_INVALID_ARG, "packed Phi_72 planes need the wave-local decomposition");
    if (!masks) plan.path = FoldPath::Ntt;
    if (!dead) st.dead_units = lfk::DeadUnits{};  // only the wave-local kernel's flags are this step's
  }
  if (!fused24) st.fold_rows.dead = st.dead_units;
  st.path = plan.path;
  c->step = st;
  lfk::VecPtrs vp{};
  if (commit_f && !z0) {  // Phi_72: f as operand row 0
    PhaseTimer pt(c, LF_PHASE_TO_FRAG);
    vp.p[0] = commit_f;
    LF_HIP(c, lfk::to_frag(vp, 1, 0, aj->geom, d, true, c->frag, c->cur));
  }
  LF_TRY(grow(c, c->scratch, c->scratch_elems, partial_elems(aj, nvec)));
  if (defer) {  // the caller contracts this step together with others (one pass over A)
    defer->Ff = c->frag;
    defer->partial = c->scratch;
    defer->dst = dst;
    defer->dead = c->step.dead_units;
    defer->zero80 = c->zero80;
    defer->nvec = nvec;
    defer->set = true;
    return LF_OK;
  }
  hipEvent_t ea = nullptr, eb = nullptr;
  if (c->timing) {
    LF_HIP(c, hipEventCreate(&ea));
    LF_HIP(c, hipEventCreate(&eb));
  }
  LF_HIP(c, lfk::ajtai_mfma(aj->Af, aj->kr, kappa, aj->geom, d, vp, nvec, true, c->frag, c->scratch, nullptr, c->cur,
                            ea, eb, &dst, &c->step.dead_units, c->zero80));
  if (c->timing) c->pending.push_back({ea, eb, nvec});
  return LF_OK;
}

// destinations of fold_commit's results in the step buffers; z0 (z_plane0): vector 0
// of a step that commits z is y_1[0], not cm
lfk::OutPtrs fold_dst(const lf_params *pr, const lf_fold_step_bufs *b, size_t kd, uint64_t *commit_cm,
                      bool z0 = false) {
  lfk::OutPtrs dst{};
  const int extra = commit_cm ? 1 : 0;
  if (commit_cm) dst.p[0] = z0 ? b->y[1] : commit_cm;
  for (int s = 0; s < 2; s++)
    for (int k = 1; k < pr->K; k++) dst.p[extra + s * (pr->K - 1) + k - 1] = b->y[s] + (size_t)k * kd;
  return dst;
}

// the coefficient-form product at d = 16 .. 512: the rho tables and the not-short flag
// (both in faux; lf_ctx_fold_flag reads the flag), then f0_coeff unless the flag is up
int fold_pow2_coeff(lf_ctx *c, const lf_params *pr, const Tables *t, const uint32_t *sm0, const uint32_t *sm1,
                    size_t N, const uint64_t *rho, uint64_t *f0_coeff, int *&bad) {
  const int d = pr->d, K = pr->K, nw = 2 * K;
  const size_t tab_u64 = ((size_t)nw * lfk::fp2_tab_bytes(d) + 7) / 8;
  LF_TRY(grow(c, c->faux, c->faux_elems, tab_u64 + 1));
  uint8_t *tab = reinterpret_cast<uint8_t *>(c->faux);
  bad = reinterpret_cast<int *>(c->faux + tab_u64);
  c->fold_flag_at = (long)tab_u64;
  LF_HIP(c, lfk::fold_pow2_rho_tables(rho, nw, d, tab, bad, t->inv, c->d_sync, c->cur));
  const int ks_n = lfk::fold_pow2_splits(N, d, K, c->ncu);
  if (ks_n > 1) LF_TRY(grow(c, c->fpart, c->fpart_elems, (size_t)ks_n * N * d));
  LF_HIP(c, lfk::fold_coeff_pow2(sm0, sm1, tab, bad, N, d, K, f0_coeff, c->ncu, c->cur, ks_n > 1 ? c->fpart : nullptr));
  return LF_OK;
}

int fold_finish(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, int lb, int lbs, size_t W,
                const lf_fold_step_bufs *b, uint64_t *cm_i, bool cm1_out = false) {
  const int d = pr->d, L = pr->L, K = pr->K, nw = 2 * K;
  const size_t N = W * (size_t)L, kappa = aj->kappa;
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  // y_0 of both sides and cm_0 = sum rho_i y_i in one pass (the y_s[k >= 1] are in place);
  // cm1_out: y_1[0] is in place too and cm_i is made from side 1's planes
  LF_HIP(c, lfk::y0_cm0(b->acc_cm, cm_i, b->y[0], b->y[1], b->rho, kappa, d, lbs, K, b->cm0, c->cur, cm1_out));
  const StepState &st = c->step;
  c->fold_flag_at = -1;  // lf_ctx_fold_flag: set below where the path has a flag
  c->fold_has_level = false;
  // the f_k rows of both sides, for the NTT-form fold
  auto fk_rows = [&] {
    lfk::VecPtrs fx{};
    for (int s = 0; s < 2; s++)
      for (int k = 0; k < K; k++) fx.p[s * K + k] = b->fk[s] + (size_t)k * N * d;
    return fx;
  };
  // a state made for another N is not this step's: the NTT-form fold
  switch (st.N == N ? st.path : FoldPath::Ntt) {
    // X^1024 + 1 after the fused decomposition: f_0 in coefficient form on the
    // matrix cores from the digits (fold_coeff.hip), then f_0 and w_ccs by one
    // forward transform per element. If a rho is not short the device flag `bad`
    // turns those kernels off and the NTT-form fold and from_f on.
    case FoldPath::Coeff1024:
    case FoldPath::Coeff1024Rows: {
      // the last u64 of aux: the not-short flag and the Karatsuba level that ran (two ints)
      const size_t tab_u64 = (lfk::fold_tab_bytes(nw) + 7) / 8, aux = (size_t)nw * 1024 + tab_u64 + 1;
      const int kara = lfk::fold_kara_cap();
      // the digit keys [2 N][K][64] u32, then each column's plane mask [2 N] u32
      LF_TRY(grow(c, c->fkeys, c->fkeys_elems, 2 * N * (size_t)K * 64 + 2 * N));
      uint32_t *nz = c->fkeys + 2 * N * (size_t)K * 64;
      LF_TRY(grow(c, c->faux, c->faux_elems, aux));
      uint64_t *rc = c->faux;
      uint8_t *tab = reinterpret_cast<uint8_t *>(c->faux + (size_t)nw * 1024);
      int *bad = reinterpret_cast<int *>(c->faux + aux - 1);
      c->fold_flag_at = (long)(aux - 1);
      c->fold_has_level = true;
      {
        PhaseTimer pt(c, LF_PHASE_FOLD);
        for (int s = 0; s < 2; s++)
          LF_HIP(c, lfk::fold_keys(st.smg_side[s], N, K, c->fkeys + (size_t)s * N * K * 64, c->cur, nz + (size_t)s * N));
        LF_HIP(c, lfk::fold_rho_tables(b->rho, nw, rc, tab, bad, t->inv, c->d_sync, c->cur, kara));
        const int ks_n = lfk::fold_coeff_splits(N, K, c->ncu);
        if (ks_n > 1) LF_TRY(grow(c, c->fpart, c->fpart_elems, (size_t)ks_n * N * 1024));
        // packed planes: the fallback (f_0 in NTT form from the operand rows) runs
        // inside the same launch when the flag is set (no separate gated launch)
        const bool in_launch = st.path == FoldPath::Coeff1024Rows;
        const lfk::FoldFallback fb{c->frag, aj->geom.nch, aj->geom.Lp, aj->geom.Wp, st.fold_rows, b->rho, b->f0};
        LF_HIP(c, lfk::fold_coeff(c->fkeys, tab, bad, N, K, b->f0_coeff, c->ncu, c->cur,
                                  ks_n > 1 ? c->fpart : nullptr, in_launch ? &fb : nullptr, L, nz, kara));
        if (!in_launch) LF_HIP(c, lfk::fold(b->rho, fk_rows(), nw, N, d, b->f0, c->cur, bad));
      }
      // f_0 and w_ccs from f_0's coefficients, or (flag set) Witness::from_f of the
      // NTT-form f_0, in one launch
      PhaseTimer pt(c, LF_PHASE_FROM_F);
      LF_HIP(c, lfk::from_fcoeff_n32(b->f0_coeff, W, lb, L, b->f0, b->w_ccs0, t->fwd, bad, c->cur, &t->inv));
      return LF_OK;
    }
    // Phi_72 after the wave-local decomposition: f_0 in coefficient form from its
    // digit masks, then f_0 = CRT and w_ccs_0 (fold.hip k_fold_coeff_phi72); a
    // rho that is not short raises `bad`, which turns that kernel off and the
    // NTT-form fold and Witness::from_f on
    case FoldPath::Masks24:
    case FoldPath::Masks24Packed: {
      const uint2 *m0 = st.masks24[0], *m1 = st.masks24[1];
      LF_TRY(grow(c, c->faux, c->faux_elems, (size_t)nw * 13 + 1));
      uint32_t *rc = reinterpret_cast<uint32_t *>(c->faux);  // 25 packed words per witness
      int *bad = reinterpret_cast<int *>(c->faux + (size_t)nw * 13);
      c->fold_flag_at = (long)nw * 13;
      {
        PhaseTimer pt(c, LF_PHASE_FOLD);
        LF_HIP(c, lfk::fold_phi72_rho(b->rho, nw, rc, bad, c->cur));
        LF_HIP(c, lfk::fold_phi72_coeff(m0, m1, rc, bad, N, K, L, lb, b->f0_coeff, b->f0, b->w_ccs0, c->cur));
        // the fallback's f_0: from the masks in Z_p when the planes are packed, else from the f_k rows
        if (st.path == FoldPath::Masks24Packed)
          LF_HIP(c, lfk::fold_phi72_masks(m0, m1, b->rho, K, N, b->f0, bad, c->cur));
        else
          LF_HIP(c, lfk::fold(b->rho, fk_rows(), nw, N, d, b->f0, c->cur, bad));
      }
      PhaseTimer pt(c, LF_PHASE_FROM_F);
      LF_HIP(c, lfk::from_f(b->f0, N, d, lb, L, b->f0_coeff, b->w_ccs0, t->inv, c->cur, bad));
      return LF_OK;
    }
    // d = 16 .. 512 after the fused decomposition, no f_k: f_0 in coefficient form on the
    // matrix cores from the packed words (fold_coeff_pow2.hip), then f_0 and w_ccs by one
    // forward transform per element. If a rho is not short the device flag `bad` turns
    // those launches off and the fold from the operand rows and from_f on.
    case FoldPath::CoeffPow2: {
      int *bad;
      {
        PhaseTimer pt(c, LF_PHASE_FOLD);
        LF_TRY(fold_pow2_coeff(c, pr, t, st.smg_side[0], st.smg_side[1], N, b->rho, b->f0_coeff, bad));
        LF_HIP(c, lfk::fold_frag(c->frag, aj->geom, st.fold_rows, b->rho, d, N, b->f0, c->cur, bad));
      }
      PhaseTimer pt(c, LF_PHASE_FROM_F);
      LF_HIP(c, lfk::from_fcoeff(b->f0_coeff, lfk::WSRC_U64, N, d, lb, L, nullptr, b->f0, b->w_ccs0, t->fwd, nullptr,
                                 c->cur, bad));
      LF_HIP(c, lfk::from_f(b->f0, N, d, lb, L, b->f0_coeff, b->w_ccs0, t->inv, c->cur, bad));
      return LF_OK;
    }
    case FoldPath::Rows: {  // the planes are only in the operand rows (fold_commit)
      PhaseTimer pt(c, LF_PHASE_FOLD);
      LF_HIP(c, lfk::fold_frag(c->frag, aj->geom, st.fold_rows, b->rho, d, N, b->f0, c->cur));
      break;
    }
    case FoldPath::Ntt: {
      PhaseTimer pt(c, LF_PHASE_FOLD);
      LF_HIP(c, lfk::fold(b->rho, fk_rows(), nw, N, d, b->f0, c->cur));
      break;
    }
  }
  PhaseTimer pt(c, LF_PHASE_FROM_F);
  LF_HIP(c, lfk::from_f(b->f0, N, d, lb, L, b->f0_coeff, b->w_ccs0, t->inv, c->cur));
  return LF_OK;
}

int step_check(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W, const lf_fold_step_bufs *b, int &lb,
               int &lbs) {
  if (!c || !aj || !b) return LF_ERR_INVALID_ARG;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (pr->d != aj->d) return fail(c, LF_ERR_INVALID_ARG, "params ring != Ajtai ring");
  if (W * (size_t)pr->L != aj->ncols) return fail(c, LF_ERR_WRONG_WITNESS_LENGTH, "W*L != Ajtai width");
  return LF_OK;
}
// commit(z) (zkvm main.rs:348-367): Witness::from_w_ccs; its A f is batched
// with the decomposition commitments of fold() in a single pass over A
int step_commit(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W, const lf_fold_step_bufs *b, int lb,
                int lbs, const lfk::OutPtrs &dst, Deferred *defer = nullptr) {
  uint32_t *smg1 = nullptr;
  {
    PhaseTimer pt(c, LF_PHASE_FROM_W_CCS);
    // the fused X^1024 + 1 decomposition that fold_commit runs next packs both
    // sides' digits into sign|magnitude words; the new witness's (side 1) are
    // written here, by the kernel that makes its digits, instead of re-read
    Tables *t;
    LF_TRY(get_tables(c, pr->d, t));
    const int L = pr->L, K = pr->K, d = pr->d;
    const size_t N = W * (size_t)L;
    if (step_plan(aj, pr, lbs, t, b).dec == Decomp::Fused1024 && t->inv.mid && lb <= K && aj->ncols == N &&
        (!b->planes[0]) == (!b->planes[1])) {
      if (!b->planes[0]) LF_TRY(grow(c, c->smg, c->smg_elems, 2 * N * lfk::SM1024_WORDS));
      smg1 = b->planes[1] ? reinterpret_cast<uint32_t *>(b->planes[1]) : c->smg + N * lfk::SM1024_WORDS;
    }
    if (!b->w_ccs || !b->f_coeff || !b->f) return fail(c, LF_ERR_INVALID_ARG, "null step buffer");
    LF_HIP(c, lfk::from_w_ccs(b->w_ccs, W, d, lb, L, b->f_coeff, b->f, t->fwd, t->inv, c->d_err, c->cur, smg1));
  }
  return fold_commit(c, aj, pr, lb, lbs, W, b, b->f_coeff, b->f, dst, defer, smg1);
}

}  // namespace

// LF_OK when a step of (scheme, params) with planes and neither f_k nor f_coeff_k runs a
// fused decomposition (step_plan), so the planes can be the decomposed witnesses' only
// form; else LF_ERR_INVALID_ARG with the reason in the context's last error
int step_packed_form(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr) {
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (pr->d != aj->d) return fail(c, LF_ERR_INVALID_ARG, "params ring != Ajtai ring");
  if (lbs != 1) return fail(c, LF_ERR_INVALID_ARG, "no packed form: packed planes need b_small = 2");
  if (pr->K > 15) return fail(c, LF_ERR_INVALID_ARG, "no packed form: packed planes hold K <= 15 digits");
  if (!lf_fold_step_planes_len(pr, 1))
    return fail(c, LF_ERR_INVALID_ARG, "no packed form at this ring degree (d = 24, 16 .. 512, 1024 or 4096)");
  if (!aj->Af || aj->geom.Lp != pr->L)
    return fail(c, LF_ERR_INVALID_ARG, "no packed form: the scheme has no fragments grouped by this L");
  Tables *t;
  LF_TRY(get_tables(c, pr->d, t));
  uint64_t some;
  lf_fold_step_bufs b{};
  b.planes[0] = b.planes[1] = &some;  // never dereferenced: step_plan reads which buffers are given
  if (step_plan(aj, pr, lbs, t, &b).dec == Decomp::Plain)
    return fail(c, LF_ERR_INVALID_ARG, "no packed form: the step has no fused decomposition for this scheme and params");
  return LF_OK;
}

extern "C" {

int lf_dev_decompose_witness(lf_ctx *c, const lf_params *pr, const uint64_t *fc, size_t N, uint64_t *fck,
                             uint64_t *fk, uint64_t *wk) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  Tables *t;
  LF_TRY(get_tables(c, pr->d, t));
  if (n4k_ok(t, pr->d, lbs, pr->K)) {
    lfk::FusedSides sd{};
    sd.nside = 1;
    sd.f_coeff[0] = fc, sd.f_coeff_k[0] = fck, sd.f_k[0] = fk, sd.w_ccs_k[0] = wk;
    return decompose_n4k_sides(c, t, sd, N, lb, pr->L, pr->K);
  }
  LF_HIP(c, lfk::decompose_witness(fc, N, pr->d, lb, pr->L, lbs, pr->K, fck, fk, wk, t->fwd, c->d_err, c->cur));
  return LF_OK;
}

int lf_commit(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, const uint64_t *z, size_t z_len, size_t l,
              uint64_t *fc, uint64_t *f, uint64_t *cm, int repr) {
  DevGuard g(c);
  if (!c || !aj || !z || !fc || !f || !cm) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (pr->d != aj->d) return fail(c, LF_ERR_INVALID_ARG, "params ring != Ajtai ring");
  if (z_len < l + 1) return fail(c, LF_ERR_INCORRECT_LENGTH, "z shorter than l + 1");
  const int d = pr->d;
  const size_t W = z_len - l - 1, N = W * pr->L;  // main.rs:354-355: w_ccs = z[l+1..]
  if (N != aj->ncols) return fail(c, LF_ERR_WRONG_WITNESS_LENGTH, "Wrong length of the witness");
  DevBuf dw, dfc, df, dcm;
  LF_TRY(upload(c, dw, z + (l + 1) * d, W * d, repr));
  LF_TRY(dev_alloc(c, dfc, N * d));
  LF_TRY(dev_alloc(c, df, N * d));
  LF_TRY(dev_alloc(c, dcm, aj->kappa * d));
  LF_TRY(lf_dev_witness_from_w_ccs(c, pr, dw.p, W, dfc.p, df.p));
  const uint64_t *v = df.p;
  LF_TRY(ajtai_launch(c, aj, &v, 1, dcm.p));
  LF_TRY(download(c, fc, dfc, N * d, repr));
  LF_TRY(download(c, f, df, N * d, repr));
  LF_TRY(download(c, cm, dcm, aj->kappa * d, repr));
  return lf_ctx_sync(c);
}

int lf_fold_hot(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, const uint64_t *acc_cm,
                const uint64_t *acc_fc, const uint64_t *cm_i, const uint64_t *wi_fc, size_t N,
                const uint64_t *rho, uint64_t *y, uint64_t *f0, uint64_t *f0c, uint64_t *w0, uint64_t *cm0,
                int repr) {
  DevGuard g(c);
  if (!c || !aj || !acc_cm || !acc_fc || !cm_i || !wi_fc || !rho || !y || !f0 || !f0c || !w0 || !cm0)
    return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (pr->d != aj->d) return fail(c, LF_ERR_INVALID_ARG, "params ring != Ajtai ring");
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  const int d = pr->d, K = pr->K;
  const size_t W = N / pr->L, kd = aj->kappa * d;
  DevBuf dacm, dafc, dcmi, dwfc, drho, dfck[2], dfk[2], dwk[2], dy, df0, df0c, dw0, dcm0;
  LF_TRY(upload(c, dacm, acc_cm, kd, repr));
  LF_TRY(upload(c, dafc, acc_fc, N * d, repr));
  LF_TRY(upload(c, dcmi, cm_i, kd, repr));
  LF_TRY(upload(c, dwfc, wi_fc, N * d, repr));
  LF_TRY(upload(c, drho, rho, 2 * (size_t)K * d, repr));
  for (int s = 0; s < 2; s++) {
    LF_TRY(dev_alloc(c, dfck[s], K * N * d));
    LF_TRY(dev_alloc(c, dfk[s], K * N * d));
    LF_TRY(dev_alloc(c, dwk[s], K * W * d));
  }
  LF_TRY(dev_alloc(c, dy, 2 * K * kd));
  LF_TRY(dev_alloc(c, df0, N * d));
  LF_TRY(dev_alloc(c, df0c, N * d));
  LF_TRY(dev_alloc(c, dw0, W * d));
  LF_TRY(dev_alloc(c, dcm0, kd));
  lf_fold_step_bufs b{};
  b.acc_cm = dacm.p;
  b.acc_f_coeff = dafc.p;
  b.rho = drho.p;
  for (int s = 0; s < 2; s++) {
    b.fk_coeff[s] = dfck[s].p;
    b.fk[s] = dfk[s].p;
    b.wk[s] = dwk[s].p;
    b.y[s] = dy.p + (size_t)s * K * kd;
  }
  b.f0 = df0.p;
  b.f0_coeff = df0c.p;
  b.w_ccs0 = dw0.p;
  b.cm0 = dcm0.p;
  LF_TRY(fold_commit(c, aj, pr, lb, lbs, W, &b, dwfc.p, nullptr, fold_dst(pr, &b, kd, nullptr)));
  LF_TRY(fold_finish(c, aj, pr, lb, lbs, W, &b, dcmi.p));
  LF_TRY(download(c, y, dy, 2 * K * kd, repr));
  LF_TRY(download(c, f0, df0, N * d, repr));
  LF_TRY(download(c, f0c, df0c, N * d, repr));
  LF_TRY(download(c, w0, dw0, W * d, repr));
  LF_TRY(download(c, cm0, dcm0, kd, repr));
  return lf_ctx_sync(c);
}

int lf_dev_expand_planes(lf_ctx *c, const lf_params *pr, const uint64_t *planes, size_t N, uint64_t *fck,
                         uint64_t *fk) {
  if (!c) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  const int d = pr->d, K = pr->K;
  if (!planes && N) return fail(c, LF_ERR_INVALID_ARG, "planes is NULL");
  if (lbs != 1) return fail(c, LF_ERR_INVALID_ARG, "packed planes need b_small = 2");
  if (d == 24) {  // [K][N] digit masks
    LF_HIP(c, lfk::expand_phi72(reinterpret_cast<const uint2 *>(planes), lfk::mask24_elems(K, N), fck, fk, c->cur));
    return LF_OK;
  }
  if ((d != 1024 && d != 4096 && !lfk::smp2_degree(d)) || K > 15)
    return fail(c, LF_ERR_UNSUPPORTED_RING, "packed planes: d = 24, 16 .. 512, 1024 or 4096");
  if (!fck && !fk) return LF_OK;
  // sign|magnitude words (d = 4096: the digit bytes) -> f_coeff_k, then f_k = NTT(f_coeff_k)
  // (CRT::elementwise_crt)
  uint64_t *dst = fck ? fck : fk;
  if (lfk::smp2_degree(d))
    LF_HIP(c, lfk::expand_smp2(reinterpret_cast<const uint32_t *>(planes), N, d, K, dst, c->cur));
  else if (d == 1024)
    LF_HIP(c, lfk::expand_sm(reinterpret_cast<const uint32_t *>(planes), N, K, dst, c->cur));
  else
    LF_HIP(c, lfk::expand_sm8(reinterpret_cast<const uint32_t *>(planes), N, K, dst, c->cur));
  if (fk) {
    if (fck) LF_HIP(c, hipMemcpyAsync(fk, fck, (size_t)K * N * d * 8, hipMemcpyDeviceToDevice, c->cur));
    LF_TRY(lf_dev_crt(c, fk, (size_t)K * N, d));
  }
  return LF_OK;
}

int lf_dev_fold_planes(lf_ctx *c, const lf_params *pr, const uint64_t *planes0, const uint64_t *planes1, size_t N,
                       const uint64_t *rho, uint64_t *f0_coeff, uint64_t *f0, uint64_t *w_ccs0) {
  if (!c) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  const int d = pr->d, K = pr->K, L = pr->L, nw = 2 * K;
  if (!planes0 || !planes1 || !rho || !f0_coeff || !f0 || !w_ccs0) return fail(c, LF_ERR_INVALID_ARG, "fold_planes: NULL pointer");
  if ((d != 24 && d != 1024 && !lfk::smp2_degree(d)) || lbs != 1 || K > 15)
    return fail(c, LF_ERR_UNSUPPORTED_RING, "fold_planes: d = 24, 16 .. 512 or 1024, b_small = 2, K <= 15");
  if (N % L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  if (!N) return LF_OK;
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  const size_t W = N / L;
  c->fold_has_level = false;
  int *bad;
  if (d == 24) {
    const uint2 *m0 = reinterpret_cast<const uint2 *>(planes0), *m1 = reinterpret_cast<const uint2 *>(planes1);
    LF_TRY(grow(c, c->faux, c->faux_elems, (size_t)nw * 13 + 1));
    uint32_t *rc = reinterpret_cast<uint32_t *>(c->faux);  // 25 packed words per witness
    bad = reinterpret_cast<int *>(c->faux + (size_t)nw * 13);
    c->fold_flag_at = (long)nw * 13;
    LF_HIP(c, lfk::fold_phi72_rho(rho, nw, rc, bad, c->cur));
    LF_HIP(c, lfk::fold_phi72_coeff(m0, m1, rc, bad, N, K, L, lb, f0_coeff, f0, w_ccs0, c->cur));
  } else if (d == 1024) {
    if (!t->fwd.mid || !t->inv.mid) return fail(c, LF_ERR_UNSUPPORTED_RING, "fold_planes: no d = 1024 register transform");
    // a pending Phi_72 step's masks may live in fkeys: its fold_combine takes the f_k rows instead
    if (c->step.path == FoldPath::Masks24) c->step = {};
    const size_t tab_u64 = (lfk::fold_tab_bytes(nw) + 7) / 8, aux = (size_t)nw * 1024 + tab_u64 + 1;
    const int kara = lfk::fold_kara_cap();
    LF_TRY(grow(c, c->fkeys, c->fkeys_elems, 2 * N * (size_t)K * 64 + 2 * N));
    uint32_t *nz = c->fkeys + 2 * N * (size_t)K * 64;
    LF_TRY(grow(c, c->faux, c->faux_elems, aux));
    uint8_t *tab = reinterpret_cast<uint8_t *>(c->faux + (size_t)nw * 1024);
    bad = reinterpret_cast<int *>(c->faux + aux - 1);
    c->fold_flag_at = (long)(aux - 1);
    c->fold_has_level = true;
    const uint32_t *sm[2] = {reinterpret_cast<const uint32_t *>(planes0), reinterpret_cast<const uint32_t *>(planes1)};
    for (int s = 0; s < 2; s++)
      LF_HIP(c, lfk::fold_keys(sm[s], N, K, c->fkeys + (size_t)s * N * K * 64, c->cur, nz + (size_t)s * N));
    LF_HIP(c, lfk::fold_rho_tables(rho, nw, c->faux, tab, bad, t->inv, c->d_sync, c->cur, kara));
    const int ks_n = lfk::fold_coeff_splits(N, K, c->ncu);
    if (ks_n > 1) LF_TRY(grow(c, c->fpart, c->fpart_elems, (size_t)ks_n * N * 1024));
    LF_HIP(c, lfk::fold_coeff(c->fkeys, tab, bad, N, K, f0_coeff, c->ncu, c->cur, ks_n > 1 ? c->fpart : nullptr, nullptr,
                              L, nz, kara));
    LF_HIP(c, lfk::from_fcoeff_n32(f0_coeff, W, lb, L, f0, w_ccs0, t->fwd, bad, c->cur));
  } else {
    LF_TRY(fold_pow2_coeff(c, pr, t, reinterpret_cast<const uint32_t *>(planes0),
                           reinterpret_cast<const uint32_t *>(planes1), N, rho, f0_coeff, bad));
    LF_HIP(c, lfk::from_fcoeff(f0_coeff, lfk::WSRC_U64, N, d, lb, L, nullptr, f0, w_ccs0, t->fwd, nullptr, c->cur, bad));
  }
  // a rho that is not short is the caller's error here: lf_ctx_sync reports it
  LF_HIP(c, lfk::flag_to_err(bad, c->d_err, LF_DERR_RHO, c->cur));
  return LF_OK;
}

// commit_witnesses from the packed planes alone: each fused decomposition's from-planes
// front end (FusedSides::planes_in) writes all K planes of every side as operand rows
// s K + k -- plane 0 too, as row_p0 -- and one contraction over A gives every y[s][k].
// Nothing here depends on an earlier step; the operand buffer and the dead flags are
// overwritten, so whatever step the context remembered is forgotten first.
int lf_dev_commit_planes(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, const uint64_t *const *planes, int nside,
                         size_t N, uint64_t *const *y, uint64_t *const *cm, uint64_t *const *wk) {
  if (!c) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!aj || !planes || !y) return fail(c, LF_ERR_INVALID_ARG, "commit_planes: NULL pointer");
  if (nside < 1 || nside > 2) return fail(c, LF_ERR_INVALID_ARG, "commit_planes: nside is 1 or 2");
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (!lf_fold_step_planes_len(pr, 1))
    return fail(c, LF_ERR_UNSUPPORTED_RING, "commit_planes: d = 24, 16 .. 512, 1024 or 4096, b_small = 2, K <= 15");
  if (pr->d != aj->d) return fail(c, LF_ERR_INVALID_ARG, "params ring != Ajtai ring");
  for (int s = 0; s < nside; s++)
    if (!planes[s] || !y[s]) return fail(c, LF_ERR_INVALID_ARG, "commit_planes: NULL planes or y");
  const int d = pr->d, L = pr->L, K = pr->K;
  if (N % L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  if (N != aj->ncols) return fail(c, LF_ERR_INCORRECT_LENGTH, "N != Ajtai width");
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  // the decomposition a lean step of this scheme would run, and its refusal where it has none
  uint64_t some;
  lf_fold_step_bufs lean{};
  lean.planes[0] = lean.planes[1] = &some;  // never dereferenced: step_plan reads which buffers are given
  const Decomp dec = step_plan(aj, pr, lbs, t, &lean).dec;
  if (dec == Decomp::Plain)
    return fail(c, LF_ERR_INVALID_ARG,
                "packed planes: d = 24 or the fused d = 16 .. 512 / 1024 / 4096 paths, b_small = 2, both sides");
  if (dec == Decomp::Fused24 && (L - 1) * lb >= 62)
    return fail(c, LF_ERR_INVALID_ARG, "packed Phi_72 planes need the wave-local decomposition");
  c->step = {};  // its operand rows, flags and packed scratch are not a step's any more
  if (!N) return LF_OK;
  const size_t kappa = aj->kappa, kd = kappa * (size_t)d;
  const int nvec = nside * K;
  LF_TRY(grow(c, c->frag, c->frag_elems, lfk::frag_elems(aj->geom, d)));
  LF_TRY(grow_dead(c, (size_t)aj->geom.nch * 64));
  lfk::FusedSides sd{};
  lfk::OutPtrs dst{};
  uint32_t rows = 0;
  sd.nside = nside;
  sd.prepacked = (1 << nside) - 1;
  sd.dead = c->dead;
  for (int s = 0; s < nside; s++) {
    sd.f_coeff[s] = nullptr;
    sd.f_coeff_k[s] = sd.f_k[s] = nullptr;
    sd.w_ccs_k[s] = wk ? wk[s] : nullptr;
    sd.row_p0[s] = lfk::planes_row(s, K, 0);
    sd.row0[s] = lfk::planes_row(s, K, 1);
    // the packed format of this ring (digitpack.hpp): the masks at d = 24, else words or bytes
    sd.masks[s] = reinterpret_cast<uint2 *>(const_cast<uint64_t *>(planes[s]));
    sd.smg[s] = reinterpret_cast<uint32_t *>(const_cast<uint64_t *>(planes[s]));
    for (int k = 0; k < K; k++) {
      rows |= 1u << lfk::planes_row(s, K, k);
      dst.p[lfk::planes_row(s, K, k)] = y[s] + (size_t)k * kd;
    }
  }
  const lfk::DeadUnits dead{c->dead, rows};
  {
    PhaseTimer pt(c, LF_PHASE_DECOMPOSE);  // every side in one launch
    switch (dec) {
      case Decomp::Fused1024:
        LF_HIP(c, lfk::decompose_fused(sd, N, lb, L, K, t->fwd, c->frag, aj->geom.nch, c->d_err, c->sink, c->ncu,
                                       c->cur));
        break;
      case Decomp::Fused4k:
        LF_HIP(c, lfk::decompose_n4k(sd, N, lb, L, K, nullptr, t->fwd, c->d_err, c->sink, c->ncu, c->cur, c->frag,
                                     aj->geom.nch));
        break;
      case Decomp::FusedPow2:
        LF_HIP(c, lfk::decompose_pow2(sd, N, d, lb, L, K, t->fwd, c->frag, aj->geom.nch, c->d_err, c->cur));
        break;
      default:  // Fused24
        LF_HIP(c, lfk::decompose_phi72_sides(sd, N, lb, L, lbs, K, c->d_err, c->frag, aj->geom.nch, c->cur));
        break;
    }
  }
  LF_TRY(grow(c, c->scratch, c->scratch_elems, partial_elems(aj, nvec)));
  hipEvent_t ea = nullptr, eb = nullptr;
  if (c->timing) {
    LF_HIP(c, hipEventCreate(&ea));
    LF_HIP(c, hipEventCreate(&eb));
  }
  lfk::VecPtrs vp{};
  LF_HIP(c, lfk::ajtai_mfma(aj->Af, aj->kr, kappa, aj->geom, d, vp, nvec, true, c->frag, c->scratch, nullptr, c->cur, ea,
                            eb, &dst, &dead, c->zero80));
  if (c->timing) c->pending.push_back({ea, eb, nvec});
  for (int s = 0; s < nside && cm; s++)
    if (cm[s]) LF_HIP(c, lfk::cm_from_y(y[s], kappa, d, lbs, K, cm[s], c->cur));
  return LF_OK;
}

int lf_dev_fold_step(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W, const lf_fold_step_bufs *b) {
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(step_check(c, aj, pr, W, b, lb, lbs));
  bool z0;
  LF_TRY(z_plane0(c, aj, pr, lbs, b, z0));
  LF_TRY(step_commit(c, aj, pr, W, b, lb, lbs, fold_dst(pr, b, aj->kappa * (size_t)pr->d, b->cm, z0)));
  return fold_finish(c, aj, pr, lb, lbs, W, b, b->cm, z0);
}

// nsteps independent steps (one context, stream and buffer set each): every
// step's commit and decompositions on its own stream, one contraction of all of
// them on ctx[0]'s stream (ajtai_mfma_steps: A read from HBM once), then every
// step's fold_finish on its own stream again. Events order the streams; nothing
// waits on the host.
int lf_dev_fold_step_batch(lf_ctx *const *cs, int nsteps, const lf_ajtai *aj, const lf_params *pr, size_t W,
                           const lf_fold_step_bufs *const *bs) {
  if (!cs || !bs || !aj || nsteps < 1 || nsteps > LF_MAX_STEPS || !cs[0]) return LF_ERR_INVALID_ARG;
  lf_ctx *c0 = cs[0];
  for (int s = 0; s < nsteps; s++) {
    if (!cs[s] || !bs[s]) return fail(c0, LF_ERR_INVALID_ARG, "null context or step buffers");
    if (cs[s]->device != aj->device) return fail(c0, LF_ERR_INVALID_ARG, "every context must be on the scheme's device");
    for (int t = 0; t < s; t++)
      if (cs[t] == cs[s]) return fail(c0, LF_ERR_INVALID_ARG, "each step needs its own context");
  }
  if (nsteps == 1) return lf_dev_fold_step(c0, aj, pr, W, bs[0]);
  DevGuard g(c0);
  int lb = 0, lbs = 0;
  for (int s = 0; s < nsteps; s++) LF_TRY(step_check(cs[s], aj, pr, W, bs[s], lb, lbs));
  const size_t kd = aj->kappa * (size_t)pr->d;
  Deferred dfr[LF_MAX_STEPS];
  bool z0[LF_MAX_STEPS];
  for (int s = 0; s < nsteps; s++) {
    DevGuard gs(cs[s]);
    LF_TRY(z_plane0(cs[s], aj, pr, lbs, bs[s], z0[s]));
    LF_TRY(step_commit(cs[s], aj, pr, W, bs[s], lb, lbs, fold_dst(pr, bs[s], kd, bs[s]->cm, z0[s]), &dfr[s]));
  }
  // steps whose path has no fragments contracted on their own already
  const uint4 *ff[LF_MAX_STEPS];
  uint64_t *pp[LF_MAX_STEPS];
  lfk::OutPtrs dd[LF_MAX_STEPS];
  lfk::DeadUnits du[LF_MAX_STEPS];
  int n = 0, nvec = 0;
  for (int s = 0; s < nsteps; s++) {
    if (!dfr[s].set) continue;
    ff[n] = dfr[s].Ff;
    pp[n] = dfr[s].partial;
    dd[n] = dfr[s].dst;
    du[n] = dfr[s].dead;
    nvec = dfr[s].nvec;
    n++;
  }
  for (int s = 0; s < nsteps; s++)
    if (!cs[s]->join) LF_HIP(cs[s], hipEventCreateWithFlags(&cs[s]->join, hipEventDisableTiming));
  if (n) {
    // the contraction runs on c0's stream, or on c0's contraction stream when one
    // is set (lf_ctx_set_contract_stream: e.g. a CU-masked stream beside the step
    // streams' CUs), after every step stream's decomposition
    const hipStream_t cst = c0->contract ? c0->contract : c0->cur;
    for (int s = c0->contract ? 0 : 1; s < nsteps; s++) {
      LF_HIP(c0, hipEventRecord(cs[s]->join, cs[s]->cur));
      LF_HIP(c0, hipStreamWaitEvent(cst, cs[s]->join, 0));
    }
    hipEvent_t ea = nullptr, eb = nullptr;
    if (c0->timing) {
      LF_HIP(c0, hipEventCreate(&ea));
      LF_HIP(c0, hipEventCreate(&eb));
    }
    LF_HIP(c0, lfk::ajtai_mfma_steps(aj->Af, aj->kr, aj->kappa, aj->geom, pr->d, nvec, n, ff, pp, dd, cst, ea, eb, du,
                                     c0->zero80, c0->toptbl));
    if (c0->timing) c0->pending.push_back({ea, eb, nvec, n});
    if (c0->contract) {
      if (!c0->cjoin) LF_HIP(c0, hipEventCreateWithFlags(&c0->cjoin, hipEventDisableTiming));
      LF_HIP(c0, hipEventRecord(c0->cjoin, cst));
      for (int s = 0; s < nsteps; s++) LF_HIP(cs[s], hipStreamWaitEvent(cs[s]->cur, c0->cjoin, 0));
    } else {
      LF_HIP(c0, hipEventRecord(c0->join, c0->cur));
      for (int s = 1; s < nsteps; s++) LF_HIP(cs[s], hipStreamWaitEvent(cs[s]->cur, c0->join, 0));
    }
  }
  for (int s = 0; s < nsteps; s++) {
    DevGuard gs(cs[s]);
    LF_TRY(fold_finish(cs[s], aj, pr, lb, lbs, W, bs[s], bs[s]->cm, z0[s]));
  }
  return LF_OK;
}

size_t lf_fold_step_planes_len(const lf_params *pr, size_t N) {
  if (!pr || pr->b_small != 2 || pr->K < 1 || pr->K > 15) return 0;
  const size_t K = pr->K, d = pr->d;
  if (d == 24) return lfk::mask24_elems((int)K, N);
  if (d == 1024) return N * lfk::SM1024_WORDS / 2;
  if (d == 4096) return N * lfk::sm8_words((int)K) / 2;
  if (lfk::smp2_degree((int)d)) return N * lfk::smp2_words((int)d) / 2;
  return 0;  // d = 2048 and unsupported degrees: the step has no packed form
}

size_t lf_fold_step_partial_len(const lf_ajtai *aj, const lf_params *pr) {
  return aj && pr ? (size_t)fold_nvec(pr, true) * aj->kappa * pr->d : 0;
}

int lf_dev_fold_step_partial(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W,
                             const lf_fold_step_bufs *b, uint64_t *partial) {
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(step_check(c, aj, pr, W, b, lb, lbs));
  if (!partial) return fail(c, LF_ERR_INVALID_ARG, "null partial buffer");
  const size_t kd = aj->kappa * (size_t)pr->d;
  lfk::OutPtrs dst{};
  for (int v = 0; v < fold_nvec(pr, true); v++) dst.p[v] = partial + v * kd;
  return step_commit(c, aj, pr, W, b, lb, lbs, dst);
}

int lf_dev_fold_step_finish(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W,
                            const lf_fold_step_bufs *b, const uint64_t *partial_sum) {
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(step_check(c, aj, pr, W, b, lb, lbs));
  if (!partial_sum) return fail(c, LF_ERR_INVALID_ARG, "null partial sum");
  const size_t kd = aj->kappa * (size_t)pr->d;
  // the all-reduce is linear: vector 0's sum is cm, or (z_plane0) y_1[0]
  bool z0;
  LF_TRY(z_plane0(c, aj, pr, lbs, b, z0));
  const lfk::OutPtrs dst = fold_dst(pr, b, kd, b->cm, z0);
  for (int v = 0; v < fold_nvec(pr, true); v++)
    LF_HIP(c, hipMemcpyAsync(dst.p[v], partial_sum + v * kd, kd * 8, hipMemcpyDeviceToDevice, c->cur));
  return fold_finish(c, aj, pr, lb, lbs, W, b, b->cm, z0);
}

// the decomposition half of fold() without commit(z): both sides' decompose_witness
// and commit_witnesses (decomposition.rs:162-201), y_0 included; inputs
// acc_f_coeff / acc_cm (accumulator) and f_coeff / cm (the linearized instance)
int lf_dev_decompose_commit(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W,
                            const lf_fold_step_bufs *b) {
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(step_check(c, aj, pr, W, b, lb, lbs));
  if (!b->acc_f_coeff || !b->f_coeff || !b->acc_cm || !b->cm || !b->y[0] || !b->y[1] || !b->wk[0] || !b->wk[1])
    return fail(c, LF_ERR_INVALID_ARG, "decompose_commit: missing buffer");
  const size_t kd = aj->kappa * (size_t)pr->d;
  LF_TRY(fold_commit(c, aj, pr, lb, lbs, W, b, b->f_coeff, nullptr, fold_dst(pr, b, kd, nullptr)));
  for (int s = 0; s < 2; s++)
    LF_HIP(c, lfk::commit_y0(s ? b->cm : b->acc_cm, b->y[s], aj->kappa, pr->d, lbs, pr->K, c->cur));
  return LF_OK;
}

// the folding half, given rho: cm_0, f_0 and Witness::from_f(f_0) (folding.rs:112-122);
// right after lf_dev_decompose_commit on the same context and buffers
int lf_dev_fold_combine(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W, const lf_fold_step_bufs *b) {
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(step_check(c, aj, pr, W, b, lb, lbs));
  if (!b->rho || !b->f0 || !b->f0_coeff || !b->w_ccs0 || !b->cm0) return fail(c, LF_ERR_INVALID_ARG, "fold_combine: missing buffer");
  return fold_finish(c, aj, pr, lb, lbs, W, b, b->cm);
}

int lf_dev_fold_step_sharded(lf_ctx *c, const lf_ajtai *aj, const lf_params *pr, size_t W,
                             const lf_fold_step_bufs *b, lf_comm *cm) {
  DevGuard g(c);
  int lb, lbs;
  LF_TRY(step_check(c, aj, pr, W, b, lb, lbs));
  if (!cm || !cm->comm) return lf_dev_fold_step(c, aj, pr, W, b);
  const size_t len = lf_fold_step_partial_len(aj, pr);
  LF_TRY(grow(c, c->stage, c->stage_elems, len));
  LF_TRY(lf_dev_fold_step_partial(c, aj, pr, W, b, c->stage));
  LF_TRY(allreduce_modp(c, cm, c->stage, len));
  return lf_dev_fold_step_finish(c, aj, pr, W, b, c->stage);
}

}  // extern "C"
