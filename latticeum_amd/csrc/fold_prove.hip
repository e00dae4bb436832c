// fold_prove.hip -- the zkvm's fold() as one call: zk_latticefold_prove
// (zkvm/src/zk_latticefold.rs:37-102) with a fresh Poseidon2 transcript
// (zkvm/src/main.rs:394), in the reference's exact transcript order:
//   sanity_check; absorb_public_input (:152-184);
//   LFLinearizationProver::prove (latticefold/src/nifs/linearization.rs:153-197);
//   LFDecompositionProver::prove of (acc, w_acc), then of the linearized
//     (cm_i, w_i) (nifs/decomposition.rs:33-88);
//   LFFoldingProver::prove (nifs/folding.rs:42-130).
// This is host code above the C ABI, the way a Rust fold() would drive it: every
// heavy step is an lf_dev_* call on the context's stream (the decomposition and
// commitments, the Mz products, both sumchecks, the MLE evaluations, the fold),
// the transcript stays on the host, and only the protocol's messages -- a few
// hundred ring elements -- cross PCIe. The witnesses stay in HBM.
// Layout: lf_prover and its construction (the CCS-structure analysis, the carved
// allocations); Run (one call's stream, transcript and first error), GroupFeed (the
// second host thread that enqueues instance groups) and Fold (what crosses the
// phases of one call); lf_fold_prove as the table FOLD_PHASES of one function per
// LF_SPAN_* span; lf_linearize and the two relation checks on the same helpers.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "api_internal.hpp"

struct lf_prover {
  lf_ctx *ctx = nullptr;
  const lf_ajtai *aj = nullptr;
  const lf_ccs *ccs = nullptr;
  lf_params pr{};
  int device = 0;
  // shape
  int d = 0, tb = 1, tau = 1, s = 0, K = 0, t = 0, q = 0, degree = 0, nm_lin = 0, nm_fold = 0;
  size_t W = 0, N = 0, n = 0, nn = 0, l = 0, kappa = 0;
  std::vector<uint64_t> one;  // ONE (From<BaseRing> of 1): 1 in every NTT slot
  std::vector<uint64_t> c;    // q NTT elements
  std::vector<int> S_off, S_idx;
  std::vector<int> lin_list;  // the matrix of every linearization MLE (c_i != 0, j in S_i)
  // the Mz MLEs are materialised live matrices first (mz_order: the matrices read by the
  // linearization's combination, then the others); S_live: each multiset entry's
  // position among the nlive live ones
  std::vector<int> mz_order, S_live;
  int nlive = 0;
  // the linearization's round-0 points per multiset: b is active for S_i when every
  // factor's matrix has an entry in row 2b or 2b + 1 (lf_sumcheck_prove_lin_sparse);
  // act_off [q + 1] into the device list act
  std::vector<uint32_t> act_off, act_host;
  uint32_t *act = nullptr;
  // device memory: one allocation, carved
  uint64_t *mem = nullptr;
  uint64_t *z = nullptr, *mz = nullptr, *lin = nullptr, *pt = nullptr, *beta = nullptr, *val = nullptr;
  uint64_t *fkc[2] = {}, *fk[2] = {}, *wk[2] = {}, *y[2] = {}, *cmd[2] = {}, *xw[2] = {}, *xs = nullptr;
  uint64_t *zdec[2] = {}, *vs = nullptr, *us = nullptr, *fold = nullptr, *coef[2] = {}, *zeta = nullptr, *mu = nullptr;
  uint64_t *theta = nullptr, *eta = nullptr, *rho = nullptr, *rhoc = nullptr, *cm0 = nullptr, *u0 = nullptr, *x0 = nullptr,
           *v0 = nullptr, *r0 = nullptr;
  // eq(r_0) and one point's Mz weights M_j^T eq (shared by the sides evaluated there)
  uint64_t *eq0 = nullptr, *mzw = nullptr;
  uint64_t *lev = nullptr;  // the live Mz MLEs at r_lin (the linearization sumcheck's final values)
  uint64_t *chk = nullptr;  // lf_lcccs_check / lf_cccs_check: the compare kernel's result words
  // lean (lf_prover_create_lean): no fkc / fk; the decomposed witnesses are the packed
  // digit planes of each side, and witness_checks takes its N elements from scr
  bool lean = false;
  uint64_t *planes[2] = {}, *scr = nullptr;
  size_t mem_elems = 0;  // the carved allocation (lf_prover_device_bytes)
  std::string err;
  // every value the last lf_fold_prove sampled from its transcript, in order
  // (lf_fold_prove_vars replays the proof on them instead of a second sponge)
  std::vector<uint64_t> samples;
  // tracing spans (the reference's #[instrument] spans, zkvm/src/main.rs:56-63):
  // wall ms of each fold() phase, measured with a stream sync at its end
  bool timing = false;
  double span_ms[LF_SPAN_COUNT] = {};
  // pinned host staging: the messages the host absorbs come back through it with
  // asynchronous copies (so the device keeps working while the host hashes), and
  // the points the device needs go out through it
  uint64_t *pin = nullptr;
  uint64_t *hx[2] = {}, *hy[2] = {}, *hu[2] = {}, *hv[2] = {}, *hr[2] = {}, *htheta = nullptr, *heta = nullptr;
  // ev[0], ev[1]: per-side / theta readiness; ev[2 + g]: instance group g's messages
  hipEvent_t ev[2 + 2 * 16] = {};
  ~lf_prover() {
    DevGuard g(device);
    if (mem) (void)hipFree(mem);
    if (pin) (void)hipHostFree(pin);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// instances per u_s / eta_s launch (and per host wait): two fill the chip with
// t blocks each, and the host starts absorbing after the first group
constexpr int MZ_GROUP = 2;

// From<BaseRing> = from_scalar: the base-ring element in every NTT slot
void broadcast(const uint64_t *base, int tb, int d, uint64_t *out) {
  for (int i = 0; i < d; i++) out[i] = base[i % tb];
}

int bad(lf_prover *P, int code, const char *msg) {
  P->err = msg;
  return code;
}

int hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? LF_ERR_OUT_OF_MEMORY : LF_ERR_DEVICE; }

bool repr_ok(int repr) { return repr == LF_REPR_CANONICAL || repr == LF_REPR_MONTGOMERY; }

// a host copy of a public input in canonical form
std::vector<uint64_t> canon(const uint64_t *src, size_t elems, int repr) {
  std::vector<uint64_t> v(src, src + elems);
  if (repr == LF_REPR_MONTGOMERY)
    for (auto &x : v) x = gl::from_mont(x);
  return v;
}

void to_mont(uint64_t *p, size_t elems) {
  for (size_t i = 0; i < elems; i++) p[i] = gl::to_mont(p[i]);
}

void lcccs_to_mont(const lf_prover *P, lf_lcccs_mut *o) {
  const size_t d = P->d;
  to_mont(o->r, P->s * d);
  to_mont(o->v, P->tau * d);
  to_mont(o->cm, P->kappa * d);
  to_mont(o->u, P->t * d);
  to_mont(o->x_w, P->l * d);
  to_mont(o->h, d);
}

bool lcccs_sizes_ok(const lf_prover *P, const lf_lcccs *a) {
  return a->d == P->d && a->r.n == (size_t)P->s && a->v.n == (size_t)P->tau && a->cm.n == P->kappa &&
         a->u.n == (size_t)P->t && a->x_w.n == P->l && a->h;
}

bool lcccs_out_ok(const lf_prover *P, const lf_lcccs_mut *o) {
  return o->r && o->v && o->cm && o->u && (!P->l || o->x_w) && o->h;
}

// the witness buffers a call reads or writes: f_coeff always, f and w_ccs where asked for
bool witness_ok(const lf_witness *w, bool f, bool w_ccs) { return w->f_coeff && (!f || w->f) && (!w_ccs || w->w_ccs); }

struct TGuard {
  lf_transcript *t;
  ~TGuard() { lf_transcript_free(t); }
};

// ---------------------------------------------------------------- lf_prover_create's parts

// the shape from the CCS, the Ajtai matrix and the parameters; LF_ERR_INVALID_ARG where
// they do not fit one another
int prover_shape(lf_prover *P) {
  const lf_params *pr = &P->pr;
  const int d = pr->d;
  size_t m = 0, n = 0, l = 0;
  int t = 0, q = 0, degree = 0;
  if (lf_ccs_shape(P->ccs, &t, &m, &n, &l, &q, &degree) != LF_OK || q < 1)
    return LF_ERR_INVALID_ARG;  // lf_ccs_set_structure first
  if (lf_ajtai_d(P->aj) != d || (m & (m - 1)) || m < 2 || pr->b_small < 2 || pr->K < 1 || pr->K > 16 || pr->L < 1 ||
      n < l + 2)
    return LF_ERR_INVALID_ARG;
  P->d = d;
  P->tb = d == 24 ? 3 : 1;
  P->tau = d == 24 ? 3 : 1;
  P->K = pr->K;
  P->t = t;
  P->q = q;
  P->degree = degree;
  P->n = n;
  P->l = l;
  P->W = n - l - 1;
  P->N = P->W * (size_t)pr->L;
  P->nn = m;
  while (((size_t)1 << P->s) < m) P->s++;
  P->kappa = lf_ajtai_kappa(P->aj);
  P->nm_fold = 5 + 2 * P->K * P->tau;
  P->one.assign(d, 0);
  for (int i = 0; i < d; i += P->tb) P->one[i] = 1;
  // sanity_check (zk_latticefold.rs:152-158): m = max((n - l - 1) L, m).next_power_of_two();
  // Witness::get_fhat gives MLEs of log2(N.next_power_of_two()) variables, which the
  // sumchecks over s = log2 m variables need to be s as well
  size_t want = std::max(P->N, m), pw = 1;
  while (pw < want) pw <<= 1;
  size_t npw = 1;
  while (npw < P->N) npw <<= 1;
  if (pw != m || npw != m || lf_ajtai_width(P->aj) != P->N)
    return LF_ERR_INVALID_ARG;  // CSError::InvalidSizeBounds / a witness of another width
  return LF_OK;
}

bool c_is_zero(const lf_prover *P, int i) {
  bool zero = true;
  for (int k = 0; k < P->d; k++) zero &= P->c[(size_t)i * P->d + k] == 0;
  return zero;
}

// c, S and lin_list: the matrix behind every position of the linearization's MLE list
void linearization_mle_list(lf_prover *P) {
  const int q = P->q;
  P->c.resize((size_t)q * P->d);
  P->S_off.resize(q + 1);
  lf_ccs_get_structure(P->ccs, P->c.data(), P->S_off.data(), nullptr);
  P->S_idx.resize(P->S_off[q]);
  lf_ccs_get_structure(P->ccs, nullptr, nullptr, P->S_idx.data());
  for (int i = 0; i < q; i++) {
    if (c_is_zero(P, i)) continue;  // prepare_lin_sumcheck_polynomial skips c_i = 0 (linearization/utils.rs:71-84)
    for (int k = P->S_off[i]; k < P->S_off[i + 1]; k++) P->lin_list.push_back(P->S_idx[k]);
  }
  P->nm_lin = (int)P->lin_list.size() + 1;
}

// mz_order, S_live and nlive; rejects (message in the context's last error) a multiset
// index that is no Mz MLE's list position
int live_matrix_order(lf_prover *P) {
  std::vector<int> pos_of(P->t, -1);
  bool eq_slot = false;
  P->S_live.resize(P->S_idx.size());
  for (size_t k = 0; k < P->S_idx.size(); k++) {
    const int p = P->S_idx[k];
    if (p < 0 || (size_t)p > P->lin_list.size()) {
      // past the eq(beta) slot or negative: malformed, the reference would panic on the index
      lf_ctx_set_error(P->ctx, "lf_prover_create: a multiset index is negative or past the Mz MLE list and its "
                               "eq(beta) slot");
      return LF_ERR_INVALID_ARG;
    }
    if ((size_t)p == P->lin_list.size()) {
      eq_slot = true;
      continue;
    }
    const int j = P->lin_list[p];
    if (pos_of[j] < 0) {
      pos_of[j] = (int)P->mz_order.size();
      P->mz_order.push_back(j);
    }
    P->S_live[k] = pos_of[j];
  }
  if (eq_slot) {
    // The reference's list position lin_list.size() is the eq(beta) MLE itself
    // (linearization/utils.rs:71-84): a multiset naming it would put a second eq
    // factor into its term, which the split-eq sumcheck (eq(beta) taken out of every
    // term) does not express. Rejected here, by name, rather than mid-fold.
    lf_ctx_set_error(P->ctx, "lf_prover_create: a multiset index is the position of eq(beta) in the MLE list; "
                             "multisets over eq(beta) are not supported");
    return LF_ERR_UNSUPPORTED_CCS;
  }
  P->nlive = (int)P->mz_order.size();
  for (int j = 0; j < P->t; j++)
    if (pos_of[j] < 0) P->mz_order.push_back(j);
  return LF_OK;
}

// act_off and act_host: the linearization's active round-0 points of every multiset
void active_points(lf_prover *P) {
  const size_t m = P->nn, half = m / 2;
  std::vector<uint8_t> row(m);
  std::vector<std::vector<uint8_t>> pair(P->nlive, std::vector<uint8_t>(half));
  for (int i = 0; i < P->nlive; i++) {
    lf_ccs_row_live(P->ccs, P->mz_order[i], row.data());
    for (size_t b = 0; b < half; b++) pair[i][b] = row[2 * b] | row[2 * b + 1];
  }
  P->act_off.assign(P->q + 1, 0);
  for (int i = 0; i < P->q; i++) {
    if (!c_is_zero(P, i))  // c_i = 0: no active point
      for (size_t b = 0; b < half; b++) {
        bool on = true;
        for (int k = P->S_off[i]; k < P->S_off[i + 1] && on; k++) on = pair[P->S_live[k]][b];
        if (on) P->act_host.push_back((uint32_t)b);
      }
    P->act_off[i + 1] = (uint32_t)P->act_host.size();
  }
}

// One allocation carved into parts, each rounded up to `align` elements: the total,
// and with a base where every part starts
struct Part {
  uint64_t **p;
  size_t elems;
};
size_t carve(const std::vector<Part> &parts, size_t align, uint64_t *base) {
  size_t off = 0;
  for (auto &x : parts) {
    if (base) *x.p = base + off;
    off += (x.elems + align - 1) / align * align;
  }
  return off;
}

// the device memory, the round-0 point list in it, the pinned staging and the events
int prover_alloc(lf_prover *P) {
  const size_t d = P->d, K = P->K, N = P->N, W = P->W, n = P->n, nn = P->nn, l = P->l, kd = P->kappa * d, tau = P->tau,
               t = P->t, s = P->s;
  // the decomposed witnesses: their f_coeff_k / f_k rows, or (lean) packed planes and one N-element scratch
  const size_t rows = P->lean ? 0 : K * N * d, pl = P->lean ? lf_fold_step_planes_len(&P->pr, N) : 0;
  const std::vector<Part> parts = {
      {&P->z, n * d}, {&P->mz, t * nn * d}, {&P->lin, (size_t)std::max(P->nlive, 1) * std::max<size_t>(nn / 4, 1) * d},
      {&P->pt, s * d}, {&P->beta, s * d}, {&P->val, (t + 3) * d},
      {&P->fkc[0], rows}, {&P->fkc[1], rows}, {&P->fk[0], rows}, {&P->fk[1], rows},
      {&P->planes[0], pl}, {&P->planes[1], pl}, {&P->scr, P->lean ? N * d : 0},
      {&P->wk[0], K * W * d}, {&P->wk[1], K * W * d}, {&P->y[0], K * kd}, {&P->y[1], K * kd},
      {&P->cmd[0], kd}, {&P->cmd[1], kd}, {&P->xw[0], (l + 1) * d}, {&P->xw[1], (l + 1) * d},
      {&P->xs, 2 * K * (l + 1) * d}, {&P->zdec[0], K * n * d}, {&P->zdec[1], K * n * d},
      {&P->vs, 2 * K * tau * d}, {&P->us, 2 * K * t * d}, {&P->fold, (size_t)P->nm_fold * nn * d},
      {&P->coef[0], K * tau * d}, {&P->coef[1], K * tau * d}, {&P->zeta, 2 * K * d}, {&P->mu, 2 * K * d},
      {&P->theta, 2 * K * tau * d}, {&P->eta, 2 * K * t * d}, {&P->rho, 2 * K * d}, {&P->rhoc, 2 * K * d},
      {&P->cm0, kd}, {&P->u0, t * d}, {&P->x0, (l + 1) * d}, {&P->v0, tau * d}, {&P->r0, s * d},
      {&P->eq0, nn * d}, {&P->mzw, lf_ccs_weights_len(P->ccs)}, {&P->lev, t * d},
      {&P->chk, 2}, {reinterpret_cast<uint64_t **>(&P->act), (P->act_host.size() + 1) / 2}};
  const std::vector<Part> pins = {
      {&P->hx[0], K * (l + 1) * d}, {&P->hx[1], K * (l + 1) * d}, {&P->hy[0], K * kd}, {&P->hy[1], K * kd},
      {&P->hu[0], K * t * d}, {&P->hu[1], K * t * d}, {&P->hv[0], K * tau * d}, {&P->hv[1], K * tau * d},
      {&P->hr[0], s * d}, {&P->hr[1], s * d}, {&P->htheta, 2 * K * tau * d}, {&P->heta, 2 * K * t * d}};
  DevGuard g(P->device);
  P->mem_elems = carve(parts, 32, nullptr);
  hipError_t e = hipMalloc(&P->mem, P->mem_elems * 8);  // 256-B aligned parts
  if (e != hipSuccess) {
    P->mem = nullptr;
    return hip_status(e);
  }
  carve(parts, 32, P->mem);
  // a zero-length part's address is the next part's: the decomposition must see NULL there
  for (int side = 0; side < 2; side++) {
    if (P->lean) P->fkc[side] = P->fk[side] = nullptr;
    if (!P->lean) P->planes[side] = nullptr;
  }
  if (!P->lean) P->scr = nullptr;
  if (!P->act_host.empty()) {
    if (hipMemcpy(P->act, P->act_host.data(), P->act_host.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return LF_ERR_DEVICE;
    P->act_host = std::vector<uint32_t>();
  }
  e = hipHostMalloc(reinterpret_cast<void **>(&P->pin), carve(pins, 8, nullptr) * 8, hipHostMallocDefault);
  for (auto &ev : P->ev)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) return hip_status(e);
  carve(pins, 8, P->pin);
  return LF_OK;
}

// ---------------------------------------------------------------- one call's state

struct Run {
  lf_prover *P;
  lf_transcript *T;
  hipStream_t st;
  int rc = LF_OK;
  std::string *err = nullptr;  // where this Run records its first error (default P->err)
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  std::string &errs() { return err ? *err : P->err; }

  // close the span that ran since the last mark (only with timing on); sync = false
  // where the device work of the span overlaps the next span's host work (the
  // span then ends when its work is enqueued, and the wait lands in the next one)
  void mark(int span, bool sync = true) {
    if (!P->timing) return;
    if (sync) (void)hipStreamSynchronize(st);
    const auto now = std::chrono::steady_clock::now();
    P->span_ms[span] += std::chrono::duration<double, std::milli>(now - t0).count();
    t0 = now;
  }

  int check(int r, const char *what) {
    if (r != LF_OK && rc == LF_OK) {
      rc = r;
      errs() = std::string(what) + ": " + lf_ctx_last_error(P->ctx);
    }
    return r;
  }
  int hip(hipError_t e, const char *what) {
    if (e != hipSuccess && rc == LF_OK) {
      rc = hip_status(e);
      errs() = std::string(what) + ": " + hipGetErrorString(e);
    }
    return rc;
  }
  int h2d(uint64_t *dst, const uint64_t *src, size_t elems) {
    return elems ? hip(hipMemcpyAsync(dst, src, elems * 8, hipMemcpyHostToDevice, st), "upload") : rc;
  }
  int d2h(uint64_t *dst, const uint64_t *src, size_t elems) {
    if (!elems) return rc;
    hip(hipMemcpyAsync(dst, src, elems * 8, hipMemcpyDeviceToHost, st), "download");
    return hip(hipStreamSynchronize(st), "sync");
  }
  int d2d(uint64_t *dst, const uint64_t *src, size_t elems) {
    return elems ? hip(hipMemcpyAsync(dst, src, elems * 8, hipMemcpyDeviceToDevice, st), "copy") : rc;
  }
  // device -> pinned host, asynchronous (completion: an event recorded after it)
  int d2p(uint64_t *dst, const uint64_t *src, size_t elems) {
    return elems ? hip(hipMemcpyAsync(dst, src, elems * 8, hipMemcpyDeviceToHost, st), "download") : rc;
  }
  // host -> device through a pinned copy of the source (no stream synchronisation)
  int h2p2d(uint64_t *dst, uint64_t *pinned, const uint64_t *src, size_t elems) {
    if (!elems) return rc;
    memcpy(pinned, src, elems * 8);
    return hip(hipMemcpyAsync(dst, pinned, elems * 8, hipMemcpyHostToDevice, st), "upload");
  }
  int wait(hipEvent_t e) { return hip(hipEventSynchronize(e), "event wait"); }
  void absorb(const uint64_t *e, size_t n) { lf_transcript_absorb_ring(T, e, n, P->d, LF_REPR_CANONICAL); }
  // absorb_field_element(BaseRing::from_base_prime_field(from_be_bytes_mod_order(label)))
  void absorb_label(const char *label) {
    uint64_t v = 0;
    for (const char *p = label; *p; p++) v = gl::add(gl::mul(v, 256), (uint8_t)*p);
    absorb_scalar(T, v, P->d);
  }
  void challenge(uint64_t *out) { sample_challenge(T, P->tb, out); }
  // get_challenges(n) mapped into NTT elements: [n][d]
  std::vector<uint64_t> challenges(size_t n) {
    std::vector<uint64_t> out(n * P->d);
    uint64_t b[3];
    for (size_t i = 0; i < n; i++) {
      challenge(b);
      broadcast(b, P->tb, P->d, out.data() + i * P->d);
    }
    return out;
  }
  // the sumcheck's point (one base-ring challenge per round) as NTT elements
  std::vector<uint64_t> point(const std::vector<uint64_t> &rnd) {
    std::vector<uint64_t> r((size_t)P->s * P->d);
    for (int i = 0; i < P->s; i++) broadcast(rnd.data() + (size_t)i * P->tb, P->tb, P->d, r.data() + (size_t)i * P->d);
    return r;
  }
};

// Instance groups go to the device from a second host thread: with the stream's queue
// deep, every enqueue blocks the calling thread for tens of microseconds, which the
// transcript thread would otherwise spend before and between its absorbs. The body
// enqueues on Q -- a Run of the feed's own, so the error state is not shared and P->err
// is never written from two threads -- and calls post(g) once group g's event
// P->ev[2 + g] is recorded; the transcript thread calls wait(R, g) before it reads
// group g's messages, and join(R) when it has read them all. Where no thread is to be
// had the body runs in the constructor (everything enqueued first); the destructor
// joins, so no return path leaves a thread behind.
class GroupFeed {
  static constexpr int DONE = 1 << 30;
  std::atomic<int> posted{0};  // groups whose event is recorded; DONE: the body has returned (also on an error)
  std::string err;             // the body's own error text, merged into R's by join
  std::thread th;

 public:
  Run Q;
  template <class Body>
  GroupFeed(const Run &R, Body body) : Q(R) {
    Q.err = &err;
    auto work = [this, body] {
      DevGuard g(Q.P->device);  // a new thread starts on device 0
      if (Q.rc == LF_OK) body(*this);
      posted.store(DONE, std::memory_order_release);
    };
    try {
      th = std::thread(work);
    } catch (const std::exception &) {
      work();
    }
  }
  ~GroupFeed() {
    if (th.joinable()) th.join();
  }
  void post(int g) { posted.store(g + 1, std::memory_order_release); }
  // nonzero: the body or the wait failed, and the caller returns join(R)
  int wait(Run &R, int g) {
    while (posted.load(std::memory_order_acquire) <= g) std::this_thread::yield();
    if (posted.load(std::memory_order_acquire) >= DONE && Q.rc != LF_OK) return Q.rc;
    return R.wait(R.P->ev[2 + g]);
  }
  int join(Run &R) {
    if (th.joinable()) th.join();
    if (Q.rc != LF_OK && R.rc == LF_OK) {
      R.rc = Q.rc;
      R.errs() = err;
    }
    return R.rc;
  }
};

// what crosses the phases of one lf_fold_prove
struct Fold {
  const lf_witness *w_acc, *w_i, *w_out;
  lf_lcccs_mut *out;
  lf_lfproof_mut *proof;
  // host copies of the public inputs in canonical form: the accumulator's r, v, cm, u, x_w, h; cm_i, x_ccs
  std::vector<uint64_t> ar, av, acm, au, axw, ah, cmi, xc;
  std::vector<uint64_t> r_lin, lv, lu;  // the linearized instance: {r, v, cm_i, u, x_ccs, h = ONE}
  std::vector<uint64_t> r0;             // the folding sumcheck's point
  std::vector<uint64_t> rhoc;           // the rho_s' coefficients
  std::vector<uint64_t> x0;             // x_0 = x_w || h of the folded instance
  lf_fold_step_bufs b{};                // the decomposition's buffers, which the fold completes
  // the folding MLEs [eq(r_0), g1, eq(r_1), g3, eq(beta), f_hat (2K x tau)], mstride words apart
  uint64_t *M = nullptr;
  size_t mstride = 0;
  int ng = 0;           // instance groups per side
  bool digits = false;  // B_SMALL = 2, f_hat values in {-1, 0, 1}: read from the coefficient rows
  std::optional<GroupFeed> feed;  // declared last: joined before anything its body reads goes away
};

// ---------------------------------------------------------------- linearization

// z = x_ccs || 1 || w_ccs (Instance::get_z_vector) and its Mz MLEs: independent of the
// transcript, so enqueued before the public input is absorbed (the device computes
// them while the host hashes). Live matrices first (lf_prover::mz_order).
int linearize_prepare(lf_prover *P, Run &R, const std::vector<uint64_t> &xc, const lf_witness *w_i) {
  const int d = P->d;
  R.h2d(P->z, xc.data(), P->l * d);
  R.h2d(P->z + P->l * d, P->one.data(), d);
  R.d2d(P->z + (P->l + 1) * d, w_i->w_ccs, P->W * d);
  return R.check(lf_dev_mz_mles_sel(P->ctx, P->ccs, P->z, P->mz_order.data(), P->t, P->s, P->mz), "Mz MLEs");
}

// LFLinearizationProver::prove (linearization.rs:153-197) of the CCCS (cm, x_ccs)
// with witness w (its Mz MLEs from linearize_prepare), on the transcript R.T: the
// sumcheck messages into lin_sumcheck (host), and r, v, u of the linearized instance
// {r, v, cm, u, x_ccs, ONE}
int linearize(lf_prover *P, Run &R, const lf_witness *w_i, uint64_t *lin_sumcheck, std::vector<uint64_t> &r_lin,
              std::vector<uint64_t> &lv, std::vector<uint64_t> &lu) {
  lf_ctx *C = P->ctx;
  const int d = P->d, tb = P->tb, tau = P->tau, s = P->s, t = P->t, nlive = P->nlive;
  const size_t N = P->N, nn = P->nn, len = nn * d;
  R.absorb_label("beta_s");  // squeeze_beta_challenges (linearization/utils.rs:111-124)
  const std::vector<uint64_t> beta = R.challenges(s);
  // The MLE list is [MLE(M_j z) for each (i, j in S_i) with c_i != 0] + [eq(beta)]
  // (linearization/utils.rs:71-84), and the combination reads list position j for
  // matrix index j (as the reference does) and the last entry -- so only the live
  // matrices' MLEs are read, each where the Mz products left it (a pointer table;
  // no copies), and eq(beta) is split off each round (lf_sumcheck_prove_lin: beta
  // itself, no eq MLE); P->lin (nlive x m/4 elements) serves the later rounds.
  std::vector<const uint64_t *> ptr(nlive);
  for (int i = 0; i < nlive; i++) ptr[i] = P->mz + (size_t)i * len;
  std::vector<uint64_t> rnd((size_t)s * tb);
  {
    lf_comb cb{};
    cb.kind = LF_COMB_LINEARIZATION;
    cb.q = P->q;
    cb.c = lf_ccs_c_device(P->ccs);
    cb.S_off = P->S_off.data();
    cb.S_idx = P->S_live.data();
    if (R.rc == LF_OK)
      R.check(lf_sumcheck_prove_lin_sparse(C, R.T, &cb, ptr.data(), nlive, s, d, P->degree + 1, beta.data(), P->act,
                                           P->act_off.data(), P->lin, lin_sumcheck, rnd.data(), P->lev),
              "linearization sumcheck");
  }
  if (R.rc) return R.rc;
  r_lin = R.point(rnd);
  R.h2d(P->pt, r_lin.data(), (size_t)s * d);
  // v = f_hat(w_i) at r, u = MLE(M_j z)(r) (compute_evaluation_vectors, :130-147): the
  // live matrices' u are the sumcheck's final values, the others are evaluated against
  // one eq(r) table -- built where the folding prover's eq(r_1) MLE lives, which it is
  uint64_t *eq_lin = P->fold + 2 * nn * d;
  R.check(lf_dev_eq_table(C, d, P->pt, s, eq_lin), "eq(r)");
  R.check(lf_dev_fhat_evaluate_eq(C, d, w_i->f_coeff, N, 0, 1, s, eq_lin, P->val), "v");
  if (t > nlive)
    R.check(lf_dev_mle_evaluate_eq(C, d, P->mz + (size_t)nlive * len, t - nlive, s, eq_lin, P->val + (size_t)tau * d),
            "u");
  lv.assign((size_t)tau * d, 0);
  std::vector<uint64_t> ub((size_t)t * d);
  R.d2h(lv.data(), P->val, (size_t)tau * d);
  R.d2h(ub.data(), P->val + (size_t)tau * d, (size_t)(t - nlive) * d);
  R.d2h(ub.data() + (size_t)(t - nlive) * d, P->lev, (size_t)nlive * d);
  if (R.rc) return R.rc;
  lu.assign((size_t)t * d, 0);
  for (int i = 0; i < t; i++) {  // position i of mz_order is matrix mz_order[i]
    const uint64_t *src = i < nlive ? ub.data() + (size_t)(t - nlive + i) * d : ub.data() + (size_t)(i - nlive) * d;
    memcpy(lu.data() + (size_t)P->mz_order[i] * d, src, d * 8);
  }
  R.absorb(lv.data(), tau);
  R.absorb(lu.data(), t);
  return LF_OK;
}

// ---------------------------------------------------------------- the phases of lf_fold_prove
// One function per LF_SPAN_* span, in protocol order (FOLD_PHASES below); each returns
// nonzero to end the call with that status.

// absorb_public_input (zk_latticefold.rs:162-184)
int public_input(lf_prover *P, Run &R, Fold &F) {
  // the linearization's Mz MLEs need no challenge: on the device while the host absorbs
  if (linearize_prepare(P, R, F.xc, F.w_i)) return R.rc;
  R.absorb_label("acc");
  R.absorb(F.ar.data(), P->s);
  R.absorb(F.av.data(), P->tau);
  R.absorb(F.acm.data(), P->kappa);
  R.absorb(F.au.data(), P->t);
  R.absorb(F.axw.data(), P->l);
  R.absorb(F.ah.data(), 1);
  R.absorb_label("cm_i");
  R.absorb(F.cmi.data(), P->kappa);
  R.absorb(F.xc.data(), P->l);
  return LF_OK;
}

// linearization (linearization.rs:153-197)
int linearization(lf_prover *P, Run &R, Fold &F) {
  return linearize(P, R, F.w_i, F.proof->lin_sumcheck, F.r_lin, F.lv, F.lu);
}

// one side's v_s and u_s at its point r_i, and its messages back to pinned memory
void enqueue_decomposed_side(lf_prover *P, GroupFeed &E, const Fold &F, int side) {
  lf_ctx *C = P->ctx;
  Run &Q = E.Q;
  const int d = P->d, tau = P->tau, s = P->s, K = P->K, t = P->t, G = MZ_GROUP;
  const size_t N = P->N, n = P->n, l = P->l, kd = P->kappa * d;
  const uint64_t *eq_s = F.M + (size_t)(2 * side) * F.mstride;
  uint64_t *vs = P->vs + (size_t)side * K * tau * d;
  Q.check(P->lean ? lf_dev_fhat_evaluate_planes(C, &P->pr, P->planes[side], N, s, eq_s, vs)
                  : lf_dev_fhat_evaluate_eq(C, d, P->fkc[side], N, N * d, K, s, eq_s, vs),
          "v_s");
  Q.d2p(P->hx[side], P->xs + (size_t)side * K * (l + 1) * d, (size_t)K * (l + 1) * d);
  Q.d2p(P->hy[side], P->y[side], (size_t)K * kd);
  Q.d2p(P->hv[side], P->vs + (size_t)side * K * tau * d, (size_t)K * tau * d);
  Q.check(lf_dev_mz_weights(C, P->ccs, s, eq_s, P->mzw), "u_s weights");
  for (int g = 0; g < F.ng; g++) {
    const int k0 = g * G, nk = std::min(G, K - k0);
    uint64_t *us = P->us + ((size_t)side * K + k0) * t * d;
    Q.check(lf_dev_mz_dots(C, P->ccs, P->mzw, P->zdec[side] + (size_t)k0 * n * d, nk, us), "u_s");
    Q.d2p(P->hu[side] + (size_t)k0 * t * d, us, (size_t)nk * t * d);
    Q.hip(hipEventRecord(P->ev[2 + side * F.ng + g], Q.st), "event");
    E.post(side * F.ng + g);
  }
}

// the two decompositions (decomposition.rs:33-88), device work of both first
int decomposition(lf_prover *P, Run &R, Fold &F) {
  lf_ctx *C = P->ctx;
  const int d = P->d, s = P->s, K = P->K;
  const size_t W = P->W, l = P->l, kd = P->kappa * d;
  R.h2d(P->cmd[0], F.acm.data(), kd);
  R.h2d(P->cmd[1], F.cmi.data(), kd);
  R.h2d(P->xw[0], F.axw.data(), l * d);  // x_w || h of each side
  R.h2d(P->xw[0] + l * d, F.ah.data(), d);
  R.h2d(P->xw[1], F.xc.data(), l * d);
  R.h2d(P->xw[1] + l * d, P->one.data(), d);
  for (int side = 0; side < 2; side++)
    R.check(lf_dev_compute_x_s(C, &P->pr, P->xw[side], l + 1, P->xs + (size_t)side * K * (l + 1) * d), "compute_x_s");
  lf_fold_step_bufs &b = F.b;
  b.acc_f_coeff = F.w_acc->f_coeff;
  b.f_coeff = const_cast<uint64_t *>(F.w_i->f_coeff);
  b.acc_cm = P->cmd[0];
  b.cm = P->cmd[1];
  for (int side = 0; side < 2; side++) {
    b.fk_coeff[side] = P->fkc[side];  // lean: NULL, the planes are the decomposed witnesses' only form
    b.fk[side] = P->fk[side];
    b.planes[side] = P->planes[side];
    b.wk[side] = P->wk[side];
    b.y[side] = P->y[side];
  }
  if (R.rc == LF_OK) R.check(lf_dev_decompose_commit(C, P->aj, &P->pr, W, &b), "decompose + commit_witnesses");
  // z_k = x_s[k] || w_ccs_k (compute_mz_mles, :229-256) for the u_s (and later eta_s), one
  // launch per side (the stream's queue holds a bounded number of commands: every one
  // saved is host time the transcript gets back)
  for (int side = 0; side < 2; side++)
    R.hip(lfk::assemble_z(P->xs + (size_t)side * K * (l + 1) * d, P->wk[side], K, l + 1, W, d, P->zdec[side], R.st),
          "z_k");
  // per side: v_s, u_s at the side's point, then its messages back to pinned memory
  // behind events, so the host absorbs while the device evaluates: x_s, y_s and v_s
  // of a side first, then u_s in groups of MZ_GROUP instances (one event each: the
  // host starts on instance 0 as soon as its u_s is back), and the challenge-
  // independent folding MLEs (the f_hat MLEs of the 2K decomposed witnesses, eq(r_i);
  // create_sumcheck_polynomial, folding/utils.rs:196-255) behind them
  // eq(r_i) of each side is the folding prover's eq(r_i) MLE (M slots 0 and 2; the
  // linearization left eq(r_lin) in slot 2): v_s and u_s read it from there
  R.h2p2d(P->pt, P->hr[0], F.ar.data(), (size_t)s * d);
  R.check(lf_dev_eq_table(C, d, P->pt, s, F.M), "eq(r_0)");
  F.feed.emplace(R, [P, &F](GroupFeed &E) {
    enqueue_decomposed_side(P, E, F, 0);
    enqueue_decomposed_side(P, E, F, 1);
    if (!F.digits)
      for (int sd = 0; sd < 2; sd++)
        E.Q.hip(lfk::get_fhat(P->fkc[sd], P->N, P->d, P->s, F.M + (5 + (size_t)sd * P->K * P->tau) * F.mstride, E.Q.st,
                              P->K, P->N * P->d),
                "f_hat");
  });
  return LF_OK;
}

// the decomposed instances' messages (:58-64), each group once its event has fired
int decomposition_transcript(lf_prover *P, Run &R, Fold &F) {
  const int d = P->d, tau = P->tau, K = P->K, t = P->t;
  const size_t l = P->l, kappa = P->kappa, kd = kappa * d;
  lf_lfproof_mut *proof = F.proof;
  for (int side = 0; side < 2; side++)
    for (int k = 0; k < K; k++) {
      if (k % MZ_GROUP == 0 && F.feed->wait(R, side * F.ng + k / MZ_GROUP)) return F.feed->join(R);
      const size_t ox = (size_t)k * (l + 1) * d, oy = (size_t)k * kd, ou = (size_t)k * t * d, ov = (size_t)k * tau * d;
      memcpy(proof->x_s[side] + ox, P->hx[side] + ox, (l + 1) * d * 8);
      memcpy(proof->y_s[side] + oy, P->hy[side] + oy, kd * 8);
      memcpy(proof->u_s[side] + ou, P->hu[side] + ou, (size_t)t * d * 8);
      memcpy(proof->v_s[side] + ov, P->hv[side] + ov, (size_t)tau * d * 8);
      R.absorb(proof->x_s[side] + ox, l + 1);
      R.absorb(proof->y_s[side] + oy, kappa);
      R.absorb(proof->u_s[side] + ou, t);
      R.absorb(proof->v_s[side] + ov, tau);
    }
  return F.feed->join(R);
}

// folding (folding.rs:42-130): its challenges and the MLEs that depend on them
int folding_mles(lf_prover *P, Run &R, Fold &F) {
  lf_ctx *C = P->ctx;
  const int d = P->d, tb = P->tb, tau = P->tau, s = P->s, K = P->K;
  const size_t N = P->N, mstride = F.mstride;
  uint64_t *M = F.M;
  R.absorb_label("alpha_s");  // squeeze_alpha_beta_zeta_mu (folding/utils.rs:51-96)
  const std::vector<uint64_t> alpha = R.challenges(2 * K);
  R.absorb_label("zeta_s");
  const std::vector<uint64_t> zeta = R.challenges(2 * K);
  R.absorb_label("mu_s");
  std::vector<uint64_t> mu = R.challenges(2 * K - 1);
  mu.insert(mu.end(), P->one.begin(), P->one.end());
  R.absorb_label("beta_s");
  const std::vector<uint64_t> fbeta = R.challenges(s);
  R.h2d(P->zeta, zeta.data(), 2 * (size_t)K * d);
  R.h2d(P->mu, mu.data(), 2 * (size_t)K * d);
  R.h2d(P->beta, fbeta.data(), (size_t)s * d);
  // Horner weights alpha_k^(j+1) of each side's f_hat MLEs (prepare_g1_and_3_k_mles_list, :519-541)
  for (int side = 0; side < 2; side++) {
    std::vector<uint64_t> cf((size_t)K * tau * d);
    for (int k = 0; k < K; k++) {
      const uint64_t *a = alpha.data() + (size_t)(side * K + k) * d;  // broadcast: slot 0 holds the base value
      uint64_t pw[3] = {a[0], tb == 3 ? a[1] : 0, tb == 3 ? a[2] : 0};
      for (int j = 0; j < tau; j++) {
        broadcast(pw, tb, d, cf.data() + ((size_t)k * tau + j) * d);
        uint64_t nx[3];
        gl::base_mul(pw, a, nx, tb);
        memcpy(pw, nx, sizeof(pw));
      }
    }
    R.h2d(P->coef[side], cf.data(), cf.size());
  }
  // the MLEs [eq(r_0), g1, eq(r_1), g3, eq(beta), f_hat (2K x tau)] (create_sumcheck_polynomial,
  // :196-255): eq(r_i) were enqueued before the decomposition transcript; the f_hat MLEs
  // (Witness::get_fhat of the decomposed witnesses) are not materialised for B_SMALL = 2 --
  // their values are the digits of the coefficient rows P->fkc, which g1 / g3 and the
  // sumcheck's first round read directly (lf_sumcheck_prove_fold_digits)
  // both sides' challenged Mz MLEs in one pass over the matrices (g1, g3 slots)
  R.check(lf_dev_mz_challenged_pair(C, P->ccs, P->zdec[0], P->zeta, P->zdec[1], P->zeta + (size_t)K * d, K, s,
                                    M + mstride, M + 3 * mstride),
          "challenged Mz");
  for (int side = 0; side < 2; side++) {
    uint64_t *g = M + (size_t)(2 * side + 1) * mstride;
    if (P->lean)
      R.check(lf_dev_fhat_lincomb_planes(C, &P->pr, P->planes[side], N, s, P->coef[side], g), "g");
    else if (F.digits)
      R.hip(lfk::fhat_lincomb_digits(P->fkc[side], K, N, N * d, P->coef[side], s, d, g, R.st), "g");
    else
      R.check(lf_dev_mle_lincomb(C, d, M + (5 + (size_t)side * K * tau) * mstride, mstride, K * tau, s, P->coef[side], g),
              "g");
  }
  R.check(lf_dev_eq_table(C, d, P->beta, s, M + 4 * mstride), "eq(beta)");
  return LF_OK;
}

int folding_sumcheck(lf_prover *P, Run &R, Fold &F) {
  const int d = P->d, s = P->s, K = P->K;
  const size_t N = P->N;
  std::vector<uint64_t> rnd((size_t)s * P->tb);
  lf_comb cb{};
  cb.kind = LF_COMB_FOLDING;
  cb.nk = 2 * K;
  cb.tau = P->tau;
  cb.bsmall = (int)P->pr.b_small;
  cb.mu = P->mu;
  if (R.rc == LF_OK && P->lean)
    R.check(lf_sumcheck_prove_fold_planes(P->ctx, R.T, &cb, F.M, &P->pr, P->planes[0], P->planes[1], N, s,
                                          F.M + 5 * F.mstride, F.proof->fold_sumcheck, rnd.data()),
            "folding sumcheck");
  else if (R.rc == LF_OK)
    R.check(F.digits ? lf_sumcheck_prove_fold_digits(P->ctx, R.T, &cb, F.M, P->fkc[0], P->fkc[1], K, N, N * d, s, d,
                                                     F.M + 5 * F.mstride, F.proof->fold_sumcheck, rnd.data())
                     : lf_sumcheck_prove(P->ctx, R.T, &cb, F.M, P->nm_fold, s, d, 2 * cb.bsmall, F.proof->fold_sumcheck,
                                         rnd.data()),
            "folding sumcheck");
  if (R.rc == LF_OK) F.r0 = R.point(rnd);
  return R.rc;
}

// theta_s = f_hat(w_i)(r_0), eta_s = MLE(M_j z_i)(r_0) (get_thetas / get_etas, :236-256):
// theta_s and side 0's eta_s come back first, so the host absorbs them while the
// device evaluates side 1's eta_s
int evaluations(lf_prover *P, Run &R, Fold &F) {
  lf_ctx *C = P->ctx;
  const int d = P->d, tau = P->tau, s = P->s, K = P->K;
  const size_t N = P->N;
  R.h2d(P->r0, F.r0.data(), (size_t)s * d);
  // one eq(r_0) table and one set of Mz weights at r_0 for both sides
  R.check(lf_dev_eq_table(C, d, P->r0, s, P->eq0), "eq(r_0)");
  for (int side = 0; side < 2; side++) {
    uint64_t *th = P->theta + (size_t)side * K * tau * d;
    R.check(P->lean ? lf_dev_fhat_evaluate_planes(C, &P->pr, P->planes[side], N, s, P->eq0, th)
                    : lf_dev_fhat_evaluate_eq(C, d, P->fkc[side], N, N * d, K, s, P->eq0, th),
            "theta");
  }
  R.d2p(P->htheta, P->theta, 2 * (size_t)K * tau * d);
  R.hip(hipEventRecord(P->ev[0], R.st), "event");
  R.check(lf_dev_mz_weights(C, P->ccs, s, P->eq0, P->mzw), "eta weights");
  if (R.rc) return R.rc;
  // the eta_s groups of both sides from a second host thread, as the u_s groups
  F.feed.emplace(R, [P, &F](GroupFeed &E) {
    Run &Q = E.Q;
    const int K = P->K, G = MZ_GROUP;
    const size_t td = (size_t)P->t * P->d;
    for (int side = 0; side < 2 && Q.rc == LF_OK; side++)
      for (int gg = 0; gg < F.ng; gg++) {  // instance groups in absorb order
        const int g = side * F.ng + gg, k0 = gg * G, nk = std::min(G, K - k0);
        const size_t o = ((size_t)side * K + k0) * td;
        Q.check(lf_dev_mz_dots(P->ctx, P->ccs, P->mzw, P->zdec[side] + (size_t)k0 * P->n * P->d, nk, P->eta + o),
                "eta");
        Q.d2p(P->heta + o, P->eta + o, (size_t)nk * td);
        Q.hip(hipEventRecord(P->ev[2 + g], Q.st), "event");
        E.post(g);
      }
  });
  return LF_OK;
}

// theta_s and eta_s into the transcript as they arrive, then the rho_s
int folding_transcript(lf_prover *P, Run &R, Fold &F) {
  const int d = P->d, tau = P->tau, K = P->K, t = P->t;
  lf_lfproof_mut *proof = F.proof;
  if (R.wait(P->ev[0])) return F.feed->join(R);
  memcpy(proof->theta_s, P->htheta, 2 * (size_t)K * tau * d * 8);
  for (int i = 0; i < 2 * K; i++) R.absorb(proof->theta_s + (size_t)i * tau * d, tau);
  for (int side = 0; side < 2; side++)
    for (int k = 0; k < K; k++) {
      if (k % MZ_GROUP == 0 && F.feed->wait(R, side * F.ng + k / MZ_GROUP)) return F.feed->join(R);
      const size_t o = ((size_t)side * K + k) * t * d;
      memcpy(proof->eta_s + o, P->heta + o, (size_t)t * d * 8);
      R.absorb(proof->eta_s + o, t);
    }
  if (F.feed->join(R)) return R.rc;
  // get_rhos (folding/utils.rs:116-127): 2K - 1 short challenges and ONE, then CRT
  R.absorb_label("rho_s");
  F.rhoc.assign(2 * (size_t)K * d, 0);
  if (lf_transcript_get_short_challenges(R.T, d, 2 * K - 1, F.rhoc.data()) != LF_OK)
    return bad(P, LF_ERR_CHALLENGE_BYTES, "short challenges");
  F.rhoc[(size_t)(2 * K - 1) * d] = 1;
  return LF_OK;
}

// f_0, cm_0, Witness::from_f(f_0) (:112-122), then v_0, u_0, x_0 (compute_v0_u0_x0_cm_0, :456-517)
int fold_and_outputs(lf_prover *P, Run &R, Fold &F) {
  lf_ctx *C = P->ctx;
  const int d = P->d, K = P->K, t = P->t;
  const size_t l = P->l;
  R.h2d(P->rhoc, F.rhoc.data(), F.rhoc.size());
  R.d2d(P->rho, P->rhoc, F.rhoc.size());
  R.check(lf_dev_crt(C, P->rho, 2 * K, d), "CRT(rho)");
  lf_fold_step_bufs &b = F.b;
  b.rho = P->rho;
  b.f0 = F.w_out->f;
  b.f0_coeff = F.w_out->f_coeff;
  b.w_ccs0 = F.w_out->w_ccs;
  b.cm0 = P->cm0;
  if (R.rc == LF_OK) R.check(lf_dev_fold_combine(C, P->aj, &P->pr, P->W, &b), "fold");
  R.check(lf_dev_fold_lcccs(C, d, 2 * K, P->rho, P->rhoc, P->eta, t, P->xs, l + 1, P->theta, P->u0, P->x0, P->v0),
          "v_0, u_0, x_0");
  if (R.rc) return R.rc;
  // prepare_public_output (folding.rs:381-392): x_w = x_0[..l], h = x_0[l]
  F.x0.resize((l + 1) * d);
  R.d2h(F.out->cm, P->cm0, P->kappa * d);
  R.d2h(F.out->u, P->u0, (size_t)t * d);
  R.d2h(F.out->v, P->v0, (size_t)P->tau * d);
  R.d2h(F.x0.data(), P->x0, (l + 1) * d);
  R.check(lf_ctx_sync(C), "sync");
  return R.rc;
}

// the phases in protocol order, each with the span it closes; sync = false: see Run::mark
constexpr struct {
  int (*run)(lf_prover *, Run &, Fold &);
  int span;
  bool sync;
} FOLD_PHASES[] = {{public_input, LF_SPAN_PUBLIC_INPUT, false},
                   {linearization, LF_SPAN_LINEARIZATION, true},
                   {decomposition, LF_SPAN_DECOMPOSITION, false},
                   {decomposition_transcript, LF_SPAN_DECOMPOSITION_TRANSCRIPT, false},
                   {folding_mles, LF_SPAN_FOLDING_MLES, true},
                   {folding_sumcheck, LF_SPAN_FOLDING_SUMCHECK, true},
                   {evaluations, LF_SPAN_EVALUATIONS, false},
                   {folding_transcript, LF_SPAN_FOLDING_TRANSCRIPT, true},
                   {fold_and_outputs, LF_SPAN_FOLD, true}};

// The checks a witness answers for on its own and against its commitment, shared by
// lf_lcccs_check and lf_cccs_check: LF_REL_WITNESS_F, _W (Witness::from_f of f against
// f_coeff and w_ccs: f = CRT(f_coeff) iff ICRT(f) = f_coeff), LF_REL_NORM and LF_REL_CM
// (Witness::commit, arith.rs:357). cm: host, canonical. *failed = the first that fails
// (LF_REL_OK: none); the return value is R.rc
int witness_checks(lf_prover *P, Run &R, const lf_witness *w, const uint64_t *cm, uint64_t bound, uint64_t *norm,
                   int *failed) {
  lf_ctx *C = P->ctx;
  const int d = P->d;
  const size_t N = P->N, W = P->W, kd = P->kappa * d;
  *failed = LF_REL_OK;
  // N and W elements of the decomposition's buffers (lean: its N-element scratch)
  uint64_t *fc = P->lean ? P->scr : P->fkc[0], *wc = P->wk[0];
  R.check(lf_dev_witness_from_f(C, &P->pr, w->f, N, fc, wc), "Witness::from_f");
  if (R.rc) return R.rc;
  R.hip(lfk::first_diff(fc, w->f_coeff, N * d, P->chk, R.st), "compare f_coeff");
  R.hip(lfk::first_diff(wc, w->w_ccs, W * d, P->chk + 1, R.st), "compare w_ccs");
  uint64_t diff[2] = {0, 0}, nm = 0;
  R.d2h(diff, P->chk, 2);
  R.check(lf_dev_linf_norm(C, w->f_coeff, N * d, &nm), "linf norm");
  if (R.rc) return R.rc;
  if (norm) *norm = nm;
  if (diff[0] != ~0ull) return *failed = LF_REL_WITNESS_F, R.rc;
  if (diff[1] != ~0ull) return *failed = LF_REL_WITNESS_W, R.rc;
  if (bound && nm >= bound) return *failed = LF_REL_NORM, R.rc;
  const uint64_t *vecs[1] = {w->f};
  R.check(lf_dev_ajtai_commit(C, P->aj, vecs, 1, P->cmd[0]), "commit");
  std::vector<uint64_t> got(kd);
  R.d2h(got.data(), P->cmd[0], kd);
  if (R.rc) return R.rc;
  if (memcmp(got.data(), cm, kd * 8)) *failed = LF_REL_CM;
  return R.rc;
}

// z = x || h || w_ccs in P->z (get_z_vector, arith.rs:411-420); x: l host elements, h: one
void assemble_z(lf_prover *P, Run &R, const uint64_t *x, const uint64_t *h, const lf_witness *w) {
  const int d = P->d;
  R.h2d(P->z, x, P->l * d);
  R.h2d(P->z + P->l * d, h, d);
  R.d2d(P->z + (P->l + 1) * d, w->w_ccs, P->W * d);
}

}  // namespace

extern "C" {

static int prover_create(lf_ctx *ctx, const lf_ajtai *aj, const lf_params *pr, const lf_ccs *ccs, bool lean,
                         lf_prover **out) {
  if (!ctx || !aj || !pr || !ccs || !out) return LF_ERR_INVALID_ARG;
  *out = nullptr;
  auto P = std::make_unique<lf_prover>();
  P->ctx = ctx;
  P->aj = aj;
  P->ccs = ccs;
  P->pr = *pr;
  P->device = lf_ctx_device(ctx);
  P->lean = lean;
  LF_TRY(prover_shape(P.get()));
  if (lean) {
    DevGuard g(P->device);
    LF_TRY(step_packed_form(ctx, aj, pr));
  }
  linearization_mle_list(P.get());
  LF_TRY(live_matrix_order(P.get()));
  active_points(P.get());
  LF_TRY(prover_alloc(P.get()));
  *out = P.release();
  return LF_OK;
}

int lf_prover_create(lf_ctx *ctx, const lf_ajtai *aj, const lf_params *pr, const lf_ccs *ccs, lf_prover **out) {
  return prover_create(ctx, aj, pr, ccs, false, out);
}

int lf_prover_create_lean(lf_ctx *ctx, const lf_ajtai *aj, const lf_params *pr, const lf_ccs *ccs, lf_prover **out) {
  return prover_create(ctx, aj, pr, ccs, true, out);
}

int lf_prover_is_lean(const lf_prover *P) { return P && P->lean ? 1 : 0; }

size_t lf_prover_device_bytes(const lf_prover *P) { return P ? P->mem_elems * 8 : 0; }

void lf_prover_destroy(lf_prover *P) { delete P; }

int lf_linearize(lf_prover *P, const uint64_t *cm, const uint64_t *x_ccs, const lf_witness *w, lf_lcccs_mut *out,
                 uint64_t *lin_sumcheck, int repr) {
  if (!P || !cm || (!x_ccs && P->l) || !w || !witness_ok(w, false, true) || !out || !lin_sumcheck ||
      !lcccs_out_ok(P, out))
    return LF_ERR_INVALID_ARG;
  if (!repr_ok(repr)) return bad(P, LF_ERR_INVALID_ARG, "repr");
  const int d = P->d;
  const size_t l = P->l, kd = P->kappa * d;
  const std::vector<uint64_t> cmv = canon(cm, kd, repr), xc = canon(x_ccs, l * d, repr);
  DevGuard dg(P->device);
  Run R{P, lf_transcript_new(), (hipStream_t)lf_ctx_get_stream(P->ctx)};
  TGuard tg{R.T};
  std::vector<uint64_t> r_lin, lv, lu;
  if (linearize_prepare(P, R, xc, w) || linearize(P, R, w, lin_sumcheck, r_lin, lv, lu)) return R.rc;
  // the LCCCS {r, v, cm, u, x_w = x_ccs, h = ONE} (linearization.rs:185-193)
  memcpy(out->r, r_lin.data(), r_lin.size() * 8);
  memcpy(out->v, lv.data(), lv.size() * 8);
  memcpy(out->cm, cmv.data(), kd * 8);
  memcpy(out->u, lu.data(), lu.size() * 8);
  if (l) memcpy(out->x_w, xc.data(), l * d * 8);
  memcpy(out->h, P->one.data(), d * 8);
  if (repr == LF_REPR_MONTGOMERY) {
    lcccs_to_mont(P, out);
    to_mont(lin_sumcheck, (size_t)P->s * (P->degree + 2) * d);
  }
  return LF_OK;
}

const char *lf_prover_last_error(const lf_prover *P) { return P ? P->err.c_str() : ""; }

int lf_prover_timing(lf_prover *P, int enable, double *span_ms) {
  if (!P) return LF_ERR_INVALID_ARG;
  if (span_ms) memcpy(span_ms, P->span_ms, sizeof(P->span_ms));
  P->timing = enable != 0;
  memset(P->span_ms, 0, sizeof(P->span_ms));
  return LF_OK;
}

int lf_fold_prove(lf_prover *P, const lf_lcccs *acc, const lf_witness *w_acc, const uint64_t *cm_i,
                  const uint64_t *x_ccs, const lf_witness *w_i, lf_lcccs_mut *out, const lf_witness *w_out,
                  lf_lfproof_mut *proof, int repr) {
  if (!P || !acc || !w_acc || !cm_i || (!x_ccs && P->l) || !w_i || !out || !w_out || !proof) return LF_ERR_INVALID_ARG;
  if (!repr_ok(repr)) return bad(P, LF_ERR_INVALID_ARG, "repr");
  const size_t d = P->d, s = P->s, tau = P->tau, K = P->K, t = P->t, l = P->l, kd = P->kappa * d;
  if (!lcccs_sizes_ok(P, acc))
    return bad(P, LF_ERR_INCORRECT_LENGTH, "accumulator LCCCS sizes (r: s, v: tau, cm: kappa, u: t, x_w: l)");
  if (!witness_ok(w_acc, false, false) || !witness_ok(w_i, false, true) || !witness_ok(w_out, true, true))
    return bad(P, LF_ERR_INVALID_ARG, "missing witness buffer");
  if (!proof->lin_sumcheck || !proof->lin_v || !proof->lin_u || !proof->fold_sumcheck || !proof->theta_s ||
      !proof->eta_s || !lcccs_out_ok(P, out))
    return bad(P, LF_ERR_INVALID_ARG, "missing output buffer");
  for (int side = 0; side < 2; side++)
    if (!proof->u_s[side] || !proof->v_s[side] || !proof->x_s[side] || !proof->y_s[side])
      return bad(P, LF_ERR_INVALID_ARG, "missing decomposition proof buffer");
  Run R{P, lf_transcript_new(), (hipStream_t)lf_ctx_get_stream(P->ctx)};
  TGuard tg{R.T};
  lf_transcript_record(R.T);
  P->samples.clear();
  DevGuard dg(P->device);
  Fold F{w_acc, w_i, w_out, out, proof};
  F.ar = canon(acc->r.elems, s * d, repr);
  F.av = canon(acc->v.elems, tau * d, repr);
  F.acm = canon(acc->cm.elems, kd, repr);
  F.au = canon(acc->u.elems, t * d, repr);
  F.axw = canon(acc->x_w.elems, l * d, repr);
  F.ah = canon(acc->h, d, repr);
  F.cmi = canon(cm_i, kd, repr);
  F.xc = canon(x_ccs, l * d, repr);
  F.M = P->fold;
  F.mstride = P->nn * d;
  F.ng = (P->K + MZ_GROUP - 1) / MZ_GROUP;
  F.digits = P->pr.b_small == 2;
  for (const auto &ph : FOLD_PHASES) {
    if (const int rc = ph.run(P, R, F)) return rc;
    R.mark(ph.span, ph.sync);
  }
  P->samples.resize(lf_transcript_samples(R.T, nullptr, 0));
  lf_transcript_samples(R.T, P->samples.data(), P->samples.size());
  memcpy(out->r, F.r0.data(), F.r0.size() * 8);
  if (l) memcpy(out->x_w, F.x0.data(), l * d * 8);
  memcpy(out->h, F.x0.data() + l * d, d * 8);
  memcpy(proof->lin_v, F.lv.data(), F.lv.size() * 8);
  memcpy(proof->lin_u, F.lu.data(), F.lu.size() * 8);
  if (repr == LF_REPR_MONTGOMERY) {
    lcccs_to_mont(P, out);
    to_mont(proof->lin_sumcheck, s * (P->degree + 2) * d);
    to_mont(proof->lin_v, tau * d);
    to_mont(proof->lin_u, t * d);
    for (int side = 0; side < 2; side++) {
      to_mont(proof->u_s[side], K * t * d);
      to_mont(proof->v_s[side], K * tau * d);
      to_mont(proof->x_s[side], K * (l + 1) * d);
      to_mont(proof->y_s[side], K * kd);
    }
    to_mont(proof->fold_sumcheck, s * (2 * P->pr.b_small + 1) * d);
    to_mont(proof->theta_s, 2 * K * tau * d);
    to_mont(proof->eta_s, 2 * K * t * d);
  }
  return LF_OK;
}

// fold() followed by generate_verification_witness_vars (zk_latticefold.rs:111-148),
// as main.rs:175-185 runs them: the vars come from a replay of the proof on this
// call's own sample log (lf_fold_replay_samples) -- bit for bit what lf_fold_replay's
// second Poseidon2 pass over the same messages gives, without the permutations
int lf_fold_prove_vars(lf_prover *P, const lf_lcccs *acc, const lf_witness *w_acc, const uint64_t *cm_i,
                       const uint64_t *x_ccs, const lf_witness *w_i, lf_lcccs_mut *out, const lf_witness *w_out,
                       lf_lfproof_mut *proof, lf_replay_vars *vars, int repr) {
  if (!vars) return LF_ERR_INVALID_ARG;
  const int rc = lf_fold_prove(P, acc, w_acc, cm_i, x_ccs, w_i, out, w_out, proof, repr);
  if (rc != LF_OK) return rc;
  if (P->d != 24) return bad(P, LF_ERR_UNSUPPORTED_RING, "verification vars: Phi_72 only (TAU = 3)");
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint64_t> c = P->c;
  if (repr == LF_REPR_MONTGOMERY)
    for (auto &x : c) x = gl::to_mont(x);
  lf_ccs_desc desc{};
  desc.t = P->t;
  desc.m = P->nn;
  desc.l = P->l;
  desc.degree = P->degree;
  desc.q = P->q;
  desc.c = c.data();
  desc.S_off = P->S_off.data();
  desc.S_idx = P->S_idx.data();
  const int r = lf_fold_replay_samples(&desc, &P->pr, acc, cm_i, x_ccs, proof, P->samples.data(), P->samples.size(),
                                       vars, repr);
  if (P->timing)
    P->span_ms[LF_SPAN_VARS] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return r == LF_OK ? LF_OK : bad(P, r, "verification vars replay");
}

size_t lf_prover_samples(const lf_prover *P, uint64_t *out, size_t cap) {
  if (!P) return 0;
  if (out) memcpy(out, P->samples.data(), (cap < P->samples.size() ? cap : P->samples.size()) * 8);
  return P->samples.size();
}

// ---------------------------------------------------------------- does this witness open this instance?
int lf_lcccs_check(lf_prover *P, const lf_lcccs *acc, const lf_witness *w, uint64_t bound, uint64_t *norm, int *failed,
                   int repr) {
  if (!P || !acc || !w || !failed) return LF_ERR_INVALID_ARG;
  *failed = LF_REL_OK;
  if (!repr_ok(repr)) return bad(P, LF_ERR_INVALID_ARG, "repr");
  const int d = P->d, tau = P->tau, s = P->s, t = P->t;
  if (!lcccs_sizes_ok(P, acc))
    return bad(P, LF_ERR_INCORRECT_LENGTH, "LCCCS sizes (r: s, v: tau, cm: kappa, u: t, x_w: l)");
  if (!witness_ok(w, true, true)) return bad(P, LF_ERR_INVALID_ARG, "missing witness buffer");
  const std::vector<uint64_t> ar = canon(acc->r.elems, (size_t)s * d, repr),
                              av = canon(acc->v.elems, (size_t)tau * d, repr),
                              acm = canon(acc->cm.elems, P->kappa * d, repr),
                              au = canon(acc->u.elems, (size_t)t * d, repr),
                              axw = canon(acc->x_w.elems, P->l * d, repr), ah = canon(acc->h, d, repr);
  lf_ctx *C = P->ctx;
  DevGuard dg(P->device);
  Run R{P, nullptr, (hipStream_t)lf_ctx_get_stream(C)};
  if (witness_checks(P, R, w, acm.data(), bound, norm, failed)) return R.rc;
  if (*failed) return LF_ERR_VERIFICATION;
  // v = f_hat(r) and u_j = MLE(M_j z)(r) (compute_u, linearization/utils.rs:24-29)
  std::vector<uint64_t> got((size_t)std::max(tau, t) * d);
  R.h2d(P->pt, ar.data(), (size_t)s * d);
  R.check(lf_dev_fhat_evaluate(C, d, w->f_coeff, P->N, 0, 1, s, P->pt, P->val), "v");
  R.d2h(got.data(), P->val, (size_t)tau * d);
  if (R.rc) return R.rc;
  if (memcmp(got.data(), av.data(), (size_t)tau * d * 8)) return *failed = LF_REL_V, LF_ERR_VERIFICATION;
  assemble_z(P, R, axw.data(), ah.data(), w);
  R.check(lf_dev_mz_evaluate(C, P->ccs, P->z, 1, s, P->pt, P->us), "u");
  R.d2h(got.data(), P->us, (size_t)t * d);
  if (R.rc) return R.rc;
  if (memcmp(got.data(), au.data(), (size_t)t * d * 8)) return *failed = LF_REL_U, LF_ERR_VERIFICATION;
  return LF_OK;
}

int lf_cccs_check(lf_prover *P, const uint64_t *cm, const uint64_t *x_ccs, const lf_witness *w, uint64_t bound,
                  uint64_t *norm, int *failed, int64_t *row, int repr) {
  if (!P || !cm || (!x_ccs && P->l) || !w || !failed) return LF_ERR_INVALID_ARG;
  *failed = LF_REL_OK;
  if (row) *row = -1;
  if (!repr_ok(repr)) return bad(P, LF_ERR_INVALID_ARG, "repr");
  if (!witness_ok(w, true, true)) return bad(P, LF_ERR_INVALID_ARG, "missing witness buffer");
  const std::vector<uint64_t> cmv = canon(cm, P->kappa * P->d, repr), xc = canon(x_ccs, P->l * P->d, repr);
  lf_ctx *C = P->ctx;
  DevGuard dg(P->device);
  Run R{P, nullptr, (hipStream_t)lf_ctx_get_stream(C)};
  if (witness_checks(P, R, w, cmv.data(), bound, norm, failed)) return R.rc;
  if (*failed) return LF_ERR_VERIFICATION;
  // CCS::check_relation of z = x_ccs || 1 || w_ccs (arith.rs:78-105)
  assemble_z(P, R, xc.data(), P->one.data(), w);
  if (R.rc) return R.rc;
  int64_t fb = -1;
  const int rc = lf_dev_ccs_check_relation(C, P->ccs, P->z, 1, nullptr, &fb);
  if (rc == LF_ERR_NOT_SATISFIED) {
    if (row) *row = fb;
    return *failed = LF_REL_CCS, LF_ERR_VERIFICATION;
  }
  return R.check(rc, "CCS relation");
}

}  // extern "C"
