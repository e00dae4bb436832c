// api_sumcheck.hip -- the multilinear sumcheck behind include/lf.h: the MLE and
// round wrappers, and the provers, which share one Fiat-Shamir round loop
// (sumcheck_rounds) so the transcript order that makes the proof bytes equal
// the reference's exists once.
#include <algorithm>

#include "api_internal.hpp"

namespace {

int comb_check(lf_ctx *c, const lf_comb *cb, int nm, int d, int degree, lfk::CombS *cs) {
  if (!cb) return fail(c, LF_ERR_INVALID_ARG, "null combination");
  if (cb->kind == LF_COMB_FOLDING) {
    if (!cb->mu || cb->nk < 1 || cb->tau < 1 || cb->bsmall < 1 || cb->bsmall > 4 || nm != 5 + cb->nk * cb->tau ||
        (degree >= 0 && degree != 2 * cb->bsmall))
      return fail(c, LF_ERR_INVALID_ARG, "folding sumcheck: 5 + nk tau MLEs, degree 2 B_SMALL, B_SMALL <= 4");
    return LF_OK;
  }
  if (cb->kind != LF_COMB_LINEARIZATION || !cb->c || !cb->S_off || !cb->S_idx || cb->q < 1 ||
      cb->q > lfk::LF_MAX_MULTISETS || degree < 1 || degree > 9)
    return fail(c, LF_ERR_INVALID_ARG, "linearization sumcheck: 1 <= q <= 64 multisets, degree <= 9");
  cs->q = cb->q;
  for (int i = 0; i <= cb->q; i++) cs->off[i] = cb->S_off[i];
  if (cs->off[0] != 0 || cs->off[cb->q] > lfk::LF_MAX_S)
    return fail(c, LF_ERR_INVALID_ARG, "linearization sumcheck: at most 512 multiset entries");
  for (int i = 0; i < cs->off[cb->q]; i++) {
    if (cb->S_idx[i] < 0 || cb->S_idx[i] >= nm - 1) return fail(c, LF_ERR_INVALID_ARG, "multiset index out of range");
    cs->idx[i] = (short)cb->S_idx[i];
  }
  return LF_OK;
}
// the *_planes entries: pr names a packed form (lf_fold_step_planes_len) of a supported ring
int planes_check(lf_ctx *c, const lf_params *pr) {
  if (!pr) return fail(c, LF_ERR_INVALID_ARG, "null params");
  if (!lf_fold_step_planes_len(pr, 1))
    return fail(c, LF_ERR_UNSUPPORTED_RING, "packed planes: d = 24, 16 .. 512, 1024 or 4096, b_small = 2, K <= 15");
  int lb, lbs;
  return check_params(c, pr, lb, lbs);
}
int comb_degree(const lf_comb *cb, int degree) { return cb->kind == LF_COMB_FOLDING ? 2 * cb->bsmall : degree; }

// one round as its message producer sees it: the MLEs with i variables fixed
struct Round {
  int i;
  size_t half;                   // 2^(nv-i-1): the points the next round sums over
  const uint64_t *cur;           // the MLEs, `stride` apart, or (round 0 of the pointer-table provers)
  const uint64_t *const *cptrs;  // a device array of nm pointers
  size_t stride;
};

// MLSumcheck::prove_as_subprotocol (sumcheck.rs:61-88): the Fiat-Shamir loop of every
// prover here, so the transcript order exists once. Round 0 reads the MLEs at `mles`
// (stride 2^nv d) or, with ptrs, wherever those point; every round fixes them into
// the next buffer, `buf` (2^(nv-1) points) and `alt` (2^(nv-2) points) in turn, and
// `evals` (optional) receives them at the whole challenge point.
//   message(round, msg): the round's nev = degree + 1 evaluations into msg (host)
//   fixed(round, ch, dst): after the challenge ch, and the launch that fixed the
//     first nm0 (round 0) / nm MLEs into dst (null in the last round)
template <class Message, class Fixed>
int sumcheck_rounds(lf_ctx *c, lf_transcript *t, const uint64_t *mles, const uint64_t *const *ptrs, uint64_t *buf,
                    uint64_t *alt, int nm, int nm0, int nv, int d, int degree, uint64_t *proof, uint64_t *randomness,
                    uint64_t *evals, Message message, Fixed fixed) {
  const int tb = lfk::slot_words(d), nev = degree + 1;
  absorb_scalar(t, (uint64_t)nv, d);  // R::from(nvars), R::from(degree)
  absorb_scalar(t, (uint64_t)degree, d);
  std::vector<uint64_t> scal(d);
  Round r{0, 0, mles, ptrs, (size_t)d << nv};
  for (; r.i < nv; r.i++) {
    r.half = (size_t)1 << (nv - r.i - 1);
    uint64_t *msg = proof + (size_t)r.i * nev * d, *ch = randomness + (size_t)r.i * tb;
    LF_TRY(message(r, msg));
    // prover message absorbed, challenge sampled (one sample for Fq) and absorbed
    lf_transcript_absorb_ring(t, msg, (size_t)nev, d, LF_REPR_CANONICAL);
    sample_challenge(t, tb, ch);
    for (int k = 0; k < d; k++) scal[k] = ch[k % tb];
    lf_transcript_absorb_ring(t, scal.data(), 1, d, LF_REPR_CANONICAL);
    // fix_variables(r) of every MLE (prover.rs:75-78), into the other buffer
    const bool last = r.i + 1 == nv;
    uint64_t *dst = last ? nullptr : r.i % 2 == 0 ? buf : alt;
    if (last && evals)  // the prover's final values
      LF_HIP(c, lfk::mle_fix_first(r.cur, r.stride, nm, r.half, d, ch, evals, d, c->cur, r.cptrs));
    if (dst)
      LF_HIP(c, lfk::mle_fix_first(r.cur, r.stride, r.i ? nm : nm0, r.half, d, ch, dst, r.half * d, c->cur, r.cptrs));
    LF_TRY(fixed(r, ch, dst));
    if (dst) r.cur = dst, r.cptrs = nullptr, r.stride = r.half * d;
  }
  return LF_OK;
}

// the folding polynomial's f_hat MLEs as digit coefficient rows (lf_sumcheck_prove_fold_digits)
struct DigitFhat {
  const uint64_t *fc0, *fc1;
  int K;
  size_t N, wstride;
  bool planes = false;  // fc0, fc1 are the sides' packed digit planes (lf_sumcheck_prove_fold_planes)
};
// Folding or (unsplit) linearization rounds: every message is one launch's round sums.
// The fixed MLEs go to the context scratch and `alt` (the input itself when ptrs is null)
int sumcheck_run(lf_ctx *c, lf_transcript *t, const lf_comb *cb, const lfk::CombS &cs, const uint64_t *mles,
                 const uint64_t *const *ptrs, uint64_t *alt, int nm, int nv, int d, int degree, uint64_t *proof,
                 uint64_t *randomness, const DigitFhat *dg = nullptr) {
  const int nev = degree + 1;
  const size_t n = (size_t)1 << nv;
  // scratch: the MLEs fixed by the first challenge, the round's partial sums, the
  // evaluations, the weights; the partial sums of every round fit the largest
  // round's (chunks only split the small ones)
  const int nfc = cb->kind == LF_COMB_FOLDING ? cb->nk * cb->tau : cb->q;  // the chunked sum (f_hat MLEs / multisets)
  size_t part = 0;
  for (size_t h = n / 2; h >= 1; h /= 2) part = std::max(part, lfk::round_partial_elems(d, h, nev, nfc));
  const size_t fixed = (size_t)nm * (n / 2) * d;
  const size_t wlen = cb->kind == LF_COMB_FOLDING ? (size_t)cb->nk * cb->tau * d : 0;
  LF_TRY(grow(c, c->sc, c->sc_elems, fixed + part + (size_t)nev * d + wlen));
  uint64_t *buf = c->sc, *partial = buf + fixed, *ev = partial + part, *w = ev + (size_t)nev * d;
  if (wlen) LF_HIP(c, lfk::fold_weights(cb->mu, cb->nk, cb->tau, d, w, c->cur));
  auto message = [&](const Round &r, uint64_t *msg) {
    if (dg && r.i == 0 && dg->planes)  // round 0 straight from the planes
      LF_HIP(c, lfk::round_folding0_planes(r.cur, r.stride, d, dg->K, dg->fc0, dg->fc1, dg->N, w, r.half, partial, ev,
                                           c->cur));
    else if (dg && r.i == 0)  // round 0 straight from the digits (cur: the 5 general MLEs)
      LF_HIP(c, lfk::round_folding0_digits(r.cur, r.stride, dg->fc0, dg->fc1, dg->K, dg->N, dg->wstride,
                                           cb->nk * cb->tau, w, r.half, d, partial, ev, c->cur));
    else if (cb->kind == LF_COMB_FOLDING)
      LF_HIP(c, lfk::round_folding(r.cur, r.stride, cb->nk * cb->tau, w, cb->bsmall, r.half, d, partial, ev, c->cur));
    else
      LF_HIP(c, lfk::round_lin(r.cur, r.stride, nm, cb->c, cs, degree, r.half, d, partial, ev, c->cur, r.cptrs));
    return download_msg(c, msg, ev, (size_t)nev * d);
  };
  auto fixed_digits = [&](const Round &r, const uint64_t *ch, uint64_t *dst) {
    if (dg && r.i == 0 && dst && dg->planes)
      LF_HIP(c, lfk::fix_fhat_planes(d, dg->K, dg->fc0, dg->fc1, dg->N, r.half, ch, dst + 5 * r.half * d, r.half * d,
                                     c->cur));
    else if (dg && r.i == 0 && dst)  // after the 5 general MLEs, the f_hat ones from the digits
      LF_HIP(c, lfk::fix_fhat_digits(dg->fc0, dg->fc1, dg->K, dg->N, dg->wstride, nm - 5, r.half, d, ch,
                                     dst + 5 * r.half * d, r.half * d, c->cur));
    return (int)LF_OK;
  };
  return sumcheck_rounds(c, t, mles, ptrs, buf, alt, nm, dg ? 5 : nm, nv, d, degree, proof, randomness, nullptr,
                         message, fixed_digits);
}

// The linearization sumcheck over [mles..., eq(beta)] with eq(beta) split off
// (lfk::round_lin_eq): round i sums q_i(e) = sum_b E_i[b] inner(e, b) for e < degree
// on the device, E_i = eq(beta_(i+1) ..) over the unbound variables (E_0 an eq table,
// then pair sums); the host extrapolates q_i(degree) (q_i has degree < degree:
// q(n) = sum_(k<n) (-1)^(n-1-k) C(n, k) q(k)) and forms the message
//   p_i(e) = P_i eq(beta_i, e) q_i(e),  P_i = prod_(k<i) eq(beta_k, r_k),
// the same field elements as the unsplit round sums, so the transcript is the same.
int sumcheck_run_lin(lf_ctx *c, lf_transcript *t, const lf_comb *cb, const lfk::CombS &cs,
                     const uint64_t *const *ptrs, uint64_t *alt, int nm, int nv, int d, int degree,
                     const uint64_t *beta, uint64_t *proof, uint64_t *randomness, uint64_t *evals,
                     const uint32_t *act = nullptr, const uint32_t *act_off = nullptr) {
  const int tb = lfk::slot_words(d), nev = degree + 1, nq = degree, ns = d / tb;
  const size_t n = (size_t)1 << nv;
  size_t part = 0;
  for (size_t h = n / 2; h >= 1; h /= 2) part = std::max(part, lfk::round_partial_elems(d, h, nq, cb->q));
  // sparse round 0: block g runs multiset bms[g] over act[boff[g] .. bend[g])
  std::vector<uint32_t> blk;  // bms | boff | bend
  int nblk = 0;
  if (act) {
    const uint32_t per = (uint32_t)lfk::round_lin_sparse_block_points(d);
    std::vector<uint32_t> bms, bo, be;
    for (int i = 0; i < cs.q; i++)
      for (uint32_t p = act_off[i]; p < act_off[i + 1]; p += per) {
        bms.push_back((uint32_t)i);
        bo.push_back(p);
        be.push_back(std::min(p + per, act_off[i + 1]));
      }
    nblk = (int)bms.size();
    blk = bms;
    blk.insert(blk.end(), bo.begin(), bo.end());
    blk.insert(blk.end(), be.begin(), be.end());
    part = std::max(part, (size_t)nblk * nq * d);
  }
  const size_t fixed = (size_t)nm * (n / 2) * d, blk_elems = (blk.size() + 1) / 2;
  // scratch: fixed MLEs | partial sums | q | E tables (n/2 + n/4 + .. + 1 < n elements) | beta | blocks
  LF_TRY(grow(c, c->sc, c->sc_elems, fixed + part + (size_t)nq * d + n * d + (size_t)nv * d + blk_elems));
  uint64_t *buf = c->sc, *partial = buf + fixed, *qd = partial + part, *Et = qd + (size_t)nq * d,
           *bd = Et + n * d, *bk = bd + (size_t)nv * d;
  LF_HIP(c, hipMemcpyAsync(bd, beta, (size_t)nv * d * 8, hipMemcpyHostToDevice, c->cur));
  if (nblk) {  // through the pinned staging, grown here so no round frees it under the copy
    LF_TRY(pinned(c, std::max(blk_elems, (size_t)nq * d)));
    memcpy(c->hmsg, blk.data(), blk.size() * 4);
    LF_HIP(c, hipMemcpyAsync(bk, c->hmsg, blk.size() * 4, hipMemcpyHostToDevice, c->cur));
  }
  if (nv > 1) {
    LF_HIP(c, lfk::eq_table(bd + d, nv - 1, d, Et, c->cur));
  } else {
    std::vector<uint64_t> one(d, 0);
    for (int k = 0; k < d; k += tb) one[k] = 1;
    LF_HIP(c, hipMemcpyAsync(Et, one.data(), (size_t)d * 8, hipMemcpyHostToDevice, c->cur));
    LF_HIP(c, hipStreamSynchronize(c->cur));
  }
  // (-1)^(nq-1-k) C(nq, k): q(nq) from q(0 .. nq-1)
  std::vector<uint64_t> wext(nq);
  for (int k = 0; k < nq; k++) {
    uint64_t b = 1;
    for (int j = 0; j < k; j++) b = b * (uint64_t)(nq - j) / (uint64_t)(j + 1);
    wext[k] = (nq - 1 - k) % 2 ? gl::neg(b % gl::P) : b % gl::P;
  }
  // eq(beta, x) = (1 - beta) + x (2 beta - 1) for a base-ring x
  auto eqv = [tb](const uint64_t *be, const uint64_t *x, uint64_t *o) {
    uint64_t a[3] = {0, 0, 0}, s[3] = {0, 0, 0};
    for (int w = 0; w < tb; w++) {
      a[w] = gl::neg(be[w]);
      s[w] = gl::add(be[w], be[w]);
    }
    a[0] = gl::add(a[0], 1);
    s[0] = gl::sub(s[0], 1);
    uint64_t m[3];
    gl::base_mul(s, x, m, tb);
    for (int w = 0; w < tb; w++) o[w] = gl::add(a[w], m[w]);
  };
  std::vector<uint64_t> qh((size_t)nq * d);
  uint64_t pfx[3] = {1, 0, 0};
  uint64_t *E = Et;
  auto message = [&](const Round &r, uint64_t *msg) {
    if (r.i == 0 && act) {
      if (nblk) {
        const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bk);
        LF_HIP(c, lfk::round_lin_eq_sparse(r.cptrs, E, cb->c, cs, degree, act, reinterpret_cast<const int *>(b32),
                                           b32 + nblk, b32 + 2 * nblk, nblk, d, partial, qd, c->cur));
      } else {
        LF_HIP(c, hipMemsetAsync(qd, 0, (size_t)nq * d * 8, c->cur));
      }
    } else {
      LF_HIP(c, lfk::round_lin_eq(r.cur, r.stride, E, cb->c, cs, degree, r.half, d, partial, qd, c->cur, r.cptrs));
    }
    LF_TRY(download_msg(c, qh.data(), qd, (size_t)nq * d));
    const uint64_t *be = beta + (size_t)r.i * d;  // slot 0 holds the base-ring value
    for (int e = 0; e < nev; e++) {
      uint64_t x[3] = {(uint64_t)e, 0, 0}, ev[3], f[3];
      eqv(be, x, ev);
      gl::base_mul(pfx, ev, f, tb);
      for (int s = 0; s < ns; s++) {
        uint64_t qv[3] = {0, 0, 0};
        if (e < nq) {
          for (int w = 0; w < tb; w++) qv[w] = qh[(size_t)e * d + s * tb + w];
        } else {
          for (int k = 0; k < nq; k++)
            for (int w = 0; w < tb; w++) qv[w] = gl::add(qv[w], gl::mul(wext[k], qh[(size_t)k * d + s * tb + w]));
        }
        gl::base_mul(f, qv, msg + (size_t)e * d + s * tb, tb);
      }
    }
    return (int)LF_OK;
  };
  auto bound = [&](const Round &r, const uint64_t *ch, uint64_t *dst) {
    uint64_t ev[3], np[3];
    eqv(beta + (size_t)r.i * d, ch, ev);
    gl::base_mul(pfx, ev, np, tb);
    for (int w = 0; w < tb; w++) pfx[w] = np[w];
    if (dst) {
      LF_HIP(c, lfk::pair_sum(E, r.half / 2, d, E + r.half * d, c->cur));
      E += r.half * d;
    }
    return (int)LF_OK;
  };
  return sumcheck_rounds(c, t, nullptr, ptrs, buf, alt, nm, nm, nv, d, degree, proof, randomness, evals, message,
                         bound);
}

// the MLE pointer table of the `ptrs`, `lin` and `lin_sparse` provers on the device
// (behind the scratch the rounds use); a null entry is an error
int upload_ptrs(lf_ctx *c, const uint64_t *const *mles, int nm) {
  for (int m = 0; m < nm; m++)
    if (!mles[m]) return fail(c, LF_ERR_INVALID_ARG, "null MLE pointer");
  LF_TRY(grow(c, c->ptrs, c->ptrs_elems, (size_t)nm));
  LF_HIP(c, hipMemcpyAsync(c->ptrs, mles, (size_t)nm * sizeof(uint64_t), hipMemcpyHostToDevice, c->cur));
  return LF_OK;
}
// the split-eq rounds sum at most degree - 1 factors beside eq(beta)
int lin_multiset_check(lf_ctx *c, const lfk::CombS &cs, int i, int degree) {
  if (cs.off[i + 1] - cs.off[i] > degree - 1)
    return fail(c, LF_ERR_INVALID_ARG, "linearization sumcheck: a multiset of degree or more factors");
  return LF_OK;
}

}  // namespace

extern "C" {

int lf_dev_eq_table(lf_ctx *c, int d, const uint64_t *r, int nv, uint64_t *out) {
  if (!c || !r || !out || nv < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  LF_HIP(c, lfk::eq_table(r, nv, d, out, c->cur));
  return LF_OK;
}

int lf_dev_get_fhat(lf_ctx *c, int d, const uint64_t *f_coeff, size_t N, int nv, uint64_t *out) {
  if (!c || !out || (N && !f_coeff) || nv < 0 || nv > 40) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  if (N > ((size_t)1 << nv)) return fail(c, LF_ERR_INCORRECT_LENGTH, "N exceeds 2^nv");
  LF_HIP(c, lfk::get_fhat(f_coeff, N, d, nv, out, c->cur));
  return LF_OK;
}

int lf_dev_fhat_evaluate(lf_ctx *c, int d, const uint64_t *f_coeff, size_t N, size_t wstride, int nw, int nv,
                         const uint64_t *point, uint64_t *out) {
  if (!c || !point || !out || nw < 0 || nv < 1 || (nw && N && !f_coeff)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  const size_t n = (size_t)1 << nv;
  if (N > n) return fail(c, LF_ERR_INCORRECT_LENGTH, "N exceeds 2^nv");
  const int tau = d == 24 ? 3 : 1;
  LF_TRY(grow(c, c->sc, c->sc_elems, n * d + lfk::mle_eval_partial_elems(d, nw * tau)));
  LF_HIP(c, lfk::eq_table(point, nv, d, c->sc, c->cur));
  LF_HIP(c, lfk::fhat_dot(f_coeff, N, wstride ? wstride : N * d, nw, c->sc, n, d, c->sc + n * d, out, c->cur));
  return LF_OK;
}

int lf_dev_fhat_evaluate_eq(lf_ctx *c, int d, const uint64_t *f_coeff, size_t N, size_t wstride, int nw, int nv,
                            const uint64_t *eq, uint64_t *out) {
  if (!c || !eq || !out || nw < 0 || nv < 1 || (nw && N && !f_coeff)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  const size_t n = (size_t)1 << nv;
  if (N > n) return fail(c, LF_ERR_INCORRECT_LENGTH, "N exceeds 2^nv");
  const int tau = d == 24 ? 3 : 1;
  LF_TRY(grow(c, c->sc, c->sc_elems, lfk::mle_eval_partial_elems(d, nw * tau)));
  LF_HIP(c, lfk::fhat_dot(f_coeff, N, wstride ? wstride : N * d, nw, eq, n, d, c->sc, out, c->cur));
  return LF_OK;
}

int lf_dev_mle_lincomb(lf_ctx *c, int d, const uint64_t *mles, size_t stride, int nm, int nv, const uint64_t *coef,
                       uint64_t *io) {
  if (!c || !io || nm < 0 || nv < 0 || (nm && (!mles || !coef))) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  const size_t n = (size_t)1 << nv;
  LF_HIP(c, lfk::mle_lincomb(mles, stride ? stride : n * d, nm, coef, n, d, io, c->cur));
  return LF_OK;
}

int lf_dev_fhat_lincomb_digits(lf_ctx *c, int d, const uint64_t *f_coeff, size_t N, size_t wstride, int nw, int nv,
                               const uint64_t *coef, uint64_t *io) {
  if (!c || !io || nw < 0 || nv < 0 || nv > 40 || (nw && (!coef || (N && !f_coeff)))) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  if (N > ((size_t)1 << nv)) return fail(c, LF_ERR_INCORRECT_LENGTH, "N exceeds 2^nv");
  if (!nw) return LF_OK;
  LF_HIP(c, lfk::fhat_lincomb_digits(f_coeff, nw, N, wstride ? wstride : N * d, coef, nv, d, io, c->cur));
  return LF_OK;
}

int lf_dev_fhat_evaluate_planes(lf_ctx *c, const lf_params *pr, const uint64_t *planes, size_t N, int nv,
                                const uint64_t *eq, uint64_t *out) {
  if (!c || !pr || !eq || !out || nv < 1 || nv > 40 || (N && !planes)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(planes_check(c, pr));
  const size_t n = (size_t)1 << nv;
  if (N > n) return fail(c, LF_ERR_INVALID_ARG, "N exceeds 2^nv");
  const int d = pr->d, nm = pr->K * (d == 24 ? 3 : 1);
  LF_TRY(grow(c, c->sc, c->sc_elems, lfk::mle_eval_partial_elems(d, nm)));
  LF_HIP(c, lfk::fhat_dot_planes(d, pr->K, planes, N, eq, n, c->sc, out, c->cur));
  return LF_OK;
}

int lf_dev_fhat_lincomb_planes(lf_ctx *c, const lf_params *pr, const uint64_t *planes, size_t N, int nv,
                               const uint64_t *coef, uint64_t *io) {
  if (!c || !pr || !coef || !io || nv < 0 || nv > 40 || (N && !planes)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(planes_check(c, pr));
  if (N > ((size_t)1 << nv)) return fail(c, LF_ERR_INVALID_ARG, "N exceeds 2^nv");
  LF_HIP(c, lfk::fhat_lincomb_planes(pr->d, pr->K, planes, N, coef, nv, io, c->cur));
  return LF_OK;
}

static_assert(LF_PLAN_FOLDING == lfk::ROUND_FOLDING && LF_PLAN_LIN == lfk::ROUND_LIN &&
                  LF_PLAN_LIN_EQ == lfk::ROUND_LIN_EQ,
              "lf.h's plan kinds are the launchers' round kinds");
int lf_sumcheck_round_plan(int d, size_t half, int nf, int kind, int out[8]) {
  if (!out || !ring_ok(d) || !half || nf < 1 || kind < LF_PLAN_FOLDING || kind > LF_PLAN_LIN_EQ)
    return LF_ERR_INVALID_ARG;
  const lfk::RoundPlan pl = lfk::round_plan(d, half, nf, kind);
  out[0] = pl.spb;
  out[1] = pl.ppb;
  out[2] = (int)pl.gx;
  out[3] = (int)pl.gy;
  out[4] = (int)pl.nchunk;
  out[5] = pl.capped;
  out[6] = pl.per_point;
  out[7] = kind == LF_PLAN_LIN_EQ ? (int)lfk::round_lin_sparse_block_points(d) : 0;
  return LF_OK;
}

int lf_sumcheck_dot_plan(int d, size_t n, int out[4]) {
  if (!out || !ring_ok(d) || !n) return LF_ERR_INVALID_ARG;
  const lfk::DotPlan pl = lfk::dot_plan(d, n);
  out[0] = pl.spb;
  out[1] = pl.ppb;
  out[2] = pl.nsplit;
  out[3] = (int)std::min(pl.passes, (size_t)INT32_MAX);
  return LF_OK;
}

int lf_dev_mle_fix_first(lf_ctx *c, int d, const uint64_t *in, size_t in_stride, int nm, int nv,
                         const uint64_t *r_base, uint64_t *out, size_t out_stride) {
  if (!c || !in || !out || !r_base || nm < 1 || nv < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  LF_HIP(c, lfk::mle_fix_first(in, in_stride, nm, (size_t)1 << (nv - 1), d, r_base, out, out_stride, c->cur));
  return LF_OK;
}

int lf_dev_mle_evaluate_eq(lf_ctx *c, int d, const uint64_t *mles, int nm, int nv, const uint64_t *eq, uint64_t *out) {
  if (!c || !mles || !eq || !out || nm < 1 || nv < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  const size_t n = (size_t)1 << nv;
  LF_TRY(grow(c, c->sc, c->sc_elems, lfk::mle_eval_partial_elems(d, nm)));
  LF_HIP(c, lfk::mle_dot(mles, n * d, nm, eq, n, d, c->sc, out, c->cur));
  return LF_OK;
}

int lf_dev_mle_evaluate(lf_ctx *c, int d, const uint64_t *mles, int nm, int nv, const uint64_t *point, uint64_t *out) {
  if (!c || !mles || !point || !out || nm < 1 || nv < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  const size_t n = (size_t)1 << nv;
  LF_TRY(grow(c, c->sc, c->sc_elems, n * d + lfk::mle_eval_partial_elems(d, nm)));
  LF_HIP(c, lfk::eq_table(point, nv, d, c->sc, c->cur));
  LF_HIP(c, lfk::mle_dot(mles, n * d, nm, c->sc, n, d, c->sc + n * d, out, c->cur));
  return LF_OK;
}

int lf_dev_sumcheck_round(lf_ctx *c, const lf_comb *cb, const uint64_t *mles, size_t stride, int nm, int nv, int d,
                          int degree, uint64_t *evals) {
  if (!c || !mles || !evals || nv < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  lfk::CombS cs;
  LF_TRY(comb_check(c, cb, nm, d, cb && cb->kind == LF_COMB_FOLDING ? -1 : degree, &cs));
  const int deg = comb_degree(cb, degree);
  const size_t half = (size_t)1 << (nv - 1);
  const size_t part = lfk::round_partial_elems(d, half, deg + 1, cb->kind == LF_COMB_FOLDING ? cb->nk * cb->tau : cb->q);
  const size_t wlen = cb->kind == LF_COMB_FOLDING ? (size_t)cb->nk * cb->tau * d : 0;
  LF_TRY(grow(c, c->sc, c->sc_elems, part + wlen));
  if (cb->kind == LF_COMB_FOLDING) {
    uint64_t *w = c->sc + part;
    LF_HIP(c, lfk::fold_weights(cb->mu, cb->nk, cb->tau, d, w, c->cur));
    LF_HIP(c, lfk::round_folding(mles, stride, cb->nk * cb->tau, w, cb->bsmall, half, d, c->sc, evals, c->cur));
  } else {
    LF_HIP(c, lfk::round_lin(mles, stride, nm, cb->c, cs, deg, half, d, c->sc, evals, c->cur));
  }
  return LF_OK;
}

int lf_sumcheck_prove_fold_digits(lf_ctx *c, lf_transcript *t, const lf_comb *cb, const uint64_t *mles5,
                                  const uint64_t *fc0, const uint64_t *fc1, int K, size_t N, size_t wstride, int nv,
                                  int d, uint64_t *work, uint64_t *proof, uint64_t *randomness) {
  if (!c || !t || !cb || !mles5 || !fc0 || !fc1 || !work || !proof || !randomness || nv < 1 || K < 1)
    return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  const int tau = d == 24 ? 3 : 1;
  if (cb->kind != LF_COMB_FOLDING || cb->bsmall != 2 || cb->nk != 2 * K || cb->tau != tau || N > ((size_t)1 << nv))
    return fail(c, LF_ERR_INVALID_ARG, "fold_digits: a folding combination with B_SMALL = 2 over 2K witnesses");
  lfk::CombS cs;
  const int nm = 5 + cb->nk * cb->tau;
  LF_TRY(comb_check(c, cb, nm, d, 4, &cs));
  const DigitFhat dg{fc0, fc1, K, N, wstride};
  return sumcheck_run(c, t, cb, cs, mles5, nullptr, work, nm, nv, d, 4, proof, randomness, &dg);
}

int lf_sumcheck_prove_fold_planes(lf_ctx *c, lf_transcript *t, const lf_comb *cb, const uint64_t *mles5,
                                  const lf_params *pr, const uint64_t *planes0, const uint64_t *planes1, size_t N,
                                  int nv, uint64_t *work, uint64_t *proof, uint64_t *randomness) {
  if (!c || !t || !cb || !mles5 || !pr || !planes0 || !planes1 || !work || !proof || !randomness || nv < 1 || nv > 40)
    return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(planes_check(c, pr));
  const int d = pr->d, K = pr->K, tau = d == 24 ? 3 : 1;
  if (cb->kind != LF_COMB_FOLDING || cb->bsmall != 2 || cb->nk != 2 * K || cb->tau != tau || N > ((size_t)1 << nv))
    return fail(c, LF_ERR_INVALID_ARG, "fold_planes: a folding combination with B_SMALL = 2 over 2K witnesses, N <= 2^nv");
  lfk::CombS cs;
  const int nm = 5 + cb->nk * cb->tau;
  LF_TRY(comb_check(c, cb, nm, d, 4, &cs));
  const DigitFhat dg{planes0, planes1, K, N, 0, true};
  return sumcheck_run(c, t, cb, cs, mles5, nullptr, work, nm, nv, d, 4, proof, randomness, &dg);
}

int lf_sumcheck_prove(lf_ctx *c, lf_transcript *t, const lf_comb *cb, uint64_t *mles, int nm, int nv, int d,
                      int degree, uint64_t *proof, uint64_t *randomness) {
  if (!c || !t || !mles || !proof || !randomness || nv < 1 || nm < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  lfk::CombS cs;
  LF_TRY(comb_check(c, cb, nm, d, degree, &cs));
  return sumcheck_run(c, t, cb, cs, mles, nullptr, mles, nm, nv, d, degree, proof, randomness);
}

int lf_sumcheck_prove_ptrs(lf_ctx *c, lf_transcript *t, const lf_comb *cb, const uint64_t *const *mles, int nm, int nv,
                           int d, int degree, uint64_t *work, uint64_t *proof, uint64_t *randomness) {
  if (!c || !t || !mles || !work || !proof || !randomness || nv < 1 || nm < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  LF_TRY(upload_ptrs(c, mles, nm));
  lfk::CombS cs;
  LF_TRY(comb_check(c, cb, nm, d, degree, &cs));
  return sumcheck_run(c, t, cb, cs, nullptr, reinterpret_cast<const uint64_t *const *>(c->ptrs), work, nm, nv, d,
                      degree, proof, randomness);
}

int lf_sumcheck_prove_lin(lf_ctx *c, lf_transcript *t, const lf_comb *cb, const uint64_t *const *mles, int nm, int nv,
                          int d, int degree, const uint64_t *beta, uint64_t *work, uint64_t *proof,
                          uint64_t *randomness, uint64_t *evals) {
  if (!c || !t || !mles || !beta || !work || !proof || !randomness || nv < 1 || nm < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  LF_TRY(upload_ptrs(c, mles, nm));
  if (cb && cb->kind != LF_COMB_LINEARIZATION)
    return fail(c, LF_ERR_INVALID_ARG, "lf_sumcheck_prove_lin: a linearization combination");
  lfk::CombS cs;
  LF_TRY(comb_check(c, cb, nm + 1, d, degree, &cs));  // the list with eq(beta) last
  for (int i = 0; i < cs.q; i++) LF_TRY(lin_multiset_check(c, cs, i, degree));
  return sumcheck_run_lin(c, t, cb, cs, reinterpret_cast<const uint64_t *const *>(c->ptrs), work, nm, nv, d, degree,
                          beta, proof, randomness, evals);
}

int lf_sumcheck_prove_lin_sparse(lf_ctx *c, lf_transcript *t, const lf_comb *cb, const uint64_t *const *mles, int nm,
                                 int nv, int d, int degree, const uint64_t *beta, const uint32_t *act,
                                 const uint32_t *act_off, uint64_t *work, uint64_t *proof, uint64_t *randomness,
                                 uint64_t *evals) {
  if (!c || !t || !cb || !mles || !beta || !act || !act_off || !work || !proof || !randomness || nv < 1 || nm < 1)
    return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  LF_TRY(upload_ptrs(c, mles, nm));
  if (cb->kind != LF_COMB_LINEARIZATION)
    return fail(c, LF_ERR_INVALID_ARG, "lf_sumcheck_prove_lin_sparse: a linearization combination");
  lfk::CombS cs;
  LF_TRY(comb_check(c, cb, nm + 1, d, degree, &cs));
  for (int i = 0; i < cs.q; i++) {
    LF_TRY(lin_multiset_check(c, cs, i, degree));
    if (act_off[i + 1] < act_off[i] || act_off[i + 1] - act_off[i] > ((size_t)1 << (nv - 1)))
      return fail(c, LF_ERR_INVALID_ARG, "sparse linearization: act_off must not decrease, at most 2^(nv-1) points each");
  }
  if (act_off[0] != 0) return fail(c, LF_ERR_INVALID_ARG, "sparse linearization: act_off[0] must be 0");
  return sumcheck_run_lin(c, t, cb, cs, reinterpret_cast<const uint64_t *const *>(c->ptrs), work, nm, nv, d, degree,
                          beta, proof, randomness, evals, act, act_off);
}

}  // extern "C"
