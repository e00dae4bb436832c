// serialize.cpp -- the wire format of the folding proof and the accumulator
// (SURVEY.md 8(f) rank 4): ark-serialize 0.5 CanonicalSerialize, as derived on
// the reference's types. For these types compressed and uncompressed are the
// same bytes:
//   Fq        8 bytes little-endian of the canonical value (ark-ff into_bigint)
//   Fq3       c0, c1, c2
//   RqNTT     its slot values in order, no length ([C::BaseCRTField; D],
//             stark-rings cyclotomic_ring/ntt_form.rs:24-27)
//   Vec<T>    u64 little-endian length, then the items
//   Commitment { val: Vec<R> }            (commitment/homomorphic_commitment.rs:7-9)
//   sumcheck::Proof(Vec<ProverMsg>), ProverMsg { evaluations: Vec<R> }
//   LFProof { linearization_proof, decomposition_proof_l, decomposition_proof_r,
//             folding_proof }             (latticefold/src/nifs.rs:28-34)
//   LCCCS has no CanonicalSerialize in the reference; its fields are written in
//   declaration order the same way (arith.rs:192-206), which is what the
//   rank-to-rank and host-to-device accumulator interchange uses.
// Host code only: these are byte layouts, no device work.
#include <cstring>
#include <vector>

#include "../../include/lf.h"
#include "gl.hpp"

namespace {

struct Writer {
  uint8_t *out;
  size_t cap, pos = 0;
  int repr;
  bool overflow = false;
  void bytes(const void *p, size_t n) {
    if (out && pos + n <= cap) memcpy(out + pos, p, n);
    if (out && pos + n > cap) overflow = true;
    pos += n;
  }
  void u64(uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i));
    bytes(b, 8);
  }
  void fq(uint64_t v) { u64(repr == LF_REPR_MONTGOMERY ? gl::from_mont(v) : gl::canon(v)); }
  void ring_vec(const lf_ring_slice &s, int d) {
    u64(s.n);
    if (s.n && s.elems)
      for (size_t i = 0; i < s.n * (size_t)d; i++) fq(s.elems[i]);
  }
  void ring_vecvec(const lf_ring_slice *v, size_t n, int d) {
    u64(n);
    for (size_t i = 0; i < n; i++) ring_vec(v[i], d);
  }
  void commitments(const lf_ring_slice *v, size_t n, int d) { ring_vecvec(v, n, d); }
  void sumcheck(const uint64_t *msgs, size_t rounds, size_t evals, int d) {
    u64(rounds);
    for (size_t r = 0; r < rounds; r++) ring_vec({msgs + r * evals * d, evals}, d);
  }
};

struct Reader {
  const uint8_t *in;
  size_t len, pos = 0;
  int repr;
  bool bad = false;
  uint64_t u64() {
    if (pos + 8 > len) {
      bad = true;
      return 0;
    }
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)in[pos + i] << (8 * i);
    pos += 8;
    return v;
  }
  uint64_t fq() {
    const uint64_t v = u64();
    if (v >= gl::P) bad = true;  // ark's deserialize_with_flags rejects non-canonical values
    return repr == LF_REPR_MONTGOMERY ? gl::to_mont(v) : v;
  }
};

}  // namespace

extern "C" {

int lf_lcccs_serialize(const lf_lcccs *a, int repr, uint8_t *out, size_t cap, size_t *len) {
  if (!a || !len || a->d < 1 || !a->h || (repr != LF_REPR_CANONICAL && repr != LF_REPR_MONTGOMERY))
    return LF_ERR_INVALID_ARG;
  Writer w{out, cap, 0, repr};
  w.ring_vec(a->r, a->d);
  w.ring_vec(a->v, a->d);
  w.ring_vec(a->cm, a->d);  // Commitment { val }
  w.ring_vec(a->u, a->d);
  w.ring_vec(a->x_w, a->d);
  for (int i = 0; i < a->d; i++) w.fq(a->h[i]);
  *len = w.pos;
  return w.overflow ? LF_ERR_INCORRECT_LENGTH : LF_OK;
}

int lf_lcccs_deserialize(const uint8_t *in, size_t len, int d, int repr, uint64_t *buf, size_t buf_elems,
                         lf_lcccs *out) {
  if (!in || !out || d < 1 || (repr != LF_REPR_CANONICAL && repr != LF_REPR_MONTGOMERY)) return LF_ERR_INVALID_ARG;
  Reader r{in, len, 0, repr};
  size_t used = 0;
  lf_ring_slice *fields[5] = {&out->r, &out->v, &out->cm, &out->u, &out->x_w};
  out->d = d;
  for (lf_ring_slice *f : fields) {
    const uint64_t n = r.u64();
    if (r.bad || n > (len - r.pos) / (8 * (size_t)d) || used + n * d > buf_elems) return LF_ERR_INCORRECT_LENGTH;
    f->elems = buf + used;
    f->n = n;
    for (size_t i = 0; i < n * (size_t)d; i++) buf[used + i] = r.fq();
    used += n * d;
  }
  if (used + d > buf_elems) return LF_ERR_INCORRECT_LENGTH;
  for (int i = 0; i < d; i++) buf[used + i] = r.fq();
  out->h = buf + used;
  if (r.bad || r.pos != len) return LF_ERR_INCORRECT_LENGTH;
  return LF_OK;
}

int lf_lfproof_serialize(const lf_lfproof *p, int repr, uint8_t *out, size_t cap, size_t *len) {
  if (!p || !len || p->d < 1 || (repr != LF_REPR_CANONICAL && repr != LF_REPR_MONTGOMERY)) return LF_ERR_INVALID_ARG;
  const int d = p->d;
  Writer w{out, cap, 0, repr};
  // LinearizationProof { linearization_sumcheck, v, u } (linearization/structs.rs:15-38)
  w.sumcheck(p->lin_sumcheck, p->lin_rounds, p->lin_evals, d);
  w.ring_vec(p->lin_v, d);
  w.ring_vec(p->lin_u, d);
  // DecompositionProof { u_s, v_s, x_s, y_s } x 2 (decomposition/structs.rs:19-48)
  for (int s = 0; s < 2; s++) {
    w.ring_vecvec(p->dec[s].u_s, p->dec[s].n_u, d);
    w.ring_vecvec(p->dec[s].v_s, p->dec[s].n_v, d);
    w.ring_vecvec(p->dec[s].x_s, p->dec[s].n_x, d);
    w.commitments(p->dec[s].y_s, p->dec[s].n_y, d);
  }
  // FoldingProof { pointshift_sumcheck_proof, theta_s, eta_s } (folding/structs.rs:17-40)
  w.sumcheck(p->fold_sumcheck, p->fold_rounds, p->fold_evals, d);
  w.ring_vecvec(p->theta_s, p->n_theta, d);
  w.ring_vecvec(p->eta_s, p->n_eta, d);
  *len = w.pos;
  return w.overflow ? LF_ERR_INCORRECT_LENGTH : LF_OK;
}

size_t lf_lfproof_shape(const lf_ccs_desc *ccs, const lf_params *pr, size_t kappa, size_t counts[14]) {
  if (!ccs || !pr || !counts) return 0;
  const int d = pr->d;
  const size_t m = ccs->m, B = (size_t)1 << 32;  // every factor below 2^32 and s <= 63: no product wraps
  if (d != 24 && (d < 16 || d > 4096 || (d & (d - 1)))) return 0;
  if (ccs->t < 1 || ccs->degree < 1 || pr->K < 1 || pr->b_small < 1 || pr->b_small >= B / 4 || !m || (m & (m - 1)) ||
      ccs->l >= B / 2 || !kappa || kappa >= B)
    return 0;
  size_t s = 0;
  while (((size_t)1 << s) < m) s++;
  const size_t tau = d == 24 ? 3 : 1, t = ccs->t, K = pr->K, L1 = ccs->l + 1;
  const size_t c[14] = {s * ((size_t)ccs->degree + 2), tau, t, K * t, K * t, K * tau, K * tau, K * L1, K * L1,
                        K * kappa, K * kappa, s * (2 * (size_t)pr->b_small + 1), 2 * K * tau, 2 * K * t};
  size_t sum = 0;
  for (int i = 0; i < 14; i++) {
    if (c[i] > SIZE_MAX / 8 / 4096 / 16) return 0;
    counts[i] = c[i];
    sum += c[i];
  }
  return sum;
}

int lf_lfproof_deserialize(const uint8_t *in, size_t len, const lf_ccs_desc *ccs, const lf_params *pr, size_t kappa,
                           int repr, uint64_t *buf, size_t buf_elems, lf_lfproof_mut *out) {
  if (!in || !ccs || !pr || !buf || !out || (repr != LF_REPR_CANONICAL && repr != LF_REPR_MONTGOMERY))
    return LF_ERR_INVALID_ARG;
  size_t n[14];
  const size_t total = lf_lfproof_shape(ccs, pr, kappa, n);
  if (!total) return LF_ERR_INVALID_ARG;
  const size_t d = pr->d, K = pr->K, tau = n[1], t = n[2], L1 = n[7] / K;
  if (buf_elems / d < total) return LF_ERR_INCORRECT_LENGTH;
  // the shape fixes the byte count too: the words, and one u64 per Vec (the two sumchecks'
  // 1 + s each, lin_v, lin_u, four Vec<Vec> of K a side, theta_s and eta_s of 2K)
  const size_t s = n[11] / (2 * (size_t)pr->b_small + 1), nvec = 2 * (1 + s) + 2 + 8 * (1 + K) + 2 * (1 + 2 * K);
  if (len != 8 * (total * d + nvec)) return LF_ERR_INCORRECT_LENGTH;
  uint64_t *at[14];  // where each lf_lfproof_mut pointer's elements go, in the struct's order
  for (size_t i = 0, off = 0; i < 14; off += n[i++] * d) at[i] = buf + off;
  Reader r{in, len, 0, repr};
  // every length the bytes carry is compared with the shape's before anything is read by
  // it, so the writes below stay inside the `total` elements checked above
  auto vec = [&](uint64_t *dst, size_t elems) {  // Vec<R> of exactly `elems` ring elements
    if (r.u64() != elems || r.bad) return false;
    if ((len - r.pos) / 8 / d < elems) return false;
    for (size_t i = 0; i < elems * d; i++) dst[i] = r.fq();
    return !r.bad;
  };
  auto vecvec = [&](uint64_t *dst, size_t outer, size_t inner) {  // Vec<Vec<R>>, [outer][inner]
    if (r.u64() != outer || r.bad) return false;
    for (size_t i = 0; i < outer; i++)
      if (!vec(dst + i * inner * d, inner)) return false;
    return true;
  };
  bool ok = vecvec(at[0], s, (size_t)ccs->degree + 2) && vec(at[1], tau) && vec(at[2], t);
  for (int side = 0; side < 2 && ok; side++)
    ok = vecvec(at[3 + side], K, t) && vecvec(at[5 + side], K, tau) && vecvec(at[7 + side], K, L1) &&
         vecvec(at[9 + side], K, kappa);
  ok = ok && vecvec(at[11], s, 2 * (size_t)pr->b_small + 1) && vecvec(at[12], 2 * K, tau) && vecvec(at[13], 2 * K, t);
  if (!ok || r.pos != len) return LF_ERR_INCORRECT_LENGTH;
  out->lin_sumcheck = at[0];
  out->lin_v = at[1];
  out->lin_u = at[2];
  for (int side = 0; side < 2; side++) {
    out->u_s[side] = at[3 + side];
    out->v_s[side] = at[5 + side];
    out->x_s[side] = at[7 + side];
    out->y_s[side] = at[9 + side];
  }
  out->fold_sumcheck = at[11];
  out->theta_s = at[12];
  out->eta_s = at[13];
  return LF_OK;
}

}  // extern "C"
