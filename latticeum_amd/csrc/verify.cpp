// verify.cpp -- the folding verifier on the host, at every supported ring:
// NIFSVerifier::verify (latticefold/src/nifs.rs:117-162) over the zkvm's
// public-input absorption (zkvm/src/zk_latticefold.rs:162-184), as main.rs:408-426
// runs it after every fold():
//   linearization (nifs/linearization.rs:200-285), the two decompositions
//   (nifs/decomposition.rs:90-155), folding (nifs/folding.rs:133-200 with
//   folding/utils.rs:51-127, 380-421, 456-517).
// One core over (d, tb): a base-ring element is tb words (Fq3 for Phi_72, Fq for
// X^d + 1), a challenge is tb transcript samples and their re-observation, broadcast
// into every slot, and a product of NTT elements is d / tb base-ring products.
// Its cost is the sequential Poseidon2 sponge (transcript.cpp); the ring
// arithmetic beside it is a few million field products, so this is host code and
// needs no device. Nothing here is quadratic in d at the X^d + 1 rings: v_0 goes
// through a host negacyclic transform (Nega).
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/lf.h"
#include "ring.hpp"

namespace {

using Vec = std::vector<uint64_t>;

bool nega_degree(int d) { return d >= 16 && d <= 4096 && !(d & (d - 1)); }

// X^d + 1: slot k = f(psi^(2k+1)), psi = 7^((p-1)/2d), natural order (ring.hpp).
// A psi^j twist, then a radix-2 DFT at omega = psi^2 (bit reversal, then log2 d
// passes of d / 2 butterflies); the inverse runs omega^-1 and untwists by psi^-j / d.
struct Nega {
  int d;
  Vec twist, itwist, root, iroot;  // psi^j, psi^-j / d (j < d); omega^e, omega^-e (e < d / 2)
  explicit Nega(int dd) : d(dd), twist(dd), itwist(dd), root(dd / 2), iroot(dd / 2) {
    const uint64_t psi = gl::pow(7, (gl::P - 1) / (2 * (uint64_t)d)), ipsi = gl::inv(psi);
    uint64_t a = 1, b = gl::inv((uint64_t)d);
    for (int j = 0; j < d; j++) {
      twist[j] = a;
      itwist[j] = b;
      a = gl::mul(a, psi);
      b = gl::mul(b, ipsi);
    }
    const uint64_t w = gl::mul(psi, psi), iw = gl::mul(ipsi, ipsi);
    a = b = 1;
    for (int e = 0; e < d / 2; e++) {
      root[e] = a;
      iroot[e] = b;
      a = gl::mul(a, w);
      b = gl::mul(b, iw);
    }
  }
  void dft(uint64_t *x, const Vec &w) const {
    for (int i = 1, j = 0; i < d; i++) {
      int bit = d >> 1;
      for (; j & bit; bit >>= 1) j ^= bit;
      j ^= bit;
      if (i < j) std::swap(x[i], x[j]);
    }
    for (int len = 2; len <= d; len <<= 1) {
      const int half = len / 2, step = d / len;
      for (int i = 0; i < d; i += len)
        for (int k = 0; k < half; k++) {
          const uint64_t u = x[i + k], v = gl::mul(x[i + k + half], w[(size_t)k * step]);
          x[i + k] = gl::add(u, v);
          x[i + k + half] = gl::sub(u, v);
        }
    }
  }
  void crt(uint64_t *x) const {
    for (int j = 0; j < d; j++) x[j] = gl::mul(x[j], twist[j]);
    dft(x, root);
  }
  void icrt(uint64_t *x) const {
    dft(x, iroot);
    for (int j = 0; j < d; j++) x[j] = gl::mul(x[j], itwist[j]);
  }
};

// RotSum over Phi_72 (X^24 = X^12 - 1, X^36 = -1): coefficient j of X^r a; the host
// twin of fold.hip k_rot_lin
uint64_t rot_coeff(const uint64_t *a, int j, int r) {
  uint64_t v = j >= r ? a[j - r] : 0;
  if (j >= 12 && r > j - 12) v = gl::add(v, a[j + 12 - r]);
  if (j < 12 && r > j) v = gl::sub(v, a[j + 24 - r]);
  if (j < 12 && r > j + 12) v = gl::sub(v, a[j + 36 - r]);
  return v;
}

// rot_lin_combination (cyclotomic-rings rotation.rs:84-101, rot_sum :45-63), canonical
// words: v0 = sum_i RotSum(rho_i, flatten(theta_i)), rho_i in coefficient form.
//  Phi_72: theta_i flattens to 24 Fq3 values; v0[j][c] = sum_i sum_r theta_i[r][c]
//    coeff_j(X^r rho_i) (d is the constant 24 there).
//  X^d + 1: flatten(theta_i) is theta_i's d words Theta_i, and sum_r Theta_i[r] X^r rho_i
//    is the ring product rho_i Theta_i with Theta_i read as coefficients, so
//    v0 = ICRT(sum_i CRT(rho_i) (.) CRT(Theta_i)): 2n + 1 transforms, nothing quadratic in d.
//    rho_ntt (may be null): CRT(rho_i), where the caller already holds it.
void rot_lin(int d, const uint64_t *rho_coeff, const uint64_t *rho_ntt, const uint64_t *theta, size_t n,
             uint64_t *v0) {
  if (d == 24) {
    memset(v0, 0, 72 * sizeof(uint64_t));
    for (size_t i = 0; i < n; i++) {
      const uint64_t *rc = rho_coeff + i * 24, *ti = theta + i * 72;
      for (int j = 0; j < 24; j++)
        for (int r = 0; r < 24; r++) {
          const uint64_t w = rot_coeff(rc, j, r);
          for (int c = 0; c < 3; c++) v0[j * 3 + c] = gl::add(v0[j * 3 + c], gl::mul(ti[r * 3 + c], w));
        }
    }
    return;
  }
  const Nega N(d);
  Vec a(d), b(d);
  memset(v0, 0, (size_t)d * sizeof(uint64_t));
  for (size_t i = 0; i < n; i++) {
    memcpy(a.data(), theta + i * d, (size_t)d * 8);
    N.crt(a.data());
    const uint64_t *r = rho_ntt ? rho_ntt + i * d : b.data();
    if (!rho_ntt) {
      memcpy(b.data(), rho_coeff + i * d, (size_t)d * 8);
      N.crt(b.data());
    }
    for (int k = 0; k < d; k++) v0[k] = gl::add(v0[k], gl::mul(a[k], r[k]));
  }
  N.icrt(v0);
}

// NTT elements of one ring as d-word spans; every function takes and returns canonical words
struct Ring {
  int d, tb;
  Vec zero() const { return Vec(d, 0); }
  Vec scal(const uint64_t *b) const {  // from_scalar of a base-ring element
    Vec e(d);
    for (int i = 0; i < d; i++) e[i] = b[i % tb];
    return e;
  }
  Vec fromu(uint64_t x) const {
    const uint64_t b[3] = {x % gl::P, 0, 0};
    return scal(b);
  }
  Vec one() const { return fromu(1); }
  Vec at(const Vec &v, size_t i) const { return Vec(v.begin() + i * d, v.begin() + (i + 1) * d); }
  Vec mul(const uint64_t *a, const uint64_t *b) const {
    Vec r(d);
    for (int s = 0; s < d; s += tb) gl::base_mul(a + s, b + s, &r[s], tb);
    return r;
  }
  Vec mul(const Vec &a, const Vec &b) const { return mul(a.data(), b.data()); }
  Vec add(const Vec &a, const uint64_t *b) const {
    Vec r(d);
    for (int i = 0; i < d; i++) r[i] = gl::add(a[i], b[i]);
    return r;
  }
  Vec add(const Vec &a, const Vec &b) const { return add(a, b.data()); }
  Vec sub(const Vec &a, const Vec &b) const {
    Vec r(d);
    for (int i = 0; i < d; i++) r[i] = gl::sub(a[i], b[i]);
    return r;
  }
  void mac(uint64_t *acc, const uint64_t *a, const uint64_t *b) const {  // acc += a b
    uint64_t p[3];
    for (int s = 0; s < d; s += tb) {
      gl::base_mul(a + s, b + s, p, tb);
      for (int c = 0; c < tb; c++) acc[s + c] = gl::add(acc[s + c], p[c]);
    }
  }
  // sum_j base^(j+1) vals[j] (the successors(Some(a), a * ..) sums of folding/utils.rs), by Horner
  Vec powers_dot(const Vec &base, const uint64_t *vals, size_t n) const {
    Vec h = zero();
    for (size_t j = n; j-- > 0;) h = mul(base, add(h, vals + j * d));
    return h;
  }
  // eq (utils/sumcheck/utils.rs:78-92): prod (2 x_i y_i - x_i - y_i + 1) over n elements
  Vec eq(const Vec &x, const Vec &y, int n) const {
    Vec res = one();
    const Vec o = one();
    for (int i = 0; i < n; i++) {
      const Vec xi = at(x, i), yi = at(y, i), p = mul(xi, yi);
      res = mul(res, add(sub(sub(add(p, p), xi), yi), o));
    }
    return res;
  }
};

struct Tr {
  lf_transcript *t;
  Ring R;
  explicit Tr(const Ring &r) : t(lf_transcript_new()), R(r) {}
  ~Tr() { lf_transcript_free(t); }
  void absorb(const uint64_t *e, size_t n) { lf_transcript_absorb_ring(t, e, n, R.d, LF_REPR_CANONICAL); }
  void absorb(const Vec &e) { absorb(e.data(), e.size() / R.d); }
  void label(const char *s) {  // BasePrimeField::from_be_bytes_mod_order
    uint64_t v = 0;
    for (const char *p = s; *p; p++) v = gl::add(gl::mul(v, 256), (uint8_t)*p);
    absorb(R.fromu(v));
  }
  // one base-ring challenge: tb samples, then their re-observation (fiat_shamir.rs:69-86 for
  // Fq3; one sample and its observe for Fq, this project's convention at X^d + 1)
  void challenge(uint64_t *b) {
    if (R.tb == 3) return lf_transcript_get_challenge(t, b);
    b[0] = lf_transcript_sample(t);
    lf_transcript_observe(t, b[0]);
  }
  void challenges(Vec &out, int n) {  // n challenges, each broadcast into an NTT element
    out.resize((size_t)n * R.d);
    for (int i = 0; i < n; i++) {
      uint64_t b[3];
      challenge(b);
      const Vec e = R.scal(b);
      memcpy(&out[(size_t)i * R.d], e.data(), (size_t)R.d * 8);
    }
  }
};

// the round polynomial through (i, p_i), i < len, at the base-ring point r: sum_i p_i L_i(r),
// L_i(r) = prod_{j != i} (r - j) / (i - j) (utils/sumcheck/verifier.rs interpolate_uni_poly);
// the weights are base-ring elements, so every slot is interpolated with the same ones
Vec interpolate(const Ring &R, const uint64_t *p, int len, const uint64_t *r) {
  Vec res = R.zero();
  for (int i = 0; i < len; i++) {
    uint64_t num[3] = {1, 0, 0};
    uint64_t den = 1;
    for (int j = 0; j < len; j++) {
      if (j == i) continue;
      const uint64_t rj[3] = {gl::sub(r[0], (uint64_t)j), r[1], r[2]};
      gl::base_mul(num, rj, num, R.tb);
      den = gl::mul(den, i > j ? (uint64_t)(i - j) : gl::P - (uint64_t)(j - i));
    }
    const uint64_t di = gl::inv(den);
    for (int c = 0; c < R.tb; c++) num[c] = gl::mul(num[c], di);
    const Vec w = R.scal(num);
    R.mac(res.data(), p + (size_t)i * R.d, w.data());
  }
  return res;
}

// MLSumcheck::verify_as_subprotocol (utils/sumcheck.rs:90-111): the round messages
// absorbed, the challenges drawn and absorbed, p_i(0) + p_i(1) checked against the running
// claim; false at the first round that misses. point: nv broadcast challenges; claim: in the
// claimed sum, out the final one
bool sumcheck(Tr &T, const Vec &proof, int nv, int degree, Vec &point, Vec &claim) {
  const Ring &R = T.R;
  T.absorb(R.fromu((uint64_t)nv));
  T.absorb(R.fromu((uint64_t)degree));
  point.resize((size_t)nv * R.d);
  for (int i = 0; i < nv; i++) {
    const uint64_t *msg = proof.data() + (size_t)i * (degree + 1) * R.d;
    T.absorb(msg, degree + 1);
    uint64_t r[3] = {0, 0, 0};
    T.challenge(r);
    const Vec re = R.scal(r);
    memcpy(&point[(size_t)i * R.d], re.data(), (size_t)R.d * 8);
    T.absorb(re);
    if (R.add(Vec(msg, msg + R.d), msg + R.d) != claim) return false;
    claim = interpolate(R, msg, degree + 1, r);
  }
  return true;
}

}  // namespace

extern "C" {

int lf_rot_lin_combination(int d, const uint64_t *rho_coeff, const uint64_t *theta, size_t n, uint64_t *v0, int repr) {
  if (!v0 || (n && (!rho_coeff || !theta)) || (repr != LF_REPR_CANONICAL && repr != LF_REPR_MONTGOMERY))
    return LF_ERR_INVALID_ARG;
  if (d != 24 && !nega_degree(d)) return LF_ERR_UNSUPPORTED_RING;
  const size_t tau = d == 24 ? 3 : 1;
  const bool mont = repr == LF_REPR_MONTGOMERY;
  Vec rc(rho_coeff, rho_coeff + n * d), th(theta, theta + n * tau * d), out(tau * d);
  for (auto &x : rc) x = mont ? gl::from_mont(x) : gl::canon(x);
  for (auto &x : th) x = mont ? gl::from_mont(x) : gl::canon(x);
  rot_lin(d, rc.data(), nullptr, th.data(), n, out.data());
  for (size_t i = 0; i < out.size(); i++) v0[i] = mont ? gl::to_mont(out[i]) : out[i];
  return LF_OK;
}

int lf_fold_verify(const lf_ccs_desc *ccs, const lf_params *pr, const lf_lcccs *acc, const uint64_t *cm_i,
                   const uint64_t *x_ccs, const lf_lfproof_mut *proof, lf_lcccs_mut *out, int *failed, int repr) {
  if (failed) *failed = LF_VERIFY_OK;
  if (!ccs || !pr || !acc || !cm_i || !proof || !out || pr->d != acc->d) return LF_ERR_INVALID_ARG;
  if (pr->d != 24 && !nega_degree(pr->d)) return LF_ERR_UNSUPPORTED_RING;
  if (repr != LF_REPR_CANONICAL && repr != LF_REPR_MONTGOMERY) return LF_ERR_INVALID_ARG;
  const Ring R{pr->d, pr->d == 24 ? 3 : 1};
  const int D = R.d, tau = R.tb;  // tau MLEs of f_hat: the base ring's degree over Fq
  const int t = ccs->t, q = ccs->q, degree = ccs->degree, K = pr->K;
  const size_t m = ccs->m, l = ccs->l, L1 = l + 1;
  if (t < 2 || q < 1 || degree < 1 || K < 1 || pr->b_small < 1 || pr->b_small > (1u << 20) || !m || (m & (m - 1)) ||
      (!x_ccs && l) || !ccs->c || !ccs->S_off || !ccs->S_idx)
    return LF_ERR_INVALID_ARG;
  const int bs = (int)pr->b_small;
  int s = 0;
  while (((size_t)1 << s) < m) s++;
  const size_t kappa = acc->cm.n;
  if (acc->r.n != (size_t)s || acc->v.n != (size_t)tau || !kappa || acc->u.n != (size_t)t || acc->x_w.n != l)
    return LF_ERR_INCORRECT_LENGTH;
  if ((s && !acc->r.elems) || !acc->v.elems || !acc->cm.elems || !acc->u.elems || (l && !acc->x_w.elems) || !acc->h)
    return LF_ERR_INVALID_ARG;
  if ((s && !out->r) || !out->v || !out->cm || !out->u || (l && !out->x_w) || !out->h) return LF_ERR_INVALID_ARG;
  const uint64_t *pp[] = {proof->lin_sumcheck, proof->lin_v,  proof->lin_u,  proof->u_s[0], proof->u_s[1],
                          proof->v_s[0],       proof->v_s[1], proof->x_s[0], proof->x_s[1], proof->y_s[0],
                          proof->y_s[1],       proof->fold_sumcheck, proof->theta_s, proof->eta_s};
  for (size_t i = 0; i < sizeof(pp) / sizeof(pp[0]); i++)
    if (!pp[i] && !((i == 0 || i == 11) && !s)) return LF_ERR_INVALID_ARG;
  for (int i = 0; i < q; i++)
    if (ccs->S_off[i] < 0 || ccs->S_off[i + 1] < ccs->S_off[i]) return LF_ERR_INVALID_ARG;
  for (int k = ccs->S_off[0]; k < ccs->S_off[q]; k++)
    if (ccs->S_idx[k] < 0 || ccs->S_idx[k] >= t) return LF_ERR_INVALID_ARG;
  const bool mont = repr == LF_REPR_MONTGOMERY;
  auto cp = [&](const uint64_t *p, size_t elems) {  // a canonical copy of `elems` NTT elements
    Vec v(p, p + elems * D);
    for (auto &x : v) x = mont ? gl::from_mont(x) : gl::canon(x);
    return v;
  };
  auto reject = [&](int what) {
    if (failed) *failed = what;
    return LF_ERR_VERIFICATION;
  };
  const Vec c = cp(ccs->c, q), ar = cp(acc->r.elems, s), av = cp(acc->v.elems, tau), acm = cp(acc->cm.elems, kappa),
            au = cp(acc->u.elems, t), cmi = cp(cm_i, kappa), lsc = cp(proof->lin_sumcheck, (size_t)s * (degree + 2)),
            lv = cp(proof->lin_v, tau), lu = cp(proof->lin_u, t),
            fsc = cp(proof->fold_sumcheck, (size_t)s * (2 * bs + 1)), th = cp(proof->theta_s, 2 * (size_t)K * tau),
            et = cp(proof->eta_s, 2 * (size_t)K * t);
  Vec xh[2] = {cp(acc->x_w.elems, l), cp(x_ccs, l)};  // x_w || h of the two decomposed instances
  const Vec ah = cp(acc->h, 1), onev = R.one();
  xh[0].insert(xh[0].end(), ah.begin(), ah.end());
  xh[1].insert(xh[1].end(), onev.begin(), onev.end());
  Vec us[2], vs[2], xs[2], ys[2];
  for (int side = 0; side < 2; side++) {
    us[side] = cp(proof->u_s[side], (size_t)K * t);
    vs[side] = cp(proof->v_s[side], (size_t)K * tau);
    xs[side] = cp(proof->x_s[side], (size_t)K * L1);
    ys[side] = cp(proof->y_s[side], (size_t)K * kappa);
  }
  Tr T(R);
  if (!T.t) return LF_ERR_OUT_OF_MEMORY;
  // absorb_public_input (zk_latticefold.rs:162-184)
  T.label("acc");
  T.absorb(ar);
  T.absorb(av);
  T.absorb(acm);
  T.absorb(au);
  T.absorb(xh[0]);  // x_w, then h
  T.label("cm_i");
  T.absorb(cmi);
  T.absorb(xh[1].data(), l);
  // linearization (linearization.rs:200-285)
  T.label("beta_s");
  Vec beta, r, claim = R.zero();
  T.challenges(beta, s);
  if (!sumcheck(T, lsc, s, degree + 1, r, claim)) return reject(LF_VERIFY_LIN_SUMCHECK);
  Vec inner = R.zero();  // sum_i c_i prod_{j in S_i} u_j
  for (int i = 0; i < q; i++) {
    Vec prod = R.at(c, i);
    for (int k = ccs->S_off[i]; k < ccs->S_off[i + 1]; k++) prod = R.mul(prod.data(), &lu[(size_t)ccs->S_idx[k] * D]);
    inner = R.add(inner, prod);
  }
  if (R.mul(R.eq(r, beta, s), inner) != claim) return reject(LF_VERIFY_LIN_CLAIM);
  T.absorb(lv);
  T.absorb(lu);
  // decompositions (decomposition.rs:90-155): the 2K decomposed instances absorbed, accumulator
  // side first; then every decomposed vector recomposes (b^k weights) to its source
  for (int side = 0; side < 2; side++)
    for (int k = 0; k < K; k++) {
      T.absorb(&xs[side][(size_t)k * L1 * D], L1);
      T.absorb(&ys[side][(size_t)k * kappa * D], kappa);
      T.absorb(&us[side][(size_t)k * t * D], t);
      T.absorb(&vs[side][(size_t)k * tau * D], tau);
    }
  const Vec *src_cm[2] = {&acm, &cmi}, *src_v[2] = {&av, &lv}, *src_u[2] = {&au, &lu};
  for (int side = 0; side < 2; side++) {
    const struct {
      const Vec &parts, &want;
      size_t n;
      int code;
    } chks[4] = {{ys[side], *src_cm[side], kappa, LF_VERIFY_DEC_Y},
                 {vs[side], *src_v[side], (size_t)tau, LF_VERIFY_DEC_V},
                 {us[side], *src_u[side], (size_t)t, LF_VERIFY_DEC_U},
                 {xs[side], xh[side], L1, LF_VERIFY_DEC_X}};
    for (const auto &ch : chks) {
      Vec sum(ch.n * D, 0);
      uint64_t bk = 1;
      for (int k = 0; k < K; k++) {
        const Vec w = R.fromu(bk);
        for (size_t j = 0; j < ch.n; j++) R.mac(&sum[j * D], &ch.parts[((size_t)k * ch.n + j) * D], w.data());
        bk = gl::mul(bk, pr->b_small);
      }
      if (sum != ch.want) return reject(ch.code);
    }
  }
  // folding (folding.rs:133-200): squeeze_alpha_beta_zeta_mu (folding/utils.rs:51-96), the
  // rounds from sum_i (alpha_i powers . v_i + zeta_i powers . u_i)
  Vec alpha, zeta, mu, fbeta, r0;
  T.label("alpha_s");
  T.challenges(alpha, 2 * K);
  T.label("zeta_s");
  T.challenges(zeta, 2 * K);
  T.label("mu_s");
  T.challenges(mu, 2 * K - 1);
  mu.insert(mu.end(), onev.begin(), onev.end());
  T.label("beta_s");
  T.challenges(fbeta, s);
  claim = R.zero();
  for (int i = 0; i < 2 * K; i++) {
    const int side = i / K, k = i % K;
    claim = R.add(claim, R.powers_dot(R.at(alpha, i), &vs[side][(size_t)k * tau * D], tau));
    claim = R.add(claim, R.powers_dot(R.at(zeta, i), &us[side][(size_t)k * t * D], t));
  }
  if (!sumcheck(T, fsc, s, 2 * bs, r0, claim)) return reject(LF_VERIFY_FOLD_SUMCHECK);
  // compute_sumcheck_claim_expected_value (folding/utils.rs:380-421); the decomposed
  // instances keep their source's point: acc.r on the left, the linearization's r on the right
  const Vec e_ast = R.eq(fbeta, r0, s), e_side[2] = {R.eq(ar, r0, s), R.eq(r, r0, s)};
  Vec should = R.zero();
  for (int i = 0; i < 2 * K; i++) {
    const Vec a = R.at(alpha, i), z = R.at(zeta, i), mi = R.at(mu, i), &e_i = e_side[i / K];
    const uint64_t *ti = &th[(size_t)i * tau * D];
    Vec norm = R.zero(), pm = mi;
    for (int j = 0; j < tau; j++) {
      const Vec tj(ti + (size_t)j * D, ti + (size_t)(j + 1) * D);
      Vec prod = tj;  // prod_{b < b_small} (theta - b)(theta + b), its b = 0 factor once
      for (int b = 1; b < bs; b++) prod = R.mul(prod, R.mul(R.sub(tj, R.fromu(b)), R.add(tj, R.fromu(b))));
      R.mac(norm.data(), pm.data(), prod.data());
      pm = R.mul(pm, mi);
    }
    const Vec sa = R.powers_dot(a, ti, tau), se = R.powers_dot(z, &et[(size_t)i * t * D], t);
    R.mac(should.data(), sa.data(), e_i.data());
    R.mac(should.data(), e_ast.data(), norm.data());
    R.mac(should.data(), e_i.data(), se.data());
  }
  if (should != claim) return reject(LF_VERIFY_FOLD_CLAIM);
  for (int i = 0; i < 2 * K; i++) T.absorb(&th[(size_t)i * tau * D], tau);
  for (int i = 0; i < 2 * K; i++) T.absorb(&et[(size_t)i * t * D], t);
  // get_rhos (folding/utils.rs:116-127): 2K - 1 short challenges and ONE, and their CRT
  T.label("rho_s");
  Vec rc(2 * (size_t)K * D, 0);
  if (lf_transcript_get_short_challenges(T.t, D, 2 * K - 1, rc.data()) != LF_OK) return LF_ERR_CHALLENGE_BYTES;
  rc[(size_t)(2 * K - 1) * D] = 1;
  Vec rho = rc;
  if (D == 24) {
    for (int i = 0; i < 2 * K; i++) ring::phi72_crt(&rho[(size_t)i * D]);
  } else {
    const Nega N(D);
    for (int i = 0; i < 2 * K; i++) N.crt(&rho[(size_t)i * D]);
  }
  // the folded instance (compute_v0_u0_x0_cm_0, folding/utils.rs:456-517; prepare_public_output)
  Vec cm0(kappa * D, 0), u0((size_t)t * D, 0), x0(L1 * D, 0), v0((size_t)tau * D, 0);
  for (int i = 0; i < 2 * K; i++) {
    const int side = i / K, k = i % K;
    const uint64_t *ri = &rho[(size_t)i * D];
    for (size_t j = 0; j < kappa; j++) R.mac(&cm0[j * D], &ys[side][((size_t)k * kappa + j) * D], ri);
    for (int j = 0; j < t; j++) R.mac(&u0[(size_t)j * D], &et[((size_t)i * t + j) * D], ri);
    for (size_t j = 0; j < L1; j++) R.mac(&x0[j * D], &xs[side][((size_t)k * L1 + j) * D], ri);
  }
  rot_lin(D, rc.data(), rho.data(), th.data(), 2 * (size_t)K, v0.data());
  auto emit = [&](uint64_t *dst, const uint64_t *src, size_t elems) {
    for (size_t i = 0; i < elems * D; i++) dst[i] = mont ? gl::to_mont(src[i]) : src[i];
  };
  emit(out->r, r0.data(), s);
  emit(out->v, v0.data(), tau);
  emit(out->cm, cm0.data(), kappa);
  emit(out->u, u0.data(), t);
  if (l) emit(out->x_w, x0.data(), l);
  emit(out->h, x0.data() + l * D, 1);
  return LF_OK;
}

}  // extern "C"
