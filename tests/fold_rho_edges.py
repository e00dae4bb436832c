"""Inputs at the edges of the short-rho range of the coefficient-form folds (fold_coeff.hip
at d = 1024: every coefficient of every rho_i in [-127, 127]; fold.hip's Phi_72 fold at
d = 24: in [-32, 32]), built from the oracle and plain integers alone. tests/
test_fold_rho_edges.py checks on the CPU that each case has the property it is about;
tests/test_gpu_fold_rho_edges.py runs them through lf_dev_fold_step.

A case is a dict: acc_fc (the accumulator's f_coeff, [N d] canonical), w_ccs (the new
witness, NTT form, [W d]), rho ([2K d], NTT form) and rc (rho's signed coefficients,
[2K][d] int64), plus what the case says about itself (target, out, ...)."""
import functools

import numpy as np

import latticeum_amd as LA
import oracle as O

P = LA.P
BOUND = {1024: 127, 24: 32}  # the accepted magnitude of a rho coefficient
KAPPA = {1024: 2, 24: 3}
TOP = 1 << 14                # B / 2 at B = 2^15
LIVE_PLANES = 14             # |x| = 2^14 - 1: planes 0..13, all with x's sign


def params(d):
    return LA.goldilocks_dp(d)


def worst_sum(d):
    """the attainable magnitude of an f0_coeff term sum: 2 sides, 14 live planes, d products of bound"""
    return 2 * LIVE_PLANES * d * BOUND[d]


def to_field(x):
    """signed integers -> canonical residues (a negative x is stored as p - |x|)"""
    x = np.asarray(x, np.int64)
    return np.where(x < 0, np.uint64(P) - (-x).astype(np.uint64), x.astype(np.uint64))


def signed(x):
    """canonical residues -> their balanced representatives (int64)"""
    x = np.asarray(x, np.uint64)
    return np.where(x > P // 2, (x - np.uint64(P)).view(np.int64), x.view(np.int64))  # u64 wraps to x - p


def rho_ntt(rc, d):
    """signed coefficients [2K][d] -> rho in NTT form, as the step takes it"""
    return O.crt(to_field(rc).ravel(), d)


# ------------------------------------------------------------------ rho
def mid_rho(d, seed):
    """uniform over the whole accepted range, both endpoints forced into every rho_i"""
    b, nw = BOUND[d], 2 * params(d).K
    rng = np.random.default_rng(seed)
    rc = rng.integers(-b, b + 1, size=(nw, d), dtype=np.int64)
    for i in range(nw):
        lo, hi = rng.choice(d, 2, replace=False)
        rc[i, lo], rc[i, hi] = -b, b
    return rc


def extreme_rho(d, seed):
    """every coefficient +-bound"""
    nw = 2 * params(d).K
    return (np.random.default_rng(seed).integers(0, 2, size=(nw, d), dtype=np.int64) * 2 - 1) * BOUND[d]


def one_out_rho(d, seed, i, c, sign):
    """mid_rho with the single coefficient c of rho_i at sign (bound + 1)"""
    rc = mid_rho(d, seed)
    rc[i, c] = sign * (BOUND[d] + 1)
    return rc


def outside(rc, d):
    """[(i, c)] of the coefficients outside the accepted range"""
    return [(int(i), int(c)) for i, c in np.argwhere(np.abs(rc) > BOUND[d])]


# ------------------------------------------------------------------ witnesses
def witness_of_digits(fc, d):
    """the w_ccs whose from_w_ccs digits are fc ([W][L][d] signed); the oracle round-trips it"""
    pr = params(d)
    _, w = O.witness_from_f(O.crt(to_field(fc).ravel(), d), d, pr.B, pr.L)
    back = signed(O.witness_from_w_ccs(w, d, pr.B, pr.L)[0]).reshape(fc.shape)
    assert np.array_equal(back, fc), "the witness does not round-trip to its digits"
    return w


def small_top(rng, W, d):
    """the top limb of a field element: |digit| <= 8"""
    return rng.integers(-6, 8, size=(W, d), dtype=np.int64)


def extreme_digits(d, W, seed, e_star=None, s_star=None):
    """[W][L][d] digits: +-(2^14 - 1) with seeded signs on the limbs below the top (element
    e_star with the signs s_star), a small top limb"""
    L = params(d).L
    rng = np.random.default_rng(seed)
    fc = (rng.integers(0, 2, size=(W, L, d), dtype=np.int64) * 2 - 1) * (TOP - 1)
    fc[:, L - 1] = small_top(rng, W, d)
    if e_star is not None:
        assert e_star % L < L - 1
        fc[e_star // L, e_star % L] = s_star * (TOP - 1)
    return fc


def top_digits(d, W, seed):
    """[W][L][d] digits: random over the balanced range, one in 16 of those below the top limb
    at +-2^14 (plane K - 1 = 14 alone is live there), a small top limb. The balanced
    decomposition keeps a remainder of magnitude B / 2 with the sign of what is left of the
    value, which is the sign of its highest nonzero digit: such a digit takes that sign"""
    L = params(d).L
    rng = np.random.default_rng(seed)
    fc = rng.integers(-(TOP - 1), TOP, size=(W, L, d), dtype=np.int64)
    pick = rng.random((W, L, d)) < 1 / 16
    rnd = rng.integers(0, 2, size=(W, L, d), dtype=np.int64) * 2 - 1
    fc[:, L - 1] = small_top(rng, W, d)
    hs = np.sign(fc[:, L - 1])
    for l in range(L - 2, -1, -1):
        fc[:, l] = np.where(pick[:, l], np.where(hs != 0, hs, rnd[:, l]) * TOP, fc[:, l])
        hs = np.where(hs != 0, hs, np.sign(fc[:, l]))
    return fc


def random_case(d, W, seed):
    """a random witness and an accumulator made like the reference's (no rho yet)"""
    pr = params(d)
    acc_fc, _ = O.witness_from_w_ccs(O.fill_uniform(W * d, seed), d, pr.B, pr.L)
    return {"acc_fc": acc_fc, "w_ccs": O.fill_uniform(W * d, seed + 1)}


def with_rho(case, rc, d, **about):
    return dict(case, rc=rc, rho=rho_ntt(rc, d), **about)


# ------------------------------------------------------------------ the cases
def worst_case(d, W, g_star, c_star, seed):
    """Both sides' element e* = g_star L + 1 is s_j (2^14 - 1) at every coefficient j and all
    2K rho are the one polynomial that multiplies every digit of it into +bound at the target:
    d = 1024: row c_star of the Toeplitz matrix, R[c][j] = rho[c - j] (c >= j), -rho[c - j + 1024]
    (c < j), so rho[c* - j] = bound s_j for j <= c*, rho[c* - j + 1024] = -bound s_j above;
    d = 24: index c_star = 23 of the degree-46 product before the reduction, rho[23 - j] = bound s_j"""
    pr = params(d)
    b, nw = BOUND[d], 2 * pr.K
    e_star = g_star * pr.L + 1
    s = np.random.default_rng(seed).integers(0, 2, size=d, dtype=np.int64) * 2 - 1
    j = np.arange(d)
    r = np.zeros(d, np.int64)
    if d == 24:
        assert c_star == d - 1
    r[(c_star - j) % d] = np.where(j <= c_star, b * s, -b * s)
    rc = np.tile(r, (nw, 1))
    acc = extreme_digits(d, W, seed + 1, e_star, s)
    new = extreme_digits(d, W, seed + 2, e_star, s)
    case = {"acc_fc": to_field(acc).ravel(), "w_ccs": witness_of_digits(new, d), "digits": (acc, new)}
    return with_rho(case, rc, d, target=(e_star, c_star))


def top_limb_case(d, W, g_live, seed):
    """d = 1024: the accumulator's top limb holds +-(2^14 - 1) on group g_live only (planes 4..13
    live in that group's top-limb tile alone), a random accumulator elsewhere, a random new witness"""
    pr = params(d)
    L = pr.L
    case = random_case(d, W, seed)
    rng = np.random.default_rng(seed + 2)
    acc = signed(case["acc_fc"]).reshape(W, L, d).copy()
    acc[g_live, L - 1] = (rng.integers(0, 2, size=d, dtype=np.int64) * 2 - 1) * (TOP - 1)
    case["acc_fc"] = to_field(acc).ravel()
    return with_rho(case, mid_rho(d, seed + 3), d, g_live=g_live, digits=(acc, None))


# ------------------------------------------------------------------ what the fold must give
def planes(case, d):
    """both sides' digit planes [2][K][N][d] in {-1, 0, 1} (the oracle's decompose_witness) and
    the new witness's f_coeff"""
    pr = params(d)
    new_fc = O.witness_from_w_ccs(case["w_ccs"], d, pr.B, pr.L)[0]
    N = new_fc.size // d
    D = [signed(O.decompose_witness(x, d, pr.B, pr.L, pr.b_small, pr.K)[0]).reshape(pr.K, N, d)
         for x in (case["acc_fc"], new_fc)]
    return np.stack(D), new_fc


def conv_sum(case, D, e):
    """sum_i rho_i D_i[e] as a polynomial of degree 2 d - 2, before any reduction (Python integers)"""
    K = D.shape[1]
    d = D.shape[3]
    out = [0] * (2 * d - 1)
    for i in range(2 * K):
        r = [int(x) for x in case["rc"][i]]
        dg = [int(x) for x in D[i // K, i % K, e]]
        for j, x in enumerate(dg):
            if x:
                for m, y in enumerate(r):
                    out[j + m] += x * y
    return out


def reduce_phi72(s):
    """a degree-46 polynomial mod X^24 - X^12 + 1"""
    s = list(s) + [0] * (47 - len(s))
    for t in range(46, 23, -1):  # X^t = X^(t - 12) - X^(t - 24)
        s[t - 12] += s[t]
        s[t - 24] -= s[t]
        s[t] = 0
    return s[:24]


def toeplitz_row(case, D, e, c):
    """d = 1024: f0_coeff[e][c] = sum_i sum_j R_i[c][j] D_i[j][e] (fold_coeff.hip's header)"""
    K, d = D.shape[1], D.shape[3]
    j = np.arange(d)
    tot = 0
    for i in range(2 * K):
        r = case["rc"][i]
        R = np.where(j <= c, r[(c - j) % d], -r[(c - j) % d])
        tot += int((R * D[i // K, i % K, e].astype(np.int64)).sum())
    return tot


def oracle_f0_coeff(case, D_ntt, d):
    """the oracle's f0_coeff [N][d] (signed) from both sides' NTT-form planes"""
    pr = params(d)
    N = D_ntt[0].size // (pr.K * d)
    f0 = O.fold_f0(case["rho"], np.concatenate(D_ntt), 2 * pr.K, N, d)
    return signed(O.witness_from_f(f0, d, pr.B, pr.L)[0]).reshape(N, d)


@functools.lru_cache(maxsize=None)
def build(kind, d, W, *args):
    """the named case (read-only, shared between the tests)
    mid: a random witness and accumulator under that rho; extreme: digits up to +-2^14
    worst: args = (g_star, c_star); top: args = (g_live,); out: args = (i, c, sign)"""
    seed = 9000 + d + 16 * W
    if kind == "mid":
        case = with_rho(random_case(d, W, seed), mid_rho(d, seed + 5), d)
    elif kind == "extreme":  # on digits that reach +-2^14 on both sides: plane K - 1 is live
        acc, new = top_digits(d, W, seed + 3), top_digits(d, W, seed + 4)
        case = {"acc_fc": to_field(acc).ravel(), "w_ccs": witness_of_digits(new, d), "digits": (acc, new)}
        case = with_rho(case, extreme_rho(d, seed + 6), d)
    elif kind == "worst":
        case = worst_case(d, W, args[0], args[1], seed + 7)
    elif kind == "top":
        case = top_limb_case(d, W, args[0], seed + 8)
    elif kind == "out":
        i, c, sign = args
        case = with_rho(random_case(d, W, seed), one_out_rho(d, seed + 5, i, c, sign), d, out=(i, c))
    else:
        raise ValueError(kind)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


# one coefficient out, d = 1024: rho_0 is the first half-wave of k_rho_prep's first block, rho_29
# the last live one of its last block (whose other wave idles on i = 30, 31), rho_14 a middle block's;
# coefficient 0 and 1023 are the two ends of the byte table. d = 24: the first and the last rho
OUT_1024 = [(0, 0, 1), (0, 1023, -1), (14, 0, -1), (14, 1023, 1), (29, 0, 1), (29, 1023, -1)]
OUT_24 = [(0, 0, 1), (0, 23, -1), (29, 0, -1), (29, 23, 1)]
