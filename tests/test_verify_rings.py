"""lf_fold_verify at the X^d + 1 rings (tests/test_verify.py is its Phi_72 twin): against the
oracle's restated verifier (oracle/nifs.py fold_verify, generic in d) it accepts the honest
proofs and re-derives the same folded LCCCS -- the prover's -- in both representations, and
rejects what the oracle rejects at the same named check. The base ring is Fq there (tau = 1):
v_s[k] and theta_s[i] hold one element. v_0 goes through the verifier's host negacyclic
transform; lf_rot_lin_combination is that step alone, pinned to the oracle's quadratic
rotation sum at every degree. Host code only (no device call)."""
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import nifs as N
import oracle as O
from test_nifs_oracle import instance
from test_replay import acc_dict, flat, proof_dict
from test_verify import lcccs_dict


def la_params(pr):
    p = LA.goldilocks_dp(pr.d)
    p.B, p.L, p.b_small, p.K = pr.B, pr.L, pr.b_small, pr.K
    return p


def verify(pr, ccs, kappa, acc, cmi, xi, proof, repr=LA.REPR_CANONICAL, conv=lambda a: a):
    return LA.fold_verify(la_params(pr), ccs.t, ccs.m, ccs.l, ccs.degree, conv(flat(ccs.c)), ccs.S, kappa,
                          {k: conv(v) for k, v in acc_dict(acc).items()}, conv(np.asarray(cmi, np.uint64)),
                          conv(flat(xi)), {k: ([conv(x) for x in v] if isinstance(v, list) else conv(v))
                                           for k, v in proof_dict(proof).items()}, repr)


@functools.lru_cache(maxsize=None)
def proved(d, W=5, l=2, t=4, deg=2, kappa=3, satisfied=True):
    """one oracle fold per shape, shared (read only) by the tests below"""
    pr, ccs, A, kappa, acc, Wa, cmi, xi, Wi = instance(d, W=W, l=l, t=t, deg=deg, kappa=kappa, seed=W + t,
                                                       satisfied=satisfied)
    out, _, proof = N.fold_prove(ccs, A, kappa, acc, Wa, cmi, xi, Wi, pr)
    return pr, ccs, kappa, acc, cmi, xi, proof, out


@pytest.mark.parametrize("d,W,l,t,deg,kappa", [(16, 5, 2, 4, 2, 3), (32, 5, 2, 4, 2, 3), (64, 5, 2, 4, 2, 3),
                                               (1024, 5, 2, 4, 2, 2), (16, 7, 0, 3, 2, 2)])
def test_verify_accepts_and_folds_like_the_oracle(d, W, l, t, deg, kappa):
    pr, ccs, kappa, acc, cmi, xi, proof, out = proved(d, W, l, t, deg, kappa)
    want = lcccs_dict(N.fold_verify(ccs, acc, cmi, xi, proof, pr))
    got = verify(pr, ccs, kappa, acc, cmi, xi, proof)
    assert got["v"].size == d  # tau = 1
    for k in want:  # v is O.rot_lin_combination's: the host transform against the rotation sum
        assert np.array_equal(got[k], want[k]), k
    for k, v in lcccs_dict(out).items():  # and it is the prover's folded LCCCS
        assert np.array_equal(got[k], v), k


def test_verify_b_small_4():
    """the norm product prod_{j < b_small} (theta - j)(theta + j) and the 2 b_small + 1 evaluations
    per folding round past b_small = 2: b_small = 4, K = 8 (4^8 >= 2 B)"""
    d, W, l, t, deg, kappa = 16, 5, 2, 4, 2, 3
    pr = N.Params(d, b_small=4, K=8)
    ccs = N.satisfied_ccs(d, W, l, t, deg, 9, pr)
    (xa, wa), (xi, wi) = N.satisfying_z(ccs, W, 13), N.satisfying_z(ccs, W, 14)
    Nn = W * pr.L
    A = O.fill_uniform(kappa * Nn * d, 15)

    def wit(w):
        fc, f = O.witness_from_w_ccs(w, d, pr.B, pr.L)
        return N.Witness(w_ccs=w, f=f, f_coeff=fc)

    Wa, Wi = wit(wa), wit(wi)
    cma, cmi = O.ajtai_commit(A, kappa, Nn, d, Wa.f), O.ajtai_commit(A, kappa, Nn, d, Wi.f)
    acc = N.linearize_fresh(ccs, cma, xa, Wa, pr)
    out, _, proof = N.fold_prove(ccs, A, kappa, acc, Wa, cmi, xi, Wi, pr)
    assert np.asarray(proof.fold_sumcheck).size == ccs.s * 9 * d
    want = lcccs_dict(N.fold_verify(ccs, acc, cmi, xi, proof, pr))
    got = verify(pr, ccs, kappa, acc, cmi, xi, proof)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for k, v in lcccs_dict(out).items():
        assert np.array_equal(got[k], v), k
    bad = tampered(proof, d, "theta_s", (5, 0))
    with pytest.raises(ValueError, match="folding evaluation claim"):
        N.fold_verify(ccs, acc, cmi, xi, bad, pr)
    with pytest.raises(LA.VerificationError) as e:
        verify(pr, ccs, kappa, acc, cmi, xi, bad)
    assert LA.VERIFY_CHECKS[e.value.check] == "folding evaluation claim"


def test_verify_montgomery_boundary():
    pr, ccs, kappa, acc, cmi, xi, proof, _ = proved(16)
    mont = np.vectorize(O.to_mont, otypes=[np.uint64])
    unmont = np.vectorize(O.from_mont, otypes=[np.uint64])
    a = verify(pr, ccs, kappa, acc, cmi, xi, proof)
    b = verify(pr, ccs, kappa, acc, cmi, xi, proof, LA.REPR_MONTGOMERY, mont)
    for k in a:
        assert np.array_equal(unmont(b[k]), a[k]), k


def tampered(proof, d, field, idx, side=None):
    """a copy of the oracle proof with one ring element of `field` bumped by ONE: idx = (i, j)
    for a list of lists, (i, None) for a flat list; side for the decomposition proofs"""
    p = N.Proof(**{**proof.__dict__})
    i, j = idx
    if side is not None:
        p.dec = [dict(proof.dec[0]), dict(proof.dec[1])]
        rows = [list(x) for x in proof.dec[side][field]]
        rows[i][j] = N.add(rows[i][j], N.one(d))
        p.dec[side][field] = rows
    elif j is None:
        vals = list(getattr(proof, field))
        vals[i] = N.add(vals[i], N.one(d))
        setattr(p, field, vals)
    else:
        vals = [list(x) for x in getattr(proof, field)]
        vals[i][j] = N.add(vals[i][j], N.one(d))
        setattr(p, field, vals)
    return p


# indices valid at tau = 1 (one element per v_s[k] and theta_s[i]), kappa = 3, t = 4, l = 2
TAMPERS = [
    ("theta_s", (3, 0), None, "folding evaluation claim"),
    ("eta_s", (17, 2), None, "folding evaluation claim"),
    ("y_s", (2, 1), 0, "decomposition recompose y"),
    ("u_s", (4, 1), 1, "decomposition recompose u"),
    ("v_s", (14, 0), 1, "decomposition recompose v"),
    ("x_s", (1, 2), 0, "decomposition recompose x"),
    ("lin_u", (0, None), None, "linearization evaluation claim"),
]


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("field,idx,side,check", TAMPERS)
def test_verify_rejects_tampering_like_the_oracle(d, field, idx, side, check):
    pr, ccs, kappa, acc, cmi, xi, proof, _ = proved(d)
    bad = tampered(proof, d, field, idx, side)
    with pytest.raises(ValueError, match=check.split()[-1] if "recompose" in check else check):
        N.fold_verify(ccs, acc, cmi, xi, bad, pr)
    with pytest.raises(LA.VerificationError) as e:
        verify(pr, ccs, kappa, acc, cmi, xi, bad)
    assert LA.VERIFY_CHECKS[e.value.check] == check


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("field,check,what", [("lin_sumcheck", 1, "linearization sumcheck"),
                                              ("fold_sumcheck", 7, "folding sumcheck")])
def test_verify_rejects_sumcheck_messages(d, field, check, what):
    """round 0 of either sumcheck: p(0) + p(1) no longer meets the claim"""
    pr, ccs, kappa, acc, cmi, xi, proof, _ = proved(d)
    p = N.Proof(**{**proof.__dict__})
    sc = np.array(getattr(proof, field), np.uint64).copy()
    sc[0] = (int(sc[0]) + 1) % LA.P  # round 0, evaluation at 0, slot 0
    setattr(p, field, sc)
    with pytest.raises(ValueError, match=what):
        N.fold_verify(ccs, acc, cmi, xi, p, pr)
    with pytest.raises(LA.VerificationError) as e:
        verify(pr, ccs, kappa, acc, cmi, xi, p)
    assert e.value.check == check and LA.VERIFY_CHECKS[check] == what


@pytest.mark.parametrize("d", [16, 64])
def test_verify_rejects_unsatisfied_ccs(d):
    pr, ccs, kappa, acc, cmi, xi, proof, _ = proved(d, satisfied=False)
    with pytest.raises(ValueError, match="linearization"):
        N.fold_verify(ccs, acc, cmi, xi, proof, pr)
    with pytest.raises(LA.VerificationError) as e:
        verify(pr, ccs, kappa, acc, cmi, xi, proof)
    assert "linearization" in LA.VERIFY_CHECKS[e.value.check]


@pytest.mark.parametrize("d", [16, 32, 64, 128, 256, 512, 1024, 2048, 4096])
def test_host_transform_v0_is_the_rotation_sum(d):
    """v_0 = ICRT(sum_i CRT(rho_i) (.) CRT(Theta_i)) through the host negacyclic transform, against
    the oracle's coefficient-by-coefficient rot_lin_combination: short rho_i (as get_rhos draws
    them) and ONE last, theta uniform; both representations"""
    n = 3
    rng = np.random.default_rng(d)
    rho = np.concatenate([LA.short_challenge(rng.integers(0, 256, 3 * d // 4, dtype=np.uint8).tobytes(), d)
                          for _ in range(n - 1)] + [np.eye(1, d, dtype=np.uint64).ravel()])
    theta = O.fill_uniform(n * d, 40 + d)
    want = O.rot_lin_combination(rho, theta, d)
    assert np.array_equal(LA.rot_lin_combination(rho, theta, d), want)
    mont = np.vectorize(O.to_mont, otypes=[np.uint64])
    got = LA.rot_lin_combination(mont(rho), mont(theta), d, LA.REPR_MONTGOMERY)
    assert np.array_equal(got, mont(want))


def test_host_rot_lin_combination_phi72_and_bad_degree():
    rho, theta = O.fill_uniform(4 * 24, 1), O.fill_uniform(4 * 72, 2)
    assert np.array_equal(LA.rot_lin_combination(rho, theta, 24), O.rot_lin_combination(rho, theta, 24))
    with pytest.raises(LA.LfError) as e:
        LA.rot_lin_combination(np.zeros(48, np.uint64), np.zeros(48, np.uint64), 48)
    assert e.value.code == 2


def test_verify_argument_checks():
    pr, ccs, kappa, acc, cmi, xi, proof, _ = proved(16)
    a, pf = acc_dict(acc), proof_dict(proof)
    args = (ccs.t, ccs.m, ccs.l, ccs.degree, flat(ccs.c), ccs.S, kappa)
    # pr.d != acc.d (fold_verify hands params.d on as the accumulator's): through the C ABI
    with pytest.raises(LA.LfError) as e:
        raw_verify(LA.goldilocks_dp(32), 16, ccs, a, cmi, xi, pf)
    assert e.value.code == 1
    with pytest.raises(LA.LfError) as e:  # a degree that is no ring of the library
        raw_verify(LA.goldilocks_dp(48), 48, ccs, a, cmi, xi, pf)
    assert e.value.code == 2
    for k in ("r", "v", "u", "x_w", "cm"):  # a slice one element short: s, tau, t, l; kappa = 0
        short = dict(a)
        short[k] = a[k][:0] if k == "cm" else a[k][:-16]
        with pytest.raises(LA.LfError) as e:
            raw_verify(LA.goldilocks_dp(16), 16, ccs, short, cmi, xi, pf)
        assert e.value.code == 7, k
    assert LA.fold_verify(LA.goldilocks_dp(16), *args, a, cmi, flat(xi), pf)["r"].size == ccs.s * 16


def raw_verify(params, acc_d, ccs, a, cmi, xi, pf):
    """lf_fold_verify with the accumulator's d and slice lengths given apart from params.d"""
    import ctypes as C

    from latticeum_amd._lib import LfCcsDesc, LfLcccs, LfLcccsMut, LfLfproofMut, LfRingSlice, load
    lib, d = load(), 16
    c = flat(ccs.c)
    off = np.zeros(len(ccs.S) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in ccs.S])
    idx = np.array([j for x in ccs.S for j in x], np.int32)
    desc = LfCcsDesc(ccs.t, ccs.m, ccs.l, ccs.degree, len(ccs.S), c.ctypes.data, off.ctypes.data, idx.ctypes.data)
    keep = {k: np.ascontiguousarray(v, np.uint64) for k, v in a.items()}
    sl = lambda x: LfRingSlice(x.ctypes.data, x.size // d)
    A = LfLcccs(acc_d, sl(keep["r"]), sl(keep["v"]), sl(keep["cm"]), sl(keep["u"]), sl(keep["x_w"]),
                keep["h"].ctypes.data)
    PM = LfLfproofMut()
    for k in ("lin_sumcheck", "lin_v", "lin_u", "fold_sumcheck", "theta_s", "eta_s"):
        setattr(PM, k, pf[k].ctypes.data)
    for k in ("u_s", "v_s", "x_s", "y_s"):
        for side in range(2):
            getattr(PM, k)[side] = pf[k][side].ctypes.data
    # outputs sized for the largest ring, so no argument check is what keeps a write in bounds
    outs = [np.zeros(64 * 4096, np.uint64) for _ in range(6)]
    O_ = LfLcccsMut(*[o.ctypes.data for o in outs])
    cm, xc = np.ascontiguousarray(cmi, np.uint64), flat(xi)
    failed = C.c_int(0)
    rc = lib.lf_fold_verify(C.byref(desc), C.byref(params), C.byref(A), cm.ctypes.data, xc.ctypes.data, C.byref(PM),
                            C.byref(O_), C.byref(failed), 0)
    if rc:
        raise LA.LfError(rc, lib.lf_status_string(rc).decode())
