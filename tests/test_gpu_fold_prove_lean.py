"""lf_fold_prove on a lean prover (lf_prover_create_lean: the 2K decomposed witnesses held as
packed digit planes only) against the oracle's fold(): the proof, the folded LCCCS and the
folded witness byte for byte, lf_fold_verify accepts the proof and lf_lcccs_check opens the
output. At d = 4096, where the Python prover is too slow, against the row prover on the same
inputs. Also two folds in a row on one lean prover, the bytes a lean prover saves, and the
(scheme, params) for which it cannot be made."""
import numpy as np
import pytest

import latticeum_amd as LA
import nifs as N
import oracle as O
from test_gpu_fold_prove import acc_dict, check_against_oracle, dev_wit, flat, host, witness, zeros

pytestmark = pytest.mark.gpu
LF_ERR_INVALID_ARG = 1  # lf.h

# test_fold_prove_matches_oracle's shapes at d = 24 and 1024, and one each at d = 16 and 64
SHAPES = [(24, 5, 2, 4, 2, 3), (24, 13, 4, 6, 3, 4), (1024, 5, 2, 4, 2, 2), (16, 7, 1, 5, 3, 3), (64, 5, 2, 4, 2, 3)]


class World:
    """a satisfied CCS, a scheme over it, and provers of either kind on one context"""

    def __init__(self, ctx, d, W, l, t, deg, kappa, seed, **par):
        self.ctx, self.d, self.W, self.l, self.deg, self.kappa = ctx, d, W, l, deg, kappa
        self.pr_o, self.pr = N.Params(d), LA.goldilocks_dp(d)
        for k, v in par.items():
            setattr(self.pr_o, k, v)
            setattr(self.pr, k, v)
        self.ccs = N.satisfied_ccs(d, W, l, t, deg, seed, self.pr_o)
        self.Nn = W * self.pr_o.L
        self.A = O.fill_uniform(kappa * self.Nn * d, seed + 6)
        self.sch = LA.AjtaiCommitmentScheme(ctx, self.A.reshape(kappa, self.Nn, d))
        self.M = LA.CCSMatrices(ctx, d, self.ccs.m, self.ccs.n, self.ccs.mats)

    def prover(self, lean):
        return LA.Prover(self.ctx, self.sch, self.pr, self.M, self.l, self.deg, np.concatenate(self.ccs.c),
                         self.ccs.S, lean=lean)

    def instance(self, seed):
        x, w = witness(self.ccs, self.pr_o, seed)
        return x, w, O.ajtai_commit(self.A, self.kappa, self.Nn, self.d, w.f)

    def w_out(self):
        return {"w_ccs": zeros(self.W * self.d), "f": zeros(self.Nn * self.d), "f_coeff": zeros(self.Nn * self.d)}

    def verify(self, acc, cmi, xi, pf):
        c = self.ccs
        return LA.fold_verify(self.pr, c.t, c.m, c.l, c.degree, flat(c.c), c.S, self.kappa, acc, cmi, flat(xi), pf)


def lcccs(a, d):
    return N.LCCCS(r=N.elems(a["r"], d), v=N.elems(a["v"], d), cm=a["cm"], u=N.elems(a["u"], d),
                   x_w=N.elems(a["x_w"], d), h=a["h"])


def accepted_and_open(w, prover, acc, cmi, xi, out, pf, w_out):
    """lf_fold_verify re-derives the folded LCCCS from the proof, and lf_lcccs_check opens it"""
    got = w.verify(acc, cmi, xi, pf)
    for k, v in out.items():
        assert np.array_equal(got[k], v), k
    prover.check_lcccs(out, w_out)


@pytest.mark.parametrize("d,W,l,t,deg,kappa", SHAPES)
def test_lean_fold_matches_oracle(d, W, l, t, deg, kappa):
    ctx = LA.Context(0)
    try:
        w = World(ctx, d, W, l, t, deg, kappa, 7 + d + W)
        prover = w.prover(lean=True)
        assert prover.lean
        (xa, Wa, cma), (xi, Wi, cmi) = w.instance(11), w.instance(12)
        acc = N.linearize_fresh(w.ccs, cma, xa, Wa, w.pr_o)
        oracle = N.fold_prove(w.ccs, w.A, kappa, acc, Wa, cmi, xi, Wi, w.pr_o)
        w_out = w.w_out()
        out, pf = prover.fold_prove(acc_dict(acc), dev_wit(Wa), cmi, flat(xi), dev_wit(Wi), w_out)
        check_against_oracle(out, pf, w_out, *oracle)
        accepted_and_open(w, prover, acc_dict(acc), cmi, xi, out, pf, w_out)
    finally:
        ctx.close()


@pytest.mark.parametrize("d,W,l,t,deg,kappa", [(24, 5, 2, 4, 2, 3), (64, 5, 2, 4, 2, 3)])
def test_two_lean_folds_in_a_row(d, W, l, t, deg, kappa):
    """the second fold takes the first's output as its accumulator: anything the first left in
    the planes or the context's step scratch would show in the second's proof"""
    ctx = LA.Context(0)
    try:
        w = World(ctx, d, W, l, t, deg, kappa, 19 + d + W)
        prover = w.prover(lean=True)
        (xa, Wa, cma), (xi, Wi, cmi), (x3, W3, cm3) = w.instance(11), w.instance(12), w.instance(13)
        acc = N.linearize_fresh(w.ccs, cma, xa, Wa, w.pr_o)
        w_out = w.w_out()
        out, pf = prover.fold_prove(acc_dict(acc), dev_wit(Wa), cmi, flat(xi), dev_wit(Wi), w_out)
        wacc2 = N.Witness(w_ccs=host(w_out["w_ccs"]), f=host(w_out["f"]), f_coeff=host(w_out["f_coeff"]))
        oracle2 = N.fold_prove(w.ccs, w.A, kappa, lcccs(out, d), wacc2, cm3, x3, W3, w.pr_o)
        w_out2 = w.w_out()
        out2, pf2 = prover.fold_prove(out, w_out, cm3, flat(x3), dev_wit(W3), w_out2)
        check_against_oracle(out2, pf2, w_out2, *oracle2)
        accepted_and_open(w, prover, out, cm3, x3, out2, pf2, w_out2)
    finally:
        ctx.close()


def test_lean_fold_equals_row_fold_at_4096():
    d, W, l, t, deg, kappa = 4096, 5, 2, 4, 2, 2
    ctx = LA.Context(0)
    try:
        w = World(ctx, d, W, l, t, deg, kappa, 7 + d + W)
        row, lean = w.prover(lean=False), w.prover(lean=True)
        assert lean.lean and not row.lean
        (xa, Wa, cma), (xi, Wi, cmi) = w.instance(11), w.instance(12)
        acc, _ = row.linearize(cma, flat(xa), dev_wit(Wa))
        acc_l, _ = lean.linearize(cma, flat(xa), dev_wit(Wa))
        for k in acc:
            assert np.array_equal(acc_l[k], acc[k]), k
        w_row, w_lean = w.w_out(), w.w_out()
        out_r, pf_r = row.fold_prove(acc, dev_wit(Wa), cmi, flat(xi), dev_wit(Wi), w_row)
        out_l, pf_l = lean.fold_prove(acc, dev_wit(Wa), cmi, flat(xi), dev_wit(Wi), w_lean)
        for k in out_r:
            assert np.array_equal(out_l[k], out_r[k]), k
        for k, v in pf_r.items():
            for a, b in zip(v, pf_l[k]) if isinstance(v, list) else [(v, pf_l[k])]:
                assert np.array_equal(a, b), k
        for k in w_row:
            assert np.array_equal(host(w_lean[k]), host(w_row[k])), k
        accepted_and_open(w, lean, acc, cmi, xi, out_l, pf_l, w_lean)
    finally:
        ctx.close()


@pytest.mark.parametrize("d,W,l,t,deg,kappa", [(24, 13, 4, 6, 3, 4), (16, 7, 1, 5, 3, 3), (1024, 5, 2, 4, 2, 2),
                                               (4096, 5, 2, 4, 2, 2)])
def test_lean_prover_saves_the_rows(d, W, l, t, deg, kappa):
    """the carve loses 4 K N d words of f_k / f_coeff_k rows and gains the two sides' planes and
    one N-element scratch; each of the 7 parts that changed is rounded up to 32 words"""
    ctx = LA.Context(0)
    try:
        w = World(ctx, d, W, l, t, deg, kappa, 3)
        K, Nn = w.pr.K, w.Nn
        saved = w.prover(lean=False).device_bytes - w.prover(lean=True).device_bytes
        want = 8 * (4 * K * Nn * d - 2 * LA.fold_step_planes_len(w.pr, Nn) - Nn * d)
        assert want > 0 and abs(saved - want) <= 8 * 7 * 31, (saved, want)
    finally:
        ctx.close()


REFUSED = [("b_small", 64, dict(b_small=4, K=8)), ("K16", 64, dict(K=16)), ("d2048", 2048, {}),
           ("not_grouped", 64, dict(L=4))]


@pytest.mark.parametrize("why,d,par", REFUSED, ids=[r[0] for r in REFUSED])
def test_lean_creation_refused_without_a_packed_form(why, d, par):
    """the row prover can be made for these (scheme, params); the lean one cannot, and says why"""
    ctx = LA.Context(0)
    try:
        w = World(ctx, d, 5, 2, 4, 2, 2, 5, **par)
        assert not w.prover(lean=False).lean
        with pytest.raises(LA.LfError) as e:
            w.prover(lean=True)
        assert e.value.code == LF_ERR_INVALID_ARG
        assert "packed form" in str(e.value)
    finally:
        ctx.close()
