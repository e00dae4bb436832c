"""The f_hat consumers of the folding prover over the packed digit planes
(lf_dev_fhat_evaluate_planes, lf_dev_fhat_lincomb_planes, lf_sumcheck_prove_fold_planes),
bit for bit against the oracle over the digit rows the planes stand for -- the expected
values are built on the CPU the way tests/test_gpu_sumcheck_paths.py builds them for the row
entries, never taken from the row kernels -- and, beside that, against the row entries on
lf_dev_expand_planes's rows. The packers (tests/planes_pack.py, from the text of lf.h) are
pinned first: the device expands their planes to the digit rows they were made from.

Shapes: every public format; at d = 24 N odd, N = 2^nv, N = 1 and an upper half that is all
padding; N odd and more than one point per thread elsewhere."""
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
import sumcheck_paths as SP
from planes_decode import digits_of
from planes_pack import pack_coeffs, pack_digits
from test_gpu_sumcheck_paths import T, dev, host, lincomb_reference, table

pytestmark = pytest.mark.gpu
LF_ERR_INVALID_ARG, LF_ERR_UNSUPPORTED_RING = 1, 2  # lf.h
EDGE_COEFFS = np.array([(1 << 15) - 1, -(1 << 15) + 1, 1 << 14, -(1 << 14), 1, -1, 0])


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def case(d, N, nv, K=15, kind="uniform"):
    return dict(id=f"d{d}-N{N}-nv{nv}-K{K}-{kind}", d=d, N=N, nv=nv, K=K, kind=kind)


CASES = [case(24, N, nv) for nv in (3, 5) for N in (1, 7, 8, 25) if N <= 1 << nv]
CASES += [case(16, 9, 4), case(64, 17, 5), case(512, 3, 2), case(1024, 33, 6), case(4096, 5, 3)]
# a plane that is all zero (per-plane masks, and a magnitude bit no coefficient has)
CASES += [case(24, 7, 3, kind="zeroplane"), case(64, 17, 5, kind="zeroplane")]
# the sign on every plane at once
CASES += [case(16, 9, 4, kind="edges")]
# the same sign|magnitude words read with K = 3: the bits above plane 2 are not digits
CASES += [case(64, 17, 5, K=3, kind="words15")]
IDS = [c["id"] for c in CASES]
ZERO_PLANE = 4


def params(c):
    pr = LA.goldilocks_dp(c["d"])
    pr.K = c["K"]
    return pr


@functools.lru_cache(maxsize=None)
def build(cid):
    """both sides' planes, the digit rows [2][K][N][d] they stand for (canonical field
    elements) and the f_hat MLEs [2 K tau][2^nv d] of those rows; read only"""
    c = CASES[IDS.index(cid)]
    d, N, nv, K, kind = c["d"], c["N"], c["nv"], c["K"], c["kind"]
    rng = np.random.default_rng(1000 + 7 * d + 3 * N + nv + K)
    planes, digits = [], []
    for side in range(2):
        kmag = 15 if kind == "words15" else K
        x = rng.integers(-(1 << kmag) + 1, 1 << kmag, (N, d))
        if kind == "edges":
            x = EDGE_COEFFS[(np.arange(N * d) + side) % len(EDGE_COEFFS)].reshape(N, d)
        if kind == "zeroplane":
            x = np.sign(x) * (np.abs(x) & ~(1 << ZERO_PLANE))
        if d in (24, 4096) and side == 1 and kind == "uniform":
            # planes that are not the digits of one number (these formats keep every plane apart)
            dg = rng.integers(-1, 2, (K, N, d))
            planes.append(pack_digits(dg, d))
        else:
            dg = digits_of(x, K)
            planes.append(pack_coeffs(x, d, K))
        digits.append(dg)
    digits = np.stack(digits)
    if kind in ("uniform", "edges") and N * d >= 24:
        for v in (-1, 0, 1):  # every plane, plane K - 1 included, holds all three values
            assert (digits == v).any(axis=(2, 3)).all(), v
    if kind == "zeroplane":
        assert not digits[:, ZERO_PLANE].any() and digits[:, ZERO_PLANE + 1].any()
    rows = SP.to_field(digits)
    mles = np.concatenate([SP.fhat_mles(rows[s, k], N, d, nv) for s in range(2) for k in range(K)])
    return planes, rows, mles


def expand(ctx, c, planes):
    """lf_dev_expand_planes's f_coeff_k of one side, on the device"""
    out = dev(n=c["K"] * c["N"] * c["d"])
    ctx.dev_expand_planes(params(c), dev(planes), c["N"], out, None)
    return out


@pytest.mark.parametrize("cid", IDS)
def test_packed_planes_expand_to_their_rows(ctx, cid):
    c = CASES[IDS.index(cid)]
    planes, rows, _ = build(cid)
    for side in range(2):
        got = expand(ctx, c, planes[side])
        ctx.sync()
        assert np.array_equal(host(got), rows[side].ravel()), side


@pytest.mark.parametrize("cid", IDS)
def test_evaluate_planes_matches_oracle(ctx, cid):
    """out[k][j] = f_hat_(k, j)(r) for the K witnesses of each side, against the oracle's
    evaluation of the materialised MLEs; and the row entry on the expanded rows agrees"""
    c = CASES[IDS.index(cid)]
    d, N, nv, K = c["d"], c["N"], c["nv"], c["K"]
    planes, _, mles = build(cid)
    tau = SP.tb_of(d)
    r = table(nv * d, 11 + d + nv, "uniform")
    eq = dev(O.eq_table(r, nv, d))
    for side in range(2):
        want = np.concatenate([O.mle_evaluate(m, nv, d, r) for m in mles[side * K * tau:(side + 1) * K * tau]])
        out = dev(n=K * tau * d)
        ctx.dev_fhat_evaluate_planes(params(c), dev(planes[side]), N, nv, eq, out)
        ctx.sync()
        assert np.array_equal(host(out), want), side
        row = dev(n=K * tau * d)
        ctx.dev_fhat_evaluate_eq(d, expand(ctx, c, planes[side]), N, N * d, K, nv, eq, row)
        ctx.sync()
        assert np.array_equal(host(row), want), side


@pytest.mark.parametrize("cid", IDS)
def test_lincomb_planes_matches_integers(ctx, cid):
    """io[x] + sum_(k, j) coef[k tau + j] (.) fhat_(k, j)[x] from a nonzero io"""
    c = CASES[IDS.index(cid)]
    d, N, nv, K = c["d"], c["N"], c["nv"], c["K"]
    planes, _, mles = build(cid)
    tau, n, side = SP.tb_of(d), 1 << nv, 1
    coef = table(K * tau * d, 21 + d + nv, "uniform")
    io = table(n * d, 22 + d + nv, "uniform")
    want = lincomb_reference(io, mles[side * K * tau:(side + 1) * K * tau], coef, n, d)
    got = dev(io)
    ctx.dev_fhat_lincomb_planes(params(c), dev(planes[side]), N, nv, dev(coef), got)
    ctx.sync()
    assert np.array_equal(host(got), want)
    row = dev(io)
    ctx.dev_fhat_lincomb_digits(d, expand(ctx, c, planes[side]), N, N * d, K, nv, dev(coef), row)
    ctx.sync()
    assert np.array_equal(host(row), want)


@pytest.mark.parametrize("cid", IDS)
def test_prove_fold_planes_matches_oracle(ctx, cid):
    """the folding sumcheck on a fresh transcript: the oracle's proof and randomness over the
    five general MLEs and get_fhat of the digit rows; lf_sumcheck_prove_fold_digits on the
    expanded rows gives the same"""
    c = CASES[IDS.index(cid)]
    d, N, nv, K = c["d"], c["N"], c["nv"], c["K"]
    planes, _, fhat = build(cid)
    tau, n, nw = SP.tb_of(d), 1 << nv, 2 * K
    nm = 5 + nw * tau
    gen = np.concatenate([SP.rand(n * d, 31 + d + nv + i) for i in range(5)])
    mu = SP.rand(nw * d, 37 + d + nv)
    want = O.sumcheck_prove(O.new_transcript(), O.SumcheckComb.folding(mu, nw, tau, 2),
                            np.concatenate([gen, fhat.ravel()]), nm, nv, d, 4)
    comb = LA.Comb.folding(dev(mu), nw, tau, 2)
    work = dev(n=nm * max(n // 4, 1) * d)
    got = ctx.sumcheck_prove_fold_planes(T(), comb, dev(gen), params(c), dev(planes[0]), dev(planes[1]), N, nv, work)
    assert np.array_equal(got[0], want[0]), "proof"
    assert np.array_equal(got[1], want[1]), "randomness"
    row = ctx.sumcheck_prove_fold_digits(T(), comb, dev(gen), expand(ctx, c, planes[0]), expand(ctx, c, planes[1]), K,
                                         N, N * d, nv, d, work)
    assert np.array_equal(row[0], want[0]) and np.array_equal(row[1], want[1])


def bad_params(which):
    pr = LA.goldilocks_dp(2048 if which == "d2048" else 64)
    if which == "b_small4":
        pr.b_small, pr.K = 4, 8
    if which == "K16":
        pr.K = 16
    return pr


@pytest.mark.parametrize("which", ["d2048", "b_small4", "K16"])
def test_no_packed_form_is_unsupported_ring(ctx, which):
    """wherever lf_fold_step_planes_len is 0, as lf_dev_expand_planes"""
    pr = bad_params(which)
    assert LA.fold_step_planes_len(pr, 1) == 0
    d, nv = pr.d, 2
    tau, nw = 1, 2 * pr.K
    buf, one = dev(n=4 * d * 64), dev(n=nw * d)
    comb = LA.Comb.folding(one, nw, tau, 2)
    calls = [lambda: ctx.dev_fhat_evaluate_planes(pr, buf, 1, nv, buf, buf),
             lambda: ctx.dev_fhat_lincomb_planes(pr, buf, 1, nv, buf, buf),
             lambda: ctx.sumcheck_prove_fold_planes(T(), comb, buf, pr, buf, buf, 1, nv, buf)]
    for call in calls:
        with pytest.raises(LA.LfError) as e:
            call()
        assert e.value.code == LF_ERR_UNSUPPORTED_RING


def test_invalid_arguments(ctx):
    """N > 2^nv, and a combination that is not the folding kind over 2K witnesses"""
    pr = LA.goldilocks_dp(64)
    d, nv, K = 64, 2, pr.K
    buf = dev(n=8 * d * 64)
    for call in (lambda: ctx.dev_fhat_evaluate_planes(pr, buf, 5, nv, buf, buf),
                 lambda: ctx.dev_fhat_lincomb_planes(pr, buf, 5, nv, buf, buf),
                 lambda: ctx.sumcheck_prove_fold_planes(T(), LA.Comb.folding(buf, 2 * K, 1, 2), buf, pr, buf, buf, 5,
                                                        nv, buf),
                 lambda: ctx.sumcheck_prove_fold_planes(T(), LA.Comb.folding(buf, 2 * K - 1, 1, 2), buf, pr, buf, buf,
                                                        4, nv, buf),
                 lambda: ctx.sumcheck_prove_fold_planes(T(), LA.Comb.folding(buf, 2 * K, 1, 4), buf, pr, buf, buf, 4,
                                                        nv, buf)):
        with pytest.raises(LA.LfError) as e:
            call()
        assert e.value.code == LF_ERR_INVALID_ARG
