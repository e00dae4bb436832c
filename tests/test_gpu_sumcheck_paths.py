"""Every sumcheck kernel instantiation and launch path against the oracle, bit for bit.

The cases are the table of tests/sumcheck_paths.py, whose census (tests/
test_sumcheck_paths.py, on the CPU) shows that they reach every path: each slot width, every
degree / NQ / B_SMALL template, the chunked, unevenly chunked, unchunked and capped launches,
both sides of the per-point threshold, the sparse round 0's block shapes, the digit round 0
at the edges of its rows, and the three splits of the dot products. Every comparison is
np.array_equal against oracle/ or plain Python integers mod p; a proof that differs is
reported by its first differing round and that round's plan."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
import sumcheck_paths as SP
from gl_model import edge_values

pytestmark = pytest.mark.gpu
P = LA.P


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def dev(x=None, n=None):
    import torch
    if x is not None:
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def dev32(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def ids(cases):
    return [c["id"] for c in cases]


def T():
    return LA.Poseidon2Transcript()


def assert_proof(got, want, pls, nev, d):
    got_p, got_r = got
    want_p, want_r = want
    msg = SP.first_difference(got_p, want_p, pls, nev, d)
    assert msg is None, msg
    assert np.array_equal(got_r, want_r)


def point_of(rnd, nv, d):
    tb = SP.tb_of(d)
    return np.concatenate([O.broadcast(rnd[i * tb:(i + 1) * tb], d) for i in range(nv)])


# ------------------------------------------------------------------ A. the split-eq provers
def lin_reference(case, sparse):
    """the inputs, the oracle's proof over [mz..., eq(beta)] and the MLEs at its challenge point"""
    d, nv, degree = case["d"], case["nv"], case["degree"]
    c, S, mz, beta = SP.lin_inputs(case)
    act = off = None
    if sparse:
        live, act, off = SP.sparse_lists(case)
        for m, on in zip(mz, live):
            m.reshape(1 << (nv - 1), 2 * d)[~on] = 0
    mles = np.concatenate(mz + [O.eq_table(beta, nv, d)])
    want = O.sumcheck_prove(O.new_transcript(), O.SumcheckComb.linearization(c, S), mles, len(mz) + 1, nv, d, degree)
    point = point_of(want[1], nv, d)
    evals = np.concatenate([O.mle_evaluate(m, nv, d, point) for m in mz])
    return c, S, mz, beta, mles, want, evals, act, off


def lin_work(nmz, nv, d):
    return dev(n=max(1, nmz * (1 << max(nv - 2, 0)) * d))


@pytest.mark.parametrize("case", SP.LIN_EQ_CASES, ids=ids(SP.LIN_EQ_CASES))
def test_prove_lin_matches_oracle(ctx, case):
    """lf_sumcheck_prove_lin: k_round_lin_eq<TB, NQ> above the per-point threshold, then
    k_round_lin_eq_pt; proof, randomness and the MLEs' final values"""
    d, nv, degree = case["d"], case["nv"], case["degree"]
    c, S, mz, beta, _, want, want_ev, _, _ = lin_reference(case, sparse=False)
    evals = dev(n=len(mz) * d)
    got = ctx.sumcheck_prove_lin(T(), LA.Comb.linearization(dev(c), S), [dev(m) for m in mz], nv, d, degree, beta,
                                 lin_work(len(mz), nv, d), evals)
    assert_proof(got, want, SP.plans(case, SP.LIN_EQ), degree + 1, d)
    ctx.sync()
    assert np.array_equal(host(evals), want_ev)


@pytest.mark.parametrize("case", SP.SPARSE_CASES, ids=ids(SP.SPARSE_CASES))
def test_prove_lin_sparse_matches_oracle(ctx, case):
    """lf_sumcheck_prove_lin_sparse over MLEs with about 30 % of their lines zeroed: round 0 in
    k_round_lin_eq_sparse<TB, NQ> over each multiset's active points (none at all in the dead
    cases: the zero message)"""
    d, nv, degree = case["d"], case["nv"], case["degree"]
    c, S, mz, beta, _, want, want_ev, act, off = lin_reference(case, sparse=True)
    evals = dev(n=len(mz) * d)
    got = ctx.sumcheck_prove_lin_sparse(T(), LA.Comb.linearization(dev(c), S), [dev(m) for m in mz], nv, d, degree,
                                        beta, dev32(act), off, lin_work(len(mz), nv, d), evals)
    assert_proof(got, want, SP.plans(case, SP.LIN_EQ), degree + 1, d)
    ctx.sync()
    assert np.array_equal(host(evals), want_ev)


# ------------------------------------------------------------------ B. the unsplit linearization
@pytest.mark.parametrize("case", SP.LIN_ROUNDS, ids=ids(SP.LIN_ROUNDS))
def test_lin_round_matches_oracle(ctx, case):
    """lf_dev_sumcheck_round: k_round_lin<TB, DEG> at every degree, one multiset, and the capped launch"""
    d, nv, degree = case["d"], case["nv"], case["degree"]
    c, S, mz, beta = SP.lin_inputs(case)
    mles = np.concatenate(mz + [O.eq_table(beta, nv, d)])
    nm = len(mz) + 1
    want = O.sumcheck_round(O.SumcheckComb.linearization(c, S), mles, nm, nv, d, degree)
    ev = dev(n=(degree + 1) * d)
    ctx.dev_sumcheck_round(LA.Comb.linearization(dev(c), S), dev(mles), (1 << nv) * d, nm, nv, d, degree, ev)
    ctx.sync()
    assert np.array_equal(host(ev), want), SP.plans(case, SP.LIN)[0]


@pytest.mark.parametrize("case", SP.LIN_PROVES, ids=ids(SP.LIN_PROVES))
def test_lin_prove_and_prove_ptrs_match_oracle(ctx, case):
    """lf_sumcheck_prove over one buffer and lf_sumcheck_prove_ptrs over MLEs in separate
    allocations give the oracle's proof down the chunk ladder and under the grid.x cap"""
    d, nv, degree = case["d"], case["nv"], case["degree"]
    c, S, mz, beta, mles, want, _, _, _ = lin_reference(case, sparse=False)
    nm, pls = len(mz) + 1, SP.plans(case, SP.LIN)
    comb = LA.Comb.linearization(dev(c), S)
    got = ctx.sumcheck_prove(T(), comb, dev(mles), nm, nv, d, degree)
    assert_proof(got, want, pls, degree + 1, d)
    n = 1 << nv
    # separate allocations of different sizes, so the MLEs are not one stride apart
    bufs = [dev(np.concatenate([mles[m * n * d:(m + 1) * n * d], np.zeros((m + 1) * 64, np.uint64)])) for m in range(nm)]
    keep = [b.clone() for b in bufs]
    got = ctx.sumcheck_prove_ptrs(T(), comb, [b[:n * d] for b in bufs], nv, d, degree, lin_work(nm, nv, d))
    assert_proof(got, want, pls, degree + 1, d)
    ctx.sync()
    assert all(bool((a == b).all()) for a, b in zip(bufs, keep))  # read in place, never written


# ------------------------------------------------------------------ C. the folding polynomial
@pytest.mark.parametrize("case", SP.FOLD_ROUNDS, ids=ids(SP.FOLD_ROUNDS))
def test_folding_round_matches_oracle(ctx, case):
    """k_round_folding<TB, BS> at every B_SMALL (the cubic form at 2, the finite-difference
    extrapolation at 1, 3 and 4), and the capped Phi_72 launch at 17 variables"""
    d, nv, nk, tau, bs = (case[k] for k in ("d", "nv", "nk", "tau", "bs"))
    mles, mu, nm = SP.fold_inputs(case)
    want = O.sumcheck_round(O.SumcheckComb.folding(mu, nk, tau, bs), mles, nm, nv, d, 2 * bs)
    ev = dev(n=(2 * bs + 1) * d)
    ctx.dev_sumcheck_round(LA.Comb.folding(dev(mu), nk, tau, bs), dev(mles), (1 << nv) * d, nm, nv, d, 2 * bs, ev)
    ctx.sync()
    assert np.array_equal(host(ev), want), SP.plans(case, SP.FOLD)[0]


@pytest.mark.parametrize("case", SP.FOLD_PROVES, ids=ids(SP.FOLD_PROVES))
def test_folding_prove_matches_oracle(ctx, case):
    d, nv, nk, tau, bs = (case[k] for k in ("d", "nv", "nk", "tau", "bs"))
    mles, mu, nm = SP.fold_inputs(case)
    want = O.sumcheck_prove(O.new_transcript(), O.SumcheckComb.folding(mu, nk, tau, bs), mles, nm, nv, d, 2 * bs)
    got = ctx.sumcheck_prove(T(), LA.Comb.folding(dev(mu), nk, tau, bs), dev(mles), nm, nv, d, 2 * bs)
    assert_proof(got, want, SP.plans(case, SP.FOLD), 2 * bs + 1, d)


# ------------------------------------------------------------------ D. the digit round 0
@pytest.mark.parametrize("case", SP.DIGIT_CASES, ids=ids(SP.DIGIT_CASES))
def test_prove_fold_digits_matches_oracle(ctx, case):
    """lf_sumcheck_prove_fold_digits against the oracle's proof over MLEs built on the CPU: the
    five general ones and get_fhat of the digit rows (the rows themselves for X^d + 1), zero past
    N. The gap between the witnesses' rows holds no digits: reading it would show."""
    d, nv, K, N, gap = (case[k] for k in ("d", "nv", "K", "N", "gap"))
    tau, n, nw = SP.tb_of(d), 1 << nv, 2 * K
    rows = SP.digit_rows(case)
    mu = SP.digit_mu(case)
    gen = np.concatenate([SP.rand(n * d, case["seed"] + 20 + i) for i in range(5)])
    mles = np.concatenate([gen] + [SP.fhat_mles(rows[w], N, d, nv).ravel() for w in range(nw)])
    nm = 5 + nw * tau
    want = O.sumcheck_prove(O.new_transcript(), O.SumcheckComb.folding(mu, nw, tau, 2), mles, nm, nv, d, 4)
    wstride = N * d + gap
    sides = []
    for side in range(2):
        buf = SP.rand(K * wstride, case["seed"] + 40 + side)  # not digits: only the rows are overwritten
        for k in range(K):
            buf[k * wstride:k * wstride + N * d] = rows[side * K + k].ravel()
        sides.append(dev(buf))
    work = dev(n=nm * max(n // 4, 1) * d)
    got = ctx.sumcheck_prove_fold_digits(T(), LA.Comb.folding(dev(mu), nw, tau, 2), dev(gen), sides[0], sides[1], K, N,
                                         wstride, nv, d, work)
    assert_proof(got, want, SP.digit_plans(case), 5, d)


# ------------------------------------------------------------------ E. evaluation and combination
def table(n, seed, fill):
    """n words: uniform, or cyclically the directed edge values of the field arithmetic"""
    if fill == "uniform":
        return SP.rand(n, seed)
    edges = np.array(edge_values()[0], np.uint64)
    return edges[(np.arange(n) + seed) % len(edges)]


def mul_rows(rows, elem, d):
    """rows [n][d] times one ring element, slot by slot: plain integers mod p for X^d + 1, the
    oracle's slot product for Phi_72"""
    if d == 24:
        return np.stack([O.slot_mul(r, elem, d) for r in rows])
    return ((rows.astype(object) * elem.astype(object)[None, :]) % P).astype(np.uint64)


def add_rows(a, b):
    return ((a.astype(object) + b.astype(object)) % P).astype(np.uint64)


def n_of(kind, n):
    return {"zero": 0, "odd": max(1, n - 3) | 1 if n > 2 else 1, "full": n}[kind]


FILLS = [("uniform", s) for s in SP.DOT_SHAPES] + [("edges", (24, 8)), ("edges", (64, 6))]
FILL_IDS = [f"{f}-d{d}-nv{nv}" for f, (d, nv) in FILLS]


@pytest.mark.parametrize("fill,shape", FILLS, ids=FILL_IDS)
def test_mle_evaluate_entries_match_oracle(ctx, fill, shape):
    """lf_dev_mle_evaluate and lf_dev_mle_evaluate_eq (k_mle_dot at each split of the points)"""
    d, nv = shape
    n, nm = 1 << nv, 3
    mles = table(nm * n * d, 70 + d + nv, fill)
    r = table(nv * d, 71 + d + nv, fill)
    want = np.concatenate([O.mle_evaluate(mles[m * n * d:(m + 1) * n * d], nv, d, r) for m in range(nm)])
    pl = LA.sumcheck_dot_plan(d, n)
    out = dev(n=nm * d)
    ctx.dev_mle_evaluate(d, dev(mles), nm, nv, dev(r), out)
    ctx.sync()
    assert np.array_equal(host(out), want), pl
    out = dev(n=nm * d)
    ctx.dev_mle_evaluate_eq(d, dev(mles), nm, nv, dev(O.eq_table(r, nv, d)), out)
    ctx.sync()
    assert np.array_equal(host(out), want), pl


FHAT_EDGES = [("zero", 1, 0), ("odd", 3, 0), ("full", 1, 5), ("odd", 3, 29), ("full", 3, 0)]


def fhat_case(d, nv, nkind, nw, pad, fill, seed, digits=False):
    """nw witnesses' rows wstride apart in a buffer whose gaps hold other values, and their
    f_hat MLEs [nw tau][2^nv d]"""
    n = 1 << nv
    N = n_of(nkind, n)
    wstride = N * d + pad
    if digits:
        rows = SP.to_field(np.random.default_rng(seed).integers(-1, 2, (nw, N, d)))
    else:
        rows = table(nw * N * d, seed, fill).reshape(nw, N, d)
    buf = SP.rand(max(1, nw * wstride), seed + 1)
    for w in range(nw):
        buf[w * wstride:w * wstride + N * d] = rows[w].ravel()
    mles = np.concatenate([SP.fhat_mles(rows[w], N, d, nv) for w in range(nw)])
    return N, wstride, buf, mles


@pytest.mark.parametrize("nkind,nw,pad", FHAT_EDGES, ids=[f"N{k}-nw{w}-pad{p}" for k, w, p in FHAT_EDGES])
@pytest.mark.parametrize("fill,shape", FILLS, ids=FILL_IDS)
def test_fhat_evaluate_entries_match_oracle(ctx, fill, shape, nkind, nw, pad):
    """lf_dev_fhat_evaluate and lf_dev_fhat_evaluate_eq (k_fhat_dot) against the oracle's
    evaluation of the materialised f_hat MLEs: N = 0, odd and 2^nv, one and three witnesses,
    rows at the default stride and apart"""
    d, nv = shape
    N, wstride, buf, mles = fhat_case(d, nv, nkind, nw, pad, fill, 80 + d + nv + nw)
    r = table(nv * d, 81 + d + nv, fill)
    want = np.concatenate([O.mle_evaluate(m, nv, d, r) for m in mles])
    pl = LA.sumcheck_dot_plan(d, 1 << nv)
    out = dev(n=len(mles) * d)
    ctx.dev_fhat_evaluate(d, dev(buf), N, wstride if pad else 0, nw, nv, dev(r), out)
    ctx.sync()
    assert np.array_equal(host(out), want), pl
    out = dev(n=len(mles) * d)
    ctx.dev_fhat_evaluate_eq(d, dev(buf), N, wstride if pad else 0, nw, nv, dev(O.eq_table(r, nv, d)), out)
    ctx.sync()
    assert np.array_equal(host(out), want), pl


def lincomb_reference(io, mles, coef, n, d):
    want = io.reshape(n, d)
    for m, cf in zip(mles, coef.reshape(-1, d)):
        want = add_rows(want, mul_rows(m.reshape(n, d), cf, d))
    return want.ravel()


@pytest.mark.parametrize("pad", [0, 40])
@pytest.mark.parametrize("fill,shape", FILLS, ids=FILL_IDS)
def test_mle_lincomb_matches_integers(ctx, fill, shape, pad):
    """lf_dev_mle_lincomb from a non-zero io: io[x] + sum_m coef[m] (.) mles[m][x]"""
    d, nv = shape
    n, nm = 1 << nv, 3
    stride = n * d + pad
    buf = table(nm * stride, 90 + d + nv, fill)
    mles = [buf[m * stride:m * stride + n * d] for m in range(nm)]
    coef = table(nm * d, 91 + d + nv, fill)
    io = table(n * d, 92 + d + nv, fill)
    want = lincomb_reference(io, mles, coef, n, d)
    got = dev(io)
    ctx.dev_mle_lincomb(d, dev(buf), stride if pad else 0, nm, nv, dev(coef), got)
    ctx.sync()
    assert np.array_equal(host(got), want)


@pytest.mark.parametrize("nkind,nw,pad", FHAT_EDGES, ids=[f"N{k}-nw{w}-pad{p}" for k, w, p in FHAT_EDGES])
@pytest.mark.parametrize("fill,shape", FILLS, ids=FILL_IDS)
def test_fhat_lincomb_digits_matches_integers(ctx, fill, shape, nkind, nw, pad):
    """lf_dev_fhat_lincomb_digits (k_fhat_lincomb_digits) from a non-zero io, over digit rows"""
    d, nv = shape
    n = 1 << nv
    N, wstride, buf, mles = fhat_case(d, nv, nkind, nw, pad, fill, 95 + d + nv + nw, digits=True)
    coef = table(len(mles) * d, 96 + d + nv, fill)
    io = table(n * d, 97 + d + nv, fill)
    want = lincomb_reference(io, mles, coef, n, d)
    got = dev(io)
    ctx.dev_fhat_lincomb_digits(d, dev(buf), N, wstride if pad else 0, nw, nv, dev(coef), got)
    ctx.sync()
    assert np.array_equal(host(got), want)
