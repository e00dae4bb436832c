"""The contraction's chunk loop (k_ajtai_mfma_ra, ajtai_mfma.hip) at its seams.

A split of n chunks runs floor((n - DP) / DP) steady rounds of DP = 4 chunks (no
test per copy or per load; one loop per piece count 8 and 7) and then the tail
form for what is left, up to 2 DP - 1 chunks. A wave with another piece count
runs the tail form throughout. Every output equals the oracle bit for bit:
* split lengths 1, 2, 3, 4, 5, 7, 8, 9 (tail only; one steady round and each
  length of tail behind it), from the short splits mfma_cps makes below 256
  slots, and a 13-chunk split at d = 1024 whose last round is one chunk;
* plain commits of 1 .. 32 vectors: waves with 0, 1, 7 and 8 pieces;
* batched steps with dead-unit flags, the top-limb class on (9 top chunks, so
  its instance runs a steady round and a one-chunk last round) and off, two A
  tiles, a zero witness, and two calls on the same contexts."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from test_gpu_batch import expand, make_step
from test_gpu_parity import check_fold_outputs, params, rand

pytestmark = pytest.mark.gpu

DP, AJ_CPS = 4, 320


def nchunks(ncols):
    """frag_geom's chunk count (fragpos.hpp); Lp = 5 when 5 divides the columns (lf_api.hip ajtai_geom)"""
    Lp = 5 if ncols % 5 == 0 else 1
    nG = (ncols // Lp + 15) // 16
    ptop = 2 * ((nG * (Lp - 1) + 1) // 2) if Lp > 1 else 0
    return (ptop + 2 * ((nG + 1) // 2)) // 2, ptop // 2


def split_lengths(ncols, d):
    """the chunk counts of the splits of a single-class launch (mfma_cps, X^d + 1: d virtual slots)"""
    nch, _ = nchunks(ncols)
    if d >= 256:
        cps = AJ_CPS
    else:
        want = max(1024 // d, 1)
        cps = min(max((nch + want - 1) // want, 1), AJ_CPS)
    return sorted({min(cps, nch - c0) for c0 in range(0, nch, cps)})


# (d, columns) -> the split lengths it must produce
SPLIT_CASES = [(64, 4349, [1, 9]), (64, 3901, [2, 8]), (64, 3453, [3, 7]), (128, 1241, [4, 5]), (1024, 413, [13])]


def test_split_cases_cover_the_seams():
    got = set()
    for d, ncols, want in SPLIT_CASES:
        assert split_lengths(ncols, d) == want
        got |= set(want)
    assert {1, 2, 3, 4, 5, 7, 8, 9} <= got
    assert 13 % DP == 1 and 13 > 2 * DP  # steady rounds, then a last round of one chunk


def commit(ctx, d, ncols, kappa, nvec, seed):
    import torch
    A = rand(kappa * ncols * d, seed).reshape(kappa, ncols, d)
    sch = LA.AjtaiCommitmentScheme(ctx, A)
    F = rand(nvec * ncols * d, seed + 1)
    Ft = torch.from_numpy(F.view(np.int64)).cuda()
    cm = torch.zeros(nvec * kappa * d, dtype=torch.int64, device="cuda")
    ctx.dev_ajtai_commit(sch, [Ft[v * ncols * d:(v + 1) * ncols * d] for v in range(nvec)], cm)
    ctx.sync()
    want = O.ajtai_commit(A, kappa, ncols, d, F, nvec)
    assert np.array_equal(cm.cpu().numpy().view(np.uint64), want)


@pytest.fixture
def ctx():
    c = LA.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("d,ncols,lengths", SPLIT_CASES)
def test_commit_split_lengths(ctx, d, ncols, lengths):
    """29 vectors: wave 0 copies 8 pieces, the others 7 (both steady loops)"""
    assert split_lengths(ncols, d) == lengths
    commit(ctx, d, ncols, 3, 29, 500 + ncols)


@pytest.mark.parametrize("nvec", [1, 3, 4, 5, 28, 29, 32])
def test_commit_piece_counts(ctx, nvec):
    """splits of 9 chunks and of 1: pieces per wave (1,0,0,0) (1,1,1,0) (1,1,1,1)
    (2,1,1,1) (7,7,7,7) (8,7,7,7) (8,8,8,8)"""
    assert split_lengths(4349, 64) == [1, 9]
    commit(ctx, 64, 4349, 2, nvec, 700 + nvec)


BENCH, ZERO_W = "bench", "zero_w"
W_TOP = 257  # 17 groups: 34 full-class chunks, 9 top chunks
W_ONE = 70  # 5 groups: 13 chunks as one class


def test_step_geometries():
    assert nchunks(5 * W_TOP) == (43, 34) and nchunks(5 * W_ONE) == (13, 10)


def run_steps(d, W, kappa, kinds, rounds=1):
    import torch
    pr = params(d)
    assert pr.L == 5
    N = W * pr.L
    A = rand(kappa * N * d, 7300 + W)
    S = len(kinds)
    ctxs = [LA.Context(0) for _ in range(S)]
    try:
        At = torch.from_numpy(A.view(np.int64)).cuda()
        sch = LA.AjtaiCommitmentScheme(ctxs[0], device_tensor=At, kappa=kappa, ncols=N, d=d)
        for rnd in range(rounds):
            steps = [make_step(torch, A, kappa, d, W, 100 * rnd + 10 * i + 5, True, zero_w=kind == ZERO_W)
                     for i, kind in enumerate(kinds)]
            torch.cuda.synchronize()  # torch wrote the inputs on its own stream
            ctxs[0].dev_fold_step_batch(ctxs[1:], sch, pr, W, [st["b"] for st in steps])
            for c in ctxs:
                c.sync()
            h = lambda t: t.cpu().numpy().view(np.uint64)
            for st in steps:
                expand(ctxs[0], torch, pr, st["keep"], N, d)
                check_fold_outputs(h, st["keep"], A, kappa, d, pr, W, st["w_ccs"], st["acc_cm"], st["acc_fc"],
                                   st["rho"])
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("S", [2, 4])
def test_steps_top_class_on(monkeypatch, S):
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "1")
    run_steps(1024, W_TOP, 2, [BENCH] * S)


@pytest.mark.parametrize("S", [1, 2, 4])
def test_steps_top_class_off(monkeypatch, S):
    """one class of 13 chunks: two steady rounds, then tail rounds of 4 chunks and of 1"""
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "0")
    run_steps(1024, W_ONE, 2, [BENCH] * S)


def test_steps_two_a_tiles(monkeypatch):
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "1")
    run_steps(1024, W_TOP, 33, [BENCH] * 2)


def test_steps_zero_witness(monkeypatch):
    """a zero witness: its rows are dead on every unit"""
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "1")
    run_steps(1024, W_TOP, 2, [BENCH, ZERO_W])


def test_steps_two_calls_same_contexts(monkeypatch):
    """nothing in the F buffers or the masks carries over between calls"""
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "1")
    run_steps(1024, W_TOP, 2, [BENCH, ZERO_W], rounds=2)
