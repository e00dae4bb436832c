"""The d = 1024 fused decomposition's middle factors from stage 1's grouped byte sums
(kernels_n32.hip mid3_apply, gl::mul_mid3): inputs that drive the sums D_t of the matrix-core
stage 1 to their extremes, through a whole step against the oracle, every word of every output
(f_k where the step writes the rows, w_ccs_k, y of both sides and all K planes, and the rest of
tests/test_gpu_commit_planes.py's check_outputs).

Shapes: kappa = 2, L = 5, K = 15, W = 16 (one full block of 16 groups) and W = 17 (a second
block with one live half-wave), in the row-writing mode (fk given) and the packed mode.
Inputs, for both sides of the step:
  plus / minus  every digit of every plane +1 / -1: the accumulator's f_coeff at +-(2^15 - 1)
                (all 15 planes), the new witness's digits at +-(2^14 - 1) (planes 0..13; its
                top limb, a field element's, at +-7)
  alt           the same magnitudes with coefficient j = j1 + 32 j2 signed (-1)^j2, which
                lines every plane's digits up against the signs of the Z planes' columns
  uniform       seeded uniform w_ccs on both sides
The oracle's step of one (kind, W) is computed once and shared by both modes."""
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from test_gpu_commit_planes import KAPPA, check_outputs, make_bufs, make_scheme, signed
from test_gpu_parity import make_rho, oracle_fold_hot, params, rand, valid_f_coeff

pytestmark = pytest.mark.gpu
P = LA.P
d = 1024
KINDS = ["plus", "minus", "alt", "uniform"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def to_field(x):
    x = np.asarray(x, np.int64).ravel()
    return np.where(x < 0, np.uint64(P) - (-x).astype(np.uint64), x.astype(np.uint64))


def sign_pattern(kind):
    if kind == "plus":
        return np.ones(d, np.int64)
    if kind == "minus":
        return -np.ones(d, np.int64)
    return 1 - 2 * ((np.arange(d, dtype=np.int64) >> 5) & 1)  # (-1)^j2, j = j1 + 32 j2


def directed(kind, W):
    """(acc_fc, w_ccs) of a directed kind"""
    pr = params(d)
    L, K = pr.L, pr.K
    sg = sign_pattern(kind)
    acc = np.broadcast_to(sg * ((1 << K) - 1), (W, L, d))
    wfc = np.empty((W, L, d), np.int64)
    wfc[:, :L - 1] = sg * ((1 << (K - 1)) - 1)
    wfc[:, L - 1] = sg * 7
    _, w = O.witness_from_f(O.crt(to_field(wfc), d), d, pr.B, L)
    # the step's own from_w_ccs gives these digits back
    assert np.array_equal(signed(O.witness_from_w_ccs(w, d, pr.B, L)[0]).reshape(W, L, d), wfc)
    return to_field(acc), w


@functools.lru_cache(maxsize=None)
def reference(kind, W):
    """inputs and the oracle's step for one case (read-only, shared between the modes)"""
    pr = params(d)
    N = W * pr.L
    A = rand(KAPPA * N * d, 9700 + W)
    if kind == "uniform":
        acc_fc, w_ccs = valid_f_coeff(d, W, 9701 + W)[0], rand(W * d, 9702 + W)
    else:
        acc_fc, w_ccs = directed(kind, W)
    acc_cm = O.ajtai_commit(A, KAPPA, N, d, O.crt(acc_fc, d))
    rho = make_rho(d, pr.K, 9703)
    ofc, of = O.witness_from_w_ccs(w_ccs, d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, KAPPA, N, d, of)
    want, sides = oracle_fold_hot(A, KAPPA, d, pr, acc_cm, acc_fc, ocm, ofc, rho)
    want = dict(want, f_coeff=ofc, f=of, cm=ocm)
    if kind != "uniform":  # the planes are what the case says: no zero digit below the top limb's plane 3
        for s, top in ((0, pr.K), (1, pr.K - 1)):
            fck = signed(sides[s][0]).reshape(pr.K, W, pr.L, d)
            assert np.array_equal(fck[:top, :, :pr.L - 1], np.broadcast_to(sign_pattern(kind), (top, W, pr.L - 1, d)))
    ref = {"A": A, "w_ccs": w_ccs, "acc_fc": acc_fc, "acc_cm": acc_cm, "rho": rho, "want": want, "sides": sides}
    for v in (A, acc_cm, rho, *want.values(), *(x for s in sides for x in s)):
        v.setflags(write=False)
    return ref


@pytest.mark.parametrize("packed", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("W", [16, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_step_on_extreme_stage1_sums(ctx, kind, W, packed):
    import torch
    ref = reference(kind, W)
    sch = make_scheme(torch, ctx, ref, d, W)
    keep, b = make_bufs(torch, ref, d, W, packed)
    torch.cuda.synchronize()  # torch wrote the inputs on its own stream
    ctx.dev_fold_step(sch, params(d), W, b)
    ctx.sync()
    check_outputs(torch, ctx, ref, keep, d, W, packed)
