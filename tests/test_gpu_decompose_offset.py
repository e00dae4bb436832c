"""The d = 1024 fused decomposition's offset middle factors (kernels_n32.hip mid3_apply,
gl::mul_mid3_off): every value of a live body leaves the middle factors as y + gl::MID3_OFF and
the 32 offsets are taken off slot m2 = 0 after stage 2, once per lane. Whole steps against the
oracle, every word of every output (tests/test_gpu_commit_planes.py's check_outputs: f_k where
the step writes the rows, w_ccs_k, y of both sides and all K planes, and the rest), at the
shapes and inputs where that can go wrong and tests/test_gpu_decompose_mid.py does not reach.

Shapes: kappa = 2, L = 5, K = 15; W = 1 (one live half-wave, its partner reading group 0 into
the sink), W = 16 (one full block of 16 groups) and W = 17 (a second block with one live
half-wave); the row-writing mode (fk given) and the packed mode. A wave transforms column l of
groups 2 w and 2 w + 1 together, and a unit is column l of 16 consecutive groups.
Inputs, for both sides of the step (the accumulator's f_coeff directly, the new witness's
through the oracle's witness_from_f, whose digits the step's own from_w_ccs gives back):
  half     column l of group g all zero where g + l is even, seeded digits elsewhere: in every
           wave (W > 1) one element's planes are zero and the other's live, so the body is live
           and the zero element enters stage 2 as 32 copies of the offset alone
  unit     column 2 of groups 0..15 all zero and bit 3 of every digit of their column 1 clear:
           units dead on every plane and on one plane only (the dead path: no correction, the
           unit flagged), the rest live
  onecoef  groups 0..15 zero but for one coefficient of one group per column, with bits 0 and 2
           set: planes 0 and 2 are live through a single digit, every other plane dead
  row0     digits nonzero only at coefficients j = 32 j2 (j1 = 0): only the constant row of the
           middle factors contributes
  uniform  seeded uniform w_ccs on both sides
The oracle's step of one (kind, W) is computed once and shared by both modes."""
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from test_gpu_commit_planes import KAPPA, check_outputs, make_bufs, make_scheme, signed
from test_gpu_decompose_mid import to_field
from test_gpu_parity import make_rho, oracle_fold_hot, params, rand, valid_f_coeff

pytestmark = pytest.mark.gpu
P = LA.P
d = 1024
KINDS = ["half", "unit", "onecoef", "row0", "uniform"]
ONE_J = [0, 31, 32, 517, 1023]  # onecoef: the live coefficient of column l


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def one_group(W, l):
    return (5 * l + 3) % min(W, 16)


def digits(kind, W, side, seed):
    """(W, L, d) signed digits of one side: magnitudes below 2^15 (accumulator, all 15 planes)
    or 2^14 (new witness), the witness's top limb, a field element's, within +-7"""
    pr = params(d)
    L, K = pr.L, pr.K
    rng = np.random.default_rng(seed)
    top = (1 << (K - side)) - 1
    fc = rng.integers(-top, top + 1, size=(W, L, d), dtype=np.int64)
    if side == 1:
        fc[:, L - 1] = rng.integers(-7, 8, size=(W, d))
    g, l = np.meshgrid(np.arange(W), np.arange(L), indexing="ij")
    if kind == "half":
        fc[(g + l) % 2 == 0] = 0
    elif kind == "unit":
        fc[:16, 2] = 0
        fc[:16, 1] = np.sign(fc[:16, 1]) * (np.abs(fc[:16, 1]) & ~np.int64(8))
    elif kind == "onecoef":
        fc[:16] = 0
        for c in range(L):
            fc[one_group(W, c), c, ONE_J[c]] = 5 * (-1) ** c
    elif kind == "row0":
        fc[:, :, np.arange(d) % 32 != 0] = 0
    else:
        raise ValueError(kind)
    return fc


def assert_planes(kind, W, fck):
    """the decomposed planes (K, W, L, d) of one side are what the case says"""
    K, L = fck.shape[0], fck.shape[2]
    live = fck.any(axis=3)  # (K, W, L): plane k of column (g, l) has a digit
    g, l = np.meshgrid(np.arange(W), np.arange(L), indexing="ij")
    if kind == "half":
        zero = (g + l) % 2 == 0
        assert not live[:, zero].any() and live[:3][:, ~zero].all()
        if W > 1:  # every wave of a column pairs a zero element with a live one
            assert all(zero[2 * w, c] != zero[2 * w + 1, c] for w in range(W // 2) for c in range(L))
    elif kind == "unit":
        assert not live[:, :16, 2].any() and not live[3, :16, 1].any()
        assert live[:3, :16, 1].all() and live[:3][:, :, [0, 3, 4]].all() and live[:3, 16:].all()
    elif kind == "onecoef":
        want = np.zeros((K, min(W, 16), L, d), np.int64)
        for c in range(L):
            want[[0, 2], one_group(W, c), c, ONE_J[c]] = (-1) ** c
        assert np.array_equal(fck[:, :16], want) and live[:3, 16:].all()
    elif kind == "row0":
        assert not fck[..., np.arange(d) % 32 != 0].any() and live[:3].all()


def directed(kind, W):
    """(acc_fc, w_ccs) of a directed kind"""
    pr = params(d)
    acc, wfc = digits(kind, W, 0, 9800 + W), digits(kind, W, 1, 9810 + W)
    _, w = O.witness_from_f(O.crt(to_field(wfc), d), d, pr.B, pr.L)
    # the step's own from_w_ccs gives these digits back
    assert np.array_equal(signed(O.witness_from_w_ccs(w, d, pr.B, pr.L)[0]).reshape(W, pr.L, d), wfc)
    return to_field(acc), w


@functools.lru_cache(maxsize=None)
def reference(kind, W):
    """inputs and the oracle's step for one case (read-only, shared between the modes)"""
    pr = params(d)
    N = W * pr.L
    A = rand(KAPPA * N * d, 9820 + W)
    if kind == "uniform":
        acc_fc, w_ccs = valid_f_coeff(d, W, 9821 + W)[0], rand(W * d, 9822 + W)
    else:
        acc_fc, w_ccs = directed(kind, W)
    acc_cm = O.ajtai_commit(A, KAPPA, N, d, O.crt(acc_fc, d))
    rho = make_rho(d, pr.K, 9823)
    ofc, of = O.witness_from_w_ccs(w_ccs, d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, KAPPA, N, d, of)
    want, sides = oracle_fold_hot(A, KAPPA, d, pr, acc_cm, acc_fc, ocm, ofc, rho)
    want = dict(want, f_coeff=ofc, f=of, cm=ocm)
    for s in range(2):
        assert_planes(kind, W, signed(sides[s][0]).reshape(pr.K, W, pr.L, d))
    ref = {"A": A, "w_ccs": w_ccs, "acc_fc": acc_fc, "acc_cm": acc_cm, "rho": rho, "want": want, "sides": sides}
    for v in (A, acc_cm, rho, *want.values(), *(x for s in sides for x in s)):
        v.setflags(write=False)
    return ref


@pytest.mark.parametrize("packed", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("W", [1, 16, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_step_with_offset_middle_factors(ctx, kind, W, packed):
    import torch
    ref = reference(kind, W)
    sch = make_scheme(torch, ctx, ref, d, W)
    keep, b = make_bufs(torch, ref, d, W, packed)
    torch.cuda.synchronize()  # torch wrote the inputs on its own stream
    ctx.dev_fold_step(sch, params(d), W, b)
    ctx.sync()
    check_outputs(torch, ctx, ref, keep, d, W, packed)
