"""The batched contraction's top-limb chunk class (ajtai_mfma.hip): with two or more
steps the chunks of the top-limb units are contracted over a compacted list of the
(step, row) pairs that are live there, in tiles that mix rows of different steps.
Every output of every step equals the oracle's step bit for bit, whatever the
list holds: bench-like accumulators (7 live rows per step), dense ones (18), zero
witnesses and zero accumulators (an empty list), one or two paddings in the
order, two A tiles, the quarter-major slots of d = 4096, and the class switched
off."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from test_gpu_batch import expand, make_step
from test_gpu_parity import check_fold_outputs, params, rand

pytestmark = pytest.mark.gpu

BENCH, DENSE, ZERO_W, ZERO = "bench", "dense", "zero_w", "zero"


@pytest.fixture(autouse=True)
def class_on(monkeypatch):
    """By default the class is on only where the top chunks are worth its fixed launch
    costs (the bench shapes; test_gpu_scale.py runs those): =1 turns it on at these
    small shapes. The library reads the switch at every launch."""
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "1")


def dense_acc(d, W, L, seed):
    """an accumulator as after a real fold: every coefficient of every column
    uniform in [-2^14 + 1, 2^14 - 1], so every digit plane of every limb is live"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-(1 << 14) + 1, 1 << 14, W * L * d, dtype=np.int64)
    fc = np.where(x < 0, np.uint64(O.P) - (-x).astype(np.uint64), x.astype(np.uint64)).astype(np.uint64)
    return fc, O.crt(fc, d)


def set_acc(torch, st, A, kappa, d, N, fc, f):
    cm = O.ajtai_commit(A, kappa, N, d, f) if f.any() else np.zeros(kappa * d, np.uint64)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    # in place: the step buffers hold these tensors' addresses
    st["keep"]["acc_f_coeff"].copy_(dev(fc))
    st["keep"]["acc_cm"].copy_(dev(cm))
    st["acc_fc"], st["acc_cm"] = fc, cm


def run(d, W, kappa, kinds, rounds=1):
    import torch
    pr = params(d)
    N = W * pr.L
    A = rand(kappa * N * d, 7100 + d)
    S = len(kinds)
    ctxs = [LA.Context(0) for _ in range(S)]
    try:
        At = torch.from_numpy(A.view(np.int64)).cuda()
        sch = LA.AjtaiCommitmentScheme(ctxs[0], device_tensor=At, kappa=kappa, ncols=N, d=d)
        for rnd in range(rounds):
            steps = []
            for i, kind in enumerate(kinds):
                st = make_step(torch, A, kappa, d, W, 100 * rnd + 10 * i + 3, True, zero_w=kind in (ZERO_W, ZERO))
                if kind == DENSE:
                    set_acc(torch, st, A, kappa, d, N, *dense_acc(d, W, pr.L, 50 + 10 * rnd + i))
                elif kind == ZERO:
                    set_acc(torch, st, A, kappa, d, N, np.zeros(N * d, np.uint64), np.zeros(N * d, np.uint64))
                steps.append(st)
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


@pytest.mark.parametrize("S", [3, 8])
def test_top_class_three_groups(S):
    """nG = 3: two top chunks, one padding position, a partly filled last group;
    7 live rows per step, so the tiles straddle steps"""
    run(1024, 37, 2, [BENCH] * S)


def test_top_class_one_group():
    """nG = 1: a top chunk with one real half"""
    run(1024, 16, 2, [BENCH] * 2)


def test_top_class_two_groups_no_padding():
    run(1024, 32, 2, [BENCH] * 3)


def test_top_class_dense_accumulator():
    """18 live rows per step: 54 entries, two tiles, one step split across them"""
    run(1024, 37, 2, [DENSE] * 3)


def test_top_class_mixed_liveness():
    run(1024, 37, 2, [DENSE, BENCH, ZERO_W])


def test_top_class_empty_list():
    """zero witnesses and zero accumulators: no tile at all, the zeroed planes alone give the sums"""
    run(1024, 37, 2, [ZERO] * 3)


def test_top_class_two_a_tiles():
    run(1024, 37, 40, [BENCH] * 2)


@pytest.mark.parametrize("W", [17, 33])
def test_top_class_quarter_major_slots(W):
    run(4096, W, 2, [BENCH] * 2)


@pytest.mark.parametrize("S", [3, 8])
def test_top_class_off(monkeypatch, S):
    """LATTICEUM_AMD_TOPCLASS=0: the single-class path on the new operand order"""
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "0")
    run(1024, 37, 2, [BENCH] * S)


def test_top_class_two_batches_same_contexts():
    """the list and the zeroed planes are rebuilt per launch: a dense batch, then
    (other seeds) another on the same contexts"""
    run(1024, 37, 2, [DENSE, BENCH, ZERO_W], rounds=2)
