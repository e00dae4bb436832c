"""The coefficient-form folds at the edges of their short-rho range (fold_coeff.hip at
d = 1024: |coefficient| <= 127 on the i8 matrix cores; fold.hip's Phi_72 fold at d = 24:
<= 32 on packed 16-bit lanes). The cases are tests/fold_rho_edges.py's, whose properties
tests/test_fold_rho_edges.py checks on the CPU: rho over the whole accepted range and at
its ends, sums that reach the attainable bound 2 * 14 * d * bound of the i32 / i16
accumulators, a top limb that is live on one tile only, and a single coefficient of a
single rho_i one past the bound. Every output of the step is compared with the oracle's
bit for bit, and lf_ctx_fold_flag says which fold ran: a parity test alone cannot, since
the NTT-form fallback gives the same answer. The oracle's step of a case is computed once."""
import functools

import numpy as np
import pytest

import fold_rho_edges as E
import latticeum_amd as LA
import oracle as O
from test_gpu_commit_planes import check_outputs, make_bufs, make_scheme
from test_gpu_parity import oracle_fold_hot, params, rand

pytestmark = pytest.mark.gpu

# d = 1024, W = 2: N = 10, fewer tiles than block slots, so the witness-split partials
# (ks_n > 1); W = 33: a ragged second 32-group tile. d = 24, W = 13 crosses the 12-group
# block of k_fold_coeff_phi72. packed: Coeff1024Rows / Masks24Packed, rows: Coeff1024 / Masks24
SHAPES = [(1024, 2), (1024, 33), (24, 3), (24, 13)]
MODES = [True, False]
mode_id = lambda p: "packed" if p else "rows"


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def matrix(d, W):
    A = rand(E.KAPPA[d] * W * params(d).L * d, 9100 + d + W)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def reference(kind, d, W, *args):
    """the case's inputs and the oracle's step (read-only, shared between tests)"""
    pr = params(d)
    kappa, N = E.KAPPA[d], W * pr.L
    case = E.build(kind, d, W, *args)
    A = matrix(d, W)
    acc_fc = case["acc_fc"]
    acc_cm = O.ajtai_commit(A, kappa, N, d, O.crt(acc_fc, d))
    ofc, of = O.witness_from_w_ccs(case["w_ccs"], d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, kappa, N, d, of)
    want, sides = oracle_fold_hot(A, kappa, d, pr, acc_cm, acc_fc, ocm, ofc, case["rho"])
    want = dict(want, f_coeff=ofc, f=of, cm=ocm)
    ref = {"A": A, "w_ccs": case["w_ccs"], "acc_fc": acc_fc, "acc_cm": acc_cm, "rho": case["rho"], "want": want,
           "sides": sides, "case": case}
    for v in (acc_cm, *want.values(), *(x for s in sides for x in s)):
        v.setflags(write=False)
    return ref


def run(c, flag, kind, d, W, packed, *args):
    """one step of the case on c: every output is the oracle's and the step judged rho as `flag` says"""
    import torch
    ref = reference(kind, d, W, *args)
    kappa = E.KAPPA[d]
    sch = make_scheme(torch, c, ref, d, W, kappa)
    keep, b = make_bufs(torch, ref, d, W, packed, kappa)
    torch.cuda.synchronize()  # torch wrote the inputs on its own stream
    c.dev_fold_step(sch, params(d), W, b)
    got = c.fold_flag()
    c.sync()
    check_outputs(torch, c, ref, keep, d, W, packed, kappa)
    assert got == flag, f"fold flag {got}"
    return ref


def f0_coeff(ref, d):
    return E.signed(ref["want"]["f0_coeff"]).reshape(-1, d)


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("d,W", SHAPES)
def test_mid_range_rho(ctx, d, W, packed):
    """coefficients over all of [-bound, bound], both ends in every rho_i: at d = 1024 the i8
    extremes and the negated half of the byte table, at d = 24 the +32 short_challenge never gives"""
    run(ctx, 0, "mid", d, W, packed)


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("d,W", SHAPES)
def test_all_extreme_rho(ctx, d, W, packed):
    """every coefficient +-bound, on witnesses whose digits reach +-2^14 (plane K - 1 live)"""
    run(ctx, 0, "extreme", d, W, packed)


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("c_star", [0, 511, 1023])  # the all-wrapped row, a mixed row, the unwrapped row
@pytest.mark.parametrize("W,g_star", [(2, 0), (33, 32)])  # W = 33: the target in the ragged tile
def test_worst_case_sum_1024(ctx, W, g_star, c_star, packed):
    """an i32 accumulator (and its ks_n > 1 partials at W = 2) at the attainable bound"""
    d = 1024
    ref = run(ctx, 0, "worst", d, W, packed, g_star, c_star)
    e, c = ref["case"]["target"]
    assert (e // 5, c) == (g_star, c_star)
    assert f0_coeff(ref, d)[e, c] == E.worst_sum(d) == 3_641_344


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("W", [3, 13])
def test_worst_case_sum_24(ctx, W, packed):
    """a 16-bit lane (and the quad's shuffle-sum) at 21 504 > 2^14, at index 23 of the
    degree-46 product; the oracle's reduced element is that product's reduction"""
    d = 24
    ref = run(ctx, 0, "worst", d, W, packed, W - 1, 23)
    case = ref["case"]
    e, _ = case["target"]
    D, _ = E.planes(case, d)
    pre = E.conv_sum(case, D, e)
    assert pre[23] == E.worst_sum(d) == 21_504
    assert [int(x) for x in f0_coeff(ref, d)[e]] == E.reduce_phi72(pre)


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("W,g_live", [(2, 1), (33, 32)])
def test_top_limb_live_on_one_tile(ctx, W, g_live, packed):
    """the data-driven plane skips of k_fold_coeff: planes 4..13 of the top limb live in one
    group of the accumulator only, dead in the new witness"""
    run(ctx, 0, "top", 1024, W, packed, g_live)


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("d,W,out", [(1024, 2, o) for o in E.OUT_1024]
                         + [(1024, 33, E.OUT_1024[0]), (1024, 33, E.OUT_1024[-1])]
                         + [(24, 3, o) for o in E.OUT_24] + [(24, 13, E.OUT_24[0]), (24, 13, E.OUT_24[-1])])
def test_one_coefficient_out(ctx, d, W, out, packed):
    """a single coefficient of a single rho_i at +-(bound + 1) (a negative one stored as
    p - (bound + 1), next to accepted p - bound): the flag is raised from that block alone and
    the fallback's outputs are exact"""
    run(ctx, 1, "out", d, W, packed, *out)


@pytest.mark.parametrize("d,W,outs", [(1024, 2, (E.OUT_1024[0], E.OUT_1024[-1])), (24, 3, (E.OUT_24[0], E.OUT_24[-1]))])
def test_flag_is_reset_every_step(d, W, outs):
    """out, short, out again on one context: no step sees the previous step's flag or sync words"""
    c = LA.Context(0)
    try:
        import torch
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        assert c.fold_flag() == -1  # no step yet
        run(c, 1, "out", d, W, True, *outs[0])
        run(c, 0, "mid", d, W, True)
        run(c, 1, "out", d, W, True, *outs[1])
        run(c, 0, "extreme", d, W, True)
    finally:
        c.close()


def test_path_without_a_flag(ctx):
    """the other degrees fold their f_k rows in NTT form (FoldPath::Ntt): no short-rho path, so
    -1 even after a step on the same context that had a flag"""
    import torch
    run(ctx, 0, "mid", 24, 3, False)
    d, W, kappa = 256, 2, 2
    pr = params(d)
    N = W * pr.L
    A = rand(kappa * N * d, 9200)
    acc_fc, acc_f = O.witness_from_w_ccs(rand(W * d, 9201), d, pr.B, pr.L)
    acc_cm = O.ajtai_commit(A, kappa, N, d, acc_f)
    w_ccs, rho = rand(W * d, 9202), rand(2 * pr.K * d, 9203)
    ofc, of = O.witness_from_w_ccs(w_ccs, d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, kappa, N, d, of)
    want, sides = oracle_fold_hot(A, kappa, d, pr, acc_cm, acc_fc, ocm, ofc, rho)
    ref = {"A": A, "w_ccs": w_ccs, "acc_fc": acc_fc, "acc_cm": acc_cm, "rho": rho,
           "want": dict(want, f_coeff=ofc, f=of, cm=ocm), "sides": sides}
    sch = make_scheme(torch, ctx, ref, d, W, kappa)
    keep, b = make_bufs(torch, ref, d, W, False, kappa)
    torch.cuda.synchronize()
    ctx.dev_fold_step(sch, pr, W, b)
    assert ctx.fold_flag() == -1
    ctx.sync()
    check_outputs(torch, ctx, ref, keep, d, W, False, kappa)


def test_batch_flags_are_per_step(ctx):
    """two packed steps in one batch, all-extreme rho and one coefficient out: each context
    reports its own step's flag and both steps are the oracle's"""
    import torch
    d, W = 1024, 17
    pr = params(d)
    refs = [reference("extreme", d, W), reference("out", d, W, *E.OUT_1024[-1])]
    other = LA.Context(0)
    try:
        sch = make_scheme(torch, ctx, refs[0], d, W)
        steps = [make_bufs(torch, r, d, W, True) for r in refs]
        torch.cuda.synchronize()
        ctx.dev_fold_step_batch([other], sch, pr, W, [b for _, b in steps])
        flags = [ctx.fold_flag(), other.fold_flag()]
        ctx.sync()
        other.sync()
        for r, (keep, _) in zip(refs, steps):
            check_outputs(torch, ctx, r, keep, d, W, True)
        assert flags == [0, 1]
    finally:
        other.close()
