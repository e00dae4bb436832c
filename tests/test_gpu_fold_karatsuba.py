"""The Karatsuba levels of the d = 1024 coefficient-form fold (fold_coeff.hip) on the device:
every output of a step is the oracle's bit for bit at whichever level ran, and
lf_ctx_fold_level says which one did. Short rho as the benchmark makes it, rho at the edge
of each level's i8 range (tests/fold_karatsuba.py, whose algebra tests/
test_fold_karatsuba_model.py checks on the CPU), and the plane-skip and accumulator-bound
cases of tests/fold_rho_edges.py under rho short enough for the split. Each case runs at the
default level and again under LATTICEUM_AMD_FOLD_KARA=0 and =1 on fresh contexts. The
oracle's step of a case is computed once."""
import functools

import numpy as np
import pytest

import fold_karatsuba as KM
import fold_rho_edges as E
import latticeum_amd as LA
import oracle as O
from test_gpu_commit_planes import check_outputs, make_bufs, make_scheme
from test_gpu_fold_rho_edges import matrix
from test_gpu_parity import oracle_fold_hot, params

pytestmark = pytest.mark.gpu

d = 1024
BEST = 1  # the highest level fold_coeff.hip builds
NW = 2 * params(d).K
# W = 2: N = 10, the witness-split partials (ks_n > 1) and one block pair with an idle half;
# W = 33: a ragged second tile, an odd tile count
SHAPES = [2, 33]
MODES = [True, False]
mode_id = lambda p: "packed" if p else "rows"
G_STAR = {2: 0, 33: 32}
G_LIVE = {2: 1, 33: 32}
WORST_BOUND = 63  # the largest |coefficient| level 1 always takes


def bench_rho(seed):
    """2K - 1 short challenges and ONE, as bench.py and get_rhos make them (signed coefficients)"""
    rng = np.random.default_rng(seed)
    rc = [E.signed(O.short_challenge(rng.integers(0, 256, 3 * d // 4, dtype=np.uint8).tobytes(), d))
          for _ in range(NW - 1)]
    one = np.zeros(d, np.int64)
    one[0] = 1
    return np.stack(rc + [one])


@functools.lru_cache(maxsize=None)
def case_of(kind, W):
    seed = 9500 + 16 * W
    if kind == "short":
        return E.with_rho(E.random_case(d, W, seed), bench_rho(seed + 1), d)
    if kind == "l2_edge":  # a level-2 entry at +128: level 1 at most
        return E.with_rho(E.random_case(d, W, seed), KM.level2_entry_at(NW, seed + 2, 32), d)
    if kind == "l1_out":   # a level-1 entry at +128, every coefficient inside [-127, 127]: level 0
        return E.with_rho(E.random_case(d, W, seed), KM.level1_entry_128(NW, seed + 3), d)
    if kind == "top":      # the plane skips: planes 4..13 of the top limb live on one group only
        base = E.build("top", d, W, G_LIVE[W])
        return E.with_rho({k: base[k] for k in ("acc_fc", "w_ccs")}, KM.short_rho(NW, seed + 4), d)
    if kind == "worst":    # an accumulator at the attainable bound under |rho| = 63
        base = E.build("worst", d, W, G_STAR[W], 511)
        rc = base["rc"] // E.BOUND[d] * WORST_BOUND
        assert np.array_equal(np.abs(rc), np.full_like(rc, WORST_BOUND))
        return E.with_rho({k: base[k] for k in ("acc_fc", "w_ccs")}, rc, d, target=base["target"])
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, W):
    """the case's inputs, the oracle's step and the level it must run at (read-only, shared)"""
    pr = params(d)
    kappa, N = E.KAPPA[d], W * pr.L
    case = case_of(kind, W)
    A = matrix(d, W)
    acc_fc = case["acc_fc"]
    acc_cm = O.ajtai_commit(A, kappa, N, d, O.crt(acc_fc, d))
    ofc, of = O.witness_from_w_ccs(case["w_ccs"], d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, kappa, N, d, of)
    want, sides = oracle_fold_hot(A, kappa, d, pr, acc_cm, acc_fc, ocm, ofc, case["rho"])
    want = dict(want, f_coeff=ofc, f=of, cm=ocm)
    ref = {"A": A, "w_ccs": case["w_ccs"], "acc_fc": acc_fc, "acc_cm": acc_cm, "rho": case["rho"], "want": want,
           "sides": sides, "case": case, "level": KM.best_level(case["rc"], BEST)}
    for v in (acc_cm, *want.values(), *(x for s in sides for x in s)):
        v.setflags(write=False)
    return ref


def step(c, ref, W, packed, level):
    """one step on c: every output is the oracle's, rho was judged short, and `level` ran"""
    import torch
    kappa = E.KAPPA[d]
    sch = make_scheme(torch, c, ref, d, W, kappa)
    keep, b = make_bufs(torch, ref, d, W, packed, kappa)
    torch.cuda.synchronize()  # torch wrote the inputs on its own stream
    c.dev_fold_step(sch, params(d), W, b)
    got = (c.fold_flag(), c.fold_level())
    c.sync()
    check_outputs(torch, c, ref, keep, d, W, packed, kappa)
    assert got == (0, level), f"(fold flag, level) {got}"


def run_all_caps(monkeypatch, kind, W, packed):
    """the default cap, then LATTICEUM_AMD_FOLD_KARA = 0 and 1, each on a fresh context"""
    import torch
    ref = reference(kind, W)
    for cap in (None, "0", "1"):
        if cap is None:
            monkeypatch.delenv("LATTICEUM_AMD_FOLD_KARA", raising=False)
        else:
            monkeypatch.setenv("LATTICEUM_AMD_FOLD_KARA", cap)
        c = LA.Context(0)
        try:
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            assert c.fold_level() == -1  # no step yet
            step(c, ref, W, packed, min(ref["level"], BEST if cap is None else int(cap)))
        finally:
            c.close()
    return ref


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("W", SHAPES)
def test_short_rho_runs_the_best_level(monkeypatch, W, packed):
    assert run_all_caps(monkeypatch, "short", W, packed)["level"] == BEST


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("W", SHAPES)
def test_level_2_entry_at_128_runs_level_1(monkeypatch, W, packed):
    """three -32 and a +32 on the level-2 entry that adds them up to +128. While level 1 is the
    highest level built (BEST = 1) this cannot tell a rejected level 2 from a missing one: it
    shows that such a rho, one past short_challenge's range, still runs at level 1 with the
    oracle's bits. The case is here so that it bites as soon as a second level is built."""
    assert run_all_caps(monkeypatch, "l2_edge", W, packed)["level"] == 1


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("W", SHAPES)
def test_level_1_entry_at_128_runs_the_dense_product(monkeypatch, W, packed):
    """T1 + T2 (or T2 - T1) at +128 from two coefficients at +-64: the flag stays 0, the level is 0"""
    assert run_all_caps(monkeypatch, "l1_out", W, packed)["level"] == 0


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("W", SHAPES)
def test_plane_skips_at_the_best_level(monkeypatch, W, packed):
    assert run_all_caps(monkeypatch, "top", W, packed)["level"] == BEST


@pytest.mark.parametrize("packed", MODES, ids=mode_id)
@pytest.mark.parametrize("W", SHAPES)
def test_accumulator_bound_at_the_best_level(monkeypatch, W, packed):
    """row 511 (the last of R0's second row half: P_a - P_c at their bounds) of the target sums
    2 sides * 14 planes * 1024 products of 63"""
    ref = run_all_caps(monkeypatch, "worst", W, packed)
    assert ref["level"] == BEST
    e, c = ref["case"]["target"]
    assert E.signed(ref["want"]["f0_coeff"]).reshape(-1, d)[e, c] == 2 * E.LIVE_PLANES * d * WORST_BOUND


def test_level_is_reset_every_step(monkeypatch):
    """level 1, level 0 (a level-1 entry out of range), level 1 again on one context"""
    import torch
    monkeypatch.delenv("LATTICEUM_AMD_FOLD_KARA", raising=False)
    c = LA.Context(0)
    try:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        for kind in ("short", "l1_out", "top"):
            ref = reference(kind, 2)
            step(c, ref, 2, True, ref["level"])
    finally:
        c.close()


def test_batched_steps_run_the_best_level(monkeypatch):
    """two packed steps in one lf_dev_fold_step_batch: each context reports its own step"""
    import torch
    monkeypatch.delenv("LATTICEUM_AMD_FOLD_KARA", raising=False)
    W = 33
    refs = [reference("short", W), reference("top", W)]
    ctx, other = LA.Context(0), LA.Context(0)
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        kappa = E.KAPPA[d]
        sch = make_scheme(torch, ctx, refs[0], d, W, kappa)
        steps = [make_bufs(torch, r, d, W, True, kappa) for r in refs]
        torch.cuda.synchronize()
        ctx.dev_fold_step_batch([other], sch, params(d), W, [b for _, b in steps])
        got = [(c.fold_flag(), c.fold_level()) for c in (ctx, other)]
        ctx.sync()
        other.sync()
        for r, (keep, _) in zip(refs, steps):
            check_outputs(torch, ctx, r, keep, d, W, True, kappa)
        assert got == [(0, BEST), (0, BEST)]
    finally:
        other.close()
        ctx.close()
