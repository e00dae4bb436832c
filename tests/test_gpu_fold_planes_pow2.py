"""GPU parity of f_0 folded from the packed digit planes at X^d + 1, d = 16 .. 512
(latticeum_amd/csrc/fold_coeff_pow2.hip): on the lean commit+fold step, where
lf_ctx_fold_flag now reports the short-rho decision, and through lf_dev_fold_planes, which
takes planes and rho alone (also at d = 1024 and d = 24, on their own kernels). Every
comparison is exact, against the CPU oracle."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from fold_rho_edges import TOP, extreme_digits, rho_ntt, signed, to_field, witness_of_digits
from test_gpu_parity import make_rho, params, rand, valid_f_coeff
from test_gpu_planes_pow2 import check_step, dev, host, make_step, scheme

pytestmark = pytest.mark.gpu
P = LA.P
DEGREES = [16, 32, 64, 128, 256, 512]
LF_ERR_INVALID_ARG, LF_ERR_UNSUPPORTED_RING, LF_ERR_INCORRECT_LENGTH = 1, 2, 7  # lf.h


def new_ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    c.close()


def set_rho(st, rc, d):
    """replace the step's rho by the signed coefficients rc [2K][d]"""
    st["rho"] = rho_ntt(rc, d)
    st["keep"]["rho"].copy_(dev(st["rho"]))


def short_rc(d, K, seed):
    """uniform over [-127, 127], both ends in every rho_i"""
    rng = np.random.default_rng(seed)
    rc = rng.integers(-127, 128, size=(2 * K, d), dtype=np.int64)
    rc[:, 0], rc[:, d - 1] = 127, -127
    return rc


def step(c, sch, st, W):
    import torch
    torch.cuda.synchronize()
    c.dev_fold_step(sch, st["pr"], W, st["b"])
    c.sync()


def setup(c, d, W, seed, kappa=2, **kw):
    pr = params(d)
    N = W * pr.L
    A = rand(kappa * N * d, seed + 77)
    return A, scheme(c, A, kappa, N, d), make_step(c, A, kappa, d, W, seed, **kw)


# ---------------------------------------------------------------- the lean step
@pytest.mark.parametrize("W", [1, 17])
@pytest.mark.parametrize("d", DEGREES)
def test_lean_step_reports_a_short_rho(ctx, d, W):
    """planes, no f_k: f_0 from the packed words; W = 1 splits the witnesses over blocks"""
    A, sch, st = setup(ctx, d, W, 2000 + d + W)
    step(ctx, sch, st, W)
    assert ctx.fold_flag() == 0
    check_step(ctx, st, A, 2, d, W)


def test_planes_beside_rows_keep_the_ntt_fold(ctx):
    d, W = 64, 17
    A, sch, st = setup(ctx, d, W, 2100, rows=True)
    step(ctx, sch, st, W)
    assert ctx.fold_flag() == -1
    check_step(ctx, st, A, 2, d, W)


def edge_case(d, W, sign, seed):
    """both sides' element e* all at sign (2^14 - 1) (the other elements +-(2^14 - 1), a small
    top limb) and every rho_i row c* of the Toeplitz matrix at +127: every coefficient of every
    rho_i is +-127 and f0_coeff[e*][c*] = sign 2 14 d 127"""
    pr = params(d)
    e_star, c_star = pr.L + 1, d // 3
    s = np.full(d, sign, np.int64)
    acc = extreme_digits(d, W, seed, e_star, s)
    new = extreme_digits(d, W, seed + 1, e_star, s)
    j = np.arange(d)
    r = np.zeros(d, np.int64)
    r[(c_star - j) % d] = np.where(j <= c_star, 127, -127)
    assert np.all(np.abs(r) == 127)
    return to_field(acc).ravel(), witness_of_digits(new, d), np.tile(r, (2 * pr.K, 1)), (e_star, c_star)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("d", [16, 64, 512])
def test_edges_of_the_short_range(ctx, d, sign):
    W = 2
    acc_fc, w_ccs, rc, (e, c) = edge_case(d, W, sign, 2200 + d)
    A, sch, st = setup(ctx, d, W, 2300 + d, w_ccs=w_ccs, acc_fc=acc_fc)
    set_rho(st, rc, d)
    step(ctx, sch, st, W)
    assert ctx.fold_flag() == 0
    got = signed(host(st["keep"]["f0_coeff"])).reshape(-1, d)
    assert got[e, c] == sign * 2 * 14 * d * 127 == sign * np.abs(got).max()
    check_step(ctx, st, A, 2, d, W)


@pytest.mark.parametrize("i,last,sign", [(0, False, 1), (14, True, -1), (15, False, -1), (29, True, 1)])
@pytest.mark.parametrize("d", [16, 64, 512])
def test_one_coefficient_just_outside(ctx, d, i, last, sign):
    """+-128 in one rho_i (a negative one is stored as p - 128): the flag goes up and the
    fallback (the fold from the operand rows, Witness::from_f) gives the oracle's step"""
    W = 2
    A, sch, st = setup(ctx, d, W, 2400 + d + i)
    rc = short_rc(d, st["pr"].K, 2500 + d + i)
    rc[i, d - 1 if last else 0] = sign * 128
    set_rho(st, rc, d)
    if sign < 0:
        assert int(O.icrt(st["rho"], d).reshape(-1, d)[i, d - 1 if last else 0]) == P - 128
    step(ctx, sch, st, W)
    assert ctx.fold_flag() == 1
    check_step(ctx, st, A, 2, d, W)


def test_flag_is_reset_between_steps():
    d, W = 64, 2
    c = new_ctx()
    try:
        A, sch, st = setup(c, d, W, 2600)
        short, out = short_rc(d, st["pr"].K, 2601), short_rc(d, st["pr"].K, 2602)
        out[7, 5] = -128
        for rc, flag in ((out, 1), (short, 0), (out, 1)):
            set_rho(st, rc, d)
            step(c, sch, st, W)
            assert c.fold_flag() == flag
            check_step(c, st, A, 2, d, W)
    finally:
        c.close()


def test_batch_keeps_each_steps_flag():
    import torch
    d, W, kappa = 64, 17, 2
    ctxs = [LA.Context(0) for _ in range(2)]
    try:
        pr = params(d)
        N = W * pr.L
        A = rand(kappa * N * d, 2700)
        sch = scheme(ctxs[0], A, kappa, N, d)
        steps = [make_step(ctxs[0], A, kappa, d, W, 2710 + 10 * i) for i in range(2)]
        out = short_rc(d, pr.K, 2720)
        out[29, d - 1] = 128
        set_rho(steps[0], short_rc(d, pr.K, 2721), d)
        set_rho(steps[1], out, d)
        torch.cuda.synchronize()
        ctxs[0].dev_fold_step_batch(ctxs[1:], sch, pr, W, [st["b"] for st in steps])
        for c in ctxs:
            c.sync()
        assert [c.fold_flag() for c in ctxs] == [0, 1]
        for st in steps:
            check_step(ctxs[0], st, A, kappa, d, W)
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- lf_dev_fold_planes
def pack_planes(fck, d, K, N):
    """the oracle's digit rows f_coeff_k [K][N][d] (mod p) -> one side's planes, by lf.h's wording"""
    dg = signed(fck).reshape(K, N, d)
    mag = sum((np.abs(dg[k]) << k) for k in range(K)).astype(np.int64)  # |x| [N][d]
    neg = (dg < 0).any(axis=0)
    if d == 24:  # [K][N] u64: bit i = coefficient i is nonzero, bit 32 + i = it is -1
        i = np.arange(24, dtype=np.uint64)
        nz = ((dg != 0).astype(np.uint64) << i).sum(axis=2, dtype=np.uint64)
        ng = ((dg < 0).astype(np.uint64) << (i + np.uint64(32))).sum(axis=2, dtype=np.uint64)
        return (nz | ng).ravel()
    sm = (mag | np.where(neg, 0x8000, 0)).astype(np.uint32)
    if d == 1024:  # word 32 q + r: coefficient r + 64 q low, r + 64 q + 32 high
        q, r = np.arange(16)[:, None], np.arange(32)[None, :]
        words = sm[:, (r + 64 * q).ravel()] | (sm[:, (r + 64 * q + 32).ravel()] << np.uint32(16))
    else:  # word j: coefficient j low, j + d / 2 high
        words = sm[:, :d // 2] | (sm[:, d // 2:] << np.uint32(16))
    return np.ascontiguousarray(words).ravel().view(np.uint64)


def small_params(d, K):
    pr = LA.LfParams()
    pr.d, pr.B, pr.L, pr.b_small, pr.K = d, 1 << 15, 5, 2, K
    return pr


def fold_planes_case(d, N, K, seed):
    """planes of both sides, rho, and the oracle's f0, f0_coeff, w_ccs0"""
    pr = params(d) if K == params(d).K else small_params(d, K)
    W = N // pr.L
    if K == params(d).K:
        fcs = [valid_f_coeff(d, W, seed + s)[0] for s in range(2)]
    else:  # fewer planes: coefficients inside (-2^(K-1), 2^(K-1))
        rng = np.random.default_rng(seed)
        fcs = [to_field(rng.integers(-(1 << (K - 1)) + 1, 1 << (K - 1), size=N * d)) for _ in range(2)]
    sides = [O.decompose_witness(fc, d, pr.B, pr.L, pr.b_small, K) for fc in fcs]
    rho = make_rho(d, K, seed + 2)
    f0 = O.fold_f0(rho, np.concatenate([s[1] for s in sides]), 2 * K, N, d)
    f0c, w0 = O.witness_from_f(f0, d, pr.B, pr.L)
    return pr, [pack_planes(s[0], d, K, N) for s in sides], rho, {"f0": f0, "f0_coeff": f0c, "w_ccs0": w0}


def run_fold_planes(c, pr, planes, rho, N):
    import torch
    d = pr.d
    pl = [dev(np.concatenate([p, np.zeros(8, np.uint64)])) for p in planes]
    out = {"f0_coeff": dev(n=N * d), "f0": dev(n=N * d), "w_ccs0": dev(n=N // pr.L * d)}
    r = dev(rho)
    torch.cuda.synchronize()
    c.dev_fold_planes(pr, pl[0], pl[1], N, r, out["f0_coeff"], out["f0"], out["w_ccs0"])
    return out


def check_fold_planes(d, N, K, seed, ncu=None):
    pr, planes, rho, want = fold_planes_case(d, N, K, seed)
    c = new_ctx()  # a context that has never run a step
    try:
        if ncu:
            c.check(c.lib.lf_ctx_set_cu_count(c.h, ncu))
        out = run_fold_planes(c, pr, planes, rho, N)
        c.sync()
        assert c.fold_flag() == 0
        for key, w in want.items():
            assert np.array_equal(host(out[key]), w), key
    finally:
        c.close()


@pytest.mark.parametrize("N", [5, 80, 85, 165])
@pytest.mark.parametrize("d", DEGREES)
def test_fold_planes_on_a_fresh_context(d, N):
    """W = 1, 16, 17, 33: a partial element tile, whole tiles, one past, an odd tile count"""
    check_fold_planes(d, N, 15, 3000 + d + N)


@pytest.mark.parametrize("d", DEGREES)
def test_fold_planes_without_witness_splits(d):
    """two compute units' worth of blocks: no split of the witnesses, and blocks that stride
    over several tile groups"""
    check_fold_planes(d, 165, 15, 3100 + d, ncu=1)


def test_fold_planes_with_three_planes():
    check_fold_planes(64, 85, 3, 3200)


@pytest.mark.parametrize("d,W", [(1024, 2), (24, 3)])
def test_fold_planes_on_the_other_rings(d, W):
    check_fold_planes(d, W * params(d).L, 15, 3300 + d)


def test_fold_planes_refusals_and_errors():
    d, N = 64, 85
    pr, planes, rho, want = fold_planes_case(d, N, 15, 3400)
    c = new_ctx()
    try:
        buf = dev(n=4096)

        def code(p, n=5):
            with pytest.raises(LA.LfError) as e:
                c.dev_fold_planes(p, buf, buf, n, buf, buf, buf, buf)
            return e.value.code

        assert code(params(4096)) == LF_ERR_UNSUPPORTED_RING
        assert code(params(2048)) == LF_ERR_UNSUPPORTED_RING
        p4 = small_params(d, 7)
        p4.b_small = 4
        assert code(p4) == LF_ERR_UNSUPPORTED_RING
        assert code(small_params(d, 16)) == LF_ERR_UNSUPPORTED_RING
        assert code(pr, 7) == LF_ERR_INCORRECT_LENGTH
        with pytest.raises(LA.LfError) as e:
            c.dev_fold_planes(pr, 0, buf, 5, buf, buf, buf, buf)  # a NULL planes0
        assert e.value.code == LF_ERR_INVALID_ARG
        c.sync()
        # a rho with one coefficient at 128: the next sync reports it, once
        rc = signed(O.icrt(rho, d)).reshape(-1, d).copy()
        rc[3, 9] = 128
        run_fold_planes(c, pr, planes, rho_ntt(rc, d), N)
        assert c.fold_flag() == 1
        with pytest.raises(LA.LfError) as e:
            c.sync()
        assert e.value.code == LF_ERR_INVALID_ARG and "rho" in str(e.value)
        c.sync()
        out = run_fold_planes(c, pr, planes, rho, N)
        c.sync()
        assert c.fold_flag() == 0
        for key, w in want.items():
            assert np.array_equal(host(out[key]), w), key
    finally:
        c.close()
