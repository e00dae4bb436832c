"""GPU parity of the lean commit+fold step at X^d + 1, d = 16 .. 512: the fused
decomposition (latticeum_amd/csrc/decompose_pow2.hip) that writes the matrix-core
operand rows directly, keeps the decomposed witnesses as packed sign|magnitude planes
(lf_fold_step_bufs.planes) and folds f_0 from the operand rows. Every comparison is
exact, against the CPU oracle's step: f, f_coeff, cm, wk, y, cm0, f0, f0_coeff,
w_ccs0, and the planes -- decoded here from include/lf.h's wording and expanded by
lf_dev_expand_planes -- against the oracle's decompose_witness rows."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from test_gpu_parity import check_dev_fold_step, check_fold_outputs, make_rho, oracle_fold_hot, params, rand, valid_f_coeff

pytestmark = pytest.mark.gpu
P = LA.P
DEGREES = [16, 32, 64, 128, 256, 512]
LF_ERR_UNSUPPORTED_RING, LF_ERR_DECOMPOSITION_OVERFLOW = 2, 6  # lf.h


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


# ---------------------------------------------------------------- buffers and decoding
def dev(x=None, n=None):
    import torch
    if x is not None:
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def scheme(ctx, A, kappa, N, d):
    import torch
    return LA.AjtaiCommitmentScheme(ctx, device_tensor=torch.from_numpy(A.view(np.int64)).cuda(), kappa=kappa,
                                    ncols=N, d=d)


def make_step(ctx, A, kappa, d, W, seed, rows=False, w_ccs=None, acc_fc=None, planes=True):
    """one step's inputs and buffers; rows: the u64 f_k / f_coeff_k buffers beside the planes"""
    pr = params(d)
    K, L = pr.K, pr.L
    N = W * L
    if w_ccs is None:
        w_ccs = rand(W * d, seed)
    if acc_fc is None:
        acc_fc, _ = valid_f_coeff(d, W, seed + 1)
    acc_cm = O.ajtai_commit(A, kappa, N, d, O.crt(acc_fc, d))
    rho = make_rho(d, K, seed + 2)
    plen = max(LA.fold_step_planes_len(pr, N), 64)
    keep = {
        "w_ccs": dev(w_ccs), "acc_cm": dev(acc_cm), "acc_f_coeff": dev(acc_fc), "rho": dev(rho),
        "f_coeff": dev(n=N * d), "f": dev(n=N * d), "cm": dev(n=kappa * d),
        "fk_coeff": [dev(n=K * N * d) for _ in range(2)] if rows else [None, None],
        "fk": [dev(n=K * N * d) for _ in range(2)] if rows else [None, None],
        "wk": [dev(n=K * W * d) for _ in range(2)], "y": [dev(n=K * kappa * d) for _ in range(2)],
        "f0": dev(n=N * d), "f0_coeff": dev(n=N * d), "w_ccs0": dev(n=W * d), "cm0": dev(n=kappa * d),
        "planes": [dev(n=plen) for _ in range(2)] if planes else [None, None],
    }
    b = LA.LfFoldStepBufs()
    for k, v in keep.items():
        if isinstance(v, list):
            for s in range(2):
                getattr(b, k)[s] = v[s].data_ptr() if v[s] is not None else None
        else:
            setattr(b, k, v.data_ptr())
    return {"keep": keep, "b": b, "w_ccs": w_ccs, "acc_cm": acc_cm, "acc_fc": acc_fc, "rho": rho, "pr": pr}


def decode_planes(words_u64, d, K, N):
    """include/lf.h, d = 16 .. 512: an element is d / 2 u32; word j of element e at
    e d / 2 + j holds coefficient j in its low half and coefficient j + d / 2 in its high
    half, as bits 0..14 = |x| and bit 15 = x is negative; digit k = sign(x) bit_k(|x|).
    Returns the digits mod p as f_coeff_k [K][N][d]."""
    w = np.ascontiguousarray(words_u64).view(np.uint32)[:N * d // 2].reshape(N, d // 2)
    halves = np.concatenate([w & 0xFFFF, w >> 16], axis=1).astype(np.uint64)  # [N][d]
    neg = (halves >> np.uint64(15)) & np.uint64(1)
    out = np.zeros((K, N, d), np.uint64)
    for k in range(K):
        bit = (halves >> np.uint64(k)) & np.uint64(1)
        out[k] = np.where(bit == 1, np.where(neg == 1, np.uint64(P - 1), np.uint64(1)), np.uint64(0))
    return out.ravel()


def check_step(ctx, st, A, kappa, d, W):
    """every output of the step that just ran against the oracle's"""
    import torch
    pr, keep = st["pr"], st["keep"]
    K, N = pr.K, W * pr.L
    ofc, _ = O.witness_from_w_ccs(st["w_ccs"], d, pr.B, pr.L)
    assert np.array_equal(host(keep["f_coeff"]), ofc), "f_coeff"
    had_rows = keep["fk"][0] is not None
    for s, fc in ((0, st["acc_fc"]), (1, ofc)):
        ofck, ofk, _ = O.decompose_witness(fc, d, pr.B, pr.L, pr.b_small, K)
        assert np.array_equal(decode_planes(host(keep["planes"][s]), d, K, N), ofck), f"planes of side {s}"
        fck, fk = dev(n=K * N * d), dev(n=K * N * d)
        torch.cuda.synchronize()
        ctx.dev_expand_planes(pr, keep["planes"][s], N, fck, fk)
        ctx.sync()
        if had_rows:  # planes beside the rows: both were written
            assert np.array_equal(host(keep["fk_coeff"][s]), ofck) and np.array_equal(host(keep["fk"][s]), ofk)
        keep["fk_coeff"][s], keep["fk"][s] = fck, fk
    # f, cm, y, f0, f0_coeff, w_ccs0, cm0, and the expanded rows and wk of both sides
    check_fold_outputs(host, keep, A, kappa, d, pr, W, st["w_ccs"], st["acc_cm"], st["acc_fc"], st["rho"])
    if not had_rows:
        keep["fk_coeff"], keep["fk"] = [None, None], [None, None]


def run_step(ctx, d, W, kappa, seed, **kw):
    import torch
    pr = params(d)
    N = W * pr.L
    A = rand(kappa * N * d, seed + 77)
    sch = scheme(ctx, A, kappa, N, d)
    st = make_step(ctx, A, kappa, d, W, seed, **kw)
    torch.cuda.synchronize()
    ctx.dev_fold_step(sch, pr, W, st["b"])
    ctx.sync()
    check_step(ctx, st, A, kappa, d, W)
    return A, sch, st


# ---------------------------------------------------------------- the step
@pytest.mark.parametrize("W", [1, 16, 17, 33])
@pytest.mark.parametrize("d", DEGREES)
def test_lean_step_matches_oracle(ctx, d, W):
    """W = 1: a unit of one live group; 16: a full unit; 17: a second unit with one group;
    33: an odd unit count, padding positions at the end of both regions of the order"""
    run_step(ctx, d, W, 2, 1000 + d + W)


def directed_witness(d, W, L):
    """side 0's f_coeff: groups 0 .. 15 zero but for group 5, limb 0 = +2^14 (plane 14
    alone, in a unit whose other planes are dead); group 16: limb 0 = +2^14, limb 1 =
    -(2^14 - 1) (fourteen planes, all negative), limb 2 = p - 1 and 1 side by side,
    limb 3 an all-zero element, limb 4 = +-1"""
    fc = np.zeros((W, L, d), np.uint64)
    fc[5, 0, :] = 1 << 14
    fc[16, 0, :] = 1 << 14
    fc[16, 1, :] = P - ((1 << 14) - 1)
    fc[16, 2, 0::2], fc[16, 2, 1::2] = P - 1, 1
    fc[16, 4, 0::2], fc[16, 4, 1::2] = 1, P - 1
    return fc.ravel()


@pytest.mark.parametrize("d", [64, 512])
def test_directed_witnesses_and_overflow(d):
    """dead units below and beyond the top limb, single planes, all-negative planes; then one
    coefficient at 2^15 gives the decomposition's range error, and the same context runs a
    valid step afterwards"""
    import torch
    W, kappa = 17, 2
    pr = params(d)
    N = W * pr.L
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        # both sides directed: the new witness is zero (all of side 1's units dead)
        A, sch, st = run_step(c, d, W, kappa, 3100 + d, acc_fc=directed_witness(d, W, pr.L),
                              w_ccs=np.zeros(W * d, np.uint64))
        bad = directed_witness(d, W, pr.L)
        bad[(16 * pr.L + 3) * d + 7] = 1 << 15
        st["keep"]["acc_f_coeff"].copy_(dev(bad))
        torch.cuda.synchronize()
        with pytest.raises(LA.LfError) as e:
            c.dev_fold_step(sch, pr, W, st["b"])
            c.sync()
        assert e.value.code == LF_ERR_DECOMPOSITION_OVERFLOW
        st2 = make_step(c, A, kappa, d, W, 3200 + d)
        torch.cuda.synchronize()
        c.dev_fold_step(sch, pr, W, st2["b"])
        c.sync()
        check_step(c, st2, A, kappa, d, W)
    finally:
        c.close()


def test_stale_flags_and_rows(ctx):
    """three steps on the same buffers: the second's witnesses are zero where the first's
    were not, the third reverses that -- a stale dead flag would contract a written row as
    zero, a stale operand row would be contracted in place of a dead unit"""
    import torch
    d, W, kappa = 128, 17, 2
    pr = params(d)
    L, N = pr.L, W * pr.L
    A, sch, st = run_step(ctx, d, W, kappa, 4100)
    keep = st["keep"]
    fc2, _ = valid_f_coeff(d, W, 4200)
    fc2 = fc2.copy()
    fc2[:16 * L * d] = 0  # unit G = 0 of side 0 all dead; side 1 zero altogether
    fc3, _ = valid_f_coeff(d, W, 4300)
    fc3 = fc3.copy()
    fc3[16 * L * d:] = 0  # and the reverse
    for acc_fc, w_ccs in ((fc2, np.zeros(W * d, np.uint64)), (fc3, rand(W * d, 4301))):
        st["acc_fc"], st["w_ccs"] = acc_fc, w_ccs
        st["acc_cm"] = O.ajtai_commit(A, kappa, N, d, O.crt(acc_fc, d))
        keep["acc_f_coeff"].copy_(dev(acc_fc))
        keep["w_ccs"].copy_(dev(w_ccs))
        keep["acc_cm"].copy_(dev(st["acc_cm"]))
        torch.cuda.synchronize()
        ctx.dev_fold_step(sch, pr, W, st["b"])
        ctx.sync()
        check_step(ctx, st, A, kappa, d, W)


def test_mixed_paths_on_one_context():
    """the lean d = 64 step between the fused d = 1024 and the packed Phi_72 steps, then the
    plain d = 64 step (f_k given, no planes), all on one context: each path leaves its own
    dead flags, operand rows and packed scratch behind"""
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        run_step(c, 64, 17, 2, 5100)
        check_dev_fold_step(c, 1024, 2, 2, packed=True)
        check_dev_fold_step(c, 24, 3, 3, packed=True)
        run_step(c, 64, 17, 2, 5200)
        check_dev_fold_step(c, 64, 17, 2)  # Decomp::Plain: fk given, no planes
    finally:
        c.close()


def test_planes_beside_rows(ctx):
    """planes given together with fk / fk_coeff: both are written, f_0 folds from the f_k rows"""
    run_step(ctx, 64, 17, 2, 6100, rows=True)


def test_without_planes_or_rows(ctx):
    """fk NULL and no planes: the packed words go to the context's scratch, f_0 from the rows"""
    import torch
    d, W, kappa = 64, 17, 2
    pr = params(d)
    N = W * pr.L
    A = rand(kappa * N * d, 6200)
    sch = scheme(ctx, A, kappa, N, d)
    st = make_step(ctx, A, kappa, d, W, 6201, planes=False)
    torch.cuda.synchronize()
    ctx.dev_fold_step(sch, pr, W, st["b"])
    ctx.sync()
    ofc, of = O.witness_from_w_ccs(st["w_ccs"], d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, kappa, N, d, of)
    want, sides = oracle_fold_hot(A, kappa, d, pr, st["acc_cm"], st["acc_fc"], ocm, ofc, st["rho"])
    keep = st["keep"]
    assert np.array_equal(host(keep["cm"]), ocm) and np.array_equal(host(keep["f"]), of)
    assert np.array_equal(np.concatenate([host(y) for y in keep["y"]]), want["y"])
    for key in ("f0", "f0_coeff", "w_ccs0", "cm0"):
        assert np.array_equal(host(keep[key]), want[key]), key
    for s in range(2):
        assert np.array_equal(host(keep["wk"][s]), sides[s][2])


def test_decompose_commit_without_rows(ctx):
    """lf_dev_decompose_commit with NULL fk: y (y_0 included) and wk of both sides"""
    import torch
    d, W, kappa = 256, 17, 2
    pr = params(d)
    K, N = pr.K, W * pr.L
    A = rand(kappa * N * d, 7100)
    sch = scheme(ctx, A, kappa, N, d)
    st = make_step(ctx, A, kappa, d, W, 7101)
    wi_fc, wi_f = valid_f_coeff(d, W, 7102)
    cm_i = O.ajtai_commit(A, kappa, N, d, wi_f)
    st["keep"]["f_coeff"].copy_(dev(wi_fc))
    st["keep"]["cm"].copy_(dev(cm_i))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.lf_dev_decompose_commit(ctx.h, sch.h, LA._lib.C.byref(pr), W, LA._lib.C.byref(st["b"])))
    ctx.sync()
    want, sides = oracle_fold_hot(A, kappa, d, pr, st["acc_cm"], st["acc_fc"], cm_i, wi_fc, st["rho"])
    assert np.array_equal(np.concatenate([host(y) for y in st["keep"]["y"]]), want["y"])
    for s in range(2):
        assert np.array_equal(host(st["keep"]["wk"][s]), sides[s][2]), f"wk side {s}"
        assert np.array_equal(decode_planes(host(st["keep"]["planes"][s]), d, K, N), sides[s][0])


OUT_KEYS = ("f_coeff", "f", "cm", "f0", "f0_coeff", "w_ccs0", "cm0")


def assert_same_outputs(a, b):
    for key in OUT_KEYS:
        assert np.array_equal(host(a[key]), host(b[key])), key
    for key in ("wk", "y", "planes"):
        for s in range(2):
            assert np.array_equal(host(a[key][s]), host(b[key][s])), f"{key}[{s}]"


def test_batch_of_two_lean_steps():
    """lf_dev_fold_step_batch (the deferred contraction): bit-equal to the steps run alone"""
    import torch
    d, W, kappa = 64, 17, 2
    pr = params(d)
    N = W * pr.L
    A = rand(kappa * N * d, 8100)
    ctxs = [LA.Context(0) for _ in range(2)]
    try:
        sch = scheme(ctxs[0], A, kappa, N, d)
        steps = [make_step(ctxs[0], A, kappa, d, W, 8200 + 10 * i) for i in range(2)]
        torch.cuda.synchronize()
        ctxs[0].dev_fold_step_batch(ctxs[1:], sch, pr, W, [st["b"] for st in steps])
        for c in ctxs:
            c.sync()
        for i, st in enumerate(steps):
            alone = make_step(ctxs[0], A, kappa, d, W, 8200 + 10 * i)
            torch.cuda.synchronize()
            ctxs[0].dev_fold_step(sch, pr, W, alone["b"])
            ctxs[0].sync()
            assert_same_outputs(st["keep"], alone["keep"])
            check_step(ctxs[0], st, A, kappa, d, W)
    finally:
        for c in ctxs:
            c.close()


def test_partial_then_finish(ctx):
    """the column-sharded halves on one GPU, the partial buffer handed through unchanged:
    equal to the whole step; vector 0 of the partial is y_1[0] (side 1's plane-0 row)"""
    import torch
    d, W, kappa = 128, 16, 2
    pr = params(d)
    N, kd = W * pr.L, kappa * d
    A, sch, whole = run_step(ctx, d, W, kappa, 9100)
    st = make_step(ctx, A, kappa, d, W, 9100)
    n = ctx.fold_step_partial_len(sch, pr)
    part = dev(n=n)
    torch.cuda.synchronize()
    ctx.dev_fold_step_partial(sch, pr, W, st["b"], part)
    ctx.dev_fold_step_finish(sch, pr, W, st["b"], part)
    ctx.sync()
    assert_same_outputs(st["keep"], whole["keep"])
    assert np.array_equal(host(part)[:kd], host(whole["keep"]["y"][1])[:kd])


def test_second_row_tile_of_the_contraction(ctx):
    """kappa = 33: a second 32-row tile of A"""
    run_step(ctx, 32, 17, 33, 9500)


@pytest.mark.parametrize("mode", ["0", "1", None])
def test_dec_nt_modes(ctx, monkeypatch, mode):
    """LATTICEUM_AMD_DEC_NT: plain stores, streaming stores, the default rule"""
    if mode is None:
        monkeypatch.delenv("LATTICEUM_AMD_DEC_NT", raising=False)
    else:
        monkeypatch.setenv("LATTICEUM_AMD_DEC_NT", mode)
    run_step(ctx, 256, 17, 2, 9700)


# ---------------------------------------------------------------- refusals that stay
def test_refusals_that_stay(ctx):
    import torch
    for d, W, kappa in ((2048, 1, 2), (16, 1, 130)):  # no packed form; a scheme without operand fragments
        pr = params(d)
        N = W * pr.L
        A = rand(kappa * N * d, 9900 + d)
        sch = scheme(ctx, A, kappa, N, d)
        st = make_step(ctx, A, kappa, d, W, 9901 + d)
        torch.cuda.synchronize()
        with pytest.raises(LA.LfError):
            ctx.dev_fold_step(sch, pr, W, st["b"])
        ctx.sync()
    pr = params(2048)
    assert LA.fold_step_planes_len(pr, 5) == 0
    with pytest.raises(LA.LfError) as e:
        ctx.dev_expand_planes(pr, dev(n=64), 1, dev(n=pr.K * 2048), None)
    assert e.value.code == LF_ERR_UNSUPPORTED_RING
