"""commit(z) from the new witness's plane-0 operand row (api_step.hip z_plane0).

A step on the fused X^1024+1 / X^4096+1 decompositions no longer converts f into
operand row 0: side 1's digit plane 0 is written there, the contraction's vector
0 is y_1[0], and cm = sum_k 2^k y_1[k] comes out of the step's epilogue. Every
output buffer of such a step is compared bit for bit with the oracle's step
(f_coeff, f, cm, y of both sides and all K planes, w_ccs_k, cm0, f0, f0_coeff,
w_ccs0, and the decomposed planes), at kappa = 2 on seeded inputs: the shapes
around one block of 16 groups, witnesses whose plane 0 is dead on every unit, on
one unit, or zero altogether, digits at the top of the balanced range, a rho
that is not short, the batched and the partial / finish launch paths, and the
to_frag phase counter. The oracle's step of one (shape, witness, rho) is computed
once and shared by the tests that need it."""
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from planes_decode import decode_planes, planes_u64
from test_gpu_parity import make_rho, oracle_fold_hot, params, rand, valid_f_coeff

pytestmark = pytest.mark.gpu
P = LA.P
KAPPA = 2
TOP = 1 << 14  # B / 2: the largest magnitude of a balanced base-2^15 digit


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def signed(x):
    """canonical residues -> their balanced representatives (int64)"""
    x = np.asarray(x, np.uint64)
    return np.where(x > P // 2, (x - np.uint64(P)).view(np.int64), x.view(np.int64))  # u64 wraps to x - p


def digits_witness(d, W, kind, seed):
    """w_ccs (NTT form, W elements) whose from_w_ccs digits are the chosen f_coeff:
    even: every digit even (plane 0 zero everywhere); unit: even on limb 2 of
    groups 0..15 only (one dead plane-0 unit); top: digits at +-2^14 among the rest"""
    pr = params(d)
    L, B = pr.L, pr.B
    rng = np.random.default_rng(seed)
    # even lower bounds: clearing bit 0 (rounding towards -inf) stays inside the ranges
    fc = rng.integers(-(TOP - 2), TOP, size=(W, L, d), dtype=np.int64)
    fc[:, L - 1] = rng.integers(-6, 8, size=(W, d))  # the top limb of a field element: |digit| <= 8
    if kind == "even":
        fc &= ~np.int64(1)
    elif kind == "unit":
        assert W >= 16
        fc[:16, 2] &= ~np.int64(1)
    elif kind == "top":
        pick = rng.random((W, L - 1, d)) < 1 / 16
        sign = rng.integers(0, 2, size=(W, L - 1, d)) * 2 - 1
        fc[:, :L - 1] = np.where(pick, sign * TOP, fc[:, :L - 1])
    else:
        raise ValueError(kind)
    fcu = np.where(fc.ravel() < 0, np.uint64(P) - (-fc.ravel()).astype(np.uint64), fc.ravel().astype(np.uint64))
    _, w = O.witness_from_f(O.crt(fcu, d), d, B, L)
    # the witness the step will make of it has the property the case is about
    ofc = signed(O.witness_from_w_ccs(w, d, B, L)[0]).reshape(W, L, d)
    if kind == "even":
        assert not (ofc & 1).any()
    elif kind == "unit":
        assert not (ofc[:16, 2] & 1).any()
        for g0 in range(0, W, 16):  # every other unit has an odd digit: its plane 0 is live
            for l in range(L):
                assert (g0, l) == (0, 2) or (ofc[g0:g0 + 16, l] & 1).any()
    else:
        assert (ofc == TOP).any() or (ofc == -TOP).any()
    return w


def witness(d, W, kind, seed=0):
    if kind == "rand":
        return rand(W * d, 8100 + d + W + seed)
    if kind == "zero":
        return np.zeros(W * d, np.uint64)
    return digits_witness(d, W, kind, 8200 + d + W)


@functools.lru_cache(maxsize=None)
def reference(d, W, wkind, short=True, seed=0):
    """inputs and the oracle's step for one case (read-only, shared between tests)"""
    pr = params(d)
    N = W * pr.L
    A = rand(KAPPA * N * d, 8000 + d + W)
    w_ccs = witness(d, W, wkind, seed)
    acc_fc, acc_f = valid_f_coeff(d, W, 8001 + d + W)
    acc_cm = O.ajtai_commit(A, KAPPA, N, d, acc_f)
    rho = make_rho(d, pr.K, 8002 + d) if short else rand(2 * pr.K * d, 8003 + d)
    ofc, of = O.witness_from_w_ccs(w_ccs, d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, KAPPA, N, d, of)
    want, sides = oracle_fold_hot(A, KAPPA, d, pr, acc_cm, acc_fc, ocm, ofc, rho)
    want = dict(want, f_coeff=ofc, f=of, cm=ocm)
    ref = {"A": A, "w_ccs": w_ccs, "acc_fc": acc_fc, "acc_cm": acc_cm, "rho": rho, "want": want, "sides": sides}
    for v in (A, w_ccs, acc_fc, acc_cm, rho, *want.values(), *(x for s in sides for x in s)):
        v.setflags(write=False)
    return ref


def make_bufs(torch, ref, d, W, packed, kappa=KAPPA):
    pr = params(d)
    K, N = pr.K, W * pr.L
    dev = lambda x: torch.from_numpy(np.array(x, copy=True).view(np.int64)).cuda()
    z = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")
    keep = {
        "w_ccs": dev(ref["w_ccs"]), "acc_cm": dev(ref["acc_cm"]), "acc_f_coeff": dev(ref["acc_fc"]),
        "rho": dev(ref["rho"]), "f_coeff": z(N * d), "f": z(N * d), "cm": z(kappa * d),
        "fk_coeff": [z(K * N * d) for _ in range(2)] if not packed else [None, None],
        "fk": [z(K * N * d) for _ in range(2)] if not packed else [None, None],
        "wk": [z(K * W * d) for _ in range(2)], "y": [z(K * kappa * d) for _ in range(2)],
        "f0": z(N * d), "f0_coeff": z(N * d), "w_ccs0": z(W * d), "cm0": z(kappa * d),
        "planes": [z(planes_u64(d, K, N)) for _ in range(2)] if packed else [None, None],
    }
    b = LA.LfFoldStepBufs()
    for k, v in keep.items():
        if isinstance(v, list):
            for s in range(2):
                getattr(b, k)[s] = v[s].data_ptr() if v[s] is not None else None
        else:
            setattr(b, k, v.data_ptr())
    return keep, b


def make_scheme(torch, c, ref, d, W, kappa=KAPPA):
    At = torch.from_numpy(np.array(ref["A"], copy=True).view(np.int64)).cuda()
    return LA.AjtaiCommitmentScheme(c, device_tensor=At, kappa=kappa, ncols=W * params(d).L, d=d)


def check_outputs(torch, c, ref, keep, d, W, packed, kappa=KAPPA):
    """every output buffer against the oracle's step"""
    pr = params(d)
    K, N = pr.K, W * pr.L
    h = lambda t: t.cpu().numpy().view(np.uint64)
    want, sides = ref["want"], ref["sides"]
    for key in ("f_coeff", "f", "cm", "f0", "f0_coeff", "w_ccs0", "cm0"):
        assert np.array_equal(h(keep[key]), want[key]), key
    y = np.concatenate([h(t) for t in keep["y"]]).reshape(2, K, kappa * d)
    oy = want["y"].reshape(2, K, kappa * d)
    for s in range(2):
        for k in range(K):
            assert np.array_equal(y[s, k], oy[s, k]), f"y side {s} plane {k}"
    for s in range(2):
        fck, fk = keep["fk_coeff"][s], keep["fk"][s]
        if packed:  # the rows as lf_dev_expand_planes makes them from the packed planes
            fck = torch.zeros(K * N * d, dtype=torch.int64, device="cuda")
            fk = torch.zeros(K * N * d, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            c.dev_expand_planes(pr, keep["planes"][s], N, fck, fk)
            c.sync()
        assert np.array_equal(h(fck), sides[s][0]), f"f_coeff_k side {s}"
        assert np.array_equal(h(fk), sides[s][1]), f"f_k side {s}"
        assert np.array_equal(h(keep["wk"][s]), sides[s][2]), f"w_ccs_k side {s}"


def run_step(c, d, W, wkind="rand", packed=True, short=True):
    import torch
    ref = reference(d, W, wkind, short)
    sch = make_scheme(torch, c, ref, d, W)
    keep, b = make_bufs(torch, ref, d, W, packed)
    torch.cuda.synchronize()  # torch wrote the inputs on its own stream
    c.dev_fold_step(sch, params(d), W, b)
    c.sync()
    check_outputs(torch, c, ref, keep, d, W, packed)
    return ref, keep


# W = 16: one block of 16 groups, nblk L odd, so the last chunk has a padding unit;
# W = 17: a partial second block; W = 33: a third
@pytest.mark.parametrize("d,W,packed", [(1024, 16, True), (1024, 17, True), (1024, 33, True),
                                        (4096, 16, True), (4096, 17, True), (1024, 17, False)])
def test_step_shapes(ctx, d, W, packed):
    run_step(ctx, d, W, packed=packed)


# the smallest shapes at which each layout can go wrong. d = 24, W = 17: one full 16-group
# unit of the wave-local decomposition plus a ragged one; d = 1024, W = 3: odd, so the
# half-wave pairing rounds up; d = 4096: the smallest W of the step tests above
@pytest.mark.parametrize("d,W", [(24, 17), (1024, 3), (4096, 16)])
def test_packed_planes_layout(ctx, d, W):
    """planes[0..1] of a packed step, downloaded and decoded by tests/planes_decode.py (written
    from include/lf.h's wording), are the oracle's decompose_witness digits -- compared
    directly, not through lf_dev_expand_planes, so a writer and a reader that moved together
    would not pass"""
    import torch
    pr = params(d)
    K, N = pr.K, W * pr.L
    ref = reference(d, W, "rand")
    sch = make_scheme(torch, ctx, ref, d, W)
    keep, b = make_bufs(torch, ref, d, W, True)
    torch.cuda.synchronize()
    ctx.dev_fold_step(sch, pr, W, b)
    ctx.sync()
    for s in range(2):
        got = decode_planes(keep["planes"][s].cpu().numpy(), d, K, N)
        want = signed(ref["sides"][s][0]).reshape(K, N, d)
        assert np.abs(want).max() == 1 and np.abs(want).any(axis=(1, 2))[:4].all()
        assert np.array_equal(got, want), f"side {s}"


def test_plane0_dead_everywhere(ctx):
    """every gadget digit of the new witness is even: all of side 1's plane-0 units
    are dead, row 0 is never written, the contraction takes the zero pieces for
    vector 0: y_1[0] = 0 and cm comes from planes 1.. alone"""
    d, W = 1024, 17
    ref, keep = run_step(ctx, d, W, "even")
    assert not ref["want"]["y"].reshape(2, params(d).K, KAPPA * d)[1, 0].any()
    assert not keep["y"][1][:KAPPA * d].any().item()
    assert ref["want"]["cm"].any()


def test_plane0_dead_on_one_unit(ctx):
    """plane 0 zero on exactly one unit (limb 2 of groups 0..15), live on the others"""
    run_step(ctx, 1024, 17, "unit")


@pytest.mark.parametrize("d", [1024, 4096])
def test_zero_witness(ctx, d):
    ref, keep = run_step(ctx, d, 17, "zero")
    assert not ref["want"]["cm"].any() and not keep["cm"].any().item()


def test_digits_at_top_of_range(ctx):
    """digits at +-2^14: plane 14 is live, the last term of cm's Horner chain"""
    d, W = 1024, 17
    ref, _ = run_step(ctx, d, W, "top")
    K = params(d).K
    assert ref["sides"][1][0].reshape(K, -1)[K - 1].any()


def test_rho_not_short(ctx):
    """the in-launch fallback of the coefficient-form fold reads (side 1, plane 0) from row 0"""
    run_step(ctx, 1024, 17, short=False)
    run_step(ctx, 1024, 17)  # and the coefficient-form fold again on the same context


def test_batch_of_two_equals_single_steps(ctx):
    import torch
    d, W = 1024, 17
    pr = params(d)
    refs = [reference(d, W, "rand"), reference(d, W, "rand", seed=1)]  # two witnesses, one A (seeded by the shape)
    assert np.array_equal(refs[0]["A"], refs[1]["A"])
    other = LA.Context(0)
    try:
        sch = make_scheme(torch, ctx, refs[0], d, W)
        steps = [make_bufs(torch, r, d, W, True) for r in refs]
        torch.cuda.synchronize()
        ctx.dev_fold_step_batch([other], sch, pr, W, [b for _, b in steps])
        ctx.sync()
        other.sync()
        singles = [make_bufs(torch, r, d, W, True) for r in refs]
        torch.cuda.synchronize()
        for keep, b in singles:
            ctx.dev_fold_step(sch, pr, W, b)
        ctx.sync()
        for r, (kb, _), (ks, _) in zip(refs, steps, singles):
            for key, v in kb.items():
                for tb, ts in zip(v, ks[key]) if isinstance(v, list) else [(v, ks[key])]:
                    assert tb is None or torch.equal(tb, ts), key
            check_outputs(torch, ctx, r, kb, d, W, True)
    finally:
        other.close()


@pytest.mark.parametrize("d", [1024, 4096])
def test_partial_then_finish_equals_step(ctx, d):
    """one GPU: the partial vectors are already the sums; vector 0 is y_1[0]'s"""
    import torch
    W = 17
    pr = params(d)
    ref = reference(d, W, "rand")
    sch = make_scheme(torch, ctx, ref, d, W)
    keep, b = make_bufs(torch, ref, d, W, True)
    n = ctx.fold_step_partial_len(sch, pr)
    assert n == (2 * (pr.K - 1) + 1) * KAPPA * d
    part = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.dev_fold_step_partial(sch, pr, W, b, part)
    ctx.dev_fold_step_finish(sch, pr, W, b, part)
    ctx.sync()
    check_outputs(torch, ctx, ref, keep, d, W, True)
    y10 = ref["want"]["y"].reshape(2, pr.K, KAPPA * d)[1, 0]
    assert np.array_equal(part[:KAPPA * d].cpu().numpy().view(np.uint64), y10)


def test_to_frag_phase_counter():
    """the packed d = 1024 and d = 4096 steps launch no to_frag pass; Phi_72's does"""
    import torch
    c = LA.Context(0)
    try:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.kernel_timing(True)
        for d in (1024, 4096):
            ref = reference(d, 17, "rand")
            sch = make_scheme(torch, c, ref, d, 17)
            keep, b = make_bufs(torch, ref, d, 17, True)
            torch.cuda.synchronize()
            c.dev_fold_step(sch, params(d), 17, b)
            c.sync()
        assert c.phase_stats("to_frag")[1] == 0
        assert c.phase_stats("decompose")[1] == 2
        d, W, kappa = 24, 17, 3
        pr = params(d)
        N = W * pr.L
        A = rand(kappa * N * d, 8300)
        acc_fc, acc_f = valid_f_coeff(d, W, 8301)
        ref = {"A": A, "w_ccs": rand(W * d, 8302), "acc_fc": acc_fc,
               "acc_cm": O.ajtai_commit(A, kappa, N, d, acc_f), "rho": make_rho(d, pr.K, 8303)}
        At = torch.from_numpy(A.view(np.int64)).cuda()
        sch = LA.AjtaiCommitmentScheme(c, device_tensor=At, kappa=kappa, ncols=N, d=d)
        keep, b = make_bufs(torch, ref, d, W, True)
        for k in ("cm", "cm0"):  # kappa = 3 here
            keep[k] = torch.zeros(kappa * d, dtype=torch.int64, device="cuda")
            setattr(b, k, keep[k].data_ptr())
        for s in range(2):
            keep["y"][s] = torch.zeros(pr.K * kappa * d, dtype=torch.int64, device="cuda")
            b.y[s] = keep["y"][s].data_ptr()
        torch.cuda.synchronize()
        c.dev_fold_step(sch, pr, W, b)
        c.sync()
        assert c.phase_stats("to_frag")[1] == 1
    finally:
        c.close()
