"""lf_dev_commit_planes: commit_witnesses from the packed digit planes and A alone.

Every comparison is exact. Two expectations:
  A, the oracle: planes packed by tests/planes_pack.py (from lf.h's wording) from seeded
     coefficients |x| <= 2^14; y[k] = O.ajtai_commit over O.decompose_witness's f_k rows, wk its
     w_ccs_k, cm = O.ajtai_commit of CRT(f_coeff);
  B, the library: y[k] = lf_dev_ajtai_commit over the f_k rows lf_dev_expand_planes makes of the
     same planes.
kappa = 2 unless stated. The oracle's side of one (ring, shape, seed) is computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
import planes_pack
from test_gpu_parity import make_rho, oracle_fold_hot, params, rand

pytestmark = pytest.mark.gpu
P = LA.P
KAPPA = 2
LF_ERR_INVALID_ARG, LF_ERR_UNSUPPORTED_RING, LF_ERR_INCORRECT_LENGTH = 1, 2, 7  # lf.h
POW2 = [16, 32, 64, 128, 256, 512]


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def fresh_context():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(x=None, n=None):
    import torch
    if x is not None:
        return torch.from_numpy(np.array(x, copy=True).view(np.int64)).cuda()
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def scheme(c, A, kappa, N, d):
    return LA.AjtaiCommitmentScheme(c, device_tensor=dev(A), kappa=kappa, ncols=N, d=d)


def to_field(x):
    """signed integers -> canonical residues"""
    x = np.asarray(x, np.int64)
    return np.where(x < 0, np.uint64(P) - (-x).astype(np.uint64), x.astype(np.uint64))


def seeded_coeffs(d, N, seed):
    """[N][d] signed coefficients, |x| <= 2^14 on every limb (every plane of every unit live)"""
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << 14), (1 << 14) + 1, size=(N, d), dtype=np.int64)


def oracle_side(A, kappa, d, pr, x):
    """expectation A for one side's signed coefficients x [N][d]: y [K][kappa d], wk [K][W d], cm"""
    N, K = x.shape[0], pr.K
    fc = to_field(x).ravel()
    _, fk, wk = O.decompose_witness(fc, d, pr.B, pr.L, pr.b_small, K)
    y = O.ajtai_commit(A, kappa, N, d, fk, K).reshape(K, kappa * d)
    cm = O.ajtai_commit(A, kappa, N, d, O.crt(fc, d))
    return {"y": y, "wk": wk.reshape(K, -1), "cm": cm, "fc": fc}


@functools.lru_cache(maxsize=None)
def case(d, W, kappa=KAPPA, seed=0):
    """seeded inputs of both sides and expectation A (read-only, shared between tests)"""
    pr = params(d)
    N = W * pr.L
    A = rand(kappa * N * d, 4000 + d + W + seed)
    xs = [seeded_coeffs(d, N, 4100 + 2 * (d + W + seed) + s) for s in range(2)]
    planes = [planes_pack.pack_coeffs(x, d, pr.K) for x in xs]
    want = [oracle_side(A, kappa, d, pr, x) for x in xs]
    for v in (A, *planes, *(a for w in want for a in w.values())):
        v.setflags(write=False)
    return {"A": A, "planes": planes, "want": want, "N": N, "pr": pr, "kappa": kappa, "d": d, "W": W}


def run_entry(c, sch, pr, planes, N, kappa, d, W, cm=True, wk=True):
    """the entry over len(planes) sides -> lists of host arrays y [K][kappa d], cm, wk [K][W d]"""
    import torch
    K, ns = pr.K, len(planes)
    pl = [dev(p) for p in planes]
    y = [dev(n=K * kappa * d) for _ in range(ns)]
    cmb = [dev(n=kappa * d) for _ in range(ns)] if cm else None
    wkb = [dev(n=K * W * d) for _ in range(ns)] if wk else None
    torch.cuda.synchronize()
    c.dev_commit_planes(sch, pr, pl, N, y, cmb, wkb)
    c.sync()
    return ([host(t).reshape(K, kappa * d) for t in y], [host(t) for t in cmb] if cm else None,
            [host(t).reshape(K, W * d) for t in wkb] if wk else None)


def check_against(want, y, cm, wk, what=""):
    for s in range(len(y)):
        K = want[s]["y"].shape[0]
        for k in range(K):
            assert np.array_equal(y[s][k], want[s]["y"][k]), f"{what} y[{s}][{k}]"
        if cm is not None:
            assert np.array_equal(cm[s], want[s]["cm"]), f"{what} cm[{s}]"
        if wk is not None:
            assert np.array_equal(wk[s], want[s]["wk"]), f"{what} wk[{s}]"


def library_side(c, sch, pr, planes, N, kappa, d):
    """expectation B: lf_dev_ajtai_commit over lf_dev_expand_planes's f_k rows -> y [K][kappa d]"""
    import torch
    K = pr.K
    fk = dev(n=K * N * d)
    torch.cuda.synchronize()
    c.dev_expand_planes(pr, dev(planes), N, None, fk)
    out = dev(n=K * kappa * d)
    c.dev_ajtai_commit(sch, [fk[k * N * d:(k + 1) * N * d] for k in range(K)], out)
    c.sync()
    return host(out).reshape(K, kappa * d)


def check_case(c, d, W, kappa=KAPPA, seed=0, library=False):
    cs = case(d, W, kappa, seed)
    sch = scheme(c, cs["A"], kappa, cs["N"], d)
    y, cm, wk = run_entry(c, sch, cs["pr"], cs["planes"], cs["N"], kappa, d, W)
    check_against(cs["want"], y, cm, wk, f"d={d} W={W}")
    if library:
        for s in range(2):
            assert np.array_equal(y[s], library_side(c, sch, cs["pr"], cs["planes"][s], cs["N"], kappa, d)), f"B, side {s}"


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("W", [1, 16, 17, 33])
@pytest.mark.parametrize("d", [24] + POW2)
def test_shapes(ctx, d, W):
    """W = 1: a unit with one live group; 16: a full unit; 17: a second unit with one group; 33: an
    odd unit count, padding at the end of both regions of the order. Against A"""
    check_case(ctx, d, W)


@pytest.mark.parametrize("W", [1, 17])
@pytest.mark.parametrize("d", [1024, 4096])
def test_shapes_large_rings(ctx, d, W):
    """against A and B"""
    check_case(ctx, d, W, library=True)


# ---------------------------------------------------------------- 2. a second row tile of A
def test_kappa_33(ctx):
    check_case(ctx, 32, 17, kappa=33)


# ---------------------------------------------------------------- 3. directed planes
def directed_witness(d, W, L):
    """signed coefficients [W L][d]: groups 0 .. 15 zero but for group 5, limb 0 = +2^14 (plane 14
    alone in one group of an otherwise zero unit); group 16: limb 0 = +2^14, limb 1 = -(2^14 - 1)
    (an all-negative element on fourteen planes), limb 2 = p - 1 and 1 side by side, limb 3 zero,
    and the top limb within +-8 (its planes 4 .. 14 zero)"""
    assert W >= 17 and L == 5
    x = np.zeros((W, L, d), np.int64)
    x[5, 0, :] = 1 << 14
    x[16, 0, :] = 1 << 14
    x[16, 1, :] = -((1 << 14) - 1)
    x[16, 2, 0::2], x[16, 2, 1::2] = -1, 1
    x[16, 4, :] = (np.arange(d) % 17) - 8
    return x.reshape(W * L, d)


@pytest.mark.parametrize("d", [64, 1024, 24])
def test_directed_planes(d):
    """side 0 directed, side 1 all zero (every unit dead); then the sides swapped on the same
    context, so every flag and row written by the first call is stale for the second"""
    W = 17
    pr = params(d)
    N = W * pr.L
    A = rand(KAPPA * N * d, 5000 + d)
    xs = [directed_witness(d, W, pr.L), np.zeros((N, d), np.int64)]
    want = [oracle_side(A, KAPPA, d, pr, x) for x in xs]
    assert not want[1]["y"].any() and not want[1]["cm"].any()
    planes = [planes_pack.pack_coeffs(x, d, pr.K) for x in xs]
    c = fresh_context()
    try:
        sch = scheme(c, A, KAPPA, N, d)
        for order in ((0, 1), (1, 0)):
            y, cm, wk = run_entry(c, sch, pr, [planes[s] for s in order], N, KAPPA, d, W)
            check_against([want[s] for s in order], y, cm, wk, f"order {order}")
    finally:
        c.close()


# ---------------------------------------------------------------- 4. arbitrary planes
@pytest.mark.parametrize("d,W", [(24, 17), (4096, 1)])
def test_arbitrary_planes(ctx, d, W):
    """the per-plane formats with random digits in {-1, 0, 1} per plane, not the digits of one
    number: every y[k] is A NTT(D_k), cm = sum_k 2^k y[k], wk[k] = recompose(NTT(D_k))"""
    pr = params(d)
    K, N = pr.K, W * pr.L
    rng = np.random.default_rng(6000 + d)
    dg = rng.integers(-1, 2, size=(K, N, d), dtype=np.int64)
    planes = planes_pack.pack_digits(dg, d)
    A = rand(KAPPA * N * d, 6001 + d)
    sch = scheme(ctx, A, KAPPA, N, d)
    y, cm, wk = run_entry(ctx, sch, pr, [planes], N, KAPPA, d, W)
    # A, with the digit rows as f_coeff_k
    fk = O.crt(to_field(dg).ravel(), d)
    want_y = O.ajtai_commit(A, KAPPA, N, d, fk, K).reshape(K, KAPPA * d)
    assert np.array_equal(y[0], want_y), "y against the oracle"
    for k in range(K):
        assert np.array_equal(wk[0][k], O.witness_from_f(fk.reshape(K, N * d)[k], d, pr.B, pr.L)[1]), f"wk[{k}]"
    total = sum(dg[k] << k for k in range(K))  # sum_k 2^k D_k, an integer of 16 bits
    assert np.array_equal(cm[0], O.ajtai_commit(A, KAPPA, N, d, O.crt(to_field(total).ravel(), d))), "cm"
    # B
    assert np.array_equal(y[0], library_side(ctx, sch, pr, planes, N, KAPPA, d)), "y against the library"


# ---------------------------------------------------------------- 5. two sides in one call
@pytest.mark.parametrize("d", [64, 24])
def test_two_sides_equal_two_calls(ctx, d):
    W = 17
    cs = case(d, W)
    sch = scheme(ctx, cs["A"], KAPPA, cs["N"], d)
    both = run_entry(ctx, sch, cs["pr"], cs["planes"], cs["N"], KAPPA, d, W)
    for s in range(2):
        one = run_entry(ctx, sch, cs["pr"], [cs["planes"][s]], cs["N"], KAPPA, d, W)
        for a, b in zip(both, one):
            assert np.array_equal(a[s], b[0]), f"side {s}"
    # without cm and wk the y are the same
    y, cm, wk = run_entry(ctx, sch, cs["pr"], cs["planes"], cs["N"], KAPPA, d, W, cm=False, wk=False)
    assert cm is None and wk is None
    for s in range(2):
        assert np.array_equal(y[s], both[0][s])


# ---------------------------------------------------------------- 6. no state
def run_step(c, d, W, kappa, seed):
    """one lean step (planes, no f_k rows) on fresh buffers, every output against the oracle's"""
    import torch
    pr = params(d)
    K, N = pr.K, W * pr.L
    A = rand(kappa * N * d, seed)
    sch = scheme(c, A, kappa, N, d)
    w_ccs = rand(W * d, seed + 1)
    acc_fc, acc_f = O.witness_from_w_ccs(rand(W * d, seed + 2), d, pr.B, pr.L)
    acc_cm = O.ajtai_commit(A, kappa, N, d, acc_f)
    rho = make_rho(d, K, seed + 3)
    keep = {
        "w_ccs": dev(w_ccs), "acc_cm": dev(acc_cm), "acc_f_coeff": dev(acc_fc), "rho": dev(rho),
        "f_coeff": dev(n=N * d), "f": dev(n=N * d), "cm": dev(n=kappa * d),
        "wk": [dev(n=K * W * d) for _ in range(2)], "y": [dev(n=K * kappa * d) for _ in range(2)],
        "f0": dev(n=N * d), "f0_coeff": dev(n=N * d), "w_ccs0": dev(n=W * d), "cm0": dev(n=kappa * d),
        "planes": [dev(n=max(LA.fold_step_planes_len(pr, N), 64)) for _ in range(2)],
    }
    b = LA.LfFoldStepBufs()
    for k, v in keep.items():
        if isinstance(v, list):
            for s in range(2):
                getattr(b, k)[s] = v[s].data_ptr()
        else:
            setattr(b, k, v.data_ptr())
    torch.cuda.synchronize()
    c.dev_fold_step(sch, pr, W, b)
    c.sync()
    ofc, of = O.witness_from_w_ccs(w_ccs, d, pr.B, pr.L)
    ocm = O.ajtai_commit(A, kappa, N, d, of)
    want, sides = oracle_fold_hot(A, kappa, d, pr, acc_cm, acc_fc, ocm, ofc, rho)
    assert np.array_equal(host(keep["cm"]), ocm) and np.array_equal(host(keep["f"]), of)
    assert np.array_equal(np.concatenate([host(t) for t in keep["y"]]), want["y"]), "y"
    for key in ("f0", "f0_coeff", "w_ccs0", "cm0"):
        assert np.array_equal(host(keep[key]), want[key]), key
    for s in range(2):
        assert np.array_equal(host(keep["wk"][s]), sides[s][2]), f"wk[{s}]"


@pytest.mark.parametrize("d,other", [(64, 1024), (24, 256), (1024, 24)])
def test_reads_no_state_and_leaves_none(d, other):
    """a context that has just run a lean step of another ring gives a fresh context's bits (the
    oracle's), and a lean step of either ring right after the entry still matches the oracle"""
    W = 17
    cs = case(d, W)
    a, b = fresh_context(), fresh_context()
    try:
        fresh = run_entry(a, scheme(a, cs["A"], KAPPA, cs["N"], d), cs["pr"], cs["planes"], cs["N"], KAPPA, d, W)
        run_step(b, other, 17, KAPPA, 7000 + other)
        used = run_entry(b, scheme(b, cs["A"], KAPPA, cs["N"], d), cs["pr"], cs["planes"], cs["N"], KAPPA, d, W)
        check_against(cs["want"], *fresh, "fresh")
        for x, z in zip(fresh, used):
            for s in range(2):
                assert np.array_equal(x[s], z[s])
        run_step(b, d, 17, KAPPA, 7100 + d)
        run_step(b, other, 17, KAPPA, 7200 + other)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 7. the stateless fold
@pytest.mark.parametrize("d", [64, 1024, 24])
def test_stateless_fold(d):
    """(planes0, planes1, rho, A) -> (f_0, w_ccs_0, y, cm_0, cm[1]) on a fresh context with no step:
    lf_dev_fold_planes, lf_dev_commit_planes and lf_dev_fold over the 2K y rows, against fold()'s"""
    import torch
    W = 17
    cs = case(d, W)
    pr, N, A = cs["pr"], cs["N"], cs["A"]
    K, kd = pr.K, KAPPA * d
    rho = make_rho(d, K, 8000 + d)
    fcs = [w["fc"] for w in cs["want"]]
    want, _ = oracle_fold_hot(A, KAPPA, d, pr, cs["want"][0]["cm"], fcs[0], cs["want"][1]["cm"], fcs[1], rho)
    c = fresh_context()
    try:
        sch = scheme(c, A, KAPPA, N, d)
        pl = [dev(p) for p in cs["planes"]]
        r = dev(rho)
        f0c, f0, w0 = dev(n=N * d), dev(n=N * d), dev(n=W * d)
        y = [dev(n=K * kd) for _ in range(2)]
        cm1, cm0 = dev(n=kd), dev(n=kd)
        torch.cuda.synchronize()
        c.dev_fold_planes(pr, pl[0], pl[1], N, r, f0c, f0, w0)
        c.dev_commit_planes(sch, pr, pl, N, y, [None, cm1])
        rows = (C.c_void_p * (2 * K))(*[y[s].data_ptr() + 8 * k * kd for s in range(2) for k in range(K)])
        c.check(c.lib.lf_dev_fold(c.h, d, r.data_ptr(), rows, 2 * K, KAPPA, cm0.data_ptr()))
        c.sync()
        assert np.array_equal(host(f0), want["f0"]) and np.array_equal(host(f0c), want["f0_coeff"])
        assert np.array_equal(host(w0), want["w_ccs0"])
        assert np.array_equal(np.concatenate([host(t) for t in y]), want["y"]), "y"
        assert np.array_equal(host(cm0), want["cm0"]), "cm_0"
        assert np.array_equal(host(cm1), cs["want"][1]["cm"]), "cm[1]"
    finally:
        c.close()


# ---------------------------------------------------------------- 8. refusals
def lean_step_status(c, sch, pr, W):
    """what a lean step (planes, no f_k rows) of this scheme returns; one zeroed buffer, larger than
    any of the step's at the shape this is used for, stands for all of them"""
    buf = dev(n=1 << 16)
    assert pr.K * sch.kappa * pr.d <= 1 << 16 and pr.K * W * pr.L * pr.d <= 1 << 16
    b = LA.LfFoldStepBufs()
    for name, _ in b._fields_:
        v = getattr(b, name)
        if hasattr(v, "__len__"):
            for s in range(2):
                v[s] = None if name in ("fk", "fk_coeff") else buf.data_ptr()
        else:
            setattr(b, name, buf.data_ptr())
    with pytest.raises(LA.LfError) as e:
        c.dev_fold_step(sch, pr, W, b)
    return e.value.code


def test_refusals():
    c = fresh_context()
    try:
        buf = dev(n=1 << 16)

        def refused(code, sch, pr, planes, N, y=None):
            with pytest.raises(LA.LfError) as e:
                c.dev_commit_planes(sch, pr, planes, N, y if y is not None else [buf] * len(planes))
            assert e.value.code == code, e.value

        def small_scheme(d, N, kappa=KAPPA):
            return scheme(c, rand(kappa * N * d, 9000 + d + N + kappa), kappa, N, d)

        # rings without a packed form
        pr = params(2048)
        refused(LF_ERR_UNSUPPORTED_RING, small_scheme(2048, pr.L), pr, [buf, buf], pr.L)
        s64 = small_scheme(64, 5)
        p4 = params(64)
        p4.b_small, p4.K = 4, 8
        refused(LF_ERR_UNSUPPORTED_RING, s64, p4, [buf, buf], 5)
        p16 = params(64)
        p16.K = 16
        refused(LF_ERR_UNSUPPORTED_RING, s64, p16, [buf, buf], 5)
        # a scheme without operand fragments: the lean step's status
        pr = params(16)
        s130 = small_scheme(16, pr.L, kappa=130)
        with pytest.raises(LA.LfError) as e:
            c.dev_commit_planes(s130, pr, [buf, buf], pr.L, [buf, buf])
        assert e.value.code == lean_step_status(c, s130, pr, 1)
        # lengths
        pr = params(64)
        refused(LF_ERR_INCORRECT_LENGTH, small_scheme(64, 10), pr, [buf, buf], 7)
        refused(LF_ERR_INCORRECT_LENGTH, small_scheme(64, 10), pr, [buf, buf], 5)
        # pointers and nside
        refused(LF_ERR_INVALID_ARG, s64, pr, [0, buf], 5, [buf, buf])
        refused(LF_ERR_INVALID_ARG, s64, pr, [buf, buf], 5, [buf, 0])
        refused(LF_ERR_INVALID_ARG, s64, pr, [buf, buf, buf], 5)
        refused(LF_ERR_INVALID_ARG, s64, pr, [], 5)
        c.sync()
        # the context is usable afterwards
        check_case(c, 64, 17)
    finally:
        c.close()
