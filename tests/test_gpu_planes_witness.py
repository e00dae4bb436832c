"""lf_dev_pack_planes, lf_dev_planes_witness, lf_dev_planes_check: the packed digit planes from a
witness's f_coeff and back, without a step. Every comparison is exact. The models are
tests/planes_pack.py and tests/planes_decode.py (written from lf.h's wording), a lean
lf_dev_fold_step's planes, lf_dev_expand_planes's rows, and the oracle's fold()."""
import ctypes as C
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from planes_decode import decode_planes
from planes_pack import pack_coeffs, pack_digits
from test_gpu_parity import make_rho, oracle_fold_hot, params, rand

pytestmark = pytest.mark.gpu
P = LA.P
KAPPA = 2
LF_ERR_INVALID_ARG, LF_ERR_UNSUPPORTED_RING, LF_ERR_DECOMPOSITION_OVERFLOW, LF_ERR_INCORRECT_LENGTH = 1, 2, 6, 7  # lf.h
SHAPES = [(24, 5), (24, 35), (24, 85), (16, 5), (16, 85), (64, 5), (64, 85), (512, 5), (512, 85),
          (1024, 5), (1024, 15), (4096, 5), (4096, 15)]
FORMATS = [(24, 35), (64, 85), (1024, 5), (4096, 5)]  # one shape per packed format
SMALL_K = 9


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


def dev(x=None, n=None, fill=0):
    import torch
    if x is not None:
        return torch.from_numpy(np.array(x, copy=True).view(np.int64)).cuda()
    return torch.full((n,), fill, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def to_field(x):
    x = np.asarray(x, np.int64)
    return np.where(x < 0, np.uint64(P) - (-x).astype(np.uint64), x.astype(np.uint64))


def signed(x):
    x = np.asarray(x, np.uint64)
    return np.where(x > P // 2, (x - np.uint64(P)).view(np.int64), x.view(np.int64))


def params_k(d, K=15):
    pr = params(d)
    pr.K = K
    return pr


def decode_any(buf, d, K, N):
    """decode_planes, and the d = 16 .. 512 words by lf.h's wording: an element is d / 2 u32, word j holds
    coefficient j in its low half and coefficient j + d / 2 in its high half, as 16-bit sign|magnitude"""
    if d in (24, 1024, 4096):
        return decode_planes(buf, d, K, N)
    w = np.ascontiguousarray(buf).view(np.uint32).reshape(N, d // 2)
    c = np.concatenate([w & 0xFFFF, w >> 16], axis=1).astype(np.int64)
    sign = 1 - 2 * (c >> 15 & 1)
    k = np.arange(K).reshape(K, 1, 1)
    return ((c[None] >> k & 1) * sign[None]).astype(np.int8)


def recompose(digits):
    return sum(digits[k].astype(np.int64) << k for k in range(digits.shape[0]))


@functools.lru_cache(maxsize=None)
def coeffs(d, N, K=15, seed=0):
    """[N][d] signed coefficients in (-2^K, 2^K), the directed values at the first and last coefficients of
    the first and last element: +-(2^K - 1), +-2^(K - 1) at the corners, +-1, 0 and -1 (the word p - 1) beside them"""
    rng = np.random.default_rng(9000 + d + N + K + seed)
    x = rng.integers(-(1 << K) + 1, 1 << K, size=(N, d), dtype=np.int64)
    T, H = (1 << K) - 1, 1 << (K - 1)
    x[0, 0], x[0, d - 1], x[N - 1, 0], x[N - 1, d - 1] = T, -T, H, -H
    x[0, 1], x[0, d - 2], x[N - 1, 1], x[N - 1, d - 2] = 1, -1, 0, -1
    x.setflags(write=False)
    return x


def pack(c, pr, x_or_field, N, already_field=False):
    """dev_pack_planes into a buffer pre-filled with 0xFF -> the device tensor"""
    import torch
    words = x_or_field if already_field else to_field(x_or_field).ravel()
    fc = dev(words)
    out = dev(n=LA.fold_step_planes_len(pr, N), fill=-1)
    torch.cuda.synchronize()
    c.dev_pack_planes(pr, fc, N, out)
    c.sync()
    return out


def witness(c, pr, planes, N, want=("fc", "f", "w")):
    """dev_planes_witness with the outputs in `want` (the others NULL) -> {name: host words}"""
    import torch
    d, W = pr.d, N // pr.L
    bufs = {"fc": dev(n=N * d, fill=-1), "f": dev(n=N * d, fill=-1), "w": dev(n=W * d, fill=-1)}
    torch.cuda.synchronize()
    c.dev_planes_witness(pr, planes, N, *[bufs[k] if k in want else None for k in ("fc", "f", "w")])
    c.sync()
    return {k: host(bufs[k]) for k in want}


def from_f_coeff(c, pr, fc_words, N):
    import torch
    d, W = pr.d, N // pr.L
    f, w = dev(n=N * d), dev(n=W * d)
    fc = dev(fc_words)
    torch.cuda.synchronize()
    c.dev_witness_from_f_coeff(pr, fc, N, f, w)
    c.sync()
    return host(f), host(w)


def scheme(c, A, kappa, N, d):
    return LA.AjtaiCommitmentScheme(c, device_tensor=dev(A), kappa=kappa, ncols=N, d=d)


def step_bufs(pr, W, kappa, acc_fc, acc_cm, w_ccs, rho):
    d, K, N = pr.d, pr.K, W * pr.L
    keep = {
        "w_ccs": dev(w_ccs), "acc_cm": dev(acc_cm), "acc_f_coeff": dev(acc_fc), "rho": dev(rho),
        "f_coeff": dev(n=N * d), "f": dev(n=N * d), "cm": dev(n=kappa * d),
        "wk": [dev(n=K * W * d) for _ in range(2)], "y": [dev(n=K * kappa * d) for _ in range(2)],
        "f0": dev(n=N * d), "f0_coeff": dev(n=N * d), "w_ccs0": dev(n=W * d), "cm0": dev(n=kappa * d),
        "planes": [dev(n=LA.fold_step_planes_len(pr, N)) for _ in range(2)],
    }
    b = LA.LfFoldStepBufs()
    for k, v in keep.items():
        if isinstance(v, list):
            for s in range(2):
                getattr(b, k)[s] = v[s].data_ptr()
        else:
            setattr(b, k, v.data_ptr())
    return keep, b


# ---------------------------------------------------------------- 1. pack
@pytest.mark.parametrize("d,N", SHAPES)
def test_pack_against_the_model_and_the_step(ctx, d, N):
    """K = 15: the model's bytes, and the bytes a lean step leaves: planes[0] for the same coefficients as
    its accumulator, planes[1] for the coefficients of the witness it made (its f_coeff output)"""
    import torch
    pr = params(d)
    K, W = pr.K, N // pr.L
    x = coeffs(d, N)
    want = pack_coeffs(x, d, K)
    assert want.size == LA.fold_step_planes_len(pr, N)
    got = host(pack(ctx, pr, x, N))
    assert np.array_equal(got, want)
    c = fresh_context()
    try:
        A = rand(KAPPA * N * d, 9100 + d + N)
        acc_fc = to_field(x).ravel()
        keep, b = step_bufs(pr, W, KAPPA, acc_fc, rand(KAPPA * d, 9101), rand(W * d, 9102 + d + N), make_rho(d, K, 9103))
        sch = scheme(c, A, KAPPA, N, d)
        torch.cuda.synchronize()
        c.dev_fold_step(sch, pr, W, b)
        c.sync()
        assert np.array_equal(host(keep["planes"][0]), got), "planes[0] of the step"
        made = host(keep["f_coeff"])
        assert np.array_equal(host(keep["planes"][1]), host(pack(c, pr, made, N, already_field=True))), "planes[1]"
        assert np.array_equal(host(keep["planes"][1]), pack_coeffs(signed(made).reshape(N, d), d, K))
    finally:
        c.close()


@pytest.mark.parametrize("d,N", [(24, 35), (64, 85), (1024, 5)])
def test_pack_with_fewer_planes(ctx, d, N):
    pr = params_k(d, SMALL_K)
    x = coeffs(d, N, SMALL_K)
    assert np.array_equal(host(pack(ctx, pr, x, N)), pack_coeffs(x, d, SMALL_K))


# ---------------------------------------------------------------- 2. overflow
@pytest.mark.parametrize("d,K", [(24, 15), (64, 15), (1024, 15), (4096, 15), (64, SMALL_K), (24, SMALL_K)])
def test_overflow(d, K):
    import torch
    pr = params_k(d, K)
    N = 5
    c = fresh_context()
    try:
        out = dev(n=LA.fold_step_planes_len(pr, N))
        for v, raises in ((1 << K, True), (-(1 << K), True), ((1 << K) - 1, False), (-(1 << K) + 1, False)):
            x = np.array(coeffs(d, N, K))
            x[N - 1, d - 1] = v
            fc = dev(to_field(x).ravel())  # -(2^K) goes in as the word p - 2^K
            torch.cuda.synchronize()
            c.dev_pack_planes(pr, fc, N, out)
            if raises:
                with pytest.raises(LA.LfError) as e:
                    c.sync()
                assert e.value.code == LF_ERR_DECOMPOSITION_OVERFLOW
            c.sync()  # once: the flag is cleared
    finally:
        c.close()


# ---------------------------------------------------------------- 3. the way back
@pytest.mark.parametrize("d,N", SHAPES)
def test_way_back(ctx, d, N):
    import torch
    pr = params(d)
    K = pr.K
    x = coeffs(d, N)
    fc = to_field(x).ravel()
    planes = pack(ctx, pr, x, N)
    got = witness(ctx, pr, planes, N)
    assert np.array_equal(got["fc"], fc)
    f, w = from_f_coeff(ctx, pr, fc, N)
    assert np.array_equal(got["f"], f) and np.array_equal(got["w"], w)
    for name in ("fc", "f", "w"):
        assert np.array_equal(witness(ctx, pr, planes, N, (name,))[name], got[name]), f"{name} alone"
    rows = dev(n=K * N * d)
    torch.cuda.synchronize()
    ctx.dev_expand_planes(pr, planes, N, rows, None)
    ctx.sync()
    total = sum(signed(host(rows)).reshape(K, N * d)[k] << k for k in range(K))
    assert np.array_equal(to_field(total), fc), "the recomposition of lf_dev_expand_planes's rows"


@pytest.mark.parametrize("d,N", [(64, 85), (1024, 5), (24, 35)])
def test_way_back_with_fewer_planes(ctx, d, N):
    pr = params_k(d, SMALL_K)
    x = coeffs(d, N, SMALL_K)
    got = witness(ctx, pr, pack(ctx, pr, x, N), N)
    f, w = from_f_coeff(ctx, pr, to_field(x).ravel(), N)
    assert np.array_equal(got["fc"], to_field(x).ravel()) and np.array_equal(got["f"], f) and np.array_equal(got["w"], w)


@pytest.mark.parametrize("d,N", [(24, 35), (4096, 5)])
def test_way_back_of_arbitrary_digits(ctx, d, N):
    """the per-plane formats with any digits in {-1, 0, 1} per plane: sum_k 2^k of the model's decode"""
    pr = params(d)
    K = pr.K
    dg = np.random.default_rng(9200 + d).integers(-1, 2, size=(K, N, d), dtype=np.int64)
    buf = pack_digits(dg, d)
    total = recompose(decode_planes(buf, d, K, N))
    assert np.array_equal(total, sum(dg[k] << k for k in range(K)))
    got = witness(ctx, pr, dev(buf), N)
    fc = to_field(total).ravel()
    assert np.array_equal(got["fc"], fc)
    assert np.array_equal(got["f"], O.crt(fc, d))
    assert np.array_equal(got["w"], O.witness_from_f(O.crt(fc, d), d, pr.B, pr.L)[1])


# ---------------------------------------------------------------- 4. check
@pytest.mark.parametrize("d,N", SHAPES)
def test_check_canonical_and_bound(ctx, d, N):
    pr = params(d)
    K = pr.K
    x = np.array(coeffs(d, N))
    x = np.clip(x, -1000, 1000)
    lo = 3 if N > 5 else 1
    x[lo, d // 2], x[N - 1, 2] = -1234, 1234  # the norm, at two elements
    planes = pack(ctx, pr, x, N)
    assert ctx.dev_planes_check(pr, planes, N) == (1234, LA.PLANES_OK, 0)
    assert ctx.dev_planes_check(pr, planes, N, 1234) == (1234, LA.PLANES_OK, 0)
    assert ctx.dev_planes_check(pr, planes, N, 1233) == (1234, LA.PLANES_BOUND, lo)
    assert ctx.dev_planes_check(pr, planes, N, 1 << 40)[1] == LA.PLANES_OK
    full = pack(ctx, pr, coeffs(d, N), N)
    assert ctx.dev_planes_check(pr, full, N) == ((1 << K) - 1, LA.PLANES_OK, 0)
    assert ctx.dev_planes_check(pr, full, N, (1 << K) - 2) == ((1 << K) - 1, LA.PLANES_BOUND, 0)


def tamper_cases():
    """(id, d, N, K, prepare(x), tamper(buf, e, N, K)): one per rule and format; buf is the planes as u64"""
    def halves(buf, N):
        return buf.view(np.uint16).reshape(N, -1)

    def zero0(x):
        x[:, 0] = 0

    def mag_bit(buf, e, N, K):
        halves(buf, N)[e, 1] |= 1 << K

    def neg_zero(buf, e, N, K):
        assert halves(buf, N)[e, 0] == 0  # coefficient 0 is the low half of word 0 at both formats
        halves(buf, N)[e, 0] = 0x8000

    def m24(buf, N, K):
        return buf.reshape(K, N)

    def prep24(x):
        x[:, 5], x[:, 7] = 2, -3

    def bit24(buf, e, N, K):
        m24(buf, N, K)[3, e] |= np.uint64(1 << 24)

    def bit56(buf, e, N, K):
        m24(buf, N, K)[K - 1, e] |= np.uint64(1 << 56)

    def sign_no_digit(buf, e, N, K):
        m24(buf, N, K)[0, e] |= np.uint64(1 << (32 + 5))  # +2: plane 0 has no digit

    def digit_no_sign(buf, e, N, K):
        m24(buf, N, K)[0, e] &= ~np.uint64(1 << (32 + 7))  # -3: plane 0's digit loses its sign

    def by(buf, N, K):
        return buf.view(np.uint8).reshape(N, K, 32, 32)

    def prep8(x):
        x[:, 40 + 1024 * 2] = 0  # quad a = 40 = 8 + 32 * 1, quarter 2

    def sign_differs(buf, e, N, K):
        by(buf, N, K)[e, 2, 3, 4] ^= 0x20

    def sign_on_zero(buf, e, N, K):
        by(buf, N, K)[e, :, 8, 1] |= 0x40

    return [("sm16p2-magnitude-bit-K", 64, 85, SMALL_K, None, mag_bit), ("sm16p2-negative-zero", 64, 85, 15, zero0, neg_zero),
            ("sm1024-magnitude-bit-K", 1024, 5, SMALL_K, None, mag_bit), ("sm1024-negative-zero", 1024, 5, 15, zero0, neg_zero),
            ("mask24-bit-24", 24, 35, 15, prep24, bit24), ("mask24-bit-56", 24, 35, 15, prep24, bit56),
            ("mask24-sign-without-digit", 24, 35, 15, prep24, sign_no_digit),
            ("mask24-digit-without-sign", 24, 35, 15, prep24, digit_no_sign),
            ("sm8-sign-differs-on-a-plane", 4096, 5, 15, prep8, sign_differs),
            ("sm8-sign-on-a-zero-quarter", 4096, 5, 15, prep8, sign_on_zero)]


@pytest.mark.parametrize("case", tamper_cases(), ids=lambda c: c[0])
def test_check_finds_tampering(ctx, case):
    _, d, N, K, prepare, tamper = case
    pr = params_k(d, K)
    x = np.array(coeffs(d, N, K))
    if prepare:
        prepare(x)
    clean = pack_coeffs(x, d, K)
    norm = int(np.abs(x).max())
    assert ctx.dev_planes_check(pr, dev(clean), N) == (norm, LA.PLANES_OK, 0)
    for where in ((0,), (N - 1,), (N - 2, 2)):
        buf = clean.copy()
        for e in where:
            tamper(buf, e, N, K)
        assert not np.array_equal(buf, clean)
        model = recompose(decode_any(buf, d, K, N))
        assert not np.array_equal(pack_coeffs(model, d, K), buf), "the tampered bytes are no fixed point"
        t = dev(buf)
        got = ctx.dev_planes_check(pr, t, N)
        assert got == (int(np.abs(model).max()), LA.PLANES_ENCODING, min(where)), where
        # an encoding fault comes before a bound fault
        assert ctx.dev_planes_check(pr, t, N, 1)[1:] == (LA.PLANES_ENCODING, min(where))
        assert np.array_equal(witness(ctx, pr, t, N, ("fc",))["fc"], to_field(model).ravel())


# ---------------------------------------------------------------- 5. no state
def entries_outputs(c, d, N):
    pr = params(d)
    x = coeffs(d, N)
    planes = pack(c, pr, x, N)
    got = witness(c, pr, planes, N)
    return [host(planes), got["fc"], got["f"], got["w"], np.array(c.dev_planes_check(pr, planes, N, 100), np.uint64)]


def test_reads_no_state_and_leaves_none():
    """a lean lf_dev_decompose_commit at d = 64, the three entries on buffers of other rings, then
    lf_dev_fold_combine: every output of the step is the oracle's, and the entries give a fresh context's bits"""
    import torch
    d, W = 64, 17
    pr = params(d)
    K, N = pr.K, W * pr.L
    A = rand(KAPPA * N * d, 9300)
    acc_fc, acc_f = O.witness_from_w_ccs(rand(W * d, 9301), d, pr.B, pr.L)
    wi_fc, wi_f = O.witness_from_w_ccs(rand(W * d, 9302), d, pr.B, pr.L)
    acc_cm, cm_i = O.ajtai_commit(A, KAPPA, N, d, acc_f), O.ajtai_commit(A, KAPPA, N, d, wi_f)
    rho = make_rho(d, K, 9303)
    want, sides = oracle_fold_hot(A, KAPPA, d, pr, acc_cm, acc_fc, cm_i, wi_fc, rho)
    a, b = fresh_context(), fresh_context()
    try:
        fresh = [entries_outputs(a, dd, NN) for dd, NN in ((24, 35), (1024, 5), (64, 85))]
        sch = scheme(b, A, KAPPA, N, d)
        keep, bufs = step_bufs(pr, W, KAPPA, acc_fc, acc_cm, np.zeros(W * d, np.uint64), rho)
        keep["f_coeff"].copy_(dev(wi_fc))
        keep["cm"].copy_(dev(cm_i))
        torch.cuda.synchronize()
        b.check(b.lib.lf_dev_decompose_commit(b.h, sch.h, C.byref(pr), W, C.byref(bufs)))
        used = [entries_outputs(b, dd, NN) for dd, NN in ((24, 35), (1024, 5), (64, 85))]
        b.check(b.lib.lf_dev_fold_combine(b.h, sch.h, C.byref(pr), W, C.byref(bufs)))
        b.sync()
        for x, z in zip(fresh, used):
            for u, v in zip(x, z):
                assert np.array_equal(u, v)
        assert np.array_equal(np.concatenate([host(t) for t in keep["y"]]), want["y"]), "y"
        for key in ("f0", "f0_coeff", "w_ccs0", "cm0"):
            assert np.array_equal(host(keep[key]), want[key]), key
        for s in range(2):
            assert np.array_equal(host(keep["wk"][s]), sides[s][2]), f"wk[{s}]"
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 6. the chain closes
def sparse_rho(d, K, seed):
    """2K challenges with one or two nonzero coefficients in {-1, 1} each, in NTT form"""
    rng = np.random.default_rng(seed)
    rc = np.zeros((2 * K, d), np.int64)
    for i in range(2 * K):
        pos = rng.choice(d, size=1 + i % 2, replace=False)
        rc[i, pos] = rng.integers(0, 2, size=pos.size) * 2 - 1
    return O.crt(to_field(rc).ravel(), d)


@pytest.mark.parametrize("d,W", [(24, 3), (64, 17)])
def test_the_chain_closes(d, W):
    """pack both sides, fold and commit their planes, pack f0_coeff as the next planes0 and fold again with
    a fresh side 1, on a context that never runs a step: both folds are the oracle's fold() run twice"""
    import torch
    pr = params(d)
    K, N, kd = pr.K, W * pr.L, KAPPA * d
    A = rand(KAPPA * N * d, 9400 + d)
    rng = np.random.default_rng(9401 + d)
    fcs = [to_field(rng.integers(-(1 << 14), (1 << 14) + 1, size=(N, d), dtype=np.int64)).ravel() for _ in range(3)]
    cms = [O.ajtai_commit(A, KAPPA, N, d, O.crt(fc, d)) for fc in fcs]
    rhos = [sparse_rho(d, K, 9402 + d), sparse_rho(d, K, 9403 + d)]
    want1, _ = oracle_fold_hot(A, KAPPA, d, pr, cms[0], fcs[0], cms[1], fcs[1], rhos[0])
    assert np.abs(signed(want1["f0_coeff"])).max() <= 60
    want2, _ = oracle_fold_hot(A, KAPPA, d, pr, want1["cm0"], want1["f0_coeff"], cms[2], fcs[2], rhos[1])
    assert np.abs(signed(want2["f0_coeff"])).max() <= 60
    c = fresh_context()
    try:
        sch = scheme(c, A, KAPPA, N, d)

        def fold(planes0, planes1, rho, want, cm1_want):
            r = dev(rho)
            f0c, f0, w0 = dev(n=N * d), dev(n=N * d), dev(n=W * d)
            y = [dev(n=K * kd) for _ in range(2)]
            cm1, cm0 = dev(n=kd), dev(n=kd)
            torch.cuda.synchronize()
            c.dev_fold_planes(pr, planes0, planes1, N, r, f0c, f0, w0)
            c.dev_commit_planes(sch, pr, [planes0, planes1], N, y, [None, cm1])
            rows = (C.c_void_p * (2 * K))(*[y[s].data_ptr() + 8 * k * kd for s in range(2) for k in range(K)])
            c.check(c.lib.lf_dev_fold(c.h, d, r.data_ptr(), rows, 2 * K, KAPPA, cm0.data_ptr()))
            c.sync()
            assert np.array_equal(host(f0), want["f0"]) and np.array_equal(host(f0c), want["f0_coeff"])
            assert np.array_equal(host(w0), want["w_ccs0"])
            assert np.array_equal(np.concatenate([host(t) for t in y]), want["y"]), "y"
            assert np.array_equal(host(cm0), want["cm0"]), "cm_0"
            assert np.array_equal(host(cm1), cm1_want), "cm of side 1"
            return f0c

        p0, p1 = (pack(c, pr, fc, N, already_field=True) for fc in fcs[:2])
        f0c = fold(p0, p1, rhos[0], want1, cms[1])
        next0 = dev(n=LA.fold_step_planes_len(pr, N), fill=-1)
        c.dev_pack_planes(pr, f0c, N, next0)  # the accumulator's planes, from the device buffer the fold wrote
        p2 = pack(c, pr, fcs[2], N, already_field=True)
        fold(next0, p2, rhos[1], want2, cms[2])
    finally:
        c.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    c = fresh_context()
    try:
        buf = dev(n=1 << 16).data_ptr()
        norm, fault, where = C.c_uint64(0), C.c_int(0), C.c_size_t(0)
        L = c.lib

        def pack_rc(pr, N, fc=buf, pl=buf):
            return L.lf_dev_pack_planes(c.h, C.byref(pr), fc, N, pl)

        def wit_rc(pr, N, pl=buf, fc=buf, f=buf, w=buf):
            return L.lf_dev_planes_witness(c.h, C.byref(pr), pl, N, fc, f, w)

        def chk_rc(pr, N, pl=buf, n=C.byref(norm), f=C.byref(fault), wh=C.byref(where)):
            return L.lf_dev_planes_check(c.h, C.byref(pr), pl, N, 0, n, f, wh)

        p4 = params(64)
        p4.b_small, p4.K = 4, 8
        for pr in (params(2048), p4, params_k(64, 16)):
            for entry in (pack_rc, wit_rc, chk_rc):
                assert entry(pr, 5) == LF_ERR_UNSUPPORTED_RING
        pr = params(64)
        assert pr.L == 5
        for entry in (pack_rc, wit_rc, chk_rc):
            assert entry(pr, 7) == LF_ERR_INCORRECT_LENGTH
            assert entry(pr, 0) == LF_ERR_INCORRECT_LENGTH
        assert pack_rc(pr, 5, fc=None) == LF_ERR_INVALID_ARG and pack_rc(pr, 5, pl=None) == LF_ERR_INVALID_ARG
        assert wit_rc(pr, 5, pl=None) == LF_ERR_INVALID_ARG
        assert wit_rc(pr, 5, fc=None, f=None, w=None) == LF_ERR_INVALID_ARG
        assert chk_rc(pr, 5, pl=None) == LF_ERR_INVALID_ARG
        for kw in ({"n": None}, {"f": None}, {"wh": None}):
            assert chk_rc(pr, 5, **kw) == LF_ERR_INVALID_ARG
        with pytest.raises(LA.LfError) as e:  # the wrapper raises on a refusal
            c.dev_planes_check(params(2048), buf, 5)
        assert e.value.code == LF_ERR_UNSUPPORTED_RING
        c.sync()
        # the context is usable afterwards
        x = coeffs(64, 5)
        assert np.array_equal(host(pack(c, pr, x, 5)), pack_coeffs(x, 64, pr.K))
    finally:
        c.close()
