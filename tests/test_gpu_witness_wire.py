"""Witness::from_f_coeff at every ring and the packed witness (include/lf.h, "witness wire
format") on the device, against the CPU oracle: f = O.crt(f_coeff), w_ccs =
O.gadget_recompose(f). Inputs are seeded full-range residues with the edge values of the
three packed widths written at the ends of the first and last element and around d / 2
(and around 1024 at d = 4096, where a quarter ends).

Launch forms: only d = 1024 has two for canonical words (one half-wave per group at
W >= witness_split_w(), one per (group, part) below it); both sides of that threshold
are run. d = 4096, d = 24 and the LDS-transform rings have one kernel each, and every
packed source has one kernel per ring."""
import functools
import struct

import numpy as np
import pytest

import latticeum_amd as LA
import nifs as NF
import oracle as O
from latticeum_amd import wire

pytestmark = pytest.mark.gpu

P = O.P
HALF = (P - 1) // 2
OVERFLOW, INVALID_ARG, INCORRECT_LENGTH, UNSUPPORTED_RING = 6, 1, 7, 2  # lf.h
RINGS = [24, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
EDGES = [0, 1, P - 1, 1 << 14, P - (1 << 14), (1 << 15) - 1, P - (1 << 15), 1 << 15, (1 << 31) - 1, P - (1 << 31),
         1 << 31, HALF, HALF + 1]
DTYPES = {16: "<i2", 32: "<i4", 64: "<u8"}


# The context runs on a non-blocking stream of its own: every buffer torch makes is
# finished (synchronize) before a library call may touch it.
def dev(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_bytes(words):
    """canonical or not: the u64 words as a device byte buffer (a 64-bit payload)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def ones(n):
    """n words of 0xFF bytes"""
    import torch
    t = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")[:n]
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().view(np.uint64)


def centred(fc):
    """the signed representatives of canonical words, as int64"""
    fc = np.asarray(fc, np.uint64)
    out = fc.copy()
    neg = fc > np.uint64(HALF)
    out[neg] = fc[neg] - np.uint64(P)  # wraps to the two's complement of x - p
    return out.view(np.int64)


def edge_positions(d, N):
    cs = [0, d - 1, d // 2 - 1, d // 2] + ([1023, 1024] if d == 4096 else [])
    return [(e, c) for e in sorted({0, N - 1}) for c in cs]


def with_edges(fc, d, edges, shift):
    """every edge once in a run inside the first element, then the edges in turn at the positions"""
    N = fc.size // d
    fc = fc.reshape(N, d)
    run = edges[:d - 2]
    fc[0, 1:1 + len(run)] = run
    for i, (e, c) in enumerate(edge_positions(d, N)):
        fc[e, c] = edges[(i + shift) % len(edges)]
    return fc.reshape(-1)


def params(d, B=None, L=None):
    pr = LA.goldilocks_dp(d)
    if B:
        pr.B, pr.L = B, L
    return pr


def oracle_from_f_coeff(fc, pr):
    f = O.crt(fc, pr.d)
    return f, O.gadget_recompose(f, pr.d, pr.B, pr.L)


@functools.lru_cache(maxsize=None)
def case(d, W, bits=64):
    """(f_coeff, f, w_ccs) of W groups whose coefficients fit `bits` (64: any residue); read only"""
    pr = params(d)
    n = W * pr.L * d
    fc = O.fill_uniform(n, 1000 + d + W)
    edges = EDGES
    if bits < 64:
        lim = 1 << (bits - 1)
        fc = (fc % np.uint64(2 * lim)).astype(np.int64) - lim          # [-lim, lim - 1]
        fc = np.where(fc < 0, fc.astype(np.uint64) + np.uint64(P), fc.astype(np.uint64)).astype(np.uint64)
        edges = [x for x in EDGES if -lim <= (x if x <= HALF else x - P) < lim] + [lim - 1, P - lim]
    fc = with_edges(fc, d, edges, W)
    f, w = oracle_from_f_coeff(fc, pr)
    for a in (fc, f, w):
        a.setflags(write=False)
    return fc, f, w


@pytest.fixture(scope="module")
def ctx():
    c = LA.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1. from_f_coeff against the oracle
@pytest.mark.parametrize("W", [1, 2, 17])
@pytest.mark.parametrize("d", RINGS)
def test_from_f_coeff_matches_oracle(ctx, d, W):
    pr = params(d)
    N = W * pr.L
    fc, f, w = case(d, W)
    fcd, fd, wd = dev(fc), ones(N * d), ones(W * d)
    ctx.dev_witness_from_f_coeff(pr, fcd, N, fd, wd)
    ctx.sync()
    assert np.array_equal(host(fd), f), "f"
    assert np.array_equal(host(wd), w), "w_ccs"
    assert np.array_equal(host(fcd), fc), "f_coeff is left unchanged"


@pytest.mark.parametrize("d", [24, 64, 1024, 4096])
def test_from_f_coeff_other_base(ctx, d):
    """B = 2^12, L = 3: the recomposition's general step (GoldiLocksDP's B = 2^15 has a form of its own)"""
    pr = params(d, 1 << 12, 3)
    W = 3
    N = W * pr.L
    fc = with_edges(O.fill_uniform(N * d, 77 + d), d, EDGES, 5)
    f, w = oracle_from_f_coeff(fc, pr)
    fd, wd = ones(N * d), ones(W * d)
    ctx.dev_witness_from_f_coeff(pr, dev(fc), N, fd, wd)
    ctx.sync()
    assert np.array_equal(host(fd), f) and np.array_equal(host(wd), w)


@pytest.mark.parametrize("side", ["below", "at"])
def test_from_f_coeff_d1024_both_launch_forms(ctx, side):
    """W = witness_split_w() - 1 (one half-wave per (group, part)) and W = witness_split_w() (one per
    group): the oracle on a seeded sample of 32 groups with the first and the last, and every group
    through Witness::from_f of the result, which must return the input f_coeff and the same w_ccs"""
    import torch
    d, pr = 1024, params(1024)
    W = LA.witness_split_w() - (1 if side == "below" else 0)
    N = W * pr.L
    fc = with_edges(O.fill_uniform(N * d, 4242 + W), d, EDGES, 3)
    fcd, fd, wd = dev(fc), ones(N * d), ones(W * d)
    ctx.dev_witness_from_f_coeff(pr, fcd, N, fd, wd)
    ctx.sync()
    rng = np.random.default_rng(W)
    groups = sorted({0, W - 1} | set(rng.choice(W, 30, replace=False).tolist()))
    assert len(groups) <= 32
    fh, wh = host(fd).reshape(W, pr.L * d), host(wd).reshape(W, d)
    fcg = fc.reshape(W, pr.L * d)
    for g in groups:
        f, w = oracle_from_f_coeff(fcg[g], pr)
        assert np.array_equal(fh[g], f) and np.array_equal(wh[g], w), g
    fc2, w2 = ones(N * d), ones(W * d)
    ctx.check(ctx.lib.lf_dev_witness_from_f(ctx.h, LA._lib.C.byref(pr), fd.data_ptr(), N, fc2.data_ptr(), w2.data_ptr()))
    ctx.sync()
    assert torch.equal(fc2, fcd) and torch.equal(w2, wd)


def test_from_f_coeff_errors(ctx):
    pr = params(24)
    buf = ones(10 * 24)
    call = lambda p, N, a=buf, b=buf, c=buf: ctx.lib.lf_dev_witness_from_f_coeff(
        ctx.h, LA._lib.C.byref(p), a.data_ptr() if a is not None else None, N,
        b.data_ptr() if b is not None else None, c.data_ptr() if c is not None else None)
    assert call(pr, 7) == INCORRECT_LENGTH
    assert call(params(48), 5) == UNSUPPORTED_RING
    assert call(pr, 5, a=None) == INVALID_ARG and call(pr, 5, b=None) == INVALID_ARG and call(pr, 5, c=None) == INVALID_ARG
    assert ctx.lib.lf_dev_witness_from_f_coeff(None, LA._lib.C.byref(pr), buf.data_ptr(), 5, buf.data_ptr(),
                                               buf.data_ptr()) == INVALID_ARG


# ---------------------------------------------------------------- 2. the host entry, Montgomery words
@pytest.mark.parametrize("d", [24, 64])
def test_host_entry_montgomery(ctx, d):
    pr = params(d)
    fc, f, w = case(d, 2)
    mont = np.vectorize(O.to_mont, otypes=[np.uint64])
    gf, gw = ctx.witness_from_f_coeff(fc, pr)
    assert np.array_equal(gf, f) and np.array_equal(gw, w)
    mf, mw = ctx.witness_from_f_coeff(mont(fc), pr, LA.REPR_MONTGOMERY)
    assert np.array_equal(mf, mont(f)) and np.array_equal(mw, mont(w))


# ---------------------------------------------------------------- 3. the width probe
BITS_CASES = [((1 << 15) - 1, 16), (1 << 15, 32), (-(1 << 15), 16), (-(1 << 15) - 1, 32),
              ((1 << 31) - 1, 32), (1 << 31, 64), (-(1 << 31), 32), (-(1 << 31) - 1, 64)]


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("extreme,want", BITS_CASES)
def test_witness_bits(ctx, extreme, want, where):
    d, N = 24, 7
    small = (O.fill_uniform(N * d, 5) % np.uint64(201)).astype(np.int64) - 100
    small[0 if where == "first" else N * d - 1] = extreme
    u = small.astype(np.uint64)  # a negative x wraps to 2^64 - |x|, and + p wraps back to p - |x|
    fc = np.where(small < 0, u + np.uint64(P), u)
    bits, norm = ctx.dev_witness_bits(d, dev(fc), N)
    assert bits == want
    assert norm == int(np.abs(centred(fc)).max()) == abs(extreme)


def test_witness_bits_zero_and_half(ctx):
    assert ctx.dev_witness_bits(64, dev(np.zeros(64 * 5, np.uint64)), 5) == (16, 0)
    fc = np.zeros(16 * 5, np.uint64)
    fc[17] = HALF + 1  # the most negative representative
    assert ctx.dev_witness_bits(16, dev(fc), 5) == (64, HALF)


# ---------------------------------------------------------------- 4. pack then unpack
def packed_buf(nbytes):
    """nbytes of 0xFF and 64 guard bytes behind them"""
    import torch
    t = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("W", [1, 17])
@pytest.mark.parametrize("d", [24, 64, 1024, 2048, 4096])
@pytest.mark.parametrize("bits", [16, 32, 64])
def test_pack_unpack(ctx, bits, d, W):
    pr = params(d)
    N = W * pr.L
    fc, f, w = case(d, W, bits)
    nbytes = N * d * bits // 8
    assert ctx.lib.lf_witness_packed_len(d, N, bits) == nbytes
    fcd, pk = dev(fc), packed_buf(nbytes)
    ctx.dev_witness_pack(d, fcd, N, bits, pk)
    ctx.sync()
    raw = pk.cpu().numpy()
    assert (raw[nbytes:] == 0xFF).all(), "pack wrote past the payload"
    vals = np.frombuffer(raw[:nbytes].tobytes(), DTYPES[bits])
    assert np.array_equal(vals.astype(np.int64) if bits < 64 else vals, centred(fc) if bits < 64 else fc)
    # all three forms, into buffers of 0xFF with a guard element behind each
    fc2, f2, w2 = ones((N + 1) * d), ones((N + 1) * d), ones((W + 1) * d)
    ctx.dev_witness_unpack(pr, pk, bits, N, fc2, f2, w2)
    ctx.sync()
    for got, want, what in ((fc2, fc, "f_coeff"), (f2, f, "f"), (w2, w, "w_ccs")):
        g = host(got)
        assert np.array_equal(g[:want.size], want), what
        assert (g[want.size:] == np.uint64((1 << 64) - 1)).all(), what + " guard"
    # bit for bit what from_f_coeff gives on that f_coeff
    f3, w3 = ones(N * d), ones(W * d)
    ctx.dev_witness_from_f_coeff(pr, fcd, N, f3, w3)
    ctx.sync()
    assert np.array_equal(host(f3), host(f2)[:N * d]) and np.array_equal(host(w3), host(w2)[:W * d])
    # f and w_ccs NULL: f_coeff alone
    fc4 = ones((N + 1) * d)
    ctx.dev_witness_unpack(pr, pk, bits, N, fc4)
    ctx.sync()
    g = host(fc4)
    assert np.array_equal(g[:N * d], fc) and (g[N * d:] == np.uint64((1 << 64) - 1)).all()


@pytest.mark.parametrize("d", [24, 64, 1024, 4096])
@pytest.mark.parametrize("bits", [16, 32])
def test_pack_overflow_one_step_outside(ctx, bits, d):
    pr = params(d)
    N = pr.L
    lim = 1 << (bits - 1)
    for x in (lim, P - lim - 1):  # lim and -lim - 1
        fc = case(d, 1, bits)[0].copy()
        fc[N * d - 1] = x
        pk = packed_buf(N * d * bits // 8)
        ctx.dev_witness_pack(d, dev(fc), N, bits, pk)
        with pytest.raises(LA.LfError) as e:
            ctx.sync()
        assert e.value.code == OVERFLOW
    ctx.sync()  # the flag was cleared
    for x in (lim - 1, P - lim):  # the ends of the range fit
        fc = case(d, 1, bits)[0].copy()
        fc[N * d - 1] = x
        ctx.dev_witness_pack(d, dev(fc), N, bits, packed_buf(N * d * bits // 8))
        ctx.sync()


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("d", [24, 64, 1024, 4096])
def test_unpack_64_refuses_a_word_not_below_p(ctx, d, full):
    pr = params(d)
    N = pr.L
    for x in (P, (1 << 64) - 1):
        words = case(d, 1)[0].copy()
        words[N * d - 3] = x
        pk = dev_bytes(words)
        fc2, f2, w2 = ones(N * d), ones(N * d), ones(d)
        ctx.dev_witness_unpack(pr, pk, 64, N, fc2, *((f2, w2) if full else ()))
        with pytest.raises(LA.LfError) as e:
            ctx.sync()
        assert e.value.code == OVERFLOW
    words = case(d, 1)[0].copy()
    words[N * d - 3] = P - 1
    ctx.dev_witness_unpack(pr, dev_bytes(words), 64, N, ones(N * d))
    ctx.sync()


def test_pack_unpack_errors(ctx):
    pr = params(24)
    buf, pk = ones(5 * 24), packed_buf(5 * 24 * 8)
    lib, ref = ctx.lib, LA._lib.C.byref
    assert lib.lf_dev_witness_pack(ctx.h, 48, buf.data_ptr(), 5, 16, pk.data_ptr()) == UNSUPPORTED_RING
    assert lib.lf_dev_witness_pack(ctx.h, 24, buf.data_ptr(), 5, 8, pk.data_ptr()) == INVALID_ARG
    assert lib.lf_dev_witness_pack(ctx.h, 24, buf.data_ptr(), 5, 16, pk.data_ptr() + 8) == INVALID_ARG
    assert lib.lf_dev_witness_pack(ctx.h, 24, None, 5, 16, pk.data_ptr()) == INVALID_ARG
    assert lib.lf_dev_witness_unpack(ctx.h, ref(pr), pk.data_ptr(), 16, 7, buf.data_ptr(), None, None) == INCORRECT_LENGTH
    assert lib.lf_dev_witness_unpack(ctx.h, ref(pr), pk.data_ptr(), 24, 5, buf.data_ptr(), None, None) == INVALID_ARG
    assert lib.lf_dev_witness_unpack(ctx.h, ref(pr), pk.data_ptr(), 16, 5, buf.data_ptr(), buf.data_ptr(), None) == INVALID_ARG
    assert lib.lf_dev_witness_unpack(ctx.h, ref(params(48)), pk.data_ptr(), 16, 5, buf.data_ptr(), None, None) == UNSUPPORTED_RING


# ---------------------------------------------------------------- 5. the format, read without the unpacker
@pytest.mark.parametrize("d", [24, 128])
@pytest.mark.parametrize("fits", [16, 32, 64])
def test_wire_bytes_field_by_field(ctx, d, fits):
    pr = params(d)
    W = 3
    N = W * pr.L
    fc = case(d, W, fits)[0]
    wit = {"w_ccs": 0, "f": 0, "f_coeff": dev(fc)}  # only f_coeff is read
    narrowest = ctx.dev_witness_bits(d, wit["f_coeff"], N)[0]
    assert narrowest == fits  # the case holds the ends of its own range
    for bits in (0, 16, 32, 64):
        eff = bits or narrowest
        if eff < fits:
            with pytest.raises(wire.LfError) as e:
                wire.serialize_witness(ctx, pr, wit, N, bits)
            assert e.value.code == OVERFLOW
            continue
        data = wire.serialize_witness(ctx, pr, wit, N, bits)
        assert len(data) == 32 + N * d * eff // 8
        assert data[:4] == b"LFW1"
        assert struct.unpack("<IIIQQ", data[4:32]) == (d, pr.L, eff, N, 0)
        assert wire.witness_wire_header(data) == {"d": d, "L": pr.L, "bits": eff, "N": N}
        vals = np.frombuffer(data[32:], DTYPES[eff])
        assert vals.size == N * d
        if eff == 64:
            assert np.array_equal(vals, fc)
        else:
            assert np.array_equal(vals.astype(np.int64), centred(fc))
    # the size query alone
    n = LA._lib.C.c_size_t()
    w = LA._lib.LfWitness(0, 0, wit["f_coeff"].data_ptr())
    rc = ctx.lib.lf_witness_serialize(ctx.h, LA._lib.C.byref(pr), LA._lib.C.byref(w), N, 0, None, 0, LA._lib.C.byref(n))
    assert rc == INCORRECT_LENGTH and n.value == 32 + N * d * fits // 8


# ---------------------------------------------------------------- 6. serialize then deserialize
def fresh(N, W, d):
    return {"w_ccs": ones(W * d), "f": ones(N * d), "f_coeff": ones(N * d)}


@pytest.mark.parametrize("d", [24, 256])
def test_serialize_deserialize(ctx, d):
    pr = params(d)
    W = 17
    N = W * pr.L
    for fits in (16, 32, 64):
        fc, f, w = case(d, W, fits)
        src = {"w_ccs": 0, "f": 0, "f_coeff": dev(fc)}
        for bits in sorted({0, fits, 64}):  # the narrowest and any wider valid width
            data = wire.serialize_witness(ctx, pr, src, N, bits)
            out = fresh(N, W, d)
            wire.deserialize_witness(ctx, pr, data, out, N)
            assert np.array_equal(host(out["f_coeff"]), fc), (fits, bits)
            assert np.array_equal(host(out["f"]), f) and np.array_equal(host(out["w_ccs"]), w), (fits, bits)
    fc = case(d, W, 64)[0]
    data = wire.serialize_witness(ctx, pr, {"w_ccs": 0, "f": 0, "f_coeff": dev(fc)}, N, 64)
    out = fresh(N, W, d)

    def code(blob, p=pr, n=N):
        with pytest.raises(wire.LfError) as e:
            wire.deserialize_witness(ctx, p, blob, out, n)
        return e.value.code

    assert code(data[:-8]) == INCORRECT_LENGTH                     # a truncated payload
    assert code(data[:40]) == INCORRECT_LENGTH
    assert code(data, p=params(64 if d != 64 else 32)) == INVALID_ARG   # d differs from the params
    assert code(data, p=params(d, 1 << 15, 1)) == INVALID_ARG      # L differs
    assert code(data, n=N + pr.L) == INVALID_ARG                   # N differs
    untouched = all((host(t) == np.uint64((1 << 64) - 1)).all() for t in out.values())
    assert untouched, "malformed input launched something"
    for x in (P, (1 << 64) - 1):                                   # a 64-bit word that is no residue
        bad = bytearray(data)
        struct.pack_into("<Q", bad, 32 + 8 * (N * d - 2), x)
        assert code(bytes(bad)) == INVALID_ARG
    wire.deserialize_witness(ctx, pr, data, out, N)                # the context is still good
    assert np.array_equal(host(out["f_coeff"]), fc)


# ---------------------------------------------------------------- 7. resume a chain from its wire bytes
def test_resume_from_wire_bytes():
    """the small Phi_72 fold shape of test_gpu_fold_prove: two steps in a row, against one step,
    the accumulator and its witness through their wire bytes into fresh buffers, lcccs_check, and
    the second step from the restored state: the same second proof and accumulator, byte for byte"""
    from test_gpu_fold_prove import acc_dict, dev_wit, flat, setup, witness
    from test_wire_proof import to_bytes

    d, W, l, t, deg, kappa = 24, 5, 2, 4, 2, 3
    ctx = LA.Context(0)
    try:
        pr_o, ccs, A, prover = setup(ctx, d, W, l, t, deg, kappa, 7 + d + W)
        pr = prover.pr
        Nn = W * pr_o.L
        xa, Wa = witness(ccs, pr_o, 11)
        cma = O.ajtai_commit(A, kappa, Nn, d, Wa.f)
        acc0 = acc_dict(NF.linearize_fresh(ccs, cma, xa, Wa, pr_o))
        steps = []
        for seed in (12, 13):
            x, Wi = witness(ccs, pr_o, seed)
            steps.append((O.ajtai_commit(A, kappa, Nn, d, Wi.f), flat(x), Wi))
        zeros = lambda: {"w_ccs": ones(W * d), "f": ones(Nn * d), "f_coeff": ones(Nn * d)}

        class Shape:  # what test_wire_proof.to_bytes reads
            pass
        sh = Shape()
        sh.d, sh.K, sh.s, sh.lin_evals, sh.fold_evals = d, pr.K, prover.s, deg + 2, 2 * pr.b_small + 1

        def lcccs_bytes(a):
            return wire.serialize_lcccs(d, a["r"], a["v"], a["cm"], a["u"], a["x_w"], a["h"])

        # the uninterrupted chain
        w1, w2 = zeros(), zeros()
        acc1, pf1 = prover.fold_prove(acc0, dev_wit(Wa), steps[0][0], steps[0][1], dev_wit(steps[0][2]), w1)
        acc2, pf2 = prover.fold_prove(acc1, w1, steps[1][0], steps[1][1], dev_wit(steps[1][2]), w2)
        # one step, then the state through its bytes
        v1 = zeros()
        bcc1, _ = prover.fold_prove(acc0, dev_wit(Wa), steps[0][0], steps[0][1], dev_wit(steps[0][2]), v1)
        acc_b, wit_b = lcccs_bytes(bcc1), wire.serialize_witness(ctx, pr, v1, Nn)
        assert wire.witness_wire_header(wit_b)["bits"] == ctx.dev_witness_bits(d, v1["f_coeff"], Nn)[0]
        del v1, bcc1
        racc = wire.deserialize_lcccs(acc_b, d)
        rw = zeros()
        wire.deserialize_witness(ctx, pr, wit_b, rw, Nn)
        for k in rw:
            assert np.array_equal(host(rw[k]), host(w1[k])), k
        prover.check_lcccs(racc, rw)  # raises unless the restored witness opens the restored accumulator
        r2 = zeros()
        racc2, rpf2 = prover.fold_prove(racc, rw, steps[1][0], steps[1][1], dev_wit(steps[1][2]), r2)
        assert to_bytes(rpf2, sh) == to_bytes(pf2, sh)
        assert lcccs_bytes(racc2) == lcccs_bytes(acc2)
        for k in r2:
            assert np.array_equal(host(r2[k]), host(w2[k])), k
    finally:
        ctx.close()
