"""Directed carry-edge tests of the device Goldilocks arithmetic (csrc/gl.hpp and its users
in slot.hpp, ring.hpp, ntt32.hpp).

Part one drives every primitive through lf_dev_gl_probe over the vector sets of
oracle/gl_model.py -- the sets its branch census counted -- bit-exact against plain % p on
Python integers (congruent for the ops whose contract is "weakly reduced").

Part two feeds the production kernels, where the same primitives are inlined and folded
differently, inputs drawn from the edge set, against the CPU oracle (plain 128-bit % p).
Every comparison is exact."""
import numpy as np
import pytest

import gl_model as G
import latticeum_amd as LA
import oracle as O

pytestmark = pytest.mark.gpu
P = LA.P
ALL_D = [24, 16, 64, 256, 1024, 4096]
CAN, ANY = (np.array(v, np.uint64) for v in G.edge_values())


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def dev(x=None, n=None):
    import torch
    if x is not None:
        return torch.from_numpy(np.ascontiguousarray(x, np.uint64).view(np.int64)).cuda()
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def edge_fill(n, seed, pool=CAN):
    """n words, each drawn from the canonical edge set by a seeded generator"""
    return pool[np.random.default_rng(seed).integers(0, len(pool), n)]


def tb_of(d):
    return 3 if d == 24 else 1


# ------------------------------------------------------------------ 4a: the probe
@pytest.fixture(scope="module")
def model():
    """the vector sets with their integer references, and the census that counted them"""
    count, bad, flags = G.census()
    assert not bad
    return list(zip(G.vector_sets(), G.expected())), count


@pytest.mark.parametrize("op", list(G.OPS))
def test_probe_matches_integers(ctx, model, op):
    sets, count = model
    ran = 0
    for vs, want in sets:
        if vs.op != op:
            continue
        # the probe's blocks are 64 threads: every set but the few 4096-product runs spans several
        # blocks and ends inside one
        assert (vs.n > 64 and vs.n % 64) or vs.m == 4096, (vs.n, vs.m)
        got = ctx.gl_probe(G.OPS[op], np.array(vs.a, np.uint64), None if vs.b is None else np.array(vs.b, np.uint64),
                           s=vs.s, m=vs.m)
        assert got.size == vs.n * vs.w
        if op in G.WEAK_OPS:  # any u64 congruent to the value
            red = [int(v) % P for v in got]
            assert red == want, (op, vs.s, vs.m, next(i for i in range(vs.n) if red[i] != want[i]))
        else:
            flat = np.array(want, np.uint64).ravel()
            assert np.array_equal(got, flat), (op, vs.s, vs.m, int(np.flatnonzero(got != flat)[0]) // vs.w)
        ran += vs.n
    assert ran == count[op] > 0  # what the census counted is what ran


def test_probe_rejects_what_it_does_not_know(ctx):
    a = np.zeros(8, np.uint64)
    for op, s, m in ((-1, 0, 1), (len(G.OPS), 0, 1), (G.OPS["shl96"], 96, 1), (G.OPS["shl192"], 192, 1),
                     (G.OPS["mul_pow2"], -1, 1), (G.OPS["shl_small_weak"], 0, 1), (G.OPS["shl_small_weak"], 32, 1),
                     (G.OPS["add"], 1, 1), (G.OPS["add"], 0, 2), (G.OPS["cacc_reduce"], 0, 0),
                     (G.OPS["cacc_reduce"], 0, 4097), (G.OPS["s_mad2_3"], 0, 1)):
        with pytest.raises(LA.LfError) as e:
            ctx.gl_probe(op, a, a, s=s, m=m)
        assert e.value.code == 1  # LF_ERR_INVALID_ARG
    with pytest.raises(LA.LfError):
        ctx.gl_probe(G.OPS["add"], a, None)


# ------------------------------------------------------------------ 4b: the kernels
def crt_inputs(d):
    """edge_fill at 1 and 3 ring elements, every v e_j at the transform's internal boundaries,
    and the alternating vector"""
    pos = {0, 1, d // 2 - 1, d // 2, d - 1}
    pos |= {j for j in (31, 32, 33, 1023, 1024, 1025, 2047, 2048, 3071, 3072) if d >= 1024 and j < d}
    rows = [edge_fill(d, 100 + d), edge_fill(3 * d, 101 + d)]
    for j in sorted(pos):
        for v in (1, P - 1, 2**32 - 1, 2**32, P - 2**32):
            e = np.zeros(d, np.uint64)
            e[j] = v
            rows.append(e)
    alt = np.ones(d, np.uint64)
    alt[0::2] = P - 1
    rows.append(alt)
    return np.concatenate(rows)


@pytest.mark.parametrize("d", ALL_D)
def test_crt_icrt_on_edges(ctx, d):
    x = crt_inputs(d)
    fwd = ctx.crt(x, d)
    assert np.array_equal(fwd, O.crt(x, d))
    assert np.array_equal(ctx.icrt(x, d), O.icrt(x, d))
    assert np.array_equal(ctx.icrt(fwd, d), x)


@pytest.mark.parametrize("d", ALL_D)
def test_ring_mul_on_edges(ctx, d):
    n = 3
    a, b = edge_fill(n * d, 200 + d), edge_fill(n * d, 201 + d)
    if d == 24:  # three (p-1)^2 products per accumulator: the largest sum a slot product meets
        a, b = (np.concatenate([v, np.full(d, P - 1, np.uint64)]) for v in (a, b))
    want = np.concatenate([O.slot_mul(a[i * d:(i + 1) * d], b[i * d:(i + 1) * d], d) for i in range(a.size // d)])
    assert np.array_equal(ctx.ring_mul(a, b, d), want)


def test_montgomery_on_any_u64(ctx):
    t = dev(ANY)
    ctx.check(ctx.lib.lf_dev_to_montgomery(ctx.h, t.data_ptr(), ANY.size))
    ctx.sync()
    assert [int(v) for v in host(t)] == [int(v) * G.EPS % P for v in ANY]
    t = dev(ANY)
    ctx.check(ctx.lib.lf_dev_from_montgomery(ctx.h, t.data_ptr(), ANY.size))
    ctx.sync()
    assert [int(v) for v in host(t)] == [int(v) * G.R_INV % P for v in ANY]


@pytest.mark.parametrize("nparts", [2, 3, 8])
def test_modp_sum_at_the_wrap_points(ctx, nparts):
    """column sums that are exactly p - 1, p, p + 1, 2^64 - 1 and 2^64 + 1 before reduction, split over the
    parts three ways: evenly, one part p - 1, and as much as possible in the last parts"""
    cols = []
    for T in (P - 1, P, P + 1, 2**64 - 1, 2**64 + 1):
        even = [T // nparts] * nparts
        even[0] += T - sum(even)
        top = [P - 1] + [0] * (nparts - 1)
        rest = T - (P - 1)
        for k in range(1, nparts):
            top[k] = rest // (nparts - 1) + (rest % (nparts - 1) if k == 1 else 0)
        tail, left = [0] * nparts, T
        for k in reversed(range(nparts)):
            tail[k] = min(left, P - 1)
            left -= tail[k]
        for parts in (even, top, tail):
            assert sum(parts) == T and all(0 <= v < P for v in parts)
            cols.append(parts)
    parts = np.array(cols, np.uint64).T.copy()  # [nparts][len]
    out = dev(n=len(cols))
    ctx.dev_modp_sum(dev(parts.ravel()), nparts, len(cols), out)
    ctx.sync()
    assert [int(v) for v in host(out)] == [sum(c) % P for c in cols]


@pytest.mark.parametrize("d,nv", [(24, 4), (16, 4)])
def test_mle_kernels_on_edges(ctx, d, nv):
    """eq_table, mle_evaluate and mle_fix_first with tables and point coordinates from the edge set: the
    s_mul_w chains carry weakly reduced values from product to product"""
    n, tb, nm = 1 << nv, tb_of(d), 3
    r = edge_fill(nv * d, 300 + d)
    eq = dev(n=n * d)
    ctx.dev_eq_table(d, dev(r), nv, eq)
    ctx.sync()
    assert np.array_equal(host(eq), O.eq_table(r, nv, d))
    mles = edge_fill(nm * n * d, 301 + d)
    out = dev(n=nm * d)
    ctx.dev_mle_evaluate(d, dev(mles), nm, nv, dev(r), out)
    ctx.sync()
    want = np.concatenate([O.mle_evaluate(mles[m * n * d:(m + 1) * n * d], nv, d, r) for m in range(nm)])
    assert np.array_equal(host(out), want)
    for k, rb in enumerate((edge_fill(tb, 302 + d), np.full(tb, P - 1, np.uint64))):
        fixed = dev(n=nm * (n // 2) * d)
        ctx.dev_mle_fix_first(d, dev(mles), n * d, nm, nv, rb, fixed, (n // 2) * d)
        ctx.sync()
        for m in range(nm):
            ref = mles[m * n * d:(m + 1) * n * d].copy()
            O.lib().lfo_mle_fix_first(ref, n // 2, d, O.broadcast(rb, d))
            assert np.array_equal(host(fixed)[m * (n // 2) * d:(m + 1) * (n // 2) * d], ref[:(n // 2) * d]), (k, m)


@pytest.mark.parametrize("d,nv", [(24, 4), (16, 4)])
def test_sumcheck_rounds_on_edges(ctx, d, nv):
    """one folding and one linearization round sum (the combinations of tests/test_gpu_sumcheck.py) over
    MLEs, mu and c from the edge set"""
    n, tau, nk = 1 << nv, tb_of(d), 4
    nm = 5 + nk * tau
    mles, mu = edge_fill(nm * n * d, 400 + d), edge_fill(nk * d, 401 + d)
    want = O.sumcheck_round(O.SumcheckComb.folding(mu, nk, tau, 2), mles, nm, nv, d, 4)
    ev = dev(n=5 * d)
    ctx.dev_sumcheck_round(LA.Comb.folding(dev(mu), nk, tau, 2), dev(mles), n * d, nm, nv, d, 4, ev)
    ctx.sync()
    assert np.array_equal(host(ev), want)
    S = [[0, 1, 2], [1], [3], [0, 3]]
    nm = 7  # the MLE list of prepare_lin_sumcheck_polynomial: S without its zero-coefficient multiset, then eq
    c = edge_fill(len(S) * d, 402 + d)
    c[d:2 * d] = 0
    mles = edge_fill(nm * n * d, 403 + d)
    want = O.sumcheck_round(O.SumcheckComb.linearization(c, S), mles, nm, nv, d, 4)
    ev = dev(n=5 * d)
    ctx.dev_sumcheck_round(LA.Comb.linearization(dev(c), S), dev(mles), n * d, nm, nv, d, 4, ev)
    ctx.sync()
    assert np.array_equal(host(ev), want)


@pytest.mark.parametrize("d,nv", [(24, 4), (16, 4)])
def test_get_fhat_on_edges(ctx, d, nv):
    N, tau, n = 13, tb_of(d), 1 << nv
    fc = edge_fill(N * d, 500 + d)
    out = dev(n=tau * n * d)
    ctx.dev_get_fhat(d, dev(fc), N, nv, out)
    ctx.sync()
    got = host(out).reshape(tau, n, d)
    want = O.get_fhat_phi72(fc).reshape(tau, N, d) if d == 24 else fc.reshape(1, N, d)
    assert np.array_equal(got[:, :N], want)
    assert not got[:, N:].any()


def edge_ccs(t, m, n, d, seed, scalar):
    """matrices with 0 .. 4 entries per row and values from the edge set: scalar-valued (the value in
    word 0 of every slot), or ring-valued with every word drawn"""
    rng = np.random.default_rng(seed)
    tb = tb_of(d)
    mats = []
    for j in range(t):
        cnt = rng.integers(0, 5, m)
        cnt[j % m] = 4
        rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        col = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
        if scalar:
            val = np.zeros((col.size, d), np.uint64)
            val[:, ::tb] = edge_fill(col.size, seed + 7 * j + 1)[:, None]
        else:
            val = edge_fill(col.size * d, seed + 7 * j + 1)
        mats.append((rp, col, val.ravel()))
    return mats


@pytest.mark.parametrize("form", ["scalar", "reordered", "gather"])
@pytest.mark.parametrize("d", [24, 16])
def test_mz_products_on_edges(ctx, d, form, monkeypatch):
    """mz_mles and mz_challenged on a small CCS whose z, entry values and zeta come from the edge set, on the
    launch paths tests/test_gpu_mz.py selects: a scalar-valued CCS (one word per entry; the reorder switch
    does not apply to it), and a ring-valued one with its reordered entry copies and, created without them,
    through the hidx / cidx gathers"""
    t, m, n, nz, nv = 3, 16, 16, 2, 4
    mats = edge_ccs(t, m, n, d, 600 + d, scalar=(form == "scalar"))
    if form == "gather":
        monkeypatch.setenv("LATTICEUM_AMD_CCS_REORDER_BYTES", "0")
    M = LA.CCSMatrices(ctx, d, m, n, mats)
    monkeypatch.delenv("LATTICEUM_AMD_CCS_REORDER_BYTES", raising=False)
    assert M.scalar == (form == "scalar")
    if form != "scalar":
        assert M.reordered is (form == "reordered")
    zs = [edge_fill(n * d, 610 + d + i) for i in range(nz)]
    zeta = edge_fill(nz * d, 620 + d)
    zd = dev(np.concatenate(zs))
    out = dev(n=nz * t * (1 << nv) * d)
    M.mz_mles(zd, nz, nv, out)
    ctx.sync()
    assert np.array_equal(host(out), np.concatenate([O.mz_mles(mats, z, nv, d) for z in zs]))
    ch = dev(n=(1 << nv) * d)
    M.mz_challenged(zd, dev(zeta), nz, nv, ch)
    ctx.sync()
    assert np.array_equal(host(ch), O.mz_challenged(mats, zs, [zeta[i * d:(i + 1) * d] for i in range(nz)], nv, d))
