"""GPU parity of the sparse CCS products against the
oracle's mat_vec_mul restatement: the Mz MLEs of compute_mz_mles, the
zeta-challenged combination of the folding prover, and the MLE evaluations
(u_s, eta_s) -- including empty rows, repeated columns in a row and an empty
matrix -- and, at the zkvm's CCS dimensions (m = 2^17 rows, n = 19 768
columns, t = 125 matrices), the evaluation route (M_j^T eq(r)) . z against
evaluating the materialised MLEs. Every launch path of mz.hip is pinned to the
oracle: the block -> tile mapping of the matrix-core zeta combination past one
block per column tile, its i32 accumulators at the largest digits, the column
splits of the evaluations, and the gathers through hidx / cidx of a CCS created
without reordered entry copies."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O

pytestmark = pytest.mark.gpu
P = LA.P


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
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def scalars(v, d):
    """one scalar per entry as ring elements in NTT form (from_scalar: v in word 0 of
    every slot, zero elsewhere)"""
    tb = 3 if d == 24 else 1
    out = np.zeros((len(v), d), np.uint64)
    out[:, ::tb] = np.asarray(v, np.uint64)[:, None]
    return out.ravel()


def random_ccs(t, m, n, d, seed, max_per_row=3, scalar=False):
    rng = np.random.default_rng(seed)
    mats = []
    for j in range(t):
        if j == 1:  # an empty matrix
            mats.append((np.zeros(m + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64)))
            continue
        cnt = rng.integers(0, max_per_row + 1, m)
        rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        col = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
        if col.size > 1:
            col[1] = col[0]  # a repeated column
        if scalar:  # the zkvm's values: small constants, -1 and arbitrary field elements
            v = O.fill_uniform(int(rp[-1]), seed + 7 * j)
            v[::3] = 1
            v[1::5] = LA.P - 1
            val = scalars(v, d)
        else:
            val = O.fill_uniform(int(rp[-1]) * d, seed + 7 * j)
        mats.append((rp, col, val))
    return mats


def covering_ccs(t, m, n, d, seed, scalar=False):
    """every column once per matrix: row r of each M_j holds the columns c = r (mod m),
    each entry with its own value and no all-zero slot -- every element of y (the zeta
    combination) and of w_j (the transposed weights) then enters exactly one output
    row with an invertible coefficient, so any single wrong element changes the result"""
    tb = 3 if d == 24 else 1
    mats = []
    for j in range(t):
        cols = [np.arange(r, n, m) for r in range(m)]
        rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.uint64)
        col = np.concatenate(cols).astype(np.uint32)
        if scalar:
            v = O.fill_uniform(col.size, seed + 7 * j)
            assert v.all()
            val = scalars(v, d)
        else:
            val = O.fill_uniform(col.size * d, seed + 7 * j)
            assert val.reshape(-1, tb).any(axis=1).all()
        assert np.array_equal(np.sort(col), np.arange(n))
        mats.append((rp, col, val))
    return mats


def split(x, k):
    return [x[i * (x.size // k):(i + 1) * (x.size // k)] for i in range(k)]


@pytest.mark.parametrize("scalar", [False, True])
@pytest.mark.parametrize("d", [24, 16, 1024])
def test_mz_products_match_oracle(ctx, d, scalar):
    """ring-valued matrices, and scalar-valued ones (the zkvm's; read one word per
    entry, lf_ccs_is_scalar)"""
    t, m, n, nz, nv = 5, 100, 37, 3, 7
    mats = random_ccs(t, m, n, d, 40 + d, scalar=scalar)
    M = LA.CCSMatrices(ctx, d, m, n, mats)
    assert M.scalar == scalar
    zs = [O.fill_uniform(n * d, 50 + d + i) for i in range(nz)]
    zd = dev(np.concatenate(zs))
    out = dev(n=nz * t * (1 << nv) * d)
    M.mz_mles(zd, nz, nv, out)
    ctx.sync()
    want = np.concatenate([O.mz_mles(mats, z, nv, d) for z in zs])
    assert np.array_equal(host(out), want)
    # the selected matrices only, in the given order (padding rows zeroed over stale data)
    sel = [3, 0, 4, 1]
    part = dev(n=len(sel) * (1 << nv) * d)
    ctx.dev_fill_uniform(part, 55 + d)
    M.mz_mles_sel(zd, sel, nv, part)
    ctx.sync()
    L = (1 << nv) * d
    assert np.array_equal(host(part), np.concatenate([want[j * L:(j + 1) * L] for j in sel]))
    zeta = O.fill_uniform(nz * d, 60 + d)
    ch = dev(n=(1 << nv) * d)
    M.mz_challenged(zd, dev(zeta), nz, nv, ch)
    ctx.sync()
    assert np.array_equal(host(ch), O.mz_challenged(mats, zs, [zeta[i * d:(i + 1) * d] for i in range(nz)], nv, d))
    # the pair form: a second (z, zeta) beside the first, one pass over the entries
    zs2 = [O.fill_uniform(n * d, 150 + d + i) for i in range(nz)]
    zeta2 = O.fill_uniform(nz * d, 160 + d)
    c0, c1 = dev(n=(1 << nv) * d), dev(n=(1 << nv) * d)
    ctx.dev_fill_uniform(c0, 5)
    ctx.dev_fill_uniform(c1, 6)  # padding rows zeroed over stale data
    M.mz_challenged_pair(zd, dev(zeta), dev(np.concatenate(zs2)), dev(zeta2), nz, nv, c0, c1)
    ctx.sync()
    assert np.array_equal(host(c0), host(ch))
    assert np.array_equal(host(c1), O.mz_challenged(mats, zs2, [zeta2[i * d:(i + 1) * d] for i in range(nz)], nv, d))
    point = O.fill_uniform(nv * d, 70 + d)
    ev = dev(n=nz * t * d)
    M.mz_evaluate(zd, nz, nv, dev(point), ev)
    ctx.sync()
    w = want.reshape(nz * t, (1 << nv) * d)
    assert np.array_equal(host(ev), np.concatenate([O.mle_evaluate(w[k], nv, d, point) for k in range(nz * t)]))


@pytest.mark.parametrize("t,n,nz", [(12, 50, 22), (1, 1, 1), (7, 33, 64), (6, 16, 21)])
def test_mz_challenged_tiles(ctx, t, n, nz):
    """the matrix-core zeta combination (d = 24, mz.hip k_zcomb_mfma) at tile edges:
    a last row tile of fewer than 5 values of j, a last column tile of fewer than 16
    columns, K = 3 nz over one, two and three 64-wide chunks (with and without a
    zero tail), one column and one matrix; both sides of the pair form"""
    d, m, nv = 24, 40, 6
    mats = random_ccs(t, m, n, d, 900 + t + n + nz, scalar=(nz % 2 == 0))
    M = LA.CCSMatrices(ctx, d, m, n, mats)
    zs = [O.fill_uniform(n * d, 910 + i) for i in range(nz)]
    zs[0][:d] = P - 1  # the largest residues in the first column
    zeta = O.fill_uniform(nz * d, 920)
    zeta[:3] = P - 1
    want = O.mz_challenged(mats, zs, [zeta[i * d:(i + 1) * d] for i in range(nz)], nv, d)
    ch = dev(n=(1 << nv) * d)
    M.mz_challenged(dev(np.concatenate(zs)), dev(zeta), nz, nv, ch)
    ctx.sync()
    assert np.array_equal(host(ch), want)
    zs2 = [O.fill_uniform(n * d, 930 + i) for i in range(nz)]
    zeta2 = O.fill_uniform(nz * d, 940)
    c0, c1 = dev(n=(1 << nv) * d), dev(n=(1 << nv) * d)
    M.mz_challenged_pair(dev(np.concatenate(zs)), dev(zeta), dev(np.concatenate(zs2)), dev(zeta2), nz, nv, c0, c1)
    ctx.sync()
    assert np.array_equal(host(c0), want)
    assert np.array_equal(host(c1), O.mz_challenged(mats, zs2, [zeta2[i * d:(i + 1) * d] for i in range(nz)], nv, d))


@pytest.mark.parametrize("t,n,nz", [(23, 141, 15), (23, 141, 22), (125, 144, 15), (21, 257, 1)])
def test_mz_challenged_grid(ctx, t, n, nz):
    """the block -> (column tile, row tile) mapping of k_zcomb_mfma past one block per
    column tile (ct = (k / nbr) 8 + (block & 7), rt = (k % nbr) 4 + wave), on a covering
    CCS so that every y[j][c] reaches the output:
    (23, 141, 15): SK path, nrt = 5 row tiles in nbr = 2 blocks (the second with one live
      wave, the last row tile 3 of 5 j), nct = 9 column tiles (a second group of eight
      with one live block, the last tile 13 columns);
    (23, 141, 22): the same grid on the non-SK path, kcn = 2;
    (125, 144, 15): the zkvm's t and nz, nrt = 25, nbr = 7, whole tiles only, nct = 9;
    (21, 257, 1): one K chunk with three live k, nct = 17 (three groups), the last row
      tile one j.
    m = 13 < 2^nv: the three padding rows are zeroed over stale data"""
    d, m, nv = 24, 13, 4
    mats = covering_ccs(t, m, n, d, 700 + t + n + nz, scalar=(nz % 2 == 0))
    M = LA.CCSMatrices(ctx, d, m, n, mats)
    assert M.scalar == (nz % 2 == 0)
    zs = [O.fill_uniform(n * d, 710 + i) for i in range(nz)]
    zs[0][:d] = P - 1
    zeta = O.fill_uniform(nz * d, 720)
    zeta[:3] = P - 1
    zs2 = [O.fill_uniform(n * d, 730 + i) for i in range(nz)]
    zeta2 = O.fill_uniform(nz * d, 740)
    want = O.mz_challenged(mats, zs, split(zeta, nz), nv, d)
    want2 = O.mz_challenged(mats, zs2, split(zeta2, nz), nv, d)
    zd, zd2 = dev(np.concatenate(zs)), dev(np.concatenate(zs2))
    ch, c0, c1 = (dev(n=(1 << nv) * d) for _ in range(3))
    for k, o in enumerate((ch, c0, c1)):
        ctx.dev_fill_uniform(o, 750 + k)
    M.mz_challenged(zd, dev(zeta), nz, nv, ch)
    M.mz_challenged_pair(zd, dev(zeta), zd2, dev(zeta2), nz, nv, c0, c1)
    ctx.sync()
    assert np.array_equal(host(ch), want)
    assert np.array_equal(host(c0), want)
    assert np.array_equal(host(c1), want2)


@pytest.mark.parametrize("nz", [21, 22, 5440, 5568])
def test_mz_challenged_extreme_digits(ctx, nz):
    """the i32 accumulators of k_zcomb_mfma at the largest digits: every word of z and
    zeta 0x7F7F7F7F7F7F7F7F, so every D8 digit is +127 and row a = 2 of the M-form
    (p_2, p_1, p_0 unshifted) adds 8 * 127^2 = 129 032 per k to the weight-7
    accumulator. nz = 21: the last SK size (the paired 32-bit weights within 3 % of
    2^31); 22: the first non-SK size; 5440: kcn = 255, the last size the i32 bound
    kcn 2^23 < 2^31 allows; 5568: kcn = 261, where 3 nz 129 032 > 2^31 -- the
    combination leaves the matrix cores there (mz.hip zcomb) and stays exact.
    Before that guard nz = 5568 returned wrong field elements and no error."""
    d, t, m, nv, n = 24, 1, 2, 1, 17
    mats = covering_ccs(t, m, n, d, 800)
    M = LA.CCSMatrices(ctx, d, m, n, mats)
    word = np.uint64(0x7F7F7F7F7F7F7F7F)
    z = np.full(n * d, word, np.uint64)
    zeta = np.full(d, word, np.uint64)
    want = O.mz_challenged(mats, [z] * nz, [zeta] * nz, nv, d)
    zd, zetad = dev(np.tile(z, nz)), dev(np.tile(zeta, nz))
    ch, c0, c1 = (dev(n=(1 << nv) * d) for _ in range(3))
    M.mz_challenged(zd, zetad, nz, nv, ch)
    M.mz_challenged_pair(zd, zetad, zd, zetad, nz, nv, c0, c1)
    ctx.sync()
    assert np.array_equal(host(ch), want)
    assert np.array_equal(host(c0), want) and np.array_equal(host(c1), want)


# nsplit below is mz.hip dots_nsplit: blocks = t ceil(nz / 4) (ns / spb) with ns = d / 3
# slots for d = 24, else d, and spb = min(ns, 256); k = min(ceil(2048 / blocks), 16);
# if 64 k > n then k = max(n / 64, 1).
#   (24 | 16, 3, 200, 5): blocks = 3 * 2 * 1 = 6, k = 16, 1024 > 200 -> nsplit = 200 / 64 = 3
#   (1024, 3, 200, 5):    blocks = 3 * 2 * 4 = 24, k = 16 -> nsplit = 3
#     column bounds 200 s / 3 = 0 / 66 / 133 / 200, instance groups of 4 and 1,
#     columns per block cpb = 256 / spb = 32 (d = 24), 16 (d = 16), 1 (d = 1024)
#   (24, 3, 129, 6): blocks = 6, k = 16, 1024 > 129 -> nsplit = 129 / 64 = 2
#   (24, 3, 127, 6): 127 / 64 = 1 -> nsplit = 1
#   (24, 2, 1030, 2): blocks = 2, k = 16, 1024 <= 1030 -> nsplit = 16
@pytest.mark.parametrize("d,t,n,nz", [(24, 3, 200, 5), (16, 3, 200, 5), (1024, 3, 200, 5), (24, 3, 129, 6),
                                      (24, 3, 127, 6), (24, 2, 1030, 2)])
def test_mz_evaluate_column_splits(ctx, d, t, n, nz):
    """k_dots over column splits (uneven bounds n split / nsplit, the k_dots_sum pass,
    a last instance group of fewer than four) against evaluating the oracle's MLEs; the
    covering CCS puts every w_j[c] into the sums"""
    m, nv = 40, 6
    mats = covering_ccs(t, m, n, d, 600 + d + n)
    M = LA.CCSMatrices(ctx, d, m, n, mats)
    zs = [O.fill_uniform(n * d, 610 + d + i) for i in range(nz)]
    point = O.fill_uniform(nv * d, 620 + d)
    ev = dev(n=nz * t * d)
    ctx.dev_fill_uniform(ev, 630)
    M.mz_evaluate(dev(np.concatenate(zs)), nz, nv, dev(point), ev)
    ctx.sync()
    mles = np.concatenate([O.mz_mles(mats, z, nv, d) for z in zs])
    want = np.concatenate([O.mle_evaluate(w, nv, d, point) for w in split(mles, nz * t)])
    assert np.array_equal(host(ev), want)


@pytest.mark.parametrize("d", [24, 16])
def test_mz_gather_path(ctx, d, monkeypatch):
    """a ring-valued CCS created without the reordered entry copies
    (LATTICEUM_AMD_CCS_REORDER_BYTES=0: the form of a CCS too large for them) reads its
    values through hidx / cidx in the challenged products and the transposed weights;
    with up to 9 entries per row the row-major k_csr also runs its four-at-a-time
    loop, with tails of 0 to 3. Both forms against the oracle"""
    t, m, n, nz, nv = 5, 100, 37, 3, 7
    mats = random_ccs(t, m, n, d, 300 + d, max_per_row=9)
    monkeypatch.setenv("LATTICEUM_AMD_CCS_REORDER_BYTES", "0")
    G = LA.CCSMatrices(ctx, d, m, n, mats)
    monkeypatch.delenv("LATTICEUM_AMD_CCS_REORDER_BYTES")
    R = LA.CCSMatrices(ctx, d, m, n, mats)
    assert G.reordered is False and R.reordered is True
    assert not G.scalar and not R.scalar
    L = (1 << nv) * d
    zs = [O.fill_uniform(n * d, 310 + d + i) for i in range(nz)]
    zs2 = [O.fill_uniform(n * d, 320 + d + i) for i in range(nz)]
    zeta, zeta2 = O.fill_uniform(nz * d, 330 + d), O.fill_uniform(nz * d, 340 + d)
    point = O.fill_uniform(nv * d, 350 + d)
    sel = [3, 0, 4, 1]
    want = np.concatenate([O.mz_mles(mats, z, nv, d) for z in zs])
    want_sel = np.concatenate([want[j * L:(j + 1) * L] for j in sel])
    want_ch = O.mz_challenged(mats, zs, split(zeta, nz), nv, d)
    want_ch2 = O.mz_challenged(mats, zs2, split(zeta2, nz), nv, d)
    want_ev = np.concatenate([O.mle_evaluate(w, nv, d, point) for w in split(want, nz * t)])
    zd, zd2 = dev(np.concatenate(zs)), dev(np.concatenate(zs2))
    for M in (G, R):
        out, part, ev = dev(n=nz * t * L), dev(n=len(sel) * L), dev(n=nz * t * d)
        ch, c0, c1 = dev(n=L), dev(n=L), dev(n=L)
        for k, o in enumerate((out, part, ev, ch, c0, c1)):
            ctx.dev_fill_uniform(o, 360 + k)  # padding rows zeroed over stale data
        M.mz_mles(zd, nz, nv, out)
        M.mz_mles_sel(zd, sel, nv, part)
        M.mz_challenged(zd, dev(zeta), nz, nv, ch)
        M.mz_challenged_pair(zd, dev(zeta), zd2, dev(zeta2), nz, nv, c0, c1)
        M.mz_evaluate(zd, nz, nv, dev(point), ev)
        ctx.sync()
        assert np.array_equal(host(out), want), M.reordered
        assert np.array_equal(host(part), want_sel), M.reordered
        assert np.array_equal(host(ch), want_ch), M.reordered
        assert np.array_equal(host(c0), want_ch), M.reordered
        assert np.array_equal(host(c1), want_ch2), M.reordered
        assert np.array_equal(host(ev), want_ev), M.reordered


def test_mz_zkvm_dimensions(ctx):
    """m = 2^17, n = 19 768, t = 125 (zkvm ccs.rs:43-67) with ~2 entries per row
    per matrix: sampled rows of the materialised products against the oracle,
    the transposed evaluation route against evaluating the materialised MLEs, and
    sampled evaluations against the oracle's"""
    import torch
    d, t, m, n, nz, nv = 24, 125, 1 << 17, 19768, 2, 17
    rng = np.random.default_rng(5)
    mats = []
    for j in range(t):
        cnt = rng.integers(0, 5, m)
        rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        col = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
        mats.append((rp, col, None))
    nnz = sum(int(x[0][-1]) for x in mats)
    vals = O.fill_uniform(nnz * d, 6)
    off = 0
    full = []
    for rp, col, _ in mats:
        k = int(rp[-1])
        full.append((rp, col, vals[off * d:(off + k) * d]))
        off += k
    M = LA.CCSMatrices(ctx, d, m, n, full)
    zs = O.fill_uniform(nz * n * d, 7)
    zd = dev(zs)
    out = dev(n=nz * t * (1 << nv) * d)
    M.mz_mles(zd, nz, nv, out)
    ctx.sync()
    for i, j, r in ((0, 0, 0), (1, 124, m - 1), (0, 63, 77777), (1, 5, 4096)):
        rp, col, val = full[j]
        a, b = int(rp[r]), int(rp[r + 1])
        want = O.spmv(np.array([0, b - a], np.uint64), col[a:b], val[a * d:b * d], d, zs[i * n * d:(i + 1) * n * d])
        got = host(out[((i * t + j) * (1 << nv) + r) * d:((i * t + j) * (1 << nv) + r + 1) * d])
        assert np.array_equal(got, want), (i, j, r)
    pt = O.fill_uniform(nv * d, 8)
    point = dev(pt)
    ev, ev2 = dev(n=nz * t * d), dev(n=nz * t * d)
    M.mz_evaluate(zd, nz, nv, point, ev)
    ctx.dev_mle_evaluate(d, out, nz * t, nv, point, ev2)
    ctx.sync()
    assert torch.equal(ev, ev2)
    for i, j in ((0, 0), (1, 124), (0, 63)):
        want = O.mle_evaluate(O.spmv(*full[j], d, zs[i * n * d:(i + 1) * n * d]), nv, d, pt)
        assert np.array_equal(host(ev[(i * t + j) * d:(i * t + j + 1) * d]), want), (i, j)
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("d", [24, 1024])
def test_scalar_ccs_montgomery_input(ctx, d):
    """scalar-valued matrices handed over as Montgomery limbs (the zero-copy form of the
    Rust structs) are still detected as scalars and give the canonical products"""
    t, m, n, nz, nv = 4, 64, 21, 2, 6
    mats = random_ccs(t, m, n, d, 90 + d, scalar=True)
    mont = [(rp, col, np.array([(int(v) << 64) % LA.P for v in val], np.uint64)) for rp, col, val in mats]
    A = LA.CCSMatrices(ctx, d, m, n, mats)
    B = LA.CCSMatrices(ctx, d, m, n, mont, repr=LA.REPR_MONTGOMERY)
    assert A.scalar and B.scalar
    zd = dev(O.fill_uniform(nz * n * d, 91 + d))
    oa, ob = dev(n=nz * t * (1 << nv) * d), dev(n=nz * t * (1 << nv) * d)
    A.mz_mles(zd, nz, nv, oa)
    B.mz_mles(zd, nz, nv, ob)
    point = dev(O.fill_uniform(nv * d, 92 + d))
    ea, eb = dev(n=nz * t * d), dev(n=nz * t * d)
    A.mz_evaluate(zd, nz, nv, point, ea)
    B.mz_evaluate(zd, nz, nv, point, eb)
    ctx.sync()
    assert np.array_equal(host(oa), host(ob)) and np.array_equal(host(ea), host(eb))
