"""The device self-checks of the proving loop (the reference's `debug` feature):
CCS::check_relation as one fused kernel (lf_dev_ccs_check_relation) with the row
values its failure report prints (lf_dev_ccs_row_evals), the witness's linf norm on
signed representatives (lf_dev_linf_norm), and the accumulator opening checks
(lf_lcccs_check / lf_cccs_check). Expected values come from the oracle's primitives
(spmv, slot products, fhat, evaluate, ajtai_commit) and numpy; everything is
bit-exact."""
import numpy as np
import pytest

import latticeum_amd as LA
import nifs as N
import oracle as O

pytestmark = pytest.mark.gpu
P = LA.P
LF_ERR_NOT_SATISFIED = 14  # lf.h


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
        return torch.from_numpy(np.ascontiguousarray(x, np.uint64).view(np.int64).copy()).cuda()
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def flat(xs):
    return np.concatenate([np.asarray(x, np.uint64).ravel() for x in xs]) if len(xs) else np.zeros(0, np.uint64)


def scalars(v, d):
    """one scalar per entry as NTT-form ring elements (from_scalar)"""
    tb = 3 if d == 24 else 1
    out = np.zeros((len(v), d), np.uint64)
    out[:, ::tb] = np.asarray(v, np.uint64)[:, None]
    return out.ravel()


def random_ccs(t, m, n, d, seed, max_per_row, scalar):
    """tests/test_gpu_mz.py's random matrices: an empty matrix, a repeated column, empty
    rows; 0..max_per_row entries per row"""
    rng = np.random.default_rng(seed)
    mats = []
    for j in range(t):
        if j == 1:
            mats.append((np.zeros(m + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64)))
            continue
        cnt = rng.integers(0, max_per_row + 1, m)
        rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        col = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
        col[1] = col[0]
        if scalar:
            v = O.fill_uniform(int(rp[-1]), seed + 7 * j)
            v[::3] = 1
            v[1::5] = P - 1
            val = scalars(v, d)
        else:
            val = O.fill_uniform(int(rp[-1]) * d, seed + 7 * j)
        mats.append((rp, col, val))
    return mats


def oracle_resid(mats, c, S, z, m, d):
    """sum_i c_i (.) prod_(j in S_i) (M_j z), the Hadamard chain from ONE (arith.rs:78-105)"""
    total, mz = np.zeros(m * d, np.uint64), {}
    for c_i, S_i in zip(c, S):
        had = np.tile(N.one(d), m)
        for j in S_i:
            if j not in mz:
                mz[j] = O.spmv(*mats[j], d, z)
            had = N.mul(had, mz[j], d)
        total = N.add(total, N.smul(c_i, had, d))
    return total


def first_bad(resid, m, d):
    rows = np.flatnonzero(resid.reshape(m, d).any(axis=1))
    return int(rows[0]) if rows.size else -1


# ---------------------------------------------------------------- the relation kernel
T1 = dict(t=5, m=100, n=37, nz=3, S=[[0, 2], [1, 3], [4, 4, 0], []])
_case1 = {}


def case1(d, scalar):
    """test 1's CCS, z batch and oracle residuals, computed once per (d, scalar)"""
    key = (d, scalar)
    if key not in _case1:
        t, m, n, nz, S = T1["t"], T1["m"], T1["n"], T1["nz"], T1["S"]
        mats = random_ccs(t, m, n, d, 300 + d, 9, scalar)
        per_row = np.concatenate([np.diff(rp.astype(np.int64)) for rp, _, _ in mats])
        assert per_row.max() >= 8 and (per_row % 4 != 0).any()  # the 4-entry batch twice over, and its tail
        c = [O.fill_uniform(d, 310 + d + i) for i in range(len(S))]
        zs = [O.fill_uniform(n * d, 320 + d + i) for i in range(nz)]
        want = [oracle_resid(mats, c, S, z, m, d) for z in zs]
        _case1[key] = (mats, c, zs, want)
    return _case1[key]


def ccs1(ctx, d, scalar):
    mats, c, zs, want = case1(d, scalar)
    M = LA.CCSMatrices(ctx, d, T1["m"], T1["n"], mats)
    assert M.scalar == scalar
    M.set_structure(0, 3, np.concatenate(c), T1["S"])
    return M, zs, want


@pytest.mark.parametrize("scalar", [False, True])
@pytest.mark.parametrize("d", [24, 16, 1024])
def test_residual_matches_oracle(ctx, d, scalar):
    """the residual bit-exact and the first nonzero row of each z: two-matrix products, an
    empty matrix in a multiset, a repeated index (squared), an empty multiset (c_i on
    every row)"""
    m, nz = T1["m"], T1["nz"]
    M, zs, want = ccs1(ctx, d, scalar)
    zd = dev(np.concatenate(zs))
    resid = dev(n=nz * m * d)
    ctx.dev_fill_uniform(resid, 5)
    rows = M.check_relation(zd, nz, resid)
    assert np.array_equal(host(resid), np.concatenate(want))
    assert rows == [first_bad(w, m, d) for w in want]
    assert M.last_status == LF_ERR_NOT_SATISFIED
    # without the residual: the same rows
    assert M.check_relation(zd, nz) == rows


def test_relation_needs_structure(ctx):
    mats, _, zs, _ = case1(16, False)
    M = LA.CCSMatrices(ctx, 16, T1["m"], T1["n"], mats)
    with pytest.raises(LA.LfError, match="lf_ccs_set_structure") as e:
        M.check_relation(dev(zs[0]))
    assert e.value.code == 1


@pytest.mark.parametrize("scalar", [False, True])
@pytest.mark.parametrize("d,W,l,t,deg", [(24, 13, 4, 6, 3), (16, 7, 1, 5, 3), (1024, 5, 2, 4, 2)])
def test_satisfied_and_first_bad_row(ctx, d, W, l, t, deg, scalar):
    """a satisfying z, the same with its last product column replaced (the recipe of
    tests/test_nifs_oracle.py), and a second satisfying z, in one batch"""
    pr = N.Params(d)
    seed = 40 + d + W
    ccs = N.satisfied_ccs(d, W, l, t, deg, seed, pr, empty=0.3, scalar=scalar)
    M = LA.CCSMatrices(ctx, d, ccs.m, ccs.n, ccs.mats)
    assert M.scalar == scalar
    M.set_structure(l, deg, np.concatenate(ccs.c), ccs.S)
    zs = []
    for sd in (seed + 4, seed + 5):
        x, w = N.satisfying_z(ccs, W, sd)
        zs.append(np.concatenate(list(x) + [N.one(d), w]))
    bad = zs[0].copy()
    bad[-d:] = O.fill_uniform(d, seed + 9)
    resid = oracle_resid(ccs.mats, ccs.c, ccs.S, bad, ccs.m, d).reshape(ccs.m, d)
    r = first_bad(resid, ccs.m, d)
    assert r >= 0 and resid.any(axis=1).sum() > 1  # several failing rows: the minimum is exercised
    if W == 13:
        assert r > 0
    assert M.check_relation(dev(np.concatenate([zs[0], bad, zs[1]])), 3) == [-1, r, -1]
    assert M.last_status == LF_ERR_NOT_SATISFIED
    assert M.check_relation(dev(np.concatenate(zs)), 2) == [-1, -1]
    assert M.last_status == 0


@pytest.mark.parametrize("m", [1000, 1])
@pytest.mark.parametrize("d", [24, 1024])
def test_one_nonzero_word(ctx, d, m):
    """S = [[0]], c = [ONE], M_0 = the identity of scalar entries: the residual is z. One
    nonzero word in the last slot of the last row (the OR across slots and slot tiles, the
    last partial block), then a second in an earlier block (the minimum across blocks)"""
    rp = np.arange(m + 1, dtype=np.uint64)
    M = LA.CCSMatrices(ctx, d, m, m, [(rp, np.arange(m, dtype=np.uint32), scalars(np.ones(m, np.uint64), d))])
    assert M.scalar
    M.set_structure(0, 1, N.one(d), [[0]])
    z = np.zeros(m * d, np.uint64)
    assert M.check_relation(dev(z)) == [-1] and M.last_status == 0
    z[-1] = 5
    resid = dev(n=m * d)
    assert M.check_relation(dev(z), 1, resid) == [m - 1] and M.last_status == LF_ERR_NOT_SATISFIED
    assert np.array_equal(host(resid), z)
    if m > 517:
        z[517 * d + d // 2] = P - 1
        assert M.check_relation(dev(z)) == [517]


@pytest.mark.parametrize("scalar", [False, True])
@pytest.mark.parametrize("d", [24, 16, 1024])
def test_row_evals_match_oracle(ctx, d, scalar):
    m, t = T1["m"], T1["t"]
    M, zs, _ = ccs1(ctx, d, scalar)
    mats = case1(d, scalar)[0]
    mz = [O.spmv(*mat, d, zs[0]).reshape(m, d) for mat in mats]
    none = np.flatnonzero(np.diff(mats[0][0].astype(np.int64)) == 0)  # rows without an entry of M_0 (nor of M_1)
    empty = int(none[(none > 0) & (none < m - 1)][0])
    zd = dev(zs[0])
    for row in (0, m - 1, empty):
        out = dev(n=t * d)
        ctx.dev_fill_uniform(out, 9)
        M.row_evals(zd, row, out)
        assert np.array_equal(host(out).reshape(t, d), np.stack([y[row] for y in mz])), row
    assert not mz[0][empty].any()
    with pytest.raises(LA.LfError):
        M.row_evals(zd, m, dev(n=t * d))


# ---------------------------------------------------------------- the norm
def np_norm(x):
    x = np.asarray(x, np.uint64)
    return int(np.minimum(x, np.uint64(P) - x).max())


@pytest.mark.parametrize("n", [1, 7, (1 << 16) + 3])
def test_linf_norm(ctx, n):
    """max min(x, p - x) against numpy, the signed edge values, and the maximum at the
    first and at the last word (the unaligned head and the tail of the 16-byte loads)"""
    x = O.fill_uniform(n, 70 + n)
    assert ctx.dev_linf_norm(dev(x)) == np_norm(x)
    assert ctx.dev_linf_norm(dev(np.zeros(n, np.uint64))) == 0
    for v, want in (((P - 1) // 2, (P - 1) // 2), ((P + 1) // 2, (P - 1) // 2), (P - 1, 1)):
        y = np.zeros(n, np.uint64)
        y[n // 2] = v
        assert ctx.dev_linf_norm(dev(y)) == want, v
    small = x % np.uint64(1000)
    for at in (0, n - 1):
        y = small.copy()
        y[at] = P - 5000
        assert ctx.dev_linf_norm(dev(y)) == 5000, at
    if n > 1:  # a view that starts 8 bytes past a 16-byte boundary
        t = dev(np.concatenate([[np.uint64(P - 1) // np.uint64(2)], x]))
        assert ctx.dev_linf_norm(t[1:]) == np_norm(x)


# ---------------------------------------------------------------- does the witness open the instance?
SHAPES = [(24, 5, 2, 4, 2, 3), (16, 7, 1, 5, 3, 3)]
_inst = {}


def instance(ctx, shape):
    """a prover over a satisfied CCS with two committed witnesses and the first one's fresh
    accumulator (the oracle's), once per shape"""
    if shape not in _inst:
        d, W, l, t, deg, kappa = shape
        pr = N.Params(d)
        seed = 7 + d + W
        ccs = N.satisfied_ccs(d, W, l, t, deg, seed, pr)
        Nn = W * pr.L
        A = O.fill_uniform(kappa * Nn * d, seed + 6)
        sch = LA.AjtaiCommitmentScheme(ctx, A.reshape(kappa, Nn, d))
        M = LA.CCSMatrices(ctx, d, ccs.m, ccs.n, ccs.mats)
        prover = LA.Prover(ctx, sch, LA.goldilocks_dp(d), M, l, deg, np.concatenate(ccs.c), ccs.S)
        wits = []
        for sd in (11, 12):
            x, w = N.satisfying_z(ccs, W, sd)
            fc, f = O.witness_from_w_ccs(w, d, pr.B, pr.L)
            wits.append((x, N.Witness(w_ccs=w, f=f, f_coeff=fc), O.ajtai_commit(A, kappa, Nn, d, f)))
        acc = N.linearize_fresh(ccs, wits[0][2], wits[0][0], wits[0][1], pr)
        _inst[shape] = (pr, ccs, A, prover, wits, acc)
    return _inst[shape]


def acc_dict(L):
    return {"r": flat(L.r), "v": flat(L.v), "cm": np.asarray(L.cm, np.uint64).copy(), "u": flat(L.u),
            "x_w": flat(L.x_w), "h": np.asarray(L.h, np.uint64).copy()}


def dev_wit(w):
    return {"w_ccs": dev(w.w_ccs), "f": dev(w.f), "f_coeff": dev(w.f_coeff)}


def bump(a, i):
    """a copy of the host array with word i replaced by another canonical value"""
    b = np.asarray(a, np.uint64).copy()
    b[i] = (int(b[i]) + 1) % P
    return b


def failed(call):
    with pytest.raises(LA.RelationError) as e:
        call()
    assert e.value.code == 12
    return e.value


@pytest.mark.parametrize("shape", SHAPES)
def test_lcccs_check(ctx, shape):
    d, W, l, t, deg, kappa = shape
    pr, ccs, A, prover, wits, acc = instance(ctx, shape)
    (xa, Wa, cma), (xi, Wi, cmi) = wits
    a, w = acc_dict(acc), dev_wit(Wa)
    norm = np_norm(Wa.f_coeff)
    assert prover.check_lcccs(a, w) == norm
    assert prover.check_lcccs(a, w, bound=norm + 1) == norm
    assert failed(lambda: prover.check_lcccs(a, w, bound=norm)).check == LA.REL_NORM
    for key, i, want in (("f", 3 * d + 1, LA.REL_WITNESS_F), ("w_ccs", W * d - 1, LA.REL_WITNESS_W),
                         ("w_ccs", 2 * d, LA.REL_WITNESS_W)):
        e = failed(lambda: prover.check_lcccs(a, {**w, key: dev(bump(getattr(Wa, key), i))}))
        assert e.check == want and e.row is None, key
    for key, i, want in (("cm", d + 2, LA.REL_CM), ("v", 1, LA.REL_V), ("u", t * d - 1, LA.REL_U), ("x_w", 0, LA.REL_U),
                         ("h", d - 1, LA.REL_U)):
        assert failed(lambda: prover.check_lcccs({**a, key: bump(a[key], i)}, w)).check == want, key
    # w_ccs as a view 8 bytes past a 16-byte boundary: the compare's word loads
    off = lambda x: dev(np.concatenate([np.zeros(1, np.uint64), x]))[1:]
    assert prover.check_lcccs(a, {**w, "w_ccs": off(Wa.w_ccs)}) == norm
    for i in (0, W * d - 1):
        assert failed(lambda: prover.check_lcccs(a, {**w, "w_ccs": off(bump(Wa.w_ccs, i))})).check == LA.REL_WITNESS_W
    # another valid witness: consistent and short, but not this commitment's
    assert failed(lambda: prover.check_lcccs(a, dev_wit(Wi))).check == LA.REL_CM
    # the folded accumulator opens to the folded witness
    Nn = W * pr.L
    w_out = {"w_ccs": dev(n=W * d), "f": dev(n=Nn * d), "f_coeff": dev(n=Nn * d)}
    out, _ = prover.fold_prove(a, w, cmi, flat(xi), dev_wit(Wi), w_out)
    assert prover.check_lcccs(out, w_out) == np_norm(host(w_out["f_coeff"]))
    assert failed(lambda: prover.check_lcccs({**out, "u": bump(out["u"], 0)}, w_out)).check == LA.REL_U


@pytest.mark.parametrize("shape", SHAPES)
def test_cccs_check(ctx, shape):
    d, W, l, t, deg, kappa = shape
    pr, ccs, A, prover, wits, _ = instance(ctx, shape)
    xi, Wi, cmi = wits[1]
    assert prover.check_cccs(cmi, flat(xi), dev_wit(Wi)) == np_norm(Wi.f_coeff)
    assert failed(lambda: prover.check_cccs(bump(cmi, 0), flat(xi), dev_wit(Wi))).check == LA.REL_CM
    # an unsatisfying witness, consistent and committed: only the CCS relation fails
    w2 = Wi.w_ccs.copy()
    w2[-d:] = O.fill_uniform(d, 99)
    fc2, f2 = O.witness_from_w_ccs(w2, d, pr.B, pr.L)
    cm2 = O.ajtai_commit(A, kappa, W * pr.L, d, f2)
    z2 = np.concatenate(list(xi) + [N.one(d), w2])
    r = first_bad(oracle_resid(ccs.mats, ccs.c, ccs.S, z2, ccs.m, d), ccs.m, d)
    assert r >= 0
    e = failed(lambda: prover.check_cccs(cm2, flat(xi), dev_wit(N.Witness(w_ccs=w2, f=f2, f_coeff=fc2))))
    assert e.check == LA.REL_CCS and e.row == r
