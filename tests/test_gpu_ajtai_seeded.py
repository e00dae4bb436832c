"""GPU: schemes whose Ajtai matrix is derived on the device from a seed
(lf_ajtai_create_seeded, latticeum_amd/csrc/ajtai_seeded.hip), for both kinds of seed.
The generator writes the matrix-core operand order and the row-sum tables directly, so
every entry of A is read back through commitments of unit vectors and compared, bit for
bit, with the host expansion (lf_ajtai_seeded_expand, pinned to the oracle by
test_ajtai_seeded.py); random commitments, the commit+fold step (the path that reads the
row-sum tables in the offset form), column shards and the memory the scheme owns are
compared with a scheme that lf_ajtai_create makes from the expanded matrix."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O

pytestmark = pytest.mark.gpu
P = LA.P
KINDS = {"poseidon2": (LA.AJTAI_SEED_POSEIDON2, [0xFEDCBA9876543210, 5, P - 1, 0]),
         "splitmix": (LA.AJTAI_SEED_SPLITMIX, 90125)}
# (d, kappa, ncols). The last: kappa beyond 32 LF_MAX_KTILES rows has no fragment form, the
# scheme materialises its window (130 rows, and 130 columns: five calls of unit vectors)
SHAPES = [
    (24, 3, 35),     # Phi_72 virtual slots, grouped geometry with a top region, a ragged last chunk
    (16, 33, 40),    # one slot block, a second 32-row tile, a row tail
    (64, 2, 7),      # Lp = 1, fewer than 32 columns
    (256, 9, 45),    # a row tile of 8 + 1, grouped
    (1024, 2, 5),
    (2048, 2, 5),
    (4096, 2, 5),    # qperm
    (16, 130, 130),  # no fragment form
]


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


_EXPANDED = {}


def expanded(kname, d, kappa, ncols_total, col0=0, ncols=None):
    """the host expansion [kappa][ncols][d], computed once per shape and left unchanged"""
    key = (kname, d, kappa, ncols_total, col0, ncols)
    if key not in _EXPANDED:
        kind, seed = KINDS[kname]
        A = LA.ajtai_seeded_expand(seed, kind, kappa=kappa, ncols_total=ncols_total, d=d, col0=col0, ncols=ncols)
        A.setflags(write=False)
        _EXPANDED[key] = A
    return _EXPANDED[key]


def seeded(ctx, kname, d, kappa, ncols, col0=0, ncols_total=None):
    kind, seed = KINDS[kname]
    return LA.AjtaiCommitmentScheme.seeded(ctx, seed, kind, kappa=kappa, ncols=ncols, d=d, col0=col0,
                                           ncols_total=ncols_total)


def dev_commits(ctx, sch, vecs):
    """commitments [len(vecs)][kappa d] of host vectors, at most 32 per call"""
    import torch
    out = []
    for i in range(0, len(vecs), 32):
        dv = [dev(v) for v in vecs[i:i + 32]]
        cm = dev(n=len(dv) * sch.kappa * sch.d)
        torch.cuda.synchronize()
        ctx.dev_ajtai_commit(sch, dv, cm)
        ctx.sync()
        out.append(host(cm).reshape(len(dv), sch.kappa * sch.d))
    return np.concatenate(out)


def unit_vectors(ncols, d):
    vecs = []
    for v in range(ncols):
        f = np.zeros((ncols, d), np.uint64)
        f[v, :] = 1
        vecs.append(f.ravel())
    return vecs


@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("d,kappa,ncols", SHAPES)
def test_every_entry_and_random_commitments(ctx, kname, d, kappa, ncols):
    A = expanded(kname, d, kappa, ncols)
    sch = seeded(ctx, kname, d, kappa, ncols)
    mat = LA.AjtaiCommitmentScheme(ctx, A)
    assert sch.layout == mat.layout == (1 if kappa <= 128 else 0)
    assert (sch.kappa, sch.width, sch.d) == (kappa, ncols, d)
    # every entry of A: vector v is 1 in every slot of column v
    units = unit_vectors(ncols, d)
    got = dev_commits(ctx, sch, units).reshape(ncols, kappa, d)
    if d == 24:  # a slot is an F_q^3 element and (1, 1, 1) is not its one: compare the schemes
        want = dev_commits(ctx, mat, units).reshape(ncols, kappa, d)
    else:
        want = A.transpose(1, 0, 2)
    assert np.array_equal(got, want)
    # random vectors
    fs = [O.fill_uniform(ncols * d, 300 + 7 * i + d) for i in range(3)]
    cs, cmat = dev_commits(ctx, sch, fs), dev_commits(ctx, mat, fs)
    assert np.array_equal(cs, cmat)
    for f, c in zip(fs, cs):
        assert np.array_equal(c, O.ajtai_commit(A, kappa, ncols, d, f))
    # the host-buffer commit as well
    assert np.array_equal(sch.commit_ntt(fs[0]), cs[0])


@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("d,kappa,ncols", SHAPES)
def test_dev_expand_matches_host(ctx, kname, d, kappa, ncols):
    import torch
    kind, seed = KINDS[kname]
    A = expanded(kname, d, kappa, ncols)
    out = dev(n=kappa * ncols * d)
    torch.cuda.synchronize()
    ctx.dev_ajtai_seeded_expand(seed, kind, out, kappa=kappa, ncols_total=ncols, d=d)
    ctx.sync()
    assert np.array_equal(host(out).reshape(kappa, ncols, d), A)
    row0, nrows, col0, nc = kappa - 1, 1, 1, ncols - 2
    win = dev(n=nrows * nc * d)
    torch.cuda.synchronize()
    ctx.dev_ajtai_seeded_expand(seed, kind, win, kappa=kappa, ncols_total=ncols, d=d, row0=row0, nrows=nrows,
                                col0=col0, ncols=nc)
    ctx.sync()
    assert np.array_equal(host(win).reshape(nrows, nc, d), A[row0:row0 + nrows, col0:col0 + nc])


def test_create_refusals(ctx):
    P2 = LA.AJTAI_SEED_POSEIDON2
    for kw, code in ((dict(seed=[1, 2, 3, 4], kind=P2, kappa=2, ncols=5, d=48), 2),
                     (dict(seed=[1, 2, 3, 4], kind=P2, kappa=2, ncols=5, d=64, col0=3, ncols_total=7), 1),
                     (dict(seed=[P, 2, 3, 4], kind=P2, kappa=2, ncols=5, d=64), 1),
                     (dict(seed=[1, 1, 0, 0], kind=LA.AJTAI_SEED_SPLITMIX, kappa=2, ncols=5, d=64), 1),
                     (dict(seed=[1, 0, 0, 0], kind=7, kappa=2, ncols=5, d=64), 1),
                     (dict(seed=[1, 2, 3, 4], kind=P2, kappa=0, ncols=5, d=64), 1)):
        seed, kind = kw.pop("seed"), kw.pop("kind")
        with pytest.raises(LA.LfError) as e:
            LA.AjtaiCommitmentScheme.seeded(ctx, seed, kind, **kw)
        assert e.value.code == code, kw


# ---------------------------------------------------------------- the step
def make_rho(d, K, seed):
    rng = np.random.default_rng(seed)
    rc = [O.short_challenge(rng.integers(0, 256, 3 * d // 4, dtype=np.uint8).tobytes(), d) for _ in range(2 * K - 1)]
    one = np.zeros(d, np.uint64)
    one[0] = 1
    rc.append(one)  # get_rhos pushes ONE last (folding/utils.rs:123-126)
    return O.crt(np.concatenate(rc), d)


def make_step(A, kappa, d, W, seed):
    """one step's inputs and buffers, with packed planes and no f_k rows"""
    pr = LA.goldilocks_dp(d)
    K, N = pr.K, W * pr.L
    w_ccs = O.fill_uniform(W * d, seed)
    acc_fc, acc_f = O.witness_from_w_ccs(O.fill_uniform(W * d, seed + 1), d, pr.B, pr.L)
    acc_cm = O.ajtai_commit(A, kappa, N, d, acc_f)
    rho = make_rho(d, K, seed + 2)
    plen = max(LA.fold_step_planes_len(pr, N), 64)
    keep = {
        "w_ccs": dev(w_ccs), "acc_cm": dev(acc_cm), "acc_f_coeff": dev(acc_fc), "rho": dev(rho),
        "f_coeff": dev(n=N * d), "f": dev(n=N * d), "cm": dev(n=kappa * d),
        "fk_coeff": [None, None], "fk": [None, None],
        "wk": [dev(n=K * W * d) for _ in range(2)], "y": [dev(n=K * kappa * d) for _ in range(2)],
        "f0": dev(n=N * d), "f0_coeff": dev(n=N * d), "w_ccs0": dev(n=W * d), "cm0": dev(n=kappa * d),
        "planes": [dev(n=plen) for _ in range(2)],
    }
    b = LA.LfFoldStepBufs()
    for k, v in keep.items():
        if isinstance(v, list):
            for s in range(2):
                getattr(b, k)[s] = v[s].data_ptr() if v[s] is not None else None
        else:
            setattr(b, k, v.data_ptr())
    return keep, b, pr


@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("d,W,kappa", [(64, 17, 2), (1024, 16, 2), (24, 17, 3)])
def test_fold_step_equals_materialised_scheme(ctx, kname, d, W, kappa):
    import torch
    N = W * 5
    A = expanded(kname, d, kappa, N)
    outs = []
    for sch in (seeded(ctx, kname, d, kappa, N), LA.AjtaiCommitmentScheme(ctx, A)):
        keep, b, pr = make_step(A, kappa, d, W, 500 + d)
        torch.cuda.synchronize()
        ctx.dev_fold_step(sch, pr, W, b)
        ctx.sync()
        outs.append(keep)
    got, want = outs
    for key in ("f_coeff", "f", "cm", "f0", "f0_coeff", "w_ccs0", "cm0"):
        assert np.array_equal(host(got[key]), host(want[key])), key
    for key in ("wk", "y", "planes"):
        for s in range(2):
            assert np.array_equal(host(got[key][s]), host(want[key][s])), f"{key}[{s}]"
    # and the step's own commitment is the oracle's on the expanded matrix
    assert np.array_equal(host(got["cm"]), O.ajtai_commit(A, kappa, N, d, host(got["f"])))


def assert_same_step_outputs(got, want):
    for key in ("f_coeff", "f", "cm", "f0", "f0_coeff", "w_ccs0", "cm0"):
        assert np.array_equal(host(got[key]), host(want[key])), key
    for key in ("wk", "y", "planes"):
        for s in range(2):
            assert np.array_equal(host(got[key][s]), host(want[key][s])), f"{key}[{s}]"


# d = 4096, kappa = 2, W = 200: 1000 columns are nch = 33 chunks, 26 below the top region and 7
# in it, for 65536 / 4096 = 16 chunk walkers -- a writer block takes two or three chunks (it
# reuses its tile and carries its sums), walkers 10 .. 15 meet both chunk classes, and the row
# sums add walkers that each did more than one chunk. The other shapes of this file have fewer
# chunks than walkers. d = 64, 24: the small shapes of the step test, for the batch.
WALK = (4096, 200, 2)


@pytest.mark.parametrize("kname", sorted(KINDS))
def test_chunk_walk_commits_and_step(ctx, kname):
    import torch
    d, W, kappa = WALK
    N = W * 5
    A = expanded(kname, d, kappa, N)
    sch, mat = seeded(ctx, kname, d, kappa, N), LA.AjtaiCommitmentScheme(ctx, A)
    assert sch.layout == 1 and mat.device_bytes - sch.device_bytes == kappa * N * d * 8
    fs = [O.fill_uniform(N * d, 900 + i) for i in range(3)]
    cs = dev_commits(ctx, sch, fs)
    assert np.array_equal(cs, dev_commits(ctx, mat, fs))
    assert np.array_equal(cs[0], O.ajtai_commit(A, kappa, N, d, fs[0]))
    outs = []
    for s in (sch, mat):
        keep, b, pr = make_step(A, kappa, d, W, 910)
        torch.cuda.synchronize()
        ctx.dev_fold_step(s, pr, W, b)
        ctx.sync()
        outs.append(keep)
    assert_same_step_outputs(*outs)
    assert np.array_equal(host(outs[0]["cm"]), O.ajtai_commit(A, kappa, N, d, host(outs[0]["f"])))


@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("d,W,kappa", [(64, 17, 2), (24, 17, 3), WALK])
def test_batched_steps_read_all_three_row_sum_tables(monkeypatch, kname, d, W, kappa):
    """two steps in one lf_dev_fold_step_batch with the top class on: the contraction of the
    chunks below the top region adds the second row-sum table, that of the top region the third"""
    import torch
    monkeypatch.setenv("LATTICEUM_AMD_TOPCLASS", "1")
    N = W * 5
    A = expanded(kname, d, kappa, N)
    ctxs = [LA.Context(0) for _ in range(2)]
    try:
        outs = []
        for which in ("seeded", "materialised"):
            s = seeded(ctxs[0], kname, d, kappa, N) if which == "seeded" else LA.AjtaiCommitmentScheme(ctxs[0], A)
            steps = [make_step(A, kappa, d, W, 930 + 10 * i) for i in range(2)]
            torch.cuda.synchronize()
            ctxs[0].dev_fold_step_batch(ctxs[1:], s, steps[0][2], W, [st[1] for st in steps])
            for c in ctxs:
                c.sync()
            outs.append([st[0] for st in steps])
        for got, want in zip(*outs):
            assert_same_step_outputs(got, want)
            assert np.array_equal(host(got["cm"]), O.ajtai_commit(A, kappa, N, d, host(got["f"])))
    finally:
        for c in ctxs:
            c.close()


def test_dev_expand_refuses_a_misaligned_destination(ctx):
    out = dev(n=2 * 3 * 16 + 1)
    with pytest.raises(LA.LfError) as e:
        ctx.check(ctx.lib.lf_dev_ajtai_seeded_expand(ctx.h, LA._ptr(LA._seed4([1, 2, 3, 4])), LA.AJTAI_SEED_POSEIDON2,
                                                     2, 3, 16, 0, 2, 0, 3, out.data_ptr() + 8))
    assert e.value.code == 1


# ---------------------------------------------------------------- shards, memory
@pytest.mark.parametrize("kname", sorted(KINDS))
def test_column_shards_sum_to_the_whole(ctx, kname):
    d, kappa, W, L = 64, 2, 32, 5
    N = W * L
    full = seeded(ctx, kname, d, kappa, N)
    f = O.fill_uniform(N * d, 71)
    whole = full.commit_ntt(f).astype(object)
    parts = []
    for col0 in (0, 80):
        sh = seeded(ctx, kname, d, kappa, 80, col0=col0, ncols_total=N)
        assert sh.layout == 1 and sh.width == 80
        parts.append(sh.commit_ntt(f[col0 * d:(col0 + 80) * d]).astype(object))
        # a shard is the scheme of the expansion's window
        win = LA.AjtaiCommitmentScheme(ctx, expanded(kname, d, kappa, N, col0, 80))
        assert np.array_equal(win.commit_ntt(f[col0 * d:(col0 + 80) * d]).astype(object), parts[-1])
    assert np.array_equal((parts[0] + parts[1]) % P, whole)
    assert not np.array_equal(parts[0], parts[1])


@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("d,kappa,ncols", [(24, 3, 35), (256, 9, 45), (4096, 2, 5)])
def test_seeded_scheme_holds_no_u64_matrix(ctx, kname, d, kappa, ncols):
    sch = seeded(ctx, kname, d, kappa, ncols)
    mat = LA.AjtaiCommitmentScheme(ctx, expanded(kname, d, kappa, ncols))
    assert sch.layout == 1 and mat.layout == 1
    assert mat.device_bytes - sch.device_bytes == kappa * ncols * d * 8
    assert sch.device_bytes > 0


def test_scheme_without_fragments_owns_its_window(ctx):
    d, kappa, ncols = 16, 130, 130
    sch = seeded(ctx, "poseidon2", d, kappa, ncols)
    assert sch.layout == 0 and sch.device_bytes == kappa * ncols * d * 8
