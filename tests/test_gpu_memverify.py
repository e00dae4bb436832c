"""The device opening checks: k_merkle_verify through lf_dev_merkle_verify, and
lf_memtree_verify / lf_memtree_audit on the records MemTree.apply returns.

The model is the oracle alone: a record opens its root when O.p2w8_hash of its row,
folded with its path by O.p2w8_compress in the order the index's bits give, equals the
root (and the index is below the row count); model_audit applies lf.h's four checks in
order with that. Every device answer is compared with the model's, and every tampered
input must be rejected where the model rejects it. Memories are O.fill_uniform values:
with equal siblings compress(a, a) would hide a flipped index bit."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O

pytestmark = pytest.mark.gpu

P = LA.P
INDEX, VALUE, OPENING, TRANSITION = LA.MEMLOG_INDEX, LA.MEMLOG_VALUE, LA.MEMLOG_OPENING, LA.MEMLOG_TRANSITION


@pytest.fixture(scope="module")
def ctx():
    c = LA.Context(0)
    yield c
    c.close()


def layer_sizes(nrows):
    n = 1 if nrows <= 1 else nrows + nrows % 2
    out = [n]
    while n > 1:
        n = 1 if n == 2 else (n // 2 + 1) & ~1
        out.append(n)
    return out


def open_path(nodes, nrows, index):
    path, off, i = [], 0, index
    for n in layer_sizes(nrows)[:-1]:
        path.append(nodes[off + (i ^ 1)])
        off += n
        i //= 2
    return np.array(path, np.uint64).reshape(-1, 4)


_folds = {}


def fold_root(row, path, index):
    """verify_batch in the oracle's primitives (cached: the tests re-open the same records)"""
    row, path = np.ascontiguousarray(row, dtype=np.uint64), np.ascontiguousarray(path, dtype=np.uint64)
    key = (row.tobytes(), path.tobytes(), int(index))
    if key not in _folds:
        dg, i = O.p2w8_hash(row), int(index)
        for sib in path.reshape(-1, 4):
            dg = O.p2w8_compress(dg, sib) if i % 2 == 0 else O.p2w8_compress(sib, dg)
            i //= 2
        _folds[key] = dg
    return _folds[key]


def opens(row, path, index, root, nrows):
    return int(index) < nrows and np.array_equal(fold_root(row, path, index), root)


def bump(a, at):
    """a copy with one word replaced by another canonical value"""
    b = np.array(a, np.uint64).copy()
    flat = b.reshape(-1)
    flat[at] = np.uint64((int(flat[at]) + 1) % P)
    return b


# ---------------------------------------------------------------- lf_dev_merkle_verify
SHAPES = [(1, 4), (2, 1), (3, 2), (5, 4), (6, 9), (13, 4), (16, 8)]
KS = [1, 7, 8, 9, 31, 32, 33, 257]  # the 8-lane group, the wave and the 256-thread block edges


def dev(a, device):
    import torch
    a = np.ascontiguousarray(a)
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view).reshape(-1).copy()).to(device)


def run_dev_verify(ctx, rows, width, nrows, index, paths, roots, one_root):
    """-> the k status bytes; the 8 bytes after them must come back untouched"""
    import torch
    device = f"cuda:{ctx.device}"
    k = index.size
    ok = torch.full((k + 8,), 7, dtype=torch.uint8, device=device)
    d_paths = dev(paths, device) if paths.size else None
    ctx.dev_merkle_verify(dev(rows, device), k, width, nrows, dev(index, device), d_paths, dev(roots, device),
                          one_root, ok)
    ctx.sync()
    got = ok.cpu().numpy()
    assert np.all(got[k:] == 7), "a group past k stored a status"
    return got[:k]


def records(nrows, width, k, first, tree):
    """k records cycling over all indices from `first`"""
    rows_all, nodes = tree
    idx = (first + np.arange(k)) % nrows
    rows = rows_all[idx].copy()
    depth = len(layer_sizes(nrows)) - 1
    paths = np.array([open_path(nodes, nrows, int(i)) for i in idx], np.uint64).reshape(k, depth, 4)
    roots = np.tile(nodes[-1], (k, 1))
    return rows, idx.astype(np.uint32), paths, roots


def corrupt(rng, rows, index, paths, roots, j, nrows, kinds):
    kind = kinds[int(rng.integers(0, len(kinds)))]
    if kind == "row":
        rows[j] = bump(rows[j], int(rng.integers(0, rows.shape[1])))
    elif kind == "path":
        lv = int(rng.integers(0, paths.shape[1]))
        paths[j, lv] = bump(paths[j, lv], int(rng.integers(0, 4)))
    elif kind == "root":
        roots[j] = bump(roots[j], int(rng.integers(0, 4)))
    elif kind == "index":  # at or past nrows
        index[j] = [nrows, nrows + 1 + int(rng.integers(0, 1000)), 0xFFFFFFFF][int(rng.integers(0, 3))]
    else:  # another row's index
        index[j] = (int(index[j]) + 1 + int(rng.integers(0, nrows - 1))) % nrows


@pytest.mark.parametrize("nrows,width", SHAPES)
def test_dev_merkle_verify(ctx, nrows, width):
    rows_all = O.fill_uniform(nrows * width, 100 * nrows + width).reshape(nrows, width)
    tree = (rows_all, O.merkle_tree(rows_all.reshape(-1), nrows, width).reshape(-1, 4))
    rng = np.random.default_rng(7 * nrows + width)
    depth = len(layer_sizes(nrows)) - 1
    assert LA.merkle_path_len(nrows) == depth
    for k in KS:
        for one_root in (False, True):
            rows, index, paths, roots = records(nrows, width, k, int(rng.integers(0, nrows)), tree)
            kinds = ["row", "index"] + (["path"] if depth else []) + ([] if one_root else ["root"]) + \
                    (["other"] if nrows > 1 else [])
            for j in np.flatnonzero(rng.integers(0, 3, k) == 0):  # a seeded third
                corrupt(rng, rows, index, paths, roots, int(j), nrows, kinds)
            want = np.array([opens(rows[j], paths[j], index[j], roots[j], nrows) for j in range(k)], np.uint8)
            got = run_dev_verify(ctx, rows, width, nrows, index, paths, roots[0] if one_root else roots, one_root)
            assert np.array_equal(got, want), (k, one_root, got, want)
    # an all-good batch, and an all-bad one: every record against one wrong shared root
    rows, index, paths, roots = records(nrows, width, 33, 0, tree)
    assert all(opens(rows[j], paths[j], index[j], roots[j], nrows) for j in range(33))
    assert np.all(run_dev_verify(ctx, rows, width, nrows, index, paths, roots, False) == 1)
    assert np.all(run_dev_verify(ctx, rows, width, nrows, index, paths, roots[0], True) == 1)
    bad = bump(roots[0], 3)
    assert not any(opens(rows[j], paths[j], index[j], bad, nrows) for j in range(33))
    assert np.all(run_dev_verify(ctx, rows, width, nrows, index, paths, bad, True) == 0)


def test_dev_merkle_verify_nothing_to_do(ctx):
    import torch
    ok = torch.full((4,), 7, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    ctx.dev_merkle_verify(0, 0, 4, 5, 0, None, 0, False, ok)  # k == 0: no launch, nothing read
    ctx.sync()
    assert np.all(ok.cpu().numpy() == 7)


# ---------------------------------------------------------------- the memory records
def memory(pages, wpp, seed):
    return (O.fill_uniform(pages * wpp, seed) % (1 << 32)).astype(np.uint32)


def addr(wpp, page, word, low=0):
    return ((page * wpp + word) << 2) | low


def seeded_batch(pages, wpp, seed):
    """the op patterns where the indexing can go wrong, on a memory of `seed`"""
    mem = memory(pages, wpp, seed)
    rng = np.random.default_rng(seed)
    val = lambda: int(rng.integers(0, 1 << 32))
    last, w1 = pages - 1, wpp - 1
    ops = []

    def push(page, word, value, is_write, low=0):
        if is_write:
            mem[page * wpp + word] = value
        ops.append((addr(wpp, page, word, low), value, is_write))

    # the same word written twice in a row with different values
    push(0, 0, 0xDEADBEEF, 1)
    push(0, 0, 0x12345678, 1)
    # two words of one page (the low address bits are dropped)
    push(last, 0, val(), 1)
    push(last, w1, val(), 1, low=3)
    # a sibling pair in consecutive ops, twice: the path's first digest is the other op's version
    for i in range(pages // 2):
        push(2 * i, 0, val(), 1)
        push(2 * i + 1, w1, val(), 1)
        push(2 * i, w1, val(), 1)
        push(2 * i + 1, 0, val(), 1)
    # a read between two writes of one page
    mid = pages // 2
    push(mid, 0, val(), 1)
    push(mid, w1, 77, 0)
    push(mid, w1, val(), 1)
    # writes of the old value: a word written above, a word never written
    push(last, 0, int(mem[last * wpp]), 1)
    push(mid, wpp // 2, int(mem[mid * wpp + wpp // 2]), 1)
    # the last page (odd counts: its sibling is a zero-digest padding node), reads and writes
    push(last, w1, val(), 1)
    push(last, 0, 5, 0)
    push(last, 0, val(), 1)
    # and a seeded tail over the whole memory
    for _ in range(8):
        w = int(rng.integers(0, pages * wpp))
        push(w // wpp, w % wpp, val(), int(rng.integers(0, 2)))
    return ops


def make_log(ctx, pages, wpp, ops, seed):
    """the records MemTree.apply returns for ops on a memory of `seed`, the start root read
    before the batch, and the word before every op from a numpy mirror"""
    mem = memory(pages, wpp, seed)
    ops = np.array(ops, np.uint32).reshape(-1, 3)
    t = ctx.memtree(mem, pages, wpp)
    try:
        start = t.root().copy()
        roots, pgs, paths, index = t.apply(ops)
    finally:
        t.close()
    old, mirror = np.zeros(len(ops), np.uint32), mem.copy()
    for j, (a, v, w) in enumerate(ops):
        old[j] = mirror[int(a) >> 2]
        if w:
            mirror[int(a) >> 2] = v
    return dict(pages=pages, wpp=wpp, mem=mem, start=start, ops=ops, old=old, roots=roots, pgs=pgs, paths=paths,
                index=index)


def copy_log(L):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in L.items()}


def model_audit(L, lo=0):
    """lf.h's checks in their order, op by op from `lo` (the ops before it are taken as good)"""
    pages, wpp = L["pages"], L["wpp"]
    for j in range(lo, len(L["ops"])):
        a, v, w = (int(x) for x in L["ops"][j])
        word = a >> 2
        page, wd = word // wpp, word % wpp
        pg, idx, path = L["pgs"][j], int(L["index"][j]), L["paths"][j]
        prev = L["roots"][j - 1] if j else L["start"]
        if page >= pages or idx != page:
            return j, INDEX
        if w and int(pg[wd]) != v:
            return j, VALUE
        if not opens(pg, path, idx, L["roots"][j], pages):
            return j, OPENING
        if w:
            pre = pg.copy()
            pre[wd] = L["old"][j]
            if not opens(pre, path, idx, prev, pages):
                return j, TRANSITION
        elif not np.array_equal(L["roots"][j], prev):
            return j, TRANSITION
    return -1, 0


def model_verify(L, lo=0):
    for j in range(lo, len(L["ops"])):
        if not opens(L["pgs"][j], L["paths"][j], L["index"][j], L["roots"][j], L["pages"]):
            return j
    return -1


def audit(ctx, L, old="log"):
    return ctx.memtree_audit(L["pages"], L["wpp"], L["start"], L["ops"], L["old"] if old == "log" else old, L["roots"],
                             L["pgs"], L["paths"], L["index"])


def verify(ctx, L):
    return ctx.memtree_verify(L["pages"], L["wpp"], L["roots"], L["pgs"], L["paths"], L["index"])


_logs = {}


def seeded_log(ctx, pages, wpp):
    """one log per shape, made once and never modified (the tests tamper copies)"""
    if (pages, wpp) not in _logs:
        seed = 10 * pages + wpp
        L = make_log(ctx, pages, wpp, seeded_batch(pages, wpp, seed), seed)
        # the start root and every record, by the oracle
        assert np.array_equal(L["start"], O.merkle_tree(L["mem"].astype(np.uint64), pages, wpp)[-4:])
        assert model_audit(L) == (-1, 0) and model_verify(L) == -1
        _logs[(pages, wpp)] = L
    return _logs[(pages, wpp)]


@pytest.mark.parametrize("pages,wpp", [(1, 4), (2, 1), (3, 2), (5, 4), (8, 8), (13, 4)])
def test_honest_logs_pass(ctx, pages, wpp):
    L = seeded_log(ctx, pages, wpp)
    assert L["paths"].shape[1] == LA.merkle_path_len(pages)
    assert verify(ctx, L) == -1
    assert audit(ctx, L) == (-1, 0)


# one tampering at op j, by name -> the check that must report it
def tamper(L, j, what):
    a, v, w = (int(x) for x in L["ops"][j])
    pages, wpp = L["pages"], L["wpp"]
    wd = (a >> 2) % wpp
    if what == "page_index":
        L["index"][j] = (int(L["index"][j]) + 1) % pages if pages > 1 else 1
        return INDEX
    if what == "page_index_past":
        L["index"][j] = pages + 3
        return INDEX
    if what == "address_past":
        L["ops"][j, 0] = addr(wpp, pages, wd)
        return INDEX
    if what == "written_word":
        assert w
        L["pgs"][j, wd] ^= 1
        return VALUE
    if what == "other_word":
        L["pgs"][j, (wd + 1) % wpp] ^= 0x100
        return OPENING
    if what == "path":
        lv = j % L["paths"].shape[1]
        L["paths"][j, lv] = bump(L["paths"][j, lv], j % 4)
        return OPENING
    if what == "root":
        L["roots"][j] = bump(L["roots"][j], j % 4)
        return OPENING
    if what == "old_word":
        assert w
        L["old"][j] ^= 0x10
        return TRANSITION
    if what == "write_as_read":  # the record stays a valid opening: a read whose root differs from its predecessor's
        assert w and v != int(L["old"][j])
        L["ops"][j, 2] = 0
        return TRANSITION
    raise ValueError(what)


def changing_writes(L, lo=1):
    return [j for j in range(lo, len(L["ops"])) if L["ops"][j, 2] and L["ops"][j, 1] != L["old"][j]]


@pytest.mark.parametrize("what", ["page_index", "page_index_past", "address_past", "written_word", "other_word", "path",
                                  "root", "old_word", "write_as_read"])
def test_each_check_reports_its_tampering(ctx, what):
    L = copy_log(seeded_log(ctx, 13, 4))
    cand = changing_writes(L)
    j = cand[int(np.random.default_rng(len(what)).integers(0, len(cand)))]
    check = tamper(L, j, what)
    assert model_audit(L) == (j, check)
    assert audit(ctx, L) == (j, check)
    if what in ("other_word", "path", "root", "page_index", "page_index_past"):
        assert model_verify(L) == j
        assert verify(ctx, L) == j


def test_wrong_start_root(ctx):
    L = copy_log(seeded_log(ctx, 13, 4))
    L["start"] = bump(L["start"], 2)
    assert L["ops"][0, 2] == 1  # a write: its page with the old word back does not open the start root
    assert model_audit(L) == (0, TRANSITION)
    assert audit(ctx, L) == (0, TRANSITION)
    assert verify(ctx, L) == -1  # every record still opens its own root


def test_reads_only_log(ctx):
    """no write: old_words may be missing; op 0 is a read, so a wrong start root is a root comparison"""
    pages, wpp = 5, 4
    ops = [(addr(wpp, 4, 1), 9, 0), (addr(wpp, 0, 0), 0, 0), (addr(wpp, 3, 3, low=2), 1, 0)]
    L = make_log(ctx, pages, wpp, ops, 77)
    assert model_audit(L) == (-1, 0)
    assert audit(ctx, L, old=None) == (-1, 0)
    L["start"] = bump(L["start"], 0)
    assert model_audit(L) == (0, TRANSITION)
    assert audit(ctx, L, old=None) == (0, TRANSITION)


def test_two_tamperings_report_the_first(ctx):
    base = seeded_log(ctx, 13, 4)
    cand = changing_writes(base)
    j1, j2 = cand[2], cand[-2]
    assert j1 < j2
    for first, second in (("other_word", "path"), ("old_word", "written_word"), ("root", "page_index")):
        L = copy_log(base)
        tamper(L, j2, second)
        check = tamper(L, j1, first)
        assert model_audit(L) == (j1, check)
        assert audit(ctx, L) == (j1, check)


@pytest.mark.parametrize("pages,wpp", [(13, 4), (2, 1)])
def test_every_tampering_is_rejected(ctx, pages, wpp):
    """every op of the log, every tampering it admits: no miss, and the op and check the model names"""
    base = seeded_log(ctx, pages, wpp)
    n = 0
    for j in range(len(base["ops"])):
        w = int(base["ops"][j, 2])
        kinds = ["page_index", "page_index_past", "address_past", "root", "path"]
        kinds += ["other_word"] if wpp > 1 else []
        kinds += ["written_word", "old_word"] if w else []
        kinds += ["write_as_read"] if w and base["ops"][j, 1] != base["old"][j] else []
        for what in kinds:
            L = copy_log(base)
            check = tamper(L, j, what)
            assert model_audit(L, lo=j) == (j, check), (j, what)
            assert audit(ctx, L) == (j, check), (j, what)
            n += 1
    assert n > 5 * len(base["ops"])


def test_chunking(ctx):
    """chunk + 3 records: the tampering sits past the chunk boundary, the index reported is the global one"""
    pages, wpp = 8, 8
    k = LA.memtree_chunk() + 3
    rng = np.random.default_rng(99)
    ops = np.stack([rng.integers(0, pages * wpp, k) << 2, rng.integers(0, 1 << 32, k), rng.integers(0, 2, k)], 1)
    ops[k - 3:, 0] = [addr(wpp, 7, 0), addr(wpp, 6, 1), addr(wpp, 7, 2)]
    ops[k - 3:, 2] = 1
    L = make_log(ctx, pages, wpp, ops, 8)
    lo = k - 8  # the model opens the records around the boundary; the device checks all of them
    assert model_audit(L, lo) == (-1, 0) and model_verify(L, lo) == -1
    assert verify(ctx, L) == -1
    assert audit(ctx, L) == (-1, 0)
    for j, what in ((k - 2, "path"), (k - 1, "old_word"), (k - 3, "root")):
        T = copy_log(L)
        check = tamper(T, j, what)
        assert model_audit(T, lo) == (j, check)
        assert audit(ctx, T) == (j, check)
        if check == OPENING:
            assert verify(ctx, T) == j
    T = copy_log(L)
    tamper(T, k - 1, "path")
    tamper(T, k - 3, "other_word")
    assert model_audit(T, lo) == (k - 3, OPENING)
    assert audit(ctx, T) == (k - 3, OPENING) and verify(ctx, T) == k - 3
    # and a tampering in the first chunk is found before anything in the second
    T = copy_log(L)
    tamper(T, k - 2, "root")
    tamper(T, 17, "root")
    assert model_audit(T, 17) == (17, OPENING)
    assert audit(ctx, T) == (17, OPENING) and verify(ctx, T) == 17


def test_zkvm_shape(ctx):
    """8192 x 256, depth 13: the model costs one p2w8_hash and 13 p2w8_compress per opening"""
    pages, wpp = 8192, 256
    rng = np.random.default_rng(31)
    where = [(0, 0), (pages - 1, wpp - 1),            # address 0, the last word of the last page
             (4096, 7), (4097, 9), (4096, 8),          # two pages under one parent
             (100, 0), (8000, 255), (100, 1),          # opposite halves of the tree
             (pages - 1, 0), (0, wpp - 1)]
    where += [(int(rng.integers(0, pages)), int(rng.integers(0, wpp))) for _ in range(40 - len(where))]
    ops = [(addr(wpp, p, w), int(rng.integers(0, 1 << 32)), int(j % 5 != 3)) for j, (p, w) in enumerate(where)]
    L = make_log(ctx, pages, wpp, ops, 31)
    assert L["paths"].shape == (40, 13, 4)
    assert model_audit(L) == (-1, 0)
    assert verify(ctx, L) == -1
    assert audit(ctx, L) == (-1, 0)
    j = 23
    T = copy_log(L)
    T["paths"][j, 12] = bump(T["paths"][j, 12], 1)
    assert model_audit(T, j) == (j, OPENING)
    assert audit(ctx, T) == (j, OPENING)
    assert verify(ctx, T) == j


def test_arguments(ctx):
    L = seeded_log(ctx, 5, 4)
    none = np.zeros((0, 4), np.uint64)
    assert ctx.memtree_verify(5, 4, none, np.zeros(0, np.uint32), none, np.zeros(0, np.uint32)) == -1
    assert ctx.memtree_audit(5, 4, L["start"], np.zeros((0, 3), np.uint32), None, none, np.zeros(0, np.uint32), none,
                             np.zeros(0, np.uint32)) == (-1, 0)
    one = dict(roots=L["roots"][:1], paths=L["paths"][:1], index=L["index"][:1])
    for pages, wpp in ((5, 3), (5, 6), (0, 4), (1 << 29, 4)):
        pg = np.zeros(wpp, np.uint32)
        with pytest.raises(LA.LfError) as e:
            ctx.memtree_verify(pages, wpp, one["roots"], pg, one["paths"], one["index"])
        assert e.value.code == 1, (pages, wpp)
        with pytest.raises(LA.LfError) as e:
            ctx.memtree_audit(pages, wpp, L["start"], L["ops"][:1], L["old"][:1], one["roots"], pg, one["paths"],
                              one["index"])
        assert e.value.code == 1, (pages, wpp)
    assert np.any(L["ops"][:, 2] == 1)
    with pytest.raises(LA.LfError) as e:
        audit(ctx, L, old=None)  # a log with writes and no old words
    assert e.value.code == 1
