"""The persistent VM memory tree (lf_memtree_*): every record of a batch -- root,
page, path, page index -- and the device tree afterwards, bit-exact against a
plain model: apply the op to a numpy memory, then O.merkle_tree of the whole
memory (the 8192 x 256 case updates one oracle tree node by node instead)."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = LA.Context(0)
    yield c
    c.close()


def layer_sizes(pages):
    n = 1 if pages <= 1 else pages + pages % 2
    out = [n]
    while n > 1:
        n = 1 if n == 2 else (n // 2 + 1) & ~1
        out.append(n)
    return out


def memory(pages, wpp, seed):
    return (O.fill_uniform(pages * wpp, seed) % (1 << 32)).astype(np.uint32)


def addr(wpp, page, word, low=0):
    return ((page * wpp + word) << 2) | low


def open_path(nodes, pages, index):
    """the sibling in every padded layer below the root, leaves first"""
    path, off, i = [], 0, index
    for n in layer_sizes(pages)[:-1]:
        path.append(nodes[off + (i ^ 1)])
        off += n
        i //= 2
    return np.array(path, np.uint64).reshape(-1, 4)


def model(mem, pages, wpp, ops):
    """(records, memory, nodes) after the ops, a full rebuild per op"""
    mem = mem.copy()
    recs, nodes = [], None
    for a, v, w in ops:
        word = int(a) >> 2
        page = word // wpp
        if w:
            mem[word] = v
        nodes = O.merkle_tree(mem.astype(np.uint64), pages, wpp).reshape(-1, 4)
        recs.append((nodes[-1].copy(), mem[page * wpp:(page + 1) * wpp].copy(), open_path(nodes, pages, page), page))
    return recs, mem, nodes


def fold_root(page_words, path, index):
    """verify_batch: the page's hash folded with the path"""
    dg, i = O.p2w8_hash(page_words.astype(np.uint64)), index
    for sib in path:
        dg = O.p2w8_compress(dg, sib) if i % 2 == 0 else O.p2w8_compress(sib, dg)
        i //= 2
    return dg


def check_records(got, recs, depth, fold=True):
    roots, pgs, paths, index = got
    assert roots.shape == (len(recs), 4) and paths.shape == (len(recs), depth, 4)
    for j, (root, page_words, path, page) in enumerate(recs):
        assert np.array_equal(roots[j], root), ("root", j)
        assert np.array_equal(pgs[j], page_words), ("page", j)
        assert np.array_equal(paths[j], path), ("path", j)
        assert index[j] == page, ("page index", j)
        if fold:
            assert np.array_equal(fold_root(pgs[j], paths[j], int(index[j])), roots[j]), ("fold", j)


def run_case(ctx, pages, wpp, ops, seed=1, fold=True):
    mem = memory(pages, wpp, seed)
    t = ctx.memtree(mem, pages, wpp)
    try:
        assert t.depth == LA.merkle_depth(pages) == len(layer_sizes(pages)) - 1
        assert np.array_equal(t.nodes(), O.merkle_tree(mem.astype(np.uint64), pages, wpp))
        got = t.apply(ops)
        recs, _, nodes = model(mem, pages, wpp, ops)
        check_records(got, recs, t.depth, fold)
        assert np.array_equal(t.nodes().reshape(-1, 4), nodes)
        assert np.array_equal(t.root(), recs[-1][0])
    finally:
        t.close()
    return got


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

    # the same address written twice in a row with different values
    push(0, 0, 0xDEADBEEF, 1)
    push(0, 0, 0x12345678, 1)
    # two words of one page (the low address bits are dropped)
    push(last, 0, val(), 1)
    push(last, w1, val(), 1, low=3)
    # pages 2i and 2i + 1 in consecutive ops, then the same pair again: the sibling is a version, not the base
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
    # writes whose value equals the old one: a word written above, a word never written
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


@pytest.mark.parametrize("pages,wpp", [(1, 4), (2, 1), (3, 2), (5, 4), (8, 8), (13, 4)])
def test_small_shapes(ctx, pages, wpp):
    ops = seeded_batch(pages, wpp, 10 * pages + wpp)
    _, _, paths, _ = run_case(ctx, pages, wpp, ops, seed=10 * pages + wpp)
    if pages == 1:  # depth 0: empty paths, root = the leaf hash (checked by the fold)
        assert paths.shape[1] == 0


def test_value_equal_to_the_old_one(ctx):
    """a write of the word's current value: the record equals a read's"""
    pages, wpp = 5, 4
    mem = memory(pages, wpp, 3)
    ops = [(addr(wpp, 2, 1), int(mem[2 * wpp + 1]), 1), (addr(wpp, 2, 1), 0, 0)]
    roots, _, _, _ = run_case(ctx, pages, wpp, ops, seed=3)
    assert np.array_equal(roots[0], roots[1])
    assert np.array_equal(roots[0], O.merkle_tree(mem.astype(np.uint64), pages, wpp)[-4:])


@pytest.mark.parametrize("k", [1, 7, 9, 33, 70])
def test_group_and_wave_edges(ctx, k):
    """a wave whose 8-lane groups are partly idle; more groups than one 256-thread block holds"""
    pages, wpp = 13, 4
    rng = np.random.default_rng(k)
    ops = [(int(rng.integers(0, pages * wpp)) << 2, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 4) > 0))
           for _ in range(k)]
    run_case(ctx, pages, wpp, ops, seed=40 + k)


def test_chunking(ctx):
    """one batch of chunk + 3 ops: the records across the boundary equal the model,
    and the same ops in two calls give identical records"""
    pages, wpp = 5, 4
    k = LA.memtree_chunk() + 3
    rng = np.random.default_rng(99)
    ops = np.stack([rng.integers(0, pages * wpp, k) << 2, rng.integers(0, 1 << 32, k), rng.integers(0, 2, k)], 1)
    # the ops on both sides of the boundary share pages and siblings
    ops[k - 6:, 0] = [addr(wpp, 4, 0), addr(wpp, 2, 1), addr(wpp, 3, 0), addr(wpp, 2, 2), addr(wpp, 4, 3),
                      addr(wpp, 3, 1)]
    ops[k - 6:, 2] = 1
    one = run_case(ctx, pages, wpp, ops, seed=8, fold=False)
    t = ctx.memtree(memory(pages, wpp, 8), pages, wpp)
    cut = k - 4
    a, b = t.apply(ops[:cut]), t.apply(ops[cut:])
    for x, y, z in zip(one, a, b):
        assert np.array_equal(x, np.concatenate([y, z]))
    for j in range(k - 8, k):
        assert np.array_equal(fold_root(one[1][j], one[2][j], int(one[3][j])), one[0][j])
    t.close()


def test_state_carries_over(ctx):
    """the second call's first op has its sibling written by the first call"""
    pages, wpp = 13, 4
    mem = memory(pages, wpp, 21)
    first = [(addr(wpp, 6, 1), 111, 1), (addr(wpp, 12, 3), 222, 1), (addr(wpp, 7, 0), 333, 1)]
    second = [(addr(wpp, 6, 2), 444, 1), (addr(wpp, 12, 0), 0, 0), (addr(wpp, 0, 0), 555, 1)]
    t = ctx.memtree(mem, pages, wpp)
    recs, mem1, _ = model(mem, pages, wpp, first)
    check_records(t.apply(first), recs, t.depth)
    assert np.array_equal(t.root(), recs[-1][0])
    # nothing to do: LF_OK, nothing changes
    empty = t.apply(np.zeros((0, 3), np.uint32))
    assert empty[0].shape == (0, 4) and np.array_equal(t.root(), recs[-1][0])
    recs, _, nodes = model(mem1, pages, wpp, second)
    got = t.apply(second)
    check_records(got, recs, t.depth)
    assert np.array_equal(got[2][0][0], O.p2w8_hash(mem1[7 * wpp:8 * wpp].astype(np.uint64)))
    assert np.array_equal(t.root(), got[0][-1])
    assert np.array_equal(t.nodes().reshape(-1, 4), nodes)
    t.close()


def tree_by_parts(rows, pages, wpp, parts=16):
    """O.merkle_tree of a power-of-two tree in a fraction of the time: the `parts`
    subtrees in threads (the oracle call releases the GIL), joined with p2w8_compress"""
    from concurrent.futures import ThreadPoolExecutor
    sub = pages // parts
    with ThreadPoolExecutor(parts) as ex:
        subs = list(ex.map(lambda i: O.merkle_tree(rows[i * sub * wpp:(i + 1) * sub * wpp], sub, wpp).reshape(-1, 4),
                           range(parts)))
    layers, off, n = [], 0, sub
    while n >= 1:
        layers.append(np.concatenate([s[off:off + n] for s in subs]))
        off, n = off + n, n // 2
    while len(layers[-1]) > 1:
        lv = layers[-1]
        layers.append(np.array([O.p2w8_compress(lv[2 * i], lv[2 * i + 1]) for i in range(len(lv) // 2)]))
    return np.concatenate(layers)


def test_zkvm_shape(ctx):
    """8192 x 256: one oracle tree updated node by node (one p2w8_hash and 13
    p2w8_compress per op); one full rebuild at the end checks the device tree"""
    pages, wpp = 8192, 256
    mem = memory(pages, wpp, 31)
    rng = np.random.default_rng(31)
    where = [(0, 0), (pages - 1, wpp - 1),            # address 0, the last word of the last page
             (4096, 7), (4097, 9), (4096, 8),          # two pages under one parent
             (100, 0), (8000, 255), (100, 1),          # opposite halves of the tree
             (pages - 1, 0), (0, wpp - 1)]
    where += [(int(rng.integers(0, pages)), int(rng.integers(0, wpp))) for _ in range(24 - len(where))]
    ops = [(addr(wpp, p, w), int(rng.integers(0, 1 << 32)), int(j % 5 != 3)) for j, (p, w) in enumerate(where)]
    assert len(ops) == 24
    t = ctx.memtree(mem, pages, wpp)
    assert t.depth == 13
    nodes = tree_by_parts(mem.astype(np.uint64), pages, wpp)
    assert np.array_equal(t.nodes().reshape(-1, 4), nodes)
    got = t.apply(ops)
    recs = []
    for a, v, w in ops:
        word = a >> 2
        page = word // wpp
        if w:
            mem[word] = v
        off, i, n = 0, page, pages
        nodes[page] = O.p2w8_hash(mem[page * wpp:(page + 1) * wpp].astype(np.uint64))
        while n > 1:
            parent = O.p2w8_compress(nodes[off + (i & ~1)], nodes[off + (i | 1)])
            off, i, n = off + n, i // 2, n // 2
            nodes[off + i] = parent
        recs.append((nodes[-1].copy(), mem[page * wpp:(page + 1) * wpp].copy(), open_path(nodes, pages, page), page))
    check_records(got, recs, 13)
    assert np.array_equal(t.root(), recs[-1][0])
    assert np.array_equal(t.nodes(), O.merkle_tree(mem.astype(np.uint64), pages, wpp))
    t.close()


def test_errors(ctx):
    pages, wpp = 5, 4
    mem = memory(pages, wpp, 51)
    t = ctx.memtree(mem, pages, wpp)
    root, nodes = t.root(), t.nodes()
    good = [(addr(wpp, 1, 1), 9, 1), (addr(wpp, 4, 3), 8, 1)]
    past = addr(wpp, pages, 0)
    for bad in ([(past, 1, 1)] + good, good[:1] + [(past, 1, 0)] + good[1:], good + [(0xFFFFFFFC, 1, 1)]):
        with pytest.raises(LA.LfError) as e:
            t.apply(bad)
        assert e.value.code != 0
        assert np.array_equal(t.root(), root) and np.array_equal(t.nodes(), nodes)
    # the handle still works, from the unchanged memory
    recs, _, _ = model(mem, pages, wpp, good)
    check_records(t.apply(good), recs, t.depth)
    t.close()
    for wpp_bad in (3, 6, 0):
        with pytest.raises(LA.LfError):
            ctx.memtree(np.zeros(pages * wpp_bad, np.uint32), pages, wpp_bad)
