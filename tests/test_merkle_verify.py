"""lf_merkle_path_len and lf_merkle_verify (verify_memory_opening, zkvm
commitments.rs:264-288) on the host, against the oracle: every index of oracle trees
opens its root under the path read off the oracle's node array, and one flipped bit of
the row, of any path digest or of the root, or the neighbouring index, does not. The
rows are O.fill_uniform values: with equal siblings compress(a, a) would hide a
flipped index bit. Host code only (no device call)."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O

SHAPES = [(1, 4), (2, 1), (3, 2), (5, 4), (6, 9), (13, 4), (16, 8)]


def layer_sizes(nrows):
    """the padded layers of a tree over nrows rows, leaves first, the root's last"""
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


def fold_root(row, path, index):
    """the model: the row's sponge folded with the path by the index's bits"""
    dg, i = O.p2w8_hash(row), index
    for sib in path:
        dg = O.p2w8_compress(dg, sib) if i % 2 == 0 else O.p2w8_compress(sib, dg)
        i //= 2
    return dg


def tree(nrows, width):
    rows = O.fill_uniform(nrows * width, 100 * nrows + width)
    return rows.reshape(nrows, width), O.merkle_tree(rows, nrows, width).reshape(-1, 4)


def flipped(a, word, bit):
    b = np.array(a, np.uint64).copy()
    b.reshape(-1)[word] ^= np.uint64(1 << bit)
    return b


@pytest.mark.parametrize("nrows", list(range(1, 41)) + [8192])
def test_path_len(nrows):
    want = len(layer_sizes(nrows)) - 1
    assert LA.merkle_path_len(nrows) == want == LA.merkle_depth(nrows)
    assert sum(layer_sizes(nrows)) == O.merkle_nodes(nrows)  # the model's layers are the oracle's


@pytest.mark.parametrize("nrows,width", SHAPES)
def test_accepts_every_index(nrows, width):
    rows, nodes = tree(nrows, width)
    for i in range(nrows):
        path = open_path(nodes, nrows, i)
        assert np.array_equal(fold_root(rows[i], path, i), nodes[-1])  # the model agrees with the oracle tree
        assert LA.merkle_verify(nodes[-1], rows[i], nrows, i, path), i
    if nrows == 1:
        assert np.array_equal(nodes[-1], O.p2w8_hash(rows[0]))  # depth 0: the root is the leaf digest


@pytest.mark.parametrize("nrows,width", SHAPES)
def test_rejects_one_flipped_bit(nrows, width):
    rows, nodes = tree(nrows, width)
    rng = np.random.default_rng(nrows * 31 + width)
    root = nodes[-1]
    lib = LA.load()
    for i in range(nrows):
        path = open_path(nodes, nrows, i)
        bit = lambda: int(rng.integers(0, 64))  # any bit: 2^b != 0 mod p, so the residue changes
        assert not LA.merkle_verify(root, flipped(rows[i], int(rng.integers(0, width)), bit()), nrows, i, path)
        for lv in range(path.shape[0]):
            assert not LA.merkle_verify(root, rows[i], nrows, i, flipped(path, 4 * lv + int(rng.integers(0, 4)), bit()))
        bad_root = flipped(root, int(rng.integers(0, 4)), bit())
        assert not LA.merkle_verify(bad_root, rows[i], nrows, i, path)
        # the status itself, through the C ABI
        rc = lib.lf_merkle_verify(bad_root.ctypes.data, np.ascontiguousarray(rows[i]).ctypes.data, width, nrows, i,
                                  path.ctypes.data if path.size else None)
        assert rc == LA.ERR_VERIFICATION == 12
        if (i ^ 1) < nrows:
            assert not LA.merkle_verify(root, rows[i], nrows, i ^ 1, path)
            assert not np.array_equal(fold_root(rows[i], path, i ^ 1), root)


def test_invalid_arguments():
    nrows, width = 5, 4
    rows, nodes = tree(nrows, width)
    path = open_path(nodes, nrows, 0)
    lib = LA.load()
    row = np.ascontiguousarray(rows[0])
    call = lambda root, r, w, n, i, p: lib.lf_merkle_verify(root, r, w, n, i, p)
    assert call(nodes[-1].ctypes.data, row.ctypes.data, width, nrows, 0, path.ctypes.data) == 0
    for n, w, i in ((nrows, width, nrows), (nrows, width, nrows + 1), (nrows, width, 8), (0, width, 0),
                    (nrows, 0, 0)):
        assert call(nodes[-1].ctypes.data, row.ctypes.data, w, n, i, path.ctypes.data) == 1, (n, w, i)
    assert call(None, row.ctypes.data, width, nrows, 0, path.ctypes.data) == 1
    assert call(nodes[-1].ctypes.data, None, width, nrows, 0, path.ctypes.data) == 1
    assert call(nodes[-1].ctypes.data, row.ctypes.data, width, nrows, 0, None) == 1
    with pytest.raises(LA.LfError) as e:
        LA.merkle_verify(nodes[-1], rows[0], nrows, nrows, path)
    assert e.value.code == 1
