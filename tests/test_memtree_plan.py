"""The dependency tables of a batch of memory ops (lf_memtree_plan, host only)
against a brute-force double loop over their definition:
  prev[j][l] = the largest j' < j with (p_j' >> l) == ((p_j >> l) ^ 1), or -1
  last[j][l] = 1 if no j'' > j has (p_j'' >> l) == (p_j >> l), l = 0..depth"""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O

PAGES = (1, 2, 3, 5, 8, 13)


def brute(pages, pg):
    depth, k = LA.merkle_depth(pages), len(pg)
    prev = np.full((k, depth), -1, np.int32)
    last = np.ones((k, depth + 1), np.uint8)
    for j in range(k):
        for l in range(depth + 1):
            for j2 in range(j + 1, k):
                if pg[j2] >> l == pg[j] >> l:
                    last[j, l] = 0
            if l < depth:
                for j1 in range(j):
                    if pg[j1] >> l == (pg[j] >> l) ^ 1:
                        prev[j, l] = j1
    return prev, last


def op_lists(pages, k):
    """seeded random pages, one page repeated, a page and its sibling alternating
    (the last page and its sibling slot's neighbour where the count is odd), only
    the last page"""
    rng = np.random.default_rng(1000 * pages + k)
    a = (pages - 1) & ~1
    b = min(a + 1, pages - 1)  # a's sibling; for odd counts a is the last page and its sibling is padding
    return {
        "random": rng.integers(0, pages, k),
        "same": np.full(k, pages // 2),
        "siblings": np.array([a if j % 2 == 0 else b for j in range(k)], np.int64),
        "low_pair": np.array([j % 2 for j in range(k)], np.int64) % pages,
        "last_only": np.full(k, pages - 1),
    }


@pytest.mark.parametrize("pages", PAGES)
@pytest.mark.parametrize("k", [0, 1, 2, 40])
def test_plan_matches_definition(pages, k):
    depth = LA.merkle_depth(pages)
    assert depth == len(_layers(pages)) - 1
    for name, pg in op_lists(pages, k).items():
        prev, last = LA.memtree_plan(pages, pg)
        assert prev.shape == (k, depth) and prev.dtype == np.int32, name
        assert last.shape == (k, depth + 1) and last.dtype == np.uint8, name
        wprev, wlast = brute(pages, [int(x) for x in pg])
        assert np.array_equal(prev, wprev), (pages, k, name)
        assert np.array_equal(last, wlast), (pages, k, name)


def _layers(pages):
    """padded layer sizes, leaves first (merkle_nodes()'s recurrence)"""
    n = 1 if pages <= 1 else pages + pages % 2
    out = [n]
    while n > 1:
        n = 1 if n == 2 else (n // 2 + 1) & ~1
        out.append(n)
    assert sum(out) == O.merkle_nodes(pages)
    return out


@pytest.mark.parametrize("pages", [3, 5, 13])
def test_padding_sibling_is_never_a_prev(pages):
    """only the last page of an odd count: its sibling is a zero-digest padding
    node in layer 0 (and wherever the path stays the last real node of an odd
    layer), which no op can have written"""
    k = 6
    pg = np.full(k, pages - 1)
    prev, last = LA.memtree_plan(pages, pg)
    assert (prev == -1).all()
    assert (last[:-1] == 0).all() and (last[-1] == 1).all()
    # with the other pages mixed in, a prev under a padding sibling stays -1
    rng = np.random.default_rng(pages)
    pg = rng.integers(0, pages, 40)
    pg[::3] = pages - 1
    prev, _ = LA.memtree_plan(pages, pg)
    real = pages
    for l in range(LA.merkle_depth(pages)):
        for j, p in enumerate(pg):
            if ((int(p) >> l) ^ 1) >= real:
                assert prev[j, l] == -1, (pages, j, l)
        real = (real + 1) // 2


def test_plan_rejects_bad_arguments():
    with pytest.raises(LA.LfError):
        LA.memtree_plan(5, [0, 5])
    with pytest.raises(LA.LfError):
        LA.memtree_plan(0, [])
