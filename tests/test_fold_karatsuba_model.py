"""The Karatsuba split of the d = 1024 coefficient-form fold (fold_coeff.hip), as a numpy
model: one and two levels, with the negacyclic signs, give the integers of the dense
definition tests/fold_rho_edges.py states, f0_coeff[e][c] = sum_i sum_j R_i[c][j] D_i[j][e],
on that module's cases; and the range predicate that picks the level on the device accepts
and rejects what the split's algebra says it must."""
import functools

import numpy as np
import pytest

import fold_karatsuba as KM
import fold_rho_edges as E

d, W = 1024, 2
CASES = [("mid",), ("extreme",), ("worst", 0, 511), ("top", 1)]
NW = 2 * E.params(d).K


@functools.lru_cache(maxsize=None)
def dense(case_id):
    """(case, planes, the dense product [N][d]), once per case"""
    case = E.build(case_id[0], d, W, *case_id[1:])
    Dp, _ = E.planes(case, d)
    f0 = KM.fold(case["rc"], Dp, 0)
    f0.setflags(write=False)
    return case, Dp, f0


@pytest.mark.parametrize("case_id", CASES, ids=lambda c: c[0])
def test_dense_model_is_the_stated_definition(case_id):
    """the model's level 0 against fold_rho_edges.toeplitz_row, at the block corners of both levels"""
    case, Dp, f0 = dense(case_id)
    for e in (0, Dp.shape[2] - 1):
        for c in (0, 255, 256, 511, 512, 767, 768, 1023):
            assert int(f0[e, c]) == E.toeplitz_row(case, Dp, e, c), (e, c)


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("case_id", CASES, ids=lambda c: c[0])
def test_split_gives_the_dense_integers(case_id, level):
    case, Dp, f0 = dense(case_id)
    assert np.array_equal(KM.fold(case["rc"], Dp, level), f0)


def test_table_counts_and_sizes():
    g = KM.generator(np.arange(d, dtype=np.int64))
    assert [len(KM.tables(g, l)) for l in (0, 1, 2)] == [1, 3, 9]
    assert {len(t) for t in KM.tables(g, 1)} == {1023} and {len(t) for t in KM.tables(g, 2)} == {511}


def test_entries_combine_two_and_four_generator_values():
    """a level-1 entry is at most two coefficients of rho, a level-2 entry at most four: the
    bounds 2 * 63 <= 127 and 4 * 31 <= 127 the ranges below rest on"""
    for level, n in ((1, 2), (2, 4)):
        assert max(int(np.abs(M).sum(1).max()) for M in KM.entry_maps(level)) == n


def test_level_1_holds_up_to_63():
    for seed in range(3):
        assert KM.fits(KM.short_rho(NW, 100 + seed, -63, 63), 1)
    assert KM.fits(np.full((1, d), 63, np.int64), 1) and KM.fits(np.full((1, d), -63, np.int64), 1)
    signs = np.random.default_rng(5).integers(0, 2, size=(4, d), dtype=np.int64) * 2 - 1
    assert KM.fits(63 * signs, 1)


def test_level_2_holds_up_to_31():
    for seed in range(3):
        assert KM.fits(KM.short_rho(NW, 200 + seed, -31, 31), 2)
    assert KM.fits(np.full((1, d), 31, np.int64), 2) and KM.fits(np.full((1, d), -31, np.int64), 2)
    signs = np.random.default_rng(6).integers(0, 2, size=(4, d), dtype=np.int64) * 2 - 1
    assert KM.fits(31 * signs, 2)


def test_no_level_2_entry_takes_four_coefficients_with_one_sign():
    """so four -32 cannot line up to +128: with the identities as fold_coeff.hip states them the
    signs of a four-coefficient entry are three and one or two and two"""
    pats = set()
    for M in KM.entry_maps(2):
        four = M[(M != 0).sum(1) == 4]
        pats |= {int(x) for x in (four < 0).sum(1)}
    assert pats == {1, 2, 3}
    assert KM.fits(np.full((1, d), -32, np.int64), 2)


def test_level_2_edge_of_the_short_range():
    """three -32 the entry negates and the fourth at +31: 127, level 2 holds over all of
    short_challenge's range; the fourth at +32 (one past it): +128, level 2 is out, level 1 in"""
    t, row, places, signs = KM.widest_entry(2)
    assert len(places) == 4 and (signs < 0).sum() == 3
    rc = KM.level2_entry_at(NW, 300, 31)
    assert rc.min() == -32 and rc.max() == 31
    assert int(KM.tables(KM.generator(rc[7]), 2)[t][row]) == 127
    assert KM.fits(rc, 2) and KM.best_level(rc, 2) == 2
    rc = KM.level2_entry_at(NW, 300, 32)
    assert int(KM.tables(KM.generator(rc[7]), 2)[t][row]) == 128
    assert not KM.fits(rc, 2) and KM.fits(rc, 1)
    assert KM.best_level(rc, 2) == 1 and KM.best_level(rc, 1) == 1


def test_level_1_entry_at_128_is_rejected():
    t, row, places, signs = KM.widest_entry(1)
    rc = KM.level1_entry_128(NW, 400)
    assert np.abs(rc).max() == 64 <= E.BOUND[d]
    assert int(KM.tables(KM.generator(rc[22]), 1)[t][row]) == 128
    assert not KM.fits(rc, 1) and KM.best_level(rc, 2) == 0


def test_rho_at_127_is_rejected_at_level_1():
    for kind in ("mid", "extreme"):
        rc = E.build(kind, d, W)["rc"]
        assert np.abs(rc).max() == 127
        assert not KM.fits(rc, 1) and KM.best_level(rc, 2) == 0
    one = np.zeros((1, d), np.int64)
    one[0, 3], one[0, 3 + 512] = 127, 127  # T1 + T2 at delta = 3: 254
    assert not KM.fits(one, 1)
    one[0, 3 + 512] = -127                 # T2 - T1 at delta = 3: -254
    assert not KM.fits(one, 1)


def test_digit_sums_stay_in_range():
    """the B operands: a sum of two ternary blocks is in [-2, 2], of four in [-4, 4]"""
    case, Dp, _ = dense(("extreme",))
    V = Dp[0, 0].T.astype(np.int64)
    s1 = V[:512] + V[512:]
    s2 = s1[:256] + s1[256:]
    assert np.abs(s1).max() <= 2 and np.abs(s2).max() <= 4
