"""The case table of tests/sumcheck_paths.py reaches every launch path of the sumcheck
kernels (no GPU needed: the plans come from lf_sumcheck_round_plan and lf_sumcheck_dot_plan,
which return what the launchers use). A failure names the empty cell: a changed threshold,
cap or block size moved the cases off that path, and the table needs a shape that reaches it
again."""
import numpy as np
import pytest

import latticeum_amd as LA
import sumcheck_paths as SP


@pytest.fixture(scope="module")
def reached():
    return SP.census()


@pytest.mark.parametrize("cell", SP.required())
def test_census_cell_is_reached(reached, cell):
    assert cell in reached, f"no case of tests/sumcheck_paths.py reaches the path `{cell}`"


def test_required_cells_are_known_to_the_census(reached):
    """a required cell that census() cannot produce would fail for ever; one it produces but
    nobody requires is a path somebody forgot to demand"""
    req = set(SP.required())
    extra = {c for c in reached if c not in req}
    # the cells the census also reports but that no case need reach
    optional = {c for c in extra if c.startswith("fold_digits/") or c.endswith("/c zero in all")}
    assert extra == optional, sorted(extra - optional)


def test_round_plan_entry():
    """the plan entry against hand-worked plans at the edges of its thresholds (Phi_72: 8 slots,
    32 points per block; d = 1024: 1024 slots over grid.y = 4)"""
    pl = LA.sumcheck_round_plan(24, 1 << 15, 3, LA.PLAN_FOLDING)  # 2^18 threads: not split, 1024 blocks uncapped
    assert (pl["spb"], pl["ppb"], pl["gx"], pl["gy"], pl["nchunk"], pl["capped"]) == (8, 32, 1024, 1, 1, 0)
    pl = LA.sumcheck_round_plan(24, 1 << 16, 3, LA.PLAN_FOLDING)
    assert (pl["gx"], pl["capped"]) == (1024, 1)
    pl = LA.sumcheck_round_plan(24, 1 << 14, 3, LA.PLAN_LIN)      # 2^17 threads: two chunks of three
    assert (pl["gx"], pl["nchunk"]) == (512, 2)
    pl = LA.sumcheck_round_plan(1024, 8, 5, LA.PLAN_LIN_EQ)       # 2^13 threads: the per-point kernel
    assert (pl["spb"], pl["ppb"], pl["gx"], pl["gy"], pl["nchunk"], pl["per_point"]) == (256, 1, 8, 4, 5, 1)
    assert LA.sumcheck_round_plan(1024, 16, 5, LA.PLAN_LIN_EQ)["per_point"] == 0
    assert LA.sumcheck_round_plan(1024, 8, 5, LA.PLAN_LIN)["per_point"] == 0
    assert LA.sumcheck_round_plan(24, 4, 2, LA.PLAN_LIN_EQ)["sparse_block_points"] == 8 * 32
    for bad in ((17, 4, 1, 0), (24, 0, 1, 0), (24, 4, 0, 0), (24, 4, 1, 3)):
        with pytest.raises(LA.LfError):
            LA.sumcheck_round_plan(*bad)


def test_dot_plan_entry():
    assert LA.sumcheck_dot_plan(24, 8) == dict(spb=8, ppb=32, nsplit=1, passes=1)
    assert LA.sumcheck_dot_plan(24, 4096) == dict(spb=8, ppb=32, nsplit=64, passes=2)
    assert LA.sumcheck_dot_plan(1024, 16) == dict(spb=256, ppb=1, nsplit=16, passes=1)
    with pytest.raises(LA.LfError):
        LA.sumcheck_dot_plan(24, 0)


def test_case_inputs_have_their_properties():
    """what the cases say about themselves: digit rows hold digits only, the alternating rows'
    line differences are +-2, a dead case has no active point, and the sparse lists name exactly
    the points whose every factor's line is live"""
    for case in SP.DIGIT_CASES:
        rows = SP.digit_rows(case)
        assert rows.shape == (2 * case["K"], case["N"], case["d"])
        assert np.isin(rows, np.array([0, 1, SP.P - 1], np.uint64)).all(), case["id"]
        if case["rows"].startswith("alt") and case["N"] > 1:
            s = np.where(rows == np.uint64(SP.P - 1), -1, rows.astype(np.int64))
            assert (np.abs(s[:, 1::2][:, :case["N"] // 2] - s[:, 0::2][:, :case["N"] // 2]) == 2).all()
    for case in SP.SPARSE_DEAD:
        assert not np.diff(SP.sparse_lists(case)[2].astype(np.int64)).any()
    for case in SP.LIN_EQ_WEAK:
        d, tb = case["d"], SP.tb_of(case["d"])
        c, S, mz, _ = SP.lin_inputs(case)
        o = SP.WEAK_SLOT[d] * tb
        assert S[0] == [] and S[1] == S[2] == [0, 1, 2] and int(c[o]) == SP.P - 1 and int(c[d + o]) == int(c[2 * d + o]) == 1
        row = 2 * SP.WEAK_POINT * d + o
        prod = int(mz[0][row]) * int(mz[1][row]) * int(mz[2][row])
        assert SP.P <= prod < 1 << 64                       # the chain's last product, unreduced: weak as it stands

        def add(a, b):  # gl::add on u64 words: one 2^64 == 2^32 - 1 fix, right for canonical operands
            t = (a + b) & M64
            u = (t + (1 << 32) - 1) & M64
            return u if a + b > M64 or t + (1 << 32) - 1 > M64 else t
        M64 = (1 << 64) - 1
        raw = add(add(SP.P - 1, prod), prod)                # summed uncanonicalised, the second one wraps twice
        assert raw % SP.P != (SP.P - 1 + 2 * prod) % SP.P
        assert add(add(SP.P - 1, prod % SP.P), prod % SP.P) == (SP.P - 1 + 2 * prod) % SP.P
        assert all(not int(x[row + k]) and not int(c[i * d + o + k]) for x in mz for i in range(3) for k in range(1, tb))
    case = SP.LIN_EQ_SWEEP[4]
    (S, _, zero), (live, act, off) = SP.lin_structure(case), SP.sparse_lists(case)
    for i, Si in enumerate(S):
        pts = act[off[i]:off[i + 1]]
        want = [b for b in range(1 << (case["nv"] - 1)) if all(live[j][b] for j in Si)] if zero[i] != "all" else []
        assert pts.tolist() == want
