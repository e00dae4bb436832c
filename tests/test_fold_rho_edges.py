"""The cases of tests/fold_rho_edges.py have the properties they are about, from the oracle
and Python integers alone (no GPU): the witnesses round-trip to the intended digits, plane
K - 1 is live where meant, the worst-case target is 2 * 14 * d * bound (3 641 344 at
d = 1024; 21 504 at index 23 of the degree-46 product at d = 24), and every
one-coefficient-out rho has exactly that one coefficient outside the accepted range.
tests/test_gpu_fold_rho_edges.py runs the same cases on the device."""
import numpy as np
import pytest

import fold_rho_edges as E
import oracle as O
from planes_decode import digits_of

P = E.P


def ntt_planes(case, new_fc, d):
    pr = E.params(d)
    return [O.decompose_witness(x, d, pr.B, pr.L, pr.b_small, pr.K)[1] for x in (case["acc_fc"], new_fc)]


def check_digits(case, D, new_fc, d):
    """both sides decompose to sign(x) bit_k(|x|) of the digits the case was built from"""
    pr = E.params(d)
    acc, new = case["digits"]
    N = new_fc.size // d
    assert np.array_equal(D[0], digits_of(acc.reshape(N, d), pr.K))
    if new is not None:
        assert np.array_equal(E.signed(new_fc), new.ravel())
        assert np.array_equal(D[1], digits_of(new.reshape(N, d), pr.K))


def test_bounds():
    assert E.worst_sum(1024) == 3_641_344 < 1 << 31
    assert 1 << 14 < E.worst_sum(24) == 21_504 < 1 << 15


@pytest.mark.parametrize("d", [1024, 24])
def test_rho_coefficients_are_stored_as_signed_representatives(d):
    """rho reaches the step in NTT form; its coefficients are the residues p - |x| of the
    negative ones: p - bound is accepted, p - (bound + 1) refused"""
    b, last = E.BOUND[d], d - 1
    rc = E.one_out_rho(d, 1, 0, last, -1)
    back = O.icrt(E.rho_ntt(rc, d), d).reshape(rc.shape)
    assert np.array_equal(back, E.to_field(rc))
    assert int(back[0, last]) == P - (b + 1)
    assert (back == np.uint64(P - b)).any(axis=1).all() and (back == np.uint64(b)).any(axis=1).all()


@pytest.mark.parametrize("d", [1024, 24])
def test_mid_and_extreme_rho_ranges(d):
    b = E.BOUND[d]
    mid = E.mid_rho(d, 2)
    assert mid.min() == -b and mid.max() == b and not E.outside(mid, d)
    assert ((mid == -b).any(axis=1) & (mid == b).any(axis=1)).all()  # both endpoints in every rho_i
    assert len(np.unique(mid)) == 2 * b + 1                          # and the whole range between
    ext = E.extreme_rho(d, 3)
    assert (np.abs(ext) == b).all() and ((ext == -b).any(axis=1) & (ext == b).any(axis=1)).all()


@pytest.mark.parametrize("d,cases", [(1024, E.OUT_1024), (24, E.OUT_24)])
def test_one_coefficient_out(d, cases):
    b = E.BOUND[d]
    assert {i for i, _, _ in cases} >= {0, 29} and {c for _, c, _ in cases} == {0, d - 1}
    assert {s for _, _, s in cases} == {-1, 1}
    for i, c, sign in cases:
        case = E.build("out", d, 2 if d == 1024 else 3, i, c, sign)
        assert E.outside(case["rc"], d) == [(i, c)] == [case["out"]]
        assert case["rc"][i, c] == sign * (b + 1)
        assert np.array_equal(O.icrt(case["rho"], d).reshape(-1, d), E.to_field(case["rc"]))


@pytest.mark.parametrize("c_star", [0, 511, 1023])
def test_worst_case_1024(c_star):
    d, W = 1024, 2
    case = E.build("worst", d, W, 0, c_star)
    e, c = case["target"]
    assert (e, c) == (1, c_star) and not E.outside(case["rc"], d)
    assert (np.abs(case["rc"]) == E.BOUND[d]).all()
    D, new_fc = E.planes(case, d)
    check_digits(case, D, new_fc, d)
    # 14 live planes of one sign on the target element, plane K - 1 dead: |x| = 2^14 - 1
    assert (np.abs(D[:, :14, e]) == 1).all() and not D[:, 14].any()
    assert E.toeplitz_row(case, D, e, c) == E.worst_sum(d)
    f0c = E.oracle_f0_coeff(case, ntt_planes(case, new_fc, d), d)
    assert f0c[e, c] == E.worst_sum(d) == np.abs(f0c).max()
    # the other rows of that element, by the same rule
    for cc in (0, 1, 510, 1022, 1023):
        assert f0c[e, cc] == E.toeplitz_row(case, D, e, cc)


def test_worst_case_24():
    d, W = 24, 3
    case = E.build("worst", d, W, W - 1, 23)
    e, c = case["target"]
    assert (e, c) == ((W - 1) * 5 + 1, 23) and not E.outside(case["rc"], d)
    D, new_fc = E.planes(case, d)
    check_digits(case, D, new_fc, d)
    assert (np.abs(D[:, :14, e]) == 1).all() and not D[:, 14].any()
    pre = E.conv_sum(case, D, e)
    assert pre[23] == E.worst_sum(d) == max(abs(x) for x in pre)
    f0c = E.oracle_f0_coeff(case, ntt_planes(case, new_fc, d), d)
    assert [int(x) for x in f0c[e]] == E.reduce_phi72(pre)
    for ee in range(W * 5):  # every element's sums before the reduction fit the 16-bit lanes
        assert max(abs(x) for x in E.conv_sum(case, D, ee)) <= E.worst_sum(d)


@pytest.mark.parametrize("d,W", [(1024, 2), (24, 3)])
def test_extreme_case_reaches_plane_k_minus_1(d, W):
    case = E.build("extreme", d, W)
    D, new_fc = E.planes(case, d)
    check_digits(case, D, new_fc, d)
    K = E.params(d).K
    for s in range(2):  # digits +2^14 and -2^14 on both sides
        assert (D[s, K - 1] == 1).any() and (D[s, K - 1] == -1).any()
    assert not E.outside(case["rc"], d)


def test_top_limb_case():
    d, W, g = 1024, 2, 1
    case = E.build("top", d, W, g)
    pr = E.params(d)
    D, new_fc = E.planes(case, d)
    check_digits(case, D, new_fc, d)
    top = D.reshape(2, pr.K, W, pr.L, d)[:, :, :, pr.L - 1]  # [side][k][group]
    live = np.abs(top).any(axis=3)
    assert live[0, 4:14, g].all() and not live[0, 4:, 1 - g].any() and not live[1, 4:].any()
    assert not live[:, 14].any() and not E.outside(case["rc"], d)
