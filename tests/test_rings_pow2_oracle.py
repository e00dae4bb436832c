"""The yardstick for the X^d + 1 rings whose degree is 2 4^k (d = 32, 128, 512, 2048):
the oracle's crt is the evaluation map slot k = f(psi^(2k+1)), psi = 7^((p-1)/2d),
icrt inverts it, and the slot product is the negacyclic product -- the same
convention as at d = 4^k, which the device is then compared with bit for bit
(tests/test_gpu_rings_pow2.py). And lf_ring_supported, the one part of the
public interface that needs no GPU."""
import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O

P = O.P
NEW = [32, 128, 512, 2048]


@pytest.mark.parametrize("d", NEW)
def test_crt_is_the_evaluation_map(d):
    f = O.fill_uniform(d, 10 + d)
    F = O.crt(f, d)
    psi = pow(7, (P - 1) // (2 * d), P)
    assert pow(psi, d, P) == P - 1  # a primitive 2d-th root: the slots are the roots of X^d + 1
    for k in (0, 1, d // 2, d - 1):
        x = pow(psi, 2 * k + 1, P)
        acc = 0
        for c in reversed(f):  # Horner
            acc = (acc * x + int(c)) % P
        assert int(F[k]) == acc, k


@pytest.mark.parametrize("d", NEW)
def test_icrt_inverts_crt(d):
    f = O.fill_uniform(3 * d, 20 + d)
    assert np.array_equal(O.icrt(O.crt(f, d), d), f)
    assert np.array_equal(O.crt(O.icrt(f, d), d), f)


@pytest.mark.parametrize("d", NEW)
def test_slot_product_is_the_negacyclic_product(d):
    a, b = O.fill_uniform(d, 30 + d), O.fill_uniform(d, 40 + d)
    assert np.array_equal(O.icrt(O.slot_mul(O.crt(a, d), O.crt(b, d), d), d), O.poly_mul(a, b, d))
    # X^(d-1) X = -1
    x1, xd = np.zeros(d, np.uint64), np.zeros(d, np.uint64)
    x1[1], xd[d - 1] = 1, 1
    minus_one = np.zeros(d, np.uint64)
    minus_one[0] = P - 1
    assert np.array_equal(O.poly_mul(xd, x1, d), minus_one)


def test_ring_supported_truth_table():
    yes = [24] + [1 << k for k in range(4, 13)]
    assert yes == [24, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    for d in yes:
        assert LA.ring_supported(d) is True, d
        assert LA.load().lf_ring_supported(d) == 1, d
    for d in (0, 8, 48, 96, 8192, -16, 1, 2, 4, 12, 25, 4095, 4097, 1 << 30, -(1 << 31)):
        assert LA.ring_supported(d) is False, d
        assert LA.load().lf_ring_supported(d) == 0, d
    assert sorted(LA.SUPPORTED_D) == sorted(yes)
