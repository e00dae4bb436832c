"""A pure-Python model of ring::stockham4 (latticeum_amd/csrc/ring.hpp): the same
pass order, the same i, k, s, j expressions and the same thread striding as the
LDS transform behind every X^d + 1 kernel, run thread by thread on Python
integers. It pins the LDS indexing before a kernel runs: in every pass each read
and write index is below D, every output index is written exactly once, and
every thread does the same number of butterflies; and the result, with the twist
the kernels apply around it, is the oracle's crt / icrt. D = 4^k runs radix-4
passes only (the code before the radix-2 pass existed); D = 2 4^k puts one
twiddle-free radix-2 pass in front."""
import numpy as np
import pytest

import oracle as O

P = O.P
SIZES = [16, 32, 64, 128, 512, 1024, 2048]


def nt(D):
    """ring.hpp NT<D>::T: threads per element"""
    return min(D // 4, 256)


def log2_odd(D):
    return (D.bit_length() - 1) % 2 == 1


def tables(D):
    """lf_api.hip get_tables: fwd twist, fwd roots, inv twist, inv roots"""
    psi = pow(7, (P - 1) // (2 * D), P)
    psi_inv = pow(psi, P - 2, P)
    w, w_inv, dinv = psi * psi % P, psi_inv * psi_inv % P, pow(D, P - 2, P)
    return ([pow(psi, j, P) for j in range(D)], [pow(w, j, P) for j in range(D)],
            [dinv * pow(psi_inv, j, P) % P for j in range(D)], [pow(w_inv, j, P) for j in range(D)])


class Lds:
    """one LDS buffer of D words that records the indices it is read and written at"""

    def __init__(self, D, vals=None):
        self.D, self.v = D, list(vals) if vals is not None else [None] * D
        self.reads, self.writes = [], []

    def __getitem__(self, i):
        assert 0 <= i < self.D, f"LDS read at {i} of {self.D}"
        self.reads.append(i)
        return self.v[i]

    def __setitem__(self, i, x):
        assert 0 <= i < self.D, f"LDS write at {i} of {self.D}"
        self.writes.append(i)
        self.v[i] = x


def stockham4(vals, D, T, roots, inv):
    """ring.hpp stockham4<D, T, INV>, every thread's loop in turn per pass (the
    passes are separated by barriers). Returns (result, [(radix, p, per-thread
    butterfly counts, written indices)])"""
    e4 = pow(2, 144 if inv else 48, P)
    x, passes = Lds(D, vals), []
    r2 = log2_odd(D)
    if r2:
        y, count = Lds(D), [0] * T
        for tid in range(T):
            for i in range(tid, D // 2, T):
                a0, a1 = x[i], x[i + D // 2]
                y[2 * i] = (a0 + a1) % P
                y[2 * i + 1] = (a0 - a1) % P
                count[tid] += 1
        passes.append((2, 1, count, y.writes))
        x = Lds(D, y.v)
    p = 2 if r2 else 1
    while p < D:
        s = D // (4 * p)
        y, count = Lds(D), [0] * T
        for tid in range(T):
            for i in range(tid, D // 4, T):
                k = i & (p - 1)
                a0, a1, a2, a3 = x[i], x[i + D // 4], x[i + D // 2], x[i + 3 * D // 4]
                if p > 1:
                    for e in (s * k, 2 * s * k, 3 * s * k):
                        assert 0 <= e < D, f"roots read at {e} of {D}"
                    a1 = a1 * roots[s * k] % P
                    a2 = a2 * roots[2 * s * k] % P
                    a3 = a3 * roots[3 * s * k] % P
                t0, t1 = (a0 + a2) % P, (a0 - a2) % P
                t2, t3 = (a1 + a3) % P, (a1 - a3) * e4 % P
                j = ((i - k) << 2) + k
                y[j] = (t0 + t2) % P
                y[j + p] = (t1 + t3) % P
                y[j + 2 * p] = (t0 - t2) % P
                y[j + 3 * p] = (t1 - t3) % P
                count[tid] += 1
        passes.append((4, p, count, y.writes))
        x = Lds(D, y.v)
        p <<= 2
    return x.v, passes


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    D = request.param
    return D, tables(D), O.fill_uniform(D, 4000 + D)


def check_passes(D, T, passes):
    want = [2] + [4] * ((D.bit_length() - 2) // 2) if log2_odd(D) else [4] * ((D.bit_length() - 1) // 2)
    assert [r for r, _, _, _ in passes] == want
    p = 1
    for r, pp, count, writes in passes:
        assert pp == p
        assert sorted(writes) == list(range(D)), "every output index exactly once"
        assert count == [D // (r * T)] * T, "the same butterfly count on every thread"
        p *= r
    assert p == D


@pytest.mark.parametrize("inv", [False, True])
def test_model_matches_oracle_and_stays_in_bounds(case, inv):
    D, (twist, roots, itwist, iroots), f = case
    T = nt(D)
    assert (D // 4) % T == 0
    assert roots[D // 4] == pow(2, 48, P) and iroots[D // 4] == pow(2, 144, P)
    if not inv:  # the kernels twist on the way into LDS
        out, passes = stockham4([int(v) * twist[j] % P for j, v in enumerate(f)], D, T, roots, False)
        want = O.crt(f, D)
    else:  # and on the way out
        out, passes = stockham4([int(v) for v in f], D, T, iroots, True)
        out = [v * itwist[j] % P for j, v in enumerate(out)]
        want = O.icrt(f, D)
    check_passes(D, T, passes)
    assert np.array_equal(np.array(out, np.uint64), want)


def test_thread_counts():
    """NT<D>::T = min(D / 4, 256): one radix-4 butterfly per thread up to D = 1024; the
    radix-2 pass has D / 2 butterflies, two per thread there and four at D = 2048"""
    for D in SIZES:
        _, passes = stockham4([0] * D, D, nt(D), tables(D)[1], False)
        per = {r: count[0] for r, _, count, _ in passes}
        assert per[4] == max(1, D // 1024)
        if log2_odd(D):
            assert per[2] == 2 * per[4]
    assert nt(2048) == 256 and nt(32) == 8 and nt(16) == 4
