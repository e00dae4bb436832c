"""The Ajtai matrix as a function of a seed, on the host (needs no GPU):
lf_ajtai_seeded_expand against a model written here from include/lf.h's wording --
the Poseidon2 kind's states built with numpy and permuted by the oracle, the SplitMix
kind's words taken from the oracle's fill_uniform -- window consistency, and the
refusals."""
import ctypes as C

import numpy as np
import pytest

import latticeum_amd as LA
import oracle as O
from latticeum_amd import _lib

P = LA.P
TAG = 0x4C46414A54414931
KAPPA, NTOT = 3, 7
DEGREES = [24, 16, 64, 1024]
SEED_P2 = [0x0123456789ABCDEF, P - 1, 0, 77]
SEED_SM = 4242
LF_ERR_INVALID_ARG, LF_ERR_UNSUPPORTED_RING = 1, 2  # lf.h


def model_poseidon2(seed, kappa, ncols_total, d):
    """A[row][col][8 j + i] = permute(seed[0..3], TAG, d, row, col, j, 0 x 7)[i], i < 8"""
    nb = d // 8
    st = np.zeros((kappa, ncols_total, nb, 16), np.uint64)
    st[..., 0:4] = np.array(seed, np.uint64)
    st[..., 4] = TAG
    st[..., 5] = d
    st[..., 6] = np.arange(kappa, dtype=np.uint64)[:, None, None]
    st[..., 7] = np.arange(ncols_total, dtype=np.uint64)[None, :, None]
    st[..., 8] = np.arange(nb, dtype=np.uint64)[None, None, :]
    out = O.p2_permute(np.ascontiguousarray(st.reshape(-1, 16)))
    return np.asarray(out, np.uint64).reshape(kappa, ncols_total, nb, 16)[..., :8].reshape(kappa, ncols_total, d)


def model_splitmix(seed, kappa, ncols_total, d):
    return O.fill_uniform(kappa * ncols_total * d, seed).reshape(kappa, ncols_total, d)


MODELS = {LA.AJTAI_SEED_POSEIDON2: (SEED_P2, model_poseidon2), LA.AJTAI_SEED_SPLITMIX: (SEED_SM, model_splitmix)}


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("lf_ajtai_create_seeded", "lf_ajtai_seeded_expand", "lf_dev_ajtai_seeded_expand",
                 "lf_ajtai_device_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


@pytest.mark.parametrize("kind", sorted(MODELS))
@pytest.mark.parametrize("d", DEGREES)
def test_expand_matches_model(kind, d):
    """every row, the full window, and the windows from col0 = 0, 3, 6"""
    seed, model = MODELS[kind]
    want = model(seed, KAPPA, NTOT, d)
    assert (want < np.uint64(P)).all()
    full = LA.ajtai_seeded_expand(seed, kind, kappa=KAPPA, ncols_total=NTOT, d=d)
    assert full.shape == (KAPPA, NTOT, d) and np.array_equal(full, want)
    for row in range(KAPPA):
        for col0 in (0, 3, 6):
            for ncols in {1, NTOT - col0}:
                got = LA.ajtai_seeded_expand(seed, kind, kappa=KAPPA, ncols_total=NTOT, d=d, row=row, col0=col0,
                                             ncols=ncols)
                assert np.array_equal(got, want[row, col0:col0 + ncols]), (row, col0, ncols)


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_window_is_a_slice_of_the_full_expansion(kind):
    seed, _ = MODELS[kind]
    d, kappa, ntot = 64, 4, 11
    full = LA.ajtai_seeded_expand(seed, kind, kappa=kappa, ncols_total=ntot, d=d)
    for col0, ncols in ((0, 11), (2, 5), (10, 1), (5, 6)):
        win = LA.ajtai_seeded_expand(seed, kind, kappa=kappa, ncols_total=ntot, d=d, col0=col0, ncols=ncols)
        assert np.array_equal(win, full[:, col0:col0 + ncols])


def test_kinds_and_seeds_differ():
    a = LA.ajtai_seeded_expand([1, 2, 3, 4], kappa=2, ncols_total=3, d=16)
    b = LA.ajtai_seeded_expand([1, 2, 3, 5], kappa=2, ncols_total=3, d=16)
    c = LA.ajtai_seeded_expand(1, LA.AJTAI_SEED_SPLITMIX, kappa=2, ncols_total=3, d=16)
    assert not np.array_equal(a, b) and not np.array_equal(a[..., :8], c[..., :8])
    # the degree is part of the Poseidon2 state: a d = 16 element is no prefix of a d = 32 one
    e = LA.ajtai_seeded_expand([1, 2, 3, 4], kappa=2, ncols_total=3, d=32)
    assert not np.array_equal(a, e[..., :16])


def expand_rc(seed, kind, kappa, ncols_total, d, row, col0, ncols):
    s = np.array(seed, np.uint64)
    out = np.zeros(max(ncols, 1) * max(d, 1), np.uint64)
    return _lib.load().lf_ajtai_seeded_expand(s.ctypes.data_as(C.c_void_p), kind, kappa, ncols_total, d, row, col0,
                                              ncols, out.ctypes.data_as(C.c_void_p))


def test_refusals():
    P2, SM = LA.AJTAI_SEED_POSEIDON2, LA.AJTAI_SEED_SPLITMIX
    assert expand_rc([1, 2, 3, 4], P2, 3, 7, 16, 0, 0, 7) == 0
    assert expand_rc([5, 0, 0, 0], SM, 3, 7, 16, 0, 0, 7) == 0
    for i in range(4):  # a seed word equal to p
        seed = [1, 2, 3, 4]
        seed[i] = P
        assert expand_rc(seed, P2, 3, 7, 16, 0, 0, 7) == LF_ERR_INVALID_ARG
    assert expand_rc([5, 1, 0, 0], SM, 3, 7, 16, 0, 0, 7) == LF_ERR_INVALID_ARG
    assert expand_rc([5, 0, 0, 9], SM, 3, 7, 16, 0, 0, 7) == LF_ERR_INVALID_ARG
    assert expand_rc([1, 2, 3, 4], P2, 3, 7, 16, 0, 3, 5) == LF_ERR_INVALID_ARG  # col0 + ncols > ncols_total
    assert expand_rc([1, 2, 3, 4], P2, 3, 7, 16, 0, 8, 1) == LF_ERR_INVALID_ARG
    assert expand_rc([1, 2, 3, 4], P2, 3, 7, 48, 0, 0, 7) == LF_ERR_UNSUPPORTED_RING
    assert expand_rc([5, 0, 0, 0], SM, 3, 7, 48, 0, 0, 7) == LF_ERR_UNSUPPORTED_RING
    for kind in (0, 3, -1):  # an unknown kind
        assert expand_rc([1, 0, 0, 0], kind, 3, 7, 16, 0, 0, 7) == LF_ERR_INVALID_ARG
    assert expand_rc([1, 2, 3, 4], P2, 3, 7, 16, 3, 0, 7) == LF_ERR_INVALID_ARG  # a row past kappa
    assert expand_rc([1, 2, 3, 4], P2, 3, 7, 16, 0, 0, 0) == LF_ERR_INVALID_ARG  # zero sizes
    assert expand_rc([1, 2, 3, 4], P2, 0, 7, 16, 0, 0, 7) == LF_ERR_INVALID_ARG
    assert expand_rc([1, 2, 3, 4], P2, (1 << 32) + 1, 7, 16, 0, 0, 7) == LF_ERR_INVALID_ARG  # kappa > 2^32
    # a matrix whose bytes do not fit 64 bits, either kind (2^32 x 2^32 x 16 x 8 = 2^71; 2^31 x 2^31 x 4096 x 8 = 2^77)
    assert expand_rc([1, 2, 3, 4], P2, 1 << 32, 1 << 32, 16, 0, 0, 1) == LF_ERR_INVALID_ARG
    assert expand_rc([5, 0, 0, 0], SM, 1 << 31, 1 << 31, 4096, 0, 0, 1) == LF_ERR_INVALID_ARG
    assert expand_rc([1, 2, 3, 4], P2, 1 << 29, 1 << 29, 16, 0, 0, 1) == LF_ERR_INVALID_ARG  # 2^65 bytes
    assert expand_rc([1, 2, 3, 4], P2, 1 << 28, 1 << 28, 16, (1 << 28) - 1, (1 << 28) - 1, 1) == 0  # 2^63 bytes
    with pytest.raises(LA.LfError) as e:
        LA.ajtai_seeded_expand([P, 0, 0, 0], kappa=1, ncols_total=1, d=16)
    assert e.value.code == LF_ERR_INVALID_ARG
    with pytest.raises(ValueError):  # col0 past ncols_total: no negative count reaches the C call
        LA.ajtai_seeded_expand([1, 2, 3, 4], kappa=2, ncols_total=3, d=16, col0=5)
