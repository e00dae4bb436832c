"""The f_hat-from-planes entries and the lean prover at the C ABI, without a GPU: the library
exports them, include/lf.h and latticeum_amd/_lib.py declare the same argument lists, and the
argument errors a call reports before it touches a device. Also the packers of
tests/planes_pack.py against the independent decoder of tests/planes_decode.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import latticeum_amd as LA
from latticeum_amd import _lib
from planes_decode import decode_planes, digits_of
from planes_pack import pack_coeffs, pack_digits

ROOT = Path(__file__).resolve().parents[1]
LF_ERR_INVALID_ARG = 1  # lf.h

NEW = ["lf_dev_fhat_evaluate_planes", "lf_dev_fhat_lincomb_planes", "lf_sumcheck_prove_fold_planes",
       "lf_prover_create_lean", "lf_prover_is_lean", "lf_prover_device_bytes"]


def header_args(name):
    """the parameter list of `name` in lf.h, one C type class per parameter"""
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include/lf.h").read_text(), flags=re.S)
    m = re.search(r"\b([a-z_ 0-9]+?)\b\s*\*?\s*" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, name
    out = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        if "*" in p:
            out.append("ptr")
        elif p.startswith("size_t"):
            out.append("size_t")
        elif p.startswith("int"):
            out.append("int")
        else:
            raise AssertionError(p)
    ret = "size_t" if "size_t" in m.group(1) else "int"
    return ret, out


def ctypes_class(t):
    if t is C.c_int:
        return "int"
    if t is C.c_size_t:
        return "size_t"
    assert t is C.c_void_p or issubclass(t, C._Pointer), t
    return "ptr"


@pytest.mark.parametrize("name", NEW)
def test_exported_and_declared_alike(name):
    lib = _lib.load()
    assert hasattr(lib, name)
    ret, args = _lib.SIGNATURES[name]
    want_ret, want_args = header_args(name)
    assert ctypes_class(ret) == want_ret
    assert [ctypes_class(a) for a in args] == want_args


def test_null_arguments_are_invalid():
    """a NULL context (or any NULL pointer, checked first) is LF_ERR_INVALID_ARG, no device touched"""
    lib = _lib.load()
    pr = LA.goldilocks_dp(24)
    assert lib.lf_dev_fhat_evaluate_planes(None, C.byref(pr), None, 0, 3, None, None) == LF_ERR_INVALID_ARG
    assert lib.lf_dev_fhat_lincomb_planes(None, C.byref(pr), None, 0, 3, None, None) == LF_ERR_INVALID_ARG
    assert lib.lf_sumcheck_prove_fold_planes(None, None, None, None, C.byref(pr), None, None, 0, 3, None, None,
                                             None) == LF_ERR_INVALID_ARG
    h = C.c_void_p()
    assert lib.lf_prover_create_lean(None, None, C.byref(pr), None, C.byref(h)) == LF_ERR_INVALID_ARG
    assert not h.value
    assert lib.lf_prover_is_lean(None) == 0
    assert lib.lf_prover_device_bytes(None) == 0


def test_prover_takes_the_lean_option():
    import inspect
    assert inspect.signature(LA.Prover.__init__).parameters["lean"].default is False
    assert isinstance(LA.Prover.lean, property) and isinstance(LA.Prover.device_bytes, property)
    for name in ("dev_fhat_evaluate_planes", "dev_fhat_lincomb_planes", "sumcheck_prove_fold_planes"):
        assert callable(getattr(LA.Context, name))


@pytest.mark.parametrize("d,K,N", [(24, 15, 7), (24, 3, 1), (16, 15, 9), (64, 5, 17), (512, 15, 3), (1024, 15, 2),
                                   (4096, 15, 2), (4096, 4, 1)])
def test_packers_invert_the_decoder(d, K, N):
    rng = np.random.default_rng(d + K + N)
    x = rng.integers(-(1 << K) + 1, 1 << K, (N, d))
    buf = pack_coeffs(x, d, K)
    pr = LA.goldilocks_dp(d)
    pr.K = K
    assert buf.size == LA.fold_step_planes_len(pr, N)
    if d in (24, 1024, 4096):
        assert np.array_equal(decode_planes(buf, d, K, N), digits_of(x, K))
    else:  # d = 16 .. 512: word j = coefficient j | coefficient j + d / 2 << 16 (lf.h)
        w = buf.view(np.uint32).reshape(N, d // 2)
        sm = np.concatenate([w & 0xFFFF, w >> 16], axis=1).astype(np.int64)
        assert np.array_equal((sm & 0x7FFF) * (1 - 2 * (sm >> 15)), x)
    if d in (24, 4096):  # any digit array, plane by plane
        dg = rng.integers(-1, 2, (K, N, d))
        assert np.array_equal(decode_planes(pack_digits(dg, d), d, K, N), dg)
