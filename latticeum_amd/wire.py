"""The wire format of the accumulator and the folding proof (include/lf.h
lf_lcccs_* / lf_lfproof_*): ark-serialize 0.5 CanonicalSerialize of
the reference's types (latticefold/src/nifs.rs:28-34, arith.rs:192-206).
Host-side byte layouts; numpy uint64 ring elements of d words each."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (LfCcsDesc, LfDecompositionProof, LfLcccs, LfLfproof, LfLfproofMut, LfParams, LfRingSlice,
                   LfWitness, load)

REPR_CANONICAL, REPR_MONTGOMERY = 0, 1


class LfError(RuntimeError):
    """.code: the lf.h status where a C call failed (7 = LF_ERR_INCORRECT_LENGTH), else None"""

    def __init__(self, msg: str, code: int | None = None):
        super().__init__(msg)
        self.code = code


def _slice(a, d, keep):
    a = np.ascontiguousarray(np.asarray(a, np.uint64)).ravel()
    keep.append(a)
    return LfRingSlice(a.ctypes.data_as(C.c_void_p) if a.size else None, a.size // d)


def _slices(vs, d, keep):
    arr = (LfRingSlice * max(1, len(vs)))(*[_slice(v, d, keep) for v in vs])
    keep.append(arr)
    return C.cast(arr, C.c_void_p), len(vs)


def _run(fn, *args):
    n = C.c_size_t()
    rc = fn(*args, None, 0, C.byref(n))
    if rc not in (0, 7):
        raise LfError(f"serialize rc={rc}")
    buf = (C.c_uint8 * max(1, n.value))()
    rc = fn(*args, buf, n.value, C.byref(n))
    if rc:
        raise LfError(f"serialize rc={rc}")
    return bytes(buf)[:n.value]


def serialize_lcccs(d, r, v, cm, u, x_w, h, repr=REPR_CANONICAL) -> bytes:
    keep = []
    acc = LfLcccs(d, _slice(r, d, keep), _slice(v, d, keep), _slice(cm, d, keep), _slice(u, d, keep),
                  _slice(x_w, d, keep), None)
    hh = np.ascontiguousarray(np.asarray(h, np.uint64))
    acc.h = hh.ctypes.data_as(C.c_void_p)
    return _run(load().lf_lcccs_serialize, C.byref(acc), repr)


def deserialize_lcccs(data: bytes, d: int, repr=REPR_CANONICAL) -> dict:
    raw = np.frombuffer(bytes(data), np.uint8).copy()
    buf = np.zeros(max(1, raw.size // 8 + d), np.uint64)
    out = LfLcccs()
    rc = load().lf_lcccs_deserialize(raw.ctypes.data_as(C.c_void_p), raw.size, d, repr,
                                     buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(out))
    if rc:
        raise LfError(f"deserialize rc={rc}", rc)
    base = buf.ctypes.data

    def take(s):
        off = (s.elems - base) // 8 if s.elems else 0
        return buf[off:off + s.n * d].copy()
    res = {k: take(getattr(out, k)) for k in ("r", "v", "cm", "u", "x_w")}
    off = (out.h - base) // 8
    res["h"] = buf[off:off + d].copy()
    return res


def serialize_lfproof(d, lin_sumcheck, lin_rounds, lin_evals, lin_v, lin_u, dec, fold_sumcheck, fold_rounds,
                      fold_evals, theta_s, eta_s, repr=REPR_CANONICAL) -> bytes:
    """dec: two dicts with u_s, v_s, x_s, y_s (lists of ring-element arrays)"""
    keep = []
    p = LfLfproof()
    p.d = d
    ls = np.ascontiguousarray(np.asarray(lin_sumcheck, np.uint64))
    fs = np.ascontiguousarray(np.asarray(fold_sumcheck, np.uint64))
    keep += [ls, fs]
    p.lin_sumcheck, p.lin_rounds, p.lin_evals = ls.ctypes.data_as(C.c_void_p), lin_rounds, lin_evals
    p.lin_v, p.lin_u = _slice(lin_v, d, keep), _slice(lin_u, d, keep)
    for s in range(2):
        dp = LfDecompositionProof()
        dp.u_s, dp.n_u = _slices(dec[s]["u_s"], d, keep)
        dp.v_s, dp.n_v = _slices(dec[s]["v_s"], d, keep)
        dp.x_s, dp.n_x = _slices(dec[s]["x_s"], d, keep)
        dp.y_s, dp.n_y = _slices(dec[s]["y_s"], d, keep)
        p.dec[s] = dp
    p.fold_sumcheck, p.fold_rounds, p.fold_evals = fs.ctypes.data_as(C.c_void_p), fold_rounds, fold_evals
    p.theta_s, p.n_theta = _slices(theta_s, d, keep)
    p.eta_s, p.n_eta = _slices(eta_s, d, keep)
    return _run(load().lf_lfproof_serialize, C.byref(p), repr)


PROOF_FIELDS = ("lin_sumcheck", "lin_v", "lin_u", "u_s", "v_s", "x_s", "y_s", "fold_sumcheck", "theta_s", "eta_s")


def deserialize_lfproof(data: bytes, params: LfParams, t: int, m: int, l: int, degree: int, q: int, kappa: int,
                        repr=REPR_CANONICAL) -> dict:
    """lf_lfproof_deserialize: the bytes of an LFProof of the shape (params, t, m, l, degree,
    kappa) fix, as the proof dict fold_verify takes (the flat buffers of lf_lfproof_mut; u_s,
    v_s, x_s, y_s as [left, right]). Every length in the bytes must be the shape's: LfError
    (code 7) otherwise, and for truncated bytes, trailing bytes and a word >= p."""
    lib = load()
    desc = LfCcsDesc(t, m, l, degree, q, None, None, None)
    counts = (C.c_size_t * 14)()
    total = lib.lf_lfproof_shape(C.byref(desc), C.byref(params), kappa, C.byref(counts))
    if not total:
        raise LfError("lf_lfproof_shape: not a proof shape", 1)
    d = params.d
    raw = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    buf = np.zeros(total * d, np.uint64)
    out = LfLfproofMut()
    rc = lib.lf_lfproof_deserialize(raw.ctypes.data_as(C.c_void_p), len(data), C.byref(desc), C.byref(params), kappa,
                                    repr, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(out))
    if rc:
        raise LfError(f"deserialize rc={rc}", rc)
    base, n = buf.ctypes.data, iter(counts)

    def take(ptr):
        off = (ptr - base) // 8
        return buf[off:off + next(n) * d].copy()
    res = {}
    for k in PROOF_FIELDS:  # the struct's order, which is the order of counts
        v = getattr(out, k)
        res[k] = take(v) if k not in ("u_s", "v_s", "x_s", "y_s") else [take(v[0]), take(v[1])]
    return res


# ---------------------------------------------------------------- the witness (lf.h "witness wire format")
def _dev(t) -> int:
    return t if isinstance(t, int) else t.data_ptr()


def _lf_witness(w: dict) -> LfWitness:
    return LfWitness(_dev(w["w_ccs"]), _dev(w["f"]), _dev(w["f_coeff"]))


def _ctx_error(ctx, what: str, rc: int) -> LfError:
    msg = ctx.lib.lf_ctx_last_error(ctx.h).decode()
    return LfError(f"{what} rc={rc}" + (f": {msg}" if msg else ""), rc)


def witness_wire_header(data: bytes) -> dict:
    """lf_witness_wire_header: {d, L, bits, N} of a witness's wire bytes after every format
    check (host only); LfError with the status in .code otherwise"""
    raw = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    d, L, bits, N = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = load().lf_witness_wire_header(raw.ctypes.data_as(C.c_void_p), len(data), C.byref(d), C.byref(L),
                                       C.byref(bits), C.byref(N))
    if rc:
        raise LfError(f"witness header rc={rc}", rc)
    return {"d": d.value, "L": L.value, "bits": bits.value, "N": N.value}


def serialize_witness(ctx, params: LfParams, witness: dict, N: int, bits: int = 0) -> bytes:
    """the wire bytes of a device witness {w_ccs, f, f_coeff} (only f_coeff is read);
    bits = 0: the narrowest of 16, 32, 64 that holds every coefficient"""
    lib, w = load(), _lf_witness(witness)
    n = C.c_size_t()
    rc = lib.lf_witness_serialize(ctx.h, C.byref(params), C.byref(w), N, bits, None, 0, C.byref(n))
    if rc != 7:
        raise _ctx_error(ctx, "witness serialize", rc)
    buf = np.empty(n.value, np.uint8)
    rc = lib.lf_witness_serialize(ctx.h, C.byref(params), C.byref(w), N, bits, buf.ctypes.data_as(C.c_void_p),
                                  buf.size, C.byref(n))
    if rc:
        raise _ctx_error(ctx, "witness serialize", rc)
    return buf[:n.value].tobytes()


def deserialize_witness(ctx, params: LfParams, data: bytes, witness: dict, N: int) -> None:
    """fills the device buffers {w_ccs, f, f_coeff} from a witness's wire bytes (synchronous);
    LfError with the status in .code for bytes that are malformed or of another shape"""
    raw = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    w = _lf_witness(witness)
    rc = load().lf_witness_deserialize(ctx.h, C.byref(params), raw.ctypes.data_as(C.c_void_p), len(data),
                                       C.byref(w), N)
    if rc:
        raise _ctx_error(ctx, "witness deserialize", rc)
