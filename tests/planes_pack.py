"""numpy packers for the public packed digit plane formats (lf_fold_step_bufs.planes), written
from the wording of include/lf.h alone -- the inverse of tests/planes_decode.py, and like it
independent of latticeum_amd/csrc/digitpack.hpp. Every packer returns one side's buffer as
little-endian u64 words of lf_fold_step_planes_len's length.

Two kinds of input. The formats that keep one entry per plane (d = 24, d = 4096) take any
digit array [K][N][d] with values in {-1, 0, 1}: the planes need not be the digits of one
number. The 16-bit sign|magnitude formats (d = 16 .. 512, 1024) hold a coefficient, of which
digit k is sign(x) bit_k(|x|): they take the coefficients [N][d], |x| < 2^15."""
import numpy as np

from planes_decode import digits_of  # noqa: F401  (coefficients -> their K digit planes)


def sm16(x):
    """coefficients -> 16-bit sign|magnitude words: bits 0..14 = |x|, bit 15 = x is negative"""
    x = np.asarray(x, np.int64)
    assert (np.abs(x) < (1 << 15)).all()
    return (np.abs(x) | ((x < 0).astype(np.int64) << 15)).astype(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(np.uint64).copy()


def pack_digits(digits, d):
    """digits [K][N][d] in {-1, 0, 1} -> planes, d = 24 or 4096"""
    dg = np.asarray(digits, np.int64)
    K, N, dd = dg.shape
    assert dd == d and (np.abs(dg) <= 1).all()
    if d == 24:
        # [K][N] u64, one per element and plane: bit i = coefficient i is nonzero, bit 32 + i = it is -1
        i = np.arange(24, dtype=np.uint64)
        nz = ((dg != 0).astype(np.uint64) << i).sum(axis=2, dtype=np.uint64)
        ng = ((dg < 0).astype(np.uint64) << (i + np.uint64(32))).sum(axis=2, dtype=np.uint64)
        return _u64(nz | ng)
    if d == 4096:
        return _pack_bytes(dg != 0, dg < 0)
    raise ValueError(d)


def _pack_bytes(nz, ng):
    """d = 4096: nz, ng [K][N][4096] booleans (the digit is nonzero / the sign bit) -> N x K KiB:
    byte ((e K + k) 32 + r) 32 + j holds the quad a = r + 32 j: bit b = the digit of coefficient
    a + 1024 b is nonzero, bit 4 + b = the sign bit of that coefficient"""
    K, N, _ = nz.shape
    by = np.zeros((N, K, 32, 32), np.uint8)  # [e][k][r][j]
    for b in range(4):
        q = lambda m: m[:, :, 1024 * b:1024 * (b + 1)].reshape(K, N, 32, 32).transpose(1, 0, 3, 2)  # a = 32 j + r
        by |= (q(nz).astype(np.uint8) << b) | (q(ng).astype(np.uint8) << (4 + b))
    return _u64(by)


def pack_coeffs(x, d, K):
    """coefficients [N][d], |x| < 2^15 -> planes of their balanced base-2 digits at any public
    format. d = 24 and 4096 keep the planes k < K; the sign|magnitude words keep the whole
    magnitude, of which a reader with K planes sees bits 0 .. K - 1"""
    x = np.asarray(x, np.int64)
    N, dd = x.shape
    assert dd == d
    if d == 24:
        return pack_digits(digits_of(x, K), 24)
    if d == 4096:
        # the sign bit is the coefficient's: set on every plane, also where the digit is zero
        return _pack_bytes(digits_of(x, K) != 0, np.broadcast_to((x < 0)[None], (K, N, d)))
    w = sm16(x)
    if d == 1024:
        # 512 u32 per element: word 32 q + r (q < 16, r < 32) holds coefficient r + 64 q in its
        # low half and coefficient r + 64 q + 32 in its high half
        c = w.reshape(N, 16, 2, 32)  # [e][q][half][r]
        return _u64(c[:, :, 0, :] | (c[:, :, 1, :] << 16))
    if 16 <= d <= 512 and d & (d - 1) == 0:
        # d / 2 u32 per element: word j holds coefficient j (low half) and j + d / 2 (high half)
        return _u64(w[:, :d // 2] | (w[:, d // 2:] << 16))
    raise ValueError(d)
