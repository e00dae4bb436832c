"""An independent decoder of the packed digit planes (lf_fold_step_bufs.planes), written
from the wording of include/lf.h alone -- not from latticeum_amd/csrc/digitpack.hpp, which
it is there to check (tests/test_digit_pack.py on the CPU, tests/test_gpu_commit_planes.py
on the device)."""
import numpy as np


def planes_u64(d, K, N):
    """u64 words of one side's planes"""
    return K * N if d == 24 else N * 256 if d == 1024 else N * K * 128


def decode_planes(buf, d, K, N):
    """planes of N elements (any integer dtype, little-endian bytes) -> digits [K][N][d] in {-1, 0, 1}"""
    raw = np.ascontiguousarray(buf).view(np.uint8)
    if d == 24:
        # [K][N] u64, one per element and plane: bit i = coefficient i is nonzero, bit 32 + i = it is -1
        p = raw.view(np.uint64).reshape(K, N, 1)
        i = np.arange(24, dtype=np.uint64)
        nz = ((p >> i) & np.uint64(1)).astype(np.int8)
        ng = ((p >> (i + np.uint64(32))) & np.uint64(1)).astype(np.int8)
        return nz * (1 - 2 * ng)
    if d == 1024:
        # N x 2 KiB = 512 u32 per element; word 32 q + r (q < 16, r < 32) holds coefficient
        # r + 64 q in its low half and r + 64 q + 32 in its high half, each as a 16-bit
        # sign|magnitude word: bits 0..14 = |x|, bit 15 = x < 0. Digit k = sign(x) bit_k(|x|)
        w = raw.view(np.uint32).reshape(N, 16, 1, 32)
        halves = np.concatenate([w & 0xFFFF, w >> 16], axis=2)  # [e][q][half][r]: coefficient 64 q + 32 half + r
        c = halves.reshape(N, 1024).astype(np.int32)
        sign = 1 - 2 * ((c >> 15) & 1)
        k = np.arange(K).reshape(K, 1, 1)
        return ((((c & 0x7FFF)[None] >> k) & 1) * sign[None]).astype(np.int8)
    if d == 4096:
        # N x K KiB: byte ((e K + k) 32 + r) 32 + j holds the quad a = r + 32 j: bit b = the digit of
        # coefficient a + 1024 b is nonzero, bit 4 + b = that coefficient is negative
        by = raw.reshape(N, K, 32, 32)  # [e][k][r][j]
        out = np.zeros((K, N, 4096), np.int8)
        for b in range(4):
            dg = ((by >> b) & 1).astype(np.int8) * (1 - 2 * ((by >> (4 + b)) & 1).astype(np.int8))
            out[:, :, 1024 * b:1024 * (b + 1)] = dg.transpose(1, 0, 3, 2).reshape(K, N, 1024)  # [k][e][j][r]: a = 32 j + r
        return out
    raise ValueError(d)


def digits_of(x, K):
    """signed coefficients (any shape) -> their K balanced base-2 digit planes [K][...]: sign(x) bit_k(|x|)"""
    x = np.asarray(x, np.int64)
    k = np.arange(K).reshape((K,) + (1,) * x.ndim)
    return (((np.abs(x)[None] >> k) & 1) * np.sign(x)[None]).astype(np.int8)
