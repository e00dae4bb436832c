"""The index arithmetic of lf_dev_commit_planes's from-planes front ends, restated lane by lane in
numpy against the public formats as tests/planes_pack.py packs them (from lf.h's wording, not from
latticeum_amd/csrc/digitpack.hpp), at W = 1, 16, 17, 33:

  d = 24 (k_decompose_phi72_w<28>): wave (G, pass), lane 16 kq + gi reads the u64 at
    (4 pass + kq) N + (16 G + gi) L + l, keeps bits 0..23 of its low word as the nonzero mask and
    the high word and-ed with it as the sign mask, and emits plane k as operand row s K + k;
  d = 16 .. 512 (k_decompose_pow2<D, NT, true>): thread (j, t) of unit G reads the u32 words
    t + q T, q < d / (2 T), of element (16 G + j) L + l; coefficient t + q T is the low half and
    t + q T + d / 2 the high half.

Every digit so read must be the schoolbook digit sign(x) bit_k(|x|) of the right coefficient, every
word must be read exactly once, and nothing past W is read."""
import numpy as np
import pytest

import planes_pack

K, L = 15, 5
WS = [1, 16, 17, 33]


def coeffs(N, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-(1 << 14), (1 << 14) + 1, size=(N, d), dtype=np.int64)
    x[0, 0], x[-1, -1] = 1 << 14, -(1 << 14)
    return x


def schoolbook(x, k):
    return ((np.abs(x) >> k) & 1) * np.sign(x)


@pytest.mark.parametrize("W", WS)
def test_phi72_lanes(W):
    N = W * L
    x = coeffs(N, 24, 100 + W)
    buf = planes_pack.pack_coeffs(x, 24, K)
    assert buf.size == K * N
    reads = np.zeros(buf.size, np.int64)
    nblk, npass = (W + 15) // 16, (K + 3) // 4
    lane = np.arange(64)
    kq, gi = lane >> 4, lane & 15
    i = np.arange(24, dtype=np.uint64)
    for task in range(nblk * npass):
        G, ps = divmod(task, npass)
        k, g = 4 * ps + kq, 16 * G + gi
        live = (g < W) & (k < K)
        for l in range(L):
            idx = (k * N + g * L + l)[live]
            np.add.at(reads, idx, 1)
            m = buf[idx]
            nz = (m & np.uint64(0xFFFFFFFF)) & np.uint64(0xFFFFFF)
            ng = (m >> np.uint64(32)) & nz
            dg = ((nz[:, None] >> i) & np.uint64(1)).astype(np.int64) * (1 - 2 * ((ng[:, None] >> i) & np.uint64(1)).astype(np.int64))
            want = np.stack([schoolbook(x[e], kk) for e, kk in zip((g * L + l)[live], k[live])])
            assert np.array_equal(dg, want), (task, l)
    assert (reads == 1).all()
    rows = [s * K + k for s in range(2) for k in range(K)]
    assert sorted(rows) == list(range(2 * K)) and max(rows) < 32


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("d", [16, 32, 64, 128, 256, 512])
def test_pow2_threads(d, W):
    N = W * L
    x = coeffs(N, d, 200 + d + W)
    words = planes_pack.pack_coeffs(x, d, K).view(np.uint32)
    assert words.size == N * d // 2
    T = min(d // 4, 64)
    PH = d // T // 2
    tid = np.arange(16 * T)
    j, t = tid // T, tid % T
    reads = np.zeros(words.size, np.int64)
    for G in range((W + 15) // 16):
        g = 16 * G + j
        ok = g < W
        for l in range(L):
            e = (g * L + l)[ok]
            for q in range(PH):
                c = (t + q * T)[ok]
                idx = e * (d // 2) + c
                np.add.at(reads, idx, 1)
                w = words[idx]
                for half, ci in ((w & 0xFFFF, c), (w >> 16, c + d // 2)):
                    mag, neg = (half & 0x7FFF).astype(np.int64), ((half >> 15) & 1).astype(np.int64)
                    assert np.array_equal(mag * (1 - 2 * neg), x[e, ci]), (G, l, q)
    assert (reads == 1).all()
