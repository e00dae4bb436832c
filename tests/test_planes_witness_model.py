"""numpy models behind lf_dev_planes_check and lf_dev_pack_planes, run before the kernels do.

1. The canonical rules of lf.h against their definition, the fixed point
   pack_coeffs(recompose(decode_planes(b))) == b, with tests/planes_pack.py and
   tests/planes_decode.py as they are: every sm16 half value at K = 15 and K = 7, every
   (nz, ng) pair of one coefficient over 3 planes at d = 24 (and the bits 24..31), every
   (digit, sign) pattern of a quarter over 3 planes at d = 4096 -- alone in each quarter and beside
   every pattern of each other quarter: the quarters are separate bit columns of the byte, so the
   2^24 byte triples of a quad are covered by their pairs.
2. The thread-to-word index arithmetic of the two new pack kernels (planes_witness.hip's
   k_pack_smp2 and k_pack_mask24, through planes_witness.hpp's sm16_unit and pk24_slot /
   pk24_word) against pack_coeffs, for d = 24 and d = 16 .. 512."""
import itertools

import numpy as np
import pytest

from planes_decode import decode_planes, planes_u64
from planes_pack import pack_coeffs, pack_digits

POW2 = [16, 32, 64, 128, 256, 512]


def recompose(digits):
    """[K][N][d] digits -> sum_k 2^k digit_k, [N][d]"""
    K = digits.shape[0]
    return sum(digits[k].astype(np.int64) << k for k in range(K))


def fixed_point(buf, d, K, N):
    """pack(recompose(decode(buf))) as bytes, beside buf's bytes"""
    x = recompose(decode_planes(buf, d, K, N))
    return pack_coeffs(x, d, K).view(np.uint8), np.ascontiguousarray(buf).view(np.uint8)


# ---------------------------------------------------------------- the rules, restated
def sm16_rule(half, K):
    half = np.asarray(half, np.uint32)
    return (((half & 0x7FFF) >> K) == 0) & (half != 0x8000)


def mask24_rule(masks):
    """masks [K] u64 of one element"""
    m = np.asarray(masks, np.uint64)
    nz, ng = (m & np.uint64(0xFFFFFFFF)).astype(np.uint32), (m >> np.uint64(32)).astype(np.uint32)
    if ((nz | ng) & 0xFF000000).any():
        return False
    for i in range(24):
        signed = {k for k in range(len(m)) if ng[k] >> i & 1}
        digit = {k for k in range(len(m)) if nz[k] >> i & 1}
        if signed and signed != digit:
            return False
    return True


def sm8_rule(quad):
    """quad [K] bytes of one coefficient quad"""
    q = np.asarray(quad, np.uint8)
    if (q >> 4 != q[0] >> 4).any():
        return False
    for b in range(4):
        if q[0] >> (4 + b) & 1 and not (q >> b & 1).any():
            return False
    return True


# ---------------------------------------------------------------- 1. rules == fixed point
@pytest.mark.parametrize("K", [15, 7])
def test_sm16_rule_is_the_fixed_point(K):
    d, N = 1024, 64
    halves = np.arange(65536, dtype=np.uint16)  # every half value once
    np.random.default_rng(K).shuffle(halves)
    buf = halves.view(np.uint64)
    assert buf.size == planes_u64(d, K, N)
    back, orig = fixed_point(buf, d, K, N)
    same = back.view(np.uint16) == orig.view(np.uint16)
    assert np.array_equal(same, sm16_rule(halves, K))
    assert same.sum() == 2 * (1 << K) - 1  # |x| < 2^K, one zero


def test_mask24_rule_is_the_fixed_point():
    d, K = 24, 3
    pairs = [(0, 0), (1, 0), (1, 1), (0, 1)]  # (nz, ng) of one coefficient on one plane
    combos = list(itertools.product(pairs, repeat=K))
    cols = [0, 23]
    extra = [(bit, hi) for bit in (24, 31) for hi in (0, 32)]  # a bit above the 24 coefficients, either word
    N = len(combos) * len(cols) + len(extra)
    m = np.zeros((K, N), np.uint64)
    e = 0
    for i in cols:
        for c in combos:
            for k, (nz, ng) in enumerate(c):
                m[k, e] = np.uint64(nz << i | ng << (32 + i))
            e += 1
    for bit, hi in extra:
        m[:, e] = np.uint64(0x5)  # a canonical +5 at coefficient 0 .. 2 on every plane
        m[1, e] |= np.uint64(1 << (bit + hi))
        e += 1
    # every other coefficient of these elements carries a canonical value, so one entry decides
    buf = m.reshape(-1)
    back, orig = fixed_point(buf, d, K, N)
    same = (back.view(np.uint64).reshape(K, N) == orig.view(np.uint64).reshape(K, N)).all(axis=0)
    rule = np.array([mask24_rule(m[:, j]) for j in range(N)])
    assert np.array_equal(same, rule)
    assert rule.sum() == 2 * (2 * (1 << K) - 1)  # per column: the values -7 .. 7
    assert not rule[-len(extra):].any()


def test_sm8_rule_is_the_fixed_point():
    d, K = 4096, 3
    pat = list(itertools.product(range(4), repeat=K))  # per plane: digit bit | sign bit << 1, of one quarter

    def byte_planes(assign):
        """{quarter: pattern} -> the K bytes of a quad"""
        q = np.zeros(K, np.uint8)
        for b, p in assign.items():
            for k in range(K):
                q[k] |= (p[k] & 1) << b | (p[k] >> 1) << (4 + b)
        return q

    quads = [byte_planes({b: p}) for b in range(4) for p in pat]
    for b0, b1 in itertools.combinations(range(4), 2):
        quads += [byte_planes({b0: p0, b1: p1}) for p0 in pat for p1 in pat]
    quads = np.array(quads, np.uint8)  # [n][K]
    N = -(-len(quads) // 1024)
    by = np.zeros((N, K, 32, 32), np.uint8)  # [e][k][r][j]: quad a = r + 32 j
    for n, q in enumerate(quads):
        e, a = divmod(n, 1024)
        by[e, :, a & 31, a >> 5] = q
    back, orig = fixed_point(by.reshape(-1).view(np.uint64), d, K, N)
    same = (back.reshape(N, K, 32, 32) == orig.reshape(N, K, 32, 32)).all(axis=1)  # [e][r][j]
    for n, q in enumerate(quads):
        e, a = divmod(n, 1024)
        assert same[e, a & 31, a >> 5] == sm8_rule(q), (n, q)
    assert sum(sm8_rule(q) for q in quads[:4 * len(pat)]) == 4 * (2 * (1 << K) - 1)


def test_per_plane_formats_take_any_digits():
    """recompose(decode(pack_digits(D))) = sum_k 2^k D_k for planes that are not the digits of one number"""
    rng = np.random.default_rng(11)
    for d, K, N in ((24, 15, 7), (4096, 4, 2)):
        dg = rng.integers(-1, 2, size=(K, N, d), dtype=np.int64)
        got = recompose(decode_planes(pack_digits(dg, d), d, K, N))
        assert np.array_equal(got, sum(dg[k] << k for k in range(K)))


# ---------------------------------------------------------------- 2. the pack kernels' index arithmetic
def sm16(x):
    return (abs(int(x)) & 0x7FFF) | (0x8000 if x < 0 else 0)


def coeffs(N, d, K, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-(1 << K) + 1, 1 << K, size=(N, d), dtype=np.int64)
    x[0, 0], x[0, -1], x[-1, 0], x[-1, -1] = (1 << K) - 1, -(1 << K) + 1, -1, 1 << (K - 1)
    return x


@pytest.mark.parametrize("d", POW2)
@pytest.mark.parametrize("N", [5, 85])
def test_pack_smp2_units(d, N):
    """thread u owns words 4 u .. 4 u + 3: element e = 4 u / (d / 2), word j = 4 u mod (d / 2) of it, low
    halves the coefficients j .. j + 3, high halves j + d / 2 ..; every word is written exactly once"""
    K = 15
    x = coeffs(N, d, K, 100 + d + N)
    wpe = d // 2
    words = np.zeros(N * wpe, np.uint32)
    hits = np.zeros(N * wpe, np.int32)
    assert (N * wpe) % 4 == 0
    for u in range(N * wpe // 4):
        e, j = divmod(4 * u, wpe)
        assert j % 4 == 0 and j + 3 < wpe  # both 32-byte runs stay inside the element
        for i in range(4):
            words[e * wpe + j + i] = sm16(x[e, j + i]) | sm16(x[e, j + wpe + i]) << 16
            hits[e * wpe + j + i] += 1
    assert (hits == 1).all()
    assert np.array_equal(words.view(np.uint64), pack_coeffs(x, d, K))


@pytest.mark.parametrize("N,K", [(5, 15), (35, 15), (85, 15), (300, 15), (513, 9)])
def test_pack_mask24_block(N, K):
    """a block of 256 threads: thread t brings words t + 256 q (q < 24) of the block's run of f_coeff into
    the tile (entry el 26 + i), then reads element t's twelve u32 (t 13 + p) and writes plane k at k N + e"""
    x = coeffs(N, 24, K, 200 + N)
    flat = x.reshape(-1)
    planes = np.full(K * N, np.uint64(0xFFFFFFFFFFFFFFFF))
    for blk in range(-(-N // 256)):
        tile = np.zeros(256 * 26, np.uint16)
        written = np.zeros(256 * 26, bool)
        for t in range(256):
            for q in range(24):
                o = t + 256 * q
                g = blk * 256 * 24 + o
                if g < N * 24:
                    slot = (o // 24) * 26 + o % 24
                    assert not written[slot]
                    tile[slot], written[slot] = sm16(flat[g]), True
        t32 = tile.view(np.uint32)
        for t in range(256):
            e = blk * 256 + t
            if e >= N:
                continue
            assert written[t * 26:t * 26 + 24].all()
            w = [int(t32[t * 13 + p]) for p in range(12)]
            for k in range(K):
                nz = ng = 0
                for i in range(24):
                    half = w[i >> 1] >> (16 * (i & 1))
                    bit = half >> k & 1
                    nz |= bit << i
                    ng |= (bit & (half >> 15)) << i
                planes[k * N + e] = np.uint64(nz | ng << 32)
    assert np.array_equal(planes, pack_coeffs(x, 24, K))
