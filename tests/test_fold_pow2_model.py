"""A numpy model of the coefficient-form fold at X^d + 1, d = 16 .. 512
(latticeum_amd/csrc/fold_coeff_pow2.hip, index arithmetic in foldpow2.hpp): the operands
are built lane by lane as the kernel builds them -- the reversed byte table of a
challenge, the 16 table bytes a lane cuts from it for the A tile of (row tile, column
tile), the 16 digit bytes it cuts from the packed smp2 words for the B tile, the rows a
wave owns, the split of the 2K witnesses over blocks and the sum of their int32 partials
-- then multiplied with the lane map of the 32 x 32 x 32 i8 product and compared with the
schoolbook negacyclic sum. No GPU and no library: plain integers."""
import numpy as np
import pytest

DEGREES = [16, 32, 64, 128, 256, 512]
K = 15
TOP = 1 << 14


# ---------------------------------------------------------------- the formats
def sm16(x):
    """digitpack.hpp sign_mag16: bits 0..14 = |x|, bit 15 = x is negative"""
    x = np.asarray(x, np.int64)
    return (np.abs(x) & 0x7FFF) | np.where(x < 0, 0x8000, 0)


def pack_words(x):
    """x [N][d] -> smp2 words [N][d / 2]: coefficient j in the low half, j + d / 2 in the high"""
    d = x.shape[1]
    return (sm16(x[:, :d // 2]) | (sm16(x[:, d // 2:]) << 16)).astype(np.uint32)


def digits_of(x, k):
    """digit k of x: sign(x) bit_k(|x|)"""
    return np.sign(x) * ((np.abs(x) >> k) & 1)


def table(rho, d):
    """foldpow2.hpp: tab[d - c] = rho[c]; tab[2 d - c] = -rho[c], c > 0; zero elsewhere"""
    tab = np.zeros(2 * d + 32, np.int8)
    c = np.arange(d)
    tab[d - c] = rho
    tab[2 * d - c[1:]] = -rho[1:]
    return tab


def digit_bytes(hw, k):
    """fp2_digit_byte of 16-bit sign|magnitude half words, as signed bytes"""
    bit = (hw >> k) & 1
    return np.where(hw & 0x8000, -bit, bit).astype(np.int64)


# ---------------------------------------------------------------- the product, lane by lane
LANE = np.arange(64)
COL, H = LANE & 31, LANE >> 5
X = np.arange(16)


def mfma(a, b, acc):
    """v_mfma_i32_32x32x32_i8: lane l = col + 32 h holds A[col][16 h + x] and B[16 h + x][col];
    register i of the result is row 8 (i / 4) + 4 h + (i % 4), column col"""
    A = np.zeros((32, 32), np.int64)
    B = np.zeros((32, 32), np.int64)
    A[COL[:, None], 16 * H[:, None] + X] = a
    B[16 * H[:, None] + X, COL[:, None]] = b
    Dm = A @ B
    i = np.arange(16)
    rows = 8 * (i >> 2)[None, :] + 4 * H[:, None] + (i & 3)[None, :]
    return acc + Dm[rows, COL[:, None]]


def geometry(d):
    nq = d // 32 if d >= 32 else 1
    rt = min(nq, 8)
    wpt = nq // rt
    return nq, rt, wpt, 4 // wpt


def model_fold(d, rc, words, N, ks_n=1):
    """f0_coeff [N][d] as k_fold_coeff_pow2 and k_fold_pow2_sum compute it; words [2][N][d / 2]"""
    nw = 2 * K
    nq, rt, wpt, tpb = geometry(d)
    tabs = [table(rc[i], d) for i in range(nw)]
    ntile = (N + 31) // 32
    ngrp = (ntile + tpb - 1) // tpb
    part = np.zeros((ks_n, N, d), np.int64)
    for task in range(ngrp * ks_n):
        for wv in range(4):
            tile = (task // ks_n) * tpb + wv // wpt
            if tile >= ntile:
                continue
            ks = task % ks_n
            i0, i1 = ks * nw // ks_n, (ks + 1) * nw // ks_n
            t0 = (wv % wpt) * rt
            e = tile * 32 + COL
            valid = e < N
            ee = np.where(valid, e, 0)
            acc = [np.zeros((64, 16), np.int64) for _ in range(rt)]
            if d == 16:
                o = 16 - (LANE & 15)
                for m in range(i0 // 2, i1 // 2):
                    i = 2 * m + H  # per lane
                    s, k = (i >= K).astype(int), i - K * (i >= K)
                    w = words[s, ee]  # [64][8]
                    hw = np.concatenate([w & 0xFFFF, w >> 16], axis=1).astype(np.int64)
                    b = np.stack([digit_bytes(hw[l], k[l]) for l in range(64)])
                    a = np.stack([tabs[i[l]][o[l]:o[l] + 16] for l in range(64)]).astype(np.int64)
                    a[COL >= 16] = 0
                    acc[0] = mfma(a, b, acc[0])
            else:
                obase = d + 16 * H - COL
                for s in range(2):
                    ka, kb = max(i0, s * K) - s * K, min(i1, (s + 1) * K) - s * K
                    for q in range(nq):
                        j0 = 32 * q + 16 * H
                        wi = (j0 & (d // 2 - 1))[:, None] + X
                        w = words[s][ee[:, None], wi].astype(np.int64)
                        hw = np.where((j0 >= d // 2)[:, None], w >> 16, w & 0xFFFF)
                        for k in range(ka, kb):
                            b = digit_bytes(hw, k)
                            tab = tabs[s * K + k]
                            for tt in range(rt):
                                o = obase - 32 * (t0 + tt - q)
                                assert o.min() >= 1 and o.max() + 15 <= 2 * d - 1  # inside the written table
                                a = tab[o[:, None] + X].astype(np.int64)
                                acc[tt] = mfma(a, b, acc[tt])
            assert max(np.abs(a_).max() for a_ in acc) < 2**31
            i = np.arange(16)
            for tt in range(rt):
                rows = 32 * (t0 + tt) + 8 * (i >> 2)[None, :] + 4 * H[:, None] + (i & 3)[None, :]
                keep = valid[:, None] & (rows < d)
                part[ks][np.broadcast_to(e[:, None], rows.shape)[keep], rows[keep]] = acc[tt][keep]
    assert np.abs(part).max() < 2**31
    return part.sum(axis=0)


def schoolbook(d, rc, x):
    """f0_coeff[e][c] = sum_i sum_j R_i[c][j] D_i[j][e]; x [2][N][d] the coefficients"""
    N = x.shape[1]
    c, j = np.arange(d)[:, None], np.arange(d)[None, :]
    out = np.zeros((N, d), np.int64)
    for s in range(2):
        for k in range(K):
            r = rc[s * K + k]
            R = np.where(c >= j, r[(c - j) % d], -r[(c - j) % d])
            out += digits_of(x[s], k) @ R.T
    return out


def random_inputs(d, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-TOP, TOP + 1, size=(2, N, d), dtype=np.int64)  # every balanced digit, +-2^14 included
    rc = rng.integers(-127, 128, size=(2 * K, d), dtype=np.int64)
    rc[0, 0], rc[0, d - 1], rc[2 * K - 1, 0], rc[2 * K - 1, d - 1] = 127, -127, -127, 127
    return x, rc


@pytest.mark.parametrize("d", DEGREES)
def test_product_equals_the_negacyclic_sum(d):
    N = 37  # a whole tile and a partial one
    x, rc = random_inputs(d, N, 100 + d)
    words = np.stack([pack_words(x[s]) for s in range(2)])
    assert np.array_equal(model_fold(d, rc, words, N), schoolbook(d, rc, x))


@pytest.mark.parametrize("d,ks_n", [(32, 30), (64, 6), (512, 15)])
def test_witness_splits_add_up(d, ks_n):
    """splits that cut inside a side (6: witnesses 15 .. 19 straddle nothing, 10 .. 14 end side 0),
    one witness a split (30), two (15)"""
    N = 5
    x, rc = random_inputs(d, N, 200 + d)
    words = np.stack([pack_words(x[s]) for s in range(2)])
    assert np.array_equal(model_fold(d, rc, words, N, ks_n), schoolbook(d, rc, x))


@pytest.mark.parametrize("d", DEGREES)
@pytest.mark.parametrize("sign", [1, -1])
def test_largest_sum_is_reached_inside_i32(d, sign):
    """every coefficient of both sides at sign (2^14 - 1) (14 live planes of one sign) and every
    rho_i the row c* of the Toeplitz matrix at +127: the sum at c* is 2 14 d 127"""
    N, cs = 3, d // 3
    x = np.full((2, N, d), sign * (TOP - 1), np.int64)
    j = np.arange(d)
    r = np.zeros(d, np.int64)
    r[(cs - j) % d] = np.where(j <= cs, 127, -127)
    rc = np.tile(r, (2 * K, 1))
    words = np.stack([pack_words(x[s]) for s in range(2)])
    got = model_fold(d, rc, words, N)
    assert np.array_equal(got, schoolbook(d, rc, x))
    worst = 2 * 14 * d * 127
    assert got[1, cs] == sign * worst and np.abs(got).max() == worst and worst < 2**31
    if d == 512:
        assert worst == 1820672


def perm(s0, s1, sel):
    """v_perm_b32: byte i of the result is byte sel_i of the eight bytes {s0 : s1} (s1 = bytes 0 .. 3)"""
    both = (s0.astype(np.uint64) << np.uint64(32)) | s1.astype(np.uint64)
    out = np.zeros_like(s1, dtype=np.uint64)
    for i in range(4):
        out |= ((both >> np.uint64(8 * ((sel >> (8 * i)) & 0xFF))) & np.uint64(0xFF)) << np.uint64(8 * i)
    return out.astype(np.uint32)


def test_digit_bytes_from_the_transposed_half_words():
    """the kernel's digit_src / digit_bytes: four half words' low and high bytes gathered with
    v_perm_b32, a plane's bit shifted to bit 0 of every byte, widened by 0xFF and masked by the
    sign bytes -- equal to fp2_digit_byte of each half word, whatever lies above bit 15"""
    rng = np.random.default_rng(7)
    hw = rng.integers(0, 1 << 32, size=(4096, 4), dtype=np.uint64).astype(np.uint32)
    hw[:16] &= 0x8000  # zero magnitudes of either sign
    t0 = perm(hw[:, 1], hw[:, 0], 0x05010400)
    t1 = perm(hw[:, 3], hw[:, 2], 0x05010400)
    lo, hi = perm(t1, t0, 0x05040100), perm(t1, t0, 0x07060302)
    sx = (((hi >> 7) & 0x01010101).astype(np.uint64) * 0xFE + 0x01010101).astype(np.uint32)
    for k in range(15):
        src, sh = (lo, k) if k < 8 else (hi, k - 8)
        b = ((((src >> sh) & 0x01010101).astype(np.uint64) * 0xFF).astype(np.uint32)) & sx
        got = np.stack([(b >> (8 * y)) & 0xFF for y in range(4)], axis=1).astype(np.uint8).view(np.int8)
        assert np.array_equal(got, digit_bytes(hw.astype(np.int64) & 0xFFFF, k))
