"""A Python model of the index arithmetic of k_decompose_pow2
(latticeum_amd/csrc/decompose_pow2.hip), the fused decomposition at X^d + 1,
d = 16 .. 512: the same tid -> (element j, transform thread t) split, the same
expressions for the packed-word, LDS, operand-row and dead-flag indices, evaluated
for every thread of every block (the threads of a block as one numpy vector). It
settles, before the kernel runs, that every packed word is written exactly once,
that every LDS index lies in the declared tile, that every operand piece of a live
unit is written exactly once and below frag_elems, that a group past W produces no
index, that every dead flag of the step's row mask is written once per owned
position, and that chunk and half are those of fragpos.hpp (compiled for the host,
under the address and UB sanitizers)."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from test_stockham_model import check_passes, stockham4, tables

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DEGREES = [16, 32, 64, 128, 256, 512]
WIDTHS = [1, 16, 17, 33]
L, K = 5, 15

DRIVER = r"""
#include "fragpos.hpp"
#include <cstdio>
using namespace lfk;
int main() {
  const size_t Ws[] = {1, 16, 17, 33};
  const int Ls[] = {1, 5};
  for (size_t W : Ws)
    for (int L : Ls) {
      const size_t nG = frag_groups(W), ptop = frag_ptop(nG, L);
      printf("%zu %d %zu %zu %zu", W, L, nG, ptop, frag_npos(nG, L));
      for (size_t G = 0; G < nG; G++)
        for (int l = 0; l < L; l++) printf(" %zu", frag_pos(G, l, L, ptop));
      printf("\n");
    }
  return 0;
}
"""


# ---------------------------------------------------------------- fragpos.hpp / frag.hpp, restated
def frag_groups(Wp):
    return (Wp + 15) // 16


def frag_ptop(nG, Lp):
    return 2 * ((nG * (Lp - 1) + 1) // 2) if Lp > 1 else 0


def frag_npos(nG, Lp):
    return frag_ptop(nG, Lp) + 2 * ((nG + 1) // 2)


def frag_pos(G, l, Lp, ptop):
    return G if Lp == 1 else G * (Lp - 1) + l if l < Lp - 1 else ptop + G


def fv_index(s, nch, c, r, h):
    return ((((s >> 2) * nch + c) * 32 + r) * 2 + h) * 32 + (s & 3)


def frag_elems(d, nch):
    return d * nch * 8 * 64


@pytest.fixture(scope="module")
def host_fragpos():
    """{(W, L): (nG, ptop, npos, [frag_pos(G, l)])} from the host compile of fragpos.hpp"""
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "fp.cpp", Path(td) / "fp"
        src.write_text(DRIVER)
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            f"-I{ROOT / 'latticeum_amd/csrc'}", str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        v = [int(x) for x in line.split()]
        got[(v[0], v[1])] = (v[2], v[3], v[4], v[5:])
    return got


# ---------------------------------------------------------------- the kernel's shape (struct P2<D>)
def shape(D):
    T = min(D // 4, 64)
    return T, 16 * T, D // T  # T, NTH, PER


def result_half(D):
    """which ping-pong half ring::stockham4 returns: every pass swaps x and y, so after
    an odd number of passes (the stockham4 model's own pass list at this T) the result is
    in y, the second half"""
    _, passes = stockham4([0] * D, D, shape(D)[0], tables(D)[1], False)
    return len(passes) % 2


def step_sides(extra, p0, z0):
    """api_step.hip step_sides: (row0[2], row_p0[2], row mask)"""
    row0 = [extra + s * (K - 1) for s in range(2)]
    row_p0 = [0 if (z0 and s == 1) else extra + 2 * (K - 1) + s if p0 else -1 for s in range(2)]
    mask = 0
    for s in range(2):
        for k in range(1, K):
            mask |= 1 << (row0[s] + k - 1)
        if row_p0[s] >= 0:
            mask |= 1 << row_p0[s]
    return row0, row_p0, mask


def run_model(D, W, extra, p0, z0, seed):
    """every block of one launch; returns the index streams"""
    T, NTH, PER = shape(D)
    PH, H = PER // 2, D // 2
    N = W * L
    nG = frag_groups(W)
    ptop = frag_ptop(nG, L)
    nch = frag_npos(nG, L) // 2
    row0, row_p0, mask = step_sides(extra, p0, z0)
    rng = np.random.default_rng(seed)
    tid = np.arange(NTH)
    j, t = tid // T, tid % T
    # x = buf + j D, y = buf + 16 D + j D; r = what stockham4 returns to this thread
    r = (16 * D if result_half(D) else 0) + j * D
    packed = [[], []]      # per side: word indices
    wk = [[], []]          # per side: w_ccs_k word indices
    rows_u64 = [[], []]    # per side: f_k / f_coeff_k word indices
    lds_fill, lds_tile = set(), set()
    frag, dead, live_units, pos_seen = [], [], [], []
    lds_fill_done = False
    for unit in range(2 * nG):  # grid-stride: one unit per block iteration
        side = int(unit >= nG)
        G = unit - side * nG
        g = 16 * G + j
        ok = g < W
        e0 = np.where(ok, g * L, 0)
        # the top limb holds 4 bits at B = 2^15, L = 5; below it any plane may be zero
        mags = [int(rng.integers(0, 1 << K)) | 1 for _ in range(L - 1)] + [int(rng.integers(0, 16))]
        for l in range(L):
            for q in range(PH):
                i = t + q * T
                assert (i < H).all()
                packed[side].append(((e0 + l) * (D // 2) + i)[ok])  # smp2_word(e0 + l, D, i)
        for k in range(K):
            row = row0[side] + k - 1 if k > 0 else row_p0[side]
            for l in range(L - 1, -1, -1):
                live = bool((mags[l] >> k) & 1)
                e = k * N + e0 + l
                for q in range(PER):
                    i = t + q * T
                    if live and not lds_fill_done:  # the same indices at every (unit, k, l)
                        lds_fill.update((j * D + i).tolist())  # x[i], x = buf + j D
                    rows_u64[side].append((e * D + i)[ok])
                lds_fill_done = lds_fill_done or live
                if row >= 0:
                    pos = frag_pos(G, l, L, ptop)
                    pos_seen.append((G, l, pos))
                    dead.append((pos * 32 + row, 0 if live else 1))  # thread 0
                    if live:
                        live_units.append((pos, row))
                        for s0 in range(0, D, NTH) if not lds_tile else ():  # the same at every unit
                            s = tid + s0
                            tile = (r - j * D)[s < D]  # each thread's own `tile` pointer
                            s = s[s < D]
                            for jj in range(16):
                                lds_tile.update((tile + jj * D + s).tolist())
                        for s0 in range(0, D, NTH):
                            s = tid + s0
                            s = s[s < D]
                            out = fv_index(s, nch, pos >> 1, row, pos & 1)
                            for b in range(8):
                                frag.append(out + 4 * b)
            for q in range(PER):
                wk[side].append(((k * W + g) * D + t + q * T)[ok])
    return dict(N=N, nG=nG, ptop=ptop, nch=nch, mask=mask, packed=packed, wk=wk, rows=rows_u64, lds_fill=lds_fill,
                lds_tile=lds_tile, frag=np.concatenate(frag) if frag else np.zeros(0, np.int64), dead=dead,
                live_units=live_units, pos_seen=pos_seen, row_p0=row_p0)


# extra (commit(z) rides along), p0 (no f_k: plane 0 has a row), z0 (side 1's plane 0 is row 0)
ROWS = [(1, True, True), (0, True, False), (1, False, True)]


@pytest.mark.parametrize("extra,p0,z0", ROWS)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("D", DEGREES)
def test_indices(host_fragpos, D, W, extra, p0, z0):
    T, NTH, PER = shape(D)
    assert NTH <= 1024 and (D // 4) % T == 0 and PER % 2 == 0 and PER >= 4
    m = run_model(D, W, extra, p0, z0, 7 * D + W)
    N, nG, nch = m["N"], m["nG"], m["nch"]
    # packed words: [0, N d / 2), each exactly once, per side
    for s in range(2):
        idx = np.sort(np.concatenate(m["packed"][s]))
        assert np.array_equal(idx, np.arange(N * D // 2)), "packed words"
        # w_ccs_k [K][W] and the u64 rows [K][N]: exactly once, nothing for a group past W
        assert np.array_equal(np.sort(np.concatenate(m["wk"][s])), np.arange(K * W * D))
        assert np.array_equal(np.sort(np.concatenate(m["rows"][s])), np.arange(K * N * D))
    # LDS: the fill covers the first half; the transpose reads exactly the half in which
    # stockham4 leaves the 16 results (element jj's row at half base + jj D), inside the tile
    tile = 2 * 16 * D  # P2<D>::LDS_U64
    assert m["lds_fill"] == set(range(16 * D))
    base = 16 * D * result_half(D)
    assert m["lds_tile"] == set(range(base, base + 16 * D)) and base + 16 * D <= tile
    # operand pieces: below frag_elems, exactly once, and exactly those of the live units
    f = m["frag"]
    assert f.size == 0 or (f.min() >= 0 and f.max() < frag_elems(D, nch))
    assert np.unique(f).size == f.size, "an operand piece written twice"
    want = set()
    for pos, row in m["live_units"]:
        for s in range(D):
            for b in range(8):
                want.add(fv_index(s, nch, pos >> 1, row, pos & 1) + 4 * b)
    assert set(f.tolist()) == want
    # dead flags: once per (owned position, row of the mask), inside [2 nch][32]
    flags = [i for i, _ in m["dead"]]
    assert len(set(flags)) == len(flags) and max(flags) < nch * 64
    owned = {pos for _, _, pos in m["pos_seen"]}
    assert len(owned) == nG * L
    rows = [r for r in range(32) if (m["mask"] >> r) & 1]
    assert set(flags) == {pos * 32 + r for pos in owned for r in rows}
    # chunk and half: fragpos.hpp on the host
    hG, hptop, hnpos, hpos = host_fragpos[(W, L)]
    assert (hG, hptop, hnpos) == (nG, m["ptop"], 2 * nch)
    for G, l, pos in m["pos_seen"]:
        assert pos == hpos[G * L + l] and pos < hnpos


@pytest.mark.parametrize("D", DEGREES)
def test_transform_threads_stay_in_their_rows(D):
    """element j's T threads run ring::stockham4<D, T, false> on x = buf + j D and
    y = buf + 16 D + j D: every pass index is below D (the model of
    tests/test_stockham_model.py at this T), so both rows stay inside the tile"""
    T, NTH, PER = shape(D)
    _, passes = stockham4([0] * D, D, T, tables(D)[1], False)
    check_passes(D, T, passes)
    for j in range(16):
        assert j * D + D <= 16 * D and 16 * D + j * D + D <= 2 * 16 * D


def test_restated_positions_match_host(host_fragpos):
    for (W, Lp), (nG, ptop, npos, pos) in host_fragpos.items():
        assert nG == frag_groups(W) and ptop == frag_ptop(nG, Lp) and npos == frag_npos(nG, Lp)
        assert pos == [frag_pos(G, l, Lp, ptop) for G in range(nG) for l in range(Lp)]
