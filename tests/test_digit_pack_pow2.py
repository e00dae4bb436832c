"""The packed digit format of X^d + 1, d = 16 .. 512 (latticeum_amd/csrc/digitpack.hpp
smp2_*), on the CPU: a stand-alone program built with the address and
undefined-behaviour sanitizers checks, at every degree, that every coefficient index
maps to its own half of a word inside the element's d / 2 words, that encode then
decode returns every digit of x in {0, +-1, +-(2^14 - 1), +-2^14, +-(2^15 - 1)}, and
that +-2^15 is flagged as an overflow. It prints one packed element per degree, which
the Python side decodes from include/lf.h's wording alone. lf_fold_step_planes_len is
checked against the table in lf.h, zeros included."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import latticeum_amd as LA
from latticeum_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DEGREES = [16, 32, 64, 128, 256, 512]
K = 15
XS = [0, 1, -1, (1 << 14) - 1, -((1 << 14) - 1), 1 << 14, -(1 << 14), (1 << 15) - 1, -((1 << 15) - 1)]

DRIVER = r"""
#include "digitpack.hpp"
#include <cstdio>
#include <vector>
using namespace lfk;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)
static int digit(int64_t x, int k) { const int b = (int)(((x < 0 ? -x : x) >> k) & 1); return x < 0 ? -b : b; }
static const int64_t XS[] = {0, 1, -1, (1 << 14) - 1, -((1 << 14) - 1), 1 << 14, -(1 << 14), (1 << 15) - 1, -((1 << 15) - 1)};

static void check_degree(int d) {
  const int K = 15, NX = sizeof(XS) / sizeof(XS[0]);
  const size_t N = 3;
  CHECK(smp2_degree(d) && smp2_words(d) == (size_t)d / 2);
  std::vector<uint32_t> buf(N * smp2_words(d), 0);
  std::vector<int> hit(buf.size() * 2, 0);
  // coefficient i of element e holds XS[(e d + i + shift) % NX]: every x at every index over the shifts
  for (int shift = 0; shift < NX; shift++) {
    for (auto &w : buf) w = 0;
    for (auto &h : hit) h = 0;
    for (size_t e = 0; e < N; e++)
      for (int i = 0; i < d; i++) {
        const size_t w = smp2_word_of(e, d, i);
        CHECK(w < buf.size());
        if (w >= buf.size()) continue;
        CHECK(w / smp2_words(d) == e && w == smp2_word(e, d, i % (d / 2)) && smp2_half_of(d, i) == i / (d / 2));
        hit[2 * w + smp2_half_of(d, i)]++;
        const int64_t x = XS[(e * d + i + shift) % NX];
        CHECK(!sm16_overflow(x, K));
        buf[w] |= sign_mag16(x) << (16 * smp2_half_of(d, i));
      }
    for (int h : hit) CHECK(h == 1);
    for (size_t e = 0; e < N; e++)
      for (int i = 0; i < d; i++)
        for (int k = 0; k < K; k++) CHECK(smp2_digit(buf.data(), e, d, i, k) == digit(XS[(e * d + i + shift) % NX], k));
    // the pair encoder the kernel uses
    for (size_t e = 0; e < N; e++)
      for (int j = 0; j < d / 2; j++)
        CHECK(buf[smp2_word(e, d, j)] == smp2_make(XS[(e * d + j + shift) % NX], XS[(e * d + j + d / 2 + shift) % NX]));
    if (shift == 1) {
      printf("smp2 d=%d", d);
      for (uint32_t w : buf) printf(" %08x", w);
      printf("\n");
    }
  }
}

int main() {
  CHECK(sm16_overflow((int64_t)1 << 15, 15) && sm16_overflow(-((int64_t)1 << 15), 15));
  CHECK(!sm16_overflow(((int64_t)1 << 15) - 1, 15) && !sm16_overflow(-(((int64_t)1 << 15) - 1), 15));
  for (int d : {16, 32, 64, 128, 256, 512}) check_degree(d);
  for (int d : {0, 8, 24, 48, 1024, 2048, 4096}) CHECK(!smp2_degree(d));
  printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails != 0;
}
"""


@pytest.fixture(scope="module")
def driver_output():
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "dp2.cpp", Path(td) / "dp2"
        src.write_text(DRIVER)
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{ROOT / 'latticeum_amd/csrc'}", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([str(exe)], capture_output=True, text=True)
    return out


def test_maps_and_round_trips_under_sanitizers(driver_output):
    out = driver_output
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def decode_words(words, d, N):
    """include/lf.h: word j (j < d / 2) of element e at e d / 2 + j; coefficient j in the low
    half, coefficient j + d / 2 in the high half; bits 0..14 = |x|, bit 15 = x is negative"""
    w = np.asarray(words, np.uint32).reshape(N, d // 2)
    halves = np.concatenate([w & 0xFFFF, w >> 16], axis=1).astype(np.int64)  # [N][d]
    mag = halves & 0x7FFF
    return np.where(halves & 0x8000, -mag, mag)


@pytest.mark.parametrize("d", DEGREES)
def test_printed_words_decode_as_the_public_header_says(driver_output, d):
    N = 3
    line = next(l for l in driver_output.stdout.splitlines() if l.startswith(f"smp2 d={d} "))
    words = np.array([int(w, 16) for w in line.split()[2:]], np.uint32)
    assert words.size == N * d // 2
    want = np.array([XS[(i + 1) % len(XS)] for i in range(N * d)], np.int64).reshape(N, d)
    assert np.array_equal(decode_words(words, d, N), want)


def params_of(d, K_=K, b_small=2):
    pr = LA.LfParams()
    pr.d, pr.B, pr.L, pr.b_small, pr.K = d, 1 << 15, 5, b_small, K_
    return pr


def test_planes_len_table():
    """lf_fold_step_planes_len: u64 words of one side's planes; 0 where there is no packed form"""
    f = LA.fold_step_planes_len  # module level: the entry is host only and takes no context
    for N in (0, 5, 85):
        assert f(params_of(24), N) == K * N
        assert f(params_of(1024), N) == N * 256
        assert f(params_of(4096), N) == N * K * 128
        assert f(params_of(4096, 7), N) == N * 7 * 128
        for d in DEGREES:
            assert f(params_of(d), N) == N * d // 4
            assert f(params_of(d, 3), N) == N * d // 4  # all K planes in one word
    for d in (2048, 8, 48, 8192):  # no packed form, or no ring of the library
        assert f(params_of(d), 85) == 0
    for d in [24, 1024, 4096] + DEGREES:
        assert f(params_of(d, b_small=4), 85) == 0
        assert f(params_of(d, 16), 85) == 0
    assert _lib.load().lf_fold_step_planes_len(None, 85) == 0
