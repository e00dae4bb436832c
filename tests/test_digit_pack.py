"""The packed digit formats (latticeum_amd/csrc/digitpack.hpp) on the CPU: a stand-alone
program built with the address and undefined-behaviour sanitizers checks, per format,
that every logical coordinate maps inside the buffer, that no two coordinates share a
word / byte / bit, that encode then decode returns the digit for every |x| < 2^K at
K = 1, 2, 15, and that a magnitude of 2^K is flagged. It then packs one small seeded
witness (N = 3 elements; K = 2 and K = 15) in each format and prints the bytes, which the
Python side decodes with tests/planes_decode.py -- written from include/lf.h's wording,
not from the header -- and compares with the digits of the same seeded coefficients."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from planes_decode import decode_planes, digits_of

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

DRIVER = r"""
#include "digitpack.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace lfk;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)

// the test's own generator (the Python side repeats it): coefficient i of the run, |x| < 2^K
static int64_t coef(uint64_t i, int K) {
  uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const int64_t m = (int64_t)(z & ((1ull << K) - 1));
  return (z >> 40 & 1) ? -m : m;
}
static int digit(int64_t x, int k) { const int b = (int)(((x < 0 ? -x : x) >> k) & 1); return x < 0 ? -b : b; }

static void check_sm16(int K) {
  for (int64_t x = -((1 << K) - 1); x < (1 << K); x++) {
    CHECK(!sm16_overflow(x, K));
    const uint32_t w = sign_mag16(x);
    CHECK(w <= 0xFFFFu);
    for (int k = 0; k < K; k++) CHECK(sm16_digit(w, k) == digit(x, k));
    CHECK(sm16_digit(w << 16 | w, 0) == digit(x, 0));  // bits above 15 are ignored
  }
  CHECK(sm16_overflow((int64_t)1 << K, K) && sm16_overflow(-((int64_t)1 << K), K));
}

static void dump(const char *name, int K, const void *p, size_t bytes) {
  printf("%s K=%d", name, K);
  for (size_t i = 0; i < bytes; i++) printf(" %02x", ((const unsigned char *)p)[i]);
  printf("\n");
}

static void check_1024(int K, size_t N) {
  std::vector<uint32_t> buf(N * SM1024_WORDS, 0);
  std::vector<int> hit(buf.size() * 2, 0);
  for (size_t e = 0; e < N; e++)
    for (int j = 0; j < 1024; j++) {
      const size_t w = sm1024_word_of(e, j);
      CHECK(w < buf.size());
      if (w >= buf.size()) continue;
      CHECK(w == sm1024_word(e, j >> 6, j & 31) && w / SM1024_WORDS == e);
      hit[2 * w + sm1024_half_of(j)]++;
      buf[w] |= sign_mag16(coef(e * 1024 + j, K)) << (16 * sm1024_half_of(j));
    }
  for (int h : hit) CHECK(h == 1);
  for (size_t e = 0; e < N; e++)
    for (int j = 0; j < 1024; j++)
      for (int k = 0; k < K; k++) CHECK(sm1024_digit(buf.data(), e, j, k) == digit(coef(e * 1024 + j, K), k));
  dump("sm1024", K, buf.data(), buf.size() * 4);
}

static void check_24(int K, size_t N) {
  std::vector<uint32_t> sm(N * SM24_WORDS, 0);
  std::vector<int> hit(sm.size() * 2, 0);
  for (size_t e = 0; e < N; e++)
    for (int i = 0; i < 24; i++) {
      const size_t w = sm24_word(e, i >> 1);
      CHECK(w < sm.size());
      if (w >= sm.size()) continue;
      hit[2 * w + (i & 1)]++;
      sm[w] |= sign_mag16(coef(e * 24 + i, K)) << (16 * (i & 1));
    }
  for (int h : hit) CHECK(h == 1);
  // the masks, made from the words as the decomposition makes them
  std::vector<uint32_t> mk(2 * mask24_elems(K, N), 0);
  std::vector<int> seen(mask24_elems(K, N), 0);
  for (int k = 0; k < K; k++)
    for (size_t e = 0; e < N; e++) {
      const size_t m = mask24_index(k, N, e);
      CHECK(m < mask24_elems(K, N));
      if (m >= mask24_elems(K, N)) continue;
      seen[m]++;
      uint32_t nz = 0, ng = 0;
      for (int i = 0; i < 24; i++) {
        CHECK(sm24_digit(sm.data(), e, i, k) == digit(coef(e * 24 + i, K), k));
        mask24_put(sm[sm24_word(e, i >> 1)] >> (16 * (i & 1)), k, i, nz, ng);
      }
      CHECK(!(nz >> 24) && !(ng >> 24) && !(ng & ~nz));
      for (int i = 0; i < 24; i++) CHECK(mask24_digit(nz, ng, i) == digit(coef(e * 24 + i, K), k));
      mk[2 * m] = nz, mk[2 * m + 1] = ng;
    }
  for (int s : seen) CHECK(s == 1);
  dump("mask24", K, mk.data(), mk.size() * 4);
}

static void check_4096(int K, size_t N) {
  std::vector<uint64_t> mo(N * SM4_WORDS, 0);
  std::vector<int> hit(mo.size(), 0);
  for (size_t e = 0; e < N; e++)
    for (int a = 0; a < 1024; a++) {
      const size_t w = sm4_word(e, a);
      CHECK(w < mo.size());
      if (w >= mo.size()) continue;
      hit[w]++;
      uint64_t used = 0;
      for (int b = 0; b < 4; b++) {
        const uint64_t v = sm4_put(sign_mag16(coef(e * 4096 + a + 1024 * b, K)), b);
        CHECK(!(used & v));  // the four quarters share no bit
        used |= v, mo[w] |= v;
      }
      CHECK(!(sm4_put(0xFFFFu, 0) & sm4_put(0xFFFFu, 1)) && !(sm4_put(0xFFFFu, 2) & sm4_put(0xFFFFu, 3)));
      for (int b = 0; b < 4; b++)
        for (int k = 0; k < K; k++) CHECK(sm4_digit(mo[w], b, k) == digit(coef(e * 4096 + a + 1024 * b, K), k));
    }
  for (int h : hit) CHECK(h == 1);
  // the digit bytes, made from the Morton words as k_pack_sm8 makes them
  std::vector<unsigned char> by(N * sm8_words(K) * 4, 0);
  std::vector<int> bhit(by.size(), 0);
  for (size_t e = 0; e < N; e++)
    for (int k = 0; k < K; k++)
      for (int a = 0; a < 1024; a++) {
        const size_t o = sm8_byte_of(e, K, k, a);
        CHECK(o < by.size());
        if (o >= by.size()) continue;
        CHECK(o == sm8_byte(e, K, k, a & 31, a >> 5) && o / (sm8_words(K) * 4) == e);
        CHECK(sm8_word(e, K, k, a & 31, a >> 7) == o / 4 && sm8_words(K) == K * SM8_PLANE_WORDS);
        bhit[o]++;
        const uint64_t w = mo[sm4_word(e, a)];
        const uint32_t v = sm8_make(sm4_nibble(w, k), sm4_signs(w));
        CHECK(v <= 0xFFu);
        by[o] = (unsigned char)v;
        for (int b = 0; b < 4; b++) CHECK(sm8_digit(v, b) == digit(coef(e * 4096 + a + 1024 * b, K), k));
      }
  for (int h : bhit) CHECK(h == 1);
  dump("sm8", K, by.data(), by.size());
}

int main() {
  for (int K : {1, 2, 15}) check_sm16(K);
  for (int K : {2, 15}) {
    check_1024(K, 3);
    check_24(K, 3);
    check_4096(K, 3);
  }
  printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails != 0;
}
"""


def coef(i, K):
    """the driver's generator, vectorised"""
    m64 = np.uint64
    with np.errstate(over="ignore"):
        z = (np.asarray(i, m64) + m64(1)) * m64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> m64(30))) * m64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> m64(27))) * m64(0x94D049BB133111EB)
    z ^= z >> m64(31)
    m = (z & m64((1 << K) - 1)).astype(np.int64)
    return np.where((z >> m64(40)) & m64(1), -m, m)


@pytest.fixture(scope="module")
def driver_output():
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "dp.cpp", Path(td) / "dp"
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


@pytest.mark.parametrize("K", [2, 15])
@pytest.mark.parametrize("name,d", [("mask24", 24), ("sm1024", 1024), ("sm8", 4096)])
def test_printed_bytes_decode_as_the_public_header_says(driver_output, name, d, K):
    N = 3
    line = next(l for l in driver_output.stdout.splitlines() if l.startswith(f"{name} K={K} "))
    raw = np.array([int(b, 16) for b in line.split()[2:]], np.uint8)
    want = digits_of(coef(np.arange(N * d), K).reshape(N, d), K)
    assert np.abs(want).any(axis=(1, 2)).all()  # every plane has digits: nothing passes by being zero
    assert np.array_equal(decode_planes(raw, d, K, N), want)
