"""The index helpers of the coefficient-form fold at d = 16 .. 512 (latticeum_amd/csrc/
foldpow2.hpp) on the CPU: a stand-alone program built with the address and
undefined-behaviour sanitizers fills a challenge's byte table through the header's
positions into a buffer of exactly fp2_tab_bytes, reads every lane's 20 table bytes (the 5
dwords the kernel loads) and 16 packed words of every (row tile, column tile) through the
header's offsets -- any index outside either buffer is a sanitizer error -- and sums the
lane products into the negacyclic product, which it compares with the schoolbook sum."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

DRIVER = r"""
#include "foldpow2.hpp"
#include <cstdio>
#include <vector>
using namespace lfk;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)
static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int digit(int64_t x, int k) { const int b = (int)(((x < 0 ? -x : x) >> k) & 1); return x < 0 ? -b : b; }

static void check_degree(int d) {
  const int K = 15, N = 3;
  std::vector<int64_t> rho(d), x((size_t)N * d);
  for (auto &r : rho) r = (int64_t)(rnd() % 255) - 127;
  rho[0] = 127, rho[d - 1] = -127;
  for (auto &v : x) v = (int64_t)(rnd() % 32769) - 16384;
  std::vector<int8_t> tab(fp2_tab_bytes(d), 0);
  for (int c = 0; c < d; c++) {
    tab[fp2_tab_pos_plus(d, c)] = (int8_t)rho[c];
    if (c > 0) tab[fp2_tab_pos_minus(d, c)] = (int8_t)-rho[c];
  }
  for (int delta = -(d - 1); delta < d; delta++)
    CHECK(tab[fp2_tab_pos(d, delta)] == (delta >= 0 ? rho[delta] : -rho[delta + d]));
  std::vector<uint32_t> words((size_t)N * smp2_words(d));
  for (int e = 0; e < N; e++)
    for (int j = 0; j < d / 2; j++) words[smp2_word(e, d, j)] = smp2_make(x[(size_t)e * d + j], x[(size_t)e * d + j + d / 2]);
  CHECK(fp2_rows_per_wave(d) * fp2_waves_per_tile(d) == fp2_row_tiles(d) && fp2_waves_per_tile(d) * fp2_tiles_per_block(d) == 4);
  for (int k : {0, 7, 14}) {
    // plane k of element e as the lanes read it, summed into rows c
    for (int e = 0; e < N; e++) {
      std::vector<int64_t> got(d, 0), want(d, 0);
      for (int c = 0; c < d; c++)
        for (int j = 0; j < d; j++) want[c] += (c >= j ? rho[c - j] : -rho[c - j + d]) * digit(x[(size_t)e * d + j], k);
      if (d == 16) {
        for (int lane = 0; lane < 16; lane++) {  // h = 0: the first witness of the pair
          const int o = fp2_a_offset16(lane);
          CHECK(o >= 1 && (o & ~3) + 20 <= fp2_tab_bytes(d));
          for (int z = 0; z < 20; z++) (void)tab[(o & ~3) + z];  // the 5 dwords
          for (int xx = 0; xx < 16; xx++) {
            const uint32_t w = words[smp2_word(e, d, xx & 7)];
            got[lane] += (int64_t)tab[o + xx] * (int8_t)fp2_digit_byte(xx < 8 ? w : w >> 16, k);
          }
        }
      } else {
        for (int t = 0; t < fp2_row_tiles(d); t++)
          for (int q = 0; q < fp2_row_tiles(d); q++)
            for (int lane = 0; lane < 64; lane++) {
              const int o = fp2_a_offset(d, lane, t, q);
              CHECK(o >= 1 && (o & ~3) + 20 <= fp2_tab_bytes(d));
              for (int z = 0; z < 20; z++) (void)tab[(o & ~3) + z];
              const int w0 = fp2_b_word(d, lane, q), half = fp2_b_half(d, lane, q);
              CHECK(w0 % 16 == 0 && w0 + 16 <= d / 2);
              for (int xx = 0; xx < 16; xx++) {
                const int j = 32 * q + 16 * (lane >> 5) + xx;
                CHECK(smp2_word_of(e, d, j) == smp2_word(e, d, w0 + xx) && smp2_half_of(d, j) == half);
                const uint32_t w = words[smp2_word(e, d, w0 + xx)] >> (16 * half);
                got[32 * t + (lane & 31)] += (int64_t)tab[o + xx] * (int8_t)fp2_digit_byte(w, k);
              }
            }
      }
      for (int c = 0; c < d; c++) CHECK(got[c] == want[c]);
    }
  }
  for (int lane = 0; lane < 64; lane++)
    for (int i = 0; i < 16; i++) CHECK(fp2_acc_row(lane, i) >= 0 && fp2_acc_row(lane, i) < 32);
  for (int ks_n : {1, 2, 3, 5, 6, 10, 15, 30}) {
    CHECK(fp2_split_begin(30, 0, ks_n) == 0 && fp2_split_begin(30, ks_n, ks_n) == 30);
    for (int ks = 0; ks < ks_n; ks++) CHECK(fp2_split_begin(30, ks, ks_n) < fp2_split_begin(30, ks + 1, ks_n));
  }
}

int main() {
  for (int d : {16, 32, 64, 128, 256, 512}) check_degree(d);
  printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails != 0;
}
"""


def test_helpers_under_sanitizers():
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "fp2.cpp", Path(td) / "fp2"
        src.write_text(DRIVER)
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{ROOT / 'latticeum_amd/csrc'}", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
