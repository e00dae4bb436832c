"""planes_witness.hpp on the CPU: the thread-to-word maps, the values and the canonical tests that
planes_witness.hip's kernels take from it, driven by a stand-alone program built with the address
and undefined-behaviour sanitizers and run directly. The program walks every unit of every kernel
as its threads do -- the d = 16 .. 512 / 1024 units of four words, the d = 24 block with its 16-bit
tile, the d = 4096 word units -- over buffers of exactly lf_fold_step_planes_len's words (K N at
d = 24, N d / 4 at d = 16 .. 512, 256 N at d = 1024, 128 K N at d = 4096), at N = 5, 35, 85, 300 and
K = 15 and 7. Any index outside a buffer is a sanitizer error; packed planes must come back as the
coefficients, be canonical, and every coefficient and word must be owned exactly once; on random
bytes canonical() must agree with the fixed point pack(value(bytes)) == bytes."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

DRIVER = r"""
#include "planes_witness.hpp"
#include <cstdio>
#include <vector>
using namespace lfk;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { if (fails < 20) printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)
static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static std::vector<int64_t> coeffs(size_t n, int K) {
  std::vector<int64_t> x(n);
  const int64_t top = ((int64_t)1 << K) - 1;
  for (auto &v : x) v = (int64_t)(rnd() % (uint64_t)(2 * top + 1)) - top;
  x[0] = top, x[1] = -top, x[n - 2] = -1, x[n - 1] = (int64_t)1 << (K - 1);
  return x;
}

// every half: the value is the digits' sum, and canonical means sign_mag16(value) gives the half back
static void halves(int K) {
  for (uint32_t h = 0; h < 65536; h++) {
    int32_t s = 0;
    for (int k = 0; k < K; k++) s += sm16_digit(h, k) * (1 << k);
    CHECK(sm16_value(h, K) == s);
    CHECK(sm16_canonical(h, K) == (sign_mag16(s) == h));
    CHECK(sm16_value(h | 0xABCD0000u, K) == s);  // bits above the half are ignored
  }
}

// k_pack_smp2 / k_pack_sm, then k_planes_sm16: thread u owns unit u
static void sm16(int d, size_t N, int K) {
  const auto x = coeffs(N * d, K);
  std::vector<uint64_t> planes(d == 1024 ? 256 * N : N * d / 4);  // lf_fold_step_planes_len
  uint32_t *words = reinterpret_cast<uint32_t *>(planes.data());
  const size_t nw = planes.size() * 2, nu = sm16_units(d, N);
  CHECK(nu * 4 == nw);
  std::vector<int> wseen(nw, 0), cseen(N * d, 0);
  for (size_t u = 0; u < nu; u++) {
    const Sm16Unit un = sm16_unit(d, u);
    CHECK(un.word % 4 == 0 && un.word + 3 < nw && un.lo % 4 == 0);
    for (int i = 0; i < 4; i++) {
      const size_t lo = un.e * d + un.lo + i, hi = lo + un.hoff;
      CHECK(hi < N * d);
      words[un.word + i] = sign_mag16(x.at(lo)) | sign_mag16(x.at(hi)) << 16;
      wseen.at(un.word + i)++, cseen.at(lo)++, cseen.at(hi)++;
    }
  }
  for (int s : wseen) CHECK(s == 1);
  for (int s : cseen) CHECK(s == 1);
  // the words are digitpack.hpp's
  for (size_t e = 0; e < N; e++)
    for (int i = 0; i < d; i += 3) {
      const uint32_t w = d == 1024 ? words[sm1024_word_of(e, i)] >> (16 * sm1024_half_of(i))
                                   : words[smp2_word_of(e, d, i)] >> (16 * smp2_half_of(d, i));
      CHECK((w & 0xFFFFu) == sign_mag16(x[e * d + i]));
    }
  for (size_t u = 0; u < nu; u++) {
    const Sm16Unit un = sm16_unit(d, u);
    for (int i = 0; i < 4; i++) {
      const uint32_t w = words[un.word + i];
      CHECK(sm16_value(w & 0xFFFFu, K) == x[un.e * d + un.lo + i]);
      CHECK(sm16_value(w >> 16, K) == x[un.e * d + un.lo + un.hoff + i]);
      CHECK(sm16_canonical(w & 0xFFFFu, K) && sm16_canonical(w >> 16, K));
    }
  }
}

// k_pack_mask24's block, then k_planes_mask24's
static void pack24_block(const std::vector<int64_t> &x, size_t N, int K, size_t blk, uint64_t *planes, size_t np) {
  std::vector<uint32_t> tile(PK24_ELEMS * PK24_STRIDE / 2, 0);
  uint16_t *half = reinterpret_cast<uint16_t *>(tile.data());
  const size_t e0 = blk * PK24_ELEMS, n = N * 24;
  for (int t = 0; t < PK24_ELEMS; t++)
    for (int q = 0; q < 24; q++) {
      const int o = t + q * PK24_ELEMS;
      const size_t g = e0 * 24 + o;
      if (g >= n) continue;
      CHECK((size_t)pk24_slot(o / 24, o % 24) < tile.size() * 2);
      half[pk24_slot(o / 24, o % 24)] = (uint16_t)sign_mag16(x.at(g));
    }
  for (int t = 0; t < PK24_ELEMS; t++) {
    const size_t e = e0 + t;
    if (e >= N) continue;
    uint32_t w[SM24_WORDS];
    for (int p = 0; p < (int)SM24_WORDS; p++) w[p] = tile.at(pk24_word(t, p));
    for (int k = 0; k < K; k++) {
      CHECK(mask24_index(k, N, e) < np);
      planes[mask24_index(k, N, e)] = mask24_make(w, k);
    }
  }
}
static void mask24(size_t N, int K) {
  const auto x = coeffs(N * 24, K);
  std::vector<uint64_t> planes(mask24_elems(K, N), ~0ull);  // K N: lf_fold_step_planes_len
  const size_t nblk = (N + PK24_ELEMS - 1) / PK24_ELEMS;
  for (size_t b = 0; b < nblk; b++) pack24_block(x, N, K, b, planes.data(), planes.size());
  for (size_t e = 0; e < N; e++) {
    Mask24Acc acc;
    acc.init();
    for (int k = 0; k < K; k++) {
      const uint64_t m = planes.at(mask24_index(k, N, e));
      CHECK(!(m & 0xFF000000FF000000ull));
      for (int i = 0; i < 24; i++) {
        const int64_t v = x[e * 24 + i];
        const int dg = (int)(((v < 0 ? -v : v) >> k) & 1) * (v < 0 ? -1 : 1);
        CHECK(mask24_digit((uint32_t)m, (uint32_t)(m >> 32), i) == dg);
      }
      acc.plane(m, k);
    }
    for (int i = 0; i < 24; i++) CHECK(acc.x[i] == x[e * 24 + i]);
    CHECK(acc.canonical());
  }
  // the values leave through the tile as 16-bit words: every |value| < 2^15 survives the round trip
  for (int32_t v : {-32767, -1, 0, 1, 32767}) CHECK((int32_t)(int16_t)(uint16_t)((uint32_t)v & 0xFFFFu) == v);
}
// random masks of one element over 3 planes on a few coefficients: canonical() is the fixed point
static void mask24_fixed_point() {
  const int K = 3;
  for (int it = 0; it < 20000; it++) {
    uint64_t m[K];
    Mask24Acc acc;
    acc.init();
    for (int k = 0; k < K; k++) {
      const uint64_t r = rnd();
      m[k] = (r & 0x3) | ((r >> 8 & 0x3) << 32) | ((r >> 16 & 1) << 23) | ((r >> 17 & 1) << 55);
      if ((r >> 20 & 63) == 0) m[k] |= 1ull << (24 + (r >> 32 & 7)) << (32 * (r >> 40 & 1));
      acc.plane(m[k], k);
    }
    uint32_t w[SM24_WORDS] = {};
    for (int i = 0; i < 24; i++) w[i >> 1] |= sign_mag16(acc.x[i]) << (16 * (i & 1));
    bool same = true;
    for (int k = 0; k < K; k++) same = same && mask24_make(w, k) == m[k];
    CHECK(acc.canonical() == same);
  }
}

// k_pack_sm8's bytes (through digitpack.hpp), then k_planes_sm8's units
static void sm8(size_t N, int K) {
  const auto x = coeffs(N * 4096, K);
  std::vector<uint64_t> planes(128 * (size_t)K * N, ~0ull);  // lf_fold_step_planes_len
  uint32_t *words = reinterpret_cast<uint32_t *>(planes.data());
  uint8_t *by = reinterpret_cast<uint8_t *>(planes.data());
  for (size_t e = 0; e < N; e++)
    for (int k = 0; k < K; k++)
      for (int a = 0; a < 1024; a++) {
        uint32_t nib = 0, sg = 0;
        for (int b = 0; b < 4; b++) {
          const int64_t v = x[e * 4096 + a + 1024 * b];
          nib |= (uint32_t)(((v < 0 ? -v : v) >> k) & 1) << b, sg |= (uint32_t)(v < 0) << b;
        }
        by[sm8_byte_of(e, K, k, a)] = (uint8_t)sm8_make(nib, sg);
      }
  std::vector<int> cseen(N * 4096, 0);
  CHECK(sm8_units(N) * (size_t)K == planes.size() * 2);
  for (size_t u = 0; u < sm8_units(N); u++) {
    const size_t e = sm8_unit_elem(u);
    const int r = sm8_unit_r(u), j4 = sm8_unit_j4(u);
    CHECK(e < N);
    Sm8Acc acc;
    acc.init();
    for (int k = 0; k < K; k++) {
      CHECK(sm8_word(e, K, k, r, j4) < planes.size() * 2);
      acc.plane(words[sm8_word(e, K, k, r, j4)], k);
    }
    for (int jj = 0; jj < 4; jj++)
      for (int b = 0; b < 4; b++) {
        const int i = sm8_unit_coeff(r, j4, jj, b);
        CHECK(i >= 0 && i < 4096);
        CHECK(acc.x[4 * jj + b] == x[e * 4096 + i]);
        cseen.at(e * 4096 + i)++;
      }
    CHECK(acc.canonical());
  }
  for (int s : cseen) CHECK(s == 1);
}
// random words over 3 planes: canonical() is the fixed point
static void sm8_fixed_point() {
  const int K = 3;
  for (int it = 0; it < 20000; it++) {
    uint32_t w[K];
    Sm8Acc acc;
    acc.init();
    const uint32_t sg = (uint32_t)rnd() & 0xF0F0F0F0u;
    for (int k = 0; k < K; k++) {
      const uint64_t r = rnd();
      w[k] = ((uint32_t)r & 0x0F0F0F0Fu) | sg;
      if ((r >> 32 & 7) == 0) w[k] ^= 0x10u << (r >> 40 & 31) % 28;  // now and then another sign
      acc.plane(w[k], k);
    }
    bool same = true;
    for (int k = 0; k < K; k++) {
      uint32_t q = 0;
      for (int jj = 0; jj < 4; jj++) {
        uint32_t nib = 0, s = 0;
        for (int b = 0; b < 4; b++) {
          const int32_t v = acc.x[4 * jj + b];
          nib |= (uint32_t)(((v < 0 ? -v : v) >> k) & 1) << b, s |= (uint32_t)(v < 0) << b;
        }
        q |= sm8_make(nib, s) << (8 * jj);
      }
      same = same && q == w[k];
    }
    CHECK(acc.canonical() == same);
  }
}

int main() {
  for (int K : {15, 7}) {
    halves(K);
    for (size_t N : {5, 35, 85, 300}) {
      for (int d : {16, 32, 64, 128, 256, 512}) sm16(d, N, K);
      mask24(N, K);
    }
    mask24(513, K);
    sm16(1024, 5, K);
    sm16(1024, 15, K);
    sm8(1, K);
    sm8(5, K);
  }
  mask24_fixed_point();
  sm8_fixed_point();
  printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails != 0;
}
"""


def test_planes_witness_header_under_sanitizers():
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "pw.cpp", Path(td) / "pw"
        src.write_text(DRIVER)
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{ROOT / 'latticeum_amd/csrc'}", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
