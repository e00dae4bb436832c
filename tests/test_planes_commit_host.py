"""The from-planes front ends of lf_dev_commit_planes on the CPU, through the headers the kernels
use (latticeum_amd/csrc/digitpack.hpp, fragpos.hpp): a stand-alone program built with the
address and undefined-behaviour sanitizers packs seeded coefficients into buffers of exactly
the public sizes and then reads them as the front ends' threads do -- k_decompose_pow2<.., PL>'s
thread (j, t) its words (e, t + q T), k_decompose_phi72_w<28>'s lane its (plane, element) mask,
the d = 1024 and d = 4096 kernels their words and bytes -- for every unit at W = 1, 16, 17, 33.
Any index outside a buffer is a sanitizer error; every digit read is compared with the
schoolbook digit sign(x) bit_k(|x|), and the operand rows planes_row gives are checked to be
distinct, below 32, and to put plane 0 in the row before plane 1's."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

DRIVER = r"""
#include "digitpack.hpp"
#include <cstdio>
#include <vector>
using namespace lfk;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { if (fails < 20) printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)
static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int digit(int64_t x, int k) { const int b = (int)(((x < 0 ? -x : x) >> k) & 1); return x < 0 ? -b : b; }
static std::vector<int64_t> coeffs(size_t n) {
  std::vector<int64_t> x(n);
  for (auto &v : x) v = (int64_t)(rnd() % 32769) - 16384;
  x[0] = 16384, x[n - 1] = -16384;
  return x;
}
constexpr int K = 15, L = 5;

// k_decompose_pow2<D, NT, true>: block = unit G, thread (j, t) of 16 T, limb l, word q
static void pow2(int d, size_t W) {
  const size_t N = W * L, nG = frag_groups(W);
  const int T = d / 4 < 64 ? d / 4 : 64, PH = d / T / 2, H = d / 2;
  const auto x = coeffs(N * d);
  std::vector<uint32_t> words(N * smp2_words(d));
  for (size_t e = 0; e < N; e++)
    for (int i = 0; i < H; i++) words.at(smp2_word(e, d, i)) = smp2_make(x[e * d + i], x[e * d + i + H]);
  std::vector<int> seen(N * d, 0);
  for (size_t G = 0; G < nG; G++)
    for (int j = 0; j < 16; j++)
      for (int t = 0; t < T; t++) {
        const size_t g = 16 * G + j;
        if (g >= W) continue;  // ok == false: the thread holds zero words and loads nothing
        for (int l = 0; l < L; l++)
          for (int q = 0; q < PH; q++) {
            const size_t e = g * L + l;
            const int i = t + q * T;
            const uint32_t w = words.at(smp2_word(e, d, i));
            for (int k = 0; k < K; k++) {
              CHECK(sm16_digit(w, k) == digit(x[e * d + i], k));
              CHECK(sm16_digit(w >> 16, k) == digit(x[e * d + i + H], k));
              CHECK(smp2_digit(words.data(), e, d, i, k) == digit(x[e * d + i], k));
            }
            seen[e * d + i]++, seen[e * d + i + H]++;
          }
      }
  for (int s : seen) CHECK(s == 1);  // every coefficient is owned by exactly one thread
}

// k_decompose_phi72_w<28>: wave = (side, G, pass), lane 16 kq + gi = plane 4 pass + kq of group 16 G + gi
static void phi72(size_t W) {
  const size_t N = W * L, nblk = (W + 15) / 16;
  const int npass = (K + 3) / 4;
  const auto x = coeffs(N * 24);
  std::vector<uint64_t> masks(mask24_elems(K, N), 0);
  for (int k = 0; k < K; k++)
    for (size_t e = 0; e < N; e++) {
      uint32_t nz = 0, ng = 0;
      for (int i = 0; i < 24; i++) mask24_put(sign_mag16(x[e * 24 + i]), k, i, nz, ng);
      masks.at(mask24_index(k, N, e)) = nz | ((uint64_t)ng << 32) | 0xFF000000FF000000ull;  // junk above bit 23
    }
  std::vector<int> seen(masks.size(), 0);
  for (size_t task = 0; task < nblk * npass; task++)
    for (int lane = 0; lane < 64; lane++) {
      const int pass = (int)(task % npass), kq = lane >> 4, gi = lane & 15, k = 4 * pass + kq;
      const size_t G = task / npass, g = 16 * G + gi;
      if (g >= W || k >= K) continue;
      for (int l = L - 1; l >= 0; l--) {
        const uint64_t m = masks.at(mask24_index(k, N, g * L + l));
        const uint32_t nz = (uint32_t)m & 0xFFFFFFu, ng = (uint32_t)(m >> 32) & nz;  // as the kernel cleans them
        for (int i = 0; i < 24; i++) CHECK(mask24_digit(nz, ng, i) == digit(x[(g * L + l) * 24 + i], k));
        seen[mask24_index(k, N, g * L + l)]++;
      }
    }
  for (int s : seen) CHECK(s == 1);
}

// d = 1024 (k_decompose_fused): half-wave lane r of group g reads words (q < 16, r) of element g L + l;
// d = 4096 (k_decompose_n4k_*): lane r reads the 8 words (32 bytes) of plane kb of that element
static void big(size_t W) {
  const size_t N = W * L;
  {
    const auto x = coeffs(N * 1024);
    std::vector<uint32_t> words(N * SM1024_WORDS);
    for (size_t e = 0; e < N; e++)
      for (int q = 0; q < 16; q++)
        for (int r = 0; r < 32; r++)
          words.at(sm1024_word(e, q, r)) = sign_mag16(x[e * 1024 + r + 64 * q]) | sign_mag16(x[e * 1024 + r + 64 * q + 32]) << 16;
    for (size_t e = 0; e < N; e++)
      for (int j = 0; j < 1024; j += 37)
        for (int k = 0; k < K; k++) CHECK(sm1024_digit(words.data(), e, j, k) == digit(x[e * 1024 + j], k));
  }
  {
    const size_t Nq = W;  // one limb per group is enough for the byte indices
    const auto x = coeffs(Nq * 4096);
    std::vector<uint32_t> sm8(Nq * sm8_words(K), 0);
    uint8_t *by = reinterpret_cast<uint8_t *>(sm8.data());
    for (size_t e = 0; e < Nq; e++)
      for (int k = 0; k < K; k++)
        for (int a = 0; a < 1024; a++) {
          uint32_t nib = 0, sg = 0;
          for (int b = 0; b < 4; b++) {
            const int64_t v = x[e * 4096 + a + 1024 * b];
            nib |= (uint32_t)(digit(v, k) != 0) << b, sg |= (uint32_t)(v < 0) << b;
          }
          CHECK(sm8_byte_of(e, K, k, a) < sm8.size() * 4);
          by[sm8_byte_of(e, K, k, a)] = (uint8_t)sm8_make(nib, sg);
        }
    for (size_t e = 0; e < Nq; e++)
      for (int k = 0; k < K; k++)
        for (int r = 0; r < 32; r++)
          for (int j4 = 0; j4 < 8; j4++) {
            const uint32_t w = sm8.at(sm8_word(e, K, k, r, j4));
            for (int jj = 0; jj < 4; jj++)
              for (int b = 0; b < 4; b++)
                CHECK(sm8_digit((w >> (8 * jj)) & 0xFFu, b) == digit(x[e * 4096 + r + 32 * (4 * j4 + jj) + 1024 * b], k));
          }
  }
}

static void rows() {
  CHECK(planes_all_packed(1, 1) && planes_all_packed(3, 2));
  CHECK(!planes_all_packed(0, 1) && !planes_all_packed(0, 2) && !planes_all_packed(2, 2) && !planes_all_packed(1, 2));
  CHECK(!planes_all_packed(3, 1) && !planes_all_packed(7, 3) && !planes_all_packed(0, 0));
  for (int Kk = 1; Kk <= 15; Kk++) {
    uint32_t mask = 0;
    for (int s = 0; s < 2; s++) {
      CHECK(planes_row(s, Kk, 0) == planes_row(s, Kk, 1) - 1);
      for (int k = 0; k < Kk; k++) {
        const int r = planes_row(s, Kk, k);
        CHECK(r >= 0 && r < 32 && !((mask >> r) & 1u));
        mask |= 1u << r;
      }
    }
    CHECK(mask == (Kk == 16 ? 0xFFFFFFFFu : (1u << (2 * Kk)) - 1));
  }
}

int main() {
  rows();
  for (size_t W : {1, 16, 17, 33}) {
    for (int d : {16, 32, 64, 128, 256, 512}) pow2(d, W);
    phi72(W);
  }
  big(1);
  big(3);
  printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails != 0;
}
"""


def test_front_end_reads_under_sanitizers():
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "pc.cpp", Path(td) / "pc"
        src.write_text(DRIVER)
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{ROOT / 'latticeum_amd/csrc'}", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
