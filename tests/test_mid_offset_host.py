"""Host checks of gl::mul_mid3_off (latticeum_amd/csrc/gl.hpp): the d = 1024 fused
decomposition's middle-factor product with both sums offset by C = 2^61, folded without sign
handling, and the constant that the offsets leave behind stage 2. A stand-alone program with
its own main, built from gl.hpp with ROCm's clang++ once plain and once with
-fsanitize=address,undefined, and run directly. It checks against 128-bit integer arithmetic
and prints one line per failure; the test asserts that there is none and that every case ran.

  value   mul_mid3_off(G, lo, hi) == (sum_g G_g (lo_g + 2^32 hi_g) + MID3_OFF) mod p, canonical,
          and for limbs from gl::mid_limbs(m) (or row j1 = 0's constants, m = 1) that is
          (Y m + MID3_OFF) mod p with Y = sum_t 2^(8t) D_t
  bounds  0 < X', H' < 2^62 and t = X' + (H' >> 32) (2^32 - 1) < 2^63 (no carry), on every case
  cases   m: all 32 x 32 middle factors psi^((2 m1 + 1) j1) of the real table (row 0 as the
          kernel forms it) and the edge values of tests/test_mid_lazy_host.py, each with D = 0,
          all 256 sign patterns of D_t = +-2^12 and (edge m) one entry +-2^12; random D with
          random m; the limbs at INT32_MIN / INT32_MAX in all 64 combinations with the groups at
          their extremes in all 8 sign patterns and at zero
  DFT     MID3_OFF = (C + 2^32 C) mod p; sum_j1 w32^(m2 j1) MID3_OFF = MID3_OFF32 at m2 = 0 and 0
          elsewhere (w32 = 2^78, a plain 32-point sum: ntt32.hpp's cyc_dif32 is device code),
          and for random y the sums of y + MID3_OFF less MID3_OFF32 at m2 = 0 are those of y
Skipped where that compiler is absent."""
import os
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

DRIVER = r"""
#include "gl.hpp"
#include <cstdio>
#include <cstdlib>
#include <climits>
typedef __int128 i128;
typedef unsigned __int128 u128;
static const i128 P = (i128)gl::P;
static unsigned long long s = 0x4F4646u;
static unsigned long long nxt() {  // SplitMix64
  unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static i128 modp(i128 x) {
  x %= P;
  return x < 0 ? x + P : x;
}
static i128 mulp(i128 a, i128 b) { return (i128)((u128)modp(a) * (u128)modp(b) % (u128)gl::P); }
static long fails = 0, value_cases = 0, m_cases = 0, dft_cases = 0;
static void fail(const char *what, unsigned long long m, const int32_t *G, const int32_t *lo, const int32_t *hi) {
  if (fails++ < 20) {
    printf("FAIL %s m=%llu", what, m);
    if (G) printf(" G %d %d %d lo %d %d %d hi %d %d %d", G[0], G[1], G[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    printf("\n");
  }
}
// the value against the limbs' own integer sum, and every bound of the derivation
static i128 check_value(const int32_t *G, const int32_t *lo, const int32_t *hi, unsigned long long m) {
  i128 X = 0, H = 0;
  for (int g = 0; g < 3; g++) X += (i128)G[g] * lo[g], H += (i128)G[g] * hi[g];
  const i128 C = (i128)gl::MID3_C, Xo = X + C, Ho = H + C, lim = (i128)1 << 62;
  if (!(Xo > 0 && Xo < lim && Ho > 0 && Ho < lim)) fail("bound X' H'", m, G, lo, hi);
  const i128 t = Xo + (Ho >> 32) * (i128)gl::EPS;
  if (!(t < ((i128)1 << 63))) fail("bound t", m, G, lo, hi);
  const i128 want = modp(X + H * ((i128)1 << 32) + (i128)gl::MID3_OFF);
  const unsigned long long got = gl::mul_mid3_off(G, lo, hi);
  if (got >= gl::P) fail("canonical", m, G, lo, hi);
  if ((i128)got != want) fail("value", m, G, lo, hi);
  value_cases++;
  return want;
}
// byte sums D with the factor m: the limbs of mid_limbs, or (row0) the kernel's constants for m = 1
static void check_m(const int *D, unsigned long long m, bool row0) {
  const int32_t G[3] = {D[0] + D[1] * 256 + D[2] * 65536, D[3] + D[4] * 256 + D[5] * 65536, D[6] + D[7] * 256};
  int32_t lo[3], hi[3];
  for (int g = 0; g < 3; g++) {
    gl::mid_limbs(m, g, lo[g], hi[g]);
    if (row0) lo[g] = g == 1 ? 1 << 24 : g == 0, hi[g] = g == 2 ? 1 << 16 : 0;
  }
  i128 Y = 0;
  for (int t = 7; t >= 0; t--) Y = Y * 256 + D[t];
  const i128 want = modp(mulp(Y, (i128)(m % gl::P)) + (i128)gl::MID3_OFF);
  if (check_value(G, lo, hi, m) != want) fail("Y m + off", m, G, lo, hi);
  m_cases++;
}
static void sign_patterns(unsigned long long m, bool row0) {
  int D[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  check_m(D, m, row0);
  for (int pat = 0; pat < 256; pat++) {
    for (int t = 0; t < 8; t++) D[t] = (pat >> t) & 1 ? -4096 : 4096;
    check_m(D, m, row0);
  }
}
// X[m2] = sum_j1 w32^(m2 j1) x[j1]
static void dft32(const i128 *x, i128 *X) {
  const i128 w32 = (i128)gl::mul_pow2(1, 78);
  for (int m2 = 0; m2 < 32; m2++) {
    i128 acc = 0, w = 1;
    const i128 wm = (i128)gl::pow((uint64_t)w32, (uint64_t)m2);
    for (int j = 0; j < 32; j++) acc = modp(acc + mulp(w, x[j])), w = mulp(w, wm);
    X[m2] = acc;
  }
}
int main(int argc, char **argv) {
  const unsigned long long p = gl::P;
  const unsigned long long edge[] = {0, 1, p - 1, (p - 1) / 2, (p + 1) / 2, 0xFFFFFFFFull, 1ull << 32, 1ull << 63,
                                     p - (1ull << 32)};
  const int n_rand = atoi(argv[1]);
  // the real table: psi^((2 m1 + 1) j1), psi the 2048th root of lf_api.hip (psi^32 = 2^39)
  const unsigned long long psi = gl::pow(7, (p - 1) / 2048);
  if (gl::pow(psi, 32) != gl::mul_pow2(1, 39)) fail("psi", psi, nullptr, nullptr, nullptr);
  for (int j1 = 0; j1 < 32; j1++)
    for (int m1 = 0; m1 < 32; m1++) sign_patterns(gl::pow(psi, (uint64_t)(2 * m1 + 1) * j1), j1 == 0);
  for (unsigned long long m : edge) {
    sign_patterns(m, false);
    for (int t = 0; t < 8; t++)
      for (int sg = -1; sg <= 1; sg += 2) {
        int D[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        D[t] = sg * 4096;
        check_m(D, m, false);
      }
  }
  for (int i = 0; i < n_rand; i++) {
    int D[8];
    for (int t = 0; t < 8; t++) D[t] = (int)(nxt() % 8193) - 4096;
    check_m(D, nxt(), false);
  }
  // the limbs at their extremes (mid_limbs stays inside them), the groups at theirs and at zero
  const int32_t gmax[3] = {4096 * (1 + 256 + 65536), 4096 * (1 + 256 + 65536), 4096 * (1 + 256)};
  for (int lp = 0; lp < 64; lp++) {
    int32_t lo[3], hi[3];
    for (int g = 0; g < 3; g++) lo[g] = (lp >> g) & 1 ? INT_MIN : INT_MAX, hi[g] = (lp >> (3 + g)) & 1 ? INT_MIN : INT_MAX;
    for (int gp = 0; gp < 9; gp++) {
      int32_t G[3];
      for (int g = 0; g < 3; g++) G[g] = gp == 8 ? 0 : (gp >> g) & 1 ? -gmax[g] : gmax[g];
      check_value(G, lo, hi, 0);
    }
  }
  // the constants, and what stage 2 makes of 32 equal offsets
  const i128 C = (i128)gl::MID3_C;
  if (modp(C + C * ((i128)1 << 32)) != (i128)gl::MID3_OFF) fail("MID3_OFF", 0, nullptr, nullptr, nullptr);
  i128 x[32], X[32], y[32], Y[32];
  for (int j = 0; j < 32; j++) x[j] = (i128)gl::MID3_OFF;
  dft32(x, X);
  for (int m2 = 0; m2 < 32; m2++, dft_cases++)
    if (X[m2] != (m2 == 0 ? (i128)gl::MID3_OFF32 : 0)) fail("dft of the offsets", m2, nullptr, nullptr, nullptr);
  for (int rep = 0; rep < 8; rep++) {
    for (int j = 0; j < 32; j++) y[j] = (i128)(nxt() % p), x[j] = modp(y[j] + (i128)gl::MID3_OFF);
    dft32(y, Y);
    dft32(x, X);
    X[0] = (i128)gl::sub((uint64_t)X[0], gl::MID3_OFF32);
    for (int m2 = 0; m2 < 32; m2++, dft_cases++)
      if (X[m2] != Y[m2]) fail("dft corrected", m2, nullptr, nullptr, nullptr);
  }
  printf("value %ld m %ld dft %ld fails %ld\n", value_cases, m_cases, dft_cases, fails);
  return fails ? 1 : 0;
}
"""

N_RAND = 1_000_000
N_EDGE = 9
N_M = (1024 + N_EDGE) * 257 + N_EDGE * 16 + N_RAND


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_mul_mid3_off_matches_integers(sanitize):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "off.cpp", Path(td) / "off"
        src.write_text(DRIVER)
        r = subprocess.run([CLANG, "-O2", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            f"-I{ROOT / 'latticeum_amd/csrc'}", "-x", "c++", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"host build of gl.hpp failed: {r.stderr[-600:]}"
        out = subprocess.run([str(exe), str(N_RAND)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    last = out.stdout.strip().split("\n")[-1].split()
    assert last == ["value", str(N_M + 64 * 9), "m", str(N_M), "dft", str(32 + 8 * 32), "fails", "0"], out.stdout[-600:]
