"""Host checks of gl::mid_limbs and gl::mul_mid3 (latticeum_amd/csrc/gl.hpp): the middle
factors of the d = 1024 fused decomposition as three tables of signed 32-bit limb pairs, and
their product with the grouped byte sums of the matrix-core stage 1. A stand-alone program
with its own main, built from gl.hpp with ROCm's clang++ once plain and once with
-fsanitize=address,undefined, and run directly. It checks against 128-bit integer arithmetic
and prints one line per failure; the test asserts that there is none and that every case ran.
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
typedef __int128 i128;
typedef unsigned __int128 u128;
static const i128 P = (i128)gl::P;
static unsigned long long s = 0x4D4944u;
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
static long fails = 0, limb_cases = 0, mul_cases = 0, bound_cases = 0;
static void fail(const char *what, unsigned long long m, int g, const int *D) {
  if (fails++ < 20) {
    printf("FAIL %s m=%llu g=%d", what, m, g);
    if (D)
      for (int t = 0; t < 8; t++) printf(" %d", D[t]);
    printf("\n");
  }
}
// lo + 2^32 hi == 2^(24g) m (mod p) for the limbs as the int32_t they are returned in
static void check_limbs(unsigned long long m) {
  for (int g = 0; g < 3; g++) {
    int32_t lo = 0, hi = 0;
    gl::mid_limbs(m, g, lo, hi);
    const i128 got = modp((i128)lo + (i128)hi * ((i128)1 << 32));
    const i128 want = modp((i128)(u128)m << (24 * g));
    if (got != want) fail("mid_limbs", m, g, nullptr);
    limb_cases++;
  }
}
// mul_mid3 of the grouped sums against ((sum_t 2^(8t) D_t) m) mod p; bounds: |X|, |H| < 2^62
static void check_mul(const int *D, unsigned long long m, bool bounds) {
  const int32_t G[3] = {D[0] + D[1] * 256 + D[2] * 65536, D[3] + D[4] * 256 + D[5] * 65536, D[6] + D[7] * 256};
  int32_t lo[3], hi[3];
  for (int g = 0; g < 3; g++) gl::mid_limbs(m, g, lo[g], hi[g]);
  i128 Y = 0;
  for (int t = 7; t >= 0; t--) Y = Y * 256 + D[t];
  const i128 want = (i128)((u128)modp(Y) * (u128)(m % gl::P) % (u128)gl::P);
  const unsigned long long got = gl::mul_mid3(G, lo, hi);
  if ((i128)got != want) fail("mul_mid3", m, -1, D);
  mul_cases++;
  if (bounds) {
    i128 X = 0, H = 0;
    for (int g = 0; g < 3; g++) X += (i128)G[g] * lo[g], H += (i128)G[g] * hi[g];
    const i128 lim = (i128)1 << 62;
    if (!(X < lim && X > -lim && H < lim && H > -lim)) fail("bound", m, -1, D);
    bound_cases++;
  }
}
int main(int argc, char **argv) {
  const unsigned long long p = gl::P;
  const unsigned long long edge[] = {0, 1, p - 1, (p - 1) / 2, (p + 1) / 2, 0xFFFFFFFFull, 1ull << 32, 1ull << 63,
                                     p - (1ull << 32)};
  const int n_rand_m = atoi(argv[1]), n_rand_d = atoi(argv[2]);
  for (unsigned long long m : edge) check_limbs(m);
  for (int i = 0; i < n_rand_m; i++) check_limbs(nxt());
  // all 256 sign patterns of D_t = +-4096, times the edge m
  for (int pat = 0; pat < 256; pat++) {
    int D[8];
    for (int t = 0; t < 8; t++) D[t] = (pat >> t) & 1 ? -4096 : 4096;
    for (unsigned long long m : edge) check_mul(D, m, true);
  }
  // one entry +-4096, the rest 0
  for (int t = 0; t < 8; t++)
    for (int sg = -1; sg <= 1; sg += 2) {
      int D[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      D[t] = sg * 4096;
      for (unsigned long long m : edge) check_mul(D, m, true);
    }
  // random D in [-4096, 4096]^8 with random m
  for (int i = 0; i < n_rand_d; i++) {
    int D[8];
    for (int t = 0; t < 8; t++) D[t] = (int)(nxt() % 8193) - 4096;
    check_mul(D, nxt(), false);
  }
  printf("limbs %ld mul %ld bounds %ld fails %ld\n", limb_cases, mul_cases, bound_cases, fails);
  return fails ? 1 : 0;
}
"""

N_RAND_M, N_RAND_D = 100_000, 1_000_000
N_EDGE = 9


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_mid_limbs_and_mul_mid3_match_integers(sanitize):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "mid.cpp", Path(td) / "mid"
        src.write_text(DRIVER)
        r = subprocess.run([CLANG, "-O2", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            f"-I{ROOT / 'latticeum_amd/csrc'}", "-x", "c++", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"host build of gl.hpp failed: {r.stderr[-600:]}"
        out = subprocess.run([str(exe), str(N_RAND_M), str(N_RAND_D)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    last = out.stdout.strip().split("\n")[-1].split()
    assert last == ["limbs", str(3 * (N_EDGE + N_RAND_M)), "mul", str((256 + 16) * N_EDGE + N_RAND_D),
                    "bounds", str((256 + 16) * N_EDGE), "fails", "0"], out.stdout[-600:]
