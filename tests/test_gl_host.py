"""Host checks of the field helpers in latticeum_amd/csrc/gl.hpp. First the one that has no
oracle counterpart: gl::from_x_y32, the exact reduction of X + Y 2^32 for signed
|X|, |Y| < 2^62 that the i8-MFMA epilogues end in (mz.hip k_zcomb_mfma), against
Python's integers -- random pairs over every magnitude and the edge values. Then every
primitive of the header on the directed vector sets of oracle/gl_model.py (the host
bodies, which differ from the device's in sub, mul_wide and cacc_mad). The
header is compiled for the host with ROCm's clang (its __builtin_addc); the tests
are skipped where that compiler is absent."""
import os
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
P = (1 << 64) - (1 << 32) + 1

DRIVER = r"""
#include "gl.hpp"
#include <cstdio>
#include <cstdlib>
static unsigned long long s = 0x4C46u;
static unsigned long long nxt() {  // SplitMix64
  unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static long long pick() {
  const int sh = (int)(nxt() % 63);  // magnitudes 0 .. 2^62 - 1
  const long long m = sh ? (long long)(nxt() >> (64 - sh)) : 0;
  return (nxt() & 1) ? -m : m;
}
int main(int argc, char **argv) {
  const long long L = (1ll << 62) - 1;
  const long long edge[] = {0, 1, -1, L, -L, 1ll << 32, -(1ll << 32), (1ll << 32) - 1, -((1ll << 32) - 1),
                            1ll << 48, -(1ll << 48), 0x7FFFFFFF, -0x80000000ll, 0xFFFFFFFF00000001ll >> 2};
  for (long long a : edge)
    for (long long b : edge) printf("%lld %lld %llu\n", a, b, (unsigned long long)gl::from_x_y32(a, b));
  const int n = atoi(argv[1]);
  for (int i = 0; i < n; i++) {
    const long long x = pick(), y = pick();
    printf("%lld %lld %llu\n", x, y, (unsigned long long)gl::from_x_y32(x, y));
  }
  return 0;
}
"""


def test_from_x_y32_matches_integers():
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "xy.cpp", Path(td) / "xy"
        src.write_text(DRIVER)
        r = subprocess.run([CLANG, "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            f"-I{ROOT / 'latticeum_amd/csrc'}", "-x", "c++", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip(f"host build of gl.hpp failed: {r.stderr[-300:]}")
        out = subprocess.run([str(exe), "200000"], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [ln.split() for ln in out if ln]
    assert len(rows) == 14 * 14 + 200000
    for x, y, v in rows:
        want = (int(x) + (int(y) << 32)) % P
        assert int(v) == want, (x, y, v)


# ---- every primitive of gl.hpp on the vector sets of oracle/gl_model.py: the host bodies
# that replay.cpp, transcript.cpp and the table builders use, against Python's integers
PROBE_DRIVER = r"""
#include "gl_probe.hpp"
#include <cstdio>
#include <vector>
// the vector file: per set a header {op, s, m, n} of u64, then n m w words of a, then (for
// two-operand ops) as many of b; one line of output per case
int main(int argc, char **argv) {
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t h[4];
  while (fread(h, 8, 4, f) == 4) {
    const int op = (int)h[0], s = (int)h[1], m = (int)h[2];
    const size_t n = h[3], w = glp::words(op), k = n * m * w;
    int slo, shi;
    glp::shift_range(op, slo, shi);
    if (op < 0 || op >= glp::OP_COUNT || s < slo || s >= shi || !glp::m_ok(op, m)) return 3;
    std::vector<uint64_t> a(k), b(glp::takes_b(op) ? k : 0), out(n * w);
    if (fread(a.data(), 8, k, f) != k || fread(b.data(), 8, b.size(), f) != b.size()) return 4;
    for (size_t i = 0; i < n; i++) {
      if (glp::is_const_shift(op))
        out[i] = glp::shift_host(op, a[i], s);
      else
        glp::elem(op, a.data(), b.data(), s, m, i, out.data());
      for (size_t j = 0; j < w; j++) printf(j + 1 < w ? "%llu " : "%llu\n", (unsigned long long)out[i * w + j]);
    }
  }
  return 0;
}
"""


def test_every_primitive_matches_integers_on_the_edge_vectors():
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    import numpy as np

    import gl_model as G
    sets = [(vs, want) for vs, want in zip(G.vector_sets(), G.expected()) if vs.op not in G.DEVICE_ONLY_OPS]
    with tempfile.TemporaryDirectory() as td:
        src, exe, vec = Path(td) / "probe.cpp", Path(td) / "probe", Path(td) / "vectors.bin"
        src.write_text(PROBE_DRIVER)
        r = subprocess.run([CLANG, "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            f"-I{ROOT / 'latticeum_amd/csrc'}", "-x", "c++", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"host build of gl_probe.hpp failed: {r.stderr[-600:]}"
        with open(vec, "wb") as f:
            for vs, _ in sets:
                np.array([G.OPS[vs.op], vs.s, vs.m, vs.n], np.uint64).tofile(f)
                np.array(vs.a, np.uint64).tofile(f)
                if vs.b is not None:
                    np.array(vs.b, np.uint64).tofile(f)
        out = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [ln.split() for ln in out if ln]
    assert len(rows) == sum(vs.n for vs, _ in sets)
    at = 0
    for vs, want in sets:
        for i, w in enumerate(want):
            got = [int(v) for v in rows[at + i]]
            if vs.op in G.WEAK_OPS:  # any u64 congruent to the value
                assert got[0] < 1 << 64 and got[0] % P == w, (vs.op, vs.s, vs.m, i, got, w)
            else:
                assert got == (list(w) if vs.w == 3 else [w]), (vs.op, vs.s, vs.m, i, got, w)
        at += vs.n
