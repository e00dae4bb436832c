"""The witness wire format's host side (include/lf.h, "witness wire format"):
lf_witness_packed_len at each width, for an unsupported d, and where the size wraps
size_t; lf_witness_wire_header on a valid header at each width and on every rejection
the format names, once each, with its code. The same inputs then go to the parser
compiled alone (latticeum_amd/csrc/witness_wire.hpp) under AddressSanitizer and UBSan,
each in an allocation of exactly its length, run as a child process. Host code only."""
import os
import shutil
import struct
import subprocess
import tempfile
from pathlib import Path

import pytest

from latticeum_amd import _lib, wire

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
OK, INVALID_ARG, UNSUPPORTED_RING, INCORRECT_LENGTH = 0, 1, 2, 7  # lf.h
RINGS = [24] + [1 << k for k in range(4, 13)]


def header(d, L, bits, N, magic=b"LFW1", reserved=0):
    return magic + struct.pack("<IIIQQ", d, L, bits, N, reserved)


def valid(d=24, L=5, bits=16, N=10):
    return header(d, L, bits, N) + bytes(N * d * bits // 8)


# name -> (bytes, status); the accepted ones also list (d, L, bits, N)
CASES = {
    "valid16": (valid(bits=16), OK, (24, 5, 16, 10)),
    "valid32": (valid(d=64, L=3, bits=32, N=6), OK, (64, 3, 32, 6)),
    "valid64": (valid(d=4096, L=1, bits=64, N=1), OK, (4096, 1, 64, 1)),
    "empty_witness": (valid(N=0), OK, (24, 5, 16, 0)),
    "len31": (valid()[:31], INCORRECT_LENGTH),
    "no_bytes": (b"", INCORRECT_LENGTH),
    "one_short": (valid()[:-1], INCORRECT_LENGTH),
    "one_long": (valid() + b"\0", INCORRECT_LENGTH),
    "size_wraps": (header(24, 1, 64, 1 << 61), INCORRECT_LENGTH),   # 2^61 * 192 wraps to 0: the bare header
    "size_wraps16": (header(16, 1, 16, 1 << 59) + bytes(5), INCORRECT_LENGTH),
    "magic": (header(24, 5, 16, 10, magic=b"LFW2") + bytes(480), INVALID_ARG),
    "bits8": (header(24, 5, 8, 10) + bytes(240), INVALID_ARG),
    "bits0": (header(24, 5, 0, 10), INVALID_ARG),
    "bits_high_word": (header(24, 5, 16 + (1 << 16), 10) + bytes(480), INVALID_ARG),
    "reserved": (header(24, 5, 16, 10, reserved=1) + bytes(480), INVALID_ARG),
    "L0": (header(24, 0, 16, 10) + bytes(480), INVALID_ARG),
    "N_not_multiple_of_L": (header(24, 5, 16, 11) + bytes(528), INVALID_ARG),
    "d48": (header(48, 5, 16, 10) + bytes(960), UNSUPPORTED_RING),
    "d8192": (header(8192, 1, 16, 1) + bytes(16384), UNSUPPORTED_RING),
    "d0": (header(0, 5, 16, 10), UNSUPPORTED_RING),
}


def test_packed_len():
    f = _lib.load().lf_witness_packed_len
    for d in RINGS:
        for N in (0, 1, 85, 98815):
            assert f(d, N, 16) == 2 * N * d and f(d, N, 32) == 4 * N * d and f(d, N, 64) == 8 * N * d
    for d in (0, 8, 48, 8192, -24):
        assert f(d, 85, 16) == 0
    for bits in (0, 8, 24, 128, -16):
        assert f(24, 85, bits) == 0
    for d in RINGS:
        for bits in (16, 32, 64):
            assert f(d, 1 << 61, bits) == 0
    # the largest N whose bytes, and the header before them, still fit
    top = ((1 << 64) - 1 - 32) // 48
    assert f(24, top, 16) == 48 * top and f(24, top + 1, 16) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_header(name):
    data, want = CASES[name][:2]
    if want == OK:
        d, L, bits, N = CASES[name][2]
        assert wire.witness_wire_header(data) == {"d": d, "L": L, "bits": bits, "N": N}
    else:
        with pytest.raises(wire.LfError) as e:
            wire.witness_wire_header(data)
        assert e.value.code == want


def test_header_null_outputs_and_null_input():
    lib = _lib.load()
    data = valid()
    assert lib.lf_witness_wire_header(data, len(data), None, None, None, None) == OK
    assert lib.lf_witness_wire_header(None, 64, None, None, None, None) == INVALID_ARG


DRIVER = r"""
#include "witness_wire.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
// lines of "name hexbytes" (hex "-" = no bytes): each input in an allocation of exactly its length
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *fp = fopen(argv[1], "r");
  if (!fp) return 2;
  static char name[64], hex[1 << 16];
  while (fscanf(fp, "%63s %65535s", name, hex) == 2) {
    const size_t n = hex[0] == '-' ? 0 : strlen(hex) / 2;
    uint8_t *buf = (uint8_t *)malloc(n ? n : 1);
    uint8_t *in = n ? buf : buf + 1;  // no bytes: a pointer one past the allocation
    for (size_t i = 0; i < n; i++) {
      unsigned v;
      sscanf(hex + 2 * i, "%2x", &v);
      buf[i] = (uint8_t)v;
    }
    int d = -1, L = -1, bits = -1;
    size_t N = (size_t)-1;
    const int rc = lfk::wire_parse_header(in, n, &d, &L, &bits, &N);
    printf("%s %d %d %d %d %zu\n", name, rc, d, L, bits, N);
    free(buf);
  }
  fclose(fp);
  // the sizes, where the product wraps
  size_t out = 1;
  if (lfk::wire_payload_len(4096, (uint64_t)1 << 61, 64, &out) || out != 1) return 3;
  if (!lfk::wire_payload_len(24, 85, 16, &out) || out != 85 * 48) return 3;
  printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver_lines():
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe, inp = Path(td) / "ww.cpp", Path(td) / "ww", Path(td) / "cases.txt"
        src.write_text(DRIVER)
        # the large valid case stays out of the text file's line limit
        inp.write_text("".join(f"{k} {v[0].hex() or '-'}\n" for k, v in sorted(CASES.items()) if len(v[0]) < 30000))
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{ROOT / 'latticeum_amd/csrc'}", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.stdout.splitlines() if " " in l}


def test_parser_alone_under_sanitizers(driver_lines):
    fed = [k for k, v in CASES.items() if len(v[0]) < 30000]
    assert sorted(driver_lines) == sorted(fed) and len(fed) >= len(CASES) - 1
    for name in fed:
        want = CASES[name][1]
        rc, d, L, bits, N = driver_lines[name]
        assert rc == want, name
        if want == OK:
            assert (d, L, bits, N) == CASES[name][2], name
        else:  # a rejected input leaves the outputs alone
            assert (d, L, bits) == (-1, -1, -1) and N == (1 << 64) - 1, name
