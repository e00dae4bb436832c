"""Reading a folding proof back from its wire bytes: lf_lfproof_shape / lf_lfproof_deserialize
(wire.deserialize_lfproof), the inverse of lf_lfproof_serialize for the shape (CCS, parameters,
kappa) fixes. Round trips at Phi_72 and X^16 + 1 whose result lf_fold_verify accepts; every
truncation, every length field set to 0, expected + 1 and 2^64 - 1, a word >= p, trailing bytes
and a too small buffer are LF_ERR_INCORRECT_LENGTH. The same malformed inputs then go through
the parser compiled alone under AddressSanitizer and UBSan, each in an allocation of exactly
its length. Host code only."""
import ctypes as C
import functools
import os
import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import latticeum_amd as LA
import nifs as N
import oracle as O
from latticeum_amd import wire
from latticeum_amd._lib import LfCcsDesc, LfLfproofMut, load
from test_nifs_oracle import instance
from test_replay import acc_dict, flat, proof_dict
from test_verify import lcccs_dict

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
INCORRECT_LENGTH = 7  # lf.h LF_ERR_INCORRECT_LENGTH


class Shape:
    """the lengths an LFProof of (ccs, params, kappa) carries"""

    def __init__(self, ccs, pr, kappa):
        self.d, self.K, self.tau, self.t, self.l, self.kappa = ccs.d, pr.K, N.tb(ccs.d), ccs.t, ccs.l, kappa
        self.m, self.s, self.degree, self.q, self.b_small = ccs.m, ccs.s, ccs.degree, len(ccs.S), pr.b_small
        self.lin_evals, self.fold_evals = ccs.degree + 2, 2 * pr.b_small + 1

    def params(self):
        p = LA.goldilocks_dp(self.d)
        p.K, p.b_small = self.K, self.b_small
        return p

    def args(self):
        return self.params(), self.t, self.m, self.l, self.degree, self.q, self.kappa

    def length_fields(self):
        """(byte offset, value) of every u64 length of the layout, in wire order"""
        out, pos, w = [], 0, 8 * self.d

        def vec(n):
            nonlocal pos
            out.append((pos, n))
            pos += 8 + n * w

        def vecvec(outer, inner):
            nonlocal pos
            out.append((pos, outer))
            pos += 8
            for _ in range(outer):
                vec(inner)

        vecvec(self.s, self.lin_evals)
        vec(self.tau)
        vec(self.t)
        for _ in range(2):
            for inner in (self.t, self.tau, self.l + 1, self.kappa):
                vecvec(self.K, inner)
        vecvec(self.s, self.fold_evals)
        vecvec(2 * self.K, self.tau)
        vecvec(2 * self.K, self.t)
        return out, pos


def to_bytes(pf, sh, repr=wire.REPR_CANONICAL):
    """wire.serialize_lfproof of the flat proof dict (lf_lfproof_mut's buffers)"""
    dec = [{k: list(np.asarray(pf[k][s], np.uint64).reshape(sh.K, -1)) for k in ("u_s", "v_s", "x_s", "y_s")}
           for s in range(2)]
    th = list(np.asarray(pf["theta_s"], np.uint64).reshape(2 * sh.K, -1))
    et = list(np.asarray(pf["eta_s"], np.uint64).reshape(2 * sh.K, -1))
    return wire.serialize_lfproof(sh.d, pf["lin_sumcheck"], sh.s, sh.lin_evals, pf["lin_v"], pf["lin_u"], dec,
                                  pf["fold_sumcheck"], sh.s, sh.fold_evals, th, et, repr=repr)


@functools.lru_cache(maxsize=None)
def case(d):
    pr, ccs, A, kappa, acc, Wa, cmi, xi, Wi = instance(d)
    out, _, proof = N.fold_prove(ccs, A, kappa, acc, Wa, cmi, xi, Wi, pr)
    sh = Shape(ccs, pr, kappa)
    return ccs, acc, cmi, xi, out, proof_dict(proof), sh, to_bytes(proof_dict(proof), sh)


def same_proof(a, b):
    assert sorted(a) == sorted(b)
    for k, v in a.items():
        if isinstance(v, list):
            assert all(np.array_equal(x, y) for x, y in zip(v, b[k])) and len(v) == len(b[k]) == 2, k
        else:
            assert np.array_equal(v, b[k]), k


@pytest.mark.parametrize("d", [24, 16])
def test_round_trip_and_verify(d):
    ccs, acc, cmi, xi, out, pf, sh, data = case(d)
    fields, size = sh.length_fields()
    assert len(data) == size
    back = wire.deserialize_lfproof(data, *sh.args())
    same_proof(back, pf)
    assert to_bytes(back, sh) == data
    got = LA.fold_verify(sh.params(), ccs.t, ccs.m, ccs.l, ccs.degree, flat(ccs.c), ccs.S, sh.kappa, acc_dict(acc),
                         cmi, flat(xi), back)
    for k, v in lcccs_dict(out).items():
        assert np.array_equal(got[k], v), k
    # the Montgomery boundary: the same bytes either way
    mont = np.vectorize(O.to_mont, otypes=[np.uint64])
    backm = wire.deserialize_lfproof(data, *sh.args(), repr=wire.REPR_MONTGOMERY)
    same_proof(backm, {k: ([mont(x) for x in v] if isinstance(v, list) else mont(v)) for k, v in pf.items()})
    assert to_bytes(backm, sh, wire.REPR_MONTGOMERY) == data


def test_shape_counts():
    sh = case(16)[6]
    counts = (C.c_size_t * 14)()
    desc = LfCcsDesc(sh.t, sh.m, sh.l, sh.degree, sh.q, None, None, None)
    total = load().lf_lfproof_shape(C.byref(desc), C.byref(sh.params()), sh.kappa, C.byref(counts))
    K, t, tau, L1, ka = sh.K, sh.t, sh.tau, sh.l + 1, sh.kappa
    assert list(counts) == [sh.s * sh.lin_evals, tau, t, K * t, K * t, K * tau, K * tau, K * L1, K * L1, K * ka, K * ka,
                            sh.s * sh.fold_evals, 2 * K * tau, 2 * K * t]
    assert total == sum(counts)
    for bad in (dict(m=sh.m + 1), dict(d=48), dict(kappa=0), dict(t=0)):  # no shape: 0, and the wrapper raises
        a = dict(d=sh.d, t=sh.t, m=sh.m, l=sh.l, degree=sh.degree, q=sh.q, kappa=sh.kappa)
        a.update(bad)
        with pytest.raises(wire.LfError):
            wire.deserialize_lfproof(b"", LA.goldilocks_dp(a["d"]), a["t"], a["m"], a["l"], a["degree"], a["q"],
                                     a["kappa"])


class Parser:
    """lf_lfproof_deserialize on one buffer with the length given apart (no copy per call)"""

    def __init__(self, sh, data):
        self.lib, self.sh = load(), sh
        self.raw = np.frombuffer(bytes(data), np.uint8).copy()
        self.desc, self.pr = LfCcsDesc(sh.t, sh.m, sh.l, sh.degree, sh.q, None, None, None), sh.params()
        counts = (C.c_size_t * 14)()
        self.total = self.lib.lf_lfproof_shape(C.byref(self.desc), C.byref(self.pr), sh.kappa, C.byref(counts))
        self.buf = np.zeros(self.total * sh.d, np.uint64)
        self.out = LfLfproofMut()

    def __call__(self, length=None, buf_elems=None):
        return self.lib.lf_lfproof_deserialize(self.raw.ctypes.data, self.raw.size if length is None else length,
                                               C.byref(self.desc), C.byref(self.pr), self.sh.kappa, 0,
                                               self.buf.ctypes.data, self.buf.size if buf_elems is None else buf_elems,
                                               C.byref(self.out))


def test_every_truncation_is_rejected():
    sh, data = case(16)[6:]
    parse = Parser(sh, data)
    assert parse() == 0
    bad = [n for n in range(len(data)) if parse(n) != INCORRECT_LENGTH]
    assert not bad, bad[:10]


def test_every_length_field_is_checked():
    sh, data = case(16)[6:]
    fields, _ = sh.length_fields()
    assert len(fields) == 2 * (1 + sh.s) + 2 + 2 * 4 * (1 + sh.K) + 2 * (1 + 2 * sh.K)
    for off, n in fields:
        assert struct.unpack_from("<Q", data, off)[0] == n, off
        for v in (0, n + 1, (1 << 64) - 1):
            bad = bytearray(data)
            struct.pack_into("<Q", bad, off, v)
            assert Parser(sh, bad)() == INCORRECT_LENGTH, (off, n, v)
            if off == fields[0][0] or off == fields[-1][0]:  # and through the wrapper
                with pytest.raises(wire.LfError) as e:
                    wire.deserialize_lfproof(bytes(bad), *sh.args())
                assert e.value.code == INCORRECT_LENGTH


def test_noncanonical_word_trailing_bytes_and_small_buffer():
    sh, data = case(16)[6:]
    fields, size = sh.length_fields()
    first, last = fields[0][0] + 16, size - 8  # the first and the last word of the proof
    for off in (first, last):
        for v, ok in ((LA.P - 1, True), (LA.P, False), ((1 << 64) - 1, False)):
            bad = bytearray(data)
            struct.pack_into("<Q", bad, off, v)
            assert Parser(sh, bad)() == (0 if ok else INCORRECT_LENGTH), (off, v)
    for extra in (b"\0", bytes(8), data[:8]):
        assert Parser(sh, data + extra)() == INCORRECT_LENGTH
    parse = Parser(sh, data)
    assert parse(buf_elems=parse.total * sh.d - 1) == INCORRECT_LENGTH and parse(buf_elems=0) == INCORRECT_LENGTH
    assert parse() == 0
    with pytest.raises(wire.LfError) as e:
        wire.deserialize_lfproof(data + b"\0", *sh.args())
    assert e.value.code == INCORRECT_LENGTH


# ---- the parser alone under the sanitizers: serialize.cpp compiled as host C++ with a main that
# replays the truncations and the length corruptions, every input in a heap block of exactly its
# size, so a read past the bytes given is a report and a nonzero exit
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/lf.h"
static std::vector<unsigned char> slurp(const char *path) {
  std::vector<unsigned char> v;
  FILE *f = fopen(path, "rb");
  if (!f) exit(2);
  unsigned char b[4096];
  for (size_t n; (n = fread(b, 1, sizeof b, f)) > 0;) v.insert(v.end(), b, b + n);
  fclose(f);
  return v;
}
// argv: proof bytes, length fields ((offset, value) u64 pairs), d t m l degree K b_small kappa
int main(int argc, char **argv) {
  if (argc != 11) return 2;
  const std::vector<unsigned char> data = slurp(argv[1]), ff = slurp(argv[2]);
  lf_params pr{atoi(argv[3]), 1ull << 15, 5, strtoull(argv[9], 0, 10), atoi(argv[8])};
  lf_ccs_desc ccs{atoi(argv[4]), strtoull(argv[5], 0, 10), strtoull(argv[6], 0, 10), atoi(argv[7]), 2, 0, 0, 0};
  const size_t kappa = strtoull(argv[10], 0, 10);
  size_t counts[14];
  const size_t total = lf_lfproof_shape(&ccs, &pr, kappa, counts);
  if (!total) return 3;
  const size_t elems = total * pr.d;
  uint64_t *full = (uint64_t *)malloc(elems * 8), *small = (uint64_t *)malloc((elems - 1) * 8);
  auto parse = [&](const unsigned char *src, size_t len, size_t cap) {
    unsigned char *in = (unsigned char *)malloc(len ? len : 1);  // exactly the bytes given
    memcpy(in, src, len);
    lf_lfproof_mut out;
    const int rc = lf_lfproof_deserialize(in, len, &ccs, &pr, kappa, LF_REPR_CANONICAL, cap == elems ? full : small,
                                          cap, &out);
    free(in);
    return rc;
  };
  if (parse(data.data(), data.size(), elems) != LF_OK) return 4;
  for (size_t n = 0; n < data.size(); n++)
    if (parse(data.data(), n, elems) != LF_ERR_INCORRECT_LENGTH) {
      fprintf(stderr, "truncation %zu accepted\n", n);
      return 5;
    }
  std::vector<unsigned char> bad = data;
  for (size_t i = 0; i + 16 <= ff.size(); i += 16) {
    uint64_t off, n;
    memcpy(&off, &ff[i], 8);
    memcpy(&n, &ff[i + 8], 8);
    const uint64_t vals[3] = {0, n + 1, ~0ull};
    for (uint64_t v : vals) {
      memcpy(&bad[off], &v, 8);
      if (parse(bad.data(), bad.size(), elems) != LF_ERR_INCORRECT_LENGTH) {
        fprintf(stderr, "length %llu at %llu accepted\n", (unsigned long long)v, (unsigned long long)off);
        return 6;
      }
    }
    memcpy(&bad[off], &n, 8);
  }
  bad.push_back(0);
  if (parse(bad.data(), bad.size(), elems) != LF_ERR_INCORRECT_LENGTH) return 7;  // trailing byte
  if (parse(data.data(), data.size(), elems - 1) != LF_ERR_INCORRECT_LENGTH) return 8;  // small buf
  free(full);
  free(small);
  return 0;
}
"""


def test_parser_under_sanitizers():
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    sh, data = case(16)[6:]
    fields, _ = sh.length_fields()
    csrc = ROOT / "latticeum_amd/csrc"
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        src, exe = td / "parse.cpp", td / "parse"
        src.write_text(DRIVER.replace("../../include/lf.h", str(ROOT / "include/lf.h")))
        r = subprocess.run([CLANG, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{csrc}",
                            "-x", "c++", str(src), str(csrc / "serialize.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
        if r.returncode != 0 and "libclang_rt" in r.stderr:
            pytest.skip(f"the sanitizer runtimes are not installed: {r.stderr[-200:]}")
        assert r.returncode == 0, f"host build of serialize.cpp failed: {r.stderr[-600:]}"
        (td / "proof.bin").write_bytes(data)
        (td / "fields.bin").write_bytes(b"".join(struct.pack("<QQ", off, n) for off, n in fields))
        run = subprocess.run([str(exe), str(td / "proof.bin"), str(td / "fields.bin")] +
                             [str(x) for x in (sh.d, sh.t, sh.m, sh.l, sh.degree, sh.K, sh.b_small, sh.kappa)],
                             capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-800:])
