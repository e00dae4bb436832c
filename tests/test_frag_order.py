"""The contraction order's position map and the top class's list compaction
(latticeum_amd/csrc/fragpos.hpp), on the CPU: a stand-alone program built with the
address and undefined-behaviour sanitizers. The contraction forms copy addresses
from these integers, so they are checked before anything runs on a GPU."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

DRIVER = r"""
#include "fragpos.hpp"
#include <cstdio>
#include <vector>
using namespace lfk;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)

static void check_map(size_t nG, int L) {
  const size_t ptop = frag_ptop(nG, L), npos = frag_npos(nG, L);
  CHECK(npos % 2 == 0 && ptop % 2 == 0);
  if (L > 1) {
    CHECK(ptop >= nG * (L - 1) && ptop <= nG * (L - 1) + 1);
    CHECK(npos / 2 == ptop / 2 + (nG + 1) / 2);  // nch
  } else {
    CHECK(ptop == 0 && npos / 2 == (nG + 1) / 2);
  }
  std::vector<int> hit(npos, 0);
  for (size_t G = 0; G < nG; G++)
    for (int l = 0; l < L; l++) {
      const size_t p = frag_pos(G, l, L, ptop);
      CHECK(p < npos);
      if (p >= npos) continue;
      hit[p]++;
      CHECK((l == L - 1 && L > 1) == (L > 1 && p >= ptop));  // the top limbs, and only they, in the top region
      size_t G2;
      int l2;
      frag_unit(p, L, ptop, G2, l2);
      CHECK(G2 == G && l2 == l);
    }
  size_t pad = 0;
  for (size_t p = 0; p < npos; p++) {
    CHECK(hit[p] <= 1);
    if (!hit[p]) {  // padding: its inverse is past the last group (A is zero there)
      pad++;
      size_t G2;
      int l2;
      frag_unit(p, L, ptop, G2, l2);
      CHECK(G2 >= nG);
      CHECK(p == npos - 1 || (L > 1 && p == ptop - 1));
    }
  }
  CHECK(pad == npos - nG * L && pad <= 2);
}

static void check_compact() {
  uint32_t tbl[TOP_TBL_WORDS];
  for (auto &x : tbl) x = 0xFFFFFFFFu;
  {  // nothing live
    const uint32_t live[3] = {0, 0, 0};
    CHECK(top_compact(live, 3, 29, tbl) == 0 && tbl[0] == 0);
    for (int t = 0; t < 3; t++) CHECK(top_tile_entries(tbl[0], t, 3) == 0);
  }
  {  // 7 rows per step, 8 steps: 56 entries, 2 tiles, tiles straddle steps
    uint32_t live[8];
    for (int s = 0; s < 8; s++) live[s] = 0x1u | (0xFu << 1) | (0x3u << 15);  // rows 0, 1..4, 15, 16
    CHECK(top_compact(live, 8, 29, tbl) == 56 && tbl[0] == 56);
    const int rows[7] = {0, 1, 2, 3, 4, 15, 16};
    for (int i = 0; i < 56; i++) CHECK(tbl[1 + i] == (((uint32_t)(i / 7) << 8) | (uint32_t)rows[i % 7]));
    for (int i = 56; i < 64; i++) CHECK(tbl[1 + i] == 0);  // padding: (step 0, row 0)
    CHECK(tbl[1 + 64] == 0xFFFFFFFFu);                     // nothing written past the last tile
    CHECK(top_tile_entries(56, 0, 8) == 32 && top_tile_entries(56, 1, 8) == 24 && top_tile_entries(56, 2, 8) == 0);
  }
  {  // everything live: one full tile per step, never more tiles than steps
    uint32_t live[8];
    for (int s = 0; s < 8; s++) live[s] = 0xFFFFFFFFu;
    CHECK(top_compact(live, 8, 32, tbl) == 256);
    for (int i = 0; i < 256; i++) CHECK(tbl[1 + i] == (((uint32_t)(i / 32) << 8) | (uint32_t)(i % 32)));
    for (int t = 0; t < 8; t++) CHECK(top_tile_entries(256, t, 8) == 32);
    // rows at or past nvec are never listed, whatever the masks say
    CHECK(top_compact(live, 8, 29, tbl) == 8 * 29);
    for (int i = 0; i < 8 * 29; i++) CHECK(top_row(tbl[1 + i]) < 29);
  }
  {  // mixed: a dense step (18 rows), a sparse one, an empty one
    const uint32_t live[3] = {0x3FFFFu, (1u << 28) | 1u, 0};
    CHECK(top_compact(live, 3, 29, tbl) == 20);
    CHECK(tbl[1 + 17] == 17 && tbl[1 + 18] == (1u << 8) && tbl[1 + 19] == ((1u << 8) | 28));
  }
  // decoding clamps: a corrupt entry or count still names a row of the launch
  CHECK(top_step(0xFFFFFFFFu, 3) == 2 && top_row(0xFFFFFFFFu) == 31);
  CHECK(top_step((2u << 8) | 5, 8) == 2 && top_row((2u << 8) | 5) == 5);
  CHECK(top_tile_entries(0xFFFFFFFFu, 7, 8) == 32 && top_tile_entries(0xFFFFFFFFu, 1, 2) == 32);
  CHECK(top_tile_entries(33, 1, 8) == 1 && top_tile_entries(32, 1, 8) == 0);
}

int main() {
  const size_t nGs[] = {1, 2, 3, 64, 1024};
  for (size_t nG : nGs)
    for (int L : {1, 4, 5}) check_map(nG, L);
  // the headline: 1024 groups of 16, L = 5 -> 2048 + 512 chunks
  CHECK(frag_ptop(1024, 5) == 4096 && frag_npos(1024, 5) == 5120);
  check_compact();
  printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails != 0;
}
"""


def test_position_map_and_compaction_under_sanitizers():
    if not os.path.exists(CLANG) and not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    with tempfile.TemporaryDirectory() as td:
        src, exe = Path(td) / "fp.cpp", Path(td) / "fp"
        src.write_text(DRIVER)
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{ROOT / 'latticeum_amd/csrc'}", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
