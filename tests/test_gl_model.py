"""The Python-integer model of gl.hpp (oracle/gl_model.py), without a GPU: its
transliterations equal plain % p on the whole vector set, and the branch census over
that set -- the one tests/test_gl_host.py and tests/test_gpu_gl.py run -- sees every
decision of every primitive both ways, or never where the module proves it cannot be
taken."""
import re
from pathlib import Path

import gl_model as G

ROOT = Path(__file__).resolve().parents[1]
P = (1 << 64) - (1 << 32) + 1


def test_op_codes_match_the_probe_header():
    txt = (ROOT / "latticeum_amd/csrc/gl_probe.hpp").read_text()
    enum = {m[1].lower(): int(m[2]) for m in re.finditer(r"\bOP_([A-Z0-9_]+) = (\d+)", txt)}
    assert enum.pop("count") == len(G.OPS)
    assert enum == G.OPS
    three = {c for op, c in G.OPS.items() if G.WORDS.get(op, 1) == 3}
    assert three == {c for c in G.OPS.values() if c == 18 or c >= 21}  # glp::words
    import latticeum_amd as LA
    assert set(LA.Context.GL_PROBE_3WORD) == three


def test_edge_set_holds_what_it_must():
    can, any64 = G.edge_values()
    assert can == sorted(set(can)) and any64 == sorted(set(any64))
    assert all(x < P for x in can) and all(x < 1 << 64 for x in any64)
    assert set(can) == {x for x in any64 if x < P}
    must = {0, 1, 2, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, P - 1, P - 2, P - 2**32, P - 2**32 + 1, (P + 1) // 2,
            (P - 1) // 2, 2**63, 2**63 + 1, 2**63 - 1, 0xFFFFFFFEFFFFFFFF, 0x00000001FFFFFFFF, 0xFFFF0000FFFF0000,
            0x7FFFFFFF80000000}
    for i in range(64):
        must |= {2**i, 2**i - 1, P - 2**i}
    assert must <= set(any64)
    assert {P, P + 1, 2**64 - 2, 2**64 - 1} <= set(any64) - set(can)
    assert G.edge_values() == (can, any64)


def test_vector_sets_cover_every_op_and_shift():
    sets = G.vector_sets()
    assert {vs.op for vs in sets} == set(G.OPS)
    for op in ("mul_pow2", "mul_pow2_rt", "shl96", "shl192", "shl_small_weak"):
        assert sorted(vs.s for vs in sets if vs.op == op) == list(G.shift_range(op))
    for op in ("acc_reduce", "acc_add", "cacc_reduce", "cacc_reduce_weak", "cacc_reduce_terms"):
        assert sorted(vs.m for vs in sets if vs.op == op) == list(G.RUN_LENGTHS)
    can, any64 = G.edge_values()
    n = {vs.op: vs.n for vs in sets}
    assert n["add"] == n["sub"] == len(can) ** 2 and n["mul"] == n["reduce128"] == len(any64) ** 2
    assert n["add_weak"] == len(any64) * len(can)


def test_transliterations_equal_the_integers():
    count, bad, _ = G.census()
    assert not bad, {op: v[:3] for op, v in bad.items()}
    assert all(count[op] > 0 for op in G.OPS)


def test_branch_census():
    _, _, flags = G.census()
    print(G.census_report())
    assert set(flags) == set(G.OPS) - set(G.DEVICE_ONLY_OPS)
    short, taken, seen = [], [], set()
    for op, fl in flags.items():
        assert fl, op
        for k, (st, cl) in fl.items():
            if G.unreachable(op, k):
                seen.add(("*", k) if ("*", k) in G.UNREACHABLE else (op, k))
                if st:
                    taken.append((op, k, st))
            elif st < G.CENSUS_MIN or cl < G.CENSUS_MIN:
                short.append((op, k, st, cl))
    assert not taken, taken
    assert not short, short
    # the table holds no entry the census never evaluated, and every entry carries its proof
    assert seen == set(G.UNREACHABLE)
    assert all(isinstance(v, str) and len(v) > 20 for v in G.UNREACHABLE.values())
    # the joint cases, by name
    for k in ("reduce128.carry=0,borrow=0", "reduce128.carry=0,borrow=1", "reduce128.carry=1,borrow=0"):
        assert flags["reduce128"][k][0] >= G.CENSUS_MIN and flags["mul"][k][0] >= G.CENSUS_MIN
    for v in (-1, 0, 1):
        assert flags["from_x_y32"][f"from_x_y32.c={v}"][0] >= G.CENSUS_MIN
        assert flags["from_x_y32"][f"from_x_y32.k={v}"][0] >= G.CENSUS_MIN
