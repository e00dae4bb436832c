"""Time lf_memtree_audit beside lf_memtree_apply on the same chunk of memory ops.

One full internal chunk (lf_memtree_chunk() = 4096 ops, seeded, two writes in three)
at the zkvm's shape, 8192 pages x 256 words. Every round applies a fresh chunk to the
handle (apply: the timed call that makes the records) and then audits those records
from the root before the chunk (audit) and checks their openings alone (verify). All
three calls are synchronous, so the host clock around a call is its time. The audit
must accept (its answer is checked every round). Prints one JSON line with each leg's
median and range over --rounds rounds after one warm-up round, in milliseconds per call.
usage: python tools/memaudit_bench.py [--rounds 9] [--small]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
import numpy as np  # noqa: E402

import latticeum_amd as LA  # noqa: E402
import oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a small shape (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    pages, wpp = (8192, 256) if not a.small else (13, 4)
    k = LA.memtree_chunk()
    rng = np.random.default_rng(7)
    mem = (O.fill_uniform(pages * wpp, 7) % (1 << 32)).astype(np.uint32)
    ctx = LA.Context(0)
    tree = ctx.memtree(mem, pages, wpp)
    mirror = mem.copy()
    times = {"apply": [], "audit": [], "verify": []}
    for rnd in range(a.rounds + 1):  # round 0: every kernel loaded, the scratch at its final size
        ops = np.ascontiguousarray(np.stack([rng.integers(0, pages * wpp, k) << 2, rng.integers(0, 1 << 32, k),
                                             rng.integers(0, 3, k) > 0], 1).astype(np.uint32))
        old = np.zeros(k, np.uint32)
        for j, (addr, v, w) in enumerate(ops):
            old[j] = mirror[addr >> 2]
            if w:
                mirror[addr >> 2] = v
        start = tree.root().copy()
        t0 = time.perf_counter()
        roots, pgs, paths, index = tree.apply(ops)
        t1 = time.perf_counter()
        res = ctx.memtree_audit(pages, wpp, start, ops, old, roots, pgs, paths, index)
        t2 = time.perf_counter()
        bad = ctx.memtree_verify(pages, wpp, roots, pgs, paths, index)
        t3 = time.perf_counter()
        assert res == (-1, 0) and bad == -1, (res, bad)
        if rnd:
            for name, dt in (("apply", t1 - t0), ("audit", t2 - t1), ("verify", t3 - t2)):
                times[name].append(dt * 1e3)
    out = {"pages": pages, "words_per_page": wpp, "depth": tree.depth, "k": k, "rounds": a.rounds, "unit": "ms per call"}
    for name, v in times.items():
        out[name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    tree.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
