"""Time the persistent memory tree against the route it replaces, per memory op.

  rebuild   what one op costs without the handle: upload the [pages][words] matrix as
            u64, lf_dev_merkle_tree, lf_merkle_open of the touched page (the host-side
            widening of the u32 words to u64 is left out of the timed window)
  apply1    lf_memtree_apply with k = 1
  apply1024 lf_memtree_apply with k = 1024, per op

at the zkvm's shape (8192 pages x 256 words, seeded ops, two writes in three). Every
leg ends in a device synchronise (lf_merkle_open and apply both do), so the host
clock around the calls is the call time. The legs alternate over --rounds rounds
after a warm-up call of each; prints one JSON line with each leg's median and range
of the per-round means, in microseconds per op.
usage: python tools/memtree_bench.py [--rounds 9] [--small]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import latticeum_amd as LA  # noqa: E402
import oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a small shape (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    pages, wpp, big = (8192, 256, 1024) if not a.small else (13, 4, 40)
    reps = {"rebuild": 10, "apply1": 2000, "apply1024": 50}  # calls per round: a fraction of a second each
    rng = np.random.default_rng(7)
    mem = (O.fill_uniform(pages * wpp, 7) % (1 << 32)).astype(np.uint32)

    def ops(k):
        return np.ascontiguousarray(np.stack([rng.integers(0, pages * wpp, k) << 2, rng.integers(0, 1 << 32, k),
                                              rng.integers(0, 3, k) > 0], 1).astype(np.uint32))

    ctx = LA.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    tree = ctx.memtree(mem, pages, wpp)
    depth = tree.depth
    wide = torch.from_numpy(mem.astype(np.uint64).view(np.int64))
    rows = torch.empty(pages * wpp, dtype=torch.int64, device="cuda")
    nodes = torch.empty(LA.merkle_nodes_len(pages) * 4, dtype=torch.int64, device="cuda")
    roots = np.zeros((big, 4), np.uint64)
    pgs = np.zeros((big, wpp), np.uint32)
    paths = np.zeros((big, depth, 4), np.uint64)
    index = np.zeros(big, np.uint32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)

    def rebuild(o):
        for addr, _, _ in o:
            rows.copy_(wide)
            ctx.dev_merkle_tree(rows, pages, wpp, nodes)
            ctx.merkle_open(nodes, pages, (int(addr) >> 2) // wpp)

    def apply1(o):
        for j in range(len(o)):
            ctx.check(ctx.lib.lf_memtree_apply(tree.h, ptr(o[j:]), 1, ptr(roots), ptr(pgs), ptr(paths), ptr(index)))

    def apply_big(o):
        for j in range(0, len(o), big):
            ctx.check(ctx.lib.lf_memtree_apply(tree.h, ptr(o[j:]), big, ptr(roots), ptr(pgs), ptr(paths), ptr(index)))

    legs = {"rebuild": (rebuild, 1), "apply1": (apply1, 1), "apply1024": (apply_big, big)}
    for name, (fn, k) in legs.items():  # warm-up: every kernel loaded, the scratch at its final size
        fn(ops(k))
    # the handle's tree is the tree of its own mirror after the warm-up's ops
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for name, (fn, k) in legs.items():
            o = ops(k * reps[name])
            t0 = time.perf_counter()
            fn(o)
            times[name].append((time.perf_counter() - t0) * 1e6 / len(o))
    res = {"pages": pages, "words_per_page": wpp, "depth": depth, "k_big": big, "rounds": a.rounds, "reps": reps,
           "unit": "us per op"}
    for k, v in times.items():
        res[k] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    tree.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
