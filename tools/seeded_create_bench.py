#!/usr/bin/env python3
"""Creation time and memory of an Ajtai scheme: derived from a seed on the device
(lf_ajtai_create_seeded, both kinds) against filling a u64 matrix on the device and
wrapping it (lf_dev_fill_uniform, then lf_ajtai_create_device).

  python tools/seeded_create_bench.py [--d 1024 --kappa 32 --n 81920 --pairs 3]

The routes alternate within each round, in the order --order gives (a 21.5 GB allocation
that follows the release of another sometimes stalls for seconds in the runtime: which
route pays depends on its place in the round). One JSON line per measurement: wall ms of the
creation (the u64 tensor's allocation is outside the timed part; every route ends with a
stream synchronisation), torch's peak allocation during it (the u64 matrix; the scheme's
own buffers are not torch's), the scheme's lf_ajtai_device_bytes, their sum, and the
device's used memory after the creation with the scheme alive (hipMemGetInfo)."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

import latticeum_amd as LA  # noqa: E402


def used_bytes():
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--kappa", type=int, default=32)
    ap.add_argument("--n", type=int, default=81920)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--order", default="012", help="the routes' order within a round: a permutation of 012 "
                    "(0 seeded Poseidon2, 1 seeded SplitMix, 2 fill + create_device)")
    a = ap.parse_args()
    ctx = LA.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    routes = [("seeded_poseidon2", LA.AJTAI_SEED_POSEIDON2, [1, 2, 3, 4]),
              ("seeded_splitmix", LA.AJTAI_SEED_SPLITMIX, 11),
              ("fill_uniform_create_device", None, 11)]
    routes = [routes[int(ch)] for ch in a.order]
    for rnd in range(a.pairs):
        for name, kind, seed in routes:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = used_bytes()
            torch.cuda.reset_peak_memory_stats()
            At = None
            if kind is None:
                At = torch.empty(a.kappa * a.n * a.d, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind is None:
                ctx.dev_fill_uniform(At, seed)
                sch = LA.AjtaiCommitmentScheme(ctx, device_tensor=At, kappa=a.kappa, ncols=a.n, d=a.d)
            else:
                sch = LA.AjtaiCommitmentScheme.seeded(ctx, seed, kind, kappa=a.kappa, ncols=a.n, d=a.d)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            peak = torch.cuda.max_memory_allocated()
            print(json.dumps({"route": name, "round": rnd, "d": a.d, "kappa": a.kappa, "n": a.n,
                              "create_ms": round(ms, 2), "torch_peak_bytes": peak,
                              "scheme_device_bytes": sch.device_bytes,
                              "peak_plus_scheme_bytes": peak + sch.device_bytes,
                              "device_used_after_bytes": used_bytes() - base, "layout": sch.layout}), flush=True)
            del sch, At
    ctx.close()


if __name__ == "__main__":
    main()
