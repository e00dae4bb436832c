"""The contraction's launch time with a dense accumulator (what a chain's later
steps fold: after a real fold every digit plane of the accumulator is live, so
the top-limb class keeps 18 rows per step instead of the 7 of bench.py's
fresh-witness-shaped accumulator).

Builds bench.py's Workload, overwrites the shared acc_f_coeff in place with
coefficients uniform in [-2^14 + 1, 2^14 - 1] (acc_cm is left as it was: no launch
time depends on its values), runs batches the way bench.py's phase pass does
(every context on one stream, so the phases do not overlap) and prints the
`ajtai` phase time per batched launch from the contexts' own counters, `reps`
times. LATTICEUM_AMD_TOPCLASS=0 in the environment gives the single-class figure.

usage: python tools/dense_acc_ajtai.py [--d 1024 --w 16384 --kappa 32 --streams 8 --batches 2 --reps 3]"""
import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

import bench  # noqa: E402
import latticeum_amd as LA  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--w", type=int, default=1 << 14)
    ap.add_argument("--kappa", type=int, default=32)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--batches", type=int, default=2, help="batched launches per repetition")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bench-acc", action="store_true", help="keep bench.py's accumulator (for comparison)")
    args = ap.parse_args()
    S = args.streams
    wl = bench.Workload(LA, torch, 0, 0, args.d, args.w, args.kappa, S, batch=S)
    if not args.bench_acc:
        acc = wl.keeps[0]["acc_f_coeff"]  # shared by every step stream
        g = torch.Generator(device=acc.device).manual_seed(1234)
        x = torch.randint(-(1 << 14) + 1, 1 << 14, acc.shape, dtype=torch.int64, device=acc.device, generator=g)
        # canonical residues as int64 bit patterns: p + x == x - 2^32 + 1 (mod 2^64) for x < 0
        acc.copy_(torch.where(x < 0, x - (1 << 32) + 1, x))
        del x
    base = torch.cuda.current_stream().cuda_stream
    for c in wl.ctxs:
        c.set_stream(base)
    torch.cuda.synchronize()
    wl.run(S)  # untimed: code object load, buffers
    wl.sync()
    nvec = 2 * (wl.pr.K - 1) + 1
    ms = []
    for _ in range(args.reps):
        wl.timing(True)
        wl.run(S * args.batches)
        wl.sync()
        t, cnt = wl.ctxs[0].kernel_stats(nvec)
        ms.append(round(t / max(cnt, 1) * S, 3))  # per launch of S steps
        wl.timing(False)
    print(json.dumps({"d": args.d, "W": args.w, "kappa": args.kappa, "steps_per_launch": S,
                      "accumulator": "bench" if args.bench_acc else "dense",
                      "topclass": os.environ.get("LATTICEUM_AMD_TOPCLASS", "1") != "0",
                      "ajtai_ms_per_launch": ms}))
    wl.close()


if __name__ == "__main__":
    main()
