"""Time the fused CCS relation check against the cheapest part of the route it replaces.

  check     lf_dev_ccs_check_relation, nz = 1, resid = NULL (one bit and a row out)
  mles_all  lf_dev_mz_mles of all t matrices, nz = 1: materialising every MLE(M_j z), what a
            host had to do first before this call existed (the products come after)
  mles_used lf_dev_mz_mles_sel of only the matrices the multisets name: the same entries
            the check reads, plus their MLE writes

at the zkvm's shape (d = 24, t = 125, m = 2^17, n = 19 768; the CCS of
tests/test_gpu_fold_prove.py::test_fold_prove_zkvm_dimensions), scalar-valued as the
zkvm's matrices are (--ring: ring-valued entries). The legs alternate over --rounds
rounds of --reps calls each, after a warm-up call of each; prints one JSON line with
each leg's median and range of the per-round means (ms).
usage: python tools/relation_bench.py [--rounds 7] [--reps 10] [--ring] [--small]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import latticeum_amd as LA  # noqa: E402
import nifs as N  # noqa: E402


def scalarise(ccs, d):
    """every entry replaced by the scalar in its first word (from_scalar)"""
    tb = N.tb(d)
    mats = []
    for rp, col, val in ccs.mats:
        v = np.zeros((col.size, d), np.uint64)
        v[:, ::tb] = val.reshape(-1, d)[:, :1]
        mats.append((rp, col, v.ravel()))
    return N.CCS(d=d, m=ccs.m, n=ccs.n, l=ccs.l, mats=mats, c=ccs.c, S=ccs.S, degree=ccs.degree)


def mean_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ring", action="store_true", help="ring-valued entries instead of scalars")
    ap.add_argument("--small", action="store_true", help="a small shape (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    d, W, l, t, deg = (24, 19763, 4, 125, 7) if not a.small else (24, 13, 4, 12, 3)
    pr = N.Params(d)
    ccs = N.satisfied_ccs_np(d, W, l, t, deg, 0x4C46, pr, extra_density=1 / 16)
    if not a.ring:
        ccs = scalarise(ccs, d)
    x, w = N.satisfying_z(ccs, W, 101)
    z = np.concatenate(list(x) + [N.one(d), w])
    nv = ccs.m.bit_length() - 1
    used = sorted({j for S_i in ccs.S for j in S_i})
    nnz = [int(rp[-1]) for rp, _, _ in ccs.mats]

    ctx = LA.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    M = LA.CCSMatrices(ctx, d, ccs.m, ccs.n, ccs.mats)
    M.set_structure(l, deg, np.concatenate(ccs.c), ccs.S)
    assert M.scalar != a.ring
    zd = torch.from_numpy(z.view(np.int64).copy()).cuda()
    out = torch.empty(t * (1 << nv) * d, dtype=torch.int64, device="cuda")
    legs = {"check": lambda: M.check_relation(zd),
            "mles_all": lambda: M.mz_mles(zd, 1, nv, out),
            "mles_used": lambda: M.mz_mles_sel(zd, used, nv, out)}
    assert M.check_relation(zd) == [-1], "the benchmark's z satisfies its CCS"
    for fn in legs.values():  # warm-up: every kernel of every leg loaded and run once
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(mean_ms(fn, a.reps))
    ctx.sync()
    res = {"d": d, "t": t, "m": ccs.m, "n": ccs.n, "scalar": not a.ring, "S": [len(S_i) for S_i in ccs.S],
           "nnz_all": sum(nnz), "nnz_used": sum(nnz[j] for j in used), "rounds": a.rounds, "reps": a.reps,
           "mles_all_bytes": t * (1 << nv) * d * 8}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
