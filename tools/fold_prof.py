"""fold() at the zkvm's shape (bench.py next_rows' CCS and fold_prove_line) on its
own, for rocprofv3 kernel traces of lf_fold_prove: `python tools/fold_prof.py [--scalar]`
prints the line bench.py reports as next_rows.fold_prove (with --scalar:
next_rows.fold_prove_scalar, the same rows with scalar values as the zkvm's).
`--lean`: the same fold() on the row prover (lf_prover_create) and on the lean prover
(lf_prover_create_lean), alternating in one process, `--rounds R` timed calls each (default
9): one JSON line with ms per call (median, min, max), the lf_prover_timing span sums of a
further timed call each, both provers' lf_prover_device_bytes, and whether the two gave
the same outputs."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def row_against_lean(LA, torch, ctx, M, S, d, n, rounds):
    """fold_prove_line's setup with both kinds of prover on the one scheme and CCS"""
    l, kappa, deg = 4, 32, 7
    W = n - l - 1
    pr = LA.goldilocks_dp(d)
    N = W * pr.L
    i64 = dict(dtype=torch.int64, device="cuda:0")
    A = torch.empty(kappa * N * d, **i64)
    ctx.dev_fill_uniform(A, bench.SEED_A)
    sch = LA.AjtaiCommitmentScheme(ctx, device_tensor=A, kappa=kappa, ncols=N, d=d)
    del A
    rng = np.random.default_rng(0x4C460018)
    c = rng.integers(0, 1 << 62, len(S) * d, dtype=np.uint64)
    provers = {"row": LA.Prover(ctx, sch, pr, M, l, deg, c, S), "lean": LA.Prover(ctx, sch, pr, M, l, deg, c, S, lean=True)}

    def wit(seed):
        w = {"w_ccs": torch.empty(W * d, **i64), "f": torch.empty(N * d, **i64), "f_coeff": torch.empty(N * d, **i64)}
        ctx.dev_fill_uniform(w["w_ccs"], seed)
        ctx.check(ctx.lib.lf_dev_witness_from_w_ccs(ctx.h, LA._lib.C.byref(pr), w["w_ccs"].data_ptr(), W,
                                                    w["f_coeff"].data_ptr(), w["f"].data_ptr()))
        cm = torch.empty(kappa * d, **i64)
        ctx.dev_ajtai_commit(sch, [w["f"]], cm)
        return rng.integers(0, 1 << 62, l * d, dtype=np.uint64), w, cm.cpu().numpy().view(np.uint64)

    xa, wa, cma = wit(bench.SEED_ACC)
    xi, wi, cmi = wit(bench.SEED_W)
    acc, _ = provers["row"].linearize(cma, xa, wa)
    outs = {k: {"w_ccs": torch.empty(W * d, **i64), "f": torch.empty(N * d, **i64), "f_coeff": torch.empty(N * d, **i64)}
            for k in provers}
    times = {k: [] for k in provers}
    res = {}
    for r in range(rounds + 1):  # round 0 warms both up
        for k, p in provers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = p.fold_prove(acc, wa, cmi, xi, wi, outs[k])
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(res["row"][0][f], res["lean"][0][f]) for f in res["row"][0])
    for f, v in res["row"][1].items():
        for a, b in zip(v, res["lean"][1][f]) if isinstance(v, list) else [(v, res["lean"][1][f])]:
            same = same and np.array_equal(a, b)
    same = same and all(torch.equal(outs["row"][f], outs["lean"][f]) for f in outs["row"])
    spans = {}
    for k, p in provers.items():
        p.timing(True)
        p.fold_prove(acc, wa, cmi, xi, wi, outs[k])
        spans[k] = p.timing(False)
    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    return {"workload": f"zkvm fold() (lf_fold_prove), row prover against lean prover, alternating: Phi_72, W={W}, "
                        f"N={N}, K={pr.K}, kappa={kappa}, {rounds} calls each",
            "ms_per_fold_prove": {k: stat(v) for k, v in times.items()}, "ms_all": times, "span_ms": spans,
            "device_bytes": {k: p.device_bytes for k, p in provers.items()}, "outputs_equal": bool(same)}


def main():
    import torch
    import latticeum_amd as LA
    torch.cuda.set_device(0)
    ctx = LA.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d, nv, t, mm, nn = 24, 17, 125, 1 << 17, 19768
    i64 = dict(dtype=torch.int64, device="cuda:0")
    rng = np.random.default_rng(0x4C460014)
    S = [list(rng.integers(0, 125, 7)) for _ in range(16)] + [list(rng.integers(0, 125, 1 + (i % 2))) for i in range(36)]
    S = [[int(j) for j in x] for x in S]
    rng = np.random.default_rng(0x4C460012)
    mats, nnz = [], 0
    for j in range(t):
        cnt = rng.integers(0, 3, mm)
        rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        mats.append([rp, rng.integers(0, nn, int(rp[-1])).astype(np.uint32), None])
        nnz += int(rp[-1])
    if "--scalar" in sys.argv:
        sv = torch.empty(nnz, **i64)
        ctx.dev_fill_uniform(sv, 0x4C460019)
        hv = np.zeros((nnz, d), np.uint64)
        hv[:, ::3] = sv.cpu().numpy().view(np.uint64)[:, None]
        hv = hv.ravel()
    else:
        vals = torch.empty(nnz * d, **i64)
        ctx.dev_fill_uniform(vals, 0x4C460013)
        hv = vals.cpu().numpy().view(np.uint64)
    off = 0
    for mt in mats:
        k = int(mt[0][-1])
        mt[2] = hv[off * d:(off + k) * d]
        off += k
    M = LA.CCSMatrices(ctx, d, mm, nn, mats)
    if "--lean" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 9
        out = row_against_lean(LA, torch, ctx, M, S, d, nn, rounds)
    else:
        out = bench.fold_prove_line(LA, torch, ctx, M, S, d, nn, t, mm)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
