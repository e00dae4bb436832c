"""The three f_hat-from-planes entries against their row entries, standalone, at the zkvm's
fold() shape (Phi_72, N = 98 815 elements, 2^17 points, K = 15) or `--d D --N N --nv NV`:
lf_dev_fhat_evaluate_planes / lf_dev_fhat_evaluate_eq, lf_dev_fhat_lincomb_planes /
lf_dev_fhat_lincomb_digits, lf_sumcheck_prove_fold_planes / lf_sumcheck_prove_fold_digits
(the whole sumcheck, host transcript included). The planes are random digits; the rows are
lf_dev_expand_planes of them, and every pair's outputs are compared. One JSON line: ms per
call, median [min, max] of `--reps` (default 7) alternating calls."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def random_planes(LA, pr, N, seed):
    """one side's buffer of random digits, every format (a coefficient's planes need not agree)"""
    rng = np.random.default_rng(seed)
    n = LA.fold_step_planes_len(pr, N)
    if pr.d == 24:  # bit i: nonzero, bit 32 + i: negative (only where nonzero)
        nz = rng.integers(0, 1 << 24, n, dtype=np.uint64)
        return nz | ((rng.integers(0, 1 << 24, n, dtype=np.uint64) & nz) << np.uint64(32))
    # d = 4096: any byte is a quad's four digits; the sign|magnitude words (K = 15): any 16 bits
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def main():
    import torch
    import latticeum_amd as LA
    torch.cuda.set_device(0)
    ctx = LA.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d, N, nv, reps = arg("--d", 24), arg("--N", 98815), arg("--nv", 17), arg("--reps", 7)
    pr = LA.goldilocks_dp(d)
    K, tau, n = pr.K, 3 if d == 24 else 1, 1 << nv
    i64 = dict(dtype=torch.int64, device="cuda:0")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    planes = [dev(random_planes(LA, pr, N, 5 + s)) for s in range(2)]
    rows = [torch.empty(K * N * d, **i64) for _ in range(2)]
    for s in range(2):
        ctx.dev_expand_planes(pr, planes[s], N, rows[s], None)

    def uniform(elems, seed):
        t = torch.empty(elems, **i64)
        ctx.dev_fill_uniform(t, seed)
        return t

    eq, coef, io0 = uniform(n * d, 11), uniform(K * tau * d, 12), uniform(n * d, 13)
    gen, mu = uniform(5 * n * d, 14), uniform(2 * K * d, 15)
    comb = LA.Comb.folding(mu, 2 * K, tau, 2)
    work = torch.empty((5 + 2 * K * tau) * max(n // 4, 1) * d, **i64)
    out = {k: torch.empty(K * tau * d, **i64) for k in ("planes", "rows")}
    io = {k: io0.clone() for k in out}
    proofs = {}

    def evaluate(k):
        if k == "planes":
            ctx.dev_fhat_evaluate_planes(pr, planes[0], N, nv, eq, out[k])
        else:
            ctx.dev_fhat_evaluate_eq(d, rows[0], N, N * d, K, nv, eq, out[k])

    def lincomb(k):
        if k == "planes":
            ctx.dev_fhat_lincomb_planes(pr, planes[0], N, nv, coef, io[k])
        else:
            ctx.dev_fhat_lincomb_digits(d, rows[0], N, N * d, K, nv, coef, io[k])

    def prove(k):
        T = LA.Poseidon2Transcript()
        if k == "planes":
            proofs[k] = ctx.sumcheck_prove_fold_planes(T, comb, gen, pr, planes[0], planes[1], N, nv, work)
        else:
            proofs[k] = ctx.sumcheck_prove_fold_digits(T, comb, gen, rows[0], rows[1], K, N, N * d, nv, d, work)

    res = {}
    for name, fn in (("evaluate", evaluate), ("lincomb", lincomb), ("prove_fold", prove)):
        ms = {"planes": [], "rows": []}
        for r in range(reps + 1):  # the first pair warms up
            for k in ms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(k)
                torch.cuda.synchronize()
                if r:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        res[name] = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in ms.items()}
    equal = (torch.equal(out["planes"], out["rows"]) and torch.equal(io["planes"], io["rows"])
             and all(np.array_equal(a, b) for a, b in zip(proofs["planes"], proofs["rows"])))
    print(json.dumps({"workload": f"f_hat from packed planes against the u64 rows: d={d}, N={N}, 2^{nv} points, K={K}",
                      "ms_per_call": res, "outputs_equal": bool(equal),
                      "bytes_per_side": {"planes": 8 * LA.fold_step_planes_len(pr, N), "rows": 8 * K * N * d}}),
          flush=True)


if __name__ == "__main__":
    main()
