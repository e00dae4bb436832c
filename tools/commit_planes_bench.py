"""lf_dev_commit_planes against the route it replaces, standalone: both sides' y_s[k] from the
packed planes in one call, against lf_dev_expand_planes (f_k only) of both sides followed by
lf_dev_ajtai_commit of the same 2K vectors. `--d D --w W --kappa KAPPA` (default: the zkvm's
fold() shape, Phi_72, W = 19 763, kappa = 32). The planes are random digits shaped like a
decomposed witness's (the top limb's planes 4 .. K-1 zero; `--dense 1`: every plane random); A is
seeded. Both routes' y are compared. One JSON line: device ms per call between stream events,
median [min, max] of `--reps` (default 7) alternating calls after a warm-up pair, the parts
lf_ctx_kernel_timing sees (the entry's front end and its contraction, the route's Ajtai launch),
and the bytes each route allocates beyond the planes, A and y."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def witness_planes(LA, pr, N, seed, dense):
    """one side's buffer of random digits; unless dense, elements g L + L - 1 (the top limb) keep
    planes 0 .. 3 only, as the balanced digits of a field element do"""
    rng = np.random.default_rng(seed)
    d, K, L = pr.d, pr.K, pr.L
    n = LA.fold_step_planes_len(pr, N)
    top = np.arange(N) % L == L - 1
    if d == 24:  # [K][N] u64: bit i nonzero, bit 32 + i negative (only where nonzero)
        nz = rng.integers(0, 1 << 24, n, dtype=np.uint64)
        m = (nz | ((rng.integers(0, 1 << 24, n, dtype=np.uint64) & nz) << np.uint64(32))).reshape(K, N)
        if not dense:
            m[4:, top] = 0
        return m.ravel()
    w = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if dense:
        return w
    if d == 4096:  # [N][K][1024] bytes: the low nibble holds the quad's digits
        by = w.view(np.uint8).reshape(N, K, 1024)
        by[np.ix_(top, np.arange(4, K))] &= 0xF0
        return w
    h = w.view(np.uint16).reshape(N, -1)  # a 16-bit sign|magnitude word per coefficient
    h[top] &= 0x800F
    return w


def main():
    import torch
    import latticeum_amd as LA
    torch.cuda.set_device(0)
    ctx = LA.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d, W, kappa, reps, dense = arg("--d", 24), arg("--w", 19763), arg("--kappa", 32), arg("--reps", 7), arg("--dense", 0)
    pr = LA.goldilocks_dp(d)
    K, N, kd = pr.K, W * pr.L, kappa * d
    i64 = dict(dtype=torch.int64, device="cuda:0")
    A = torch.empty(kappa * N * d, **i64)
    ctx.dev_fill_uniform(A, 0x4C460001)
    sch = LA.AjtaiCommitmentScheme(ctx, device_tensor=A, kappa=kappa, ncols=N, d=d)
    planes = [torch.from_numpy(witness_planes(LA, pr, N, 5 + s, dense).view(np.int64)).cuda() for s in range(2)]
    y = {k: [torch.zeros(K * kd, **i64) for _ in range(2)] for k in ("entry", "route")}
    ycat = torch.zeros(2 * K * kd, **i64)
    rows = [torch.empty(K * N * d, **i64) for _ in range(2)]  # the route's [K][N][d] u64 rows
    ctx.reserve(kappa, N, d, 2 * K)

    def entry():
        ctx.dev_commit_planes(sch, pr, planes, N, y["entry"])

    def route():
        for s in range(2):
            ctx.dev_expand_planes(pr, planes[s], N, None, rows[s])
        ctx.dev_ajtai_commit(sch, [rows[s][k * N * d:(k + 1) * N * d] for s in range(2) for k in range(K)], ycat)

    ctx.kernel_timing(True)
    ms = {"entry": [], "route": []}
    parts = {"entry_front_end": [], "entry_contraction": [], "route_ajtai": []}

    def stats():
        return ctx.phase_stats("decompose")[0], ctx.kernel_stats(2 * K)[0]

    for r in range(reps + 1):  # the first pair warms up
        for name, fn in (("entry", entry), ("route", route)):
            p0, a0 = stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ctx.sync()
            p1, a1 = stats()
            if r:
                ms[name].append(e0.elapsed_time(e1))
                if name == "entry":
                    parts["entry_front_end"].append(p1 - p0)
                    parts["entry_contraction"].append(a1 - a0)
                else:
                    parts["route_ajtai"].append(a1 - a0)
    for s in range(2):
        y["route"][s].copy_(ycat[s * K * kd:(s + 1) * K * kd])
    equal = all(torch.equal(y["entry"][s], y["route"][s]) for s in range(2))
    summary = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(json.dumps({
        "workload": f"y_s[k] of both sides from packed planes: d={d}, W={W}, N={N}, kappa={kappa}, K={K}, "
                    f"{'dense' if dense else 'witness-shaped'} planes",
        "ms_per_call": {k: summary(v) for k, v in ms.items()},
        "kernel_timing_ms": {k: summary(v) for k, v in parts.items()},
        "outputs_equal": bool(equal),
        "bytes_allocated": {"entry": "the context's operand rows only (shared with every step)",
                            "route_rows": 2 * 8 * K * N * d, "planes_both_sides": 2 * 8 * LA.fold_step_planes_len(pr, N)},
    }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
