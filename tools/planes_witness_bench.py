"""lf_dev_pack_planes, lf_dev_planes_witness and lf_dev_planes_check beside existing entries that move
the same input bytes, standalone: `--d D --w W` (default Phi_72, W = 19 763), one process per run.
  pack_planes     beside  lf_dev_witness_pack(bits = 16): f_coeff in, 2 bytes per coefficient out at the
                          sm16 formats (d = 24: 120 B against 48 B per element, d = 4096: K KiB against 8 KiB)
  planes_witness  beside  lf_dev_witness_unpack(bits = 16): f_coeff, f and w_ccs out
  planes_check    beside  lf_dev_linf_norm over the u64 f_coeff
The coefficients are seeded in (-2^14, 2^14). Each pair runs `--reps` (default 7) alternating calls
after a warm-up pair; device ms between stream events (the two synchronous entries include their
copy back). One JSON line: per entry the median [min, max], its algorithmic bytes (every input read
once, every output written once) and those bytes over the median as a fraction of 8 TB/s, and the
bytes lf_dev_planes_witness saves against lf_dev_expand_planes plus a recomposition of both sides."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
PEAK = 8e12  # bytes / s


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    import latticeum_amd as LA
    torch.cuda.set_device(0)
    ctx = LA.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d, W, reps = arg("--d", 24), arg("--w", 19763), arg("--reps", 7)
    pr = LA.goldilocks_dp(d)
    K, N = pr.K, W * pr.L
    n = N * d
    i64 = dict(dtype=torch.int64, device="cuda:0")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x4C46)
    x = torch.randint(-(1 << 14) + 1, 1 << 14, (n,), generator=gen, **i64)
    fc = torch.where(x < 0, x + (LA.P - (1 << 64)), x)  # p - |x| as a two's-complement word
    del x
    plen = LA.fold_step_planes_len(pr, N)
    planes, packed = torch.empty(plen, **i64), torch.empty(n // 4, **i64)
    out = {k: (torch.empty(n, **i64), torch.empty(n, **i64), torch.empty(W * d, **i64)) for k in ("planes", "packed")}
    seen = {}

    pairs = {
        "pack": (("pack_planes", lambda: ctx.dev_pack_planes(pr, fc, N, planes)),
                 ("witness_pack16", lambda: ctx.dev_witness_pack(d, fc, N, 16, packed))),
        "witness": (("planes_witness", lambda: ctx.dev_planes_witness(pr, planes, N, *out["planes"])),
                    ("witness_unpack16", lambda: ctx.dev_witness_unpack(pr, packed, 16, N, *out["packed"]))),
        "check": (("planes_check", lambda: seen.__setitem__("check", ctx.dev_planes_check(pr, planes, N))),
                  ("linf_norm", lambda: seen.__setitem__("linf", ctx.dev_linf_norm(fc)))),
    }
    outputs = 8 * (2 * n + W * d)
    nbytes = {"pack_planes": 8 * n + 8 * plen, "witness_pack16": 8 * n + 2 * n,
              "planes_witness": 8 * plen + outputs, "witness_unpack16": 2 * n + outputs,
              "planes_check": 8 * plen, "linf_norm": 8 * n}
    ms = {name: [] for pair in pairs.values() for name, _ in pair}
    for pair in pairs.values():
        for r in range(reps + 1):  # the first pair warms up
            for name, fn in pair:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ctx.sync()
                if r:
                    ms[name].append(e0.elapsed_time(e1))
    equal = all(torch.equal(a, b) for a, b in zip(out["planes"], out["packed"])) and torch.equal(out["planes"][0], fc)
    norm, fault, _ = seen["check"]

    def line(name):
        v = ms[name]
        med = float(np.median(v))
        return {"ms": {"median": med, "min": float(min(v)), "max": float(max(v))}, "bytes": nbytes[name],
                "fraction_of_8TBps": nbytes[name] / (med * 1e-3) / PEAK}

    print(json.dumps({
        "workload": f"packed planes <-> witness: d={d}, W={W}, N={N}, K={K}",
        "entries": {name: line(name) for name in ms},
        "outputs_equal": bool(equal), "norm_equal": norm == seen["linf"], "fault": fault,
        "rows_not_allocated_bytes_both_sides": 2 * 8 * K * N * d,
        "planes_bytes_one_side": 8 * plen,
    }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
