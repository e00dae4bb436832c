"""Benchmark: LatticeFold commit + fold steps per second on MI355X.

A step = zkvm commit(z) (Witness::from_w_ccs + Ajtai A.f) followed by the
commit+fold arithmetic of fold(): decompose accumulator and new witness into
K=15 witnesses each, 28 batched Ajtai commitments, y_0 fix-ups, f_0 / cm_0 linear
fold with 30 short challenges, Witness::from_f(f_0). Inputs are synthetic
(seeded SplitMix64, SURVEY.md §8d seeds) and resident in HBM before timing.

Default workload (BASELINE.json configs[2], "Ajtai commit + single LatticeFold
step on 2^14 synthetic CCS witnesses", at the metric's d=1024): ring
Fq[X]/(X^1024+1), w_ccs = 2^14 ring elements, kappa = 32, B=2^15, L=5, K=15.

Each GPU runs `--streams` (default 8) independent step streams -- independent
witness / accumulator pairs, the trace-batch shard of BASELINE configs[3] --
and, with `--batch G` (default 8), every G of them are one
lf_dev_fold_step_batch call: each step's arithmetic on its own stream, their
Ajtai contractions one launch, so the 21.5 GB matrix A is read from HBM once
per G steps. Every step is complete; nothing is shared
but the read of A.

Multi-GPU (torchrun, one rank per GPU): `value` counts every rank's step
streams (weak scaling, no collective on the data path). At N > 1 the line also carries
`sharded_fold`: one fold column-sharded over all ranks, with an RCCL
all-reduce (mod p) of the partial commitments in every step, through the C
ABI's communicator (lf_dev_fold_step_sharded; latticeum_amd.dist).

A plain run (`--gpus 1 --steps N --warmup W`) sets the workload up, warms up,
times the N steps and prints the result line: `value` and `ms_per_step` and the
contract's other keys. `--dump-outputs DIR` also writes what the last timed step
computed as DIR/<name>.npy (dump_outputs), so two builds can be compared output
for output; the inputs are seeded, the same on every run.

With `--full` the line also reports (same run, each its own timed batch): the
per-phase HIP-event times and roofline of the headline workload, the CPU
baselines, the reference ring Phi_72 at the real zkvm shape (the path with
reference parity), the byte-equivalent d=1024 shape W=464, configs[4]'s d=4096
ring with kappa=64, the configs[1] NTT batch, batched Poseidon2, the sumcheck /
Mz / fold() rows, at N > 1 the sharded fold, and the detail file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

SEED_W = 0x4C460003
SEED_A = 0x4C460004
SEED_RHO = 0x4C460005
SEED_ACC = 0x4C460006
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
SHARDED_LIMIT_S = 240  # N > 1: the sharded fold's watchdog (main)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--w", type=int, default=1 << 14, help="w_ccs length W (ring elements)")
    ap.add_argument("--kappa", type=int, default=32)
    ap.add_argument("--streams", type=int, default=8,
                    help="concurrent step streams per GPU (independent witness / accumulator pairs)")
    ap.add_argument("--full", action="store_true", default=False,
                    help="beside the headline: the per-phase times and roofline (a timed pass of their own), the "
                         "CPU baselines, the other shapes and rings, the NTT / Poseidon2 / sumcheck / Mz / fold() "
                         "rows, at N > 1 the sharded fold, and the detail file; without it only the timed steps run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step to DIR/<name>.npy "
                         "(float64; dump_outputs)")
    ap.add_argument("--no-small-shape", dest="small", action="store_false", default=True,
                    help="with --full: skip the W=464 / d=24 multi-stream measurements and the NTT / Poseidon2 "
                         "timings reported beside the default workload")
    ap.add_argument("--cu-partition", action="store_true", default=False,
                    help="give each step stream its own contiguous block of CUs (lf_stream_create_cu_mask)")
    ap.add_argument("--cu-split", type=int, default=0,
                    help="N > 0 (batched groups): each group's contraction runs on a stream of the last N CUs "
                         "(lf_ctx_set_contract_stream) and the step streams on the others, so a group's "
                         "contraction runs beside the next group's decompositions")
    ap.add_argument("--packed", type=int, default=None,
                    help="1: keep the decomposed witnesses as packed digit planes (no u64 f_k / f_coeff_k rows); "
                         "0: write the rows; default: the ring's default (Workload)")
    ap.add_argument("--batch", type=int, default=8,
                    help="G > 1: the step streams form groups of G whose G steps' contractions run as one "
                         "launch (lf_dev_fold_step_batch: one pass over A for the group); 1: all streams")
    ap.add_argument("--cpu-baseline", dest="cpu", action="store_true", default=True)
    ap.add_argument("--no-cpu-baseline", dest="cpu", action="store_false")
    ap.add_argument("--detail", default=None,
                    help="file for the full record (every side workload and phase); the printed line is the compact "
                         "headline, which names this file. Default: DETAIL_DEFAULT with --full, none without")
    return ap.parse_args()


def algorithmic_bytes(d, W, kappa, L=5, K=15):
    """SURVEY.md 8(d)'s bytes/step (B1..B5) and the algorithmic bytes of one
    launch of each step phase: its inputs read once and its outputs written
    once in the Witness forms the reference materialises (u64 per residue).
    `operand` is what a phase moves on top of that because the contraction
    runs on the i8 matrix cores: the operand rows (offset form) the fused decompositions
    write (F bytes per element; Phi_72 has 40 Toom-3 virtual slots, F = 320 B
    against E = 192 B) and the larger operand form of A and the vectors."""
    E, N = 8 * d, W * L
    step = (E * (W + 3 * N + kappa * N + kappa) + 2 * E * (N + K * (2 * N + W))
            + E * (kappa * N + 2 * (K - 1) * N + 2 * (K - 1) * kappa) + E * (2 * K * N + N)
            + E * (2 * N + W))
    nvec = 2 * (K - 1) + 1  # commit(z)'s A.f rides in the decomposition-commitment pass
    F = 8 * (40 if d == 24 else d)
    fused = d in (24, 1024, 4096)  # the decompositions write planes 1..K-1 as operand rows
    alg = {
        # B2 (per side; phase_report scales by the sides one launch covers):
        # f_coeff in; f_k_coeff, f_k (K N each), w_ccs_k (K W) out
        "decompose": E * (N + 2 * K * N + K * W),
        # B3 + commit(z)'s A f: A once, the 29 vectors, the 29 kappa-element results
        "ajtai": E * (kappa * N + nvec * N + nvec * kappa),
        "fold": E * (2 * K * N + N),  # B4
        "from_w_ccs": E * (W + 2 * N),
        "from_f": E * (2 * N + W),  # B5
        "to_frag": E * N + F * N,  # commit(z)'s f into operand form (fused paths)
    }
    operand = {
        "decompose": F * (K - 1) * N if fused else 0,
        "ajtai": (F - E) * (kappa * N + nvec * N),
    }
    return step, alg, operand


def step_hbm(d, W, kappa, group, phases, value_per_gpu, L=5, K=15):
    """Step-level HBM figures beside SURVEY B1..B5 (which count A twice per step):
    the bytes the step needs when A is read once per `group` steps (one batched
    contraction launch), and the PMC-measured bytes summed over the step's kernels
    (traffic per launch x launches per step; null if any phase lacks a PMC figure)."""
    E, N = 8 * d, W * L
    survey, _, _ = algorithmic_bytes(d, W, kappa, L, K)
    needed = survey - 2 * E * kappa * N + E * kappa * N / max(1, group)
    tr = [p.get("traffic_bytes_per_launch") for p in phases.values()]
    pmc = None if not tr or any(t is None for t in tr) else \
        sum(p["traffic_bytes_per_launch"] * p["launches_per_step"] for p in phases.values())
    out = {"survey_bytes_per_step": survey, "survey_frac_hbm": survey * value_per_gpu / 1e9 / HBM_PEAK_GBS,
           "needed_bytes_per_step": needed, "steps_per_A_read": max(1, group),
           "needed_gbs": needed * value_per_gpu / 1e9, "needed_frac_hbm": needed * value_per_gpu / 1e9 / HBM_PEAK_GBS,
           "pmc_bytes_per_step": pmc}
    if pmc is not None:
        out["pmc_gbs"] = pmc * value_per_gpu / 1e9
        out["pmc_frac_hbm"] = out["pmc_gbs"] / HBM_PEAK_GBS
    return out


I8_DENSE_TOPS = 5000.0  # MI355X dense i8 MFMA peak (2x the dense bf16 2.5 PFLOP/s)


def coeff_fold(d, layout, keep_fk):
    """whether lf_dev_fold_step folds f_0 in coefficient form on the i8 matrix
    cores (fold_coeff.hip): X^1024+1 after the fused decomposition, f_k kept or
    the planes packed (not the operand-rows-only mode)"""
    return d == 1024 and layout == 1 and keep_fk


def kernel_names(LA, d, W, layout, keep_fk=True, packed=False):
    """the kernel each lf_dev_fold_step phase launches (for the rocprof / PMC joins)"""
    mfma = "k_ajtai_mfma_ra"  # the i8 contraction, A in registers (ajtai_mfma.hip)
    if d == 24:
        return {"decompose": "k_decompose_phi72_w", "ajtai": mfma if layout == 1 else "k_ajtai_phi72",
                "fold": "k_fold_coeff_phi72", "from_w_ccs": "k_from_w_ccs_phi72", "from_f": "k_from_f_phi72",
                "to_frag": "k_to_frag<true, true, true>"}
    if d == 1024:
        small = W < LA.witness_split_w()  # one half-wave per (element, limb) below this W
        cf = coeff_fold(d, layout, keep_fk)
        return {"decompose": "k_decompose_fused", "ajtai": mfma if layout == 1 else "k_ajtai_nega",
                "fold": "k_fold_coeff" if cf else "k_fold_nega" if keep_fk else "k_fold_frag",
                "from_w_ccs": "k_from_w_ccs_digits" if small else "k_from_w_ccs_n32",
                "from_f": ("k_from_fcoeff_split" if small else "k_from_fcoeff_n32") if cf
                else "k_from_f_split" if small else "k_from_f_n32",
                "to_frag": "k_to_frag<true, false, true>"}
    if d == 4096:  # packed planes fold f_0 from the operand rows
        # packed steps run the matrix-core stage 1 (k_decompose_n4k_mx) unless LATTICEUM_AMD_N4K=valu
        mx = packed and os.environ.get("LATTICEUM_AMD_N4K") != "valu"
        return {"decompose": ("k_decompose_n4k_mx" if mx else "k_decompose_n4k_fused") if layout == 1
                else "k_decompose_n4k",
                "ajtai": mfma if layout == 1 else "k_ajtai_nega",
                "fold": "k_fold_frag" if packed else "k_fold_nega", "from_w_ccs": "k_from_w_ccs_n4k",
                "from_f": "k_from_f_n4k",
                "to_frag": "k_to_frag<true, false, true>"}
    return {"decompose": "k_decompose_nega", "ajtai": mfma if layout == 1 else "k_ajtai_nega",
            "fold": "k_fold_nega", "from_w_ccs": "k_from_w_ccs_nega", "from_f": "k_from_f_nega",
            "to_frag": "k_to_frag"}


def by_base(t, kern):
    """look a templated kernel (k_decompose_fused<true>, k_ajtai_mfma_ra<0, 2, 4>)
    up by its plain name too: the instance the step launches most often (the
    workload setup launches other instances once, e.g. the accumulator's commit)"""
    bases = {}
    for k in t:
        base = k.split("<")[0]
        if base != k and base not in t:
            bases.setdefault(base, []).append(k)
    for base, ks in bases.items():
        t[base] = t[max(ks, key=lambda k: kern[k].get("launches", 0))]


def kernel_source_hash():
    """sha256 (12 hex digits) over the product's device and host sources
    (latticeum_amd/csrc): the PMC files carry the hash of the code they were
    collected on, and bench.py uses a file only while the sources still hash
    the same (no git on the GPU box, so not the revision)."""
    import hashlib
    h = hashlib.sha256()
    src = ROOT / "latticeum_amd" / "csrc"
    for p in sorted(src.iterdir()):
        if p.suffix in (".hip", ".hpp", ".cpp", ".inc", ".h"):
            h.update(p.name.encode())
            h.update(p.read_bytes())
    return h.hexdigest()[:12]


_PMC_STALE = set()


def _pmc_doc(kind, d, W, kappa, name=None, config=None):
    """profiles/pmc_<kind>_d<d>_W<W>_k<kappa>.json (or `name` with `config`) when it
    is this configuration's and was collected on the current kernel sources; None
    otherwise (a stale file is recorded in _PMC_STALE and reported as such, never
    paired with new timings)"""
    name = name or f"pmc_{kind}_d{d}_W{W}_k{kappa}.json"
    try:
        doc = json.loads((ROOT / "profiles" / name).read_text())
    except (OSError, ValueError):
        return None
    if doc.get("config") != (config or {"d": d, "W": W, "kappa": kappa}):
        return None
    if doc.get("src_hash") != kernel_source_hash():
        _PMC_STALE.add(name)
        return None
    return doc


def load_traffic(d, W, kappa):
    """PMC-measured HBM bytes per launch (profiles/pmc_traffic_d<d>_W<W>_k<kappa>.json, written by
    tools/prof_summary.py traffic from separate FETCH_SIZE / WRITE_SIZE passes of
    this same configuration on the same kernel sources); {} otherwise."""
    doc = _pmc_doc("traffic", d, W, kappa)
    if doc is None:
        return {}
    kern = doc.get("kernels", {})
    t = {k: v["hbm_bytes_per_launch"] for k, v in kern.items()}
    by_base(t, kern)
    for dec, pack in (("k_decompose_fused", "k_pack_sm"), ("k_decompose_n4k_fused", "k_pack_sm4"),
                      ("k_decompose_n4k", "k_pack_sm4"), ("k_fold_coeff", "k_pack_keys")):
        if dec in t and pack in t:  # the decompose phase launches both
            t[dec] += t[pack]
    return t


def load_sq(d, W, kappa, field="valu_busy"):
    """PMC-measured VALU (or, field="mfma_busy", matrix-pipe) busy fraction per kernel
    (profiles/pmc_sq_d<d>_W<W>_k<kappa>.json, written by tools/prof_summary.py sq from one
    SQ pass of this configuration on the same kernel sources); {} otherwise."""
    doc = _pmc_doc("sq", d, W, kappa)
    if doc is None:
        return {}
    kern = doc.get("kernels", {})
    t = {k: v.get(field) for k, v in kern.items()}
    by_base(t, kern)
    return t


def cpu_limits():
    """the host's CPU picture, each figure separately: the machine's CPUs
    (os.cpu_count(); the whole host on the GPU box), this process's affinity set,
    and the cgroup CPU quota in CPUs (None when unlimited or absent)"""
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = int(q) / int(period)
    except (OSError, ValueError):
        pass
    return {"machine_cpus": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)), "cgroup_quota_cpus": quota}


def host_cores():
    """CPUs this process may use: its affinity set, capped by a cgroup CPU quota
    (the GPU box shows the whole machine in os.cpu_count())"""
    lim = cpu_limits()
    n = lim["affinity_cpus"]
    if lim["cgroup_quota_cpus"] is not None:
        n = min(n, -(-int(lim["cgroup_quota_cpus"] * 1000) // 1000))
    return max(1, n)


def cpu_step_seconds(O, d, kappa, W, threads):
    """one commit+fold step of the oracle's C restatement at w_ccs length W"""
    B, L, bs, K = 1 << 15, 5, 2, 15
    N = W * L
    A = O.fill_uniform(kappa * N * d, SEED_A)
    w_ccs = O.fill_uniform(W * d, SEED_W)
    acc_fc, acc_f = O.witness_from_w_ccs(O.fill_uniform(W * d, SEED_ACC), d, B, L, threads)
    acc_cm = O.ajtai_commit(A, kappa, N, d, acc_f, 1, threads)
    rho = O.crt(O.fill_uniform(2 * K * d, SEED_RHO), d)
    t0 = time.perf_counter()
    fc, f = O.witness_from_w_ccs(w_ccs, d, B, L, threads)
    cm = O.ajtai_commit(A, kappa, N, d, f, 1, threads)
    sides = [O.decompose_witness(x, d, B, L, bs, K, threads) for x in (acc_fc, fc)]
    vecs = np.concatenate([s[1].reshape(K, N * d)[1:] for s in sides]).ravel()
    ycat = O.ajtai_commit(A, kappa, N, d, vecs, 2 * (K - 1), threads).reshape(2, K - 1, kappa * d)
    ys = []
    for s, c in enumerate((acc_cm, cm)):
        y = np.zeros((K, kappa * d), np.uint64)
        y[1:] = ycat[s]
        ys.append(O.commit_witnesses_y0(c, y.ravel(), kappa, d, bs, K))
    f0 = O.fold_f0(rho, np.concatenate([s[1] for s in sides]), 2 * K, N, d, threads)
    O.fold_cm0(rho, np.concatenate(ys), 2 * K, kappa, d)
    O.witness_from_f(f0, d, B, L, threads)
    return time.perf_counter() - t0


def cpu_baseline(d, W_full, kappa):
    """The oracle's C restatement of the same step (kind "port": the Rust
    reference cannot be built here), parallelised where the reference uses
    rayon, timed on all host cores the process may use and on one core. Each is
    one step on a bounded sample of about 10 s of CPU work: the whole workload
    when that fits (the reference ring's W = 19 763 on all cores), else a prefix
    of the witness scaled linearly in W (every stage is linear in W). It is the
    naive u128-% restatement, not a tuned rayon build, so it understates what
    the reference's own CPU path would reach."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O

    cores = host_cores()
    w_all = max(1, min(W_full, 4096 if d >= 1024 else W_full))
    w_one = max(1, min(W_full, 256 if d >= 1024 else 4096))
    t_all = cpu_step_seconds(O, d, kappa, w_all, cores)
    t_one = cpu_step_seconds(O, d, kappa, w_one, 1)
    v_all = 1.0 / (t_all * W_full / w_all)
    v_one = 1.0 / (t_one * W_full / w_one)
    scaled = lambda w: "the full workload" if w == W_full else f"scaled linearly from W={w} to W={W_full}"
    return {"value": v_all, "unit": "fold-steps/s", "cores": cores, "kind": "port",
            "sample": f"1 step at W={w_all} on {cores} threads ({t_all:.2f} s; {scaled(w_all)}) and at W={w_one} on "
                      f"1 thread ({t_one:.2f} s; {scaled(w_one)}), d={d}, kappa={kappa}",
            "sample_short": f"oracle C step, W={w_all} on {cores} threads ({t_all:.1f} s), x{W_full / w_all:g} in W",
            "host": cpu_limits(),
            "single_core": {"value": v_one, "cores": 1}}


class _Roctx:
    """roctx ranges (librocprofiler-sdk-roctx) around the serialized phase pass of
    every workload, so `tools/prof_summary.py stats` can keep exactly the kernels
    the bench line's per-phase HIP-event times come from (rocprofv3
    --marker-trace); a no-op when the library is absent."""

    def __init__(self):
        import ctypes
        self.lib = None
        for name in ("librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1"):
            try:
                lib = ctypes.CDLL(name)
                lib.roctxRangePushA.argtypes = [ctypes.c_char_p]
                lib.roctxRangePushA.restype = ctypes.c_int
                lib.roctxRangePop.restype = ctypes.c_int
                self.lib = lib
                break
            except OSError:
                continue

    def push(self, msg):
        if self.lib is not None:
            self.lib.roctxRangePushA(msg.encode())

    def pop(self):
        if self.lib is not None:
            self.lib.roctxRangePop()


ROCTX = _Roctx()


def window_name(wl, what="phase_pass"):
    """the roctx range name of a workload's serialized pass (prof_summary keys on it)"""
    return f"{what} d={wl.d} W={wl.W} kappa={wl.kappa}"


_STREAMS = {}


def step_stream(torch, local, i):
    """Step stream i (> 0) of this process, created once and shared by every
    workload: a fresh torch.cuda.Stream per workload hands later workloads pool
    streams that share hardware queues with each other (the W = 464 shape ran at
    1,020 steps/s after the other workloads against 1,320 in a process of its
    own; HIP maps streams onto GPU_MAX_HW_QUEUES = 4 queues)."""
    key = (local, i)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=local)
    return _STREAMS[key]


class Workload:
    """One fold-step workload resident in HBM: the Ajtai scheme, the accumulator
    side and rho (shared, read-only), and `streams` independent step streams,
    each an lf context on its own HIP stream with its own w_ccs and outputs."""

    def __init__(self, LA, torch, local, rank, d, W, kappa, streams, seed_a=SEED_A, keep_fk=True, cu_partition=False,
                 packed=None, batch=False, cu_split=0):
        # keep_fk=False (fused X^1024+1 path only): the decomposed planes live only
        # as MFMA operand rows (lf.h: f_k buffers omitted) -- 20 GB less HBM at
        # W = 2^14, but slower, so the bench keeps f_k.
        # packed (default for d = 24 and 1024): the decomposed witnesses are kept as
        # packed digit planes (lf_fold_step_bufs.planes: 8 B per element and plane at
        # d = 24, 2 B per coefficient for all planes at d = 1024) instead of u64 f_k /
        # f_coeff_k rows (2 x 8 d B per element and plane); lf_dev_expand_planes
        # makes the rows. d = 1024, W = 2^14: decomposition 14.0 -> 12.4 ms, 41.5 -> 44.0 steps/s
        self.packed = packed = (d in (24, 1024, 4096)) if packed is None else packed
        # batch = G > 1: the step streams form groups of G; each group's G steps are one
        # lf_dev_fold_step_batch call (independent steps on their own streams, one
        # contraction launch for the group); the groups take turns, so one group's
        # contraction overlaps the others' decompositions. batch = 1: one group of all
        g = streams if batch == 1 else int(batch or 0)
        self.group = g if 1 < g <= streams and streams % g == 0 else 0
        self.batch = self.group > 0
        self.keep_fk = keep_fk and not packed
        self.LA, self.torch = LA, torch
        self.d, self.W, self.kappa = d, W, kappa
        self.pr = pr = LA.goldilocks_dp(d)
        K, L = pr.K, pr.L
        self.N = N = W * L
        i64 = dict(dtype=torch.int64, device=f"cuda:{local}")
        z = lambda n: torch.empty(n, **i64)
        ctx = LA.Context(local)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        A = z(kappa * N * d)
        ctx.dev_fill_uniform(A, seed_a)
        self.sch = sch = LA.AjtaiCommitmentScheme(ctx, device_tensor=A, kappa=kappa, ncols=N, d=d)
        if sch.layout == 1:  # the scheme keeps A in MFMA fragment order; drop the AoS copy
            del A
            torch.cuda.empty_cache()
        # accumulator side: a previous witness built the reference way (from_w_ccs + commit)
        acc_w = z(W * d)
        ctx.dev_fill_uniform(acc_w, SEED_ACC)
        acc_fc, acc_f, acc_cm = z(N * d), z(N * d), z(kappa * d)
        ctx.check(ctx.lib.lf_dev_witness_from_w_ccs(ctx.h, LA._lib.C.byref(pr), acc_w.data_ptr(), W,
                                                    acc_fc.data_ptr(), acc_f.data_ptr()))
        ctx.dev_ajtai_commit(sch, [acc_f], acc_cm)
        del acc_w, acc_f
        # rho: 29 short challenges from seeded bytes (CR/rings/goldilocks.rs:41-67) + ONE, NTT form
        rng = np.random.default_rng(SEED_RHO)
        rc = [LA.short_challenge(rng.integers(0, 256, 3 * d // 4, dtype=np.uint8).tobytes(), d)
              for _ in range(2 * K - 1)]
        one = np.zeros(d, np.uint64)
        one[0] = 1
        rho = torch.from_numpy(np.concatenate(rc + [one]).view(np.int64)).to(f"cuda:{local}")
        ctx.dev_crt(rho, d)
        self.ctxs, self.keeps, self.bufs, self.streams = [], [], [], []
        for i in range(streams):
            c = ctx if i == 0 else LA.Context(local)
            if i > 0:
                st = step_stream(torch, local, i)
                c.set_stream(st.cuda_stream)
                self.streams.append(st)
            w_ccs = z(W * d)
            c.dev_fill_uniform(w_ccs, SEED_W + 7919 * rank + 104729 * i)
            keep = {
                "w_ccs": w_ccs, "acc_cm": acc_cm, "acc_f_coeff": acc_fc, "rho": rho,
                "f_coeff": z(N * d), "f": z(N * d), "cm": z(kappa * d),
                "fk_coeff": [z(K * N * d) for _ in range(2)] if not packed else [None, None],
                "fk": [z(K * N * d) for _ in range(2)] if self.keep_fk else [None, None],
                "wk": [z(K * W * d) for _ in range(2)], "y": [z(K * kappa * d) for _ in range(2)],
                "f0": z(N * d), "f0_coeff": z(N * d), "w_ccs0": z(W * d), "cm0": z(kappa * d),
                "planes": [z(K * N if d == 24 else N * 256 if d == 1024 else N * K * 128) for _ in range(2)]
                if packed else [None, None],
            }
            bufs = LA.LfFoldStepBufs()
            for k, v in keep.items():
                if isinstance(v, list):
                    for s in range(2):
                        getattr(bufs, k)[s] = v[s].data_ptr() if v[s] is not None else None
                else:
                    setattr(bufs, k, v.data_ptr())
            ncu = torch.cuda.get_device_properties(local).multi_processor_count
            if cu_partition and streams > 1:
                c.use_cu_mask(range(i * ncu // streams, (i + 1) * ncu // streams))
            elif cu_split and self.batch:
                # step streams on CUs [0, ncu - cu_split), every group's contraction on one
                # stream of the last cu_split CUs (shared: the groups' contractions queue)
                c.use_cu_mask(range(ncu - cu_split))
                if i == 0:
                    self.cstream = c.cu_mask_stream(range(ncu - cu_split, ncu))
                if i % self.group == 0:
                    c.set_contract_stream(self.cstream)
            c.reserve(kappa, N, d, 2 * (K - 1) + 1)
            self.ctxs.append(c)
            self.keeps.append(keep)
            self.bufs.append(bufs)
        torch.cuda.synchronize()

    def run(self, steps, comm=None, streams=None):
        """`steps` fold steps, round-robin over the step streams (asynchronous);
        with `comm`, each step is this rank's column shard of one fold
        (lf_dev_fold_step_sharded: RCCL all-reduce of the commitments)"""
        S = streams or len(self.ctxs)
        i = 0
        if self.batch and comm is None and S == len(self.ctxs):
            g = self.group
            for b in range(steps // g):
                j = (b % (S // g)) * g
                self.ctxs[j].dev_fold_step_batch(self.ctxs[j + 1:j + g], self.sch, self.pr, self.W,
                                                 self.bufs[j:j + g])
                self.last_stream = j + g - 1
            i = steps // g * g
            r = steps - i
            if r > 1:  # a partial last group is one smaller batch (every step still one full step)
                j = ((steps // g) % (S // g)) * g
                self.ctxs[j].dev_fold_step_batch(self.ctxs[j + 1:j + r], self.sch, self.pr, self.W,
                                                 self.bufs[j:j + r])
                self.last_stream = j + r - 1
                i = steps
        for i in range(i, steps):
            if comm is None:
                self.ctxs[i % S].dev_fold_step(self.sch, self.pr, self.W, self.bufs[i % S])
            else:
                self.ctxs[i % S].dev_fold_step_sharded(self.sch, self.pr, self.W, self.bufs[i % S], comm)
            self.last_stream = i % S

    def timing(self, on):
        for c in self.ctxs:
            c.kernel_timing(on)

    def phase_totals(self):
        """(device ms, launches) per phase, summed over every step stream"""
        nvec = 2 * (self.pr.K - 1) + 1
        tot = {}
        for c in self.ctxs:
            for ph, (ms, cnt) in [("ajtai", c.kernel_stats(nvec))] + [(p, c.phase_stats(p)) for p in c.PHASES]:
                a = tot.setdefault(ph, [0.0, 0])
                a[0] += ms
                a[1] += cnt
        return tot

    def sync(self):
        for c in self.ctxs:
            c.sync()  # surfaces any decomposition overflow

    def close(self):
        self.sync()
        self.sch = None
        self.keeps, self.bufs = [], []
        if getattr(self, "cstream", None) is not None:
            # the group leaders hold ctx 0's CU-masked contract stream: clear it
            # everywhere before ctx 0 (its owner) releases it
            for c in self.ctxs:
                c.set_contract_stream(None)
            self.cstream = None
        for c in self.ctxs[1:] + self.ctxs[:1]:  # ctx 0, the owner of shared streams, last
            c.close()
        self.ctxs = []


def warmup_steps(wl, warmup, comm=None):
    """the untimed steps measure() runs: `warmup`, rounded up to whole groups
    when the step streams' contractions are batched"""
    if wl.batch and comm is None and wl.group > 1:
        return -(-warmup // wl.group) * wl.group
    return warmup


def measure(LA, torch, LD, pg, world, wl, steps, warmup, comm=None, phases=True, after_timed=None):
    """time `steps` fold steps of workload `wl` (after `warmup` untimed ones):
    barrier + device sync on both sides, max over ranks; every phase timed
    with HIP events on its launch stream inside the timed region. With several
    step streams the phases overlap, so their launch times would not be the
    kernels' own: the phases are then timed in a second batch on one stream.
    phases=False: only the timed steps (no phase times, no second batch; the
    report is empty). `after_timed()` runs once the timed steps are done and
    checked, before any further pass."""
    S = len(wl.ctxs)
    # batched groups: the warmup covers at least one whole group, so the
    # batched contraction's first launch (code object load) is not timed
    wl.run(warmup_steps(wl, warmup, comm), comm)
    wl.sync()
    serial = S == 1 and phases  # one stream: the timed steps are the phase pass
    if serial:
        wl.timing(True)
    LD.barrier(pg)
    torch.cuda.synchronize()
    if serial:
        ROCTX.push(window_name(wl))
    t0 = time.perf_counter()
    wl.run(steps, comm)
    torch.cuda.synchronize()
    if serial:
        ROCTX.pop()
    LD.barrier(pg)
    dt = time.perf_counter() - t0
    wl.sync()  # surfaces any decomposition overflow
    dt_max = LD.max_over_ranks(pg, dt)
    if after_timed is not None:
        after_timed()
    if not phases:
        return dt_max, ({}, None)
    if S > 1 and wl.batch and comm is None:
        # the phase pass of batched steps: every context on the first one's stream,
        # so the phases run one at a time and the contraction covers `group` steps
        base = torch.cuda.current_stream().cuda_stream
        for c in wl.ctxs:
            c.set_stream(base)
        wl.timing(True)
        n = max(1, steps // wl.group) * wl.group
        torch.cuda.synchronize()
        ROCTX.push(window_name(wl))
        wl.run(n, comm)
        wl.sync()
        ROCTX.pop()
        tot = wl.phase_totals()
        wl.timing(False)
        for c, st in zip(wl.ctxs[1:], wl.streams):
            c.set_stream(st.cuda_stream)
        return dt_max, phase_report(LA, wl, tot, n)
    if S > 1:  # the phase pass: one stream
        wl.ctxs[0].kernel_timing(True)
        torch.cuda.synchronize()
        ROCTX.push(window_name(wl))
        wl.run(steps // S, comm, streams=1)
        wl.sync()
        ROCTX.pop()
        tot = wl.phase_totals()
        wl.timing(False)
        return dt_max, phase_report(LA, wl, tot, steps // S)
    tot = wl.phase_totals()
    wl.timing(False)
    return dt_max, phase_report(LA, wl, tot, steps)


def phase_report(LA, wl, tot, steps):
    """per phase: average launch, launches and device ms per step, algorithmic
    bytes, achieved GB/s and fraction of HBM peak; the dominant phase's roofline"""
    d, W, kappa = wl.d, wl.W, wl.kappa
    _, alg, operand = algorithmic_bytes(d, W, kappa, wl.pr.L, wl.pr.K)
    if not wl.keep_fk and not wl.packed:  # the planes are written once, as the operand rows: no bytes beyond B2
        operand["decompose"] = 0
    # packed planes fold in coefficient form as with f_k (the operand rows are only the fallback's)
    kernel_of = kernel_names(LA, d, W, wl.sch.layout, wl.keep_fk or wl.packed, wl.packed)
    traffic = load_traffic(d, W, kappa)
    valu = load_sq(d, W, kappa)
    mfma = load_sq(d, W, kappa, "mfma_busy")
    phases = {}
    for ph, (ms, cnt) in tot.items():
        if not cnt:
            continue
        avg = ms / cnt
        # the decomposition covers both sides of a step in one launch or one per launch
        sides = max(1, round(2 * steps / cnt)) if ph == "decompose" else 1
        a = alg[ph] * sides
        cf = ph == "fold" and kernel_of[ph] == "k_fold_coeff"
        cf24 = ph == "fold" and kernel_of[ph] == "k_fold_coeff_phi72"
        if cf:  # the coefficient-form fold never reads the 2K NTT-form planes (B4): count what it moves
            a = wl.N * (2 * 2048 + 2 * 2 * wl.pr.K * 256 + 8 * 1024)  # packed digits in, keys out + in, f0_coeff out
        if ph == "decompose" and wl.packed:
            # B2 counts the u64 f_k / f_coeff_k rows the reference materialises; this
            # launch keeps them as packed planes instead (d = 24: 8 B per element and
            # plane written; d = 1024: the 2 B-per-coefficient words it reads anyway)
            planes_b = wl.pr.K * wl.N * 8 if d == 24 else wl.N * 2 * d if d == 1024 else wl.pr.K * wl.N * d // 4
            phases_note = {"packed_planes": True,
                           "moved_bytes_per_launch": sides * (wl.N * 8 * d + planes_b + wl.pr.K * W * 8 * d)
                           + operand.get(ph, 0) * sides}
        else:
            phases_note = {}
        if ph == "ajtai" and wl.sch.layout == 1:
            # the matrix-core work one step's contraction issues: per (virtual) slot, 32-row
            # tile and 32-column chunk, 64 v_mfma_i32_32x32x32_i8 (8 x 8 byte planes)
            dv = 40 if d == 24 else d
            nch = ((wl.W + 15) // 16 * wl.pr.L + 1) // 2
            macs = dv * ((kappa + 31) // 32) * nch * 64 * 32 ** 3
            tops = 2 * macs / (avg * 1e-3) / 1e12
            phases_note["matrix"] = {"bound": "mfma", "i8_macs_per_step": macs, "achieved_tops": tops,
                                     "peak_tops": I8_DENSE_TOPS, "frac_mfma": tops / I8_DENSE_TOPS}
        if cf24:  # digit masks in (8 B per element and plane); f0_coeff, f0 (E each) and w_ccs0 out (from_f's outputs)
            a = wl.N * (2 * wl.pr.K * 8 + 2 * 8 * d) + wl.W * 8 * d
        if ph == "ajtai" and wl.batch:
            # one launch covers `group` steps and reads A once for all of them; the
            # context records it as `group` launches, so avg / bytes here are per step
            # and A counts 1 / group of its bytes (SURVEY B1 + B3 count it twice per step)
            E = 8 * d
            nvec = 2 * (wl.pr.K - 1) + 1
            phases_note.update({"steps_per_launch": wl.group, "launch_ms": avg * wl.group,
                                "survey_bytes_per_step": alg[ph]})
            a = E * (kappa * wl.N / wl.group + nvec * wl.N + nvec * kappa)
        gbs = a / (avg * 1e-3) / 1e9
        extra = operand.get(ph, 0) * sides
        tr = traffic.get(kernel_of[ph])
        if ph == "ajtai" and wl.batch and tr is not None:
            # one batched contraction launch covers `group` steps (the PMC run uses the
            # same grouping); avg and bytes here are per step
            tr = tr / wl.group
        phases[ph] = {"kernel": kernel_of[ph], "avg_launch_ms": avg, "launches_per_step": cnt / steps,
                      "ms_per_step": ms / steps, "algorithmic_bytes_per_launch": a,
                      "achieved_gbs": gbs, "frac_hbm": gbs / HBM_PEAK_GBS,
                      "operand_bytes_per_launch": extra,
                      "achieved_gbs_incl_operands": (a + extra) / (avg * 1e-3) / 1e9,
                      "traffic_bytes_per_launch": tr,
                      "valu_busy": valu.get(kernel_of[ph]), "mfma_busy": mfma.get(kernel_of[ph]), **phases_note}
        if cf:
            # an exact i8 GEMM: 1024 coefficients x 2K 1024 digit rows x N elements
            macs = 1024 * 2 * wl.pr.K * 1024 * wl.N
            tops = 2 * macs / (avg * 1e-3) / 1e12
            phases[ph]["coefficient_form"] = {
                "bound": "mfma", "i8_macs": macs, "achieved_tops": tops, "peak_tops": I8_DENSE_TOPS,
                "frac_mfma": tops / I8_DENSE_TOPS, "survey_b4_bytes": alg[ph],
                "note": "f_0 = NTT(sum_i rho_i * D_i) from the digit planes D_i on the i8 matrix cores "
                        "(fold_coeff.hip, with the digit-key packing in the same phase); "
                        "algorithmic_bytes_per_launch is what it moves, SURVEY B4 would read the 2K NTT-form planes"}
        if cf24:
            phases[ph]["coefficient_form"] = {
                "survey_b4_bytes": alg[ph],
                "note": "f_0 = CRT(sum_i rho_i * D_i) from the decomposition's digit masks, with Witness::from_f "
                        "(f0_coeff, w_ccs0) in the same launch (k_fold_coeff_phi72); the from_f phase only "
                        "launches the gated fallback"}
    if not phases:
        return phases, None
    dom = max(phases, key=lambda k: phases[k]["ms_per_step"])
    p = phases[dom]
    roof = {"kernel": p["kernel"], "phase": dom, "bound": "hbm", "achieved": p["achieved_gbs"],
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": p["frac_hbm"], "traffic": p["traffic_bytes_per_launch"],
            "avg_launch_ms": p["avg_launch_ms"], "bytes_per_launch": p["algorithmic_bytes_per_launch"],
            "extra_bytes": p["operand_bytes_per_launch"], "valu_busy": p["valu_busy"],
            # the roctx range whose kernels these HIP-event times cover (rocprofv3
            # --marker-trace; tools/prof_summary.py stats summarises that window)
            "profile_window": window_name(wl)}
    return phases, roof


def extra_shape(LA, torch, LD, pg, local, rank, world, d, W, kappa, S, steps, warmup, what, batch=False):
    """Another commit+fold workload with S concurrent step streams per GPU,
    reported beside the default one (not as `value`): the reference's own ring
    at the real zkvm shape (d = 24, W = 19 763; the bit-exact-vs-reference
    path), SURVEY.md 8(d)'s byte-equivalent shape (d = 1024, W = 464), whose
    per-GPU rate the north-star target (1e4 steps/s on 8 GPUs) is about, and
    BASELINE configs[4]'s ring (d = 4096, kappa = 64)."""
    wl = Workload(LA, torch, local, rank, d, W, kappa, S, batch=batch)
    dt, (phases, roof) = measure(LA, torch, LD, pg, world, wl, steps, warmup)
    batched, group = wl.batch, wl.group
    wl.close()
    del wl
    torch.cuda.empty_cache()
    value = world * steps / dt
    step_bytes, _, _ = algorithmic_bytes(d, W, kappa)
    how = (f"{S} concurrent step streams per GPU" +
           (f", in groups of {group} whose contractions are one launch (one pass over A)"
            if batched else ""))
    return {"workload": f"commit+fold step, {what}, w_ccs W={W}, kappa={kappa}, {how}",
            "d": d, "W": W, "kappa": kappa, "streams": S, "value": value, "unit": "fold-steps/s", "n_gpus": world,
            "steps": steps, "ms_per_step_per_gpu": dt / steps * 1e3,
            "hbm_gbs_step_algorithmic": step_bytes * value / world / 1e9,
            "step_hbm": step_hbm(d, W, kappa, group if batched else 1, phases, value / world),
            "roofline": roof, "phases": phases}


def sharded_fold(LA, torch, LD, pg, local, rank, world, d, W, kappa, steps, warmup):
    """One fold sharded by columns over all ranks: rank r holds
    W w_ccs groups (its shard of a world * W witness) and A's matching columns;
    every step all-reduces the 29 partial commitments over RCCL (mod p, limb
    transport) on the step's stream (lf_dev_fold_step_sharded)."""
    wl = Workload(LA, torch, local, rank, d, W, kappa, 1, seed_a=SEED_A + 7919 * rank)
    comm = LD.make_comm(wl.ctxs[0], pg, world, rank)
    comm_size = comm.size if comm is not None else 1  # the rank count RCCL reports (lf_comm_size)
    try:
        dt, (phases, roof) = measure(LA, torch, LD, pg, world, wl, steps, warmup, comm)
    finally:
        if comm is not None:
            comm.close()
        wl.close()
        del wl
        torch.cuda.empty_cache()
    # bit-exact self-check of the same path over the same communicator kind: each
    # rank's shard of a world x 64-group fold against the unsharded fold on its GPU
    ctx = LA.Context(local)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        verified = LD.verify_sharded_step(LA, ctx, pg, local, rank, world, d=d, kappa=kappa)
    finally:
        ctx.close()
        torch.cuda.empty_cache()
    kd = 29 * kappa * d * 8
    return {"workload": f"one commit+fold step of a w_ccs of W={world}x{W} ring elements, column-sharded "
                        f"over {world} GPUs (W={W} per GPU), d={d}, kappa={kappa}; per step one RCCL all-reduce "
                        f"of the 29 partial commitments ({kd / 1e6:.1f} MB as 2x32-bit limbs)",
            "value": steps / dt, "unit": "sharded fold-steps/s", "shard_steps_per_s": world * steps / dt,
            "n_gpus": world, "steps": steps, "ms_per_step": dt / steps * 1e3, "scaling": "weak",
            "roofline": roof, "phases": phases,
            "verified": verified, "comm_size": comm_size,
            "verification": f"after timing, every rank's shard of a {world} x 64-group fold through the same RCCL "
                            f"exchange equals the unsharded fold on its GPU, every output bit for bit "
                            f"(latticeum_amd.dist.verify_sharded_step)"}


def side_ops(LA, torch, local):
    """BASELINE.json configs[1] (batched d = 1024 NTT/INTT of 2^16 polynomials)
    and the Poseidon2 batch of configs[4] (2^20 states), device time per launch."""
    ctx = LA.Context(local)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def ev_ms(fn, reps=10):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    out = {}
    d, n = 1024, 1 << 16
    x = torch.empty(n * d, dtype=torch.int64, device=f"cuda:{local}")
    ctx.dev_fill_uniform(x, SEED_W - 2)
    by = 2 * n * d * 8
    for name, fn in (("fwd", lambda: ctx.dev_crt(x, d)), ("inv", lambda: ctx.dev_icrt(x, d))):
        ms = ev_ms(fn)
        out[f"ntt_{name}"] = {"npoly": n, "d": d, "ms": ms, "polys_per_s": n / ms * 1e3,
                              "achieved_gbs": by / ms / 1e6, "frac_hbm": by / ms / 1e6 / HBM_PEAK_GBS}
    del x
    m = 1 << 20
    st = torch.empty(16 * m, dtype=torch.int64, device=f"cuda:{local}")
    ctx.dev_fill_uniform(st, 0x4C460007)
    ms = ev_ms(lambda: ctx.dev_poseidon2_permute(st))
    out["poseidon2_w16"] = {"states": m, "ms": ms, "perms_per_s": m / ms * 1e3,
                            "achieved_gbs": 2 * 16 * 8 * m / ms / 1e6}
    del st
    # the side ops' own PMC passes (tools/gpu_pmc_side.sh: these launches at these sizes)
    cfg = {"side_ops": True}
    tr = _pmc_doc("traffic", 0, 0, 0, "pmc_traffic_side_ops.json", cfg) or {}
    sq = _pmc_doc("sq", 0, 0, 0, "pmc_sq_side_ops.json", cfg) or {}
    for key, kern in (("ntt_fwd", "k_xform_n32<true>"), ("ntt_inv", "k_xform_n32<false>"),
                      ("poseidon2_w16", "k_p2_permute")):
        t = (tr.get("kernels") or {}).get(kern) or {}
        q = (sq.get("kernels") or {}).get(kern) or {}
        b = t.get("hbm_bytes_per_launch")
        out[key]["pmc"] = {"kernel": kern, "traffic_bytes_per_launch": b,
                           "frac_hbm_pmc": b / (out[key]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS if b else None,
                           "valu_busy": q.get("valu_busy"), "wait_cnt_frac": q.get("wait_cnt_frac"),
                           "wait_issue_frac": q.get("wait_issue_frac")}
    ctx.sync()
    ctx.close()
    torch.cuda.empty_cache()
    return out


def next_rows(LA, torch, local, cpu):
    """SURVEY.md 8(f) rows 1 and 2 at the zkvm's shapes on the reference ring
    (Phi_72, log m = 17): the folding sumcheck prover (95 MLEs, degree 4, 17
    rounds through the Poseidon2 transcript; folding/utils.rs:196-331) and the
    sparse CCS products of one fold (t = 125 matrices 2^17 x 19 768, ~1 entry
    per row per matrix; the zeta-challenged Mz MLE of K = 15 instances and the
    15 x 125 evaluations eta_s). Device time with the host transcript in the loop."""
    ctx = LA.Context(local)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {}
    d, nv, nk, tau = 24, 17, 30, 3
    n = 1 << nv
    nm = 5 + nk * tau
    i64 = dict(dtype=torch.int64, device=f"cuda:{local}")
    m = torch.empty(nm * n * d, **i64)
    mu = torch.empty(nk * d, **i64)
    ctx.dev_fill_uniform(mu, 0x4C460010)
    comb = LA.Comb.folding(mu, nk, tau, 2)
    times = []
    for rep_ in range(4):
        ctx.dev_fill_uniform(m, 0x4C460011 + rep_)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.sumcheck_prove(LA.Poseidon2Transcript(), comb, m, nm, nv, d, 4)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    ms = min(times[1:]) * 1e3
    mle_bytes = nm * n * d * 8
    out["folding_sumcheck"] = {
        "workload": f"folding sumcheck prover: Phi_72, {nm} MLEs of 2^{nv} ring elements ({mle_bytes / 1e9:.2f} GB), "
                    f"degree 4, {nv} rounds with the Poseidon2 transcript on the host",
        "ms_per_prove": ms, "rounds": nv,
        "hbm_gbs_min_traffic": 2.5 * mle_bytes / (ms * 1e-3) / 1e9,
        "note": "VALU-bound: four Fq3 products and four lazy multiply-accumulates per MLE value per point (B_SMALL = 2 cubic form)"}
    del m
    torch.cuda.empty_cache()
    if cpu is not None:
        # the oracle's prover over the same comb at log m = 12, scaled by 2^(17-12)
        sys.path.insert(0, str(ROOT / "oracle"))
        import oracle as O
        nvs = 12
        mles = O.fill_uniform(nm * (1 << nvs) * d, 5)
        mu_h = O.fill_uniform(nk * d, 6)
        t0 = time.perf_counter()
        O.sumcheck_prove(O.new_transcript(), O.SumcheckComb.folding(mu_h, nk, tau, 2), mles, nm, nvs, d, 4)
        dt = time.perf_counter() - t0
        out["folding_sumcheck"]["cpu_baseline"] = {
            "ms_per_prove": dt * (1 << (nv - nvs)) * 1e3, "cores": 1, "kind": "port",
            "sample": f"the oracle's prover at log m = {nvs} ({dt:.2f} s, 1 thread), scaled by 2^{nv - nvs}"}
    # the linearization sumcheck at the zkvm's CCS degree: 125 Mz MLEs + eq(beta),
    # 52 multisets (16 of size 7, the Poseidon2 S-box, and 36 of size 1 or 2),
    # degree 8 (LINEARIZATION_DEGREE - 1, zkvm/src/ccs.rs:55-67), 17 rounds
    rng = np.random.default_rng(0x4C460014)
    S = [list(rng.integers(0, 125, 7)) for _ in range(16)] + \
        [list(rng.integers(0, 125, 1 + (i % 2))) for i in range(36)]
    S = [[int(j) for j in x] for x in S]
    nml = 126
    m = torch.empty(nml * n * d, **i64)
    cdev = torch.empty(len(S) * d, **i64)
    ctx.dev_fill_uniform(cdev, 0x4C460015)
    combl = LA.Comb.linearization(cdev, S)
    times = []
    for rep_ in range(3):
        ctx.dev_fill_uniform(m, 0x4C460016 + rep_)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.sumcheck_prove(LA.Poseidon2Transcript(), combl, m, nml, nv, d, 8)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out["linearization_sumcheck"] = {
        "workload": f"linearization sumcheck prover: Phi_72, {nml} MLEs of 2^{nv} ring elements "
                    f"({nml * n * d * 8 / 1e9:.2f} GB), 52 multisets (16 of size 7), degree 8, {nv} rounds",
        "ms_per_prove": min(times[1:]) * 1e3, "rounds": nv}
    del m
    torch.cuda.empty_cache()
    # sparse CCS products at the zkvm's dimensions
    t, mm, nn, K = 125, 1 << 17, 19768, 15
    rng = np.random.default_rng(0x4C460012)
    mats, nnz = [], 0
    for j in range(t):
        cnt = rng.integers(0, 3, mm)
        rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        mats.append([rp, rng.integers(0, nn, int(rp[-1])).astype(np.uint32), None])
        nnz += int(rp[-1])
    vals = torch.empty(nnz * d, **i64)
    ctx.dev_fill_uniform(vals, 0x4C460013)
    hv = vals.cpu().numpy().view(np.uint64)
    del vals
    off = 0
    for mt in mats:
        k = int(mt[0][-1])
        mt[2] = hv[off * d:(off + k) * d]
        off += k
    M = LA.CCSMatrices(ctx, d, mm, nn, mats)
    structure = [(mt[0], mt[1]) for mt in mats]
    del hv, mats
    z = torch.empty(K * nn * d, **i64)
    ctx.dev_fill_uniform(z, 0x4C460014)
    zeta = torch.empty(K * d, **i64)
    ctx.dev_fill_uniform(zeta, 0x4C460015)
    point = torch.empty(nv * d, **i64)
    ctx.dev_fill_uniform(point, 0x4C460016)
    ch = torch.empty(mm * d, **i64)
    ev = torch.empty(K * t * d, **i64)

    def ev_ms(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_ch = ev_ms(lambda: M.mz_challenged(z, zeta, K, nv, ch))
    ms_ev = ev_ms(lambda: M.mz_evaluate(z, K, nv, point, ev))
    val_bytes = nnz * d * 8
    out["mz_products"] = {
        "workload": f"CCS t={t} matrices {mm} x {nn} ({nnz} ring-element entries, {val_bytes / 1e9:.2f} GB), "
                    f"K={K} decomposed vectors",
        "challenged_mle_ms": ms_ch, "etas_ms": ms_ev,
        "challenged_gbs_values": val_bytes / (ms_ch * 1e-3) / 1e9}
    out["fold_prove"] = fold_prove_line(LA, torch, ctx, M, S, d, nn, t, mm)
    del M
    torch.cuda.empty_cache()
    # the same rows with scalar values, as the zkvm's R1CS-derived matrices hold
    # (R::one(), negations, from_goldilocks constants: zkvm/src/constraints.rs:127-364):
    # the products then read one word per entry (lf_ccs_is_scalar)
    sv = torch.empty(nnz, **i64)
    ctx.dev_fill_uniform(sv, 0x4C460019)
    hs = sv.cpu().numpy().view(np.uint64)
    del sv
    full = np.zeros((nnz, d), np.uint64)
    full[:, ::3] = hs[:, None]
    full = full.ravel()
    mats, off = [], 0
    for rp, col in structure:
        k = int(rp[-1])
        mats.append([rp, col, full[off * d:(off + k) * d]])
        off += k
    M = LA.CCSMatrices(ctx, d, mm, nn, mats)
    assert M.scalar
    del full, hs, mats, structure
    ms_ch_s = ev_ms(lambda: M.mz_challenged(z, zeta, K, nv, ch))
    ms_ev_s = ev_ms(lambda: M.mz_evaluate(z, K, nv, point, ev))
    out["mz_products_scalar"] = {
        "workload": f"the rows of mz_products with scalar values (the zkvm's matrices: R::one(), -1, "
                    f"from_goldilocks constants), {nnz} entries of one word each, K={K} decomposed vectors",
        "challenged_mle_ms": ms_ch_s, "etas_ms": ms_ev_s}
    del z, ch, ev
    out["fold_prove_scalar"] = fold_prove_line(LA, torch, ctx, M, S, d, nn, t, mm)
    out["fold_prove_scalar"]["workload"] += "; the CCS values scalars as the zkvm's (lf_ccs_is_scalar)"
    out["zkvm_chain"] = zkvm_chain(LA, torch, ctx, M, S, d, nn, t, mm)
    out["zkvm_chain"]["workload"] += "; the CCS values scalars as the zkvm's (lf_ccs_is_scalar)"
    del M
    # the memory Merkle tree of the zkvm's 8 MB VM (8192 pages of 256 words,
    # vm.rs:106-124; commitments.rs:192-262): 8192 sponge chains of 64 width-8
    # permutations, then 13 levels of compressions
    pages, words = 8192, 256
    mem = torch.empty(pages * words, **i64)
    ctx.dev_fill_uniform(mem, 0x4C460017)
    mem.remainder_(1 << 32)  # u32 memory words
    nodes = torch.empty((2 * pages - 1) * 4, **i64)
    ms_mk = ev_ms(lambda: ctx.dev_merkle_tree(mem, pages, words, nodes))
    out["merkle_memory"] = {"workload": f"Merkle tree of the 8 MB VM memory: {pages} pages x {words} words, "
                                        "width-8 Poseidon2 sponge leaves + compressions",
                            "ms_per_tree": ms_mk, "permutations": pages * words // 4 + pages - 1}
    del mem, nodes
    ctx.close()
    torch.cuda.empty_cache()
    return out


def fold_prove_line(LA, torch, ctx, M, S, d, n, t, m):
    """the zkvm's whole fold() (lf_fold_prove: zk_latticefold_prove with its
    transcript, linearization, two decompositions and the folding prover) at the
    zkvm's shape on the reference ring: l = 4, W = n - 5 = 19 763, kappa = 32,
    the CCS above (t = 125, m = 2^17) with the 52 multisets of the
    linearization line and degree 7; random (not satisfying) witnesses, which
    the prover does not check. Wall time per call, host transcript included."""
    l, kappa, deg = 4, 32, 7
    W = n - l - 1
    pr = LA.goldilocks_dp(d)
    N = W * pr.L
    i64 = dict(dtype=torch.int64, device=f"cuda:{torch.cuda.current_device()}")
    A = torch.empty(kappa * N * d, **i64)
    ctx.dev_fill_uniform(A, SEED_A)
    sch = LA.AjtaiCommitmentScheme(ctx, device_tensor=A, kappa=kappa, ncols=N, d=d)
    del A
    rng = np.random.default_rng(0x4C460018)
    c = rng.integers(0, 1 << 62, len(S) * d, dtype=np.uint64)
    prover = LA.Prover(ctx, sch, pr, M, l, deg, c, S)

    def wit(seed):
        w = {"w_ccs": torch.empty(W * d, **i64), "f": torch.empty(N * d, **i64), "f_coeff": torch.empty(N * d, **i64)}
        ctx.dev_fill_uniform(w["w_ccs"], seed)
        ctx.check(ctx.lib.lf_dev_witness_from_w_ccs(ctx.h, LA._lib.C.byref(pr), w["w_ccs"].data_ptr(), W,
                                                    w["f_coeff"].data_ptr(), w["f"].data_ptr()))
        cm = torch.empty(kappa * d, **i64)
        ctx.dev_ajtai_commit(sch, [w["f"]], cm)
        x = rng.integers(0, 1 << 62, l * d, dtype=np.uint64)
        return x, w, cm.cpu().numpy().view(np.uint64)

    xa, wa, cma = wit(SEED_ACC)
    xi, wi, cmi = wit(SEED_W)
    acc, _ = prover.linearize(cma, xa, wa)
    w_out = {"w_ccs": torch.empty(W * d, **i64), "f": torch.empty(N * d, **i64), "f_coeff": torch.empty(N * d, **i64)}
    times, times_v = [], []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prover.fold_prove(acc, wa, cmi, xi, wi, w_out)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # fold() + generate_verification_witness_vars as the zkvm loop runs them (main.rs:175-185):
    # lf_fold_prove_vars, the vars from the call's own sample log
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prover.fold_prove(acc, wa, cmi, xi, wi, w_out, vars=True)
        torch.cuda.synchronize()
        times_v.append(time.perf_counter() - t0)
    prover.timing(True)
    _, pf, vv = prover.fold_prove(acc, wa, cmi, xi, wi, w_out, vars=True)
    spans = prover.timing(False)
    # the standalone verifier-variable replay of that proof (lf_fold_replay: a second
    # pass of the Poseidon2 transcript), the check the sample-log vars must equal
    t_rep = []
    for _ in range(3):
        t0 = time.perf_counter()
        vr = prover.replay(acc, cmi, xi, pf)
        t_rep.append(time.perf_counter() - t0)
    vars_equal = all(np.array_equal(vv[k], vr[k]) for k in vr)
    t0 = time.perf_counter()
    prover.linearize(cma, xa, wa)
    torch.cuda.synchronize()
    t_lin = time.perf_counter() - t0
    del prover, sch
    torch.cuda.empty_cache()
    return {"workload": f"zkvm fold() end to end (lf_fold_prove): Phi_72, W={W} (n={n}, l={l}), kappa={kappa}, "
                        f"CCS t={t} x {m} rows, {len(S)} multisets, degree {deg}; transcript on the host",
            "ms_per_fold_prove": min(times[1:]) * 1e3, "ms_per_fold_prove_median": float(np.median(times[1:])) * 1e3,
            "ms_per_fold_prove_vars": min(times_v[1:]) * 1e3,
            "ms_per_fold_prove_vars_median": float(np.median(times_v[1:])) * 1e3,
            "ms_per_linearize": t_lin * 1e3, "span_ms": spans, "ms_per_replay": min(t_rep) * 1e3,
            "vars_equal_replay": vars_equal,
            "note": "beside the rho-as-input step of reference_ring: this adds the linearization (Mz, degree-8 "
                    "sumcheck), the decompositions' u_s / v_s, the folding sumcheck, theta_s / eta_s and the "
                    "transcript"}


def zkvm_chain(LA, torch, ctx, M, S, d, n, t, m, steps=16, warmup=2):
    """The zkvm's proving loop (zkvm/src/main.rs:121-219) at its shape, chained: every
    step commits a new z (commit(), :348-367: the witness uploaded from the host,
    Witness::from_w_ccs and the Ajtai commitment on the device), folds it into the
    running accumulator with fold() + generate_verification_witness_vars
    (lf_fold_prove_vars), and seals the step with acc_comm and ivc_step_comm
    (:187-196; state_i_comm from register / code / memory commitments). The folded
    accumulator and its witness feed the next step; the next z's public input
    x_ccs is this step's ivc_step_comm (arithmetize, ivc.rs:107-109). The VM trace
    itself is not reproducible here, so w_ccs is synthetic (seeded per step);
    initialize_accumulator (:305-344) linearizes the zero witness."""
    l, kappa, deg = 4, 32, 7
    W = n - l - 1
    pr = LA.goldilocks_dp(d)
    N = W * pr.L
    dev = f"cuda:{torch.cuda.current_device()}"
    i64 = dict(dtype=torch.int64, device=dev)
    A = torch.empty(kappa * N * d, **i64)
    ctx.dev_fill_uniform(A, SEED_A)
    sch = LA.AjtaiCommitmentScheme(ctx, device_tensor=A, kappa=kappa, ncols=N, d=d)
    del A
    rng = np.random.default_rng(0x4C460018)
    c = rng.integers(0, 1 << 62, len(S) * d, dtype=np.uint64)
    prover = LA.Prover(ctx, sch, pr, M, l, deg, c, S)
    wit = lambda: {"w_ccs": torch.empty(W * d, **i64), "f": torch.empty(N * d, **i64),
                   "f_coeff": torch.empty(N * d, **i64)}
    accw, nxt, wi = wit(), wit(), wit()
    # the synthetic VM witnesses, host-resident as arithmetize leaves them (pinned for the upload)
    total = warmup + steps
    zs = torch.empty((total, W * d), dtype=torch.int64).pin_memory()
    tmp = torch.empty(W * d, **i64)
    for i in range(total):
        ctx.dev_fill_uniform(tmp, SEED_W + 31 * i)
        zs[i].copy_(tmp)
    del tmp
    cm = torch.empty(kappa * d, **i64)
    pr_c = LA._lib.C.byref(pr)

    def broadcast4(comm):  # GoldilocksRingNTT::from(u64) of each limb (main.rs:320-325)
        x = np.zeros(4 * d, np.uint64)
        for k in range(4):
            x[k * d:(k + 1) * d:3] = np.uint64(int(comm[k]))
        return x

    def commit(w):
        ctx.check(ctx.lib.lf_dev_witness_from_w_ccs(ctx.h, pr_c, w["w_ccs"].data_ptr(), W, w["f_coeff"].data_ptr(),
                                                    w["f"].data_ptr()))
        ctx.dev_ajtai_commit(sch, [w["f"]], cm)
        return cm.cpu().numpy().view(np.uint64).copy()

    # initialize_accumulator: the zero witness, x_ccs = the zero step commitment
    accw["w_ccs"].zero_()
    zero4 = np.zeros(4, np.uint64)
    cm0 = commit(accw)
    acc, _ = prover.linearize(cm0, broadcast4(zero4), accw)
    regs = np.arange(32, dtype=np.uint32)
    # the VM's code / memory / memory-ops commitments (synthetic: the zkvm computes them
    # with the width-8 Merkle trees, lf_vm_code_comm / lf_dev_merkle_tree)
    code_comm, mem_comm, ops_comm = [LA.hash_iter(np.arange(4 * k, 4 * k + 4, dtype=np.uint64)) for k in range(3)]
    z0_comm = LA.state_i_comm(code_comm, 0, mem_comm, LA.vm_regs_comm(regs), ops_comm)
    acc_comm = LA.acc_comm(acc)
    h, _ = LA.ivc_step_comm(0, z0_comm, z0_comm, acc_comm)
    t_commit = t_fold = t_comm = 0.0
    vv = pf = None
    x_ccs = cm_i = None
    for i in range(total):
        if i == warmup:
            torch.cuda.synchronize()
            prover.timing(True)
            t_start = time.perf_counter()
        t0 = time.perf_counter()
        x_ccs = broadcast4(h)  # z = [x_ccs | 1 | w_ccs]: the public input is the previous h_i
        wi["w_ccs"].copy_(zs[i], non_blocking=True)
        cm_i = commit(wi)
        t1 = time.perf_counter()
        prev_acc = acc
        acc, pf, vv = prover.fold_prove(acc, accw, cm_i, x_ccs, wi, nxt, vars=True)
        t2 = time.perf_counter()
        regs[1] = i  # the VM state after step i (synthetic registers)
        state_i = LA.state_i_comm(code_comm, 4 * (i + 1), mem_comm, LA.vm_regs_comm(regs), ops_comm)
        acc_comm = LA.acc_comm(acc)
        h, _ = LA.ivc_step_comm(i + 1, z0_comm, state_i, acc_comm)
        t3 = time.perf_counter()
        accw, nxt = nxt, accw  # the folded witness is the next step's w_acc
        if i >= warmup:
            t_commit += t1 - t0
            t_fold += t2 - t1
            t_comm += t3 - t2
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    sp = prover.timing(False)
    # the last step's vars against the standalone replay (a second transcript pass)
    vr = prover.replay(prev_acc, cm_i, x_ccs, pf)
    vars_equal = all(np.array_equal(vv[k], vr[k]) for k in vr)
    del prover, sch
    torch.cuda.empty_cache()
    return {"workload": f"the zkvm proving loop (main.rs:121-219), {steps} chained steps at its shape: commit(z) "
                        f"(upload + from_w_ccs + Ajtai), fold() + generate_verification_witness_vars "
                        f"(lf_fold_prove_vars), acc_comm + state_i_comm + ivc_step_comm; Phi_72, W={W}, kappa={kappa}, "
                        f"CCS t={t} x {m} rows, degree {deg}; synthetic VM witnesses, x_ccs = the previous h_i",
            "value": steps / dt, "unit": "IVC steps/s", "steps": steps, "warmup": warmup, "ms_per_step": dt / steps * 1e3,
            "ms_per_step_commit": t_commit / steps * 1e3, "ms_per_step_fold_vars": t_fold / steps * 1e3,
            "ms_per_step_commitments": t_comm / steps * 1e3,
            "span_ms_per_step": {k: v / steps for k, v in sp.items()},
            "last_vars_equal_replay": vars_equal}


DUMP_SAMPLE = 1 << 18  # words kept of a larger output (the default shape's 13 outputs: 45 MB of float64)
DUMP_SEED = 0x4C460020


def _sample_index(numel, n, seed):
    """n indices below numel, ascending: the first n outputs of SplitMix64(seed)
    mod numel (fixed by `seed` alone, so two builds sample the same elements)"""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return np.sort(x % np.uint64(numel)).astype(np.int64)


def dump_outputs(wl, torch, path):
    """Write the outputs of the last step `wl` ran (lf_fold_step_bufs' output
    buffers of the step stream that ran it: f_coeff, f, cm, wk, y, f0, f0_coeff,
    w_ccs0, cm0, and the planes / fk / fk_coeff forms the workload keeps) as
    `path`/<name>.npy, <name>_0 / <name>_1 for the two sides. An output of more
    than DUMP_SAMPLE elements is sampled (_sample_index, seeded by the output's
    position). Every file is float64 of shape (n, 2): the low and the high 32
    bits of each u64 word, so the values are exact."""
    keep = wl.keeps[wl.last_stream]
    outs = []
    for name in ("f_coeff", "f", "cm", "fk_coeff", "fk", "wk", "y", "f0", "f0_coeff", "w_ccs0", "cm0", "planes"):
        v = keep[name]
        if isinstance(v, list):
            outs += [(f"{name}_{s}", t) for s, t in enumerate(v) if t is not None]
        else:
            outs.append((name, v))
    p = Path(path)
    p.mkdir(parents=True, exist_ok=True)
    for k, (name, t) in enumerate(outs):
        if t.numel() > DUMP_SAMPLE:
            t = t[torch.from_numpy(_sample_index(t.numel(), DUMP_SAMPLE, DUMP_SEED + k)).to(t.device)]
        w = t.cpu().numpy().view(np.uint64)
        np.save(p / f"{name}.npy", np.stack([w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)], axis=1).astype(np.float64))


EXCLUDED = ("outside the timed step (other tiers): the Poseidon2 transcript and challenge derivation (rho is an "
            "input), linearization, the sumcheck provers and the Mz matrix-vector products")
EXCLUDED_SHORT = "rho is an input; transcript, linearization, sumchecks, Mz outside the step"
LINE_LIMIT = 4000  # bytes: the driver keeps only the tail of stdout, so the headline line stays small
DETAIL_DEFAULT = "gpurun_out/bench_detail.json"


def _sig(x, n=4):
    """floats to n significant digits, recursively (the compact line)"""
    if isinstance(x, float):
        return float(f"{x:.{n}g}")
    if isinstance(x, dict):
        return {k: _sig(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, n) for v in x]
    return x


def _phase_row(p):
    """one phase of the compact line: [kernel, ms per step, frac of HBM, PMC bytes per launch, VALU busy,
    matrix-pipe busy]"""
    return [p["kernel"], p["ms_per_step"], p["frac_hbm"], p.get("traffic_bytes_per_launch"), p.get("valu_busy"),
            p.get("mfma_busy")]


def _side_value(s):
    if not isinstance(s, dict):
        return None
    r = s.get("roofline") or {}
    return {"value": s.get("value"), "ms": s.get("ms_per_step_per_gpu"), "frac": r.get("frac"),
            "kernel": r.get("kernel")}


def compact_line(out, detail):
    """The headline JSON line bench.py prints last: the contract's keys, the
    roofline, the CPU baseline, the step-level HBM figures, one row per phase
    and one value per side workload; everything else is in the detail file
    `detail` (the full record). Stays below LINE_LIMIT bytes."""
    keys = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "warmup_steps_run", "ms_per_step",
            "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    line = {k: out.get(k) for k in keys}
    cfg = {k: v for k, v in (out.get("config") or {}).items() if v is not None}
    cfg["workload"] = cfg.get("workload_short", cfg.get("workload"))
    cfg.pop("workload_short", None)
    line["config"] = cfg
    roof = out.get("roofline")
    if roof:
        line["roofline"] = {k: roof.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel",
                                                      "avg_launch_ms", "bytes_per_launch", "valu_busy")}
    cpu = out.get("cpu_baseline")
    if cpu:
        line["cpu_baseline"] = {k: cpu.get(k) for k in ("value", "unit", "cores", "kind")}
        line["cpu_baseline"]["sample"] = cpu.get("sample_short", cpu.get("sample"))
        if cpu.get("single_core"):
            line["cpu_baseline"]["single_core_value"] = cpu["single_core"].get("value")
    else:
        line["cpu_baseline"] = cpu
    sh = out.get("step_hbm") or {}
    line["step_hbm"] = {"survey_frac": sh.get("survey_frac_hbm"), "needed_frac": sh.get("needed_frac_hbm"),
                        "pmc_frac": sh.get("pmc_frac_hbm"), "pmc_bytes_per_step": sh.get("pmc_bytes_per_step"),
                        "steps_per_A_read": sh.get("steps_per_A_read")}
    ph = out.get("phases") or {}
    line["phases"] = {"cols": ["kernel", "ms_per_step", "frac_hbm", "pmc_bytes_per_launch", "valu_busy", "mfma_busy"],
                      **{k: _phase_row(v) for k, v in ph.items()}}
    if ph:
        line["phases"]["sum_ms"] = sum(v["ms_per_step"] for v in ph.values())
        # the matrix-core kernels against the dense i8 peak: [achieved TOPS, fraction]
        mx = {k: (v.get("matrix") or v.get("coefficient_form") or {}) for k, v in ph.items()}
        line["i8_mfma"] = {k: [m.get("achieved_tops"), m.get("frac_mfma")] for k, m in mx.items()
                           if m.get("achieved_tops") is not None}
    side = {}
    for k in ("reference_ring", "small_shape", "configs4_d4096_kappa64"):
        if k in out:
            side[k] = _side_value(out[k])
    rr = out.get("reference_ring") or {}
    if isinstance(rr.get("cpu_baseline"), dict):
        side["reference_ring"]["cpu_value"] = rr["cpu_baseline"].get("value")
    ops = out.get("side_ops") or {}
    if ops:
        side["ntt_ms"] = [ops.get("ntt_fwd", {}).get("ms"), ops.get("ntt_inv", {}).get("ms")]
        side["poseidon2_perms_per_s"] = ops.get("poseidon2_w16", {}).get("perms_per_s")
        # [valu_busy, PMC fraction of HBM] per side op (null when no PMC file matches these sources)
        side["side_ops_pmc"] = {k: [(ops.get(k, {}).get("pmc") or {}).get("valu_busy"),
                                    (ops.get(k, {}).get("pmc") or {}).get("frac_hbm_pmc")]
                                for k in ("ntt_fwd", "ntt_inv", "poseidon2_w16")}
    nx = out.get("next_rows") or {}
    if nx:
        side["fold_prove_ms"] = [nx.get(k, {}).get("ms_per_fold_prove") for k in ("fold_prove", "fold_prove_scalar")]
        side["chain_ivc_steps_per_s"] = nx.get("zkvm_chain", {}).get("value")
    if side:
        line["side"] = side
    if "sharded_fold" in out:
        s = out["sharded_fold"] or {}
        line["sharded_fold"] = {k: s.get(k) for k in ("value", "unit", "ms_per_step", "verified", "comm_size", "error")
                                if k in s}
    if "pmc_files" in out:  # PMC figures are used only when collected on these kernel sources
        line["pmc_src_hash"] = out["pmc_files"]["src_hash"]
        line["pmc_stale"] = len(out["pmc_files"]["stale"])
    line["detail"] = detail
    line = _sig(line)
    txt = json.dumps(line, separators=(",", ":"))
    if len(txt) > LINE_LIMIT:  # never let the headline outgrow the driver's tail: drop the optional parts
        for k in ("side", "phases", "step_hbm"):
            line.pop(k, None)
            txt = json.dumps(line, separators=(",", ":"))
            if len(txt) <= LINE_LIMIT:
                break
    return txt


def emit(out, detail_path):
    """write the full record to `detail_path` (best effort) and print the compact headline line"""
    out["pmc_files"] = {"src_hash": kernel_source_hash(), "stale": sorted(_PMC_STALE)}
    detail = None
    if detail_path:
        try:
            p = Path(detail_path)
            if not p.is_absolute():
                p = ROOT / p
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(out) + "\n")
            detail = str(detail_path)
        except OSError as e:
            detail = f"not written: {e}"
    print(compact_line(out, detail), flush=True)


def main():
    args = parse()
    import torch
    import latticeum_amd as LA
    from latticeum_amd import dist as LD

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if os.environ.get("LATTICEUM_AMD_REHEARSE_ONE_GPU") == "1":
        # rehearsal of the N > 1 control flow on a one-GPU box: every rank on
        # cuda:0 and a gloo group (RCCL refuses two ranks on one GPU, so the
        # sharded fold reports its communicator error instead of a timing)
        local = 0
    torch.cuda.set_device(local)
    pg = LD.init(world)

    d, W, kappa = args.d, args.w, args.kappa
    wl = Workload(LA, torch, local, rank, d, W, kappa, args.streams, cu_partition=args.cu_partition,
                  cu_split=args.cu_split,
                  packed=None if args.packed is None else bool(args.packed), batch=args.batch)
    batched, group = wl.batch, wl.group
    warmup_run = warmup_steps(wl, args.warmup)
    K, L, N = wl.pr.K, wl.pr.L, wl.N
    detail = args.detail or (DETAIL_DEFAULT if args.full else None)
    dump = (lambda: dump_outputs(wl, torch, args.dump_outputs)) if args.dump_outputs and rank == 0 else None
    dt_max, (phases, roof) = measure(LA, torch, LD, pg, world, wl, args.steps, args.warmup, phases=args.full,
                                     after_timed=dump)
    wl.close()
    del wl
    torch.cuda.empty_cache()

    step_bytes, _, _ = algorithmic_bytes(d, W, kappa, L, K)
    out = None
    if rank == 0:
        cpu = None
        if args.full and args.cpu and world == 1:
            cpu = cpu_baseline(d, W, kappa)
        value = world * args.steps / dt_max
        out = {
            "metric": "fold-steps/sec (Ajtai commit+fold) at d=1024",
            "value": value, "unit": "fold-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "warmup_steps_run": warmup_run,
            "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u64 (Goldilocks mod-p integer)",
            "data": "synthetic (seeded SplitMix64 inputs, random Ajtai matrix)",
            "config": {"workload": f"commit+fold step, X^{d}+1 ring, w_ccs W={W}, N={N}, kappa={kappa}, "
                                   f"B=2^15 L=5 K=15, 29 Ajtai products in one pass over A; {EXCLUDED}",
                       "workload_short": f"configs[2] at d={d}: commit+fold step, X^{d}+1, W={W}, kappa={kappa}, "
                                         f"K=15; {EXCLUDED_SHORT}",
                       "d": d, "W": W, "N": N, "kappa": kappa,
                       "parallelism": f"{world} ranks x {args.streams} independent step streams (weak, "
                                      f"no collective on the data path)"
                                      + (f"; groups of {group} steps whose contractions are one launch "
                                         f"(one pass over A per group)" if batched else "")
                                      + (f"; each group's contraction on the last {args.cu_split} CUs, the step "
                                         f"streams on the others" if args.cu_split and batched else ""),
                       # BASELINE configs[3] names an "RCCL accumulator reduce": in LatticeFold
                       # that is the column-sharded fold's all-reduce of the partial commitments,
                       # timed in `sharded_fold` (N > 1); the independent step streams of `value`
                       # have nothing to reduce (summing unrelated accumulators has no meaning)
                       "configs3_reduce": ("the RCCL accumulator reduce of configs[3] is the column-sharded fold's "
                                           "mod-p all-reduce of the 29 partial commitments per step, timed in "
                                           "sharded_fold; value counts independent step streams (no collective)")
                       if world > 1 else None},
            "hbm_gbs_step_algorithmic": step_bytes * value / world / 1e9,
            "step_hbm": step_hbm(d, W, kappa, group if batched else 1, phases, value / world, L, K),
            # the dominant phase by device time per step (HIP events on the launch
            # stream, inside the timed region); bytes per SURVEY.md 8(d)
            "roofline": roof,
            "phases": phases,
            "cpu_baseline": cpu,
        }
    if args.full and args.small and args.d == 1024:
        ref = extra_shape(LA, torch, LD, pg, local, rank, world, 24, 19763, 32, 4, 128, 8,
                          "the reference ring Phi_72 = X^24 - X^12 + 1 at the real zkvm shape", batch=4)
        small = extra_shape(LA, torch, LD, pg, local, rank, world, 1024, 464, args.kappa, 4, 256, 16,
                            "X^1024+1 ring (byte-equivalent to the real zkvm step)", batch=2)
        c4 = extra_shape(LA, torch, LD, pg, local, rank, world, 4096, 1024, 64, 2, 20, 4,
                         "BASELINE configs[4]'s ring X^4096+1 with kappa=64", batch=2)
        ops = side_ops(LA, torch, local)
        nxt = next_rows(LA, torch, local, out.get("cpu_baseline") if out is not None else None)
        if out is not None:
            if args.cpu and world == 1:  # the reference ring's own CPU baseline (the oracle restatement)
                ref["cpu_baseline"] = cpu_baseline(24, 19763, 32)
            out["next_rows"] = nxt
            out["reference_ring"] = ref
            out["small_shape"] = small
            out["configs4_d4096_kappa64"] = c4
            out["side_ops"] = ops
    if args.full and world > 1:
        # the sharded fold is the only part with a collective on the data path
        # (its own RCCL communicator): a rank stuck in it must not cost the
        # headline line, so past SHARDED_LIMIT_S rank 0 prints the line with the
        # timeout recorded and every rank leaves (os._exit: no exec, no teardown
        # of a communicator that is still waiting on its peers)
        import threading

        def give_up():
            if out is not None:
                out["sharded_fold"] = {"error": f"timeout after {SHARDED_LIMIT_S} s"}
                emit(out, detail)
            sys.stderr.flush()
            os._exit(0)

        dog = threading.Timer(SHARDED_LIMIT_S, give_up)
        dog.daemon = True
        dog.start()
        try:
            sh = sharded_fold(LA, torch, LD, pg, local, rank, world, d, W, kappa, 5, 2)
        except Exception as e:  # reported, never fatal for the headline line
            sh = {"error": f"{type(e).__name__}: {e}"}
        dog.cancel()
        if out is not None:
            out["sharded_fold"] = sh
    if out is not None:
        emit(out, detail)
    LD.finalize(pg)
    return out


if __name__ == "__main__":
    main()
