"""Time lf_dev_crt and lf_dev_icrt at every supported X^d + 1 degree over the same
2^26 words (n = 2^26 / d ring elements, 512 MiB in place), so the degrees compare
on equal traffic: each call reads and writes the buffer once, 2 x 8 x 2^26 bytes.

Device events around each call on the context's stream; 3 warm-up calls, then the
median of 10, per degree and direction. d = 1024 runs the register kernel
(kernels_n32.hip), every other degree the LDS Stockham family (ring.hpp
stockham4: radix-4 passes, one radix-2 pass in front when log2 d is odd), so the
4^k degrees in the same run are the comparison for the 2 4^k ones. Prints one
JSON document (ms and TB/s per degree, stamped with bench.py's kernel_source_hash)
and a markdown table; --out also writes the JSON to a file. Nothing is asserted
on the numbers.
usage: python tools/ntt_degrees.py [--log2-words 26] [--out profiles/ntt_degrees.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import latticeum_amd as LA  # noqa: E402
from bench import kernel_source_hash  # noqa: E402

WARMUP, RUNS = 3, 10


def time_call(fn, stream):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-words", type=int, default=26, help="u64 words per call (a smaller value rehearses the tool)")
    ap.add_argument("--out", default=None, help="also write the JSON document here")
    a = ap.parse_args()
    words = 1 << a.log2_words
    degrees = [d for d in sorted(LA.SUPPORTED_D) if d != 24 and LA.ring_supported(d)]
    ctx = LA.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    buf = torch.empty(words, dtype=torch.int64, device="cuda")
    ctx.dev_fill_uniform(buf, 26)
    ctx.sync()
    nbytes = 2 * 8 * words  # one read and one write of every word
    rows = []
    for d in degrees:
        row = {"d": d, "n": words // d}
        for name, fn in (("crt", ctx.dev_crt), ("icrt", ctx.dev_icrt)):
            ms = time_call(lambda: fn(buf, d), stream)
            med = statistics.median(ms)
            row[name] = {"ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                         "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
        rows.append(row)
    ctx.close()
    doc = {"tool": "tools/ntt_degrees.py", "kernel_source_hash": kernel_source_hash(),
           "device": torch.cuda.get_device_name(0), "words": words, "bytes_per_call": nbytes, "warmup": WARMUP,
           "runs": RUNS, "statistic": "median of the runs' device-event times", "degrees": rows}
    print(json.dumps(doc))
    print("| d | n | crt ms | crt TB/s | icrt ms | icrt TB/s |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['d']} | {r['n']} | {r['crt']['ms']:.3f} | {r['crt']['tb_per_s']:.2f} | {r['icrt']['ms']:.3f} | "
              f"{r['icrt']['tb_per_s']:.2f} |")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
