"""bench.py --full / --dump-outputs: a plain run times the steps and nothing
else (no phase pass), and the dump holds exactly the output buffers of the step
stream that ran the last timed step, the u64 words split into exact float64 halves."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

OUTPUTS = ("f_coeff", "f", "cm", "wk_0", "wk_1", "y_0", "y_1", "f0", "f0_coeff", "w_ccs0", "cm0")


def words(path):
    """the u64 words of a dumped file"""
    a = np.load(path)
    assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 2
    assert np.array_equal(a, np.floor(a)) and a.min() >= 0 and a.max() < 2.0 ** 32
    return a[:, 0].astype(np.uint64) | (a[:, 1].astype(np.uint64) << np.uint64(32))


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.detail is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "x"


def test_sample_index_is_fixed_by_its_seed():
    i = bench._sample_index(1000003, 4096, 7)
    assert i.dtype == np.int64 and len(i) == 4096 and i.min() >= 0 and i.max() < 1000003
    assert np.all(np.diff(i) >= 0) and len(np.unique(i)) > 4000
    assert np.array_equal(i, bench._sample_index(1000003, 4096, 7))
    assert not np.array_equal(i, bench._sample_index(1000003, 4096, 8))
    # SplitMix64's first output for seed 0
    assert int(bench._sample_index(1 << 63, 1, 0)[0]) == 0xE220A8397B1DCDAF % (1 << 63)


def test_dump_outputs_exact_and_sampled(tmp_path, monkeypatch):
    """host tensors in place of a workload's: every word comes back exactly (also
    above 2^63 and 2^53), a large output as its seeded sample"""
    import torch
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    rng = np.random.default_rng(5)
    u = lambda n: rng.integers(0, 1 << 64, n, dtype=np.uint64)
    host = {"f_coeff": u(200), "f": u(64), "cm": u(8), "fk_coeff": [None, None], "fk": [None, None],
            "wk": [u(65), u(3)], "y": [u(16), u(16)], "f0": u(200), "f0_coeff": u(1), "w_ccs0": u(40), "cm0": u(8),
            "planes": [u(10), None]}
    host["cm"][:2] = [0xFFFFFFFF00000000, (1 << 53) + 1]
    t = lambda v: None if v is None else torch.from_numpy(v.view(np.int64))
    keep = {k: [t(x) for x in v] if isinstance(v, list) else t(v) for k, v in host.items()}
    other = {k: [None if x is None else torch.zeros_like(x) for x in v] if isinstance(v, list) else torch.zeros_like(v)
             for k, v in keep.items()}
    wl = SimpleNamespace(keeps=[other, keep], last_stream=1)
    bench.dump_outputs(wl, torch, tmp_path / "d")
    names = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert names == sorted(f"{n}.npy" for n in OUTPUTS + ("planes_0",))
    assert np.array_equal(words(tmp_path / "d" / "cm.npy"), host["cm"])
    assert np.array_equal(words(tmp_path / "d" / "wk_1.npy"), host["wk"][1])
    assert np.array_equal(words(tmp_path / "d" / "f.npy"), host["f"])  # DUMP_SAMPLE words: still whole
    order = ["f_coeff", "f", "cm", "wk_0", "wk_1", "y_0", "y_1", "f0", "f0_coeff", "w_ccs0", "cm0", "planes_0"]
    for name, full in (("f_coeff", host["f_coeff"]), ("wk_0", host["wk"][0]), ("f0", host["f0"])):
        idx = bench._sample_index(len(full), 64, bench.DUMP_SEED + order.index(name))
        assert np.array_equal(words(tmp_path / "d" / f"{name}.npy"), full[idx]), name


@pytest.mark.gpu
@pytest.mark.parametrize("steps,last", [(5, 0), (4, 3), (6, 1), (3, 2)])
def test_plain_measure_dumps_the_last_timed_step(tmp_path, steps, last):
    """4 step streams in groups of 2 at the W = 464 shape: measure(phases=False)
    runs `steps` timed steps and no phase pass, and the dump taken right after them
    is the output set of the stream that ran the last one (whole groups, a last
    group of one as a single step, a wrap to the first group)"""
    import torch
    import latticeum_amd as LA
    from latticeum_amd import dist as LD
    wl = bench.Workload(LA, torch, 0, 0, 1024, 464, 32, 4, batch=2)
    try:
        seen = []
        dt, (phases, roof) = bench.measure(
            LA, torch, LD, None, 1, wl, steps, 2, phases=False,
            after_timed=lambda: (seen.append(wl.last_stream), bench.dump_outputs(wl, torch, tmp_path)))
        assert dt > 0 and phases == {} and roof is None
        assert seen == [last]
        assert all(c.phase_stats(p)[1] == 0 for c in wl.ctxs for p in c.PHASES), "no phase was timed"
        keep = wl.keeps[last]
        order = list(OUTPUTS) + ["planes_0", "planes_1"]
        assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{n}.npy" for n in order)
        for k, name in enumerate(order):
            t = keep[name[:-2]][int(name[-1])] if name[-2:] in ("_0", "_1") else keep[name]
            full = t.cpu().numpy().view(np.uint64)
            if len(full) > bench.DUMP_SAMPLE:
                full = full[bench._sample_index(len(full), bench.DUMP_SAMPLE, bench.DUMP_SEED + k)]
            assert np.array_equal(words(tmp_path / f"{name}.npy"), full), name
        # the streams hold different witnesses, so the dump identifies its stream
        other = 0 if last else 1  # a stream that has also run
        assert not torch.equal(keep["f0"], wl.keeps[other]["f0"])
    finally:
        wl.close()
        del wl
        torch.cuda.empty_cache()
