"""bench.py's command line: a plain run times the headline only, ``--full``
adds the side measurements, ``--dump-outputs DIR`` writes what the timed path
left in the caller's buffers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

FULL_ONLY = ("parity_sample", "trig_leaves", "fp32", "side_configs",
             "c3_sharded", "evolved", "deep_core", "cpu_baseline")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 5, 2)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"


def _buffers(n):
    import torch
    rng = np.random.default_rng(1)
    hi = rng.standard_normal(n)
    hi[::7] = np.nan
    lo = rng.standard_normal(n) * 2.0 ** -53
    err = rng.integers(0, 2 ** 20, n)
    err[::5] = -1                              # "no error": all ones
    flags = rng.integers(0, 8, n).astype(np.int32)
    return (hi, lo, err, flags), tuple(torch.from_numpy(a)
                                       for a in (hi, lo, err, flags))


def test_dump_outputs_writes_the_four_buffers_as_float64(tmp_path):
    (hi, lo, err, flags), t = _buffers(1000)
    bench.dump_outputs(str(tmp_path / "d"), *t)
    got = {f[:-4]: np.load(tmp_path / "d" / f)
           for f in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["err", "flags", "hi", "lo"]
    assert all(a.dtype == np.float64 and a.shape == (1000,)
               for a in got.values())
    assert (got["hi"].view(np.uint64) == hi.view(np.uint64)).all()
    assert (got["lo"] == lo).all() and (got["flags"] == flags).all()
    assert (got["err"] == err.view(np.uint64).astype(np.float64)).all()


def test_dump_outputs_samples_past_the_size_limit(tmp_path, monkeypatch):
    (hi, _, _, flags), t = _buffers(1000)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 5 * 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), *t)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["err.npy", "flags.npy", "hi.npy", "index.npy",
                         "lo.npy"]
    assert sum(v.nbytes for v in a.values()) <= 8 * 5 * 100
    idx = a["index.npy"].astype(np.int64)
    assert len(idx) == 100 and (np.diff(idx) > 0).all()
    assert (a["flags.npy"] == flags[idx]).all()
    assert (a["hi.npy"].view(np.uint64) == hi[idx].view(np.uint64)).all()
    for f in a:                                # the same sample every run
        assert (a[f].view(np.uint64) == b[f].view(np.uint64)).all()


def _run_bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--gpus", "1", "--pop", "600", "--cases", "50000",
                        "--min-depth", "2", "--max-depth", "5"] + list(argv),
                       stdout=subprocess.PIPE, timeout=120, check=True)
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    """A plain run reports the headline fields and none of the ``--full``
    legs; its dump is what ``Context.run`` returns for the same workload."""
    from deap_amd import _lib, configs
    from deap_amd.flatten import Flattener
    out = tmp_path / "dump"
    r = _run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype",
              "ms_per_step"):
        assert k in r
    assert (r["steps"], r["warmup"], r["dtype"]) == (3, 1, "f64")
    assert r["ms_per_step"] > 0
    work = r["config"]["node_evals_per_step"]
    assert r["value"] == pytest.approx(work / r["ms_per_step"] / 1e6,
                                       rel=2e-2)
    assert not [k for k in FULL_ONLY if k in r] and "cold" not in r["e2e"]
    pset, trees, X, y = configs.headline_c4(600, 50000, 2024, 2, 5)
    ctx = _lib.Context(0)
    ctx.set_cases(_lib.GPE_MACHINE_F, X, y)
    ctx.load_programs(Flattener(pset).flatten(trees))
    ref = ctx.run(_lib.GPE_MODE_MSE)
    ctx.close()
    assert sorted(os.listdir(out)) == ["err.npy", "flags.npy", "hi.npy",
                                       "lo.npy"]
    for name, a in zip(("hi", "lo", "err", "flags"), ref):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == (600,)
        assert (got.view(np.uint64) ==
                a.astype(np.float64).view(np.uint64)).all(), name


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements():
    r = _run_bench("--full", "--no-side-configs", "--no-cpu-baseline",
                   "--steps", "1", "--warmup", "1")
    assert r["trig_leaves"]["value"] > 0 and r["fp32"]["dtype"] == "f32"
    assert r["steps"] == 1 and r["dtype"] == "f64"
