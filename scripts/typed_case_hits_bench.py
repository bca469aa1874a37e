#!/usr/bin/env python3
"""Cost and use of the typed core's hit planes, on C5's shape
(scripts/bench_configs.py: spambase-like rows, ``genHalfAndHalf(1, 2)``
classifiers).

* ``kernels`` (a, b): one process holds three evaluators on the same batch —
  ``TypedBoolHits`` on the library given as ``--parent-lib`` (a build of the
  parent commit), ``TypedBoolHits`` on this tree's library, and
  ``TypedCaseHits(cases="device")`` — and runs them in turn, ``--reps`` rounds
  after one warm-up each.  Kernel ms are the library's device events around
  the interpreter kernels (``gpe_last_timing``).  Reported per evaluator: every
  run, the median, and min-max (the parent's min-max is the run-to-run spread
  the count-only difference is read against).  The counts of all three must be
  equal.
* ``percase`` (c): the per-case hits of ``--sample`` classifiers the way the
  parent commit offers — ``predict`` on the programs, compared with the labels
  on the host — against ``evaluate`` with ``cases="device"`` followed by
  ``last_case_hits()``; alternating, end to end (host clock around calls that
  end in a device synchronise).  The two matrices must be equal.
* ``select`` (d): one ``select_lexicase(pop, len(pop), parallel=True)`` and one
  ``informed_subsample(256, apply=False)`` on the same sample.

Run from the root of the tree on the GPU.  Prints one JSON line per part.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from deap_amd import _lib  # noqa: E402
from deap_amd.evaluator import GPUEvaluator, TypedBoolHits, TypedCaseHits  # noqa: E402

sys.path.insert(0, os.path.join(os.getcwd(), "scripts"))
import bench_configs  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def evaluator_on(lib_path, pset, spec):
    """An evaluator whose context lives in the library at *lib_path* (None:
    this tree's): the parent commit's build lacks the newer entry points, so
    only the ones it exports are bound."""
    if lib_path is None:
        return GPUEvaluator(pset, spec, device=0)
    mine = _lib.load()
    other = ctypes.CDLL(os.path.abspath(lib_path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(other, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    _lib._lib = other
    try:
        return GPUEvaluator(pset, spec, device=0)
    finally:
        _lib._lib = mine


def stats(runs):
    return {"runs_ms": [round(x, 4) for x in runs], "median_ms": round(statistics.median(runs), 4),
            "min_ms": round(min(runs), 4), "max_ms": round(max(runs), 4)}


def kernels_part(pset, spec, pop, parent_lib, reps):
    X, lab = spec.X, spec.labels[0]
    evs = [("count_this", evaluator_on(None, pset, TypedBoolHits(X, lab))),
           ("planes_this", evaluator_on(None, pset, TypedCaseHits(X, lab, cases="device")))]
    if parent_lib:
        evs.insert(0, ("count_parent", evaluator_on(parent_lib, pset, TypedBoolHits(X, lab))))
    res = {"part": "kernels", "trees": len(pop), "cases": spec.n_cases, "reps": reps}
    try:
        first = {name: ev.evaluate(pop) for name, ev in evs}              # warm-up
        res["same_counts"] = all(v == first["count_this"] for v in first.values())
        res["geometry"] = evs[-1][1].ctx.geometry()
        kern = {name: [] for name, _ in evs}
        e2e = {name: [] for name, _ in evs}
        for _ in range(reps):
            for name, ev in evs:
                out = None
                ms, out = timed(lambda: ev.evaluate(pop))
                e2e[name].append(ms)
                kern[name].append(ev.ctx.timing()["kernel_ms"])
        for name, _ in evs:
            res[name + "_kernel"] = stats(kern[name])
            res[name + "_evaluate"] = stats(e2e[name])
        units = (spec.n_cases + 31) // 32
        res["plane_matrix_MB"] = round(len(pop) * units * 4 / 1e6, 1)
        res["planes_minus_count_kernel_ms"] = round(
            res["planes_this_kernel"]["median_ms"] - res["count_this_kernel"]["median_ms"], 4)
        if parent_lib:
            res["count_this_minus_parent_kernel_ms"] = round(
                res["count_this_kernel"]["median_ms"] - res["count_parent_kernel"]["median_ms"], 4)
            res["parent_spread_ms"] = round(res["count_parent_kernel"]["max_ms"] -
                                            res["count_parent_kernel"]["min_ms"], 4)
    finally:
        for _, ev in evs:
            ev.close()
    print(json.dumps(res), flush=True)


def percase_part(pset, spec, pop, reps):
    X, lab = spec.X, spec.labels[0]
    want = lab.astype(bool)[None, :]
    ev = GPUEvaluator(pset, TypedCaseHits(X, lab, cases="device"), device=0)
    res = {"part": "percase", "trees": len(pop), "cases": spec.n_cases, "reps": reps}
    try:
        def new_route():
            ev.evaluate(pop)
            return ev.last_case_hits()

        def old_route():
            vals = ev.predict(pop, max_bytes=1 << 40)
            return (vals != 0) == want                     # (bool(nan) is True)

        a, b = new_route(), old_route()                    # warm-up
        res["same_matrix"] = bool(np.array_equal(a, b))
        t_new, t_old = [], []
        for _ in range(reps):
            ms, a = timed(new_route)
            t_new.append(ms)
            ms, b = timed(old_route)
            t_old.append(ms)
        res["planes"] = stats(t_new)
        res["predict"] = stats(t_old)
        res["predict_over_planes"] = round(res["predict"]["median_ms"] /
                                           res["planes"]["median_ms"], 2)
        units = (spec.n_cases + 31) // 32
        res["d2h_bytes"] = {"planes": len(pop) * units * 4,
                            "predict": len(pop) * spec.n_cases * 8}
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


def select_part(pset, spec, pop):
    X, lab = spec.X, spec.labels[0]
    ev = GPUEvaluator(pset, TypedCaseHits(X, lab, cases="device"), device=0)
    res = {"part": "select", "trees": len(pop), "cases": spec.n_cases}
    try:
        res["evaluate_ms"], _ = timed(lambda: ev.evaluate(pop))
        random.seed(5)
        ev.select_lexicase(pop, 2, parallel=True)          # warm-up (and the transposition)
        ev.informed_subsample(2, apply=False)
        random.seed(6)
        ms, picks = timed(lambda: ev.select_lexicase(pop, len(pop), parallel=True))
        res["select_lexicase_parallel_k_equals_n_ms"] = round(ms, 3)
        res["distinct_picks"] = len(set(id(x) for x in picks))
        ms, idx = timed(lambda: ev.informed_subsample(256, apply=False))
        res["informed_subsample_256_ms"] = round(ms, 3)
        res["informed_first_distances"] = ev.last_informed_distances[:4].tolist()
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None,
                    help="libgpeval.so built from the parent commit (part kernels, a)")
    ap.add_argument("--trees", type=int, default=None, help="default: C5's 1,000,000")
    ap.add_argument("--sample", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--part", choices=("kernels", "percase", "select"), action="append")
    a = ap.parse_args()
    parts = a.part or ["kernels", "percase", "select"]
    pset, spec, pop = bench_configs.population("c5")
    if a.trees:
        pop = pop[:a.trees]
    if "kernels" in parts:
        kernels_part(pset, spec, pop, a.parent_lib, a.reps)
    sample = pop[:a.sample]
    if "percase" in parts:
        percase_part(pset, spec, sample, max(3, a.reps // 2))
    if "select" in parts:
        select_part(pset, spec, sample)
