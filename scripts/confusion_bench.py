#!/usr/bin/env python3
"""Cost of the confusion figures on one MI355X.

* ``kernel`` (a): the counting kernel's device time (the library's events
  around ``gpe_hit_group_counts``' launch, ``ctx.hit_group_ms()``) beside the
  hit-planes kernels' time (``gpe_last_timing``) of the same evaluation, at
  C5's shape — ``--trees`` (1,000,000) classifiers x 4,601 spambase-like rows,
  ``TypedConfusion`` — and at parity-6's, ``--trees`` x 64 cases,
  ``BooleanConfusion``.  The populations are 1/16 of ``--trees`` trees from the
  benchmark's generators (scripts/bench_configs.py: c5, c3) repeated 16 times:
  the kernels' work depends on the shape and, for the interpreter, on the
  trees' sizes, not on the trees being distinct.  One mask (the confusion
  call) and eight (``group_hits`` on random folds) are timed.  Read against
  the matrix's bytes over the 1.16 TB/s DESIGN 6.16 observed for the plane
  stores: ``fraction`` is bytes / ms / 1.16e9.
* ``route`` (b): tp and tn of ``--sample`` (16,384) classifiers x 4,601 rows by
  the only route the parent commit has — ``evaluate`` with
  ``TypedCaseHits(cases="device")``, ``last_case_hits()``, numpy on the host —
  against ``evaluate`` with ``TypedConfusion``; whole calls (host clock around
  calls that end in a device synchronise), alternating in one process after one
  warm-up each.  The two answers must be equal.

Run from the root of the tree on the GPU.  Prints one JSON line per part.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from deap_amd import configs, datasets  # noqa: E402
from deap_amd.evaluator import (BooleanConfusion, GPUEvaluator,  # noqa: E402
                                TypedCaseHits, TypedConfusion)

sys.path.insert(0, os.path.join(os.getcwd(), "scripts"))
import bench_configs  # noqa: E402

PLANE_STORE_BPS = 1.16e12          # the plane stores' observed rate
REPEAT = 16


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(runs):
    return {"runs_ms": [round(x, 4) for x in runs], "median_ms": round(statistics.median(runs), 4),
            "min_ms": round(min(runs), 4), "max_ms": round(max(runs), 4)}


def tiled_population(name, n):
    """(pset, spec, n trees): n / REPEAT trees of config *name*'s generator,
    repeated."""
    pset_name, data, gen, _, lo, hi, seed = bench_configs.CONFIGS[name]
    pset = configs.pset_for(pset_name)
    base = configs.population(pset, gen, max(1, n // REPEAT), seed, lo, hi)
    pop = (base * (n // len(base) + 1))[:n]
    return pset, configs.spec_for(pset_name, data), pop


def kernel_shape(label, ev, pop, reps):
    n_cases = ev.spec.n_cases
    units = (n_cases + 31) // 32
    nbytes = len(pop) * units * 4
    res = {"part": "kernel", "shape": label, "trees": len(pop), "cases": n_cases,
           "words_per_row": units, "matrix_MB": round(nbytes / 1e6, 1), "reps": reps}
    rng = np.random.default_rng(1)
    folds = rng.integers(0, 8, size=n_cases)[None, :] == np.arange(8)[:, None]
    planes, count1, count8, call8 = [], [], [], []
    for rep in range(reps + 1):
        ev.evaluate(pop)
        k = ev.ctx.timing()["kernel_ms"]
        c1 = ev.ctx.hit_group_ms()
        ms, got = timed(lambda: ev.group_hits(folds))
        c8 = ev.ctx.hit_group_ms()
        ok = got[:, 0] >= 0                           # (-1: an individual that raised)
        assert np.array_equal(got[ok].sum(1), ev.last_hits[ok])
        if rep:                                       # (rep 0: the warm-up)
            planes.append(k)
            count1.append(c1)
            count8.append(c8)
            call8.append(ms)
    res["hit_planes_kernel"] = stats(planes)
    res["count_1_mask_kernel"] = stats(count1)
    res["count_8_masks_kernel"] = stats(count8)
    res["group_hits_8_call"] = stats(call8)
    for key in ("count_1_mask_kernel", "count_8_masks_kernel"):
        ms = res[key]["median_ms"]
        res[key]["GBps"] = round(nbytes / ms / 1e6, 1)
        res[key]["fraction_of_plane_store_rate"] = round(nbytes / (ms * 1e-3) / PLANE_STORE_BPS, 3)
    print(json.dumps(res), flush=True)


def kernel_part(n, reps):
    pset, spec, pop = tiled_population("c5", n)
    ev = GPUEvaluator(pset, TypedConfusion(spec.X, spec.labels[0]), device=0)
    try:
        kernel_shape("c5", ev, pop, reps)
    finally:
        ev.close()
    del pop
    pset, _, pop = tiled_population("c3", n)
    ins, outs = datasets.parity6_table()
    ev = GPUEvaluator(pset, BooleanConfusion(ins, outs), device=0)
    try:
        kernel_shape("parity6", ev, pop, reps)
    finally:
        ev.close()


def route_part(n, reps):
    pset, spec, pop = tiled_population("c5", n * REPEAT)
    pop = pop[:n]                                       # (n distinct trees)
    X, lab = spec.X, spec.labels[0]
    pos = lab.astype(bool)
    old = GPUEvaluator(pset, TypedCaseHits(X, lab, cases="device"), device=0)
    new = GPUEvaluator(pset, TypedConfusion(X, lab, fitness=("tp", "tn")), device=0)
    res = {"part": "route", "trees": len(pop), "cases": spec.n_cases, "reps": reps}
    try:
        def old_route():
            old.evaluate(pop)
            mat = old.last_case_hits()
            return mat[:, pos].sum(1), mat[:, ~pos].sum(1)

        def new_route():
            new.evaluate(pop)
            return new.last_confusion[:, 0], new.last_confusion[:, 3]

        a, b = old_route(), new_route()                 # warm-up
        res["same_counts"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
        t_old, t_new = [], []
        for _ in range(reps):
            ms, _ = timed(old_route)
            t_old.append(ms)
            ms, _ = timed(new_route)
            t_new.append(ms)
        res["readback_and_numpy"] = stats(t_old)
        res["typed_confusion"] = stats(t_new)
        res["old_over_new"] = round(res["readback_and_numpy"]["median_ms"] /
                                    res["typed_confusion"]["median_ms"], 2)
        units = (spec.n_cases + 31) // 32
        res["d2h_bytes"] = {"readback": len(pop) * units * 4, "typed_confusion": len(pop) * 4}
    finally:
        old.close()
        new.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1000000)
    ap.add_argument("--sample", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--part", choices=("kernel", "route"), action="append")
    a = ap.parse_args()
    parts = a.part or ["kernel", "route"]
    if "route" in parts:
        route_part(a.sample, a.reps)
    if "kernel" in parts:
        kernel_part(a.trees, a.reps)
