#!/usr/bin/env python3
"""Cost of the case weights on one MI355X.

* ``kernel``: per shape, one evaluation leaves the hit matrix on the GPU and
  ``shared_hits``, ``weighted_hits`` with G = 1 and G = 8 and
  ``case_solve_counts`` then run on it ``--reps`` times in turn (one after the
  other inside every repetition, after one warm-up round of all four): the
  kernels' device time (the library's events, ``ctx.case_weights_ms()``) and
  the whole call (host clock around a call that ends in a device
  synchronise).  Shapes: C5's 4,601 spambase-like rows at ``--sample``
  (16,384) and ``--trees`` (1,048,576) classifiers, ``TypedCaseHits``, and
  parity-6's 64 cases at ``--trees``, ``BooleanCaseHits``.  The populations
  are 1/16 of the trees from the benchmark's generators
  (scripts/bench_configs.py: c5, c3) repeated 16 times: the kernels' work
  depends on the shape, not on the trees being distinct.  ``GBps`` is the
  matrix's bytes over the kernel time; ``dd_adds_per_s`` the double-double
  adds (one per case, row and weight row) over it.
* ``route``: at ``--sample`` x 4,601 the route a user has without these calls,
  in the same process and alternating with them: ``last_case_hits()`` (the bit
  matrix read back and unpacked), then ``H @ W.T`` and ``H.sum(0)`` in numpy,
  against ``weighted_hits(W)`` plus ``case_solve_counts()``; G = 1 and G = 8.
  The two answers must agree (counts equal, sums within 1e-12).

Run from the root of the tree on the GPU.  Prints one JSON line per part and
appends them to ``--log`` (profiles/case_weights_bench.log).
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
from deap_amd.evaluator import BooleanCaseHits, GPUEvaluator, TypedCaseHits  # noqa: E402

sys.path.insert(0, os.path.join(os.getcwd(), "scripts"))
import bench_configs  # noqa: E402

REPEAT = 16
LOG = None


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as fh:
            fh.write(line + "\n")


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
    rng = np.random.default_rng(1)
    w8 = rng.random((8, n_cases))
    calls = {"shared_hits": lambda: ev.shared_hits(),
             "weighted_hits_G1": lambda: ev.weighted_hits(w8[0]),
             "weighted_hits_G8": lambda: ev.weighted_hits(w8),
             "case_solve_counts": lambda: ev.case_solve_counts()}
    rows = {"shared_hits": 1, "weighted_hits_G1": 1, "weighted_hits_G8": 8}
    ev.evaluate(pop)
    kern = {k: [] for k in calls}
    call = {k: [] for k in calls}
    for rep in range(reps + 1):
        for k, fn in calls.items():
            ms, _ = timed(fn)
            if rep:                                     # (rep 0: the warm-up)
                call[k].append(ms)
                kern[k].append(ev.ctx.case_weights_ms())
    res = {"part": "kernel", "shape": label, "trees": len(pop), "cases": n_cases,
           "words_per_row": units, "matrix_MB": round(nbytes / 1e6, 1), "reps": reps}
    for k in calls:
        res[k] = {"kernel": stats(kern[k]), "call": stats(call[k])}
        ms = res[k]["kernel"]["median_ms"]
        res[k]["kernel"]["GBps"] = round(nbytes / ms / 1e6, 1)
        if k in rows:
            res[k]["kernel"]["dd_adds_per_s"] = float("%.3g" % (
                len(pop) * n_cases * rows[k] / (ms * 1e-3)))
    emit(res)


def route_part(ev, pop, reps):
    n_cases = ev.spec.n_cases
    rng = np.random.default_rng(2)
    w8 = rng.random((8, n_cases))
    ev.evaluate(pop)
    res = {"part": "route", "trees": len(pop), "cases": n_cases, "reps": reps}
    for G in (1, 8):
        w = w8[:G]

        def old_route():
            H = ev.last_case_hits()
            return H @ w.T, H.sum(0)

        def new_route():
            return ev.weighted_hits(w), ev.case_solve_counts()

        a, b = old_route(), new_route()                 # warm-up
        ok = bool(np.array_equal(a[1], b[1]) and
                  (np.abs(a[0] - b[0]) <= 1e-12 * np.abs(b[0])).all())
        t_old, t_new = [], []
        for _ in range(reps):
            ms, _ = timed(old_route)
            t_old.append(ms)
            ms, _ = timed(new_route)
            t_new.append(ms)
        res["G%d" % G] = {"same_answers": ok, "readback_and_numpy": stats(t_old),
                          "weighted_hits_and_counts": stats(t_new),
                          "old_over_new": round(statistics.median(t_old) /
                                                statistics.median(t_new), 2)}
    units = (n_cases + 31) // 32
    res["d2h_bytes"] = {"readback": len(pop) * units * 4,
                        "weighted_hits_G8_and_counts": len(pop) * 8 * 8 + n_cases * 4}
    emit(res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1048576)
    ap.add_argument("--sample", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log", default=os.path.join("profiles", "case_weights_bench.log"))
    a = ap.parse_args()
    LOG = a.log
    if LOG and os.path.exists(LOG):
        os.remove(LOG)
    pset, spec, pop = tiled_population("c5", a.trees)
    ev = GPUEvaluator(pset, TypedCaseHits(spec.X, spec.labels[0], cases="device"), device=0)
    try:
        small = pop[:a.sample]
        route_part(ev, small, a.reps)
        kernel_shape("c5_sample", ev, small, a.reps)
        kernel_shape("c5", ev, pop, a.reps)
    finally:
        ev.close()
    del pop
    pset, _, pop = tiled_population("c3", a.trees)
    ins, outs = datasets.parity6_table()
    ev = GPUEvaluator(pset, BooleanCaseHits(ins, outs, "device"), device=0)
    try:
        kernel_shape("parity6", ev, pop, a.reps)
    finally:
        ev.close()
