#!/usr/bin/env python3
"""Parallel against replaying lexicase selection: whole
``select_lexicase`` calls on the host clock (each ends in a stream
synchronise), the two routes alternating in one session, one warm-up each,
medians of ``--reps`` (default 5).

* ``regression``: the shape of profiles/case_subset_bench_ab.log — the
  ``unwrapped_ball`` configuration, 16,384 trees, 256 subsampled of 2**20
  resident cases, ``SymbRegCaseAbsErrors(cases="device")``, ``"automatic"``
  mode.  Replaying and parallel at ``k = 32``; parallel alone at ``k = n`` (the
  replaying route selects in sequence and is not waited for there), its first
  call after an evaluation (which transposes the matrix) apart from the later
  ones (which find the transposed copy).
* ``bits``: the 11-multiplexer (2,048 cases), 16,384 ``genFull(2, 4)`` trees,
  ``BooleanCaseHits(cases="device")``.  Replaying and parallel at ``k = 64``;
  parallel alone at ``k = n``.
* ``--only split``: one parallel ``k = n`` call per shape after a fresh
  evaluation and nothing else, for a kernel trace (transposition, stats and
  selection kernels apart).

Run from the root of the tree on the GPU.  Prints one JSON line per part.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from deap_amd import configs, datasets, gp  # noqa: E402
from deap_amd.evaluator import (BooleanCaseHits, GPUEvaluator,  # noqa: E402
                                SymbRegCaseAbsErrors)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(routes, reps):
    """``{name: [ms] * reps}`` of the calls in *routes*, alternating, after one
    warm-up each."""
    for fn in routes.values():
        fn()
    runs = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            runs[name].append(timed(fn)[0])
    return runs


def summary(res, runs):
    for name, v in runs.items():
        res[name + "_ms"] = statistics.median(v)
        res[name + "_runs_ms"] = [round(x, 3) for x in v]


def regression_evaluator(n_trees, n_cases, m):
    pset, pop, X, Y = configs.headline_c4(pop=n_trees, cases=n_cases)
    ev = GPUEvaluator(pset, SymbRegCaseAbsErrors(X, np.ascontiguousarray(Y[0]), cases="device"),
                      device=0)
    # (selection wants an error-free batch, as a run's survivors are)
    ev.subsample(random.Random(0).sample(range(ev.full_n_cases), m))
    pop = [t for t, r in zip(pop, ev.evaluate(pop)) if not isinstance(r, BaseException)]
    ev.evaluate(pop)
    return ev, pop


def regression(a, split=False):
    ev, pop = regression_evaluator(a.trees, a.cases, 256)
    n = len(pop)
    res = {"part": "regression", "trees": n, "cases": 256, "of": a.cases, "mode": "automatic",
           "k_small": 32, "k_large": n, "reps": a.reps}
    try:
        if split:
            ev.select_lexicase(pop, n, "automatic", parallel=True)
            return
        random.seed(1)
        runs = alternate({
            "serial_k32": lambda: ev.select_lexicase(pop, 32, "automatic"),
            "parallel_k32": lambda: ev.select_lexicase(pop, 32, "automatic", parallel=True),
        }, a.reps)
        summary(res, runs)
        runs = alternate({
            "parallel_kn": lambda: ev.select_lexicase(pop, n, "automatic", parallel=True)},
            a.reps)
        summary(res, runs)
        # a call that has to transpose first: the one after an evaluation
        first = []
        for _ in range(a.reps):
            ev.evaluate(pop)
            first.append(timed(lambda: ev.select_lexicase(pop, n, "automatic",
                                                          parallel=True))[0])
        summary(res, {"parallel_kn_after_evaluate": first})
        picks = ev.select_lexicase(pop, n, "automatic", parallel=True)
        res["distinct_parents_of_k_large"] = len({id(x) for x in picks})
        res["parallel_below_serial_at_k_small"] = res["parallel_k32_ms"] < res["serial_k32_ms"]
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


def bits(a, split=False):
    ps = configs.pset_for("mux11")
    random.seed(11)
    pop = [gp.PrimitiveTree(gp.genFull(ps, 2, 4)) for _ in range(a.trees)]
    ins, outs = datasets.mux11_table()
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, cases="device"), device=0)
    n = len(pop)
    res = {"part": "bits", "trees": n, "cases": int(ins.shape[1]), "k_small": 64, "k_large": n,
           "reps": a.reps}
    try:
        ev.evaluate(pop)
        if split:
            ev.select_lexicase(pop, n, parallel=True)
            return
        random.seed(1)
        runs = alternate({
            "serial_k64": lambda: ev.select_lexicase(pop, 64),
            "parallel_k64": lambda: ev.select_lexicase(pop, 64, parallel=True),
        }, a.reps)
        summary(res, runs)
        runs = alternate({"parallel_kn": lambda: ev.select_lexicase(pop, n, parallel=True)},
                         a.reps)
        summary(res, runs)
        picks = ev.select_lexicase(pop, n, parallel=True)
        res["distinct_parents_of_k_large"] = len({id(x) for x in picks})
        res["parallel_below_serial_at_k_small"] = res["parallel_k64_ms"] < res["serial_k64_ms"]
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trees", type=int, default=16384)
    ap.add_argument("--cases", type=int, default=2 ** 20)
    ap.add_argument("--only", choices=("regression", "bits", "split"))
    a = ap.parse_args()
    if a.only in (None, "regression", "split"):
        regression(a, split=a.only == "split")
    if a.only in (None, "bits", "split"):
        bits(a, split=a.only == "split")
