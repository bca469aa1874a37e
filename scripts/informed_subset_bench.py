#!/usr/bin/env python3
"""Cost of choosing an informed case subset: the device route,
``ev.informed_subsample(m, apply=False)`` on the per-case matrix the last
evaluation left on the GPU, against the host route it replaces — reading the
matrix back and running the numpy restatement of the definition
(``tests/informed_ref.py``):

* mux-11, 2,048 cases, ``BooleanCaseHits(cases="device")``, 164 and 16,384
  trees: host = ``ev.last_case_hits()`` + the traversal;
* a 10-variable regression, 65,536 cases, ``SymbRegCaseAbsErrors``, 164 trees:
  host = the ``n x n_cases`` copy of the matrix (a cases run with the host copy
  less one without, each timed in turn) + the threshold + the traversal.

m = 256 everywhere.  The two routes are interleaved, one warm-up each, medians
of ``--reps`` repetitions; each repetition draws a new seed and the two routes'
subsets are compared.  Run from the root of the tree.  Prints the table, then
one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))

import numpy as np  # noqa: E402

import informed_ref as ir  # noqa: E402
from deap_amd import configs, datasets  # noqa: E402
from deap_amd.evaluator import (BooleanCaseHits, GPUEvaluator,  # noqa: E402
                                SymbRegCaseAbsErrors)

M = 256
HIT_EPS = 0.5       # (random trees against unwrapped_ball: a hit rate away from 0 and 1)


def ms_of(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def med(v):
    return statistics.median(v)


def replayed_seed():
    twin = random.Random()
    twin.setstate(random.getstate())
    return twin.getrandbits(64)


def mux(n_trees, reps):
    ps = configs.pset_for("mux11")
    pop = configs.population(ps, "half", n_trees, 17, 2, 6)
    ins, outs = datasets.mux11_table()
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, "device"), device=0)
    dev, read, trav = [], [], []
    try:
        ev.evaluate(pop)
        for rep in range(reps + 1):
            random.seed(1000 + rep)
            seed = replayed_seed()
            a, idx = ms_of(lambda: ev.informed_subsample(M, apply=False))
            b, hit = ms_of(ev.last_case_hits)
            c, (want, dist) = ms_of(lambda: ir.informed_cases(hit, M, seed))
            assert idx.tolist() == want.tolist()
            assert ev.last_informed_distances.tolist() == dist.tolist()
            if rep:                                   # (rep 0: the warm-up)
                dev.append(a)
                read.append(b)
                trav.append(c)
    finally:
        ev.close()
    return {"problem": "mux11", "trees": n_trees, "cases": 2048, "m": M,
            "device_ms": med(dev), "device_min_max_ms": [min(dev), max(dev)],
            "host_read_ms": med(read), "host_traversal_ms": med(trav),
            "host_ms": med([x + y for x, y in zip(read, trav)]),
            "distinct_cases": int(len(np.unique(hit, axis=1).T)), "last_dist": int(dist[-1])}


def regression(n_trees, n_cases, reps):
    pset, pop, X, Y = configs.headline_c4(pop=4 * n_trees, cases=n_cases)
    y = np.ascontiguousarray(Y[0])
    ev = GPUEvaluator(pset, SymbRegCaseAbsErrors(X, y, hit_eps=HIT_EPS, cases="device"),
                      device=0)
    dev, run_host, run_dev, thr, trav = [], [], [], [], []
    try:
        # (the call wants an error-free batch, as a run's survivors are)
        pop = [t for t, r in zip(pop, ev.evaluate(pop)) if not isinstance(r, BaseException)]
        pop = pop[:n_trees]
        assert len(pop) == n_trees
        ev.evaluate(pop)
        for rep in range(reps + 1):
            random.seed(2000 + rep)
            seed = replayed_seed()
            a, idx = ms_of(lambda: ev.informed_subsample(M, apply=False))
            b, (E, _, _, _) = ms_of(lambda: ev.ctx.run_abserr_cases(HIT_EPS, n_cases, True))
            b0, _ = ms_of(lambda: ev.ctx.run_abserr_cases(HIT_EPS, n_cases, False))
            c, hit = ms_of(lambda: ir.threshold(E, HIT_EPS))
            d, (want, dist) = ms_of(lambda: ir.informed_cases(hit, M, seed))
            assert idx.tolist() == want.tolist()
            assert ev.last_informed_distances.tolist() == dist.tolist()
            if rep:
                dev.append(a)
                run_host.append(b)
                run_dev.append(b0)
                thr.append(c)
                trav.append(d)
    finally:
        ev.close()
    copy = med(run_host) - med(run_dev)
    return {"problem": "symreg10", "trees": n_trees, "cases": n_cases, "m": M,
            "device_ms": med(dev), "device_min_max_ms": [min(dev), max(dev)],
            "run_with_host_copy_ms": med(run_host), "run_resident_only_ms": med(run_dev),
            "host_read_ms": copy, "host_threshold_ms": med(thr), "host_traversal_ms": med(trav),
            "host_ms": copy + med(thr) + med(trav),
            "hit_rate": float(hit.mean()), "last_dist": int(dist[-1])}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal)")
    a = ap.parse_args()
    rows = []
    for n in ((20,) if a.small else (164, 16384)):
        rows.append(mux(n, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(regression(*((12, 300) if a.small else (164, 65536)), a.reps))
    print(json.dumps(rows[-1]), flush=True)
    print("m = %d, medians of %d (ms); host = read + threshold + traversal" % (M, a.reps))
    print("%-9s %6s %6s %10s %10s %10s %10s %8s" % ("problem", "trees", "cases", "device", "host",
                                                    "read", "traversal", "ratio"))
    for r in rows:
        print("%-9s %6d %6d %10.3f %10.3f %10.3f %10.3f %8.1f"
              % (r["problem"], r["trees"], r["cases"], r["device_ms"], r["host_ms"],
                 r["host_read_ms"], r["host_traversal_ms"], r["host_ms"] / r["device_ms"]))
    print(json.dumps({"reps": a.reps, "rows": rows}), flush=True)
