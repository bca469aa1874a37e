#!/usr/bin/env python3
"""Cost of a case subset, on the ``unwrapped_ball`` configuration
at 10 variables x 2**20 resident cases with trig leaves on and 16,384 loaded
trees:

* ``subsample``: ``ev.subsample(idx)`` — the device gather, nothing reloaded;
* ``parent``: what the library offered for the same end before —
  ``ctx.set_cases(F, X[:, idx], y[idx])`` (host slice, upload, host bounds
  scan), ``set_trig_leaves(True)`` and loading the programs again,

for m in {256, 4096, 65536}: the same ``idx`` for both, interleaved, medians of
``--reps`` (default 25) repetitions after one warm-up each.  Then generations
of down-sampled automatic epsilon-lexicase, the workload the feature exists
for: ``subsample`` + ``evaluate`` + ``select_lexicase`` at 16,384 trees x 256
of 2**20 cases, ``--parents`` (default 32; 0: one per tree) selections
each — ``gpe_lexicase`` runs its selections in sequence, so that step's time
is linear in the count.  Run from the root of the tree to measure.  Prints
the table and the generations as they finish, then one JSON line.
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

from deap_amd import _lib, configs  # noqa: E402
from deap_amd.evaluator import (GPUEvaluator, SymbRegCaseAbsErrors,  # noqa: E402
                                SymbRegMSE)

SIZES = (256, 4096, 65536)


def ms_of(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def ab(pset, pop, X, y, reps):
    ev = GPUEvaluator(pset, SymbRegMSE(X, y), device=0)
    old = GPUEvaluator(pset, SymbRegMSE(X[:, :256], y[:256]), device=0)
    out = {}
    try:
        batch = ev.flatten(pop)
        ev.prepare(batch, pop)
        ev.run_batch(batch)
        old_batch = old.flatten(pop)
        n_cases = X.shape[1]

        def parent(idx):
            old.ctx.set_cases(_lib.GPE_MACHINE_F, np.ascontiguousarray(X[:, idx]),
                              np.ascontiguousarray(y[idx]))
            old.ctx.set_trig_leaves(True)
            old.ctx.load_programs(old_batch)

        for m in SIZES:
            rng = np.random.default_rng(m)
            sub, par = [], []
            for rep in range(reps + 1):
                idx = rng.integers(0, n_cases, m)
                a = ms_of(lambda: ev.subsample(idx))
                b = ms_of(lambda: parent(idx))
                if rep:                               # (rep 0: the warm-up)
                    sub.append(a)
                    par.append(b)
            assert ev.ctx.resident is batch and ev.case_uploads == 1
            out[m] = {"subsample_ms": statistics.median(sub), "parent_ms": statistics.median(par),
                      "subsample_min_max_ms": [min(sub), max(sub)],
                      "parent_min_max_ms": [min(par), max(par)],
                      "gathered_bytes": m * (X.shape[0] + 1) * 8}
    finally:
        ev.close()
        old.close()
    return out


def generation(pset, pop, X, y, reps, parents, m=256):
    """*parents*: how many parents each generation selects.  gpe_lexicase runs
    its selections one after another in one block, so its time is linear in
    that count; a generation that selects a parent per tree is the
    ``--parents 0`` run."""
    ev = GPUEvaluator(pset, SymbRegCaseAbsErrors(X, y, cases="device"), device=0)
    rows = {"subsample_ms": [], "evaluate_ms": [], "select_ms": [], "total_ms": []}
    raised = 0
    try:
        # (selection wants an error-free batch, as a run's survivors are: the
        # trees that raise on the warm-up's draw are left out)
        ev.subsample(random.Random(0).sample(range(ev.full_n_cases), m))
        pop = [t for t, r in zip(pop, ev.evaluate(pop)) if not isinstance(r, BaseException)]
        k = parents or len(pop)
        ev.select_lexicase(pop, min(k, 64), "automatic")        # warm-up
        print("generation: %d trees, %d parents per generation" % (len(pop), k), flush=True)
        for rep in range(1, reps + 1):
            random.seed(rep)
            idx = random.sample(range(ev.full_n_cases), m)
            a = ms_of(lambda: ev.subsample(idx))
            b = ms_of(lambda: ev.evaluate(pop))
            try:
                c = ms_of(lambda: ev.select_lexicase(pop, k, "automatic"))
            except (ValueError, OverflowError):       # a tree raised on this draw
                raised += 1
                continue
            print("  rep %d: subsample %.3f evaluate %.3f select %.3f ms" % (rep, a, b, c),
                  flush=True)
            for name, v in zip(rows, (a, b, c, a + b + c)):
                rows[name].append(v)
        assert ev.case_uploads == 1
    finally:
        ev.close()
    out = {name: statistics.median(v) if v else None for name, v in rows.items()}
    out.update(trees=len(pop), parents=k, generations=len(rows["total_ms"]),
               draws_with_a_raise=raised)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--trees", type=int, default=16384)
    ap.add_argument("--cases", type=int, default=2 ** 20)
    ap.add_argument("--only", choices=("ab", "generation"), help="one of the two parts")
    ap.add_argument("--parents", type=int, default=32,
                    help="parents selected per generation (0: one per tree)")
    ap.add_argument("--generations", type=int, default=5)
    a = ap.parse_args()
    pset, pop, X, Y = configs.headline_c4(pop=a.trees, cases=a.cases)
    y = np.ascontiguousarray(Y[0])
    res = {"trees": len(pop), "cases": a.cases, "reps": a.reps}
    if a.only != "generation":
        res["ab"] = ab(pset, pop, X, y, a.reps)
        print("%d trees loaded, %d resident cases x %d variables, trig leaves on; medians of %d"
              % (len(pop), a.cases, X.shape[0], a.reps))
        print("%8s %14s %14s %8s" % ("m", "subsample ms", "parent ms", "ratio"))
        for m, r in res["ab"].items():
            print("%8d %14.3f %14.3f %8.1f" % (m, r["subsample_ms"], r["parent_ms"],
                                               r["parent_ms"] / r["subsample_ms"]), flush=True)
    if a.only != "ab":
        g = res["generation"] = generation(pset, pop, X, y, a.generations, a.parents)
        print("one generation of down-sampled automatic epsilon-lexicase, %d trees x 256 of %d "
              "cases, %d parents (medians of %d):"
              % (g["trees"], a.cases, g["parents"], g["generations"]))
        if g["generations"]:
            print("  subsample %.3f ms + evaluate %.3f ms + select_lexicase %.3f ms = %.3f ms"
                  % (g["subsample_ms"], g["evaluate_ms"], g["select_ms"], g["total_ms"]))
    print(json.dumps(res), flush=True)
