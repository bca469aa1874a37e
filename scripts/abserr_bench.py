#!/usr/bin/env python3
"""Cost of an abs-error run beside an MSE run and a linear-scaling run
(DESIGN 6.11): the same headline trees and cases through ``SymbRegMSE``,
``SymbRegScaledMSE`` and ``SymbRegAbsError``, at 4,096 trees x 2**16 cases
(``--small``, the default) and at the headline shape, 65,536 trees x 2**20
cases (``--headline``), in one session.  Each figure is the median of five
runs after one warm-up.  Run from the root of the tree to measure.  Prints one
JSON line per shape.

Resident: the programs stay loaded and only the run is timed (``gpe_run``,
``gpe_run_scaled``, ``gpe_run_abserr``).  Evaluate: ``GPUEvaluator.evaluate``
of the whole population, lowering included.  ``--no-trig-leaves``: no sin/cos
leaf columns, an 11-column tile instead of 31 (bench.py's own geometry).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

from deap_amd import _lib, configs  # noqa: E402
from deap_amd.evaluator import (GPUEvaluator, SymbRegAbsError, SymbRegMSE,  # noqa: E402
                                SymbRegScaledMSE)

FIELDS = ("programs", "P", "dbuf", "groups", "lds_bytes")


def median_ms(fn, reps=5):
    fn()                                    # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def shape(n_pop, n_cases, reps, leaves=True):
    pset, pop, X, Y = configs.headline_c4(pop=65536, cases=n_cases)
    pop = pop[:n_pop]
    res = {"trees": len(pop), "cases": n_cases, "trig_leaves": leaves}
    absspec = SymbRegAbsError(X, Y[0], fitness=("mae", "max", "hits"))
    scspec = SymbRegScaledMSE(X, Y[0])
    evs = {"mse": GPUEvaluator(pset, SymbRegMSE(X, Y), device=0, trig_leaves=leaves),
           "scaled": GPUEvaluator(pset, scspec, device=0, trig_leaves=leaves),
           "abserr": GPUEvaluator(pset, absspec, device=0, trig_leaves=leaves)}
    try:
        for ev in evs.values():
            ev.prepare(ev.flatten(pop), pop)
        runs = {"mse": lambda: evs["mse"].ctx.run(_lib.GPE_MODE_MSE),
                "scaled": lambda: evs["scaled"].ctx.run_scaled(scspec.sy, scspec.syy),
                "abserr": lambda: evs["abserr"].ctx.run_abserr(absspec.hit_eps)}
        for k in ("mse", "scaled", "abserr", "mse"):      # (MSE again: the session's drift)
            ms, all_ms = median_ms(runs[k], reps)
            again = "_again" if "resident_%s_ms" % k in res else ""
            res["resident_%s_ms%s" % (k, again)] = ms
            res["resident_%s_runs_ms%s" % (k, again)] = all_ms
        sh = evs["mse"].ctx.launch_shape("asm_fast")
        res["mse_launch"] = {f: sh[f] for f in FIELDS}
        for name, ev, keys in (("scaled", evs["scaled"], ("moments", "moments_deep")),
                               ("abserr", evs["abserr"], ("abserr", "abserr_deep"))):
            for k in keys + ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep"):
                sh = ev.ctx.launch_shape(k)
                if sh["programs"]:
                    res["%s_launch_%s" % (name, k)] = {f: sh[f] for f in FIELDS}
        res["abserr_over_mse"] = res["resident_abserr_ms"] / res["resident_mse_ms"]
        res["scaled_over_mse"] = res["resident_scaled_ms"] / res["resident_mse_ms"]
        res["abserr_over_scaled"] = res["resident_abserr_ms"] / res["resident_scaled_ms"]
        for k in ("mse", "abserr"):
            res["evaluate_%s_ms" % k], _ = median_ms(lambda: evs[k].evaluate(pop), reps)
        res["evaluate_ratio"] = res["evaluate_abserr_ms"] / res["evaluate_mse_ms"]
    finally:
        for ev in evs.values():
            ev.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trig-leaves", action="store_true",
                    help="no sin/cos leaf columns: an 11-column tile instead of 31")
    a = ap.parse_args()
    if a.small or not a.headline:
        shape(4096, 2 ** 16, a.reps, not a.no_trig_leaves)
    if a.headline:
        shape(65536, 2 ** 20, a.reps, not a.no_trig_leaves)
