#!/usr/bin/env python3
"""Cost of a linear-scaling run beside an MSE run: the same
headline trees and cases through ``SymbRegMSE`` and ``SymbRegScaledMSE``, at
4,096 trees x 2**16 cases (``--small``, the default) and at the headline
shape, 65,536 trees x 2**20 cases (``--headline``).  Each figure is the median
of five runs after one warm-up.  Run from the root of the tree to measure.
Prints one JSON line per shape.

Resident: the programs stay loaded and only the run is timed (``gpe_run``
against ``gpe_run_scaled``).  Evaluate: ``GPUEvaluator.evaluate`` of the whole
population, lowering included.  The launch shapes of the scaled run are the
moments kernels' (``moments``, ``moments_deep``) and the rows route's last
values run; ``--max-gb`` sets the rows route's scratch budget
(``GPE_MOMENTS_MB``).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

from deap_amd import _lib, configs  # noqa: E402
from deap_amd.evaluator import GPUEvaluator, SymbRegMSE, SymbRegScaledMSE  # noqa: E402


def median_ms(fn, reps=5):
    fn()                                    # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def shape(n_pop, n_cases, max_gb, reps, leaves=True):
    pset, pop, X, Y = configs.headline_c4(pop=65536, cases=n_cases)
    pop = pop[:n_pop]
    res = {"trees": len(pop), "cases": n_cases, "max_gb": max_gb, "trig_leaves": leaves,
           "scratch_GB": len(pop) * n_cases * 8 / 1e9}
    mse = GPUEvaluator(pset, SymbRegMSE(X, Y), device=0, trig_leaves=leaves)
    spec = SymbRegScaledMSE(X, Y[0])
    keep = os.environ.get("GPE_MOMENTS_MB")
    if max_gb is not None:              # (read when the context is made)
        os.environ["GPE_MOMENTS_MB"] = str(int(max_gb * 1024))
    try:
        sc = GPUEvaluator(pset, spec, device=0, trig_leaves=leaves)
    finally:
        if max_gb is not None:
            os.environ.pop("GPE_MOMENTS_MB")
            if keep is not None:
                os.environ["GPE_MOMENTS_MB"] = keep
    try:
        for ev in (mse, sc):
            batch = ev.flatten(pop)
            ev.prepare(batch, pop)
        res["resident_mse_ms"], _ = median_ms(
            lambda: mse.ctx.run(_lib.GPE_MODE_MSE), reps)
        res["resident_mse_kernel_ms"] = mse.ctx.timing()["total_ms"]
        g = mse.ctx.geometry()
        res["mse_P"], res["mse_groups"] = g["P"], g["groups"]
        res["mse_dbuf"] = mse.ctx.launch_shape("asm_fast")["dbuf"]
        res["resident_scaled_ms"], _ = median_ms(
            lambda: sc.ctx.run_scaled(spec.sy, spec.syy), reps)
        for k in ("moments", "moments_deep", "asm_fast", "asm_deep", "cpp_fast", "cpp_deep"):
            sh = sc.ctx.launch_shape(k)
            res[k] = {f: sh[f] for f in ("programs", "P", "dbuf", "groups", "lds_bytes")}
        res["resident_ratio"] = res["resident_scaled_ms"] / res["resident_mse_ms"]
        res["evaluate_mse_ms"], _ = median_ms(lambda: mse.evaluate(pop), reps)
        res["evaluate_scaled_ms"], runs = median_ms(lambda: sc.evaluate(pop), reps)
        res["evaluate_scaled_runs_ms"] = runs
        res["evaluate_ratio"] = res["evaluate_scaled_ms"] / res["evaluate_mse_ms"]
    finally:
        mse.close()
        sc.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--max-gb", type=float, default=None,
                    help="scratch budget of the rows route (default: the library's)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trig-leaves", action="store_true",
                    help="no sin/cos leaf columns: an 11-column tile instead of 31")
    a = ap.parse_args()
    if a.small or not a.headline:
        shape(4096, 2 ** 16, a.max_gb, a.reps, not a.no_trig_leaves)
    if a.headline:
        shape(65536, 2 ** 20, a.max_gb, a.reps, not a.no_trig_leaves)
