#!/usr/bin/env python3
"""Cost of the per-case absolute errors: on the same headline
trees and cases, with the programs resident,

* ``plain``: ``gpe_run_abserr``, the summaries alone;
* ``resident``: ``gpe_run_abserr_cases`` with ``out_cases = NULL`` (the matrix
  stays on the device);
* ``host``: the same with the ``n x n_cases`` host copy;
* ``predict_route``: what a user had before — ``predict`` (which lowers the
  trees itself), ``abs(... - y)`` on the host, and an abs-error run for the
  summaries (``predict_alone``: its first step),

at 4,096 trees x 2**16 cases and at a lexicase-sized 16,384 trees x 4,096
cases.  Each figure is the median of five runs after one warm-up.  Run from
the root of the tree to measure.  Prints one JSON line per shape.

``--plain``: ``gpe_run_abserr`` alone at the three shapes of DESIGN 6.11 (the
headline with 11-column and with 31-column tiles, and the small shape): the
A/B of a build against its parent.  This mode uses nothing newer than
``SymbRegAbsError``, so the same file measures the parent from its own tree.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from deap_amd import configs  # noqa: E402
from deap_amd.evaluator import GPUEvaluator, SymbRegAbsError  # noqa: E402

FIELDS = ("programs", "P", "dbuf", "groups", "lds_bytes")


def median_ms(fn, reps=5):
    fn()                                    # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def launches(ctx):
    out = {}
    for k in ("abserr", "abserr_deep", "asm_fast", "asm_deep", "cpp_fast", "cpp_deep"):
        sh = ctx.launch_shape(k)
        if sh["programs"]:
            out[k] = {f: sh[f] for f in FIELDS}
    return out


def plain(n_pop, n_cases, reps, leaves):
    pset, pop, X, Y = configs.headline_c4(pop=65536, cases=n_cases)
    pop = pop[:n_pop]
    spec = SymbRegAbsError(X, Y[0], fitness=("mae", "max", "hits"))
    ev = GPUEvaluator(pset, spec, device=0, trig_leaves=leaves)
    res = {"mode": "plain", "trees": len(pop), "cases": n_cases, "trig_leaves": leaves}
    try:
        ev.prepare(ev.flatten(pop), pop)
        ms, runs = median_ms(lambda: ev.ctx.run_abserr(spec.hit_eps), reps)
        res["resident_abserr_ms"], res["resident_abserr_runs_ms"] = ms, runs
        res["launch"] = launches(ev.ctx)
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


def cost(n_pop, n_cases, reps):
    from deap_amd.evaluator import SymbRegCaseAbsErrors
    pset, pop, X, Y = configs.headline_c4(pop=65536, cases=n_cases)
    pop = pop[:n_pop]
    y = np.ascontiguousarray(Y[0])
    spec = SymbRegCaseAbsErrors(X, y, cases="device")
    ev = GPUEvaluator(pset, spec, device=0)
    res = {"mode": "cost", "trees": len(pop), "cases": n_cases,
           "matrix_MiB": len(pop) * n_cases * 8 / 2 ** 20}
    try:
        ev.prepare(ev.flatten(pop), pop)
        ctx, eps = ev.ctx, spec.hit_eps

        def predict_route():
            # (predict lowers and loads the trees itself; the abs-error run
            # then finds them resident, as the other runs here do)
            vals = ev.predict(pop, errors="nan", max_bytes=1 << 40)
            np.abs(np.subtract(vals, y[None, :], out=vals), out=vals)
            ctx.run_abserr(eps)
            return vals

        runs = (("plain", lambda: ctx.run_abserr(eps)),
                ("resident", lambda: ctx.run_abserr_cases(eps, n_cases, want_cases=False)),
                ("host", lambda: ctx.run_abserr_cases(eps, n_cases)),
                ("predict_route", predict_route),
                ("predict_alone", lambda: ev.predict(pop, errors="nan", max_bytes=1 << 40)),
                ("plain_again", lambda: ctx.run_abserr(eps)))   # (the session's drift)
        for name, fn in runs:
            res[name + "_ms"], res[name + "_runs_ms"] = median_ms(fn, reps)
            if name == "resident":
                res["launch"] = launches(ctx)
        res["resident_over_plain"] = res["resident_ms"] / res["plain_ms"]
        res["host_over_plain"] = res["host_ms"] / res["plain_ms"]
        res["host_copy_share"] = (res["host_ms"] - res["resident_ms"]) / res["host_ms"]
        res["predict_route_over_host"] = res["predict_route_ms"] / res["host_ms"]
        # the two routes give the same matrix
        a = ctx.run_abserr_cases(eps, n_cases)[0]
        b = predict_route()
        res["same_bits"] = bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", action="store_true",
                    help="gpe_run_abserr alone at the three shapes of DESIGN 6.11")
    ap.add_argument("--shape", choices=("small", "lexicase", "headline", "headline-leaves"),
                    action="append", help="only these shapes")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.plain:
        for name, args in (("headline", (65536, 2 ** 20, a.reps, False)),
                           ("headline-leaves", (65536, 2 ** 20, a.reps, True)),
                           ("small", (4096, 2 ** 16, a.reps, True))):
            if not a.shape or name in a.shape:
                plain(*args)
    else:
        for name, args in (("small", (4096, 2 ** 16, a.reps)),
                           ("lexicase", (16384, 4096, a.reps))):
            if not a.shape or name in a.shape:
                cost(*args)
