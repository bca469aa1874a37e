#!/usr/bin/env python3
"""NSGA-II selection on the GPU against the host mirror.

A random ``symbreg`` population is evaluated with ``SymbRegMSE.quartic()`` and
``size_objective=True``; its two objectives, error and size, both minimised,
are what ``tools.selNSGA2GPU`` selects ``k = n / 2`` individuals by.  Per size:

* ``call_ms``: whole ``selNSGA2GPU`` calls on the host clock (grouping by
  fitness in Python, upload, the kernels, one readback per front, crowding
  distances in numpy, the last front's ``sorted``), one warm-up, median of
  ``--reps``;
* ``nd_sort_call_ms`` / ``kernel_ms``: ``Context.nd_sort`` alone on the distinct
  rows, and the device time of its kernels (``gpe_last_nd_sort_ms``);
* ``fronts``, ``distinct_rows``: what the sort went through;
* at ``--host-size`` only: the host mirror ``tools.selNSGA2`` on the same
  individuals, once (it is quadratic in Python), and whether it selected the
  same individuals in the same order.

Individuals whose evaluation raised or gave nan are left out (a nan is an
argument error of the sort).  Run from the root of the tree on the GPU.
Prints one JSON line per size and appends it to profiles/nsga2_bench.log.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from deap_amd import base, configs, tools  # noqa: E402
from deap_amd.evaluator import GPUEvaluator, SymbRegMSE  # noqa: E402

LOG = os.path.join("profiles", "nsga2_bench.log")


class FitnessMulti(base.Fitness):
    weights = (-1.0, -1.0)


class Ind(object):
    def __init__(self, values):
        self.fitness = FitnessMulti(values)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def evaluated(n, seed):
    """n individuals carrying the (error, size) of evaluated random trees."""
    pset = configs.pset_for("symbreg")
    trees = configs.population(pset, "half", n, seed, 2, 6)
    ev = GPUEvaluator(pset, SymbRegMSE.quartic(), device=0, size_objective=True)
    try:
        fits = ev.evaluate(trees)
    finally:
        ev.close()
    return [Ind(f) for f in fits
            if not isinstance(f, BaseException) and not math.isnan(f[0])]


def main(a):
    pool = evaluated(max(a.sizes), a.seed)
    for n in a.sizes:
        pop = pool[:n]
        n, k = len(pop), len(pop) // 2
        res = {"n": n, "k": k, "objectives": 2, "reps": a.reps}
        chosen = tools.selNSGA2GPU(pop, k, device=0)         # warm-up
        calls = [timed(lambda: tools.selNSGA2GPU(pop, k, device=0))[0] for _ in range(a.reps)]
        ctx = tools._LEX_CTX[0]
        groups = {}
        for ind in pop:
            groups[ind.fitness.wvalues] = groups.get(ind.fitness.wvalues, 0) + 1
        w = np.asarray(list(groups), dtype=np.float64)
        mult = np.asarray(list(groups.values()), dtype=np.int32)
        sort_calls, kernels = [], []
        for _ in range(a.reps):
            sort_calls.append(timed(lambda: ctx.nd_sort(w, k, mult))[0])
            kernels.append(ctx.nd_sort_ms())
        res.update(distinct_rows=len(w), fronts=ctx.nd_sort_fronts(),
                   call_ms=round(statistics.median(calls), 3),
                   call_runs_ms=[round(x, 3) for x in calls],
                   nd_sort_call_ms=round(statistics.median(sort_calls), 3),
                   kernel_ms=round(statistics.median(kernels), 3),
                   kernel_runs_ms=[round(x, 3) for x in kernels])
        if n == a.host_size:
            ms, host = timed(lambda: tools.selNSGA2(pop, k))
            res["host_mirror_ms"] = round(ms, 1)
            res["host_mirror_selects_the_same"] = \
                [id(x) for x in host] == [id(x) for x in chosen]
        line = json.dumps(res)
        print(line, flush=True)
        with open(LOG, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+",
                    default=[4096, 16384, 65536, 1048576])
    ap.add_argument("--host-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    main(ap.parse_args())
