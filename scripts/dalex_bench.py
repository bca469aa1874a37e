#!/usr/bin/env python3
"""DALex selection and weighted error sums against what they replace
(DESIGN 3.21, 6.20), at the shape of scripts/lexicase_par_bench.py: the
``unwrapped_ball`` configuration, 16,384 trees (those that raise nothing are
kept), 256 subsampled cases, ``SymbRegCaseAbsErrors(cases="device")``,
``k = n`` selections.

* ``select``: whole ``select_dalex`` calls on the host clock (each ends in a
  stream synchronise) and the device time of their kernels
  (``gpe_last_dalex_ms``: fit rows, sigma, weights, product, fold), alternating
  in one session with ``select_lexicase(parallel=True)`` (``"automatic"``), one
  warm-up each, medians of ``--reps``.  Then the readback route: the matrix as
  a host-mode evaluation returns it, ``E @ W`` and ``argmin`` in numpy on the
  device's own weights; the copy itself is priced as the difference of a
  host-mode and a device-mode ``evaluate``.  The fp64 matrix rate is
  ``2 n C k`` over the kernels' time.
* ``sums``: ``weighted_errors`` with G = 1, 8 and 256 weight rows against
  ``E @ W.T`` in numpy on the read-back matrix.
* ``--only split``: one ``select_dalex`` call and nothing else, for a kernel
  trace.

Run from the root of the tree on the GPU.  Prints one JSON line per part and
appends them to profiles/dalex_bench.log.
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

from deap_amd import configs  # noqa: E402
from deap_amd.evaluator import GPUEvaluator, SymbRegCaseAbsErrors  # noqa: E402

# AMD's MI355X data sheet: 78.6 TFLOPS peak FP64 matrix
PEAK_FP64_MATRIX_TFLOPS = 78.6
LOG = os.path.join("profiles", "dalex_bench.log")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(routes, reps):
    for fn in routes.values():
        fn()
    runs = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            runs[name].append(timed(fn)[0])
    return runs


def summary(res, runs):
    for name, v in runs.items():
        res[name + "_ms"] = round(statistics.median(v), 3)
        res[name + "_runs_ms"] = [round(x, 3) for x in v]


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    with open(LOG, "a") as fh:
        fh.write(line + "\n")


def evaluators(a):
    """(device-mode evaluator, host-mode evaluator, error-free trees)."""
    pset, pop, X, Y = configs.headline_c4(pop=a.trees, cases=a.cases)
    idx = random.Random(0).sample(range(a.cases), 256)
    y = np.ascontiguousarray(Y[0])
    dev = GPUEvaluator(pset, SymbRegCaseAbsErrors(X, y, cases="device"), device=0)
    dev.subsample(idx)
    pop = [t for t, r in zip(pop, dev.evaluate(pop)) if not isinstance(r, BaseException)]
    host = GPUEvaluator(pset, SymbRegCaseAbsErrors(X, y, cases="host"), device=0)
    host.subsample(idx)
    return dev, host, pop


def main(a):
    dev, host, pop = evaluators(a)
    n, C = len(pop), 256
    try:
        dev.evaluate(pop)
        if a.only == "split":
            dev.select_dalex(pop, n, a.pressure)
            return
        if a.only in (None, "select"):
            res = {"part": "select", "trees": n, "cases": C, "k": n, "pressure": a.pressure,
                   "reps": a.reps}
            random.seed(1)
            kernel = []

            def dalex():
                dev.select_dalex(pop, n, a.pressure)
                kernel.append(dev.ctx.dalex_ms())

            runs = alternate({
                "dalex_call": dalex,
                "lexicase_par_call": lambda: dev.select_lexicase(pop, n, "automatic",
                                                                 parallel=True)}, a.reps)
            summary(res, runs)
            summary(res, {"dalex_kernels": kernel[1:]})
            first = []
            for _ in range(a.reps):                  # a call that has to transpose first
                dev.evaluate(pop)
                first.append(timed(lambda: dev.select_dalex(pop, n, a.pressure))[0])
            summary(res, {"dalex_call_after_evaluate": first})
            tf = 2.0 * n * C * n / (res["dalex_kernels_ms"] * 1e-3) / 1e12
            res["fp64_tflops_over_all_kernels"] = round(tf, 2)
            res["fraction_of_fp64_matrix_peak"] = round(tf / PEAK_FP64_MATRIX_TFLOPS, 3)
            res["peak_source"] = "AMD MI355X data sheet, 78.6 TFLOPS FP64 matrix"
            # the readback route
            ev_dev = [timed(lambda: dev.evaluate(pop))[0] for _ in range(a.reps)]
            ev_host, rows = [], None
            for _ in range(a.reps):
                ms, rows = timed(lambda: host.evaluate(pop))
                ev_host.append(ms)
            summary(res, {"evaluate_device_mode": ev_dev, "evaluate_host_mode": ev_host})
            E = np.asarray(rows, dtype=np.float64)
            dev.evaluate(pop)
            picks = dev.select_dalex(pop, n, a.pressure)
            seed = dev.last_dalex_seed
            wt = dev.ctx.dalex_weights(C, n, seed, a.pressure, dev.ctx.dalex_sigma(E))
            fit = np.isfinite(E).all(axis=1)

            def numpy_route():
                with np.errstate(invalid="ignore", over="ignore"):
                    S = E @ wt
                S[~fit] = np.inf
                return S.argmin(axis=0)

            runs = alternate({"numpy_product_argmin": numpy_route}, max(1, min(a.reps, 3)))
            summary(res, runs)
            got = np.array([id(t) for t in picks])
            ids = np.array([id(t) for t in pop])
            res["picks_equal_to_numpy_argmin"] = float((ids[numpy_route()] == got).mean())
            res["distinct_parents"] = len(set(got.tolist()))
            res["unfit_rows"] = int((~fit).sum())
            emit(res)
        if a.only in (None, "sums"):
            rows = host.evaluate(pop)
            E = np.asarray(rows, dtype=np.float64)
            dev.evaluate(pop)
            res = {"part": "sums", "trees": n, "cases": C, "reps": a.reps}
            for G in (1, 8, 256):
                W = np.random.default_rng(G).random((G, C))
                kernel = []

                def gpu():
                    dev.weighted_errors(W)
                    kernel.append(dev.ctx.dalex_ms())

                def cpu():
                    with np.errstate(invalid="ignore", over="ignore"):
                        return E @ W.T

                runs = alternate({"weighted_errors_G%d_call" % G: gpu,
                                  "numpy_G%d" % G: cpu}, a.reps)
                summary(res, runs)
                summary(res, {"weighted_errors_G%d_kernels" % G: kernel[1:]})
            emit(res)
    finally:
        dev.close()
        host.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trees", type=int, default=16384)
    ap.add_argument("--cases", type=int, default=2 ** 17)
    ap.add_argument("--pressure", type=float, default=3.0)
    ap.add_argument("--only", choices=("select", "sums", "split"))
    main(ap.parse_args())
