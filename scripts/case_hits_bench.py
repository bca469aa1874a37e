#!/usr/bin/env python3
"""Cost of the per-case hit planes and of lexicase selection on them (DESIGN
6.13): the 11-multiplexer (2,048 cases), 16,384 ``genFull(2, 4)`` trees.

* ``evaluate``: ``GPUEvaluator.evaluate`` with ``BooleanCaseHits(cases=
  "device")`` against ``BooleanHits`` on the same batch, alternating, the
  median of ``--reps`` runs after one warm-up each (end to end, and the
  kernels' device time): what storing the planes costs.
* ``select``: ``select_lexicase(pop, k)`` on the resident bit matrix against
  the route there was before — ``predict``, the comparison with the outputs on
  the host, one tuple of ``n_cases`` values per individual,
  ``tools.selLexicaseGPU`` (which uploads them as doubles) — alternating, at
  ``--k-old`` selections (the double kernel gathers one value per candidate
  and case, so ``k = n`` of it is not waited for), then the new route alone at
  ``k = n``.  Both routes are seeded alike and must pick the same individuals.
* the bytes each route moves over PCIe, computed from the shapes;
* one ``select_lexicase`` in ``"automatic"`` mode at 65,536 individuals, which
  the double kernel refuses (16,384 at most).

Run from the root of the tree on the GPU.  Prints one JSON line per part.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from deap_amd import configs, datasets, gp, tools  # noqa: E402
from deap_amd.evaluator import BooleanCaseHits, BooleanHits, GPUEvaluator  # noqa: E402

MT_STATE_BYTES = 625 * 4


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def trees(n, seed=11):
    ps = configs.pset_for("mux11")
    random.seed(seed)
    return ps, [gp.PrimitiveTree(gp.genFull(ps, 2, 4)) for _ in range(n)]


def evaluate_part(n, reps):
    ps, pop = trees(n)
    ins, outs = datasets.mux11_table()
    new = GPUEvaluator(ps, BooleanCaseHits(ins, outs, cases="device"), device=0)
    old = GPUEvaluator(ps, BooleanHits(ins, outs), device=0)
    res = {"part": "evaluate", "trees": n, "cases": int(ins.shape[1])}
    try:
        a, b = new.evaluate(pop), old.evaluate(pop)          # warm-up
        res["same_counts"] = a == b
        t = {"case_hits": [], "hits": []}
        kern = {"case_hits": [], "hits": []}
        for _ in range(reps):
            for name, ev in (("case_hits", new), ("hits", old)):
                ms, _ = timed(lambda: ev.evaluate(pop))
                t[name].append(ms)
                kern[name].append(ev.ctx.timing()["total_ms"])
        for name in t:
            res[name + "_ms"] = statistics.median(t[name])
            res[name + "_runs_ms"] = t[name]
            res[name + "_kernel_ms"] = statistics.median(kern[name])
        res["case_hits_over_hits"] = res["case_hits_ms"] / res["hits_ms"]
        res["plane_matrix_MiB"] = n * ((ins.shape[1] + 31) // 32) * 4 / 2 ** 20
    finally:
        new.close()
        old.close()
    print(json.dumps(res), flush=True)


def select_part(n, k_old, reps):
    ps, pop = trees(n)
    ins, outs = datasets.mux11_table()
    nc = int(ins.shape[1])
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, cases="device"), device=0)
    res = {"part": "select", "trees": n, "cases": nc, "k_old": k_old}
    try:
        ev.evaluate(pop)
        want = outs.astype(bool)[None, :]

        def new_route(k, seed):
            random.seed(seed)
            return [id(x) for x in ev.select_lexicase(pop, k, "plain")]

        def old_route(k, seed):
            hit = ev.predict(pop, max_bytes=1 << 40) == want
            inds = [SimpleNamespace(fitness=SimpleNamespace(values=row, weights=(1.0,) * nc),
                                    tree=t)
                    for row, t in zip(map(tuple, hit.astype(np.int64).tolist()), pop)]
            random.seed(seed)
            return [id(x.tree) for x in tools.selLexicaseGPU(inds, k, device=0)]

        new_route(2, 0), old_route(2, 0)                     # warm-up
        ev.evaluate(pop)                                      # (predict reloaded the programs)
        t_new, t_old, same = [], [], True
        for r in range(reps):
            ms, a = timed(lambda: new_route(k_old, 100 + r))
            t_new.append(ms)
            ms, b = timed(lambda: old_route(k_old, 100 + r))
            t_old.append(ms)
            same = same and a == b
            ev.evaluate(pop)
        res.update(new_ms=statistics.median(t_new), new_runs_ms=t_new,
                   old_ms=statistics.median(t_old), old_runs_ms=t_old, same_picks=same)
        ms, picks = timed(lambda: new_route(n, 7))
        res["new_k_equals_n_ms"] = ms
        res["new_k_equals_n_distinct_picks"] = len(set(picks))
        # bytes over PCIe per route (selection only; the programs are resident)
        units = (nc + 31) // 32
        res["new_pcie_bytes"] = {"h2d": MT_STATE_BYTES, "d2h": MT_STATE_BYTES + 4 * k_old + 8}
        res["old_pcie_bytes"] = {"d2h_predict_planes": n * units * 4,
                                 "h2d_values_as_doubles": n * nc * 8,
                                 "h2d_other": MT_STATE_BYTES + nc,
                                 "d2h_other": MT_STATE_BYTES + 4 * k_old + 8}
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


def large_part(n, k):
    ps, pop = trees(n, seed=12)
    ins, outs = datasets.mux11_table()
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, cases="device"), device=0)
    res = {"part": "large", "trees": n, "cases": int(ins.shape[1]), "k": k, "mode": "automatic"}
    try:
        res["evaluate_ms"], _ = timed(lambda: ev.evaluate(pop))
        random.seed(5)
        ev.select_lexicase(pop, 2, "automatic")               # warm-up (and the transposition)
        random.seed(5)
        res["select_ms"], picks = timed(lambda: ev.select_lexicase(pop, k, "automatic"))
        res["distinct_picks"] = len(set(id(x) for x in picks))
    finally:
        ev.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=16384)
    ap.add_argument("--k-old", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--large", type=int, default=65536)
    ap.add_argument("--large-k", type=int, default=1024)
    ap.add_argument("--part", choices=("evaluate", "select", "large"), action="append")
    a = ap.parse_args()
    parts = a.part or ["evaluate", "select", "large"]
    if "evaluate" in parts:
        evaluate_part(a.trees, a.reps)
    if "select" in parts:
        select_part(a.trees, a.k_old, a.reps)
    if "large" in parts:
        large_part(a.large, a.large_k)
