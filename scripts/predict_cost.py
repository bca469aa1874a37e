#!/usr/bin/env python3
"""Cost of a values run: the first 4,096 headline trees at 2**16
cases.  Run from the root of the tree to measure (it imports that tree's
deap_amd): run_cases of a SymbRegCaseErrors evaluator, and where the build has
them run_values, run_values_device and predict.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

from deap_amd import _lib, configs
from deap_amd.evaluator import GPUEvaluator, SymbRegCaseErrors

pset, pop, X, Y = configs.headline_c4(pop=65536, cases=2 ** 16)
pop = pop[:4096]
n, nc = len(pop), X.shape[1]
gb = n * nc * 8 / 1e9
res = {"tree": os.getcwd(), "n": n, "cases": nc, "output_GB": gb}
ev = GPUEvaluator(pset, SymbRegCaseErrors(X, Y), device=0)
batch = ev.flatten(pop)
ev.prepare(batch, pop)


def timed(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


rc = timed(lambda: ev.ctx.run_cases(ev.spec.mode, nc))
res["run_cases_ms"] = rc
res["run_cases_kernel_ms"] = ev.ctx.timing()["total_ms"]
res["run_cases_GBps"] = gb / (min(rc) / 1e3)
if hasattr(ev.ctx, "run_values"):
    import torch
    out = np.empty((n, nc))
    rv = timed(lambda: ev.ctx.run_values(out=out))
    res["run_values_ms"] = rv
    res["run_values_kernel_ms"] = ev.ctx.timing()["total_ms"]
    res["run_values_GBps"] = gb / (min(rv) / 1e3)
    t = torch.empty((n, nc), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rd = timed(lambda: ev.ctx.run_values_device(t.data_ptr()))
    res["run_values_device_ms"] = rd
    res["run_values_device_GBps"] = gb / (min(rd) / 1e3)
    del t
    pr = timed(lambda: ev.predict(pop, errors="nan", max_bytes=1 << 32), reps=2)
    res["predict_ms"] = pr
    # a fitness run after the values runs: the plan and translation again
    rc2 = timed(lambda: ev.ctx.run_cases(ev.spec.mode, nc), reps=2)
    res["run_cases_after_ms"] = rc2
print(json.dumps(res), flush=True)
