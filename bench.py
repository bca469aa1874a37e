#!/usr/bin/env python3
"""Benchmark: BASELINE.json's headline metric on config 4.

    GPop/s (node-evals x cases / s) — symbolic regression, 65,536 trees
    (genHalfAndHalf(4, 8) over the symbreg primitive set with 10 arguments)
    x 2**20 fp64 fitness cases, target unwrapped_ball.

A *step* is one evaluation of the whole population on all cases (what one
``toolbox.map(toolbox.evaluate, population)`` does in the reference, minus the
host flattening, which is timed separately as ``e2e``).  Programs and cases are
resident in HBM when the timed region starts.

Multi-GPU (``torchrun --nproc-per-node N bench.py --gpus N``): cases are
sharded across ranks (each rank holds 2**20/N cases and every program); the
per-program partial SSEs (double-double hi/lo) are combined over RCCL by the
library's own communicator (``gpe_run_sharded_device``: all-gather + rank-
order double-double sum on the device).  The total work is fixed, so scaling
is "strong".

Rank 0 prints one JSON line.

A plain run does only what the headline needs: set up, warm up, time the
steps, write the outputs (``--dump-outputs DIR``), print the line.  Everything
else the benchmark measures or checks — the reference parity sample, the
trig-leaf and fp32 variants, the side configs, the evolved / deep-core / cold
end-to-end legs, the C3 population-sharded leg, the CPU baseline — runs with
``--full`` (each leg can still be switched off by its ``--no-...`` option).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

METRIC = ("GPop/s (node-evals×cases/s) symreg 64K pop×1M cases, "
          "1/2/4/8 GPUs")
FP64_LANES_PER_CU_CLK = 64     # 4 SIMD x 16 fp64 lanes per clock (gfx950)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--pop", type=int, default=65536)
    p.add_argument("--cases", type=int, default=2 ** 20)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--min-depth", type=int, default=4)
    p.add_argument("--max-depth", type=int, default=8)
    p.add_argument("--full", action="store_true",
                   help="also run the side measurements and checks (parity "
                        "sample, trig-leaf and fp32 variants, side configs, "
                        "evolved / deep-core / cold legs, CPU baseline)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs (hi, lo, err, "
                        "flags per program) as DIR/<name>.npy, float64")
    p.add_argument("--cpu-trees", type=int, default=0,
                   help="CPU baseline sample (default: 48 trees per worker)")
    p.add_argument("--cpu-cases", type=int, default=65536)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-trig", action="store_true",
                   help="diagnostic: primitive set without sin/cos")
    p.add_argument("--no-fp32", action="store_true",
                   help="skip the fp32-mode side measurement")
    p.add_argument("--no-trig-leaves", action="store_true",
                   help="skip the trig-leaf (GPUEvaluator default) variant")
    p.add_argument("--profile-only", action="store_true",
                   help="skip the CPU baseline and e2e pass (for rocprofv3)")
    p.add_argument("--no-side-configs", action="store_true",
                   help="skip the C3 / C5 side legs (1M-individual boolean "
                        "populations, GPUEvaluator end to end)")
    return p.parse_args()


# --------------------------------------------------------- CPU baseline ----
_CPU = {}


def progress(msg):
    """A stage marker on stderr (long runs show they are alive)."""
    print("[bench %.0fs] %s" % (time.perf_counter() - _T0, msg),
          file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def measured_traffic(args, world):
    """HBM bytes per launch of the dominant kernel from the committed PMC
    profile (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE cannot run inside the
    timed process), when this run is the profiled workload."""
    path = os.path.join(REPO, "profiles", "r06c_traffic.json")
    try:
        with open(path) as fh:
            rec = json.load(fh)
    except (OSError, ValueError):
        return None
    w = rec.get("workload", {})
    if (w.get("pop"), w.get("cases"), w.get("seed"), w.get("min_depth"),
            w.get("max_depth"), w.get("world")) != (
            args.pop, args.cases, args.seed, args.min_depth, args.max_depth,
            world) or args.no_trig:
        return None
    return rec


def parity_sample(hi, lo, err, flags, spec, golden=None):
    """Fitness of the 48 golden trees of tests/golden/c4_bench_sample.json.gz
    (the reference's own values on this very workload; 16 of them had a
    sin/cos argument past 2^40, the table core's redo test) against this
    run's outputs: max relative error,
    bit-identical count, exception types.  Computed after the timed
    region.  hi/lo/err/flags: host arrays over the whole population (when
    sharded: gpe_run_sharded's combined result, identical on every rank)."""
    import gzip
    if golden is None:
        path = os.path.join(REPO, "tests", "golden", "c4_bench_sample.json.gz")
        try:
            with gzip.open(path, "rt") as fh:
                golden = json.load(fh)
        except OSError:
            return None
    worst, exact, bad = 0.0, 0, []
    for i, fit, e in zip(golden["index"], golden["fitness"], golden["error"]):
        got = spec.finish(i, hi[i], lo[i], err[i], flags[i])
        if e is not None or isinstance(got, BaseException):
            if type(got).__name__ != e:
                bad.append(i)
            continue
        exp, val = float.fromhex(fit), got[0]
        if val == exp:
            exact += 1
            continue
        rel = abs(val - exp) / abs(exp) if exp else math.inf
        worst = max(worst, rel)
        if not rel <= 1e-12:
            bad.append(i)
    return {"n": len(golden["index"]), "args_past_2_40": sum(golden["redo"]),
            "max_rel": worst, "bit_identical": exact, "failed": bad,
            "tolerance": 1e-12,
            "source": "tests/golden/c4_bench_sample.json.gz (reference "
                      "gp.compile + symbreg.py:60-61 loop at 2^20 cases)"}


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def dump_outputs(path, out_hi, out_lo, out_err, out_flags):
    """``--dump-outputs``: what the last timed step left in the caller's four
    buffers, one value per program, as ``hi.npy``, ``lo.npy`` (the double-
    double SSE), ``err.npy`` (first failing case, as the unsigned value) and
    ``flags.npy``, all float64.  Past 64 MB in all, a fixed seeded sample of
    the programs, its sorted indices in ``index.npy``."""
    os.makedirs(path, exist_ok=True)
    arrs = {"hi": out_hi.cpu().numpy(), "lo": out_lo.cpu().numpy(),
            "err": out_err.cpu().numpy().view(np.uint64),
            "flags": out_flags.cpu().numpy().view(np.uint32)}
    n = len(arrs["hi"])
    keep = DUMP_LIMIT_BYTES // (8 * (len(arrs) + 1))
    if n > keep:
        idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrs = {k: v[idx] for k, v in arrs.items()}
        arrs["index"] = idx
    for name, a in arrs.items():
        np.save(os.path.join(path, name + ".npy"), a.astype(np.float64))


def _oracle_data(name):
    """The oracle's view of a side config's cases (tests/test_oracle.py)."""
    from deap_amd import datasets
    if name == "c2":
        ins, outs = datasets.mux11_table()
    elif name == "c3":
        ins, outs = datasets.parity6_table()
    else:
        X, L = datasets.spambase_csv(os.path.join(
            REPO, "tests", "golden", "spambase.csv.gz")) if name == "c5_real" \
            else datasets.spambase_like(4601, 5)
        return {"rows": list(zip(*X.tolist())), "labels": list(map(int, L))}
    return {"inputs": [list(map(int, c)) for c in ins.T],
            "outputs": list(map(int, outs))}


def side_configs():
    """BASELINE configs 2, 3 and 5 (11-multiplexer at 40K, parity-6 and
    spambase at 1M individuals; C5 on the synthetic stand-in and on the
    reference's own spambase.csv rows) through GPUEvaluator.evaluate, as
    toolbox.map calls it: kernel, device (upload + kernels + download) and
    end-to-end ms (host flattening and fitness tuples included), best of 3
    (scripts/bench_configs.py).  After the timing, 64 individuals of each
    population are evaluated by the oracle (the reference's gp.compile +
    evaluate restated, oracle/gp_ref.py): their hit counts must be
    bit-identical."""
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    from bench_configs import measure
    from oracle import gp_ref
    out = {}
    pset_name = {"c2": "mux11", "c3": "parity6", "c5": "spambase",
                 "c5_real": "spambase"}
    for name in ("c2", "c3", "c5", "c5_real"):
        r, pop, res = measure(name, 3, keep=True)
        rec = {k: r[k] for k in ("pop", "cases", "nodes", "kernel_ms",
                                 "device_ms", "e2e_ms", "hostflat_flatten_ms",
                                 "hostflat_device_ms", "kernel_gpops", "e2e_gpops")}
        data = _oracle_data(name)
        idx = np.random.default_rng(3).choice(len(pop), 64, replace=False)
        bad = []
        for i in idx.tolist():
            kind, val = gp_ref.evaluate(str(pop[i]), pset_name[name], data)
            if kind != "ok" or isinstance(res[i], BaseException) or \
                    res[i][0] != val:
                bad.append(i)
        rec["oracle_sample"] = {"n": len(idx), "bit_identical": len(idx) - len(bad),
                                "failed": bad}
        out[name] = rec
    return out


def c3_sharded_leg(device, reps=3):
    """BASELINE config 3 as it is named there: even-6 parity at 1M
    individuals, population-sharded over the job's ranks
    (distributed.PopulationSharded: length-balanced contiguous slices, each
    rank reads and lowers its own slice, gpe_run_gathered all-gathers every
    rank's results over the library's RCCL communicator, every rank builds
    all 1M fitness tuples).  Wall time of the whole ``evaluate`` per rep,
    barrier on both sides, max over ranks, best of *reps*; per-rank host
    phases of the last rep; 64 individuals checked against the oracle after
    the timing (bit-exact hit counts).  Replaces the reference's
    ``Pool.map`` over individuals (examples/ga/onemax_mp.py:58-59)."""
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    from bench_configs import population
    from deap_amd.distributed import PopulationSharded, _lengths
    from deap_amd.evaluator import GPUEvaluator
    rank, world = dist.get_rank(), dist.get_world_size()
    pset, spec, pop = population("c3")
    ev = GPUEvaluator(pset, spec, device=device)
    ps = PopulationSharded(ev)
    ps.evaluate(pop[:64 * world])                  # warm up, joins the comm
    dev = torch.device("cuda", device)
    best, res = None, None
    for _ in range(reps):
        res = None
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ps.evaluate(pop)
        el = time.perf_counter() - t0
        dist.barrier()
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
        best = el if best is None else min(best, el)
    lens = _lengths(pop)
    nodes = int(lens.sum())
    # this rank's kernel and all-gather time of the last rep, then min / max
    # over the ranks (an imbalance or a slow collective shows here)
    k_ms = ev.ctx.timing()["total_ms"]
    c_ms = ev.ctx.comm_timing()["comm_ms"]
    t = torch.tensor([k_ms, -k_ms, c_ms, -c_ms], dtype=torch.float64,
                     device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    out = {"pop": len(pop), "cases": spec.n_cases, "nodes": nodes,
           "ranks": world, "evaluate_ms": round(best * 1e3, 3),
           "e2e_gpops": round(nodes * spec.n_cases / best / 1e9, 2),
           "kernel_ms_rank": round(k_ms, 3),
           "kernel_ms_min_max": [round(-float(t[1]), 3), round(float(t[0]), 3)],
           "comm_ms_min_max": [round(-float(t[3]), 3), round(float(t[2]), 3)],
           "note": "PopulationSharded -> gpe_run_gathered (RCCL all-gather); "
                   "max over ranks of GPUEvaluator-equivalent wall time, "
                   "fitness tuples for all individuals on every rank"}
    if rank == 0:
        from oracle import gp_ref
        data = _oracle_data("c3")
        idx = np.random.default_rng(3).choice(len(pop), 64, replace=False)
        bad = []
        for i in idx.tolist():
            kind, val = gp_ref.evaluate(str(pop[i]), "parity6", data)
            if kind != "ok" or isinstance(res[i], BaseException) or \
                    res[i][0] != val:
                bad.append(i)
        out["oracle_sample"] = {"n": len(idx),
                                "bit_identical": len(idx) - len(bad),
                                "failed": bad}
    ev.ctx.close()
    return out


def cold_e2e(pset, X, y, args, device):
    """What a new generation costs through the product path: a FRESH
    population (seed + 1, same shape) through GPUEvaluator.evaluate (the
    toolbox.map drop-in, trig leaves on as by default), cold — node codes
    read on the host, device lowering, threaded-code translation and launch
    plan, the run, D2H and the fitness tuples — then its phases one by one
    on another fresh population (seed + 2)."""
    from deap_amd import _lib, configs
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    ev = GPUEvaluator(pset, SymbRegMSE(X, y), device=device)
    ev.evaluate(configs.population(pset, "half", 64, args.seed + 9,
                                   args.min_depth, args.max_depth))
    pop = configs.population(pset, "half", args.pop, args.seed + 1,
                             args.min_depth, args.max_depth)
    nodes = sum(len(t) for t in pop)
    t0 = time.perf_counter()
    res = ev.evaluate(pop)
    wall = time.perf_counter() - t0
    assert len(res) == len(pop)
    pop2 = configs.population(pset, "half", args.pop, args.seed + 2,
                              args.min_depth, args.max_depth)
    t0 = time.perf_counter()
    codes = ev.flattener.read_codes(pop2)
    t1 = time.perf_counter()
    ev.ctx.lower_programs(*codes)
    t2 = time.perf_counter()
    hi, lo, err, flags = ev.ctx.run(_lib.GPE_MODE_MSE)
    t3 = time.perf_counter()
    kern = ev.ctx.timing()["total_ms"]
    ev.spec.finish_all(hi, lo, err, flags)
    t4 = time.perf_counter()
    out = {"evaluate_ms": round(wall * 1e3, 1),
           "gpops": round(nodes * X.shape[1] / wall / 1e9, 1),
           "phases_ms": {"read_codes": round((t1 - t0) * 1e3, 1),
                         "device_lowering": round((t2 - t1) * 1e3, 1),
                         "run": round((t3 - t2) * 1e3, 1),
                         "of_which_kernels": round(kern, 1),
                         "run_host_overhead": round((t3 - t2) * 1e3 - kern, 1),
                         "fitness_tuples": round((t4 - t3) * 1e3, 1)},
           "note": "fresh populations (seeds %d, %d), trig leaves on; "
                   "run_host_overhead = threaded-code translation, launch "
                   "plan, copies" % (args.seed + 1, args.seed + 2)}
    ev.ctx.close()
    return out


def deep_core_leg(X, y, steps, device):
    """The deep asm core (programs needing 6..12 operand-stack slots) at the
    headline's 2^20 cases: the 288 trees of tests/golden/c4_deep_core.json.gz
    (reference-pinned at 4,096 cases; 32 of them on the redo path), 16
    copies each, evaluated every node."""
    import gzip
    from deap_amd import _lib, configs, gp
    from deap_amd.flatten import Flattener
    path = os.path.join(REPO, "tests", "golden", "c4_deep_core.json.gz")
    with gzip.open(path, "rt") as fh:
        g = json.load(fh)
    pset = configs.pset_for("symreg10")
    trees = [gp.PrimitiveTree.from_string(t, pset) for t in g["trees"]] * 16
    batch = Flattener(pset).flatten(trees)
    ctx = _lib.Context(device)
    ctx.set_cases(_lib.GPE_MACHINE_F, X, y)
    ctx.load_programs(batch)
    ctx.run(_lib.GPE_MODE_MSE)                 # warm up (translation, plan)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.run(_lib.GPE_MODE_MSE)
    el = (time.perf_counter() - t0) / steps
    work = int(batch.length.sum()) * X.shape[1]
    out = {"value": round(work / el / 1e9, 1), "ms_per_step": round(el * 1e3, 1),
           "kernel_ms": round(ctx.timing()["kernel_ms"], 1),
           "programs": len(trees), "nodes": int(batch.length.sum()),
           "slots": [int(batch.depth.min()), int(batch.depth.max())],
           "geometry": ctx.geometry()}
    ctx.close()
    return out


def evolved_leg(X, y, steps, device):
    """An evolved population at the headline's 2^20 cases: the 4,096 final
    trees of eight seeded symbreg.py-style runs (150 generations,
    staticLimit(17); tests/golden/c4_evolved.json.gz, scripts/evolve_c4.py),
    16 copies each, every node evaluated (trig leaves off, as the headline).
    After the timing, 32 of the trees are evaluated on the first 4,096 cases
    by the GPU and by the oracle (the reference path restated,
    oracle/gp_ref.py): within 1e-12."""
    import gzip
    from deap_amd import _lib, configs, gp
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    from deap_amd.flatten import Flattener
    from oracle import gp_ref
    path = os.path.join(REPO, "tests", "golden", "c4_evolved.json.gz")
    with gzip.open(path, "rt") as fh:
        g = json.load(fh)
    pset = configs.pset_for("symreg10")
    base_trees = [gp.PrimitiveTree.from_string(t, pset) for t in g["trees"]]
    trees = base_trees * 16
    batch = Flattener(pset).flatten(trees)
    ctx = _lib.Context(device)
    ctx.set_cases(_lib.GPE_MACHINE_F, X, y)
    ctx.load_programs(batch)
    ctx.run(_lib.GPE_MODE_MSE)                 # warm up (translation, plan)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.run(_lib.GPE_MODE_MSE)
    el = (time.perf_counter() - t0) / steps
    work = int(batch.length.sum()) * X.shape[1]
    out = {"value": round(work / el / 1e9, 1), "ms_per_step": round(el * 1e3, 1),
           "kernel_ms": round(ctx.timing()["kernel_ms"], 1),
           "programs": len(trees), "nodes": int(batch.length.sum()),
           "mean_tree_len": round(batch.length.mean(), 1),
           "max_height": max(t.height for t in base_trees),
           "slots": [int(batch.depth.min()), int(batch.depth.max())],
           "geometry": ctx.geometry(), "source": g.get("source")}
    ctx.close()
    # parity: 32 trees on 4,096 cases against the oracle
    n = 4096
    Xs, ys = np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(y[:, :n])
    idx = np.random.default_rng(5).choice(len(base_trees), 32, replace=False)
    ev = GPUEvaluator(pset, SymbRegMSE(Xs, ys), device=device, trig_leaves=False)
    got = ev.evaluate([base_trees[i] for i in idx])
    rows = list(zip(*Xs.tolist()))
    terms = [(v,) for v in ys[0].tolist()]
    worst, bad = 0.0, []
    for i, r in zip(idx.tolist(), got):
        try:
            val = gp_ref.eval_symreg_mse(g["trees"][i], "symreg10", rows, terms)
        except (ValueError, OverflowError) as e:      # the reference raises
            if type(e) is not type(r):
                bad.append(i)
            continue
        if isinstance(r, BaseException):
            bad.append(i)
            continue
        rel = abs(r[0] - val) / abs(val) if val else abs(r[0])
        worst = max(worst, rel)
        if rel > 1e-12:
            bad.append(i)
    ev.ctx.close()
    out["oracle_sample"] = {"n": len(idx), "cases": n, "max_rel": worst, "failed": bad,
                            "tolerance": 1e-12}
    return out


def _cpu_eval(tree_str):
    from oracle import gp_ref
    return gp_ref.eval_symreg_mse(tree_str, "symreg10", _CPU["rows"],
                                  _CPU["terms"])


def cpu_baseline(trees, X, y, n_trees, n_cases):
    """The reference path (gp.compile -> per-case Python calls -> fsum,
    oracle/gp_ref.py) under multiprocessing.Pool.map, as in
    examples/ga/onemax_mp.py:58-59, on a bounded sample."""
    import multiprocessing as mp
    _CPU["rows"] = list(zip(*X[:, :n_cases].tolist()))
    _CPU["terms"] = [(v,) for v in y[0, :n_cases].tolist()]
    # the host CPUs this process may use: the affinity set, bounded by the
    # CPU share the host grants one GPU's job (OMP_NUM_THREADS on the GPU
    # box: 16 of 256 visible) — more workers than that only oversubscribe
    visible = len(os.sched_getaffinity(0))
    share = os.environ.get("OMP_NUM_THREADS", "")
    cores = min(visible, int(share)) if share.isdigit() and int(share) > 0 \
        else visible
    n_trees = n_trees or 48 * cores
    sample = [str(t) for t in trees[:n_trees]]
    ctx = mp.get_context("fork")
    with ctx.Pool(cores) as pool:
        pool.map(_cpu_eval, sample[:cores])          # warm the workers
        t0 = time.perf_counter()
        pool.map(_cpu_eval, sample, chunksize=1)
        dt = time.perf_counter() - t0
    nodes = sum(len(t) for t in trees[:n_trees])
    return {"value": nodes * n_cases / dt / 1e9, "unit": "GPop/s",
            "cores": cores, "kind": "port",
            "sample": "%d trees (%d nodes) x %d cases, %.1f s wall, %d worker "
                      "processes (%d CPUs visible, the host's CPU share "
                      "OMP_NUM_THREADS=%s)" % (n_trees, nodes, n_cases, dt, cores,
                                                visible, share or "unset")}


# ------------------------------------------------------------ launcher ----
def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_env(base, rank, world, port):
    """The environment of rank *rank* of a *world*-rank job on this node:
    what ``torch.distributed.run --nnodes=1 --nproc-per-node world`` sets."""
    env = dict(base)
    env.update({"RANK": str(rank), "LOCAL_RANK": str(rank),
                "WORLD_SIZE": str(world), "LOCAL_WORLD_SIZE": str(world),
                "GROUP_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": str(port)})
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def launch(world, argv, child=None, poll_s=0.2):
    """``bench.py --gpus N`` (N > 1) run without a launcher: start N rank
    processes of this script (children, never an exec; this process touches
    no GPU and has not imported torch), relay rank 0's JSON line and return
    the exit code: non-zero if any rank fails — the others are then
    terminated — or if the line does not report ``n_gpus == N``.  *child*
    replaces the child command (tests)."""
    import subprocess
    cmd = child or [sys.executable, "-u", os.path.abspath(__file__)] + argv
    port = _free_port()
    procs = []
    for r in range(world):
        procs.append(subprocess.Popen(
            cmd, env=rank_env(os.environ, r, world, port),
            stdout=subprocess.PIPE, start_new_session=True))
    import threading
    lines = []

    def relay(p):                    # other ranks' stdout goes to stderr
        for l in p.stdout:
            sys.stderr.write(l.decode(errors="replace"))
    reader = threading.Thread(target=lambda: lines.extend(
        l.decode(errors="replace") for l in procs[0].stdout), daemon=True)
    reader.start()
    for p in procs[1:]:
        threading.Thread(target=relay, args=(p,), daemon=True).start()
    failed = None
    while failed is None and any(p.poll() is None for p in procs):
        for r, p in enumerate(procs):
            if p.poll() not in (None, 0):
                failed = (r, p.returncode)
                break
        time.sleep(poll_s)
    if failed is None:
        failed = next(((r, p.returncode) for r, p in enumerate(procs)
                       if p.returncode != 0), None)
    if failed is not None:
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, 15)
                except OSError:
                    pass
        for p in procs:
            try:
                p.wait(30)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, 9)
                p.wait()
        print("bench launcher: rank %d exited with %d" % failed,
              file=sys.stderr, flush=True)
        return failed[1] if failed[1] > 0 else 1
    reader.join(30)
    out = [l for l in lines if l.lstrip().startswith("{")]
    for l in lines:
        if l not in out:
            sys.stderr.write(l)
    if not out:
        print("bench launcher: rank 0 printed no JSON line", file=sys.stderr)
        return 1
    rec = json.loads(out[-1])
    if rec.get("n_gpus") != world:
        print("bench launcher: rank 0 reports n_gpus=%r, launched %d"
              % (rec.get("n_gpus"), world), file=sys.stderr)
        return 1
    print(out[-1].rstrip("\n"), flush=True)
    return 0


# ----------------------------------------------------------------- main ----
def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    torch.cuda.set_device(local)
    dist = None
    if world > 1 or os.environ.get("DEAP_AMD_FORCE_DIST") == "1":
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)

    from deap_amd import _lib, configs, datasets
    from deap_amd.evaluator import SymbRegMSE
    from deap_amd.flatten import Flattener

    # data (configs.headline_c4): every rank builds the same X, keeps its
    # case shard
    rng = np.random.default_rng(args.seed)
    X_all = np.ascontiguousarray(rng.uniform(-1.0, 1.0,
                                             size=(args.cases, 10)).T)
    lo_c = rank * args.cases // world
    hi_c = (rank + 1) * args.cases // world
    X = np.ascontiguousarray(X_all[:, lo_c:hi_c])
    y = datasets.unwrapped_ball_py(X)[None, :]
    n_local = hi_c - lo_c

    pset = configs.pset_for("symreg10_notrig" if args.no_trig
                            else "symreg10")
    t0 = time.perf_counter()
    pop = configs.population(pset, "half", args.pop, args.seed,
                             args.min_depth, args.max_depth)
    t_gen = time.perf_counter() - t0
    fl = Flattener(pset)
    t0 = time.perf_counter()
    batch = fl.flatten(pop)
    t_flat = time.perf_counter() - t0
    nodes = int(batch.length.sum())

    ctx = _lib.Context(local)
    info = ctx.device_info()
    ctx.set_cases(_lib.GPE_MACHINE_F, X, y)
    t0 = time.perf_counter()
    ctx.load_programs(batch)
    t_h2d = time.perf_counter() - t0

    n = args.pop
    out_hi = torch.empty(n, dtype=torch.float64, device=dev)
    out_lo = torch.empty(n, dtype=torch.float64, device=dev)
    out_err = torch.empty(n, dtype=torch.int64, device=dev)
    out_flags = torch.empty(n, dtype=torch.int32, device=dev)

    if dist is not None:
        # the C ABI's RCCL communicator (gpe_comm_init); torch's store only
        # carries rank 0's id to the other ranks
        from types import SimpleNamespace
        from deap_amd.distributed import native_comm
        assert native_comm(SimpleNamespace(ctx=ctx)) is ctx

    def step():
        if dist is None:
            ctx.run_device(_lib.GPE_MODE_MSE, out_hi.data_ptr(),
                           out_lo.data_ptr(), out_err.data_ptr(),
                           out_flags.data_ptr())
        else:
            # evaluate this rank's case slice, then on the context's stream:
            # all-gather the (hi, lo) partials + rank-order double-double
            # sum, first error MIN, flags OR (gpe_run_sharded_device)
            ctx.run_sharded_device(_lib.GPE_MODE_MSE, lo_c, out_hi.data_ptr(),
                                   out_lo.data_ptr(), out_err.data_ptr(),
                                   out_flags.data_ptr())

    def timed():
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        kms = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
            kms.append(ctx.timing())
            if dist is not None:             # (waits for the step's collectives)
                kms[-1].update(ctx.comm_timing())
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, kms

    progress("headline: timing %d steps" % args.steps)
    elapsed, kernel_ms = timed()

    if args.dump_outputs and rank == 0:
        torch.cuda.synchronize()
        dump_outputs(args.dump_outputs, out_hi, out_lo, out_err, out_flags)

    # parity of the timed launch (after the timed region): the reference's
    # fitness of 48 of these very trees, 16 on the redo path
    sample = None
    if args.full and (args.pop, args.cases, args.seed, args.min_depth,
                      args.max_depth) == (65536, 2 ** 20, 2024, 4, 8) \
            and not args.no_trig:
        torch.cuda.synchronize()
        spec = SymbRegMSE(X, y)          # finish() of the product path
        spec.n_cases = args.cases        # (all ranks' cases when sharded)
        sample = parity_sample(out_hi.cpu().numpy(), out_lo.cpu().numpy(),
                               out_err.cpu().numpy().view(np.uint64),
                               out_flags.cpu().numpy().view(np.uint32),
                               spec)

    node_evals_step = nodes * args.cases
    value = node_evals_step * args.steps / elapsed / 1e9
    ms_per_step = elapsed * 1e3 / args.steps

    # roofline of the dominant kernel (interpreter), this rank
    kern_ms = float(np.mean([k["kernel_ms"] for k in kernel_ms]))
    red_ms = float(np.mean([k["reduce_ms"] for k in kernel_ms]))
    achieved = nodes * n_local / (kern_ms / 1e3) / 1e9
    clock_ghz = info["clock_khz"] / 1e6
    peak = info["cu"] * FP64_LANES_PER_CU_CLK * clock_ghz
    geo = ctx.geometry()
    # N > 1: where a step's time goes, per rank, min / max over the ranks —
    # the interpreter kernels, the RCCL group of gpe_run_sharded_device
    # (all-gather of the partials, first-error MIN, flag SUM) and the
    # redo-flag all-reduce (none with the exact cores)
    multi = None
    if dist is not None:
        comm_ms = float(np.mean([k["comm_ms"] for k in kernel_ms]))
        redo_ms = float(np.mean([k["redo_ms"] for k in kernel_ms]))
        t = torch.tensor([kern_ms, -kern_ms, comm_ms, -comm_ms, redo_ms,
                          -redo_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        mm = lambda i: [round(-float(t[i + 1]), 3), round(float(t[i]), 3)]
        multi = {"kernel_ms_min_max": mm(0), "comm_ms_min_max": mm(2),
                 "redo_allreduce_ms_min_max": mm(4),
                 "cases_per_rank": n_local,
                 "comm_timeout_s": float(os.environ.get("GPE_COMM_TIMEOUT_S",
                                                        "120"))}

    # product default of GPUEvaluator: sin/cos of bare arguments evaluated
    # once per case into device columns (same values); reported beside the
    # headline, which evaluates every node of every tree like the reference
    leaves = None
    if args.full and not args.no_trig and not args.no_trig_leaves:
        fl2 = Flattener(pset, trig_leaves=range(X.shape[0]))
        t0 = time.perf_counter()
        batch2 = fl2.flatten(pop)
        t_flat2 = time.perf_counter() - t0
        ctx.set_trig_leaves(True)
        ctx.load_programs(batch2)
        progress("trig-leaf variant")
        el2, kms2 = timed()
        leaves = {"value": round(node_evals_step * args.steps / el2 / 1e9, 3),
                  "ms_per_step": round(el2 * 1e3 / args.steps, 3),
                  "kernel_ms": round(float(np.mean(
                      [k["kernel_ms"] for k in kms2])), 3),
                  "flatten_s": round(t_flat2, 2),
                  "geometry": ctx.geometry(),
                  "note": "GPUEvaluator default (trig_leaves=True): "
                          "sin/cos(ARGv) computed once per case per run"}

    # fp32 mode (GPUEvaluator(precision="fp32")): the same programs and
    # cases evaluated in single precision (C++ f_eval<.., float>); reported
    # beside the fp64 headline with its tolerance
    fp32 = None
    if args.full and not args.no_fp32 and not args.profile_only:
        ctx.set_trig_leaves(False)
        ctx.set_precision(_lib.GPE_PREC_F32)
        ctx.load_programs(batch)
        progress("fp32 variant")
        el3, kms3 = timed()
        fp32 = {"value": round(node_evals_step * args.steps / el3 / 1e9, 3),
                "ms_per_step": round(el3 * 1e3 / args.steps, 3),
                "kernel_ms": round(float(np.mean(
                    [k["kernel_ms"] for k in kms3])), 3),
                "dtype": "f32", "geometry": ctx.geometry(),
                "note": "GPUEvaluator(precision='fp32'): tree and d*d in "
                        "fp32, SSE in fp64; not reference-exact"}
        ctx.set_precision(_lib.GPE_PREC_F64)

    side = cold = deep = evolved = c3s = None
    legs = args.full and not args.no_side_configs and not args.profile_only
    if dist is not None and legs:
        progress("c3 population-sharded leg")
        c3s = c3_sharded_leg(local)
    if world == 1 and legs:
        progress("side configs")
        side = side_configs()
        if not args.no_trig and args.pop == 65536 and args.cases == 2 ** 20:
            progress("evolved-population leg")
            evolved = evolved_leg(X, y, 2, local)
            progress("deep-core leg")
            deep = deep_core_leg(X, y, 2, local)
            progress("cold e2e")
            cold = cold_e2e(pset, X, y, args, local)

    prof = measured_traffic(args, world)
    res = None
    if rank == 0:
        res = {
            "metric": METRIC, "value": round(value, 3), "unit": "GPop/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic (X~U(-1,1)^10 seed %d, y=unwrapped_ball; "
                    "trees genHalfAndHalf(%d,%d) seed %d)"
                    % (args.seed, args.min_depth, args.max_depth, args.seed),
            "config": {"workload": "C4 symreg10: %d trees x %d fp64 cases%s"
                                   % (args.pop, args.cases,
                                      "" if dist is None else
                                      ", case-sharded over %d GPU(s), RCCL "
                                      "all-gather + rank-order sum of the "
                                      "partial SSEs" % world),
                       "pop": args.pop, "cases": args.cases,
                       "nodes": nodes, "mean_tree_len": nodes / args.pop,
                       "node_evals_per_step": node_evals_step,
                       "parallelism": "case-shard x%d" % world,
                       "geometry": geo},
            "roofline": {"bound": "valu", "achieved": round(achieved, 2),
                         "peak": round(peak, 1), "unit": "GPop/s",
                         "frac": round(achieved / peak, 4),
                         "traffic": (prof or {}).get(
                             "traffic_bytes_per_launch"),
                         "traffic_source": "profiles/r06c_traffic.json "
                                           "(PMC FETCH_SIZE x2 + WRITE_SIZE)",
                         "pmc": None if prof is None else {
                             k: prof.get(k) for k in (
                                 "fp64_lane_ops_per_node_case",
                                 "fp64_issue_util", "valu_busy",
                                 "occupancy_waves_per_cu")},
                         "kernel": "f_eval_asm<exact> (the threaded-code core "
                                   "with glibc 2.35's sin/cos in its "
                                   "handlers, the product's fp64 core): "
                                   "HIP events around it, = its traced "
                                   "time in profiles/r06c_f_eval_asm.md",
                         "kernel_ms": round(kern_ms, 3),
                         "reduce_ms": round(red_ms, 3),
                         "note": "1 fp64 VALU lane-op per node-case; peak = "
                                 "%d CU x 64 lanes x %.2f GHz"
                                 % (info["cu"], clock_ghz)},
            "e2e": {"generate_s": round(t_gen, 2),
                    "flatten_s": round(t_flat, 2),
                    "h2d_s": round(t_h2d, 3),
                    "gpops_incl_flatten": round(
                        node_evals_step / (t_flat + t_h2d + ms_per_step / 1e3)
                        / 1e9, 2)},
        }
        if sample is not None:
            res["parity_sample"] = sample
        if multi is not None:
            res["multi_gpu"] = multi
        if leaves is not None:
            res["trig_leaves"] = leaves
        if fp32 is not None:
            res["fp32"] = fp32
        if side is not None:
            res["side_configs"] = side
        if c3s is not None:
            res["c3_sharded"] = c3s
        if evolved is not None:
            res["evolved"] = evolved
        if deep is not None:
            res["deep_core"] = deep
        if cold is not None:
            res["e2e"]["cold"] = cold
        if args.full and world == 1 and not args.no_cpu_baseline \
                and not args.profile_only:
            progress("cpu baseline")
            res["cpu_baseline"] = cpu_baseline(pop, X_all, y, args.cpu_trees,
                                               args.cpu_cases)
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
