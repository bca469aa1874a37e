"""The exact cores' range-specialised sin/cos handlers on the GPU: with
``GPE_TRIG_RANGES`` on (the default) and off the results are the same in
every bit, the classes the device translation picked are the host pass's, and
the fitness is the reference's.

300 programs (hand-written ones around the range rules, 250 seeded symreg10
trees, 16 trees of the deep-core golden) over 421 cases: three full 128-case
tiles and a partial one, so pad lanes run the handlers.  The columns are
U(-1, 1), U(-0.3, 0.3), U(0.9, 2.4), U(-50, 50) and one column with a single
inf (the primitive set has ten arguments: columns 5..9 repeat the first four
kinds and U(-1, 1)).  No handler is fed an argument outside its range on
purpose: the classes come from the library's own pass over these columns.
"""
import gzip
import json
import math
import os

import numpy as np
import pytest

from deap_amd import _lib, configs, gp
from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
from test_launch_geometry import Values, check_mse, mse_reference, _same_bits
from test_trig_ranges import HAND

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_CASES = 421
NV = 10
MORE = ["sin(ARG2)", "cos(ARG2)", "sin(ARG1)", "cos(ARG1)", "sin(ARG3)",
        "cos(ARG3)", "sin(ARG4)", "cos(ARG4)", "sin(mul(ARG1, ARG1))",
        "cos(mul(ARG1, ARG6))", "sin(add(ARG2, ARG1))", "cos(sub(ARG2, ARG7))",
        "sin(mul(ARG0, ARG2))", "cos(add(ARG1, sin(ARG3)))",
        "sin(protectedDiv(ARG1, ARG2))", "cos(protectedDiv(ARG0, add(ARG2, 1)))",
        "sin(add(sin(ARG4), cos(ARG3)))", "add(sin(ARG1), cos(mul(ARG2, ARG1)))"]
_CACHE = {}


def population():
    if "pop" not in _CACHE:
        pset = configs.pset_for("symreg10")
        with gzip.open(os.path.join(HERE, "golden", "c4_deep_core.json.gz"), "rt") as fh:
            deep = json.load(fh)["trees"][:16]
        pop = [gp.PrimitiveTree.from_string(s, pset) for s in HAND + MORE + deep]
        pop += configs.population(pset, "half", 300 - len(pop), 91, 1, 8)
        assert len(pop) == 300 and len(HAND + MORE) == 34
        _CACHE["pop"] = pop
    return _CACHE["pop"]


def data():
    if "data" not in _CACHE:
        rng = np.random.default_rng(421)
        kinds = [(-1, 1), (-0.3, 0.3), (0.9, 2.4), (-50, 50), (-1, 1),
                 (-1, 1), (-0.3, 0.3), (0.9, 2.4), (-50, 50), (-1, 1)]
        X = np.array([rng.uniform(a, b, N_CASES) for a, b in kinds])
        X[4, 400] = math.inf                    # (in the partial last tile)
        Y = rng.uniform(-2, 2, size=(1, N_CASES))
        _CACHE["data"] = (np.ascontiguousarray(X), np.ascontiguousarray(Y))
    return _CACHE["data"]


def reference():
    if "ref" not in _CACHE:
        X, Y = data()
        vals = Values(configs.pset_for("symreg10"), population(), X)
        _CACHE["ref"] = mse_reference(vals, Y, N_CASES)
    return _CACHE["ref"]


def column_bounds(X, leaves):
    """gpe_set_cases' bounds: [min, max] hulled with 0.0, unbounded for a
    column with a nan or an inf; the trig leaves' columns [-1, 1]."""
    lo, hi = [], []
    for col in X:
        ok = bool(np.isfinite(col).all())
        lo.append(min(col.min(), 0.0) if ok else -math.inf)
        hi.append(max(col.max(), 0.0) if ok else math.inf)
    if leaves:
        n = len(lo)
        for _ in range(2):
            lo += [-1.0 if math.isfinite(lo[v]) else -math.inf for v in range(n)]
            hi += [1.0 if math.isfinite(hi[v]) else math.inf for v in range(n)]
    return np.array(lo), np.array(hi)


def run(monkeypatch, ranges, leaves):
    """One fresh evaluator: (fitness list, raw (hi, lo, err, flags), classes,
    geometry, the host pass's class counts)."""
    if ranges is None:
        monkeypatch.delenv("GPE_TRIG_RANGES", raising=False)
    else:
        monkeypatch.setenv("GPE_TRIG_RANGES", ranges)
    X, Y = data()
    pop = population()
    ev = GPUEvaluator(configs.pset_for("symreg10"), SymbRegMSE(X, Y), device=0,
                      trig_leaves=leaves)
    raw = {}
    inner = ev.run_batch

    def spy(batch, *a, **k):
        k["want"] = None                        # every output, copied back
        r = inner(batch, *a, **k)
        raw["out"] = [np.array(v, copy=True) for v in r[:4]]
        return r
    ev.run_batch = spy
    try:
        got = ev.evaluate(pop)
        classes = ev.ctx.trig_classes()
        geo = ev.ctx.geometry()
        batch = ev.flattener.flatten(pop)
    finally:
        ev.ctx.close()
    lo, hi = column_bounds(X, leaves)
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    host = np.zeros(3, dtype=np.int64)
    valid = 0
    for i in range(len(pop)):
        if batch.err[i]:
            continue
        valid += 1
        cls = _lib.debug_trig_classes(code[off[i]:off[i + 1]], lo, hi)
        host += np.bincount(cls, minlength=3)
    # every valid program ran on an exact core (asm counts both cores'); the
    # golden trees need six stack slots, the deep core's (as leaf columns,
    # their sin(ARGv) operands save the slot)
    assert geo["asm"] == valid and (leaves or geo["asm_deep"] >= 16), geo
    return got, raw["out"], classes, host


@pytest.mark.parametrize("leaves", [False, True], ids=["inline", "trig_leaves"])
def test_ranges_on_and_off_agree_bit_for_bit(monkeypatch, leaves):
    pop = population()
    on, raw_on, cls_on, host = run(monkeypatch, None, leaves)
    off, raw_off, cls_off, _ = run(monkeypatch, "0", leaves)
    print("TRIGCLS|gpu leaves=%d|on=%s off=%s host=%s"
          % (leaves, cls_on, cls_off, host.tolist()))
    # the switch: off, only general handlers; on, all three classes, as the
    # host pass counts them
    assert cls_off["mid"] == 0 and cls_off["small"] == 0 and cls_off["general"] > 0
    assert [cls_on[k] for k in _lib.TRIG_CLASSES] == host.tolist()
    assert all(cls_on[k] > 0 for k in _lib.TRIG_CLASSES), cls_on
    assert sum(cls_on.values()) == cls_off["general"]
    # hi, lo, err, flags: the same bits, program for program
    for name, a, b in zip(("hi", "lo", "err", "flags"), raw_on, raw_off):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape == (len(pop),)
        same = a.view(np.uint8).reshape(len(pop), -1) == \
            b.view(np.uint8).reshape(len(pop), -1)
        bad = np.flatnonzero(~same.all(axis=1))
        assert len(bad) == 0, (name, [(int(i), str(pop[i])[:100]) for i in bad[:3]])
    assert all(_same_bits(a, b) for a, b in zip(on, off))
    # and the reference's: exception types exact, otherwise 1e-12
    check_mse(pop, on, reference(), ("ranges on", leaves))
    check_mse(pop, off, reference(), ("ranges off", leaves))
