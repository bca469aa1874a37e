"""The exact cores' MID / MIDLO sin/cos bodies with static lane roles
(``GPE_TRIG_RANGES=3``, the default) on the GPU: ``predict``'s per-case outputs
are the host libm's in every bit, hi, lo, err and flags are equal in every
bit between a mode-2 context (the bodies before them) and a default one, and
the classes picked show the new pick (sin nodes move from mid to midlo).

300 cases (two full 128-case tiles and a partial one) of hand-made columns:
ARG0 within +-1.44 and ARG1 within +-0.97 hold the 0.126, 0.85546875 and 1.44
edges by ulps, zeros and denormals; ARG2 lies between 1.44 and 2.419 around
pi/2; ARG3 is U(-1, 1) with one inf.  The programs are the smallest that
reach each pick, a nanable argument, and one tree for the deep core.
"""
import itertools
import math

import numpy as np
import pytest

import predict_ref as pr
from deap_amd import _lib, configs, gp
from deap_amd.evaluator import GPUEvaluator, SymbRegMSE

pytestmark = pytest.mark.gpu
N = 300
ULP = 2.0 ** -52
T0855 = 0.85546875
GENERAL, MID, SMALL, MIDLO, WIDE = range(5)
LEAVES = ["sin(ARG0)", "cos(ARG0)", "sin(ARG2)", "cos(add(ARG0, ARG1))",
          "sin(mul(ARG0, ARG1))", "cos(ARG2)", "sin(add(ARG0, ARG1))", "cos(mul(ARG0, ARG1))"]


def _balanced(depth, leaves=None):
    """A full binary tree of adds over LEAVES taken in turn, left to right:
    `depth` stack slots."""
    leaves = leaves or itertools.cycle(LEAVES)
    if depth == 0:
        return next(leaves)
    return "add(%s, %s)" % (_balanced(depth - 1, leaves), _balanced(depth - 1, leaves))


# (program, the class picked per sin/cos node in mode 3; None: not pinned)
PROGRAMS = [
    ("sin(ARG0)", [MIDLO]), ("cos(ARG0)", [MIDLO]),
    ("sin(mul(ARG0, ARG1))", [MIDLO]), ("cos(add(ARG0, ARG1))", [MID]),
    ("sin(add(ARG0, ARG1))", [MID]), ("cos(mul(ARG0, ARG1))", [MIDLO]),
    ("sin(ARG2)", [MID]), ("cos(ARG2)", [MID]),                  # 1.44 <= bound < 2.42
    ("sin(sub(ARG2, ARG1))", [WIDE]),                            # (bound 3.39)
    ("sin(cos(ARG3))", [GENERAL, MIDLO]), ("cos(sin(ARG3))", [GENERAL, MIDLO]),
    ("cos(add(ARG1, sin(ARG3)))", [GENERAL, MID]),
    ("sin(add(ARG1, cos(ARG3)))", [GENERAL, MID]),
    ("sin(sin(ARG0))", [MIDLO, MIDLO]), ("cos(neg(ARG2))", [MID]),
    ("mul(sin(ARG0), cos(ARG2))", [MIDLO, MID]),
    (_balanced(6), None),
]
_CACHE = {}


def _column(vals, lim, rng):
    v = np.asarray([x for x in vals if abs(x) <= lim], dtype=np.float64)
    v = np.concatenate([v, -v])
    assert len(v) <= N
    out = np.concatenate([v, rng.uniform(-lim, lim, N - len(v))])
    return out[rng.permutation(N)]


def data():
    if "data" not in _CACHE:
        rng = np.random.default_rng(1440)
        lim0 = float(np.nextafter(1.44, 0))
        edges = [0.0, 5e-324, 2.0 ** -1074, 2.2250738585072014e-308, 2.0 ** -27, 2.0 ** -26,
                 0.5, 1.0, 1.25, lim0, float(np.nextafter(lim0, 0))]
        for e in (0.126, T0855, 1.44, math.pi / 2 - 0.126):
            edges += [e * (1 + k * ULP) for k in range(-4, 5)]
        edges += [math.ldexp(1.0, e) for e in range(-1070, 0, 97)]
        X = rng.uniform(-1.0, 1.0, (10, N))
        X[0] = _column(edges, lim0, rng)
        X[1] = _column(edges, 0.97, rng)
        mid = [1.44, float(np.nextafter(1.44, 2)), 2.419, 2.0, 1.5]
        mid += [math.pi / 2 * (1 + k * ULP) for k in range(-6, 7)]
        mid += [(math.pi / 2 + s * 0.126) * (1 + k * ULP) for s in (-1, 1) for k in range(-3, 4)]
        X[2] = np.concatenate([mid, rng.uniform(1.44, 2.419, N - len(mid))])[rng.permutation(N)]
        X[3, 290] = math.inf                    # (in the partial last tile)
        Y = rng.uniform(-2, 2, size=(1, N))
        _CACHE["data"] = (np.ascontiguousarray(X), np.ascontiguousarray(Y))
    return _CACHE["data"]


def population():
    pset = configs.pset_for("symreg10")
    return pset, [gp.PrimitiveTree.from_string(s, pset) for s, _ in PROGRAMS]


def reference():
    if "ref" not in _CACHE:
        pset, pop = population()
        _CACHE["ref"] = pr.values(pset, pop, data()[0])
    return _CACHE["ref"]


def run(monkeypatch, mode):
    """One fresh evaluator under GPE_TRIG_RANGES=mode (None: the default):
    raw (hi, lo, err, flags), predict's values, the picked classes, geometry."""
    if mode is None:
        monkeypatch.delenv("GPE_TRIG_RANGES", raising=False)
    else:
        monkeypatch.setenv("GPE_TRIG_RANGES", mode)
    X, Y = data()
    pset, pop = population()
    ev = GPUEvaluator(pset, SymbRegMSE(X, Y), device=0, trig_leaves=False)
    raw = {}
    inner = ev.run_batch

    def spy(batch, *a, **k):
        k["want"] = None                        # every output, copied back
        r = inner(batch, *a, **k)
        raw["out"] = [np.array(v, copy=True) for v in r[:4]]
        return r
    ev.run_batch = spy
    try:
        ev.evaluate(pop)
        picked = ev.ctx.trig_classes(picked=True)
        geo = ev.ctx.geometry()
        ev.run_batch = inner
        pred = ev.predict(pop, errors="nan")
    finally:
        ev.close()
    return raw["out"], pred, picked, geo


def test_modes_2_and_3_agree_and_predict_is_the_host_libm(monkeypatch):
    X, _ = data()
    pset, pop = population()
    F, exc = reference()
    # the inf case raises in the ARG3 programs only
    assert [bool(e) for e in exc] == ["ARG3" in s for s, _ in PROGRAMS]
    raw2, pred2, picked2, geo2 = run(monkeypatch, "2")
    raw3, pred3, picked3, geo3 = run(monkeypatch, None)
    print("TRIGCLS3|gpu|mode2=%s mode3=%s geometry=%s" % (picked2, picked3, geo3))
    # every program ran on an exact core, the balanced tree on the deep one
    assert geo3["asm"] == geo2["asm"] == len(pop) and geo3["asm_deep"] >= 1, geo3
    # the host pass over the same columns: the picks per program and in all
    lo = np.minimum(X.min(axis=1), 0.0)
    hi = np.maximum(X.max(axis=1), 0.0)
    lo[3], hi[3] = -math.inf, math.inf
    from deap_amd.flatten import Flattener
    batch = Flattener(pset).flatten(pop)        # (no leaf columns: every sin/cos a word)
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    host2, host3 = np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64)
    for i, (s, want) in enumerate(PROGRAMS):
        w = code[off[i]:off[i + 1]]
        c3 = _lib.debug_trig_picks(w, lo, hi, mode=3)
        assert want is None or list(c3) == want, (s, list(c3))
        host3 += np.bincount(c3, minlength=5)
        host2 += np.bincount(_lib.debug_trig_picks(w, lo, hi, mode=2), minlength=5)
    assert [picked3[k] for k in _lib.TRIG_PICKED] == host3.tolist()
    assert [picked2[k] for k in _lib.TRIG_PICKED] == host2.tolist()
    # the new pick: sin nodes move from mid to midlo, nothing else moves
    moved = picked3["midlo"] - picked2["midlo"]
    assert moved > 0 and picked2["mid"] - picked3["mid"] == moved
    assert all(picked2[k] == picked3[k] for k in ("general", "small", "wide"))
    assert picked3["mid"] > 0
    # hi, lo, err, flags: the same bits, program for program
    for name, a, b in zip(("hi", "lo", "err", "flags"), raw2, raw3):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape == (len(pop),)
        same = a.view(np.uint8).reshape(len(pop), -1) == b.view(np.uint8).reshape(len(pop), -1)
        bad = np.flatnonzero(~same.all(axis=1))
        assert len(bad) == 0, (name, [(int(i), PROGRAMS[i][0][:80]) for i in bad[:3]])
    # predict: the host libm's bits in every case, in both modes
    pr.assert_same_bits(pred3, F, "mode 3")
    pr.assert_same_bits(pred2, F, "mode 2")
