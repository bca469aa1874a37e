"""Test helper for ``SymbRegAbsError``: its definition restated in Python over
the doubles ``gp.compile(tree, pset)(*row)`` returns.  Not product code.

    e_i  = abs(f(*row_i) - t0_i - t1_i - ...)        # left to right
    mae  = math.fsum(e) / n
    mx   = float(numpy.max(e))      # nan if any e_i is nan, else the largest
    hits = sum(1 for v in e if v <= hit_eps)         # nan and inf: never

An individual raises what its first erroring case raises, at that case; with
every ``e_i`` finite and an overflowing sum it raises ``OverflowError`` from
``fsum``; with an inf ``e_i`` and no nan ``mae = inf``; with a nan ``mae = nan``.

The cells are ``scaled_ref``'s (its population, data and case counts, used as
they are) with the hand-written trees below appended.  The reference of all of
them is recorded in ``tests/golden/abs_error_n*.npz`` — written by
:func:`write_golden` (``python tests/golden/_ref_abs_error.py``, two minutes of
``gp.compile`` calls) — and ``tests/test_abs_error.py`` recomputes a sample of
it here on every run.
"""
import math
import os

import numpy as np

import scaled_ref as sr
from deap_amd import gp

HIT_EPS = 0.01
TOL = sr.TOL
CASES = sr.CASES
G = sr.GENERATOR
# finite and near 1e308 on every case: mae is that value at n = 1, and fsum
# overflows from n = 2
HUGE = "mul(%s, add(1e108, ARG1))" % sr.E200
EXTRA = [
    G,                                   # 0 the target itself: no error at all
    "add(%s, 0.005)" % G,                # 1 every case a hit
    "add(%s, 0.01)" % G,                 # 2 the rounding of (y + 0.01) - y puts
    "sub(%s, 0.01)" % G,                 # 3 ... cases on either side of 0.01
    "add(%s, mul(0.02, ARG0))" % G,      # 4 a hit where |x0| <= 0.5
    HUGE,                                # 5 fsum overflow
]
# status: 0 a value; 1 / 2 the first erroring case's ValueError /
# OverflowError (first: that case); 3 fsum's OverflowError (first: -1)
FSUM_OVERFLOW = 3
FIELDS = ("status", "first", "mae", "max", "hits", "hits0", "hits_finite",
          "any_nan", "any_inf", "Se_hi", "Se_lo")


def population():
    """``(pset, trees, n_base)``: scaled_ref's population, then EXTRA."""
    ps, trees = sr.population()
    return ps, trees + [gp.PrimitiveTree.from_string(s, ps) for s in EXTRA], len(trees)


def figures(e, hit_eps=HIT_EPS):
    """``(mae, mx, hits)`` of the per-case absolute errors *e* (a list of
    floats), as the definition states them; mae is the exception where fsum
    raises."""
    n = len(e)
    try:
        mae = math.fsum(e) / n
    except OverflowError as exc:
        mae = exc
    mx = float(np.max(np.array(e, dtype=np.float64)))
    hits = sum(1 for v in e if v <= hit_eps and v != math.inf)
    return mae, mx, hits


def record(f, y, first=None, kind=None):
    """The FIELDS of one program on one case set: *f* its values, *y* the
    term column, *first* / *kind* its first erroring case within them."""
    out = dict.fromkeys(FIELDS, 0.0)
    out["first"] = -1.0
    if first is not None:
        out["status"], out["first"] = float(sr.STATUS[kind]), float(first)
        out["mae"] = out["max"] = math.nan
        out["hits"] = out["hits0"] = out["hits_finite"] = -1.0
        return [out[k] for k in FIELDS]
    e = [abs(a - b) for a, b in zip(f.tolist(), y.tolist())]
    mae, mx, hits = figures(e)
    out["any_nan"] = float(any(v != v for v in e))
    out["any_inf"] = float(any(v == math.inf for v in e))
    out["hits0"] = float(sum(1 for v in e if v == 0.0))
    out["hits_finite"] = float(sum(1 for v in e if v < math.inf))
    out["max"], out["hits"] = mx, float(hits)
    if isinstance(mae, OverflowError):
        assert not out["any_nan"] and not out["any_inf"]
        out["status"] = float(FSUM_OVERFLOW)
        out["mae"] = math.nan
        out["hits"] = out["hits0"] = out["hits_finite"] = -1.0
        out["max"] = math.nan
    else:
        out["mae"] = mae
        if not out["any_nan"] and not out["any_inf"]:
            out["Se_hi"], out["Se_lo"] = sr.dd(sr.exact_sum(e))
    return [out[k] for k in FIELDS]


def reference(ps, tree, X, y, cases=CASES):
    """``{n: record}`` of one tree on the first n cases, for every n."""
    rows = list(zip(*X[:, :max(cases)].tolist()))
    f, first, kind = sr.outputs(ps, tree, rows)
    out = {}
    for n in cases:
        err = first is not None and first < n
        out[n] = record(f[:n], y[:n], first if err else None, kind if err else None)
    return out


def golden_path(n):
    return os.path.join(sr.GOLDEN, "abs_error_n%d.npz" % n)


def load_golden(n, key=None):
    """float64 ``[n_trees, len(FIELDS)]`` of the recorded reference; *key*
    (``scaled_ref.cells_key`` over the extended tree list): asserted to be the
    one it was recorded for."""
    with np.load(golden_path(n)) as z:
        assert key is None or str(z["key"]) == key, \
            "tests/golden/abs_error_n%d.npz was recorded for other trees or cases: run " \
            "tests/golden/_ref_abs_error.py" % n
        return z["ref"]


def write_golden():
    ps, trees, _ = population()
    X, y = sr.data()
    tab = {n: np.zeros((len(trees), len(FIELDS))) for n in CASES}
    for i, t in enumerate(trees):
        for n, rec in reference(ps, t, X, y).items():
            tab[n][i] = rec
    key = np.array(sr.cells_key(trees, X, y))
    for n in CASES:
        np.savez_compressed(golden_path(n), ref=tab[n], key=key)
