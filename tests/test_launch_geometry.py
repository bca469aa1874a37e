"""Launch geometry at ragged shapes: every core at programs-per-wave > 1,
partial tiles, short tile groups, padded waves and each planner knob, against
the reference's own evaluate body in plain Python.

Each cell sets its knobs (read once, in ``gpe_create``) before it builds its
own evaluator, asserts through ``Context.launch_shape`` that the launch shape
it is named for was reached (``gpe_create`` silently ignores a value out of
range), asserts the plan invariants, and compares every result with the
reference: ``gp.compile`` of the tree, called per case; ``math.fsum`` of the
squared residuals over ``n`` (or the hit count); the first exception by type.
fp64 MSE: exception type, nan, inf and 0.0 exact, else 1e-12 relative; hit
counts exact.  The reference is computed once per (population, data) pair:
the programs' values per case are kept, and every prefix of the cases, every
target layout and the per-case outputs are derived from them with the same
Python operations.

``GPE_TARGET_BLOCKS=256`` (the lowest value accepted) is the base of every
cell: ``P = min(pmax, programs * tiles / 1024)`` before the LDS fit, so 1000
programs over 9 tiles reach P = 8.

Each cell also prints one ``LG|`` line per launch (run with ``-s``): the
shape reached and how many results differ in any bit from the base cell of
the same population and data (reported, not asserted: the partial sums are
double-double, a different grouping may move a last bit).
"""
import math
import time

import numpy as np
import pytest

from deap_amd import configs, datasets, gp
from deap_amd.evaluator import (BooleanHits, GPUEvaluator, SymbRegCaseErrors,
                                SymbRegMSE, TypedBoolHits)
from deap_amd.flatten import Flattener

pytestmark = pytest.mark.gpu
REL = 1e-12                       # the project's stated fp64 bound
ERRORS = (ValueError, OverflowError, ZeroDivisionError, TypeError)

KNOBS = ("GPE_ASM", "GPE_ASM_P", "GPE_ASM_WAVES", "GPE_ASM_LDS_KB",
         "GPE_ASM_DBUF", "GPE_DEAL_MIX", "GPE_TARGET_BLOCKS",
         "GPE_ASM_TARGET_BLOCKS", "GPE_XASM_TARGET_BLOCKS",
         "GPE_TYPED_TARGET_BLOCKS", "GPE_MIN_GROUP_TILES",
         "GPE_ASM_DEEP_WAVES", "GPE_F_WAVES", "GPE_B_LANES", "GPE_TYPED_ASM",
         "GPE_TYPED_PMAX", "GPE_TYPED_WAVES", "GPE_EXACT_ALL", "GPE_DIAG")
BASE = {"GPE_TARGET_BLOCKS": "256"}
MAX_ASM_WAVES = 16                # gpe_create: waves * 64 <= the core's block

_CACHE = {}                       # populations, data, references, base runs


def _cached(key, make):
    if key not in _CACHE:
        t0 = time.perf_counter()
        _CACHE[key] = make()
        if key[0] == "ref":
            print("LGREF|%s|%.2f s" % ("/".join(map(str, key[1:])),
                                       time.perf_counter() - t0))
    return _CACHE[key]


# ------------------------------------------------------------- reference --
class Values(object):
    """``func(*row)`` of every program at every case (float64; the psets'
    ints are small) and the exceptions it raised, by case."""

    def __init__(self, pset, pop, X):
        rows = list(zip(*X.tolist()))
        self.F = np.empty((len(pop), len(rows)), dtype=np.float64)
        self.exc = [dict() for _ in pop]
        for i, tree in enumerate(pop):
            func = gp.compile(tree, pset)
            try:
                self.F[i] = [func(*row) for row in rows]
            except ERRORS:
                self.patch(i, func, rows, range(len(rows)))

    def patch(self, i, func, rows, cases):
        for c in cases:
            self.exc[i].pop(c, None)
            try:
                self.F[i, c] = func(*rows[c])
            except ERRORS as exc:
                self.exc[i][c] = type(exc).__name__
                self.F[i, c] = np.nan


def _residual_squares(vals, i, terms, n):
    """``(func(*row) - t0 - t1 ...)**2`` of program *i*'s first *n* cases as
    the reference computes them, or the name of the first exception."""
    with np.errstate(all="ignore"):
        d = vals.F[i, :n].copy()
        for t in terms:
            d = d - t[:n]                       # the same IEEE subtraction
    first = min((c for c in vals.exc[i] if c < n), default=None)
    d = d.tolist()
    try:
        return [x ** 2 for x in d], first       # Python's float ** 2
    except OverflowError:
        sq = []
        for c, x in enumerate(d):
            if first is not None and c >= first:
                break
            try:
                sq.append(x ** 2)
            except OverflowError:
                return "OverflowError", c
        return sq, first


def mse_reference(vals, terms, n):
    out = []
    for i in range(vals.F.shape[0]):
        sq, first = _residual_squares(vals, i, terms, n)
        if isinstance(sq, str):
            out.append(sq)
        elif first is not None:
            out.append(vals.exc[i][first])
        else:
            try:
                out.append(math.fsum(sq) / n)
            except OverflowError:
                out.append("OverflowError")
    return out


def check_mse(pop, got, exp, what):
    assert len(got) == len(exp) == len(pop)
    for tree, res, e in zip(pop, got, exp):
        if isinstance(e, str):
            assert isinstance(res, BaseException) and \
                type(res).__name__ == e, (what, str(tree)[:120], res, e)
            continue
        assert not isinstance(res, BaseException), \
            (what, str(tree)[:120], res, e)
        v = res[0]
        if math.isnan(e):
            assert math.isnan(v), (what, str(tree)[:120], v)
        elif math.isinf(e) or e == 0.0:
            assert v == e, (what, str(tree)[:120], v, e)
        else:
            assert abs(v - e) <= REL * abs(e), (what, str(tree)[:120], v, e)


def _same_bits(a, b):
    if isinstance(a, BaseException) or isinstance(b, BaseException):
        return type(a) is type(b)
    return len(a) == len(b) and all(
        x == y and math.copysign(1, x) == math.copysign(1, y) or
        (x != x and y != y) for x, y in zip(a, b))


def n_differ(got, base):
    return sum(not _same_bits(a, b) for a, b in zip(got, base))


# ----------------------------------------------------------- plan checks --
def check_plan(s, n_units, per_tile, lds_cap=None):
    """The plan invariants of one launch; *per_tile*: the units (cases, or
    32-case words) of one of its tiles."""
    assert s["programs"] > 0 and s["lds_bytes"] > 0, s
    assert s["n_slots"] == s["waves"] * s["P"], s
    assert s["waves"] % s["wpb"] == 0, s
    assert (s["waves"] - s["wpb"]) * s["P"] < s["programs"] <= s["n_slots"], s
    assert (s["groups"] - 1) * s["tiles_per_group"] < s["n_tiles"] \
        <= s["groups"] * s["tiles_per_group"], s
    assert s["n_tiles"] == max(1, -(-n_units // per_tile)), (s, n_units)
    if lds_cap is not None and s["P"] > 1:
        assert s["lds_bytes"] <= lds_cap, (s, lds_cap)


def report(cell, data, which, s, ndiff):
    print("LG|%s|%s|%s|P=%d|wpb=%d|groups=%d|tpg=%d|dbuf=%d|lds=%d|differ=%s"
          % (cell, data, which, s["P"], s["wpb"], s["groups"],
             s["tiles_per_group"], s["dbuf"], s["lds_bytes"], ndiff))


def set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(BASE, **knobs).items():
        monkeypatch.setenv(k, str(v))


def run(monkeypatch, knobs, make_ev, pop):
    """One evaluator under *knobs*: ``(results, geometry, shapes)``; the
    context is closed before returning."""
    set_knobs(monkeypatch, knobs)
    ev = make_ev()
    try:
        got = ev.evaluate(pop)
        geo = ev.ctx.geometry()
        shapes = {w: ev.ctx.launch_shape(w) for w in ev.ctx.LAUNCHES}
    finally:
        ev.ctx.close()
    return got, geo, shapes


def base_run(monkeypatch, key, make_ev, pop):
    return _cached(("base",) + key,
                   lambda: run(monkeypatch, {}, make_ev, pop)[0])


# ============================================ A: the exact fast asm core ==
A_CASES = 3950                    # every case count below is a prefix
A_SEED = 11


def pop_a():
    return _cached(("pop", "A"), lambda: configs.population(
        configs.pset_for("symreg10"), "half", 1000, 31, 2, 5))


def data_a():
    return _cached(("data", "A"),
                   lambda: datasets.symreg10_cases(A_CASES, A_SEED))


def values_a():
    return _cached(("ref", "A", "values"), lambda: Values(
        configs.pset_for("symreg10"), pop_a(), data_a()[0]))


SPECIAL_N = 1100
# (column, case, value): the first tile and the last, partial tile (cases
# 1024..1099); 2e8 is a finite sin/cos argument past the exact core's range
SPECIAL = [(0, 3, np.nan), (1, 17, 2e8), (2, 40, 1e200), (3, 70, 2e8),
           (4, 100, 2e8), (5, 127, np.inf), (6, 1024, 2e8), (7, 1060, 1e200),
           (8, 1090, 2e8), (9, 1098, np.nan), (0, 1095, 2e8),
           (1, 1099, -np.inf)]


def data_special():
    def make():
        X, Y = data_a()
        X = np.ascontiguousarray(X[:, :SPECIAL_N]).copy()
        for col, case, v in SPECIAL:
            X[col, case] = v
        return X, np.ascontiguousarray(Y[:, :SPECIAL_N])
    return _cached(("data", "A'"), make)


def values_special():
    def make():
        import copy
        base = values_a()
        vals = copy.copy(base)
        vals.F = base.F[:, :SPECIAL_N].copy()
        vals.exc = [{c: e for c, e in d.items() if c < SPECIAL_N}
                    for d in base.exc]
        pset = configs.pset_for("symreg10")
        rows = list(zip(*data_special()[0].tolist()))
        cases = sorted({case for _, case, _ in SPECIAL})
        for i, tree in enumerate(pop_a()):
            vals.patch(i, gp.compile(tree, pset), rows, cases)
        return vals
    return _cached(("ref", "A'", "values"), make)


# data id -> (cases, trig leaves, special values)
A_DATA = {"1100": (1100, False, False), "1100t": (1100, True, False),
          "1101": (1101, False, False), "2900": (2900, False, False),
          "2950": (2950, False, False), "3950": (3950, False, False),
          "129": (129, False, False),
          "1100s": (SPECIAL_N, False, True)}
# (2900 cases: 23 tiles.  No count of 1100, 1101, 2950 and 129 can give a
# multiple of 8 groups with a short last one: 24 tiles in 8 groups are 3
# each, 9 tiles make 9 or 5 groups.)


def a_inputs(did):
    n, leaves, special = A_DATA[did]
    if special:
        X, Y = data_special()
        vals = values_special()
    else:
        X, Y = data_a()
        X, Y = np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(Y[:, :n])
        vals = values_a()
    exp = _cached(("ref", "A", "mse", n, special),
                  lambda: mse_reference(vals, Y, n))
    pset = configs.pset_for("symreg10")
    return (lambda: GPUEvaluator(pset, SymbRegMSE(X, Y), device=0,
                                 trig_leaves=leaves)), exp, n


# cell id -> (knobs, {data id: property of the asm_fast shape}); the
# property of every other data id is only reported
def _p_is(p):
    return lambda s: s["P"] == p


A_CELLS = {
    # the LDS fit (80 KiB, 8 waves, 11 tile columns twice) leaves P = 6
    "base": ({}, {"1100": lambda s: s["P"] == 6 and s["dbuf"] == 1 and
                  s["tiles_per_group"] == 1 and s["wpb"] == 8,
                  "1100t": lambda s: s["P"] == 5 and s["dbuf"] == 0,
                  "1101": lambda s: s["P"] == 7 and s["dbuf"] == 0,
                  "2950": lambda s: s["P"] == 6 and s["n_tiles"] == 24,
                  "129": lambda s: 1 <= s["P"] <= 2 and s["n_tiles"] == 2,
                  "1100s": lambda s: s["P"] == 6}),
    "P1": ({"GPE_ASM_P": 1}, {d: _p_is(1) for d in A_DATA}),
    "P2": ({"GPE_ASM_P": 2}, {"1100": _p_is(2), "1100t": _p_is(2),
                              "1101": _p_is(2), "2950": _p_is(2)}),
    "P3": ({"GPE_ASM_P": 3}, {"1100": _p_is(3), "1100t": _p_is(3),
                              "1101": _p_is(3), "2950": _p_is(3)}),
    "P5": ({"GPE_ASM_P": 5}, {"1100": _p_is(5), "1100t": _p_is(5),
                              "1101": _p_is(5), "2950": _p_is(5),
                              "1100s": _p_is(5)}),
    # asked 8: the fit leaves 6 (two buffers), 7 (one), 5 (31 columns)
    "P8": ({"GPE_ASM_P": 8}, {"1100": _p_is(6), "1101": _p_is(7),
                              "1100t": _p_is(5)}),
    "W2": ({"GPE_ASM_WAVES": 2},
           {d: (lambda s: s["wpb"] == 2) for d in A_DATA}),
    "W4": ({"GPE_ASM_WAVES": 4},
           {d: (lambda s: s["wpb"] == 4) for d in A_DATA}),
    "W8": ({"GPE_ASM_WAVES": 8},
           {d: (lambda s: s["wpb"] == 8) for d in A_DATA}),
    "Wmax": ({"GPE_ASM_WAVES": MAX_ASM_WAVES},
             {d: (lambda s: s["wpb"] == MAX_ASM_WAVES) for d in A_DATA}),
    "LDS48": ({"GPE_ASM_LDS_KB": 48},
              {"1100": lambda s: 1 < s["P"] < 6 and
               s["lds_bytes"] <= 48 * 1024}),
    "LDS80": ({"GPE_ASM_LDS_KB": 80},
              {"1100": lambda s: s["P"] == 6 and 48 * 1024 < s["lds_bytes"]}),
    "LDS160": ({"GPE_ASM_LDS_KB": 160},
               {"1100": lambda s: s["P"] == 8 and 80 * 1024 < s["lds_bytes"],
                "1100t": lambda s: s["P"] == 8}),
    "DBUF0": ({"GPE_ASM_DBUF": 0},
              {d: (lambda s: s["dbuf"] == 0) for d in A_DATA}),
    "DBUF1": ({"GPE_ASM_DBUF": 1},
              {"1100": lambda s: s["dbuf"] == 1,
               "2950": lambda s: s["dbuf"] == 1,
               "1100s": lambda s: s["dbuf"] == 1,
               "1101": lambda s: s["dbuf"] == 0}),     # odd: turned off
    # (the deal is not part of the shape: a reversal or rotation moves
    # something only with several programs per wave)
    "MIX0": ({"GPE_DEAL_MIX": 0}, {"1100": lambda s: s["P"] >= 3}),
    "MIX1": ({"GPE_DEAL_MIX": 1}, {"1100": lambda s: s["P"] >= 3,
                                   "1101": lambda s: s["P"] >= 3}),
    "MIX2": ({"GPE_DEAL_MIX": 2}, {"1100": lambda s: s["P"] >= 3,
                                   "1101": lambda s: s["P"] >= 3}),
    # tile groups: one tile each is the base; several tiles with a short
    # last group, the groups no multiple of 8 ...
    "GROUPS_ODD": ({"GPE_XASM_TARGET_BLOCKS": 64},
                   {"2900": lambda s: s["groups"] % 8 != 0 and
                    s["tiles_per_group"] >= 2 and
                    s["n_tiles"] % s["tiles_per_group"] != 0 and
                    s["dbuf"] == 1,
                    "1101": lambda s: s["groups"] % 8 != 0 and
                    s["tiles_per_group"] >= 2}),
    # ... and a multiple of 8 (the XCD remap); with two buffers an odd
    # (2900: 3) and an even (1100: 2) count of tiles per group
    "GROUPS_XCD": ({"GPE_MIN_GROUP_TILES": 2},
                   {"2900": lambda s: s["groups"] % 8 == 0 and
                    s["tiles_per_group"] >= 2 and
                    s["n_tiles"] % s["tiles_per_group"] != 0 and
                    s["tiles_per_group"] % 2 == 1 and s["dbuf"] == 1,
                    "2950": lambda s: s["groups"] % 8 == 0 and
                    s["tiles_per_group"] >= 2,
                    # 31 tiles: 8 groups of 4, the last of 3
                    "3950": lambda s: s["groups"] % 8 == 0 and
                    s["tiles_per_group"] % 2 == 0 and
                    s["n_tiles"] % s["tiles_per_group"] != 0 and
                    s["dbuf"] == 1,
                    "1100": lambda s: s["tiles_per_group"] == 2 and
                    s["n_tiles"] % 2 == 1 and s["dbuf"] == 1,
                    "1100s": lambda s: s["tiles_per_group"] == 2 and
                    s["dbuf"] == 1}),
    "PMAX_DBUF1_MIX2": ({"GPE_ASM_P": 16, "GPE_ASM_DBUF": 1,
                         "GPE_DEAL_MIX": 2},
                        {"1100": lambda s: s["P"] >= 5 and s["dbuf"] == 1,
                         "2950": lambda s: s["P"] >= 5 and s["dbuf"] == 1}),
    "P5_W2": ({"GPE_ASM_P": 5, "GPE_ASM_WAVES": 2},
              {"1100": lambda s: s["P"] == 5 and s["wpb"] == 2,
               "1100t": lambda s: s["P"] == 5 and s["wpb"] == 2}),
    "P2_Wmax": ({"GPE_ASM_P": 2, "GPE_ASM_WAVES": MAX_ASM_WAVES},
                {"1100": lambda s: s["P"] == 2 and s["wpb"] == MAX_ASM_WAVES,
                 "1100t": lambda s: s["wpb"] == MAX_ASM_WAVES}),
}


@pytest.mark.parametrize("cell", list(A_CELLS))
def test_exact_fast_core(cell, monkeypatch):
    """A and A': 1000 programs (not a multiple of P * waves per block: the
    last wave is partly -1 and whole padding waves exist), 8 full tiles and
    one of 76 cases (and 1101, 2900, 2950, 129 cases; trig-leaf columns;
    special values), one knob at a time around the base."""
    knobs, want = A_CELLS[cell]
    pop = pop_a()
    for did in A_DATA:
        make_ev, exp, n = a_inputs(did)
        base = base_run(monkeypatch, ("A", did), make_ev, pop)
        got, geo, shapes = run(monkeypatch, knobs, make_ev, pop)
        s = shapes["asm_fast"]
        report("A:" + cell, did, "asm_fast", s, n_differ(got, base))
        assert geo["asm"] == len(pop) and s["programs"] == len(pop), geo
        assert s["K"] == 2 and s["sdepth"] <= 5, s
        check_plan(s, n, 64 * s["K"],
                   int(knobs.get("GPE_ASM_LDS_KB", 80)) * 1024)
        assert s["dbuf"] == 0 or n % 2 == 0, s
        if did in want:
            assert want[did](s), (cell, did, s)
        if A_DATA[did][2]:
            # the (program, tile) pair pass ran, here on a partial tile
            assert geo["redo_exact_cpp"] > 0, geo
        check_mse(pop, got, exp, (cell, did))


# ------------------------------------------- A'': other accumulation paths
A2_CELLS = {"base": {}, "P5": {"GPE_ASM_P": 5}, "DBUF0": {"GPE_ASM_DBUF": 0},
            "GROUPS_XCD": {"GPE_MIN_GROUP_TILES": 2},
            "MIX2_W4": {"GPE_DEAL_MIX": 2, "GPE_ASM_WAVES": 4}}


@pytest.mark.parametrize("cell", list(A2_CELLS))
def test_exact_fast_core_two_target_columns(cell, monkeypatch):
    """Two target rows (not the lean epilogue): ``f - t0 - t1``."""
    pop, n = pop_a(), 1100
    X, Y = data_a()
    X = np.ascontiguousarray(X[:, :n])
    T = np.ascontiguousarray(np.vstack([
        Y[0, :n], np.random.default_rng(5).uniform(-2, 2, n)]))
    exp = _cached(("ref", "A", "mse2", n),
                  lambda: mse_reference(values_a(), T, n))
    pset = configs.pset_for("symreg10")

    def make_ev():
        return GPUEvaluator(pset, SymbRegMSE(X, T), device=0,
                            trig_leaves=False)
    base = base_run(monkeypatch, ("A2", n), make_ev, pop)
    got, geo, shapes = run(monkeypatch, A2_CELLS[cell], make_ev, pop)
    s = shapes["asm_fast"]
    report("A2:" + cell, n, "asm_fast", s, n_differ(got, base))
    assert s["programs"] == len(pop) and s["P"] >= 4, s
    check_plan(s, n, 64 * s["K"], 80 * 1024)
    check_mse(pop, got, exp, cell)


@pytest.mark.parametrize("cell", list(A2_CELLS))
def test_exact_fast_core_per_case_output(cell, monkeypatch):
    """Per-case output of 200 of the programs over 2950 cases (P = 4), as
    test_per_case_errors_match_reference_cases compares it."""
    pop, n = pop_a()[100:300], 2950
    X, Y = data_a()
    X, Y = np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(Y[:, :n])
    vals = values_a()
    pset = configs.pset_for("symreg10")

    def make_ev():
        return GPUEvaluator(pset, SymbRegCaseErrors(X, Y), device=0,
                            trig_leaves=False)
    base = base_run(monkeypatch, ("A2cases", n), make_ev, pop)
    got, geo, shapes = run(monkeypatch, A2_CELLS[cell], make_ev, pop)
    s = shapes["asm_fast"]
    report("A2cases:" + cell, n, "asm_fast", s, n_differ(got, base))
    assert s["programs"] == len(pop) and s["P"] >= 3, s
    check_plan(s, n, 64 * s["K"], 80 * 1024)
    same = total = 0
    for i, (tree, res) in enumerate(zip(pop, got)):
        sq, first = _residual_squares(vals, 100 + i, Y, n)
        if isinstance(sq, str) or first is not None:
            name = sq if isinstance(sq, str) else vals.exc[100 + i][first]
            assert isinstance(res, BaseException) and \
                type(res).__name__ == name, (str(tree), res, name)
            continue
        assert len(res) == n
        for a, b in zip(res, sq):
            total += 1
            if a == b or (math.isnan(a) and math.isnan(b)):
                same += 1
            else:
                assert abs(a - b) <= REL * abs(b), (str(tree), a, b)
    assert total > 0 and same >= 0.99 * total


# ============================================ B: the exact deep asm core ==
def _bushy(rnd, height, plain=False):
    """A tree whose binary nodes all have two subtrees of the same height:
    it needs ``height - 1`` operand-stack slots (its Strahler number), the
    fewest nodes that do; sin, cos and neg are sprinkled over it (*plain*:
    argument leaves only, sin and cos only)."""
    if height == 0:
        return "ARG%d" % rnd.randrange(10) if plain or rnd.random() < 0.9 \
            else str(rnd.choice((-1, 0, 1)))
    op = rnd.choices(["add", "sub", "mul", "protectedDiv"],
                     [35, 35, 20, 10])[0]
    s = "%s(%s, %s)" % (op, _bushy(rnd, height - 1, plain),
                        _bushy(rnd, height - 1, plain))
    if plain and rnd.random() < 0.08:
        s = "%s(%s)" % (rnd.choice(("sin", "cos")), s)
    elif not plain and rnd.random() < 0.12:
        s = "%s(%s)" % (rnd.choice(("sin", "cos", "neg")), s)
    return s


# (height, trees): 6 slots need 255 nodes, 9 slots 2047, 11 slots 8191 (12
# would need 16383) — most trees are small, since the reference walks every
# node of every case; one tree each of 10 and 11 slots (DEEP_TOP)
DEEP_MIX = [(7, 300), (8, 70), (9, 22), (10, 6)]
DEEP_TOP = (10, 11)


def pop_deep():
    """400 trees needing 6..11 operand-stack slots (the deep cores hold
    6..12), the smallest first."""
    def make():
        import random
        pset = configs.pset_for("symreg10")
        rnd = random.Random(77)
        pop = []
        for h, count in DEEP_MIX:
            # (folded constants and negations may save a slot or two)
            keep = []
            for _ in range(8):
                if len(keep) >= count:
                    break
                pool = [gp.PrimitiveTree.from_string(_bushy(rnd, h), pset)
                        for _ in range(count)]
                depth = Flattener(pset).flatten(pool).depth
                keep += [t for t, d in zip(pool, depth) if 6 <= d <= 12]
            pop += keep[:count]
        top = [gp.PrimitiveTree.from_string(_bushy(rnd, d + 1, True), pset)
               for d in DEEP_TOP]
        assert Flattener(pset).flatten(top).depth.tolist() == list(DEEP_TOP)
        pop += top
        assert len(pop) == 400
        return pop
    return _cached(("pop", "deep"), make)


B_CELLS = {
    "base": ({}, lambda s: s["P"] == 2 and s["wpb"] == 4),
    "DW4": ({"GPE_ASM_DEEP_WAVES": 4}, lambda s: s["P"] == 2 and s["wpb"] == 4),
    "DW8": ({"GPE_ASM_DEEP_WAVES": 8}, lambda s: s["P"] == 2 and s["wpb"] == 8),
    "P1": ({"GPE_ASM_P": 1}, lambda s: s["P"] == 1),
    "DBUF0": ({"GPE_ASM_DBUF": 0}, lambda s: s["P"] == 2 and s["dbuf"] == 0),
    "GROUPS": ({"GPE_ASM_TARGET_BLOCKS": 256, "GPE_DEAL_MIX": 1},
               lambda s: s["P"] == 2 and s["tiles_per_group"] >= 2),
}


@pytest.mark.parametrize("cell", list(B_CELLS))
def test_exact_deep_core(cell, monkeypatch):
    """400 programs of 6..11 stack slots, 5 full tiles and one of 60."""
    knobs, want = B_CELLS[cell]
    pop, n = pop_deep(), 700
    X, Y = data_a()
    X, Y = np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(Y[:, :n])
    pset = configs.pset_for("symreg10")
    vals = _cached(("ref", "B", "values"), lambda: Values(pset, pop, X))
    exp = _cached(("ref", "B", "mse", n), lambda: mse_reference(vals, Y, n))

    def make_ev():
        return GPUEvaluator(pset, SymbRegMSE(X, Y), device=0,
                            trig_leaves=False)
    base = base_run(monkeypatch, ("B", n), make_ev, pop)
    got, geo, shapes = run(monkeypatch, knobs, make_ev, pop)
    s = shapes["asm_deep"]
    report("B:" + cell, n, "asm_deep", s, n_differ(got, base))
    assert geo["asm_deep"] == len(pop) and s["programs"] == len(pop), geo
    assert s["K"] == 2 and 6 <= s["sdepth"] <= 12, s
    check_plan(s, n, 64 * s["K"], 48 * 1024)
    assert want(s), (cell, s)
    check_mse(pop, got, exp, cell)


# ======================================================= C: fp32 cores ==
C_CELLS = {
    "base": ({}, lambda f, d: f["P"] >= 4 and d["P"] == 2),
    "P2": ({"GPE_ASM_P": 2}, lambda f, d: f["P"] == 2 and d["P"] == 2),
    "P5_W4": ({"GPE_ASM_P": 5, "GPE_ASM_WAVES": 4},
              lambda f, d: f["P"] == 5 and f["wpb"] == 4),
    "DW8": ({"GPE_ASM_DEEP_WAVES": 8}, lambda f, d: d["wpb"] == 8),
    "DW4_MIX1": ({"GPE_ASM_DEEP_WAVES": 4, "GPE_DEAL_MIX": 1},
                 lambda f, d: d["wpb"] == 4 and f["P"] >= 4),
}


@pytest.mark.parametrize("cell", list(C_CELLS))
def test_fp32_cores(cell, monkeypatch):
    """Population A plus 200 deep trees in fp32 mode over 2950 cases (a
    partial tile of the fp32 cores' 64 K cases): the fp64 reference under
    test_fp32_mode_stated_tolerance's C4 rule, and the fp32 C++ kernels
    (GPE_ASM=0) as test_fp32_asm_cores_match_fp32_cpp_kernels compares."""
    knobs, want = C_CELLS[cell]
    n = 2950
    pop = pop_a() + pop_deep()[:200]
    X, Y = data_a()
    X, Y = np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(Y[:, :n])
    pset = configs.pset_for("symreg10")
    deep_vals = _cached(("ref", "C", "values"),
                        lambda: Values(pset, pop_deep()[:200], X))

    def reference():
        return mse_reference(values_a(), Y, n) + mse_reference(deep_vals, Y, n)
    exp = _cached(("ref", "C", "mse", n), reference)

    def make_ev():
        return GPUEvaluator(pset, SymbRegMSE(X, Y), device=0,
                            precision="fp32")
    cpp = _cached(("base", "C", "cpp"),
                  lambda: run(monkeypatch, {"GPE_ASM": 0}, make_ev, pop))
    assert cpp[1]["asm"] == 0, cpp[1]
    base = base_run(monkeypatch, ("C", n), make_ev, pop)
    got, geo, shapes = run(monkeypatch, knobs, make_ev, pop)
    f, d = shapes["asm_fast"], shapes["asm_deep"]
    report("C:" + cell, n, "asm_fast", f, n_differ(got, base))
    report("C:" + cell, n, "asm_deep", d, n_differ(got, base))
    assert geo["asm"] == len(pop) and d["programs"] >= 100, geo
    assert f["programs"] + d["programs"] == len(pop)
    for s in (f, d):
        assert s["K"] == 4 and n % (64 * s["K"]) != 0, s
        check_plan(s, n, 64 * s["K"],
                   (48 if s is d else 80) * 1024)
    assert want(f, d), (cell, f, d)
    rel = []
    for res, e in zip(got, exp):
        if isinstance(e, str) or isinstance(res, BaseException):
            continue
        if math.isfinite(e) and math.isfinite(res[0]):
            rel.append(abs(res[0] - e) / max(abs(e), 1e-300))
    r = np.array(rel)
    print("LGC|%s|n=%d|median=%.3g|<=1e-4: %.4f|<=1e-3: %.4f"
          % (cell, len(r), np.median(r), (r <= 1e-4).mean(),
             (r <= 1e-3).mean()))
    assert len(r) >= 0.8 * len(pop)
    assert np.median(r) <= 1e-5 and (r <= 1e-4).mean() >= 0.80 \
        and (r <= 1e-3).mean() >= 0.90
    for a, b, t in zip(got, cpp[0], pop):
        if isinstance(b, BaseException):
            assert type(a) is type(b), str(t)[:120]
            continue
        assert not isinstance(a, BaseException), (str(t)[:120], a)
        x, y = a[0], b[0]
        assert x == y or abs(x - y) <= 1e-12 * abs(y) or \
            (math.isnan(x) and math.isnan(y)), (str(t)[:120], x, y)


# =================================================== D: C++ F kernels ==
@pytest.mark.parametrize("waves", [4, 8])
def test_cpp_f_kernels(waves, monkeypatch):
    """40 variables (past the asm cores' 32): the C++ kernels at P >= 4."""
    n = 1100
    pset = _cached(("pset", "arith40"), lambda: configs.arith_pset(40))
    pop = _cached(("pop", "D"),
                  lambda: configs.population(pset, "half", 1000, 41, 2, 5))
    rng = np.random.default_rng(40)
    X, Y = _cached(("data", "D"), lambda: (rng.uniform(-3, 3, size=(40, n)),
                                           rng.uniform(-2, 2, size=(1, n))))
    vals = _cached(("ref", "D", "values"), lambda: Values(pset, pop, X))
    exp = _cached(("ref", "D", "mse", n), lambda: mse_reference(vals, Y, n))

    def make_ev():
        return GPUEvaluator(pset, SymbRegMSE(X, Y), device=0,
                            trig_leaves=False)
    base = base_run(monkeypatch, ("D", n), make_ev, pop)
    got, geo, shapes = run(monkeypatch, {"GPE_F_WAVES": waves}, make_ev, pop)
    # (programs that read only the first 32 variables still fit the asm core)
    assert geo["asm"] + geo["fast"] + geo["deep"] == len(pop), geo
    if geo["asm"]:
        a = shapes["asm_fast"]
        report("D:F_WAVES%d" % waves, n, "asm_fast", a, n_differ(got, base))
        check_plan(a, n, 64 * a["K"], 80 * 1024)
    s = shapes["cpp_fast"]
    report("D:F_WAVES%d" % waves, n, "cpp_fast", s, n_differ(got, base))
    # the fast kernel stages 64 * 2 cases per tile, the deep one 64
    check_plan(s, n, 128)
    # (8 waves are taken while (40 + 1 + 8 * stack slots) KiB fit 80 KiB:
    # this population needs at most 4 slots)
    assert s["sdepth"] <= 4, s
    assert s["P"] >= 4 and s["wpb"] == waves and s["K"] == 0, s
    if shapes["cpp_deep"]["programs"]:
        check_plan(shapes["cpp_deep"], n, 64)
    check_mse(pop, got, exp, waves)


# =================================================== E: boolean kernels ==
E_CASES = [1, 31, 33, 50, 65, 100, 257, 511, 512, 513, 2049]


def bool_inputs(name):
    def make():
        pset = configs.pset_for(name)
        nv = len(pset.arguments)
        rng = np.random.default_rng(nv)
        ins = rng.integers(0, 2, size=(nv, max(E_CASES)))
        outs = rng.integers(0, 2, size=max(E_CASES))
        pop = configs.population(pset, "full", 300, nv, 2, 5)
        return pset, pop, ins, outs
    return _cached(("data", "E", name), make)


def bool_hits(name):
    """hit[program, case] = ``func(*in_) == out``."""
    def make():
        pset, pop, ins, outs = bool_inputs(name)
        rows, out = list(zip(*ins.tolist())), outs.tolist()
        hit = np.zeros((len(pop), len(out)), dtype=np.int64)
        for i, tree in enumerate(pop):
            func = gp.compile(tree, pset)
            hit[i] = [func(*r) == o for r, o in zip(rows, out)]
        return hit
    return _cached(("ref", "E", name), make)


@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("n_cases", E_CASES)
@pytest.mark.parametrize("name", ["parity6", "mux11"])
def test_boolean_kernels(name, n_cases, lanes, monkeypatch):
    """Every lane-group width of the lane-packed kernel (1, 2, 4, 8, 16
    words), 17 words and two tiles of the word-tiled kernel, partial words."""
    pset, pop, ins, outs = bool_inputs(name)
    exp = bool_hits(name)[:, :n_cases].sum(axis=1).tolist()

    def make_ev():
        return GPUEvaluator(pset, BooleanHits(ins[:, :n_cases],
                                              outs[:n_cases]), device=0)
    base = base_run(monkeypatch, ("E", name, n_cases), make_ev, pop)
    got, geo, shapes = run(monkeypatch, {"GPE_B_LANES": lanes}, make_ev, pop)
    words = -(-n_cases // 32)
    group = 0
    if lanes and words <= 16:
        group = 1
        while group < words:
            group *= 2
    total = 0
    for which in ("cpp_fast", "cpp_deep"):
        s = shapes[which]
        if not s["programs"]:
            continue
        total += s["programs"]
        report("E:%s:lanes%d" % (name, lanes), n_cases, which, s,
               n_differ(got, base))
        check_plan(s, words, 64)                 # 64 words per tile
        assert s["P"] == (64 // group if group else 1) and s["wpb"] == 4, s
    assert total == len(pop)
    assert [h for (h,) in got] == exp


# ======================================================= F: typed core ==
def typed_inputs():
    def make():
        pset = configs.pset_for("spambase")
        X, lab = datasets.spambase_like(1000, 57)
        pop = configs.population(pset, "half", 12000, 57, 2, 4)
        return pset, pop, X, lab
    return _cached(("data", "F"), make)


def typed_hits(lo, hi, n_cases):
    """hit[program, case] = ``bool(func(*row)) is bool(label)`` of programs
    lo..hi, per case in plain Python."""
    def make():
        pset, pop, X, lab = typed_inputs()
        rows = list(zip(*X[:, :n_cases].tolist()))
        labels = [bool(v) for v in lab[:n_cases].tolist()]
        hit = np.zeros((hi - lo, n_cases), dtype=np.int64)
        for i, tree in enumerate(pop[lo:hi]):
            func = gp.compile(tree, pset)
            hit[i] = [bool(func(*r)) is b for r, b in zip(rows, labels)]
        return hit
    return _cached(("ref", "F", lo, hi, n_cases), make)


def _np_div(left, right):
    with np.errstate(all="ignore"):
        return np.where(np.asarray(right) == 0, 1.0,
                        np.divide(left, np.where(np.asarray(right) == 0, 1.0,
                                                 right)))


def typed_hits_vectorised(lo, hi, n_cases):
    """hit[program, case] with the same primitives on whole columns
    (numpy), for the large population only; proven equal to typed_hits on
    256 programs, hit for hit, first."""
    pset, pop, X, lab = typed_inputs()
    ctx = {"__builtins__": None, "True": True, "False": False,
           "and_": np.logical_and, "or_": np.logical_or,
           "not_": np.logical_not, "add": np.add, "sub": np.subtract,
           "mul": np.multiply, "protectedDiv": _np_div, "lt": np.less,
           "eq": np.equal,
           "if_then_else": lambda c, a, b: np.where(c, a, b)}
    cols = [X[i, :n_cases] for i in range(X.shape[0])]
    labels = lab[:n_cases] != 0
    out = np.zeros((hi - lo, n_cases), dtype=bool)
    with np.errstate(all="ignore"):
        for i, tree in enumerate(pop[lo:hi]):
            func = eval("lambda %s: %s" % (",".join(pset.arguments),
                                           str(tree)), dict(ctx), {})
            res = np.broadcast_to(np.asarray(func(*cols)) != 0, labels.shape)
            out[i] = res == labels
    return out


def check_typed(s, geo, n_cases):
    assert geo["asm_typed"] == s["programs"], (geo, s)
    check_plan(s, n_cases, 64 * s["K"])
    assert s["K"] == 2 and s["dbuf"] == 0, s


@pytest.mark.parametrize("n_cases", [1, 127, 129, 300])
@pytest.mark.parametrize("waves", [1, 3, 8, 16])
def test_typed_core_waves(waves, n_cases, monkeypatch):
    """1000 spambase programs on the typed core, GPE_TYPED_WAVES."""
    pset, pop, X, lab = typed_inputs()
    pop = pop[:1000]
    exp = typed_hits(0, 1000, 300)[:, :n_cases].sum(axis=1).tolist()

    def make_ev():
        return GPUEvaluator(pset, TypedBoolHits(X[:, :n_cases],
                                                lab[:n_cases]), device=0)
    base = base_run(monkeypatch, ("F", n_cases), make_ev, pop)
    got, geo, shapes = run(monkeypatch, {"GPE_TYPED_WAVES": waves}, make_ev,
                           pop)
    s = shapes["typed"]
    report("F:TW%d" % waves, n_cases, "typed", s, n_differ(got, base))
    assert s["programs"] >= 300 and s["wpb"] == waves, (s, geo)
    check_typed(s, geo, n_cases)
    assert [h for (h,) in got] == exp


@pytest.mark.parametrize("pmax", [1, 7, 64])
def test_typed_core_programs_per_wave(pmax, monkeypatch):
    """12000 programs over 1000 cases (7 full tiles and one of 104): at
    least 8192 of them on the typed core give P = GPE_TYPED_PMAX up to 64."""
    pset, pop, X, lab = typed_inputs()
    n = 1000

    def reference():
        vec = typed_hits_vectorised(0, len(pop), n)
        assert np.array_equal(vec[:256], typed_hits(0, 256, n) != 0)
        return vec.sum(axis=1).tolist()
    exp = _cached(("ref", "F", "vectorised", n), reference)

    def make_ev():
        return GPUEvaluator(pset, TypedBoolHits(X, lab), device=0)
    base = base_run(monkeypatch, ("F", "big", n), make_ev, pop)
    got, geo, shapes = run(monkeypatch, {"GPE_TYPED_PMAX": pmax}, make_ev,
                           pop)
    s = shapes["typed"]
    report("F:PMAX%d" % pmax, n, "typed", s, n_differ(got, base))
    assert s["programs"] >= 8192 and s["P"] == pmax and s["n_tiles"] == 8, s
    check_typed(s, geo, n)
    assert [h for (h,) in got] == exp
