"""The range pass's later classes (csrc/trig_ranges.h, mode 2, the library's
default): midlo (cos, |x| < 1.44), wide (clean, |x| < 1e8) and the
"bounded or NaN" state that lets a sin/cos over a possibly non-finite value
feed mid / small / midlo.  Soundness against sampled evaluation as in
test_trig_ranges.py, the rules on hand-written programs, the share on the
headline population, and programs that really produce an inf.  No GPU.

What a class promises the handlers, for every case inside the column bounds
(corners and 0.0 included):
  small, mid   finite and |x| below glibc's 0.85546875 / 2.426265, or NaN
  midlo        finite and |x| < 1.44 (so pi/2 - |x| > 0.126), or NaN
  wide         finite and |x| below __branred's 105414350 — never NaN
and never an inf in any of them.
"""
import math
import struct

import numpy as np
import pytest

from deap_amd import _lib, configs, gp
from deap_amd.flatten import Flattener
from test_trig_ranges import BOUNDS, HAND, NV, cases, trig_arguments

GENERAL, MID, SMALL, MIDLO, WIDE = range(5)
T_SMALL = 0.85546875
T_MID = struct.unpack("<d", struct.pack("<Q", 0x400368fd << 32))[0]
T_BRANRED = struct.unpack("<d", struct.pack("<Q", 0x419921fb << 32))[0]
LIMIT = {SMALL: T_SMALL, MID: T_MID, MIDLO: 1.44, WIDE: T_BRANRED}

# protectedDiv by a tiny column, mul to overflow, sin (an inf argument: nan),
# then cos / sin over the nan
INF_PROGRAMS = [
    "cos(sin(mul(protectedDiv(ARG0, ARG3), 1e300)))",
    "sin(cos(mul(protectedDiv(ARG1, ARG3), 1e300)))",
    "cos(mul(ARG2, sin(mul(protectedDiv(1.0, ARG3), 1e300))))",
    "sin(add(cos(mul(protectedDiv(ARG0, ARG3), 1e300)), ARG1))",
    "cos(sub(ARG0, cos(sin(mul(protectedDiv(ARG0, ARG3), 1e300)))))",
    "cos(protectedDiv(sin(mul(protectedDiv(ARG0, ARG3), 1e300)), add(ARG1, 2.0)))",
]


@pytest.fixture(scope="module")
def pset():
    return configs.pset_for("symreg10")


def words_of(pset, pop):
    batch = Flattener(pset).flatten(pop)
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    return [code[off[i]:off[i + 1]] for i in range(len(pop))]


@pytest.fixture(scope="module")
def programs(pset):
    pop = configs.population(pset, "half", 1200, 1440, 1, 8)
    pop += [gp.PrimitiveTree.from_string(s, pset) for s in HAND + INF_PROGRAMS]
    return pop, words_of(pset, pop)


def check_node(c, arg, dirty, what):
    if c == GENERAL:
        return
    nan = np.isnan(arg)
    assert not np.isinf(arg).any(), what
    assert np.all(np.abs(arg[~nan]) < LIMIT[c]), (what, c, np.abs(arg[~nan]).max())
    if c == WIDE:
        assert not nan.any() and not dirty, what
    if nan.any():                       # only downstream of a possible inf / nan
        assert dirty, what


@pytest.mark.parametrize("name", list(BOUNDS))
def test_mode2_classes_hold_for_every_sampled_case(programs, name):
    pop, words = programs
    lo = np.array([b[0] for b in BOUNDS[name]])
    hi = np.array([b[1] for b in BOUNDS[name]])
    unbounded = {v for v, b in enumerate(BOUNDS[name]) if math.isinf(b[0])}
    X = cases(name)
    count = [0] * 5
    nan_nodes = 0
    for tree, w in zip(pop, words):
        cls = _lib.debug_trig_classes(w, lo, hi, mode=2)
        base = _lib.debug_trig_classes(w, lo, hi)
        args = trig_arguments(w, X, unbounded)
        assert len(cls) == len(args) == len(base), str(tree)
        for c, b, (arg, dirty) in zip(cls, base, args):
            count[c] += 1
            check_node(c, arg, dirty, (name, str(tree)[:200]))
            nan_nodes += int(c != GENERAL and np.isnan(arg).any())
            # mode 2 only ever refines: what mode 1 proves stays proven
            assert b == GENERAL or c in ((SMALL,) if b == SMALL else (MID, MIDLO)), str(tree)
    print("TRIGCLS2|%s|general=%d mid=%d small=%d midlo=%d wide=%d nan_nodes=%d"
          % ((name,) + tuple(count) + (nan_nodes,)))
    assert sum(count) > 1500
    if name in ("unit", "offset"):
        assert count[MIDLO] > 0
    if name == "wide":
        assert count[WIDE] > 0
    if name == "unbounded3":            # the unbounded column holds inf and nan
        assert nan_nodes > 0


def classes(pset, expr, bounds, mode=2):
    b = Flattener(pset).flatten([gp.PrimitiveTree.from_string(expr, pset)])
    lo, hi = zip(*bounds)
    return list(_lib.debug_trig_classes(b.code, np.array(lo), np.array(hi), mode=mode))


def test_hand_written_rules(pset):
    unit, wide, ub = BOUNDS["unit"], BOUNDS["wide"], BOUNDS["unbounded3"]

    def col(lo, hi):
        return [(lo, hi)] * NV
    # ---- midlo: a cos class, on both sides of 1.44
    assert classes(pset, "cos(ARG0)", col(0.0, np.nextafter(1.44, 0))) == [MIDLO]
    assert classes(pset, "cos(ARG0)", col(0.0, 1.44)) == [MID]
    assert classes(pset, "cos(ARG0)", col(-np.nextafter(1.44, 0), 0.0)) == [MIDLO]
    assert classes(pset, "cos(ARG0)", col(-1.44, 0.0)) == [MID]
    assert classes(pset, "sin(ARG0)", col(0.0, 1.0)) == [MID]      # never a sin
    assert classes(pset, "cos(ARG0)", col(0.0, 0.8)) == [SMALL]
    assert classes(pset, "cos(mul(ARG0, ARG1))", unit) == [MIDLO]
    assert classes(pset, "cos(add(ARG0, ARG1))", unit) == [MID]
    # ---- wide: clean and below 1e8
    assert classes(pset, "sin(add(ARG0, ARG1))", wide) == [WIDE]
    assert classes(pset, "cos(mul(ARG0, ARG1))", wide) == [WIDE]
    assert classes(pset, "sin(ARG0)", col(0.0, np.nextafter(1e8, 0))) == [WIDE]
    assert classes(pset, "sin(ARG0)", col(0.0, 1e8)) == [GENERAL]
    assert classes(pset, "sin(ARG0)", col(-1e8, 0.0)) == [GENERAL]
    # ---- nanable: sin/cos of a tainted value is [-1, 1] or NaN
    assert classes(pset, "sin(cos(protectedDiv(ARG0, ARG3)))", unit) == [GENERAL, MID]
    assert classes(pset, "cos(sin(ARG3))", ub) == [GENERAL, MIDLO]
    assert classes(pset, "cos(mul(0.5, sin(ARG3)))", ub) == [GENERAL, SMALL]
    assert classes(pset, "sin(neg(add(cos(ARG3), ARG0)))", ub) == [GENERAL, MID]
    # ... refused by wide (2.5 .. 3.5 is past mid, and the value may be NaN)
    assert classes(pset, "sin(add(3.0, mul(0.5, cos(ARG3))))", ub) == [GENERAL, GENERAL]
    assert classes(pset, "sin(add(3.0, mul(0.5, cos(ARG0))))", ub) == [MIDLO, WIDE]
    # ... closed under protectedDiv while the denominator excludes 0
    assert classes(pset, "cos(protectedDiv(sin(ARG3), add(ARG0, 2.0)))", ub) == [GENERAL, MIDLO]
    assert classes(pset, "cos(protectedDiv(ARG0, add(sin(ARG3), 2.0)))", ub) == [GENERAL, MIDLO]
    # ... tainted again by a denominator that may be 0 (the exact 0 too), and
    # what follows that is nanable once more
    assert classes(pset, "cos(protectedDiv(ARG0, sin(ARG3)))", ub) == [GENERAL, GENERAL]
    assert classes(pset, "cos(protectedDiv(ARG0, mul(0.0, sin(ARG3))))", ub) == [GENERAL, GENERAL]
    assert classes(pset, "sin(cos(protectedDiv(ARG0, sin(ARG3))))", ub) == [GENERAL, GENERAL, MID]
    # ... and by a bound past kHuge (1e300)
    assert classes(pset, "cos(mul(1e200, mul(1e200, sin(ARG3))))", ub) == [GENERAL, GENERAL]
    assert classes(pset, "cos(mul(1e-200, mul(1e200, sin(ARG3))))", ub) == [GENERAL, MIDLO]
    # ---- mode 1 is the pass without any of this
    assert classes(pset, "sin(cos(protectedDiv(ARG0, ARG3)))", unit, mode=1) == [GENERAL, GENERAL]
    assert classes(pset, "cos(mul(ARG0, ARG1))", unit, mode=1) == [MID]
    assert classes(pset, "sin(add(ARG0, ARG1))", wide, mode=1) == [GENERAL]
    with pytest.raises(_lib.GpeError):
        classes(pset, "sin(ARG0)", unit, mode=3)


def test_headline_share_is_not_below_the_parents(pset):
    """The first 8,192 headline trees, columns [-1, 1]: mode 1 proved a range
    for 75.2 % of the sin/cos nodes; mode 2's mid + small + midlo (wide not
    counted: it keeps the general body's range tests) is not below that."""
    pop = configs.population(pset, "half", 8192, 2024, 4, 8)
    lo, hi = -np.ones(NV), np.ones(NV)
    count = np.zeros(5, dtype=np.int64)
    base = np.zeros(3, dtype=np.int64)
    for w in words_of(pset, pop):
        count += np.bincount(_lib.debug_trig_classes(w, lo, hi, mode=2), minlength=5)
        base += np.bincount(_lib.debug_trig_classes(w, lo, hi), minlength=3)
    total = int(count.sum())
    spec = (count[MID] + count[SMALL] + count[MIDLO]) / total
    print("TRIGCLS2|headline8192|general=%d mid=%d small=%d midlo=%d wide=%d of %d|"
          "specialised %.2f %% (mode 1: %.2f %%), with wide %.2f %%"
          % (tuple(count) + (total, 100 * spec, 100 * (base[1] + base[2]) / total,
                             100 * (total - count[GENERAL]) / total)))
    assert total == base.sum() > 30000
    assert spec >= 0.752
    assert spec >= (base[1] + base[2]) / total


def test_programs_that_produce_inf(pset):
    """ARG3 within [0, 1e-300] (tiny and 0.0: pad lanes): the quotient times
    1e300 overflows in most lanes, the inner sin/cos sees inf and is general,
    and every specialised node above it sees its range or NaN."""
    pop = [gp.PrimitiveTree.from_string(s, pset) for s in INF_PROGRAMS]
    bounds = [(-1.0, 1.0)] * 3 + [(0.0, 1e-300)] + [(-1.0, 1.0)] * (NV - 4)
    lo, hi = (np.array(v) for v in zip(*bounds))
    rng = np.random.default_rng(300)
    X = rng.uniform(-1.0, 1.0, (NV, 256))
    X[3] = rng.uniform(1e-306, 1e-300, 256)
    X[3, :4] = [0.0, 1e-300, 5e-324, 1e-300]
    X[0, :4] = [1.0, -1.0, 1.0, 0.0]
    seen_nan = 0
    for tree, w in zip(pop, words_of(pset, pop)):
        cls = list(_lib.debug_trig_classes(w, lo, hi, mode=2))
        args = trig_arguments(w, X, set())
        assert len(cls) == len(args)
        assert cls[0] == GENERAL and np.isinf(args[0][0]).any(), str(tree)
        assert any(c in (MID, SMALL, MIDLO) for c in cls[1:]), (str(tree), cls)
        for c, (arg, dirty) in zip(cls, args):
            check_node(c, arg, True, str(tree))
            assert c != WIDE
            seen_nan += int(c != GENERAL and np.isnan(arg).any())
        assert list(_lib.debug_trig_classes(w, lo, hi)) == [GENERAL] * len(cls)
    assert seen_nan >= len(pop)


def test_translation_picks_the_new_handlers(pset):
    """gpe_debug_translate with bounds in mode 2: the same word count, only
    sin/cos words differ, each the handler of its class (midlo: COS_MIDLO)."""
    import asm_emu
    try:
        lay = asm_emu.read_layout("_exact")
    except OSError:
        pytest.skip("asm cores not generated")
    pop = configs.population(pset, "half", 300, 79, 1, 6)
    pop += [gp.PrimitiveTree.from_string(s, pset) for s in HAND + INF_PROGRAMS]
    batch = Flattener(pset).flatten(pop)
    table = np.arange(lay["H_COUNT"], dtype=np.uint32) * 4 + 0x1000
    lo = np.array([-1.0] * 3 + [-50.0] + [-1.0] * (NV - 4))
    hi = -lo
    plain, s0 = _lib.debug_translate(batch, NV, table)
    ranged, s1 = _lib.debug_translate(batch, NV, table, bounds=(lo, hi), mode=2)
    assert len(plain) == len(ranged) and np.array_equal(s0, s1)
    name = {("H_SIN", GENERAL): "H_SIN", ("H_SIN", MID): "H_SIN_MID",
            ("H_SIN", SMALL): "H_SIN_SMALL", ("H_SIN", WIDE): "H_SIN_WIDE",
            ("H_COS", GENERAL): "H_COS", ("H_COS", MID): "H_COS_MID",
            ("H_COS", SMALL): "H_COS_SMALL", ("H_COS", MIDLO): "H_COS_MIDLO",
            ("H_COS", WIDE): "H_COS_WIDE"}
    word = {k: int(table[lay[k]]) for k in set(name.values())}
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    seen = set()
    for i in range(len(pop)):
        if s0[i] < 0:
            continue
        end = s0[i + 1:][s0[i + 1:] >= 0]
        a, b = int(s0[i]), int(end[0]) if len(end) else len(plain)
        cls = list(_lib.debug_trig_classes(code[off[i]:off[i + 1]], lo, hi, mode=2))
        trig = [j for j in range(a, b) if plain[j] in (word["H_SIN"], word["H_COS"])]
        assert len(trig) == len(cls), str(pop[i])
        for j in np.nonzero(plain[a:b] != ranged[a:b])[0]:
            assert a + j in trig, str(pop[i])
        for j, c in zip(trig, cls):
            kind = "H_SIN" if plain[j] == word["H_SIN"] else "H_COS"
            assert ranged[j] == word[name[(kind, c)]], str(pop[i])
            seen.add(name[(kind, c)])
    assert seen == set(word)
