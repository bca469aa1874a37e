"""The range pass (csrc/trig_ranges.h) that picks the exact cores' sin/cos
handlers: soundness against sampled evaluation, a floor on what it proves on
the headline population, and the translation it drives.  No GPU.

Soundness: a node the pass calls *small* (*mid*) must receive only finite
arguments with |x| < 0.85546875 (below the double whose high word is
0x400368fd) — glibc's own thresholds, which the specialised handlers assume —
for every case inside the column bounds the pass was given, the bounds'
corners and 0.0 (a partial tile's pad lanes) included.  The arguments are
evaluated from the same flattener words with Python floats (numpy's IEEE
add / sub / mul / div, ``math.sin`` / ``math.cos``).
"""
import math
import struct

import numpy as np
import pytest

import bytecode_ref as ref
from deap_amd import _lib, configs, gp
from deap_amd.flatten import Flattener, Op

GENERAL, MID, SMALL = 0, 1, 2
T_SMALL = 0.85546875                                  # hx < 0x3feb6000
T_MID = struct.unpack("<d", struct.pack("<Q", 0x400368fd << 32))[0]
NV = 10
N_CASES = 512

HAND = ["sin(sin(ARG0))", "cos(mul(ARG1, sin(ARG0)))", "sin(add(ARG0, ARG1))",
        "cos(protectedDiv(ARG0, ARG3))", "sin(protectedDiv(ARG0, cos(ARG1)))",
        "sin(protectedDiv(ARG0, sub(ARG1, ARG1)))",
        "cos(protectedDiv(ARG2, mul(ARG1, 0)))",
        "sin(protectedDiv(ARG0, 0))", "cos(neg(neg(neg(ARG4))))",
        "sin(neg(sub(neg(ARG0), neg(ARG1))))", "cos(sub(ARG5, neg(cos(ARG6))))",
        "sin(mul(cos(ARG0), cos(ARG1)))", "cos(add(sin(ARG7), sin(ARG8)))",
        "sin(mul(add(ARG0, ARG1), add(ARG2, ARG3)))",
        "cos(protectedDiv(1, add(cos(ARG0), 1)))", "sin(cos(sin(cos(ARG9))))"]

inf = math.inf
# name -> per-column (lo, hi) as gpe_set_cases stores them (hulled with 0.0)
BOUNDS = {
    "unit": [(-1.0, 1.0)] * NV,
    "third": [(-0.3, 0.3)] * NV,
    "offset": [(0.0, 2.4)] * NV,           # columns drawn from [0.9, 2.4]
    "wide": [(-50.0, 50.0)] * NV,
    "unbounded3": [(-1.0, 1.0)] * 3 + [(-inf, inf)] + [(-1.0, 1.0)] * (NV - 4),
}
DRAW = {"offset": (0.9, 2.4)}              # where the cases themselves lie


@pytest.fixture(scope="module")
def pset():
    return configs.pset_for("symreg10")


@pytest.fixture(scope="module")
def programs(pset):
    pop = configs.population(pset, "half", 2000, 77, 1, 8)
    pop += [gp.PrimitiveTree.from_string(s, pset) for s in HAND]
    batch = Flattener(pset).flatten(pop)
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    return pop, [code[off[i]:off[i + 1]] for i in range(len(pop))]


def cases(name, seed=5):
    """512 cases inside the bounds: the corners, 0.0 and uniform draws; the
    unbounded column also holds inf, -inf, nan and huge values."""
    rng = np.random.default_rng(seed)
    X = np.empty((NV, N_CASES))
    for v, (lo, hi) in enumerate(BOUNDS[name]):
        if math.isinf(lo):
            X[v] = rng.uniform(-1e3, 1e3, N_CASES)
            X[v, :8] = [inf, -inf, math.nan, 1e308, -1e308, 0.0, 1e-310, 2e8]
            continue
        dlo, dhi = DRAW.get(name, (lo, hi))
        X[v] = rng.uniform(dlo, dhi, N_CASES)
        X[v, 0], X[v, 1], X[v, 2] = lo, hi, 0.0
    # every combination of two columns' corners appears somewhere
    for c in range(3, 3 + 4 * NV):
        v = (c - 3) // 4
        lo, hi = BOUNDS[name][v]
        if not math.isinf(lo):
            X[:, c] = [b[(c + i) % 2] if not math.isinf(b[0]) else 1.0
                       for i, b in enumerate(BOUNDS[name])]
            X[v, c] = (lo, hi)[(c - 3) % 2]
    return X


def trig_arguments(words, X, unbounded):
    """Per sin/cos node in word order: (argument per case, dirty) — dirty: the
    value depends on an unbounded column or passed a protectedDiv whose
    sampled denominators straddle or touch 0."""
    n = X.shape[1]
    T, dT = np.zeros(n), False
    R, dR = {}, {}
    out = []
    pc = 0
    with np.errstate(all="ignore"):
        while True:
            w = int(words[pc])
            pc += 1
            op, d, x = w & 0xff, (w >> 8) & 0xff, w >> 16
            if op == Op.END:
                return out
            form = -1
            if Op.ADD <= op < Op.NEG or op >= Op.NPDIV:
                b0 = Op.NPDIV if op >= Op.NPDIV else Op.ADD
                form, base = (op - b0) % 3, b0 + 3 * ((op - b0) // 3)
            const = None
            if op in (Op.LDC, Op.PUSHC) or form == 2:
                const = ref._f64(words[pc], words[pc + 1])
                pc += 2
            if op in (Op.PUSH, Op.PUSHV, Op.PUSHC):
                R[d], dR[d] = T, dT
            if op in (Op.LDV, Op.PUSHV):
                T, dT = X[x].copy(), x in unbounded
            elif op in (Op.LDC, Op.PUSHC):
                T, dT = np.full(n, const), not math.isfinite(const)
            elif op == Op.NEG:
                T = -T
            elif op in (Op.SIN, Op.COS):
                out.append((T.copy(), dT))
                fn = math.sin if op == Op.SIN else math.cos
                T = np.array([fn(v) if math.isfinite(v) else math.nan
                              for v in T.tolist()])
            elif form >= 0:
                a, da = (R[d], dR[d]) if form == 0 else \
                    (X[x], x in unbounded) if form == 1 else \
                    (np.full(n, const), not math.isfinite(const))
                fam = ref._FAMS[base]
                if fam in ("div", "rdiv", "npdiv", "rnpdiv"):
                    den = T if fam in ("div", "npdiv") else a
                    fin = den[np.isfinite(den)]
                    if not (len(fin) and np.all(fin == 0.0)) and \
                            (len(fin) == 0 or (fin.min() <= 0.0 <= fin.max())):
                        dT = True
                T, dT = ref._fbin(fam, a, T), dT or da
            else:
                raise ValueError(op)


@pytest.mark.parametrize("name", list(BOUNDS))
def test_classes_hold_for_every_sampled_case(programs, name):
    pop, words = programs
    lo = np.array([b[0] for b in BOUNDS[name]])
    hi = np.array([b[1] for b in BOUNDS[name]])
    unbounded = {v for v, b in enumerate(BOUNDS[name]) if math.isinf(b[0])}
    X = cases(name)
    count = [0, 0, 0]
    for tree, w in zip(pop, words):
        cls = _lib.debug_trig_classes(w, lo, hi)
        args = trig_arguments(w, X, unbounded)
        assert len(cls) == len(args), str(tree)
        for c, (arg, dirty) in zip(cls, args):
            count[c] += 1
            if c == GENERAL:
                continue
            assert not dirty, (name, str(tree)[:200])
            assert np.all(np.isfinite(arg)), (name, str(tree)[:200])
            m = np.abs(arg).max()
            assert m < (T_SMALL if c == SMALL else T_MID), (name, str(tree)[:200], m)
    print("TRIGCLS|%s|general=%d mid=%d small=%d" % ((name,) + tuple(count)))
    assert sum(count) > 2000
    if name in ("unit", "third"):
        assert count[MID] + count[SMALL] > 0


def test_hand_written_classes(pset):
    """What the rules must prove, and what they must refuse."""
    def classes(expr, bounds):
        b = Flattener(pset).flatten([gp.PrimitiveTree.from_string(expr, pset)])
        lo, hi = zip(*bounds)
        return list(_lib.debug_trig_classes(b.code, np.array(lo), np.array(hi)))
    unit, wide, ub = BOUNDS["unit"], BOUNDS["wide"], BOUNDS["unbounded3"]
    # sin of [-1, 1] is within +-0.8417: the outer sin is small
    assert classes("sin(sin(ARG0))", unit) == [MID, SMALL]
    assert classes("sin(add(ARG0, ARG1))", unit) == [MID]
    assert classes("sin(add(ARG0, ARG1))", BOUNDS["third"]) == [SMALL]
    assert classes("sin(add(ARG0, ARG1))", wide) == [GENERAL]
    # a denominator that may be 0: inf or nan downstream
    assert classes("cos(protectedDiv(ARG0, ARG3))", unit) == [GENERAL]
    assert classes("sin(cos(protectedDiv(ARG0, ARG3)))", unit) == [GENERAL, GENERAL]
    # cos of [-1, 1] is within [0.5, 1]: the quotient is within [-2, 2]
    assert classes("sin(protectedDiv(ARG0, cos(ARG1)))", unit) == [MID, MID]
    assert classes("sin(protectedDiv(ARG0, cos(ARG1)))", wide) == [GENERAL, GENERAL]
    # protectedDiv by exactly 0 is 1.0
    assert classes("sin(protectedDiv(ARG0, sub(ARG1, ARG1)))", unit) == [GENERAL]
    assert classes("cos(mul(ARG0, protectedDiv(ARG0, mul(ARG1, 0))))", unit)[-1] \
        in (MID, SMALL)
    assert classes("cos(neg(neg(neg(ARG4))))", unit) == [MID]
    # an unbounded column taints everything computed from it, sin included
    assert classes("sin(ARG3)", ub) == [GENERAL]
    assert classes("cos(sin(ARG3))", ub) == [GENERAL, GENERAL]
    assert classes("cos(mul(ARG3, 0))", ub)[-1] == GENERAL
    assert classes("cos(add(ARG2, sin(ARG0)))", ub) == [MID, MID]
    assert classes("sin(mul(1e200, mul(ARG0, 1e200)))", unit) == [GENERAL]


def test_headline_population_is_mostly_specialised(pset):
    """The first 8,192 trees of the headline population (bench.py's default
    seed and depths) with its columns' bounds [-1, 1]: the pass proves a
    range for at least 70 % of the sin/cos nodes, the small one for 5 %."""
    pop = configs.population(pset, "half", 8192, 2024, 4, 8)
    batch = Flattener(pset).flatten(pop)
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    lo, hi = -np.ones(NV), np.ones(NV)
    count = np.zeros(3, dtype=np.int64)
    for i in range(len(pop)):
        cls = _lib.debug_trig_classes(code[off[i]:off[i + 1]], lo, hi)
        count += np.bincount(cls, minlength=3)
    total = int(count.sum())
    print("TRIGCLS|headline8192|general=%d mid=%d small=%d of %d"
          % (count[0], count[1], count[2], total))
    assert total > 30000
    assert (count[MID] + count[SMALL]) / total >= 0.70
    assert count[SMALL] / total >= 0.05


def test_translation_with_bounds_changes_only_sincos_words(pset):
    """gpe_debug_translate with and without bounds: the same word count, and
    only sin/cos words differ — each by its class's handler."""
    import asm_emu
    try:
        lay = asm_emu.read_layout("_exact")
    except OSError:
        pytest.skip("asm cores not generated")
    pop = configs.population(pset, "half", 400, 78, 1, 6)
    pop += [gp.PrimitiveTree.from_string(s, pset) for s in HAND]
    batch = Flattener(pset).flatten(pop)
    table = np.arange(lay["H_COUNT"], dtype=np.uint32) * 4 + 0x1000
    lo, hi = -np.ones(NV), np.ones(NV)
    plain, s0 = _lib.debug_translate(batch, NV, table)
    ranged, s1 = _lib.debug_translate(batch, NV, table, bounds=(lo, hi))
    assert len(plain) == len(ranged) and np.array_equal(s0, s1)
    word = {k: int(table[lay[k]]) for k in
            ("H_SIN", "H_COS", "H_SIN_MID", "H_COS_MID", "H_SIN_SMALL", "H_COS_SMALL")}
    by_class = {"H_SIN": {GENERAL: "H_SIN", MID: "H_SIN_MID", SMALL: "H_SIN_SMALL"},
                "H_COS": {GENERAL: "H_COS", MID: "H_COS_MID", SMALL: "H_COS_SMALL"}}
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    seen = set()
    for i in range(len(pop)):
        if s0[i] < 0:
            continue
        end = s0[i + 1:][s0[i + 1:] >= 0]
        a, b = int(s0[i]), int(end[0]) if len(end) else len(plain)
        cls = list(_lib.debug_trig_classes(code[off[i]:off[i + 1]], lo, hi))
        # (the table's words, 0x1000 + 4 id, are no half of any constant of
        # this primitive set: the sin/cos words are found by value)
        trig = [j for j in range(a, b) if plain[j] in (word["H_SIN"], word["H_COS"])]
        assert len(trig) == len(cls), str(pop[i])
        for j in np.nonzero(plain[a:b] != ranged[a:b])[0]:
            assert a + j in trig, str(pop[i])
        for j, c in zip(trig, cls):
            kind = "H_SIN" if plain[j] == word["H_SIN"] else "H_COS"
            assert ranged[j] == word[by_class[kind][c]], str(pop[i])
            seen.add(by_class[kind][c])
    assert seen == set(word)
