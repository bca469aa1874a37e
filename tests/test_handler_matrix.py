"""The handler matrix on the CPU (no GPU): the edge data has the properties
its GPU cells rely on, the trees of tests/handler_ref.py execute every handler
of the exact D = 5 core, the exact deep core and the typed core but an
explicit, reasoned list, the vectorised twins are the per-case reference bit
for bit, and the reference alone meets the conditions the GPU cells assume.

A handler is *hit* when a program's threaded code holds its word: for the
D = 5 and deep layouts (shared by the table, exact and fp32 cores) that code
comes from the library's own translator run with the identity table; for the
typed core, which the host translator does not serve, from the flattener's
words, which ``translate_words`` maps to handlers one to one.
"""
import random

import numpy as np
import pytest

import handler_ref as hr
import predict_ref as pr
from deap_amd import configs
from deap_amd.flatten import Flattener

# ------------------------------------------------------- what no tree reaches
# The flattener's rules (handler_ref's docstring) can never emit these:
UNREACHABLE = {
    # a PUSH is emitted only before the second operand of a binary node or a
    # branch of if_then_else, whose code always starts with a leaf load (LDV
    # or LDC); the encoder merges the two into PUSHV / PUSHC (flatten.py
    # _encode, lower_core.h's Emitter)
    "fast": {("PUSH", d): "PUSH then a leaf load is PUSHV / PUSHC" for d in range(5)},
    "deep": {("PUSH", d): "PUSH then a leaf load is PUSHV / PUSHC" for d in range(12)},
    "typed": dict(
        [(("PUSH", d), "PUSH then a leaf load is PUSHV / PUSHC") for d in range(5)] +
        # and_ / or_ take bools; a float argument is no bool, and the typed
        # core runs float-argument sets only
        [(("BIN", f, "V", v), "and_ / or_ of a float argument does not type-check")
         for f in ("and", "or") for v in range(hr.NV_TYPED)]),
}


def _same_ids(a, b):
    keys = ("H_LDC", "H_LDV0", "H_PUSH0", "H_PUSHC0", "H_PUSHV0", "H_BIN0", "H_FAM_STRIDE",
            "H_NEG", "H_ABS", "H_SQRT", "H_COUNT", "D", "NV", "WINDOW")
    return all(a[k] == b[k] for k in keys)


def test_the_cores_of_one_depth_share_their_handler_ids():
    """The translator's layouts are the exact cores' (fp32: static_asserts in
    gpeval.hip), so one hit set serves the table, exact and fp32 core."""
    assert _same_ids(hr.layout(""), hr.layout("_exact"))
    assert _same_ids(hr.layout("_deep"), hr.layout("_exact_deep"))
    assert len(hr.universe(hr.layout("_exact"))) == 8 * 38 + 32 + 10 + 160 + 4
    assert hr.layout("_typed")["NV"] == hr.NV_TYPED


# ------------------------------------------------------------------- data --
def test_edge_set_and_blocks():
    X, Xb = hr.data(), hr.benign()
    E = hr.E
    assert len(E) == 29 and X.shape == (32, hr.N) and hr.N == 29 * 29 + 513
    assert hr.N // 128 >= 9 and hr.N % 128 != 0
    assert len(set(E.view(np.uint64).tolist())) == 29
    assert np.isnan(E[-4:]).all() and E.view(np.uint64)[-1] == 0x7ff0000000000001
    # block A: case i |E| + j holds E[i] in the even and E[j] in the odd columns
    for i, j in ((0, 1), (3, 28), (28, 5), (17, 17)):
        c = i * 29 + j
        assert (X[0::2, c].view(np.uint64) == E.view(np.uint64)[i]).all()
        assert (X[1::2, c].view(np.uint64) == E.view(np.uint64)[j]).all()
    # both chains of a lane (cases 64 apart, K = 2) see other pairs
    assert (pr.bits(X[:2, :hr.N_A - 64]) != pr.bits(X[:2, 64:hr.N_A])).any(axis=0).all()
    # block B: no two columns agree in more than 5 % of its cases
    B = pr.bits(X[:, hr.N_A:])
    agree = max((B[a] == B[b]).mean() for a in range(32) for b in range(a))
    assert agree <= 0.05, agree
    with np.errstate(all="ignore"):
        q = np.abs(X[0, hr.N_A:] / X[1, hr.N_A:])
    assert ((q > 0) & (q < 2.0 ** -1022)).sum() >= 30
    assert Xb.shape == (32, 257) and Xb.min() >= 0.5 and Xb.max() <= 2.0


def test_python_raises_on_no_pair_and_rounds_in_the_subnormal_range():
    import operator
    vals = hr.E.tolist()
    sub = 0
    for fn in (operator.add, operator.sub, operator.mul, configs.protectedDiv):
        for a in vals:
            for b in vals:
                r = float(fn(a, b))                     # raises nothing
                sub += 0.0 < abs(r) < 2.0 ** -1022
    print("HM|subnormal results of the pair matrix: %d of %d" % (sub, 4 * len(vals) ** 2))
    assert sub >= 161                                   # (the 26-value subset's count)


# --------------------------------------------------------------- coverage --
def float_hits():
    """``{core: [(string, hit set)]}`` of the arithmetic and numpy trees."""
    def make():
        out = {"fast": [], "deep": [], "cpp": []}
        for pset, strings in ((hr.arith_pset(), hr.arith_small()[0] + hr.arith_big()),
                              (hr.numpy_pset(), hr.numpy_trees() + hr.numpy_big())):
            _, route, hits = hr.programs(pset, strings)
            for s, r, h in zip(strings, route, hits):
                out[hr.ROUTES[r]].append((s, h))
        return out
    return hr.cached("float_hits", make)


def typed_hit_sets():
    def make():
        pset = hr.typed_pset()
        batch = Flattener(pset).flatten(hr.parse(hr.typed_trees(), pset))
        assert not batch.err.any() and batch.depth.max() <= 5
        return hr.word_hits(batch)
    return hr.cached("typed_hits", make)


def _union(hits):
    u = set()
    for h in hits:
        u |= h
    return u


@pytest.mark.parametrize("core", ["fast", "deep", "typed"])
def test_every_handler_but_the_listed_ones_is_hit(core):
    lay = hr.layout({"fast": "_exact", "deep": "_exact_deep", "typed": "_typed"}[core])
    universe = hr.universe(lay)
    hit = _union(typed_hit_sets()) if core == "typed" else \
        _union(h for _, h in float_hits()[core])
    hit = {h for h in hit if h[0] != "TRIG"}
    assert hit <= universe, sorted(hit - universe)[:10]
    missing = universe - hit
    listed = set(UNREACHABLE[core])
    print("HM|%s: %d handlers, %d hit, %d listed" % (core, len(universe), len(hit),
                                                   len(listed)))
    assert missing == listed, ("not hit: %s; listed but hit: %s" % (
        sorted(hr.name(h) for h in missing - listed)[:40],
        sorted(hr.name(h) for h in listed - missing)[:40]))


def test_routing_of_the_float_trees():
    fh = float_hits()
    assert len(fh["cpp"]) == 1 and len(fh["deep"]) > 300 and len(fh["fast"]) > 500
    # the issue's examples of handlers no test was known to reach
    deep = _union(h for _, h in fh["deep"])
    assert {("BIN", "rdiv", "V", 29), ("PUSHV", 11, 31), ("BIN", "mul", "S", 11)} <= deep


def test_a_random_population_emits_none_of_the_listed_handlers():
    """20,000 seeded trees per primitive set (200 of the float ones random
    bushy trees of height 7 to 10, which need the deep core: genHalfAndHalf's
    own, half of whose nodes are unary, stay within four slots)."""
    for core, pset, lo, hi in (("float", hr.arith_pset(), 2, 6),
                               ("typed", hr.typed_pset(), 2, 4)):
        pop = configs.population(pset, "half", 19800 if core == "float" else 20000, 97, lo, hi)
        if core == "float":
            rnd = random.Random(98)
            pop += hr.parse([hr.random_bushy(rnd, 7 + i % 4) for i in range(200)], pset)
        batch = Flattener(pset).flatten(pop)
        if core == "typed":
            hit = _union(hr.word_hits(batch))
            assert not hit & set(UNREACHABLE["typed"])
            continue
        fast = _union(h for h in hr.translator_hits(batch, hr.NV, hr.layout("")) if h)
        deep = _union(h for h in hr.translator_hits(batch, hr.NV, hr.layout("_deep")) if h)
        assert not fast & set(UNREACHABLE["fast"]) and not deep & set(UNREACHABLE["deep"])
        assert ((batch.depth > 5) & (batch.depth <= 12)).sum() > 100


# ------------------------------------------------------------- references --
def small_reference():
    """``(F, exc)`` of every small arithmetic tree at every case of X, per
    case through gp.compile."""
    return hr.cached("small_ref", lambda: pr.values(
        hr.arith_pset(), hr.parse(hr.arith_small()[0], hr.arith_pset()), hr.data()))


def test_fp64_twin_is_the_per_case_reference_on_every_small_tree():
    strings, classes = hr.arith_small()
    F, exc = small_reference()
    T, first = hr.Twin(hr.arith_pset()).values(hr.parse(strings, hr.arith_pset()), hr.data())
    pr.assert_same_bits(T, F, "arith twin")
    assert first.tolist() == pr.first_errors(exc).tolist()
    # only math.sqrt raises, at the negative cases; -0.0 and nan do not
    for s, e in zip(strings, exc):
        assert not e or "sqrt(ARG" in s and "psqrt" not in s, s
        assert set(e.values()) <= {"ValueError"}
    i = strings.index("sqrt(ARG0)")
    neg = np.flatnonzero(hr.data()[0] < 0)
    assert sorted(exc[i]) == neg.tolist() and first[i] == neg[0]
    # the 40-variable evaluator's trees and the numpy-flavoured families
    ps40 = hr.arith_pset(40)
    t40 = hr.parse(hr.trees40(), ps40)
    F40, exc40 = pr.values(ps40, t40, hr.data40())
    assert not any(exc40)
    pr.assert_same_bits(hr.Twin(ps40).values(t40, hr.data40())[0], F40, "40 columns")
    psn = hr.numpy_pset()
    tn = hr.parse(hr.numpy_trees(), psn)
    with np.errstate(all="ignore"):
        Fn, excn = pr.values(psn, tn, hr.data())
    assert not any(excn)
    pr.assert_same_bits(hr.Twin(psn, numpy_sem=True).values(tn, hr.data())[0], Fn, "numpy")


def test_typed_twin_is_the_per_case_reference():
    pset = hr.typed_pset()
    trees = hr.parse(hr.typed_trees(), pset)
    Xt, labels = hr.typed_data()
    hit = hr.typed_hits(pset, trees, Xt, labels)
    assert np.array_equal(hr.typed_hits_twin(pset, trees, Xt, labels), hit)
    # every typed tree has a hit and a miss
    n = hit.sum(axis=1)
    assert (n > 0).all() and (n < hr.N).all(), np.flatnonzero((n == 0) | (n == hr.N))[:10]
    # the precision pins hit on all of block A but the nan cells
    strings = hr.typed_trees()
    for (fam, rev), r in hr.R_COLS.items():
        i = strings.index("eq(%s(ARG%d, ARG%d), ARG%d)" % (fam, rev, 1 - rev, r))
        val = np.array([bool(v) for v in (Xt[r] == Xt[r])])      # not nan
        assert np.array_equal(hit[i], val == (labels != 0))


def test_reference_conditions():
    strings, classes = hr.arith_small()
    F, exc = small_reference()
    tiny = (np.abs(F) > 0) & (np.abs(F) < 2.0 ** -1022)
    for i, c in enumerate(classes):
        if c.startswith("pair"):
            assert tiny[i].any() and np.isnan(F[i]).any(), strings[i]
    # the large slot trees on Xb: at most 5 % of the cells not finite, and the
    # moments route's range rule (|f| >= 2**500, inf, nan) skips under 10 %
    ps = hr.arith_pset()
    big = hr.parse(hr.arith_big(), ps)
    depth = Flattener(ps).flatten(big).depth.tolist()
    assert depth == [t + 1 for t in hr.BIG_TOPS] + [13], depth
    Fb, first = hr.Twin(ps).values(big, hr.benign())
    assert (first == -1).all()
    assert (~np.isfinite(Fb)).mean() <= 0.05
    small_b, first_b = hr.Twin(ps).values(hr.parse(strings, ps), hr.benign())
    allb = np.vstack([Fb, small_b])
    with np.errstate(invalid="ignore"):
        skipped = (~(np.abs(allb) < 2.0 ** 500)).any(axis=1) & (np.r_[first, first_b] < 0)
    print("HM|moments route: %d of %d programs under the range rule"
          % (skipped.sum(), len(skipped)))
    assert skipped.mean() < 0.10
    # the twin against the per-case reference on one large tree, a few cases
    Fp, _ = pr.values(ps, big[4:5], hr.benign()[:, :5])
    pr.assert_same_bits(Fb[4:5, :5], Fp, "large tree")
