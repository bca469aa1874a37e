"""Confusion figures on the GPU: ``gpe_hit_group_counts`` on explicit planes
against its host twin and numpy at every row-length path, ``TypedConfusion``
and ``BooleanConfusion`` against tuples counted in Python from the reference's
hits, ``group_hits``, subsets, and that selection and the older specs did not
move.

The counting kernel has one path threshold: rows of up to 64 words (2,048
cases) get a power-of-two lane group each, longer rows a whole wave per four
rows.  The masks sit in registers on the short side and are read through the
caches on the long side, never in LDS, so the 70 KB of masks of the
(70, 70001) shape take the long path like any other: (130, 2048) and
(130, 2049) are the two sides of the only threshold."""
import math
import random

import numpy as np
import pytest

from deap_amd import _lib, configs, datasets, gp
from deap_amd.evaluator import (BooleanCaseHits, BooleanConfusion, GPUEvaluator, TypedBoolHits,
                                TypedCaseHits, TypedConfusion, pack_bitplanes,
                                unpack_bitplanes)

pytestmark = pytest.mark.gpu

N_MAX = 300
KNOBS = ("GPE_TYPED_WAVES", "GPE_TYPED_PMAX", "GPE_TYPED_TARGET_BLOCKS", "GPE_MIN_GROUP_TILES",
         "GPE_TYPED_ASM", "GPE_ASM", "GPE_TARGET_BLOCKS", "GPE_F_WAVES")
NAMES = ("tp", "fp", "fn", "tn", "hits", "accuracy", "recall", "specificity", "precision",
         "balanced_accuracy", "f1", "mcc")
_CACHE = {}


def _full(depth, leaf):
    """A full binary tree of add / mul over distinct columns: *depth* + 1
    values live at once, more than the typed core's five stack slots."""
    if depth == 0:
        return "IN%d" % (next(leaf) % 57)
    return "%s(%s, %s)" % ("add" if depth % 2 else "mul", _full(depth - 1, leaf),
                           _full(depth - 1, leaf))


def inputs():
    """(pset, trees, X, labels, hit): about 600 generated classifiers (more
    than one 64-program wave, more than one 512-program block) and hand-built
    trees for every route; hit[i, c] is the reference, computed once."""
    if "data" in _CACHE:
        return _CACHE["data"]
    ps = configs.pset_for("spambase")
    X, lab = datasets.spambase_like(N_MAX, 57)
    trees = configs.population(ps, "half", 600, 57, 2, 4)
    one = "protectedDiv(IN0, sub(IN1, IN1))"               # the int 1 (a zero divisor)
    big = "add(%s, %s)" % (one, one)
    for _ in range(6):
        big = "mul(%s, %s)" % (big, big)                   # the int 2 ** 64: the exact pass
    hand = ["True", "False", "lt(1.0, 2.0)", "not_(eq(3.0, 3.0))",         # constants
            "lt(IN0, IN1)", "and_(lt(IN3, IN4), not_(eq(IN5, IN6)))",
            "lt(%s, %s)" % (_full(7, iter(range(10 ** 6))), _full(6, iter(range(7, 10 ** 6)))),
            "lt(if_then_else(lt(IN1, IN2), %s, IN3), 1.5)" % _full(7, iter(range(3, 10 ** 6))),
            "lt(%s, IN0)" % big]
    trees = trees + [gp.PrimitiveTree.from_string(s, ps) for s in hand]
    rows = list(zip(*X.tolist()))
    labels = [bool(v) for v in lab.tolist()]
    hit = np.zeros((len(trees), N_MAX), dtype=bool)
    for i, tree in enumerate(trees):
        func = gp.compile(tree, ps)
        hit[i] = [bool(func(*r)) is b for r, b in zip(rows, labels)]
    _CACHE["data"] = (ps, trees, X, lab, hit)
    return _CACHE["data"]


TRUE_TREE, FALSE_TREE = 600, 601                           # positions of the hand trees


def make(monkeypatch, spec):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return GPUEvaluator(inputs()[0], spec, device=0)


def check_routes(ev, got):
    """Every route held a program and nobody was skipped."""
    geo = ev.ctx.geometry()
    assert geo["asm_typed"] >= 1 and geo["typed_const"] >= 1, geo
    assert geo["fast"] + geo["deep"] >= 1, geo             # the C++ kernels
    assert ev.stats.get("exact_programs", 0) >= 1          # the exact-integer pass
    assert len(got) == ev.ctx.n_prog
    assert geo["asm_typed"] + geo["typed_const"] + geo["fast"] + geo["deep"] == len(got), geo
    assert all(type(r) is tuple for r in got), [r for r in got if type(r) is not tuple][:1]
    return geo


def figures_ref(tp, fp, fn, tn):
    """The definitions on Python ints."""
    P, N = tp + fn, fp + tn
    recall = tp / P if P else 0.0
    specificity = tn / N if N else 0.0
    if P == 0:
        balanced = specificity
    elif N == 0:
        balanced = recall
    else:
        balanced = (recall + specificity) / 2
    a, b = (tp + fp) * (tp + fn), (tn + fp) * (tn + fn)
    mcc = 0.0 if a == 0 or b == 0 else \
        float(tp * tn - fp * fn) / (math.sqrt(float(a)) * math.sqrt(float(b)))
    den = 2 * tp + fp + fn
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "hits": tp + tn,
            "accuracy": (tp + tn) / (P + N), "recall": recall, "specificity": specificity,
            "precision": tp / (tp + fp) if tp + fp else 0.0, "balanced_accuracy": balanced,
            "f1": (2 * tp) / den if den else 0.0, "mcc": mcc}


def cells_ref(hit, positive):
    """[(tp, fp, fn, tn)] per row of a reference hit matrix, counted in Python."""
    positive = [bool(p) for p in positive]
    n_pos = sum(positive)
    n_neg = len(positive) - n_pos
    out = []
    for row in hit.tolist():
        tp = sum(1 for h, p in zip(row, positive) if h and p)
        tn = sum(1 for h, p in zip(row, positive) if h and not p)
        out.append((tp, n_neg - tn, n_pos - tp, tn))
    return out


def tuples_ref(cells, names=NAMES):
    return [tuple(figures_ref(*c)[k] for k in names) for c in cells]


# ------------------------------------------------------------- confusion --
@pytest.mark.parametrize("n_cases", [1, 2, 33, 64, 65, 129, 300])
def test_the_confusion_is_the_references(monkeypatch, n_cases):
    ps, trees, X, lab, hit = inputs()
    cells = cells_ref(hit[:, :n_cases], lab[:n_cases])
    plain = make(monkeypatch, TypedBoolHits(X[:, :n_cases], lab[:n_cases]))
    try:
        counts = [h for (h,) in plain.evaluate(trees)]
    finally:
        plain.close()
    ev = make(monkeypatch, TypedConfusion(X[:, :n_cases], lab[:n_cases], fitness=NAMES))
    try:
        got = ev.evaluate(trees)
        check_routes(ev, got)
        assert got == tuples_ref(cells)
        assert all(type(v) is (int if k < 5 else float) for k, v in enumerate(got[0]))
        assert ev.last_confusion.dtype == np.int64
        assert ev.last_confusion.tolist() == [list(c) for c in cells]
        assert ev.last_hits.tolist() == counts == hit[:, :n_cases].sum(axis=1).tolist()
        assert np.array_equal(ev.last_case_hits(), hit[:, :n_cases])
        tp, fp, fn, tn = ev.last_confusion[TRUE_TREE].tolist()
        assert tn + fn == 0 and tp + fp == n_cases           # "True" predicts the positive class
        tp, fp, fn, tn = ev.last_confusion[FALSE_TREE].tolist()
        assert tp + fp == 0 and tn + fn == n_cases
        if n_cases == 1:                                      # the one-class prefix
            assert not lab[:1].any() and (ev.last_confusion[:, [0, 2]] == 0).all()
    finally:
        ev.close()


# ------------------------------------------------------------ the kernel --
@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def random_words(rng, n, units):
    return rng.integers(0, 1 << 32, size=(n, units), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n, n_cases, groups", [
    (1, 1, (1, 3, 8)),
    (65, 32, (1, 3, 8)), (1000, 33, (1, 3, 8)), (1000, 64, (1, 3, 8)),    # short rows, ragged wave
    (130, 2048, (1, 3, 8)), (130, 2049, (1, 3, 8)),           # 64 / 65 words: the path threshold
    (130, 4601, (1, 3, 8)),                                   # 144 words: 2 1/4 strides
    (70, 70001, (8,))])                                       # 70 KB of masks
def test_the_kernel_counts_what_the_host_twin_counts(ctx, n, n_cases, groups):
    rng = np.random.default_rng(n * 100003 + n_cases)
    units = (n_cases + 31) // 32
    planes = random_words(rng, n, units)                      # (pad bits set)
    for G in groups:
        masks = random_words(rng, G, units)                   # (pad bits set)
        if G > 1:
            masks[1] = 0
            masks[G - 1] = 0xFFFFFFFF
        exp = _lib.host_hit_group_counts(planes, n_cases, masks)
        got = ctx.hit_group_counts(planes, n, n_cases, masks)
        assert got.dtype == np.int64 and got.shape == (n, G)
        assert np.array_equal(got, exp), np.argwhere(got != exp)[:5]
        if n * n_cases <= 1000 * 4601:
            rows, sel = unpack_bitplanes(planes, n_cases), unpack_bitplanes(masks, n_cases)
            assert np.array_equal(got, np.stack([(rows & s).sum(1) for s in sel], axis=1))
        if G > 1:
            assert not got[:, 1].any()
            clean = planes.copy()
            if n_cases % 32:
                clean[:, -1] &= np.uint32((1 << (n_cases % 32)) - 1)
            pop = np.unpackbits(clean.view(np.uint8), axis=1).sum(1)
            assert np.array_equal(got[:, G - 1], pop)


def test_the_library_refuses_and_accepts_what_the_header_says(ctx):
    planes, masks = np.zeros((3, 2), dtype=np.uint32), np.zeros((1, 2), dtype=np.uint32)
    P = _lib._ptr
    out = np.zeros((3, 1), dtype=np.int32)
    call = ctx.lib.gpe_hit_group_counts
    for G, text in ((0, "G = 0 groups"), (9, "G = 9 groups")):
        with pytest.raises(_lib.GpeError, match=text):
            ctx.hit_group_counts(planes, 3, 40, np.zeros((G, 2), dtype=np.uint32))
    for args in ((P(planes), -1, 40, P(masks), 1, P(out)),
                 (P(planes), 3, 0, P(masks), 1, P(out)),
                 (P(planes), 3, 40, None, 1, P(out)),
                 (P(planes), 3, 40, P(masks), 1, None)):
        assert call(ctx.h, *args) == _lib.GPE_E_ARG, args[1:5]
        assert b"hit_group_counts" in ctx.lib.gpe_last_error(ctx.h)
    assert call(ctx.h, P(planes), 0, 40, P(masks), 1, None) == 0           # n == 0
    assert ctx.hit_group_counts(np.zeros((0, 2), dtype=np.uint32), 0, 40, masks).shape == (0, 1)
    fresh = _lib.Context(0)
    try:
        assert call(fresh.h, None, 0, 0, P(masks), 1, P(out)) == -3        # GPE_E_STATE
        assert b"no hit planes of the loaded programs" in fresh.lib.gpe_last_error(fresh.h)
    finally:
        fresh.close()


# ---------------------------------------------------------------- subset --
def test_a_subset_counts_with_its_own_labels(monkeypatch):
    ps, trees, X, lab, hit = inputs()
    rng = np.random.default_rng(40)
    idx = rng.integers(0, N_MAX, size=40)
    idx[7] = idx[3]                                           # a duplicate for certain
    assert len(set(idx.tolist())) < 40 and (np.diff(idx) < 0).any()
    folds = [list(range(0, 13)), list(range(13, 40))]
    ev = make(monkeypatch, TypedConfusion(X, lab, fitness=NAMES))
    try:
        ev.subsample(idx)
        got = ev.evaluate(trees)
        conf = ev.last_confusion.copy()
        in_folds = ev.group_hits(folds)
        assert ev.case_uploads == 1 and ev.n_cases == 40
    finally:
        ev.close()
    fresh = make(monkeypatch, TypedConfusion(X[:, idx], lab[idx], fitness=NAMES))
    try:
        assert fresh.evaluate(trees) == got
        assert np.array_equal(fresh.last_confusion, conf)
        assert np.array_equal(fresh.group_hits(folds), in_folds)
    finally:
        fresh.close()
    cells = cells_ref(hit[:, idx], lab[idx])
    assert got == tuples_ref(cells) and conf.tolist() == [list(c) for c in cells]
    sub = hit[:, idx]
    assert np.array_equal(in_folds, np.stack([sub[:, f].sum(1) for f in folds], axis=1))


# ------------------------------------------------------------ group_hits --
def test_group_hits_counts_folds_on_the_resident_matrix(monkeypatch):
    ps, trees, X, lab, hit = inputs()
    rng = np.random.default_rng(4)
    perm = rng.permutation(N_MAX)
    folds = [perm[:100].tolist(), perm[100:200].tolist(), perm[200:].tolist()]
    ev = make(monkeypatch, TypedCaseHits(X, lab, "device"))
    try:
        ev.evaluate(trees)
        got = ev.group_hits(folds)
        assert got.dtype == np.int64 and got.shape == (len(trees), 3)
        assert np.array_equal(got.sum(1), ev.last_hits)
        for g, fold in enumerate(folds):
            assert np.array_equal(got[:, g], hit[:, fold].sum(1))
        masks = np.zeros((3, N_MAX), dtype=bool)
        for g, fold in enumerate(folds):
            masks[g, fold] = True
        assert np.array_equal(ev.group_hits(masks), got)
        many = rng.random((11, N_MAX)) < 0.4                   # two slices: 8 and 3
        assert np.array_equal(ev.group_hits(many), (hit[:, None, :] & many[None]).sum(-1))
        assert np.array_equal(ev.group_hits([[5, 5, 299]]),
                              (hit[:, 5] * 1 + hit[:, 299])[:, None])
        with pytest.raises(IndexError, match=r"groups\[0\]\[1\] = 300 is outside \[0, 300\)"):
            ev.group_hits([[0, 300]])
        # nothing resident moved
        assert np.array_equal(ev.last_case_hits(), hit)
        assert len(ev.select_lexicase(trees, 3)) == 3
        ev.subsample(np.arange(0, N_MAX, 2))
        with pytest.raises(ValueError, match="group_hits: .* left no hit planes on the GPU"):
            ev.group_hits(folds)
        ev.evaluate(trees)
        assert np.array_equal(ev.group_hits([list(range(150))])[:, 0], hit[:, 0:N_MAX:2].sum(1))
        few = trees[:10]
        ev.prepare(ev.flatten(few), few)                       # another batch, loaded not run
        with pytest.raises(ValueError, match="group_hits: the context now holds 10 programs"):
            ev.group_hits([[0]])
        with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs"):
            ev.ctx.hit_group_counts(None, 0, 0, np.zeros((1, 5), dtype=np.uint32))
    finally:
        ev.close()


# --------------------------------------------------------------- boolean --
def _boolean_problem(name):
    """(pset, rows[case][var], outputs[case]): the reference's tables — 64
    cases are 2 words a row, 2,048 are 64."""
    ins, outs = datasets.parity6_table() if name == "parity6" else datasets.mux11_table()
    return configs.pset_for(name), ins.T.tolist(), outs.tolist()


@pytest.mark.parametrize("name", ["parity6", "mux11"])
def test_the_boolean_machine_counts_the_same_way(monkeypatch, name):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    ps, rows, outs = _boolean_problem(name)
    trees = configs.population(ps, "half", 300, 11, 2, 5)
    host = GPUEvaluator(ps, BooleanCaseHits.from_rows(rows, outs, "host"), device=0)
    try:
        per_case = np.array(host.evaluate(trees), dtype=bool)
    finally:
        host.close()
    cells = cells_ref(per_case, outs)
    ev = GPUEvaluator(ps, BooleanConfusion.from_rows(rows, outs, fitness=NAMES), device=0)
    try:
        got = ev.evaluate(trees)
        assert got == tuples_ref(cells)
        assert ev.last_confusion.tolist() == [list(c) for c in cells]
        assert ev.last_hits.tolist() == per_case.sum(1).tolist()
        assert np.array_equal(ev.last_case_hits(), per_case)
        half = len(rows) // 2
        assert np.array_equal(ev.group_hits([list(range(half)), list(range(half, len(rows)))]),
                              np.stack([per_case[:, :half].sum(1), per_case[:, half:].sum(1)], 1))
    finally:
        ev.close()


# ------------------------------------------------------------- selection --
def test_selection_on_the_confusion_spec_is_typed_case_hits_selection(monkeypatch):
    ps, trees, X, lab, hit = inputs()
    n_cases = 200
    index = {id(t): i for i, t in enumerate(trees)}
    picks, states, par = [], [], []
    for spec in (TypedCaseHits(X[:, :n_cases], lab[:n_cases], "device"),
                 TypedConfusion(X[:, :n_cases], lab[:n_cases])):
        ev = make(monkeypatch, spec)
        try:
            ev.evaluate(trees)
            random.seed(77)
            picks.append([index[id(t)] for t in ev.select_lexicase(trees, 50)])
            states.append(random.getstate())
            random.seed(78)
            par.append([index[id(t)] for t in ev.select_lexicase(trees, 50, parallel=True)])
        finally:
            ev.close()
    assert picks[0] == picks[1] and states[0] == states[1] and par[0] == par[1]
    assert len(picks[0]) == 50


# -------------------------------------------------------- unchanged path --
def test_the_older_specs_give_what_they_gave(monkeypatch):
    ps, trees, X, lab, hit = inputs()

    def older():
        out = []
        for spec in (TypedBoolHits(X, lab), TypedCaseHits(X, lab, "device"),
                     TypedCaseHits(X[:, :129], lab[:129], "host")):
            ev = make(monkeypatch, spec)
            try:
                out.append(ev.evaluate(trees))
                if isinstance(spec, TypedCaseHits):
                    out.append(ev.ctx.hit_planes(len(trees)).tolist())
            finally:
                ev.close()
        return out

    before = older()
    ev = make(monkeypatch, TypedConfusion(X, lab, fitness=("mcc", "tp")))
    try:
        got = ev.evaluate(trees)
        assert got == tuples_ref(cells_ref(hit, lab), ("mcc", "tp"))
    finally:
        ev.close()
    assert older() == before
    assert before[0] == before[1] == [(int(h),) for h in hit.sum(axis=1)]
