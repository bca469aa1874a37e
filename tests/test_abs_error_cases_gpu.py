"""``SymbRegCaseAbsErrors`` on the GPU: the per-case absolute errors of a cases
run (``gpe_run_abserr_cases``) against ``gp.compile``, bit for bit, on every
tree of ``abs_error_ref``'s population (2,022) at the edges of the 128-case
tile, and at 10,240 / 10,243 cases against ``gp.compile`` on a sample and
``predict`` on all; the summaries against a plain abs-error run's; the rows
route in chunks; two term columns; what stays resident; epsilon-lexicase from
the resident matrix against the host loop and the drop-ins; the resident-only
mode; the C ABI."""
import ctypes
import math
import random

import numpy as np
import pytest

import abs_error_ref as ar
import predict_ref as pr
import scaled_ref as sr
from deap_amd import _lib, base, configs, creator, datasets, gp, tools

pytestmark = pytest.mark.gpu
EXC = {1: ValueError, 2: OverflowError}
ALL3 = ("mae", "max", "hits")
SHAPES = ("abserr", "abserr_deep", "asm_fast", "asm_deep", "cpp_fast", "cpp_deep")
N_SMALL = 257
BIG_TREE = 5000          # nodes: past this a tree is not compiled on 10,243 rows
_CACHE = {}


def cells():
    """``(pset, trees, X, y)``, once."""
    if "cells" not in _CACHE:
        ps, trees, n_base = ar.population()
        X, y = sr.data()
        _CACHE["cells"] = (ps, trees, X, y)
        _CACHE["n_base"] = n_base
    return _CACHE["cells"]


def reference(idx, n):
    """``gp.compile``'s rows of the trees *idx* on the first n cases, computed
    once per (tree, n <= N_SMALL or n) and shared: ``{i: (e, first, kind)}``
    with ``e = abs(f - y)`` in Python floats up to the first erroring case
    (nan from there on)."""
    ps, trees, X, y = cells()
    top = N_SMALL if n <= N_SMALL else sr.N_MAX
    store = _CACHE.setdefault(("ref", top), {})
    rows = None
    for i in idx:
        if i not in store:
            if rows is None:
                rows = list(zip(*X[:, :top].tolist()))
            f, first, kind = sr.outputs(ps, trees[i], rows)
            e = np.array([abs(a - b) for a, b in zip(f.tolist(), y[:top].tolist())])
            store[i] = (e, first, kind)
    out = {}
    for i in idx:
        e, first, kind = store[i]
        err = first is not None and first < n
        out[i] = (e[:n], first if err else None, kind if err else None)
    return out


def evaluator(n, cases="host", fitness=ALL3, terms=None, spec_cls=None, **kw):
    from deap_amd.evaluator import GPUEvaluator, SymbRegCaseAbsErrors
    ps, trees, X, y = cells()
    Xn = np.ascontiguousarray(X[:, :n])
    T = np.ascontiguousarray(y[:n]) if terms is None else terms
    spec = spec_cls(Xn, T) if spec_cls else \
        SymbRegCaseAbsErrors(Xn, T, hit_eps=ar.HIT_EPS, cases=cases, fitness=fitness)
    return GPUEvaluator(ps, spec, device=0, **kw)


def run(n, pop=None, **kw):
    """One evaluation of the population on the first n cases, then on the same
    resident programs a cases run and a plain abs-error run by the context."""
    ps, trees, X, y = cells()
    ev = evaluator(n, **kw)
    try:
        res = ev.evaluate(trees if pop is None else pop)
        last = (ev.last_mae.copy(), ev.last_max_error.copy(), ev.last_hits.copy())
        cases, w4, err, flags = ev.ctx.run_abserr_cases(ar.HIT_EPS, n)
        shapes = {k: ev.ctx.launch_shape(k) for k in SHAPES}
        plain = ev.ctx.run_abserr(ar.HIT_EPS)
        plain_shapes = {k: ev.ctx.launch_shape(k) for k in SHAPES}
    finally:
        ev.close()
    return dict(res=res, last=last, cases=cases, w4=w4, err=err, flags=flags, shapes=shapes,
                plain=plain, plain_shapes=plain_shapes)


def _same(x1, x2, what=""):
    x1, x2 = np.asarray(x1), np.asarray(x2)
    if x1.dtype.kind == "f":
        pr.assert_same_bits(x1, x2, what)
    else:
        assert x1.dtype == x2.dtype and np.array_equal(x1, x2), what


def _rows_programs(shapes):
    return sum(shapes[k]["programs"] for k in ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep"))


def _first(err):
    first = (err >> np.uint64(2)).astype(np.int64)
    first[err == np.uint64(_lib.GPE_NO_ERROR)] = -1
    return first


def _check_rows(r, ref, n, what):
    """The matrix and the results of run *r* against the rows *ref*: a tree
    whose reference raises gives that exception at that case (its row equal up
    to there and nan at it); every other row is equal on every case."""
    ps, trees, X, y = cells()
    first = _first(r["err"])
    raised = values = 0
    for i, (e, f0, kind) in ref.items():
        w = (what, i, str(trees[i])[:80])
        got = r["cases"][i]
        if f0 is not None:
            assert isinstance(r["res"][i], EXC[sr.STATUS[kind]]), (w, r["res"][i])
            assert first[i] == f0, (w, first[i], f0)
            pr.assert_same_bits(got[:f0], e[:f0], repr(w))
            assert math.isnan(got[f0]), (w, got[f0])
            raised += 1
            continue
        assert first[i] == -1, (w, first[i])
        pr.assert_same_bits(got, e, repr(w))
        res = r["res"][i]
        if isinstance(res, BaseException):          # fsum's, as SymbRegAbsError's
            assert isinstance(res, OverflowError) and \
                str(res) == "intermediate overflow in fsum", (w, res)
            assert np.isfinite(e).all() and r["w4"][i, 0] == math.inf
        else:
            assert type(res) is tuple and len(res) == n and type(res[0]) is float
            pr.assert_same_bits(np.array(res), e, repr(w))
            values += 1
    return raised, values


# ------------------------------------------- 1. every program, every case --
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257])
def test_every_program_against_the_reference(n):
    """All 2,022 trees, all n cases: one lane, a partial wave, an exact last
    tile, ragged ones.  The reference is computed here (gp.compile on 257
    rows, once for the six counts)."""
    ps, trees, X, y = cells()
    ref = reference(range(len(trees)), n)
    assert len(ref) == len(trees) == 2022
    r = _CACHE[("run", n)] = run(n)
    assert r["cases"].shape == (len(trees), n)
    raised, values = _check_rows(r, ref, n, "n = %d" % n)
    assert raised + values >= len(trees) - 2 and values > 1900, (raised, values)
    if n >= 4:
        assert raised >= 3                          # sin(inf), sqrt(ARG6 < 0), float(int)
    a, ad = r["shapes"]["abserr"], r["shapes"]["abserr_deep"]
    assert a["programs"] > 1000 and ad["programs"] > 0 and _rows_programs(r["shapes"]) > 0
    assert a["n_tiles"] == (n + 127) // 128
    # the evaluator's three figures are the plain run's
    assert np.array_equal(r["last"][2] >= 0, [not isinstance(x, BaseException) for x in r["res"]])


# ------------------------------ 2. the two-buffer and leaf-column plans --
def big_sample():
    """The CPU suite's sample and every 16th tree, without the trees too
    large to compile on 10,243 rows in a test (those are held to predict
    below, like every tree)."""
    ps, trees, X, y = cells()
    nb = _CACHE["n_base"]
    idx = set(range(nb, len(trees))) | set(range(len(sr.HAND))) | \
        set(range(len(sr.HAND), nb, 64)) | set(range(0, len(trees), 16))
    return sorted(i for i in idx if len(trees[i]) < BIG_TREE)


@pytest.mark.parametrize("n", [10240, 10243])
def test_the_two_buffer_and_the_leaf_column_plans(n):
    """10,240 cases without the leaf columns: three programs per wave and two
    tile buffers (LDS-DMA).  10,243 with them: 31 columns, one buffer, and the
    last case's inf column, which makes rows inf / nan and sends programs to
    the rows route by a redo.  The sample against gp.compile; every tree
    against ``abs(predict - y)``, nan where predict documents nan."""
    ps, trees, X, y = cells()
    kw = dict(trig_leaves=False) if n == 10240 else {}
    idx = big_sample()
    assert len(idx) >= 120
    ref = reference(idx, n)
    ev = evaluator(n, **kw)
    try:
        res = ev.evaluate(trees)
        cases, w4, err, flags = ev.ctx.run_abserr_cases(ar.HIT_EPS, n)
        shapes = {k: ev.ctx.launch_shape(k) for k in SHAPES}
        plain = ev.ctx.run_abserr(ar.HIT_EPS)
        vals = ev.predict(trees, errors="nan")
        pfirst = ev.last_predict_first_error.copy()
    finally:
        ev.close()
    r = dict(res=res, cases=cases, w4=w4, err=err, flags=flags)
    raised, values = _check_rows(r, ref, n, "n = %d" % n)
    assert values >= (100 if n == 10240 else 60) and raised >= 3, (values, raised)
    a, ad = shapes["abserr"], shapes["abserr_deep"]
    assert a["programs"] > 1000 and ad["programs"] > 0 and _rows_programs(shapes) > 0, shapes
    if n == 10240:
        assert a["P"] == 3 and a["dbuf"] == 1 and a["lds_bytes"] == 77696, a
    else:
        assert a["P"] == 2 and a["dbuf"] == 0, a
        assert shapes["asm_fast"]["programs"] + shapes["asm_deep"]["programs"] > 50, shapes
        assert np.isinf(cases).any(axis=1).sum() > 20 and np.isnan(cases).any(axis=1).sum() > 20
    with np.errstate(invalid="ignore"):
        exp = np.abs(vals - y[:n][None, :])
    pr.assert_same_bits(cases, exp, "n = %d against predict" % n)
    assert np.array_equal(_first(err), pfirst)
    # (3.) the summaries of the cases run are the plain run's, bit for bit
    for x1, x2 in zip((w4, err, flags), plain):
        _same(x1, x2, "summaries at n = %d" % n)


# ------------------------------------------------ 3. summaries unchanged --
def test_summaries_are_those_of_a_plain_run():
    """The four words, first errors and flags of a cases run (with the host
    copy and resident-only) and of ``gpe_run_abserr`` on the same resident
    programs, and the launch shapes of both, at 257 cases (10,243: the test
    above)."""
    n = 257
    r = _CACHE.get(("run", n)) or run(n)
    for x1, x2 in zip((r["w4"], r["err"], r["flags"]), r["plain"]):
        _same(x1, x2)
    assert r["shapes"]["abserr"] == r["plain_shapes"]["abserr"]
    assert r["shapes"]["abserr_deep"] == r["plain_shapes"]["abserr_deep"]
    ps, trees, X, y = cells()
    ev = evaluator(n, cases="device")
    try:
        ev.evaluate(trees)
        none, w4, err, flags = ev.ctx.run_abserr_cases(ar.HIT_EPS, n, want_cases=False)
        assert none is None
        for x1, x2 in zip((w4, err, flags), r["plain"]):
            _same(x1, x2)
        for x1, x2 in zip((ev.last_mae, ev.last_max_error, ev.last_hits), r["last"]):
            _same(x1, x2)
    finally:
        ev.close()


# ------------------------------------------------------------ 4. chunking --
def test_chunks_of_the_rows_route_write_their_own_rows(monkeypatch):
    """With the asm cores off (GPE_ASM=0) every program takes the rows route;
    a scratch budget of 1 MiB holds 510 rows of 257 cases, so the 2,022
    programs take 4 chunks.  The matrix has the bits of the one-chunk run and
    of the default run: a row written relative to its chunk would not."""
    ps, trees, X, y = cells()
    n = 257
    per = (1 << 20) // (n * 8)
    assert -(-len(trees) // per) >= 3
    default = _CACHE.get(("run", n)) or run(n)
    monkeypatch.setenv("GPE_ASM", "0")              # (read when the context is made)
    monkeypatch.delenv("GPE_MOMENTS_MB", raising=False)
    whole = run(n)
    monkeypatch.setenv("GPE_MOMENTS_MB", "1")
    chunked = run(n)
    assert whole["shapes"]["abserr"]["programs"] == 0 == chunked["shapes"]["abserr"]["programs"]
    assert _rows_programs(whole["shapes"]) == len(trees)
    assert 0 < _rows_programs(chunked["shapes"]) <= per      # (the last chunk's launches)
    for other in (whole, default):
        pr.assert_same_bits(chunked["cases"], other["cases"])
        for k in ("err", "flags"):
            _same(chunked[k], other[k])
        for a, b in zip(chunked["res"], other["res"]):
            assert type(a) is type(b)
    _same(chunked["w4"], whole["w4"])


# ---------------------------------------------------- 5. two term columns --
def test_two_term_columns():
    """``e = abs(f - t0 - t1)``, left to right, on every route (the tile then
    has 32 columns), f from predict (pinned to gp.compile by its own suite)."""
    ps, trees, X, y = cells()
    n = 257
    pick = list(range(0, len(trees), 7)) + [10, 11]
    pop = [trees[i] for i in pick]
    T = np.stack([y[:n] * 0.75, X[3, :n] * 0.001])
    ev = evaluator(n, terms=T)
    try:
        res = ev.evaluate(pop)
        cases, w4, err, flags = ev.ctx.run_abserr_cases(ar.HIT_EPS, n)
        shapes = {k: ev.ctx.launch_shape(k) for k in SHAPES}
        plain = ev.ctx.run_abserr(ar.HIT_EPS)
        vals = ev.predict(pop, errors="nan")
    finally:
        ev.close()
    assert shapes["abserr"]["programs"] > 200 and shapes["abserr_deep"]["programs"] > 0
    assert _rows_programs(shapes) > 0
    with np.errstate(invalid="ignore"):
        exp = np.abs(vals - T[0][None, :] - T[1][None, :])
    pr.assert_same_bits(cases, exp)
    first = _first(err)
    checked = 0
    for k, r in enumerate(res):
        if first[k] >= 0:
            assert isinstance(r, (ValueError, OverflowError))
            continue
        e = [abs(f - a - b) for f, a, b in zip(vals[k].tolist(), T[0].tolist(), T[1].tolist())]
        pr.assert_same_bits(cases[k], np.array(e), "row %d" % k)
        if not isinstance(r, BaseException):
            pr.assert_same_bits(np.array(r), np.array(e))
            checked += 1
    assert checked > 250
    for x1, x2 in zip((w4, err, flags), plain):
        _same(x1, x2)


# ----------------------------------------------------------- 6. residency --
def test_what_stays_resident():
    """The matrix of a cases run outlives a plain abs-error run, a moments run
    and a predict; a SymbRegCaseErrors evaluator's matrix is its own; the
    resident fitness of gpe_tournament(NULL) is not touched by a cases run."""
    from deap_amd.evaluator import SymbRegCaseErrors
    ps, trees, X, y = cells()
    n, k = 257, 60
    ref = reference(range(len(trees)), n)
    with np.errstate(over="ignore"):
        pick = [i for i in range(len(trees))
                if ref[i][1] is None and np.isfinite(ref[i][0] ** 2).all()][:600]
    pop = [trees[i] for i in pick]
    mx = np.zeros(n, dtype=np.uint8)

    def select(ctx, values, mode=2):
        rng = random.Random(5)
        idx, failed = ctx.lexicase(values, mx, k, rng, mode)
        assert failed == -1
        return idx.tolist(), rng.getstate()

    ev = evaluator(n)
    sq = evaluator(n, spec_cls=SymbRegCaseErrors)
    try:
        batch = ev.flatten(pop)
        ev.prepare(batch, pop)
        # the resident fitness: an MSE run's, before any abs-error run
        ev.ctx.run(_lib.GPE_MODE_MSE)
        t0 = ev.ctx.tournament(None, 40, 3, random.Random(9), weight=-1.0).tolist()
        cases, w4, err, flags = ev.ctx.run_abserr_cases(ar.HIT_EPS, n)
        assert ev.ctx.tournament(None, 40, 3, random.Random(9), weight=-1.0).tolist() == t0
        before = select(ev.ctx, None)
        assert before == select(ev.ctx, cases)
        ev.ctx.run_abserr(ar.HIT_EPS)
        assert select(ev.ctx, None) == before
        ev.ctx.run_moments()
        assert select(ev.ctx, None) == before
        assert ev.ctx.tournament(None, 40, 3, random.Random(9), weight=-1.0).tolist() == t0
        # (predict loads the programs again, which ends the resident fitness
        # as any load does; the matrix is untouched)
        ev.predict(pop, errors="nan")
        assert select(ev.ctx, None) == before
        # another evaluator's squared errors: each context keeps its own
        sq_res = sq.evaluate(pop)
        squares = np.array(sq_res)
        pr.assert_same_bits(squares, cases * cases)
        assert select(sq.ctx, None) == select(sq.ctx, squares)
        assert select(ev.ctx, None) == before
        # a resident-only cases run replaces the matrix as one with a copy does
        ev.ctx.run_abserr_cases(0.5, n, want_cases=False)
        assert select(ev.ctx, None) == before
    finally:
        ev.close()
        sq.close()


# ------------------------------------------------- 7. selection end to end --
def lexicase_cells():
    """symreg10's 700 seeded trees on 512 cases, those that do not raise and
    whose rows (and their squares) are finite, evaluated as one batch by a
    SymbRegCaseAbsErrors and a SymbRegCaseErrors evaluator (kept open for the
    three modes; closed by the last)."""
    if "lex" in _CACHE:
        return _CACHE["lex"]
    from deap_amd.evaluator import GPUEvaluator, SymbRegCaseAbsErrors, SymbRegCaseErrors
    X, Y = datasets.symreg10_cases(512, 9)
    pset = configs.pset_for("symreg10")
    trees = configs.population(pset, "half", 700, 9, 2, 5)
    if not hasattr(creator, "FitnessAbsCases"):
        creator.create("FitnessAbsCases", base.Fitness, weights=(-1.0,) * 512)
        creator.create("IndividualAbsCases", gp.PrimitiveTree, fitness=creator.FitnessAbsCases)
    ev = GPUEvaluator(pset, SymbRegCaseAbsErrors(X, Y), device=0)
    sq = GPUEvaluator(pset, SymbRegCaseErrors(X, Y), device=0)
    with np.errstate(over="ignore"):
        kept = [creator.IndividualAbsCases(t) for t, r in zip(trees, ev.evaluate(trees))
                if not isinstance(r, BaseException) and
                np.isfinite(np.array(r) ** 2).all()]
    assert len(kept) >= 500, len(kept)
    squared = [creator.IndividualAbsCases(t) for t in kept]
    for ind, fit in zip(squared, sq.evaluate(squared)):
        ind.fitness.values = fit
    _CACHE["lex"] = (ev, sq, kept, squared)
    return _CACHE["lex"]


@pytest.mark.parametrize("mode", ["automatic", "plain", "epsilon"])
def test_selection_from_the_resident_matrix(mode):
    """The host loop on the fitness tuples, the GPU drop-in on them and
    ``select_lexicase`` on the resident matrix pick the same 100 individuals
    from the same seed and leave the same ``random`` state; on the squared
    errors of SymbRegCaseErrors automatic (and fixed) epsilon picks others —
    what the absolute errors are for."""
    ev, sq, kept, squared = lexicase_cells()
    try:
        eps, k, seed = 0.05, 100, 77
        host = {"automatic": lambda p: tools.selAutomaticEpsilonLexicase(p, k),
                "plain": lambda p: tools.selLexicase(p, k),
                "epsilon": lambda p: tools.selEpsilonLexicase(p, k, eps)}[mode]
        drop = {"automatic": lambda p: tools.selAutomaticEpsilonLexicaseGPU(p, k, device=0),
                "plain": lambda p: tools.selLexicaseGPU(p, k, device=0),
                "epsilon": lambda p: tools.selEpsilonLexicaseGPU(p, k, eps, device=0)}[mode]
        # (the batch select_lexicase takes is the evaluator's last one)
        for ind, fit in zip(kept, ev.evaluate(kept)):
            ind.fitness.values = fit
        where = {id(x): j for j, x in enumerate(kept)}
        picks, states = [], []
        for sel in (host, drop, lambda p: ev.select_lexicase(p, k, mode, eps)):
            random.seed(seed)
            got = sel(kept)
            assert len(got) == k
            picks.append([where[id(x)] for x in got])
            states.append(random.getstate())
        assert picks[0] == picks[1] == picks[2]
        assert states[0] == states[1] == states[2]
        assert len(set(picks[0])) > 10
        random.seed(seed)
        where_sq = {id(x): j for j, x in enumerate(squared)}
        other = [where_sq[id(x)] for x in sq.select_lexicase(squared, k, mode, eps)]
        if mode == "plain":           # squaring is monotone: the same survivors
            assert other == picks[0]
        else:
            assert other != picks[0]
    finally:
        if mode == "epsilon":
            ev.close()
            sq.close()
            del _CACHE["lex"]


def test_select_lexicase_surfaces_the_librarys_limits():
    """16,384 individuals for ``"automatic"`` and ``n/32 + n_cases`` words
    within 48 KiB of LDS (12,289 cases do not fit), in the library's words;
    another batch is refused before the device."""
    ps, trees, X, y = cells()
    n = sr.N_MAX
    pop = [trees[i] for i in (1, 2, 3, 17, 18)]
    ev = evaluator(n, cases="device")
    try:
        ev.evaluate(pop)
        assert len(ev.select_lexicase(pop, 3, "plain")) == 3
        with pytest.raises(ValueError, match="last evaluate / map"):
            ev.select_lexicase(pop[:4], 3)
    finally:
        ev.close()
    # "automatic" keeps a case's values in LDS: 16,384 individuals at most
    many = [trees[20 + i % 100] for i in range(16385)]
    ev = evaluator(2, cases="device")
    try:
        ev.evaluate(many)
        assert len(ev.select_lexicase(many, 3, "epsilon", 0.1)) == 3
        with pytest.raises(_lib.GpeError, match="at most 16384 individuals"):
            ev.select_lexicase(many, 3, "automatic")
    finally:
        ev.close()
    from deap_amd.evaluator import GPUEvaluator, SymbRegCaseAbsErrors
    m = 12289
    Xm = np.ascontiguousarray(np.resize(X[:, :sr.N_MAX - 1], (10, m)))
    ev = GPUEvaluator(ps, SymbRegCaseAbsErrors(Xm, Xm[0].copy(), cases="device"), device=0)
    try:
        ev.evaluate(pop)
        with pytest.raises(_lib.GpeError, match="n/32 \\+ n_cases words exceed 48 KiB of LDS"):
            ev.select_lexicase(pop, 3, "plain")
    finally:
        ev.close()


# ------------------------------------- 8. resident mode, lazy exceptions --
def test_resident_mode_through_gpu_map():
    """``cases="device"``: the summary tuples of SymbRegAbsError, no host
    matrix asked for or made, exceptions when ``map`` reaches them."""
    from deap_amd.evaluator import GPUEvaluator, SymbRegAbsError, gpu_map
    ps, trees, X, y = cells()
    n = 257
    ref = reference(range(len(trees)), n)
    bad = [i for i in range(len(trees)) if ref[i][1] is not None]
    good = [i for i in range(len(trees)) if ref[i][1] is None][:300]
    pop = [trees[i] for i in good]
    plain = GPUEvaluator(ps, SymbRegAbsError(np.ascontiguousarray(X[:, :n]), y[:n].copy(),
                                             hit_eps=ar.HIT_EPS, fitness=("hits", "mae")),
                         device=0)
    ev = evaluator(n, cases="device", fitness=("hits", "mae"))
    asked = []
    inner = ev.ctx.run_abserr_cases

    def spy(hit_eps, n_cases, want_cases=True):
        out = inner(hit_eps, n_cases, want_cases=want_cases)
        asked.append((want_cases, out[0]))
        return out

    ev.ctx.run_abserr_cases = spy
    tb = base.Toolbox()
    tb.register("evaluate", ev)
    tb.register("map", gpu_map)
    try:
        exp = plain.evaluate(pop)
        fits = list(tb.map(tb.evaluate, pop))
        assert asked == [(False, None)]
        assert len(fits) == len(pop)
        for f, e in zip(fits, exp):
            if isinstance(e, BaseException):
                raise AssertionError("the good trees do not raise")
            assert type(f) is tuple and type(f[0]) is int and type(f[1]) is float
            assert f[0] == e[0] and (f[1] == e[1] or (math.isnan(f[1]) and math.isnan(e[1])))
        _same(ev.last_mae, plain.last_mae)
        _same(ev.last_max_error, plain.last_max_error)
        _same(ev.last_hits, plain.last_hits)
        # lazily, in order: two good ones, then the first bad one's exception
        mixed = [pop[0], pop[1], trees[bad[0]], pop[2], trees[bad[1]]]
        it = tb.map(tb.evaluate, mixed)
        assert next(it) == fits[0] and next(it) == fits[1]
        with pytest.raises(EXC[sr.STATUS[ref[bad[0]][2]]]):
            next(it)
        assert ev.last_hits[2] == -1 and ev.last_hits[3] >= 0
        # ... and select_lexicase raises it too: the first in order
        with pytest.raises(EXC[sr.STATUS[ref[bad[0]][2]]]):
            ev.select_lexicase(mixed, 2)
        # the host mode through the same map
        host = evaluator(n, fitness=("hits", "mae"))
        try:
            rows = list(gpu_map(host, pop[:40]))
            assert all(type(r) is tuple and len(r) == n for r in rows)
            pr.assert_same_bits(np.array(rows), np.array([ref[i][0] for i in good[:40]]))
            _same(host.last_hits, plain.last_hits[:40])
        finally:
            host.close()
    finally:
        ev.close()
        plain.close()


# ------------------------------------------------------------ 9. the C ABI --
def test_the_c_abi_by_raw_ctypes():
    from deap_amd.evaluator import BooleanHits, GPUEvaluator, SymbRegMSE
    ps, trees, X, y = cells()
    n = 64
    Xn = np.ascontiguousarray(X[:, :n])
    f64 = GPUEvaluator(ps, SymbRegMSE(Xn, y[:n]), device=0)
    empty = GPUEvaluator(ps, SymbRegMSE(Xn, y[:n]), device=0)
    f32 = GPUEvaluator(ps, SymbRegMSE(Xn, y[:n]), device=0, precision="fp32")
    pins, pouts = datasets.parity6_table()
    bps = configs.pset_for("parity6")
    bm = GPUEvaluator(bps, BooleanHits(np.ascontiguousarray(pins), np.ascontiguousarray(pouts)),
                      device=0)
    lib, P = f64.ctx.lib, _lib._ptr
    D = ctypes.c_double
    try:
        pop = trees[16:48]
        f64.evaluate(pop)
        f32.evaluate(pop)
        bm.evaluate(configs.population(bps, "half", 32, 17, 2, 5))
        m = len(pop)
        cases = np.full((m, n), -1.0)
        out4, out4b = np.zeros((m, 4)), np.zeros((m, 4))
        err, flags = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint32)
        call = lib.gpe_run_abserr_cases
        assert call(f64.ctx.h, D(0.01), P(cases), P(out4), P(err), P(flags)) == 0
        # out_cases = NULL: accepted, the matrix stays on the device
        assert call(f64.ctx.h, D(0.01), None, P(out4b), None, None) == 0
        pr.assert_same_bits(out4, out4b)
        mx = np.zeros(n, dtype=np.uint8)
        a = f64.ctx.lexicase(None, mx, 20, random.Random(3), 2)
        b = f64.ctx.lexicase(cases, mx, 20, random.Random(3), 2)
        assert a[1] == b[1] == -1 and a[0].tolist() == b[0].tolist()
        w4, e2, f2 = f64.ctx.run_abserr(0.01)
        pr.assert_same_bits(out4, w4)
        assert np.array_equal(err, e2) and np.array_equal(flags, f2)
        vals = f64.predict(pop, errors="nan")
        with np.errstate(invalid="ignore"):
            pr.assert_same_bits(cases, np.abs(vals - y[:n][None, :]))
        # refusals and their codes
        assert call(None, D(0.01), None, P(out4), None, None) == _lib.GPE_E_INVALID
        assert call(f64.ctx.h, D(0.01), P(cases), None, None, None) == _lib.GPE_E_INVALID
        assert call(empty.ctx.h, D(0.01), None, P(out4), None, None) == _lib.GPE_E_INVALID
        assert b"no programs loaded" in lib.gpe_last_error(empty.ctx.h)
        for ctx in (f32.ctx, bm.ctx):
            assert call(ctx.h, D(0.01), None, P(out4), None, None) == _lib.GPE_E_ARG
        for eps in (-1e-300, -math.inf, math.nan):
            assert call(f64.ctx.h, D(eps), None, P(out4), None, None) == _lib.GPE_E_ARG
            assert b"hit_eps" in lib.gpe_last_error(f64.ctx.h)
        with pytest.raises(_lib.GpeError, match=r"\(-6\)"):
            f32.ctx.run_abserr_cases(0.01, n)
        with pytest.raises(ValueError, match="holds 64 cases"):
            f64.ctx.run_abserr_cases(0.01, n + 1)
        # a refused call leaves the next plain run plain, and the matrix alone
        w4b, _, _ = f64.ctx.run_abserr(0.01)
        pr.assert_same_bits(w4b, w4)
        assert f64.ctx.lexicase(None, mx, 20, random.Random(3), 2)[0].tolist() == a[0].tolist()
    finally:
        for ev in (f64, empty, f32, bm):
            ev.close()
