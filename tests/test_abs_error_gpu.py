"""``SymbRegAbsError`` on the GPU against its Python reference
(``abs_error_ref``; recorded in tests/golden/abs_error_n*.npz, recomputed on a
sample by tests/test_abs_error.py): scaled_ref's 2,016 trees and this suite's
six hand-written ones on 1, 2, 127, 128, 129, 257, 1,000, 10,243 and 10,240
cases (the edges of the 128-case tile, the first count with more than one tile
group, and the count whose last case has an inf column).

Per case count: the exceptions and their first cases, ``hits`` equal, ``max``
bit-equal (nan where the reference has nan), the flags, ``mae`` within 1e-12
of the reference relative to it (inf and nan exact), the raw double-double sum
within ``n 2**-100 sum e`` of the exact sum.  No tree is skipped.
"""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import abs_error_ref as ar
import predict_ref as pr
import scaled_ref as sr
from deap_amd import _lib, base, configs, creator, datasets, gp

pytestmark = pytest.mark.gpu
EXC = {1: ValueError, 2: OverflowError, ar.FSUM_OVERFLOW: OverflowError}
NONF, NAN, INF = (_lib.GPE_FLAG_NONFINITE_TERM, _lib.GPE_FLAG_NAN_TERM,
                  _lib.GPE_FLAG_INF_TERM)
ALL3 = ("mae", "max", "hits")
SHAPES = ("abserr", "abserr_deep", "asm_fast", "asm_deep", "cpp_fast", "cpp_deep")
_CACHE = {}


def cells():
    """``(pset, trees, X, y)``, once."""
    if "cells" not in _CACHE:
        ps, trees, n_base = ar.population()
        X, y = sr.data()
        _CACHE["cells"] = (ps, trees, X, y)
        _CACHE["n_base"] = n_base
        _CACHE["key"] = sr.cells_key(trees, X, y)
    return _CACHE["cells"]


def golden(n):
    """The recorded reference as a dict of columns, checked to belong to
    these trees and cases."""
    cells()
    if n not in _CACHE:
        g = ar.load_golden(n, _CACHE["key"])
        _CACHE[n] = {k: g[:, j] for j, k in enumerate(ar.FIELDS)}
    return _CACHE[n]


def evaluator(n, spec_cls=None, fitness=ALL3, hit_eps=ar.HIT_EPS, **kw):
    from deap_amd.evaluator import GPUEvaluator, SymbRegAbsError
    ps, trees, X, y = cells()
    Xn, yn = np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(y[:n])
    spec = spec_cls(Xn, yn) if spec_cls else SymbRegAbsError(Xn, yn, hit_eps=hit_eps,
                                                             fitness=fitness)
    return GPUEvaluator(ps, spec, device=0, **kw)


def run(n, **kw):
    """One evaluation of the population on the first n cases: the results,
    an abs-error run of the same resident programs (words, first errors,
    flags), the launch shapes, and the evaluator's three figures."""
    ps, trees, X, y = cells()
    ev = evaluator(n, **kw)
    try:
        res = ev.evaluate(trees)
        last = (ev.last_mae.copy(), ev.last_max_error.copy(), ev.last_hits.copy())
        w4, err, flags = ev.ctx.run_abserr(ar.HIT_EPS)
        shapes = {k: ev.ctx.launch_shape(k) for k in SHAPES}
    finally:
        ev.close()
    return res, w4, err, flags, shapes, last


def _same(x1, x2, what=""):
    x1, x2 = np.asarray(x1), np.asarray(x2)
    if x1.dtype.kind == "f":
        pr.assert_same_bits(x1, x2, what)
    else:
        assert x1.dtype == x2.dtype and np.array_equal(x1, x2), what


def _rows_programs(shapes):
    return sum(shapes[k]["programs"] for k in ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep"))


# the exact cores' glibc tables, then the tile's columns of 1 KiB (two
# buffers with LDS-DMA), then 2 KiB per program and wave: lds_bytes_asm with
# accw = 2
def _lds(ncol, dbuf, P, wpb):
    return 6016 + ncol * 1024 * (1 + dbuf) + wpb * P * 2 * 1024


@pytest.mark.parametrize("n", ar.CASES)
def test_population_against_the_reference(n):
    """With the evaluator's sin/cos leaf columns the tile has 31 columns
    (10 variables, their sines and cosines, the target): 37,760 B of tables
    and tile leave room for two programs per wave of eight (32 KiB of
    accumulators) under the 80 KB cap, and none for a second tile buffer.
    With a tile or two the planner spreads the 2,018 programs one per wave to
    fill the grid (its rule for every launch); from 80 tiles on the LDS is
    what bounds P."""
    a, ad = _check_population(n)
    assert a["wpb"] == 8 and a["dbuf"] == 0 and 1 <= a["P"] <= 2, a
    assert a["lds_bytes"] == _lds(31, 0, a["P"], 8)
    assert _lds(31, 0, 2, 8) == 70528 <= 80 * 1024 < _lds(31, 0, 3, 8)
    assert _lds(31, 1, 1, 8) > 80 * 1024
    if n >= 10240:
        assert a["P"] == 2, a


@pytest.mark.parametrize("n", [10240, 10243])
def test_three_programs_per_wave_and_two_tile_buffers(n):
    """Without the leaf columns the tile has 11: three programs per wave fit
    with one buffer (66,432 B) and with two (77,696 B), so at an even case
    count the second tile buffer (LDS-DMA) is taken; a fourth would not fit
    (82,816 B with one buffer)."""
    a, ad = _check_population(n, trig_leaves=False)
    dbuf = 1 if n % 2 == 0 else 0
    assert a["wpb"] == 8 and a["P"] == 3 and a["dbuf"] == dbuf, a
    assert a["lds_bytes"] == 6016 + 11 * 1024 * (1 + a["dbuf"]) + 8 * a["P"] * 2 * 1024
    assert a["lds_bytes"] == (77696 if dbuf else 66432) <= 80 * 1024
    assert _lds(11, 0, 4, 8) > 80 * 1024


def _check_population(n, **kw):
    ps, trees, X, y = cells()
    G = golden(n)
    res, w4, err, flags, shapes, last = run(n, **kw)
    assert len(res) == len(trees) == len(G["status"])
    # every route runs: the abs-error kernels of the exact D = 5 and deep
    # cores (more programs than two blocks' P x waves, so they cross waves and
    # blocks) and the rows route (the C++ kernels; at 10,243 cases the values
    # kernels too, for the programs with a redo (program, tile))
    a, ad = shapes["abserr"], shapes["abserr_deep"]
    assert a["programs"] > 1000 and ad["programs"] > 0, shapes
    assert a["programs"] > 2 * a["P"] * a["wpb"]
    assert a["lds_bytes"] <= 80 * 1024 and ad["lds_bytes"] <= 64 * 1024
    assert a["tile_loop"] == 0 and a["K"] == 2
    assert a["n_tiles"] == (n + 127) // 128
    if n >= 10240:
        assert a["groups"] > 1                       # the group reduction is live
    assert shapes["cpp_fast"]["programs"] + shapes["cpp_deep"]["programs"] > 0, shapes
    if n == 10243:
        assert shapes["asm_fast"]["programs"] + shapes["asm_deep"]["programs"] > 50, shapes
    first = (err >> np.uint64(2)).astype(np.int64)
    first[err == np.uint64(_lib.GPE_NO_ERROR)] = -1
    bound = Fraction(n, 2 ** 100)
    worst = {"mae": 0.0, "S": 0.0}
    same_bits = values = 0
    for i, r in enumerate(res):
        what = (i, str(trees[i])[:80])
        st = int(G["status"][i])
        if st:                                   # the reference raises
            assert isinstance(r, EXC[st]), (what, r)
            assert first[i] == int(G["first"][i]), (what, first[i], G["first"][i])
            assert math.isnan(last[0][i]) and math.isnan(last[1][i]) and last[2][i] == -1
            if st == ar.FSUM_OVERFLOW:
                assert str(r) == "intermediate overflow in fsum"
                assert w4[i, 0] == math.inf and not flags[i]
            continue
        assert not isinstance(r, BaseException), (what, r)
        assert first[i] == -1, what
        mae, mx, hits = r
        assert type(hits) is int and type(mae) is float and type(mx) is float
        assert (last[0][i] == mae or math.isnan(mae)) and last[2][i] == hits
        any_nan, any_inf = bool(G["any_nan"][i]), bool(G["any_inf"][i])
        assert bool(flags[i] & NAN) == any_nan, (what, flags[i])
        assert bool(flags[i] & INF) == any_inf, (what, flags[i])
        assert bool(flags[i] & NONF) == (any_nan or any_inf), (what, flags[i])
        assert hits == w4[i, 3] == G["hits"][i], (what, hits, G["hits"][i])
        assert pr.same_bits(np.array([mx]), np.array([G["max"][i]])).all(), \
            (what, mx, G["max"][i])
        if any_nan:
            assert math.isnan(mae) and math.isnan(G["mae"][i])
        elif any_inf:
            assert mae == math.inf == G["mae"][i]
        else:
            ref = float(G["mae"][i])
            assert abs(mae - ref) <= ar.TOL * ref, (what, mae, ref)
            exact = Fraction(float(G["Se_hi"][i])) + Fraction(float(G["Se_lo"][i]))
            d = abs(Fraction(float(w4[i, 0])) + Fraction(float(w4[i, 1])) - exact)
            assert d <= bound * exact, (what, float(d), float(bound * exact))
            if exact:
                worst["S"] = max(worst["S"], float(d / (bound * exact)))
            if ref:
                worst["mae"] = max(worst["mae"], abs(mae - ref) / (ar.TOL * ref))
            values += 1
            same_bits += mae == ref
    print("n = %d: %d of %d finite mae bit-identical to fsum(e) / n; worst error / tolerance %r"
          % (n, same_bits, values, worst))
    print("abs-error launches %r %r" % (a, ad))
    return a, ad


@pytest.mark.parametrize("n", [257, 10243])
def test_two_runs_give_the_same_bits(n):
    r1 = run(n)
    r2 = run(n)
    for x1, x2 in zip(r1[1:4] + r1[5], r2[1:4] + r2[5]):
        _same(x1, x2)
    for a, b in zip(r1[0], r2[0]):
        assert type(a) is type(b)


def test_chunks_of_programs_give_the_same_bits_as_one_run(monkeypatch):
    """The rows route in chunks (as the moments run's test).  With the exact
    cores off (GPE_EXACT_ALL=0) every program takes it: a scratch budget of
    1 MiB (131 rows of 1,000 cases) makes 16 chunks of the 2,022 programs,
    with the bits of one chunk; with the abs-error kernels on, the same budget
    chunks their leftovers, with the bits of the default run."""
    ps, trees, X, y = cells()
    n = 1000
    for exact_all in ("0", "1"):
        monkeypatch.setenv("GPE_EXACT_ALL", exact_all)   # (read when the context is made)
        monkeypatch.delenv("GPE_MOMENTS_MB", raising=False)
        whole = run(n)
        monkeypatch.setenv("GPE_MOMENTS_MB", "1")
        chunked = run(n)
        if exact_all == "0":
            assert whole[4]["abserr"]["programs"] == 0 and _rows_programs(whole[4]) == len(trees)
        else:
            assert whole[4]["abserr"]["programs"] > 1000
        assert 0 < _rows_programs(chunked[4]) <= 131, chunked[4]
        for x1, x2 in zip(whole[1:4] + whole[5], chunked[1:4] + chunked[5]):
            _same(x1, x2)
        for r, w in zip(chunked[0], whole[0]):
            assert type(r) is type(w)


def test_runs_of_other_kinds_around_an_abs_error_run_are_unchanged():
    """The planner's state does not leak: an MSE run and a moments run after
    an abs-error run have the bits, the geometry and every launch shape they
    had before it, and the abs-error run its own."""
    from deap_amd.evaluator import SymbRegMSE
    ps, trees, X, y = cells()
    n = 10243
    ev = evaluator(n, spec_cls=SymbRegMSE)
    try:
        batch = ev.flatten(trees)
        ev.prepare(batch, trees)
        before = ev.ctx.run(_lib.GPE_MODE_MSE)
        geo = ev.ctx.geometry()
        shape = [ev.ctx.launch_shape(k) for k in ev.ctx.LAUNCHES[:7]]
        m1 = ev.ctx.run_moments()
        mshape = [ev.ctx.launch_shape(k) for k in ("moments", "moments_deep")]
        a1 = ev.ctx.run_abserr(ar.HIT_EPS)
        ashape = [ev.ctx.launch_shape(k) for k in ("abserr", "abserr_deep")]
        assert ashape[0]["programs"] > 1000
        assert [ev.ctx.launch_shape(k) for k in ("moments", "moments_deep")] == mshape
        after = ev.ctx.run(_lib.GPE_MODE_MSE)
        assert ev.ctx.geometry() == geo
        assert [ev.ctx.launch_shape(k) for k in ev.ctx.LAUNCHES[:7]] == shape
        for x1, x2 in zip(before, after):
            _same(x1, x2)
        m2 = ev.ctx.run_moments()
        assert [ev.ctx.launch_shape(k) for k in ("moments", "moments_deep")] == mshape
        for x1, x2 in zip(m1, m2):
            _same(x1, x2)
        a2 = ev.ctx.run_abserr(ar.HIT_EPS)
        assert [ev.ctx.launch_shape(k) for k in ("abserr", "abserr_deep")] == ashape
        for x1, x2 in zip(a1, a2):
            _same(x1, x2)
    finally:
        ev.close()


@pytest.mark.parametrize("n", [129, 10243])
def test_threshold_edges(n):
    """``hit_eps = 0`` counts exactly the cases with ``e == 0`` (the target's
    own tree: all n), ``hit_eps = inf`` every finite case (an inf or nan
    ``e`` is never a hit); neither changes the sum or the max."""
    ps, trees, X, y = cells()
    G = golden(n)
    ok = G["status"] == 0
    ev = evaluator(n)
    try:
        ev.evaluate(trees)
        base_w4, err, _ = ev.ctx.run_abserr(ar.HIT_EPS)
        for eps, col in ((0.0, "hits0"), (math.inf, "hits_finite")):
            w4, err2, _ = ev.ctx.run_abserr(eps)
            assert np.array_equal(w4[ok, 3], G[col][ok]), \
                np.flatnonzero(ok & (w4[:, 3] != G[col]))[:10]
            _same(w4[:, :3], base_w4[:, :3])
            _same(err2, err)
        g = _CACHE["n_base"]                       # the target's own tree
        assert G["hits0"][g] == n and G["hits_finite"][g] == n
        if n == 10243:
            assert (G["hits_finite"][ok] < n).sum() > 50     # the inf column's case
    finally:
        ev.close()


def test_two_term_columns():
    """``d = f - t0 - t1``, left to right, on every route (the tile then has
    32 columns): against the host twin on predict's values for what is exact,
    and the Python definition for the mean."""
    from deap_amd.evaluator import GPUEvaluator, SymbRegAbsError
    ps, trees, X, y = cells()
    n = 257
    G = golden(n)
    pick = [i for i in range(0, len(trees), 7) if G["status"][i] == 0][:250] + [10, 11]
    pop = [trees[i] for i in pick]
    Xn = np.ascontiguousarray(X[:, :n])
    T = np.stack([y[:n] * 0.75, X[3, :n] * 0.001])
    ev = GPUEvaluator(ps, SymbRegAbsError(Xn, T, hit_eps=0.05, fitness=ALL3), device=0)
    try:
        res = ev.evaluate(pop)
        w4, err, flags = ev.ctx.run_abserr(0.05)
        assert ev.ctx.launch_shape("abserr")["programs"] > 200
        assert ev.ctx.launch_shape("abserr_deep")["programs"] > 0
        vals = ev.predict(pop)
        for k, r in enumerate(res):
            h4, hf = _lib.host_abserr(vals[k], T, 0.05)
            assert flags[k] == hf and w4[k, 3] == h4[3], (k, w4[k], h4)
            assert pr.same_bits(w4[k, 2:3], h4[2:3]).all()
            if hf:
                continue
            e = [abs(f - a - b) for f, a, b in zip(vals[k].tolist(), T[0].tolist(),
                                                   T[1].tolist())]
            mae, mx, hits = ar.figures(e, 0.05)
            assert r[1] == mx and r[2] == hits and abs(r[0] - mae) <= ar.TOL * mae
    finally:
        ev.close()


def test_the_c_abi_refuses_what_it_does_not_take():
    from deap_amd.evaluator import BooleanHits, GPUEvaluator, SymbRegMSE
    ps, trees, X, y = cells()
    n = 64
    Xn = np.ascontiguousarray(X[:, :n])
    f64 = GPUEvaluator(ps, SymbRegMSE(Xn, y[:n]), device=0)
    f32 = GPUEvaluator(ps, SymbRegMSE(Xn, y[:n]), device=0, precision="fp32")
    pins, pouts = datasets.parity6_table()
    bps = configs.pset_for("parity6")
    bm = GPUEvaluator(bps, BooleanHits(np.ascontiguousarray(pins), np.ascontiguousarray(pouts)),
                      device=0)
    try:
        f64.evaluate(trees[16:48])
        f32.evaluate(trees[16:48])
        bm.evaluate(configs.population(bps, "half", 32, 17, 2, 5))
        for ev in (f32, bm):
            with pytest.raises(_lib.GpeError, match=r"\(-6\)"):
                ev.ctx.run_abserr(0.01)
        for eps in (-1e-300, -math.inf, math.nan):
            with pytest.raises(_lib.GpeError, match=r"\(-6\)"):
                f64.ctx.run_abserr(eps)
        w4, err, flags = f64.ctx.run_abserr(0.0)
        assert w4.shape == (32, 4)
    finally:
        f64.close()
        f32.close()
        bm.close()


def test_device_outputs_equal_the_host_outputs():
    import torch
    ps, trees, X, y = cells()
    n = 257
    ev = evaluator(n)
    try:
        ev.evaluate(trees[:600])
        w4, err, flags = ev.ctx.run_abserr(ar.HIT_EPS)
        dev = torch.device("cuda:0")
        d = torch.zeros((600, 4), dtype=torch.float64, device=dev)
        de = torch.zeros(600, dtype=torch.int64, device=dev)
        df = torch.zeros(600, dtype=torch.int32, device=dev)
        ev.ctx.run_abserr_device(ar.HIT_EPS, d.data_ptr(), de.data_ptr(), df.data_ptr())
        torch.cuda.synchronize()
        pr.assert_same_bits(d.cpu().numpy(), w4)
        assert (de.cpu().numpy().view(np.uint64) == err).all()
        assert (df.cpu().numpy().view(np.uint32) == flags).all()
    finally:
        ev.close()


def test_fitness_order_through_gpu_map():
    """``fitness=("hits", "mae")`` with a creator fitness of weights
    (1.0, -1.0): ``(int, float)`` tuples in that order, one per individual,
    exceptions delivered lazily by ``map``."""
    from deap_amd.evaluator import gpu_map
    ps, trees, X, y = cells()
    n = 1000
    G = golden(n)
    ev = evaluator(n, fitness=("hits", "mae"))
    creator.create("FitnessHitsMae", base.Fitness, weights=(1.0, -1.0))
    creator.create("IndividualHitsMae", gp.PrimitiveTree, fitness=creator.FitnessHitsMae)
    tb = base.Toolbox()
    tb.register("evaluate", ev)
    tb.register("map", gpu_map)
    random.seed(3)
    ok = [i for i in range(len(trees)) if G["status"][i] == 0 and not G["any_nan"][i]]
    pick = random.sample(ok, 200)
    pop = [creator.IndividualHitsMae(trees[i]) for i in pick]
    try:
        fits = list(tb.map(tb.evaluate, pop))
        assert len(fits) == len(pop)
        for ind, fit, i in zip(pop, fits, pick):
            assert type(fit) is tuple and type(fit[0]) is int and type(fit[1]) is float
            ind.fitness.values = fit
            assert ind.fitness.valid and fit[0] == G["hits"][i]
            assert fit[1] == G["mae"][i] or abs(fit[1] - G["mae"][i]) <= ar.TOL * G["mae"][i]
        assert ev.last_hits.dtype == np.int64 and len(ev.last_hits) == len(pop)
        assert ev.last_mae.dtype == ev.last_max_error.dtype == np.float64
        best = max(pop, key=lambda ind: ind.fitness)
        assert best.fitness.values[0] == max(f[0] for f in fits)
        # an individual that raises: the exception arrives when map reaches it
        bad = [i for i in range(len(trees)) if G["status"][i] == 1][:1]
        it = ev.map([trees[pick[0]], trees[bad[0]]])
        assert next(it) == fits[0]
        with pytest.raises(ValueError):
            next(it)
        assert ev.last_hits[1] == -1 and math.isnan(ev.last_mae[1])
        single = ev(trees[pick[1]])
        assert single == fits[1]
    finally:
        ev.close()
