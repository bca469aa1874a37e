"""``SymbRegScaledMSE`` on the GPU against the exact-rational reference
(``scaled_ref``; recorded in tests/golden/scaled_mse_n*.npz, recomputed on a
sample by tests/test_scaled_mse.py): 2,000 seeded trees of the headline
primitive set and the hand-written ones (a constant, x0, affine images of the
target, outputs past 2**500 and inf, sin of an overflowing product, sqrt of a
negative column, exact-int programs, the deep core's and the C++ kernels'
stack depths, a column with an inf in the last case) on 1, 2, 127, 128, 129,
257, 1,000, 10,243 and 10,240 cases.

Per case count: the raw moments within ``n 2**-100 sum|term|`` of the exact
sums, ``mse`` within ``1e-12 max(mse, vy/n)``, ``a`` and ``b`` within 1e-12 of
their scales (``scaled_ref.record``), the exceptions and their first cases.
A program under the range rule (an inf, nan or ``|f| >= 2**500`` output)
leaves such cases out of its sums, so its moments are not the reference's
(which has none): its flag, ``mse = inf``, ``b = 0`` and ``a`` are checked.
"""
import math
import operator
import random
from fractions import Fraction

import numpy as np
import pytest

import predict_ref as pr
import scaled_ref as sr
from deap_amd import _lib, algorithms, base, configs, creator, gp, tools

pytestmark = pytest.mark.gpu
EXC = {1: ValueError, 2: OverflowError}
_CACHE = {}


def cells():
    """``(pset, trees, X, y)``, once."""
    if "cells" not in _CACHE:
        ps, trees = sr.population()
        X, y = sr.data()
        _CACHE["cells"] = (ps, trees, X, y)
        _CACHE["key"] = sr.cells_key(trees, X, y)
    return _CACHE["cells"]


def golden(n):
    """The recorded reference, checked to belong to these trees and cases."""
    cells()
    return sr.load_golden(n, _CACHE["key"])


def evaluator(n, spec_cls=None, **kw):
    from deap_amd.evaluator import GPUEvaluator, SymbRegScaledMSE
    ps, trees, X, y = cells()
    return GPUEvaluator(ps, (spec_cls or SymbRegScaledMSE)(
        np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(y[:n])), device=0, **kw)


def run(n, **kw):
    """One evaluation of the population on the first n cases: the results,
    (a, b), and a moments run of the same resident programs."""
    ps, trees, X, y = cells()
    ev = evaluator(n, **kw)
    try:
        res = ev.evaluate(trees)
        a, b = ev.last_scaling
        m6, err, flags = ev.ctx.run_moments()
        # the moments kernels' launches, and the rows route's last values run
        shapes = {k: ev.ctx.launch_shape(k)
                  for k in ("moments", "moments_deep", "asm_fast", "asm_deep", "cpp_fast",
                            "cpp_deep")}
    finally:
        ev.close()
    return res, a.copy(), b.copy(), m6, err, flags, shapes


def _same(x1, x2, what=""):
    x1, x2 = np.asarray(x1), np.asarray(x2)
    if x1.dtype.kind == "f":
        pr.assert_same_bits(x1, x2, what)
    else:
        assert x1.dtype == x2.dtype and np.array_equal(x1, x2), what


def _fr(hi, lo):
    return Fraction(float(hi)) + Fraction(float(lo))


@pytest.mark.parametrize("n", sr.CASES)
def test_population_against_the_reference(n):
    """With the evaluator's sin/cos leaf columns the tile has 31 columns: one
    program per wave, one tile buffer."""
    m, md = _check_population(n)
    assert m["P"] == 1 and m["dbuf"] == 0


@pytest.mark.parametrize("n", [10240, 10243])
def test_two_programs_per_wave_and_two_tile_buffers(n):
    """Without the leaf columns the tile has 11: the three-pair accumulators
    leave two programs per wave at the 80 KB cap, and at an even case count
    the second tile buffer (LDS-DMA) is taken."""
    m, md = _check_population(n, trig_leaves=False)
    assert m["P"] == 2 and m["dbuf"] == (1 if n % 2 == 0 else 0), m
    assert m["lds_bytes"] == 6016 + 11 * 1024 * (1 + m["dbuf"]) + 8 * 2 * 3 * 1024


def _check_population(n, **kw):
    ps, trees, X, y = cells()
    gold = golden(n)
    G = {k: gold[:, j] for j, k in enumerate(sr.FIELDS)}
    res, a, b, m6, err, flags, shapes = run(n, **kw)
    assert len(res) == len(trees) == len(gold)
    # every route runs: the moments kernels of the exact D = 5 and deep cores
    # (more programs than one block's P x waves, so they cross waves and
    # blocks) and the rows route (the C++ kernels; at 10,243 cases the values
    # kernels too, for the programs with a redo (program, tile))
    m, md = shapes["moments"], shapes["moments_deep"]
    assert m["programs"] > 1000 and md["programs"] > 0, shapes
    assert m["programs"] > 2 * m["P"] * m["wpb"]
    # (the deep core's 48 KB is a target its tables and one program's 3 KiB
    # per wave pass at P = 1; a block may use 160 KB)
    assert m["lds_bytes"] <= 80 * 1024 and md["lds_bytes"] <= 64 * 1024 and md["P"] == 1
    assert m["tile_loop"] == 0 and m["K"] == 2
    assert m["n_tiles"] == (n + 127) // 128
    if n >= 10240:
        assert m["groups"] > 1                       # the group reduction is live
    assert shapes["cpp_fast"]["programs"] + shapes["cpp_deep"]["programs"] > 0, shapes
    if n == 10243:
        assert shapes["asm_fast"]["programs"] + shapes["asm_deep"]["programs"] > 50, shapes
    first = (err >> np.uint64(2)).astype(np.int64)
    first[err == np.uint64(_lib.GPE_NO_ERROR)] = -1
    bound = Fraction(n, 2 ** 100)
    worst = {"mse": 0.0, "a": 0.0, "b": 0.0, "S": 0.0}
    for i, r in enumerate(res):
        st = int(G["status"][i])
        if st:                                   # the reference raises
            assert isinstance(r, EXC[st]), (i, str(trees[i])[:80], r)
            assert first[i] == int(G["first"][i]), (i, first[i], G["first"][i])
            continue
        assert not isinstance(r, BaseException), (i, str(trees[i])[:80], r)
        assert first[i] == -1
        mse, = r
        flagged = bool(flags[i] & _lib.GPE_FLAG_MOMENT_RANGE)
        assert flagged == bool(G["flagged"][i]), (i, str(trees[i])[:80])
        if flagged:
            assert mse == math.inf and b[i] == 0.0
        else:
            assert abs(mse - G["mse"][i]) <= G["tol_mse"][i], \
                (i, str(trees[i])[:80], mse, G["mse"][i])
            assert abs(b[i] - G["b"][i]) <= G["tol_b"][i], (i, b[i], G["b"][i])
            for k, (name, A) in enumerate((("Sf", G["Af"][i]), ("Sff", G["Sff_hi"][i]),
                                           ("Sfy", G["Afy"][i]))):
                d = abs(_fr(m6[i, 2 * k], m6[i, 2 * k + 1]) -
                        _fr(G[name + "_hi"][i], G[name + "_lo"][i]))
                lim = bound * Fraction(float(A))
                assert d <= lim, (i, name, str(trees[i])[:80], float(d), float(lim))
                if lim:
                    worst["S"] = max(worst["S"], float(d / lim))
            for k, got in (("mse", mse), ("b", b[i])):
                if G["tol_" + k][i]:
                    worst[k] = max(worst[k], abs(got - G[k][i]) / G["tol_" + k][i])
        assert abs(a[i] - G["a"][i]) <= G["tol_a"][i], (i, a[i], G["a"][i])
        if G["tol_a"][i]:
            worst["a"] = max(worst["a"], abs(a[i] - G["a"][i]) / G["tol_a"][i])
    print("n = %d: worst error / tolerance %r" % (n, worst))
    print("moments launches %r %r" % (m, md))
    return m, md


@pytest.mark.parametrize("n", [257, 10243])
def test_two_runs_give_the_same_bits(n):
    r1 = run(n)
    r2 = run(n)
    for x1, x2 in zip(r1[1:6], r2[1:6]):
        _same(x1, x2)
    f1 = [math.nan if isinstance(r, BaseException) else r[0] for r in r1[0]]
    f2 = [math.nan if isinstance(r, BaseException) else r[0] for r in r2[0]]
    pr.assert_same_bits(np.array(f1), np.array(f2), "mse")


def _rows_programs(shapes):
    return sum(shapes[k]["programs"] for k in ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep"))


def test_chunks_of_programs_give_the_same_bits_as_one_run(monkeypatch):
    """The rows route in chunks.  With the exact cores off (GPE_EXACT_ALL=0)
    every program takes it: a scratch budget of 1 MiB (131 rows of 1,000
    cases) makes 16 chunks of the 2,016 programs, exact-int programs, redo
    programs and first errors included, with the bits of one chunk.  With the
    moments kernels on, the same budget chunks their leftovers, with the bits
    of the default run.  An MSE run afterwards plans every program again."""
    ps, trees, X, y = cells()
    n = 1000
    for exact_all in ("0", "1"):
        monkeypatch.setenv("GPE_EXACT_ALL", exact_all)   # (read when the context is made)
        monkeypatch.delenv("GPE_MOMENTS_MB", raising=False)
        whole = run(n)
        monkeypatch.setenv("GPE_MOMENTS_MB", "1")
        chunked = run(n)
        if exact_all == "0":
            assert whole[6]["moments"]["programs"] == 0 and _rows_programs(whole[6]) == len(trees)
        else:
            assert whole[6]["moments"]["programs"] > 1000
        assert 0 < _rows_programs(chunked[6]) <= 131, chunked[6]
        for x1, x2 in zip(whole[1:6], chunked[1:6]):
            _same(x1, x2)
        for r, w in zip(chunked[0], whole[0]):
            assert type(r) is type(w) and (isinstance(r, BaseException) or r == w)
    from deap_amd.evaluator import SymbRegMSE
    monkeypatch.delenv("GPE_MOMENTS_MB")
    ref = evaluator(n, spec_cls=SymbRegMSE)
    monkeypatch.setenv("GPE_MOMENTS_MB", "1")
    ev = evaluator(n, spec_cls=SymbRegMSE)
    try:
        for e in (ref, ev):
            e.prepare(e.flatten(trees), trees)
        exp = ref.ctx.run(_lib.GPE_MODE_MSE)
        m6 = ev.ctx.run_moments()[0]
        _same(m6, whole[3])
        got = ev.ctx.run(_lib.GPE_MODE_MSE)
        for x1, x2 in zip(got, exp):
            _same(x1, x2)
        assert ev.ctx.geometry() == ref.ctx.geometry()
        assert [ev.ctx.launch_shape(k) for k in ev.ctx.LAUNCHES[:7]] == \
            [ref.ctx.launch_shape(k) for k in ref.ctx.LAUNCHES[:7]]
    finally:
        ref.close()
        ev.close()


def test_the_c_abi_refuses_what_it_does_not_take():
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    ps, trees, X, y = cells()
    n = 64
    Xn = np.ascontiguousarray(X[:, :n])
    two = GPUEvaluator(ps, SymbRegMSE(Xn, np.stack([y[:n], y[:n]])), device=0)
    f32 = GPUEvaluator(ps, SymbRegMSE(Xn, y[:n]), device=0, precision="fp32")
    try:
        for ev in (two, f32):
            ev.evaluate(trees[16:48])
            with pytest.raises(_lib.GpeError, match=r"\(-6\)"):
                ev.ctx.run_moments()
            with pytest.raises(_lib.GpeError, match=r"\(-6\)"):
                ev.ctx.run_scaled((0.0, 0.0), (1.0, 0.0))
    finally:
        two.close()
        f32.close()


def test_device_outputs_equal_the_host_outputs():
    import torch
    ps, trees, X, y = cells()
    n = 257
    ev = evaluator(n)
    try:
        ev.evaluate(trees[:600])
        mse, a, b, err, flags = ev.ctx.run_scaled(ev.spec.sy, ev.spec.syy)
        dev = torch.device("cuda:0")
        d = [torch.zeros(600, dtype=torch.float64, device=dev) for _ in range(3)]
        de = torch.zeros(600, dtype=torch.int64, device=dev)
        df = torch.zeros(600, dtype=torch.int32, device=dev)
        ev.ctx.run_scaled_device(ev.spec.sy, ev.spec.syy, d[0].data_ptr(), d[1].data_ptr(),
                                 d[2].data_ptr(), de.data_ptr(), df.data_ptr())
        torch.cuda.synchronize()
        for got, exp in zip(d, (mse, a, b)):
            pr.assert_same_bits(got.cpu().numpy(), exp)
        assert (de.cpu().numpy().view(np.uint64) == err).all()
        assert (df.cpu().numpy().view(np.uint32) == flags).all()
    finally:
        ev.close()


def test_five_generations_with_gpu_map():
    from deap_amd.evaluator import GPUEvaluator, SymbRegScaledMSE, gpu_map
    ps0, trees, X, y = cells()
    pset = configs.pset_for("symreg10")
    n = 1024
    ev = GPUEvaluator(pset, SymbRegScaledMSE(np.ascontiguousarray(X[:, :n]), y[:n].copy()),
                      device=0)
    creator.create("FitnessMinS", base.Fitness, weights=(-1.0,))
    creator.create("IndividualS", gp.PrimitiveTree, fitness=creator.FitnessMinS)
    tb = base.Toolbox()
    tb.register("expr", gp.genHalfAndHalf, pset=pset, min_=1, max_=3)
    tb.register("individual", tools.initIterate, creator.IndividualS, tb.expr)
    tb.register("population", tools.initRepeat, list, tb.individual)
    tb.register("evaluate", ev)
    tb.register("map", gpu_map)
    tb.register("select", tools.selTournament, tournsize=3)
    tb.register("mate", gp.cxOnePoint)
    tb.register("expr_mut", gp.genFull, min_=0, max_=2)
    tb.register("mutate", gp.mutUniform, expr=tb.expr_mut, pset=pset)
    for op in ("mate", "mutate"):
        tb.decorate(op, gp.staticLimit(key=operator.attrgetter("height"), max_value=17))
    random.seed(7)
    pop = tb.population(n=200)
    try:
        pop, log = algorithms.eaSimple(pop, tb, 0.5, 0.1, 5, verbose=False)
        assert len(log) == 6 and all(ind.fitness.valid for ind in pop)
        fit = np.array([ind.fitness.values[0] for ind in pop])
        assert not np.isnan(fit).any() and (fit >= 0.0).all()
        # 1:1 and in order: each individual's fitness is its own
        again = list(gpu_map(tb.evaluate, pop))
        assert [ind.fitness.values for ind in pop] == again
        vy_n = np.var(y[:n])
        assert fit.min() <= vy_n * (1 + 1e-9)       # no fit is worse than a constant's
    finally:
        ev.close()


def test_predict_scaled_uses_the_training_coefficients():
    ps, trees, X, y = cells()
    n = 257
    gold = golden(n)
    pop = [t for t, g in zip(trees, gold) if g[0] == 0][:150]
    held = np.ascontiguousarray(X[:, 300:431])
    ev = evaluator(n)
    try:
        ev.evaluate(pop)
        a, b = (v.copy() for v in ev.last_scaling)
        for rows in (None, held):
            plain = ev.predict(pop, X=rows)
            got = ev.predict(pop, X=rows, scaled=True)
            with np.errstate(invalid="ignore"):
                pr.assert_same_bits(got, a[:, None] + b[:, None] * plain)
        pr.assert_same_bits(ev.last_scaling[0], a)
        with pytest.raises(ValueError):           # an erroring training case: no fit
            ev.predict([trees[7]], scaled=True)
    finally:
        ev.close()
    from deap_amd.evaluator import SymbRegMSE
    other = evaluator(n, spec_cls=SymbRegMSE)
    try:
        with pytest.raises(ValueError, match="SymbRegScaledMSE"):
            other.predict(pop[:2], scaled=True)
    finally:
        other.close()


def test_an_mse_run_after_a_moments_run_is_the_run_before_it():
    """The planner's state does not leak: the same bits and the same launch
    geometry (compare test_planner_state_across_batches_of_different_routing)."""
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
        after = ev.ctx.run(_lib.GPE_MODE_MSE)
        assert ev.ctx.geometry() == geo
        assert [ev.ctx.launch_shape(k) for k in ev.ctx.LAUNCHES[:7]] == shape
        for x1, x2 in zip(before, after):
            _same(x1, x2)
        m2 = ev.ctx.run_moments()
        for x1, x2 in zip(m1, m2):
            _same(x1, x2)
    finally:
        ev.close()
