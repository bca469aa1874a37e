"""DALex selection and weighted error sums on the GPU: the fp64 MFMA product
on exact data (which catches a wrong lane map), on general data under the gap
criterion of ``dalex_ref``, at shapes that straddle the MFMA's 16 and 4, the
64-row and 64-column wave tiles and the 256-column blocks; the device's weights
and sigma against the host twins; position independence; hit planes; and
``GPUEvaluator.select_dalex`` / ``weighted_errors`` / ``tools.selDALexGPU`` end
to end, with what they must leave undisturbed.

A wave's tile is 64 rows x 64 selections and a block is four of them side by
side, so n = 130 and 200 span three and four row tiles, k = 300 two blocks (the
second with idle waves), and n_cases = 1, 3, 5, 33, 257 leave every remainder
of the k-step of 4."""
import random

import numpy as np
import pytest

import dalex_ref as ref
from deap_amd import _lib, configs, datasets, gp, tools
from deap_amd.evaluator import (BooleanCaseHits, GPUEvaluator, SymbRegCaseAbsErrors,
                                SymbRegMSE, TypedCaseHits, pack_bitplanes)

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def errors(seed, n, n_cases):
    rng = np.random.default_rng(seed)
    return np.abs(rng.normal(size=(n, n_cases))) * rng.uniform(0.1, 10.0, n_cases)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# --------------------------------------------------------- exact data --
@pytest.mark.parametrize("n, n_cases, G", [
    (1, 1, 1), (15, 3, 15), (17, 5, 17), (130, 33, 300), (200, 257, 17), (64, 4, 64),
    (65, 256, 257)])
def test_weighted_errors_on_exact_data_is_numpy_bit_for_bit(ctx, n, n_cases, G):
    """Small integers times powers of two: every product and partial sum is
    exact, so any wrong lane, row or column shows as a wrong number."""
    rng = np.random.default_rng(n * 1009 + n_cases * 31 + G)
    E = rng.integers(0, 8, size=(n, n_cases)).astype(np.float64)
    W = 2.0 ** rng.integers(-3, 4, size=(G, n_cases))
    W[rng.random((G, n_cases)) < 0.1] = 0.0
    got = ctx.weighted_errors(E, W)
    assert got.shape == (n, G) and got.dtype == np.float64
    assert bits_equal(got, E @ W.T), np.argwhere(got != E @ W.T)[:5]
    assert ctx.dalex_ms() >= 0.0
    if n >= 15:
        E[3, 1 % n_cases] = np.inf
        E[n - 1, 0] = np.nan
        got = ctx.weighted_errors(E, W)
        keep = np.ones(n, dtype=bool)
        keep[[3, n - 1]] = False
        assert np.isnan(got[~keep]).all() and bits_equal(got[keep], E[keep] @ W[:, :].T)


@pytest.mark.parametrize("n, n_cases, k", [
    (1, 1, 1), (15, 4, 15), (17, 32, 17), (130, 256, 300), (200, 8, 300), (130, 1, 17)])
def test_dalex_on_exact_data_picks_what_the_host_twin_picks(ctx, n, n_cases, k):
    """pressure 0 without standardisation, C a power of two: the weights are
    exactly 1 / C and the scores exact; with four values per case many rows
    tie, so the tie keys are at work as well."""
    rng = np.random.default_rng(n * 7 + n_cases)
    E = rng.integers(0, 4 if n_cases <= 8 else 2, size=(n, n_cases)).astype(np.float64)
    if n >= 15:
        E[n - 2] = E[1]                               # duplicates for certain
        E[0, 0] = np.inf
    for seed in (3, 1 << 63):
        exp, efail = _lib.host_dalex(E, k, seed, 0.0, False)
        got, failed = ctx.dalex(E, k, seed, 0.0, False)
        assert failed == efail == -1
        assert got.tolist() == exp.tolist()
    wt = ctx.dalex_weights(n_cases, k, 3, 0.0)
    assert wt.shape == (n_cases, k) and np.all(wt == 1.0 / n_cases)
    E[:, 0] = np.nan                                  # nobody is fit
    got, failed = ctx.dalex(E, k, 3, 0.0, False)
    assert got.tolist() == [-1] * k and failed == 0
    assert np.isnan(ctx.weighted_errors(E, np.ones(n_cases))).all()


# ------------------------------------------------------- general data --
@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("n, n_cases, k, pressure", [
    (1, 1, 1, 1.0), (15, 3, 15, 0.5), (17, 5, 300, 3.0), (130, 33, 300, 3.0),
    (200, 257, 17, 1.0), (130, 257, 15, 20.0)])
def test_dalex_on_general_data_under_the_gap_criterion(ctx, n, n_cases, k, pressure,
                                                       standardize):
    E = errors(n * 7 + n_cases, n, n_cases)
    if n >= 15:
        E[2, 0] = np.inf                              # an unfit row
    seed = 0xC0FFEE + n
    sigma = ctx.dalex_sigma(E) if standardize else None
    wt = ctx.dalex_weights(n_cases, k, seed, pressure, sigma)
    S = ref.scores(E, wt)                             # fsum on the device's own weights
    got, failed = ctx.dalex(E, k, seed, pressure, standardize)
    assert failed == -1 and got.shape == (k,)
    ref.check(got, S, seed, n_cases)
    if n >= 15:
        assert 2 not in got.tolist()


@pytest.mark.parametrize("pressure", [0.0, 0.25, 3.0, 20.0, 200.0])
@pytest.mark.parametrize("n_cases, k", [(1, 1), (3, 15), (5, 17), (33, 300), (257, 65)])
def test_the_device_weights_agree_with_the_host_twin(ctx, n_cases, k, pressure):
    seed = 0x1234567890ABCDEF ^ k
    got = ctx.dalex_weights(n_cases, k, seed, pressure)
    exp = _lib.host_dalex_weights(n_cases, k, seed, pressure)
    assert got.shape == exp.shape
    assert ref.weights_close(got, exp, pressure), np.abs(got - exp).max()
    assert np.all(np.abs(got.sum(axis=0) - 1.0) <= n_cases * 2.0 ** -53)
    sigma = np.linspace(0.5, 2.0, n_cases)
    sigma[n_cases // 2] = 0.0
    std = ctx.dalex_weights(n_cases, k, seed, pressure, sigma)
    assert np.all(std[n_cases // 2] == 0.0)
    keep = sigma > 0
    assert bits_equal(std[keep], got[keep] / sigma[keep, None])


@pytest.mark.parametrize("n, n_cases", [(1, 1), (15, 3), (17, 5), (130, 33), (600, 257)])
def test_the_device_sigma_agrees_with_the_host_twin_and_numpy(ctx, n, n_cases):
    E = errors(n, n, n_cases)
    E[:, 0] = 2.5
    got = ctx.dalex_sigma(E)
    assert got[0] == 0.0
    for exp in (_lib.host_dalex_sigma(E), E.std(axis=0)):
        assert np.all(np.abs(got - exp) <= 1e-12 * exp)
    if n >= 15:
        F = E.copy()
        F[4, n_cases - 1] = np.nan
        exp = np.delete(E, 4, axis=0).std(axis=0)
        assert np.all(np.abs(ctx.dalex_sigma(F) - exp) <= 1e-12 * exp)


@pytest.mark.parametrize("n, n_cases, G", [(1, 1, 1), (17, 5, 15), (130, 33, 17), (200, 257, 8)])
def test_weighted_errors_on_general_data_is_within_gamma_of_fsum(ctx, n, n_cases, G):
    E = errors(n + G, n, n_cases)
    W = np.random.default_rng(G).random((G, n_cases))
    if n >= 15:
        E[5, 2] = np.inf
    got = ctx.weighted_errors(E, W)
    exp = ref.scores(E, np.ascontiguousarray(W.T))
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.all(np.abs(got[ok] - exp[ok]) <= ref.gamma(n_cases) * exp[ok])
    one = ctx.weighted_errors(E, W[0])                # 1-D weights: one row
    assert bits_equal(one[:, 0], got[:, 0])


# ----------------------------------------------- position independence --
def test_permuting_the_rows_permutes_nothing_but_the_indices(ctx):
    E = errors(99, 200, 33)
    perm = np.random.default_rng(1).permutation(200)
    for standardize in (True, False):
        a, _ = ctx.dalex(E, 300, 42, 3.0, standardize)
        b, _ = ctx.dalex(E[perm], 300, 42, 3.0, standardize)
        assert np.array_equal(E[a], E[perm][b])
    # a row scores the same bits wherever it stands, and whatever n and k are
    W = np.random.default_rng(2).random((300, 33))
    full = ctx.weighted_errors(E, W)
    assert bits_equal(ctx.weighted_errors(E[perm], W), full[perm])
    assert bits_equal(ctx.weighted_errors(E[60:131], W[250:]), full[60:131, 250:])


def test_duplicated_rows_are_picked_by_key_as_the_host_twin_picks(ctx):
    rng = np.random.default_rng(5)
    base = rng.integers(0, 3, size=(20, 16)).astype(np.float64)
    E = base[rng.integers(0, 20, size=200)]           # 200 rows, 20 distinct
    exp, _ = _lib.host_dalex(E, 300, 77, 0.0, False)
    got, failed = ctx.dalex(E, 300, 77, 0.0, False)
    assert failed == -1 and got.tolist() == exp.tolist()
    assert len(set(got.tolist())) > 3 and len({tuple(E[i]) for i in got}) == 1
    # general weights: identical rows score identical bits, so the winner's
    # duplicates tie exactly and the key picks among them
    F = errors(6, 10, 33)[rng.integers(0, 10, size=130)]
    got, _ = ctx.dalex(F, 300, 78, 1.0, True)
    wt = ctx.dalex_weights(33, 300, 78, 1.0, ctx.dalex_sigma(F))
    S = ctx.weighted_errors(F, np.ascontiguousarray(wt.T))
    for s in range(300):
        col = S[:, s]
        tied = np.flatnonzero(col == col.min())
        assert len({tuple(F[i]) for i in tied}) == 1
        assert got[s] == ref.pick(S, 78, s)


# ----------------------------------------------------------- hit planes --
def boolean():
    if "bool" not in _CACHE:
        ps = configs.pset_for("parity6")
        ins, outs = datasets.parity6_table()
        _CACHE["bool"] = (ps, configs.population(ps, "half", 200, 11, 2, 5), ins, outs)
    return _CACHE["bool"]


def typed():
    if "typed" not in _CACHE:
        ps = configs.pset_for("spambase")
        X, lab = datasets.spambase_like(129, 57)
        _CACHE["typed"] = (ps, configs.population(ps, "half", 130, 57, 2, 4), X, lab)
    return _CACHE["typed"]


@pytest.mark.parametrize("machine", ["boolean", "typed"])
def test_hit_planes_give_the_picks_of_the_unpacked_matrix(machine):
    if machine == "boolean":
        ps, pop, ins, outs = boolean()
        spec = BooleanCaseHits(ins, outs, "device")
    else:
        ps, pop, X, lab = typed()
        spec = TypedCaseHits(X, lab, "device")
    ev = GPUEvaluator(ps, spec, device=0)
    try:
        fit = ev.evaluate(pop)
        H = ev.last_case_hits()
        n, C = H.shape
        E = 1.0 - H.astype(np.float64)
        random.seed(12)
        lex = [id(t) for t in ev.select_lexicase(pop, 40, parallel=True)]
        for standardize, pressure in ((True, 2.0), (False, 2.0), (True, 0.0)):
            got, failed = ev.ctx.dalex_bits(None, 0, 0, 300, 31, pressure, standardize)
            exp, _ = ev.ctx.dalex(E, 300, 31, pressure, standardize)
            assert failed == -1 and got.tolist() == exp.tolist()
            mine, _ = ev.ctx.dalex_bits(pack_bitplanes(H), n, C, 300, 31, pressure, standardize)
            assert mine.tolist() == exp.tolist()
        sigma = ev.ctx.dalex_sigma(E)
        p = E.mean(axis=0)
        assert np.allclose(sigma, np.sqrt(p * (1.0 - p)), rtol=1e-12, atol=0.0)
        # through the evaluator, and nothing resident has moved
        random.seed(4)
        picks = ev.select_dalex(pop, 50, 2.0)
        seed = ev.last_dalex_seed
        assert [pop.index(t) for t in picks] == \
            ev.ctx.dalex(E, 50, seed, 2.0, True)[0].tolist()
        assert np.array_equal(ev.last_case_hits(), H)
        random.seed(12)
        assert [id(t) for t in ev.select_lexicase(pop, 40, parallel=True)] == lex
        assert ev.evaluate(pop) == fit
        with pytest.raises(ValueError, match="weighted_errors: this evaluator's last evaluate / "
                                             "map left no per-case errors on the GPU"):
            ev.weighted_errors(np.ones(C))
    finally:
        ev.close()


# ------------------------------------------------- through the evaluator --
def regression():
    """(pset, trees, X [10, 129], y): real-valued cases; ARG3 is inf at case 9
    (rows with an inf error are unfit), ``sqrt(ARG0)`` raises where ARG0 < 0."""
    if "reg" not in _CACHE:
        ps = configs.pset_for("symreg10_sqrt")
        rng = np.random.default_rng(129)
        X = rng.normal(size=(10, 129))
        y = X[0] * X[1] + X[2]
        X[3, 9] = np.inf
        hand = ["ARG0", "ARG3", "mul(ARG0, ARG1)", "add(mul(ARG0, ARG1), ARG1)", "sqrt(ARG0)",
                "add(ARG2, mul(ARG1, ARG1))"]
        trees = [gp.PrimitiveTree.from_string(s, ps) for s in hand] + \
            configs.population(ps, "half", 150, 23, 1, 4)
        _CACHE["reg"] = (ps, trees, X, y)
    return _CACHE["reg"]


def host_matrix(ps, trees, X, y, idx=None):
    ev = GPUEvaluator(ps, SymbRegCaseAbsErrors(X, y, cases="host"), device=0)
    try:
        if idx is not None:
            ev.subsample(idx)
        return ev.evaluate(trees)
    finally:
        ev.close()


@pytest.mark.parametrize("subset", [False, True])
def test_select_dalex_after_case_abs_errors_on_the_device(subset):
    ps, trees, X, y = regression()
    # (a subset keeps case 9, where ARG3 is inf)
    idx = np.r_[np.random.default_rng(3).choice(np.delete(np.arange(129), 9), size=32,
                                                replace=False), 9] if subset else None
    ev = GPUEvaluator(ps, SymbRegCaseAbsErrors(X, y, cases="device"), device=0)
    try:
        if subset:
            ev.subsample(idx)
        fit = ev.evaluate(trees)
        assert isinstance(fit[4], ValueError)
        with pytest.raises(ValueError) as raised:     # the first exception of the batch
            ev.select_dalex(trees, 5, 1.0)
        assert raised.value is fit[4]
        nan_row = ev.weighted_errors(np.ones(ev.spec.n_cases))
        assert np.isnan(nan_row[4]) and nan_row.shape == (len(trees),)
        keep = [t for t, f in zip(trees, fit) if not isinstance(f, BaseException)]
        E = np.asarray(host_matrix(ps, keep, X, y, idx), dtype=np.float64)
        # one tree per distinct row of errors: duplicates tie exactly, and the
        # criterion below needs selections the reference alone decides
        first = np.sort(np.unique(E, axis=0, return_index=True)[1])
        keep, E = [keep[i] for i in first], np.ascontiguousarray(E[first])
        rows = [tuple(r) for r in E.tolist()]
        n, C = E.shape
        assert C == (33 if subset else 129) and not ref.fit_rows(E).all()
        fit = ev.evaluate(keep)

        def lexicase():
            random.seed(8)
            return [id(t) for t in ev.select_lexicase(keep, 30, "epsilon", 0.5, parallel=True)]

        before = lexicase()
        assert ev.select_dalex(keep, 0, 1.0) == [] and ev.last_dalex_seed is None
        random.seed(21)
        picks = ev.select_dalex(keep, 300, 3.0)
        state = random.getstate()
        random.seed(21)
        seed = random.getrandbits(64)
        assert ev.last_dalex_seed == seed and random.getstate() == state   # the single draw
        got = [keep.index(t) for t in picks]
        assert got == ev.ctx.dalex(E, 300, seed, 3.0, True)[0].tolist()
        wt = ev.ctx.dalex_weights(C, 300, seed, 3.0, ev.ctx.dalex_sigma(E))
        ref.check(got, ref.scores(E, wt), seed, C)
        assert ref.fit_rows(E)[got].all()
        random.seed(21)                               # a seeded random reproduces the picks
        assert [keep.index(t) for t in ev.select_dalex(keep, 300, 3.0)] == got
        assert [keep.index(t) for t in ev.select_dalex(keep, 300, 3.0, standardize=False)] != got
        # weighted_errors is the store epilogue of the same product
        W = np.random.default_rng(9).random((17, C))
        sums = ev.weighted_errors(W)
        assert bits_equal(sums, ev.ctx.weighted_errors(E, W)) and sums.shape == (n, 17)
        assert np.array_equal(np.isnan(sums[:, 0]), ~ref.fit_rows(E))
        # nothing resident has moved
        assert lexicase() == before and repr(ev.evaluate(keep)) == repr(fit)   # (nan in it)
        # the drop-in on fitness tuples: the same values and seed, the same picks
        class Ind(object):
            def __init__(self, row):
                self.fitness = type("Fit", (), {"values": row, "weights": (-1.0,) * C,
                                                "wvalues": tuple(-v for v in row)})()
        inds = [Ind(r) for r in rows]
        random.seed(21)
        assert [inds.index(t) for t in tools.selDALexGPU(inds, 300, 3.0, device=0)] == got
        assert random.getstate() == state
    finally:
        ev.close()


# ------------------------------------------------------------- refusals --
def test_the_refusals_by_their_words(ctx):
    E = errors(0, 4, 3)
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.GpeError, match="no per-case values on the device"):
            fresh.dalex(None, 3, 1, 1.0)
        with pytest.raises(_lib.GpeError, match="no per-case values on the device"):
            fresh.dalex_sigma(None)
        with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs"):
            fresh.dalex_bits(None, 0, 0, 3, 1, 1.0)
    finally:
        fresh.close()
    out, failed = ctx.dalex(E, 0, 1, 1.0)
    assert out.shape == (0,) and failed == -1
    assert ctx.dalex_weights(3, 0, 1, 1.0).shape == (3, 0)
    with pytest.raises(_lib.GpeError, match=r"dalex: k selections = -1 \(need 0 \.\. 2\^31 - 1\)"):
        ctx.dalex(E, -1, 1, 1.0)
    with pytest.raises(_lib.GpeError, match=r"dalex: n = 0 individuals \(need 1 \.\. 2\^31 - 1\)"):
        ctx.dalex(np.zeros((0, 3)), 1, 1, 1.0)
    with pytest.raises(_lib.GpeError, match=r"dalex: n_cases = 0 \(need 1 \.\. 2\^31 - 1\)"):
        ctx.dalex(np.zeros((3, 0)), 1, 1, 1.0)
    with pytest.raises(_lib.GpeError, match=r"dalex_bits: n = 0 individuals"):
        ctx.dalex_bits(np.zeros((0, 1), dtype=np.uint32), 0, 3, 1, 1, 1.0)
    for bad in (-0.5, float("nan"), float("inf")):
        for call in (lambda: ctx.dalex(E, 1, 1, bad), lambda: ctx.dalex_weights(3, 1, 1, bad),
                     lambda: ctx.dalex_bits(np.zeros((4, 1), dtype=np.uint32), 4, 3, 1, 1, bad)):
            with pytest.raises(_lib.GpeError, match="pressure must be finite and >= 0"):
                call()
    with pytest.raises(_lib.GpeError, match=r"dalex_weights: n_cases = 0"):
        ctx.dalex_weights(0, 1, 1, 1.0)
    for w in ([1.0, -1.0, 0.0], [1.0, float("nan"), 0.0], [float("inf"), 1.0, 1.0]):
        with pytest.raises(ValueError, match="weighted_errors: every weight must be"):
            ctx.weighted_errors(E, w)
        bad = np.array([w])
        out = np.zeros((4, 1))
        rc = ctx.lib.gpe_weighted_errors(ctx.h, _lib._ptr(E), 4, 3, _lib._ptr(bad), 1,
                                         _lib._ptr(out))
        assert rc == _lib.GPE_E_ARG
        assert b"weighted_errors: every weight must be finite and >= 0" in \
            ctx.lib.gpe_last_error(ctx.h)
    rc = ctx.lib.gpe_weighted_errors(ctx.h, _lib._ptr(E), 4, 3, _lib._ptr(np.ones(3)), 0,
                                     _lib._ptr(np.zeros(4)))
    assert rc == _lib.GPE_E_INVALID and b"G = 0 weight rows" in ctx.lib.gpe_last_error(ctx.h)
    with pytest.raises(ValueError, match=r"weights must be float64 \[3\] or \[G, 3\]"):
        ctx.weighted_errors(E, np.ones(4))


def test_the_value_errors_of_the_evaluator():
    ps, trees, X, y = regression()
    good = [t for i, t in enumerate(trees[:40]) if i != 4]
    ev = GPUEvaluator(ps, SymbRegCaseAbsErrors(X, y, cases="device"), device=0)
    try:
        with pytest.raises(ValueError, match="select_dalex: this evaluator's last evaluate / "
                                             "map left no per-case matrix on the GPU"):
            ev.select_dalex(good, 3, 1.0)
        good = [t for t, f in zip(good, ev.evaluate(good)) if not isinstance(f, BaseException)]
        ev.evaluate(good)
        with pytest.raises(ValueError, match="select_dalex: individuals must be the batch of "
                                             "this evaluator's last evaluate / map"):
            ev.select_dalex(good[:-1], 3, 1.0)
        with pytest.raises(ValueError, match="select_dalex: individuals must be the batch"):
            ev.select_dalex(list(reversed(good)), 3, 1.0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="select_dalex: pressure must be finite and >= 0"):
                ev.select_dalex(good, 3, bad)
        with pytest.raises(ValueError, match="weighted_errors: every weight must be >= 0"):
            ev.weighted_errors(-np.ones(129))
        state = random.getstate()
        assert ev.select_dalex(good, 0, 1.0) == [] and random.getstate() == state
        assert len(ev.select_dalex(good, 7, 1.0)) == 7
    finally:
        ev.close()
    Xs, ys = X[:, :20].copy(), y[:20]
    Xs[3, 9] = 0.5
    ev = GPUEvaluator(ps, SymbRegMSE(Xs, ys), device=0)
    try:
        ev.evaluate(good)
        with pytest.raises(ValueError, match="select_dalex: this evaluator's last evaluate / "
                                             r"map left no per-case matrix on the GPU \(its spec "
                                             "is SymbRegMSE"):
            ev.select_dalex(good, 3, 1.0)
        with pytest.raises(ValueError, match="weighted_errors: this evaluator's last evaluate / "
                                             "map left no per-case errors"):
            ev.weighted_errors(np.ones(20))
    finally:
        ev.close()
