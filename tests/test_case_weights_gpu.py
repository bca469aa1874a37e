"""Case weights on the GPU: ``case_solve_counts`` and ``hit_weighted_sums``
on explicit planes against their host twins, bit for bit, at every row length
the kernels treat differently; the library's refusals; and
``GPUEvaluator.case_solve_counts`` / ``weighted_hits`` / ``shared_hits`` end
to end against the definitions of ``case_weights_ref`` on the boolean, the
typed and the regression machine, around exceptions, subsets and other
batches, with what they must leave undisturbed.

The sums kernel gives every row a wave whatever its length, so 64 and 65
words (2,048 and 2,049 cases) are one and two 64-word loads of the row; its
weights sit in LDS up to 64 KiB (8,192 doubles: G = 1 at 4,601 cases, not
G = 3) and are read through the caches beyond, as the 4.5 MB of the
(70, 70001) shape are.  The counts kernel shares a case between a power-of-two
group of lanes up to 64 words of 64 programs."""
import math
import random

import numpy as np
import pytest

import case_weights_ref as ref
from deap_amd import _lib, configs, datasets, gp
from deap_amd.evaluator import (BooleanCaseHits, GPUEvaluator, SymbRegCaseAbsErrors,
                                SymbRegCaseErrors, TypedBoolHits, TypedCaseHits,
                                TypedConfusion, pack_bitplanes, unpack_bitplanes)

pytestmark = pytest.mark.gpu

HIT_EPS = 0.25
_CACHE = {}


def random_words(rng, n, units):
    return rng.integers(0, 1 << 32, size=(n, units), dtype=np.uint64).astype(np.uint32)


def dyadic_weights(rng, G, n_cases):
    """Multiples of 2**-20 in [0, 1024], a fifth of them zero: every partial
    sum is representable, so any order gives fsum's bits."""
    w = rng.integers(0, (1 << 30) + 1, size=(G, n_cases)).astype(np.float64) / float(1 << 20)
    w[rng.random((G, n_cases)) < 0.2] = 0.0
    return w


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def twin_sums(planes, n_cases, w):
    """The host twin on any number of weight rows, in slices of 8."""
    return np.concatenate([_lib.host_hit_weighted_sums(planes, n_cases, w[s:s + 8])
                           for s in range(0, len(w), 8)], axis=1)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------ the kernels --
@pytest.mark.parametrize("n, n_cases, groups", [
    (1, 1, (1, 3, 8)),
    (65, 32, (1, 3, 8)), (1000, 33, (1, 3, 8)), (1000, 64, (1, 3, 8)),    # short rows, ragged wave
    (130, 2048, (1, 3, 8)), (130, 2049, (1, 3, 8)),           # 64 / 65 words: one / two row loads
    (130, 4601, (1, 3, 8)),                                   # 144 words: the lane-64 tail; G = 1 in LDS
    (70, 70001, (8,))])                                       # 4.5 MB of weights: past LDS
def test_the_kernels_give_what_the_host_twins_give(ctx, n, n_cases, groups):
    rng = np.random.default_rng(n * 100003 + n_cases)
    units = (n_cases + 31) // 32
    planes = random_words(rng, n, units)                      # (pad bits set)
    clean = planes.copy()
    if n_cases % 32:
        clean[:, -1] &= np.uint32((1 << (n_cases % 32)) - 1)
    pop = np.unpackbits(clean.view(np.uint8), axis=1).sum(1)
    counts = ctx.case_solve_counts(planes, n, n_cases)
    assert counts.dtype == np.int64 and counts.shape == (n_cases,)
    assert np.array_equal(counts, _lib.host_case_solve_counts(planes, n_cases))
    assert counts.sum() == pop.sum()
    for G in groups:
        w = rng.random((G, n_cases))
        if G > 1:
            w[1] = 0.0
            w[G - 1] = 1.0
        exp = _lib.host_hit_weighted_sums(planes, n_cases, w)
        got = ctx.hit_weighted_sums(planes, n, n_cases, w)
        assert got.dtype == np.float64 and got.shape == (n, G)
        assert bits_equal(got, exp), np.argwhere(got != exp)[:5]
        if G > 1:
            assert bits_equal(got[:, 1], np.zeros(n))         # (+0.0)
            assert np.array_equal(got[:, G - 1], pop.astype(np.float64))
    cnt, sh = ctx.hit_shared_sums(planes, n, n_cases)
    tcnt, tsh = _lib.host_hit_shared_sums(planes, n_cases)
    assert np.array_equal(cnt, tcnt) and np.array_equal(cnt, counts) and bits_equal(sh, tsh)
    assert ctx.case_weights_ms() >= 0.0


@pytest.mark.parametrize("n", [64, 65, 129, 4100])
def test_the_counts_under_a_live_mask(ctx, n):
    """W = 1, 2, 3 words of 64 programs with a ragged last word, and 65 words
    (a whole wave per case)."""
    rng = np.random.default_rng(n)
    for n_cases in (1, 33, 300):
        planes = random_words(rng, n, (n_cases + 31) // 32)
        alive = rng.random(n) < 0.6
        live = _lib.pack_live_mask(alive)
        if n % 64:
            live[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)     # (pad bits set)
        H = unpack_bitplanes(planes, n_cases)
        got = ctx.case_solve_counts(planes, n, n_cases, live=live)
        assert np.array_equal(got, H[alive].sum(0)), (n, n_cases)
        assert np.array_equal(got, _lib.host_case_solve_counts(planes, n_cases, live))
        cnt, sh = ctx.hit_shared_sums(planes, n, n_cases, live=live)
        tcnt, tsh = _lib.host_hit_shared_sums(planes, n_cases, live)
        assert np.array_equal(cnt, got) and np.array_equal(tcnt, got) and bits_equal(sh, tsh)
        ones = np.full((n + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        assert np.array_equal(ctx.case_solve_counts(planes, n, n_cases, live=ones), H.sum(0))


# ---------------------------------------------------------------- refusals --
def test_the_library_refuses_and_accepts_what_the_header_says(ctx):
    planes, w = np.zeros((3, 2), dtype=np.uint32), np.ones((9, 40))
    P = _lib._ptr
    out, cnt = np.zeros((3, 9)), np.zeros(40, dtype=np.int32)
    lib, ARG = ctx.lib, _lib.GPE_E_ARG
    sums, counts, shared = lib.gpe_hit_weighted_sums, lib.gpe_case_solve_counts, \
        lib.gpe_hit_shared_sums
    for call, args, text in (
            (sums, (P(planes), 3, 40, 0.0, P(w), 0, P(out)), b"G = 0 weight rows (need 1 .. 8)"),
            (sums, (P(planes), 3, 40, 0.0, P(w), 9, P(out)), b"G = 9 weight rows (need 1 .. 8)"),
            (sums, (P(planes), 3, 40, 0.0, None, 1, P(out)), b"hit_weighted_sums: weights is NULL"),
            (sums, (P(planes), 3, 40, 0.0, P(w), 1, None), b"hit_weighted_sums: out is NULL"),
            (sums, (P(planes), -1, 40, 0.0, P(w), 1, P(out)), b"hit_weighted_sums: n = -1 individuals"),
            (sums, (P(planes), 3, 0, 0.0, P(w), 1, P(out)), b"hit_weighted_sums: n_cases = 0 "),
            (sums, (P(planes), 3, 2 ** 31, 0.0, P(w), 1, P(out)),
             b"hit_weighted_sums: n_cases = 2147483648 "),
            (counts, (P(planes), 3, 40, 0.0, None, None), b"case_solve_counts: out_counts is NULL"),
            (counts, (P(planes), -1, 40, 0.0, None, P(cnt)), b"case_solve_counts: n = -1 individuals"),
            (counts, (P(planes), 3, 0, 0.0, None, P(cnt)), b"case_solve_counts: n_cases = 0 "),
            (counts, (P(planes), 2 ** 31, 40, 0.0, None, P(cnt)),
             b"case_solve_counts: n = 2147483648 individuals (the counts need n <= 2^31 - 1)"),
            (shared, (P(planes), 3, 40, 0.0, None, P(cnt), None), b"hit_shared_sums: out is NULL"),
            (shared, (P(planes), -1, 40, 0.0, None, P(cnt), P(out)), b"hit_shared_sums: n = -1 "),
            (shared, (P(planes), 3, 2 ** 31, 0.0, None, P(cnt), P(out)), b"hit_shared_sums: n_cases = "),
            (shared, (P(planes), 2 ** 31, 40, 0.0, None, P(cnt), P(out)),
             b"hit_shared_sums: n = 2147483648 individuals")):
        assert call(ctx.h, *args) == ARG, text
        assert text in lib.gpe_last_error(ctx.h), lib.gpe_last_error(ctx.h)
    for bad in (np.nan, np.inf, -1.0):
        wb = np.ones((1, 40))
        wb[0, 39] = bad
        assert sums(ctx.h, P(planes), 3, 40, 0.0, P(wb), 1, P(out)) == ARG
        assert b"every weight must be finite and >= 0" in lib.gpe_last_error(ctx.h)
    for G, text in ((0, "G = 0 weight rows"), (9, "G = 9 weight rows")):
        with pytest.raises(_lib.GpeError, match=text):
            ctx.hit_weighted_sums(planes, 3, 40, np.ones((G, 40)))
    # n == 0
    assert sums(ctx.h, P(planes), 0, 40, 0.0, P(w), 1, None) == 0
    cnt[:] = 5
    assert counts(ctx.h, P(planes), 0, 40, 0.0, None, P(cnt)) == 0 and not cnt.any()
    assert shared(ctx.h, P(planes), 0, 40, 0.0, None, None, None) == 0
    none = np.zeros((0, 2), dtype=np.uint32)
    assert ctx.hit_weighted_sums(none, 0, 40, w[:2]).shape == (0, 2)
    assert ctx.case_solve_counts(none, 0, 40).tolist() == [0] * 40
    assert ctx.hit_shared_sums(none, 0, 40)[1].shape == (0,)
    fresh = _lib.Context(0)
    try:
        for rc in (sums(fresh.h, None, 0, 0, 0.0, P(w), 1, P(out)),
                   counts(fresh.h, None, 0, 0, 0.0, None, P(cnt)),
                   shared(fresh.h, None, 0, 0, 0.0, None, P(cnt), P(out))):
            assert rc == -3                                    # GPE_E_STATE
            assert b"no hit planes of the loaded programs" in lib.gpe_last_error(fresh.h)
    finally:
        fresh.close()


# -------------------------------------------------------------- end to end --
def check_all(ev, H, live=None, eps=None, seed=0):
    """The three calls of *ev* on its resident matrix against the reference
    and the host twins on the reference matrix H (``bool[n, n_cases]``); *live*:
    who did not raise.  Returns what they gave."""
    n, n_cases = H.shape
    kw = {} if eps is None else {"eps": eps}
    rows = np.ones(n, dtype=bool) if live is None else live
    lv = None if live is None else live.tolist()
    mask = None if live is None else _lib.pack_live_mask(live)
    planes = pack_bitplanes(H)
    cnt = ev.case_solve_counts(**kw)
    assert cnt.dtype == np.int64 and cnt.tolist() == ref.solve_counts(H.tolist(), lv)
    rng = np.random.default_rng(1000 + n_cases + seed)
    out = [cnt]
    for w, exact in ((dyadic_weights(rng, 3, n_cases), True), (rng.random((9, n_cases)), False)):
        got = ev.weighted_hits(w, **kw)
        assert got.dtype == np.float64 and got.shape == (n, len(w))
        assert bits_equal(got[rows], twin_sums(planes, n_cases, w)[rows])
        assert np.isnan(got[~rows]).all()
        exp = np.array(ref.weighted_hits(H[rows].tolist(), w.tolist())).reshape(-1, len(w))
        if exact:
            assert bits_equal(got[rows], exp)
        else:
            assert (np.abs(got[rows] - exp) <= 1e-12 * exp).all()
        one = ev.weighted_hits(w[0].tolist(), **kw)            # 1-D weights
        assert one.shape == (n,) and np.array_equal(one, got[:, 0], equal_nan=True)
        out.append(got)
    sh = ev.shared_hits(**kw)
    s, exp = ref.shared_hits(H.tolist(), lv)
    assert ev.last_solve_counts.dtype == np.int64 and ev.last_solve_counts.tolist() == s
    assert cnt.tolist() == s
    exp = np.array(exp)
    tcnt, tsh = _lib.host_hit_shared_sums(planes, n_cases, mask)
    assert sh.dtype == np.float64 and sh.shape == (n,) and bits_equal(sh[rows], tsh[rows])
    assert np.isnan(sh[~rows]).all() and np.isnan(exp[~rows]).all()
    assert (np.abs(sh[rows] - exp[rows]) <= 1e-12 * exp[rows]).all()
    out.append(sh)
    return out


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and len(a) == len(b)


def boolean(name):
    if name not in _CACHE:
        ps = configs.pset_for(name)
        ins, outs = datasets.parity6_table() if name == "parity6" else datasets.mux11_table()
        pop = configs.population(ps, "half", 200 if name == "parity6" else 150, 11, 2, 5)
        _CACHE[name] = (ps, pop, ins, outs)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["parity6", "mux11"])
def test_the_boolean_machine(name):
    ps, pop, ins, outs = boolean(name)
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, "device"), device=0)
    try:
        ev.evaluate(pop)
        H = ev.last_case_hits()
        assert H.shape == (len(pop), ins.shape[1]) and 0.2 < H.mean() < 0.9
        check_all(ev, H)
        with pytest.raises(ValueError, match="eps applies to SymbRegCaseAbsErrors"):
            ev.shared_hits(eps=0.5)
    finally:
        ev.close()


def typed():
    """(pset, about 300 classifiers, X [57, 300], labels)."""
    if "typed" not in _CACHE:
        ps = configs.pset_for("spambase")
        X, lab = datasets.spambase_like(300, 57)
        trees = configs.population(ps, "half", 300, 57, 2, 4)
        hand = ["True", "False", "lt(IN0, IN1)", "and_(lt(IN3, IN4), not_(eq(IN5, IN6)))"]
        _CACHE["typed"] = (ps, trees + [gp.PrimitiveTree.from_string(s, ps) for s in hand], X, lab)
    return _CACHE["typed"]


@pytest.mark.parametrize("n_cases", [1, 2, 33, 64, 65, 129, 300])
def test_the_typed_machine(n_cases):
    ps, trees, X, lab = typed()
    got = []
    for spec in (TypedCaseHits(X[:, :n_cases], lab[:n_cases], "device"),
                 TypedConfusion(X[:, :n_cases], lab[:n_cases])):
        ev = GPUEvaluator(ps, spec, device=0)
        try:
            ev.evaluate(trees)
            H = ev.last_case_hits()
            assert H.shape == (len(trees), n_cases)
            got.append(check_all(ev, H))
        finally:
            ev.close()
    assert same(got[0], got[1])
    assert got[0][0].max() <= len(trees) and got[0][0].sum() > 0


def regression(n_cases):
    """(pset, trees, X [10, n_cases], y, P): small integers, so that many
    errors are exactly 0, 1, 2, ...; case 5's target is ARG0 + 0.25, an error
    of exactly HIT_EPS for the tree ``ARG0``; ARG3 is inf at case 9.
    ``sqrt(ARG0)`` raises where ARG0 < 0.  P: what every tree computes on every
    case (nan where it raises), from ``predict``."""
    key = ("reg", n_cases)
    if key not in _CACHE:
        ps = configs.pset_for("symreg10_sqrt")
        rng = np.random.default_rng(n_cases)
        X = rng.integers(-2, 3, (10, n_cases)).astype(np.float64)
        y = X[0] * X[1] + X[2]
        y[5] = X[0, 5] + HIT_EPS
        X[3, 9] = np.inf
        hand = ["ARG0", "ARG3", "sub(ARG3, ARG3)", "mul(ARG0, ARG1)", "add(mul(ARG0, ARG1), ARG2)",
                "sqrt(ARG0)", "add(ARG2, mul(ARG1, ARG0))"]
        trees = [gp.PrimitiveTree.from_string(s, ps) for s in hand] + \
            configs.population(ps, "half", 200, 23, 1, 4)
        ev = GPUEvaluator(ps, SymbRegCaseAbsErrors(X, y, hit_eps=HIT_EPS, cases="device"), device=0)
        try:
            P = ev.predict(trees, errors="nan")
        finally:
            ev.close()
        _CACHE[key] = (ps, trees, X, y, P)
    return _CACHE[key]


def threshold(P, y, eps):
    with np.errstate(invalid="ignore"):
        E = np.abs(P - y[None, :])
    return np.isfinite(E) & (E <= eps)


@pytest.mark.parametrize("n_cases", [127, 128, 129])
def test_the_regression_machine_thresholds_its_errors(n_cases):
    ps, trees, X, y, P = regression(n_cases)
    ev = GPUEvaluator(ps, SymbRegCaseAbsErrors(X, y, hit_eps=HIT_EPS, cases="device"), device=0)
    try:
        fit = ev.evaluate(trees)
        live = np.array([not isinstance(f, BaseException) for f in fit])
        assert isinstance(fit[5], ValueError) and live.sum() >= 10
        a = check_all(ev, threshold(P, y, HIT_EPS), live)               # the default eps
        b = check_all(ev, threshold(P, y, 1.0), live, eps=1.0)
        assert threshold(P, y, HIT_EPS)[0, 5] and not threshold(P, y, 0.0)[0, 5]
        assert not same(a[:1], b[:1])
        z = check_all(ev, threshold(P, y, 0.0), live, eps=0.0)
        assert z[0][5] < a[0][5]                                         # e == eps is a hit
        for eps in (-0.5, float("nan")):
            with pytest.raises(ValueError, match="eps must be >= 0"):
                ev.case_solve_counts(eps=eps)
            rc = ev.ctx.lib.gpe_case_solve_counts(ev.ctx.h, None, 0, 0, eps, None,
                                                  _lib._ptr(np.zeros(n_cases, dtype=np.int32)))
            assert rc == _lib.GPE_E_ARG
            assert b"case_solve_counts: eps must be >= 0" in ev.ctx.lib.gpe_last_error(ev.ctx.h)
        again = ev.evaluate(trees)
        assert all(type(p) is type(q) and (isinstance(p, BaseException) or
                                           np.array_equal(p, q, equal_nan=True))
                   for p, q in zip(fit, again))
    finally:
        ev.close()


# -------------------------------------------------- around the batch --
def test_a_too_tall_tree_gets_nan_and_is_not_counted():
    ps, pop, ins, outs = boolean("parity6")
    pop = list(pop[:70])
    pop[2] = gp.PrimitiveTree([ps.mapping["not_"]] * 201 + [ps.mapping["IN0"]])
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, "device"), device=0)
    try:
        fit = ev.evaluate(pop)
        assert isinstance(fit[2], SyntaxError) and type(fit[1]) is tuple
        live = np.ones(len(pop), dtype=bool)
        live[2] = False
        H = ev.last_case_hits()
        out = check_all(ev, H, live)
        assert out[0].tolist() == H[live].sum(0).tolist()
        assert ev.group_hits([[0, 1]])[2].tolist() == [-1]
    finally:
        ev.close()
    tps, trees, X, lab = typed()
    trees = list(trees[:70])
    trees[69] = gp.PrimitiveTree([tps.mapping["not_"]] * 201 +
                                 [tps.mapping["lt"], tps.mapping["IN0"], tps.mapping["IN1"]])
    ev = GPUEvaluator(tps, TypedCaseHits(X[:, :65], lab[:65], "device"), device=0)
    try:
        fit = ev.evaluate(trees)
        assert isinstance(fit[69], SyntaxError)
        live = np.ones(70, dtype=bool)
        live[69] = False
        check_all(ev, ev.last_case_hits(), live)
    finally:
        ev.close()


def test_a_subset_with_duplicates_is_a_fresh_evaluator_on_those_cases():
    ps, trees, X, lab = typed()
    rng = np.random.default_rng(40)
    idx = rng.integers(0, 300, size=40)
    idx[7] = idx[3]                                           # a duplicate for certain
    ev = GPUEvaluator(ps, TypedCaseHits(X, lab, "device"), device=0)
    try:
        ev.subsample(idx)
        ev.evaluate(trees)
        got = check_all(ev, ev.last_case_hits())
        assert len(got[0]) == 40
    finally:
        ev.close()
    fresh = GPUEvaluator(ps, TypedCaseHits(X[:, idx], lab[idx], "device"), device=0)
    try:
        fresh.evaluate(trees)
        assert same(got, check_all(fresh, fresh.last_case_hits()))
    finally:
        fresh.close()
    rps, rtrees, RX, ry, P = regression(129)
    ev = GPUEvaluator(rps, SymbRegCaseAbsErrors(RX, ry, hit_eps=HIT_EPS, cases="device"), device=0)
    try:
        ev.subsample(idx[:33] % 129)
        fit = ev.evaluate(rtrees)
        live = np.array([not isinstance(f, BaseException) for f in fit])
        sub = idx[:33] % 129
        got = check_all(ev, threshold(P[:, sub], ry[sub], HIT_EPS), live)
    finally:
        ev.close()
    fresh = GPUEvaluator(rps, SymbRegCaseAbsErrors(np.ascontiguousarray(RX[:, sub]), ry[sub],
                                                   hit_eps=HIT_EPS, cases="device"), device=0)
    try:
        fit = fresh.evaluate(rtrees)
        assert same(got, check_all(fresh, threshold(P[:, sub], ry[sub], HIT_EPS), live))
    finally:
        fresh.close()


def test_nothing_resident_is_disturbed():
    ps, trees, X, lab = typed()
    folds = [list(range(0, 100)), list(range(100, 300))]
    ev = GPUEvaluator(ps, TypedCaseHits(X, lab, "device"), device=0)
    try:
        fit = ev.evaluate(trees)
        H = ev.last_case_hits()

        def others():
            random.seed(77)
            picks = [id(t) for t in ev.select_lexicase(trees, 30)]
            random.seed(78)
            par = [id(t) for t in ev.select_lexicase(trees, 30, parallel=True)]
            random.seed(79)
            inf = ev.informed_subsample(20, apply=False).tolist()
            return picks, par, inf, ev.group_hits(folds).tolist(), ev.last_case_hits().tolist(), \
                ev.last_hits.tolist()

        before = others()
        state = random.getstate()
        check_all(ev, H)
        assert random.getstate() == state                     # nothing drawn from random
        assert others() == before
        assert ev.evaluate(trees) == fit
        # straight after an evaluation: the calls build the transpose themselves
        sh = ev.shared_hits()
        assert others() == before and np.array_equal(ev.shared_hits(), sh)
    finally:
        ev.close()
    rps, rtrees, RX, ry, P = regression(128)
    ev = GPUEvaluator(rps, SymbRegCaseAbsErrors(RX, ry, hit_eps=HIT_EPS, cases="device"), device=0)
    try:
        fit = ev.evaluate(rtrees)
        live = np.array([not isinstance(f, BaseException) for f in fit])
        keep = [t for t, ok in zip(rtrees, live) if ok]
        ev.evaluate(keep)

        def picks():
            random.seed(5)
            try:
                out = [id(t) for t in ev.select_lexicase(keep, 20, "epsilon", 0.5)]
            except IndexError as e:
                out = str(e)
            random.seed(6)
            return out, ev.informed_subsample(10, apply=False).tolist()

        before = picks()
        check_all(ev, threshold(P[live], ry, HIT_EPS))
        assert picks() == before
    finally:
        ev.close()


def test_the_value_errors_of_the_docstrings():
    ps, trees, X, lab = typed()
    few = trees[:10]
    ev = GPUEvaluator(ps, TypedCaseHits(X, lab, "device"), device=0)
    try:
        calls = (("case_solve_counts", lambda: ev.case_solve_counts()),
                 ("weighted_hits", lambda: ev.weighted_hits(np.ones(300))),
                 ("shared_hits", lambda: ev.shared_hits()))
        for name, call in calls:                              # before any evaluate
            with pytest.raises(ValueError, match=name + ": this evaluator's last evaluate / map "
                               "left no hit planes and no per-case absolute errors on the GPU"):
                call()
        ev.evaluate(trees)
        for name, call in calls:
            call()
        good = np.ones(300)
        for bad, text in ((np.ones(299), r"weights must be float64 \[300\] or \[G, 300\]"),
                          (np.ones((2, 2, 300)), "weights must be float64"),
                          (np.where(np.arange(300) == 3, np.nan, good), "finite"),
                          (np.where(np.arange(300) == 3, np.inf, good), "finite"),
                          (np.where(np.arange(300) == 3, -1e-300, good), ">= 0"),
                          (np.stack([good, np.full(300, 1e308)]), r"sum of weights\[1\] overflows")):
            with pytest.raises(ValueError, match="weighted_hits: .*" + text):
                ev.weighted_hits(bad)
        assert ev.weighted_hits(np.zeros((0, 300))).shape == (len(trees), 0)
        ev.prepare(ev.flatten(few), few)                      # another batch, loaded not run
        for name, call in calls:
            with pytest.raises(ValueError, match=name + ": the context now holds 10 programs, "
                               "not the %d" % len(trees)):
                call()
        with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs"):
            ev.ctx.hit_shared_sums(None, 0, 0)
    finally:
        ev.close()
    rps, rtrees, RX, ry, P = regression(127)
    for spec in (TypedBoolHits(X, lab), SymbRegCaseErrors(RX, ry)):
        ev = GPUEvaluator(ps if isinstance(spec, TypedBoolHits) else rps, spec, device=0)
        try:
            ev.evaluate(few if isinstance(spec, TypedBoolHits) else rtrees[:5])
            with pytest.raises(ValueError, match="shared_hits: .* left no hit planes and no "
                               "per-case absolute errors .*its spec is " + type(spec).__name__):
                ev.shared_hits()
        finally:
            ev.close()
    ev = GPUEvaluator(rps, SymbRegCaseAbsErrors(RX, ry, hit_eps=HIT_EPS, cases="device"), device=0)
    try:
        ev.evaluate(rtrees)
        ev.predict(rtrees[:10], errors="nan")                 # another batch
        with pytest.raises(ValueError, match="case_solve_counts: the context now holds 10"):
            ev.case_solve_counts()
        with pytest.raises(_lib.GpeError, match="another batch was loaded since the per-case run"):
            ev.ctx.case_solve_counts(None, 0, 0, HIT_EPS)
    finally:
        ev.close()
