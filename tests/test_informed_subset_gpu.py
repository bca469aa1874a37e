"""Informed down-sampling on the GPU: ``gpe_informed_cases`` on host matrices
against the definition (``informed_ref``) at the case counts with a ragged last
word (whose pad rows must never be picked) and the program counts with ragged
64-program groups, and at 65,536 cases (more block partials than one pass
reduces); ``GPUEvaluator.informed_subsample`` on the resident hit planes of a
``BooleanCaseHits`` run and on the thresholded resident matrix of a
``SymbRegCaseAbsErrors`` run in both ``cases`` modes, with what it must leave
undisturbed; ``apply=True``; the library's refusals."""
import random

import numpy as np
import pytest

import informed_ref as ir
from deap_amd import _lib, configs, datasets, gp

pytestmark = pytest.mark.gpu

# (cases, programs), as the hit planes' own tests: 1, 33 and 513, 2049, 4097
# cases end in a partial 32-case word; 1, 63, 64, 65, 129 programs are one, one
# short of a 64-program group, a full one, one past, two and one
SHAPES = [(1, 129), (33, 63), (512, 64), (513, 65), (2049, 1), (4097, 65)]
SEEDS = (0x1234567, (1 << 64) - 1)
HIT_EPS = 0.25
_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, hit, m, seed, what):
    from deap_amd.evaluator import pack_bitplanes
    n, n_cases = hit.shape
    exp_idx, exp_dist = ir.informed_cases(hit, m, seed)
    idx, dist = ctx.informed_cases(pack_bitplanes(hit), n, n_cases, 0.0, seed, m)
    assert idx.dtype == np.int64 and dist.dtype == np.int32 and len(idx) == len(dist) == m
    assert idx.tolist() == exp_idx.tolist(), what
    assert dist.tolist() == exp_dist.tolist(), what
    assert idx.max() < n_cases and len(set(idx.tolist())) == m         # no pad row, no repeat


# ------------------------------------------------------ a host matrix --
@pytest.mark.parametrize("n_cases, n", SHAPES)
def test_host_planes_against_the_definition(ctx, n_cases, n):
    for t, (kind, hit) in enumerate(ir.matrices([(n_cases, n)], seed=n_cases)):
        for j, m in enumerate(sorted({min(k, n_cases) for k in (1, 2, 64, n_cases)})):
            check(ctx, hit, m, SEEDS[(t + j) % 2], (kind, n_cases, n, m))


def test_65536_cases_take_more_blocks_than_one_partials_pass(ctx):
    (_, hit), (_, equal) = ir.matrices([(65536, 130)], seed=65536)
    check(ctx, hit, 64, SEEDS[0], "mixed")
    check(ctx, equal, 64, SEEDS[1], "equal")
    # the winner's block is anywhere: the first pick is the smallest key (with
    # this seed case 63,785, past the first 1,024 cases: another seed moves it)
    key = ir.splitmix_keys_np(SEEDS[0], 65536)
    idx, _ = ctx.informed_cases(_planes(hit), 130, 65536, 0.0, SEEDS[0], 1)
    assert idx[0] == int(np.argmin(key)) and idx[0] >= 1024


def _planes(hit):
    from deap_amd.evaluator import pack_bitplanes
    return pack_bitplanes(hit)


# ------------------------------------------------------ resident, B machine --
def mux():
    """``(pset, population of 129, inputs, outputs)``, built as the hit planes'
    tests build theirs."""
    if "mux" not in _CACHE:
        ps = configs.pset_for("mux11")
        deep = configs.population(ps, "full", 2, 3, 7, 7)[1:]
        pop = deep + configs.population(ps, "half", 128, 17, 2, 6)
        ins, outs = datasets.mux11_table()
        _CACHE["mux"] = (ps, pop, ins, outs)
    return _CACHE["mux"]


@pytest.fixture(scope="module")
def mux_ev():
    from deap_amd.evaluator import BooleanCaseHits, GPUEvaluator
    ps, pop, ins, outs = mux()
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, "device"), device=0)
    yield ev
    ev.close()


def replayed_seed(state):
    twin = random.Random()
    twin.setstate(state)
    return twin.getrandbits(64), twin.getstate()


@pytest.mark.parametrize("m", [1, 33, 2048])
def test_the_resident_hit_planes(mux_ev, m):
    ps, pop, ins, outs = mux()
    ev = mux_ev
    ev.subsample(None)
    fit = ev.evaluate(pop)
    hit = ev.last_case_hits()
    assert hit.shape == (129, 2048) and 0.2 < hit.mean() < 0.9
    hits = ev.last_hits.copy()
    random.seed(50 + m)
    picks = [id(x) for x in ev.select_lexicase(pop, 30)]
    random.seed(70 + m)
    state = random.getstate()
    idx = ev.informed_subsample(m, apply=False)
    seed, after = replayed_seed(state)
    assert random.getstate() == after
    exp_idx, exp_dist = ir.informed_cases(hit, m, seed)
    assert idx.dtype == np.int64 and idx.tolist() == exp_idx.tolist()
    assert ev.last_informed_distances.tolist() == exp_dist.tolist()
    # nothing else moved
    assert ev.case_subset is None and ev.n_cases == 2048
    assert (ev.last_hits == hits).all() and (ev.last_case_hits() == hit).all()
    assert fit == [(int(h),) for h in hits]
    random.seed(50 + m)
    assert [id(x) for x in ev.select_lexicase(pop, 30)] == picks
    r1, r2 = random.Random(5), random.Random(5)            # the resident fitness
    a = ev.ctx.tournament(None, 50, 3, r1)
    ev.evaluate(pop)
    assert a.tolist() == ev.ctx.tournament(None, 50, 3, r2).tolist()


def test_apply_on_the_b_machine(mux_ev):
    from deap_amd.evaluator import BooleanCaseHits, GPUEvaluator
    ps, pop, ins, outs = mux()
    ev = mux_ev
    ev.subsample(None)
    ev.evaluate(pop[:40])                                  # the parent sample
    hit = ev.last_case_hits()
    random.seed(91)
    seed, _ = replayed_seed(random.getstate())
    idx = ev.informed_subsample(70)
    try:
        assert idx.tolist() == ir.informed_cases(hit, 70, seed)[0].tolist()
        assert ev.case_subset.tolist() == idx.tolist() and ev.n_cases == 70
        with pytest.raises(ValueError, match="left no per-case matrix on the GPU"):
            ev.select_lexicase(pop[:40], 3)
        with pytest.raises(ValueError, match=r"subsample\(None\) and evaluate the parent sample"):
            ev.informed_subsample(10)
        with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs"):
            ev.ctx.informed_cases(None, 0, 0, 0.0, 1, 3)   # (select_cases dropped them)
        fit = ev.evaluate(pop)
        fresh = GPUEvaluator(ps, BooleanCaseHits(ins[:, idx], outs[idx], "device"), device=0)
        try:
            assert fit == fresh.evaluate(pop)
            assert (ev.last_case_hits() == fresh.last_case_hits()).all()
        finally:
            fresh.close()
        assert len(ev.select_lexicase(pop, 5)) == 5
        with pytest.raises(ValueError, match=r"subsample\(None\) and evaluate the parent sample"):
            ev.informed_subsample(10)                      # a matrix, but of the subset
    finally:
        ev.subsample(None)


# ------------------------------------------------------ resident, F machine --
N_REG = 257
HAND = ["ARG0", "ARG3", "sub(ARG3, ARG3)", "mul(ARG0, ARG1)", "add(ARG0, 1)",
        "add(mul(ARG0, ARG1), ARG2)", "neg(ARG2)", "mul(ARG3, ARG4)"]


def regression():
    """``(pset, 48 trees without sin/cos, X [10, 257], y)``: small integers, so
    that many errors are exactly 0, 1, 2 ...; case 5's target is ARG0 + 0.25
    there, an error of exactly HIT_EPS for the tree ``ARG0``; ARG3 is inf at
    case 9 (errors inf, and nan from ARG3 - ARG3)."""
    if "reg" not in _CACHE:
        ps = configs.pset_for("symreg10_notrig")
        rng = np.random.default_rng(257)
        X = rng.integers(-2, 3, (10, N_REG)).astype(np.float64)
        y = X[0] * X[1] + X[2]
        y[5] = X[0, 5] + HIT_EPS
        X[3, 9] = np.inf
        trees = [gp.PrimitiveTree.from_string(s, ps) for s in HAND] + \
            configs.population(ps, "half", 40, 23, 1, 4)
        _CACHE["reg"] = (ps, trees, X, y)
    return _CACHE["reg"]


def reg_evaluator(cases, X=None, y=None):
    from deap_amd.evaluator import GPUEvaluator, SymbRegCaseAbsErrors
    ps, trees, X0, y0 = regression()
    spec = SymbRegCaseAbsErrors(X0 if X is None else X, y0 if y is None else y,
                                hit_eps=HIT_EPS, cases=cases)
    return GPUEvaluator(ps, spec, device=0)


def host_matrix():
    if "E" not in _CACHE:
        ps, trees, X, y = regression()
        ev = reg_evaluator("host")
        try:
            fit = ev.evaluate(trees)
        finally:
            ev.close()
        assert not any(isinstance(f, BaseException) for f in fit)
        E = np.array(fit, dtype=np.float64)
        assert E.shape == (len(trees), N_REG)
        assert E[0, 5] == HIT_EPS and np.isinf(E[1, 9]) and np.isnan(E[2, 9])
        assert (E == 0.0).any() and (E == HIT_EPS).sum() >= 1 and np.isnan(E).sum() >= 1
        _CACHE["E"] = E
    return _CACHE["E"]


def lexicase_outcome(ev, trees, seed):
    """25 epsilon-lexicase selections from the resident matrix: the picks and
    the ``random`` state after them, or the reference's IndexError (a leading
    candidate whose error at a case is nan leaves that case no survivor)."""
    random.seed(seed)
    try:
        return [id(x) for x in ev.select_lexicase(trees, 25, "epsilon", 0.5)], random.getstate()
    except IndexError as e:
        return str(e), random.getstate()


@pytest.mark.parametrize("cases", ["host", "device"])
def test_the_resident_errors_thresholded(cases):
    ps, trees, X, y = regression()
    E = host_matrix()
    ev = reg_evaluator(cases)
    try:
        fit = ev.evaluate(trees)
        picks = lexicase_outcome(ev, trees, 11)
        for j, (eps, m) in enumerate([(None, 40), (0.0, N_REG), (np.inf, 7), (1.0, 1)]):
            random.seed(20 + j)
            state = random.getstate()
            idx = ev.informed_subsample(m, eps=eps, apply=False)
            seed, after = replayed_seed(state)
            assert random.getstate() == after
            hit = ir.threshold(E, HIT_EPS if eps is None else eps)
            exp_idx, exp_dist = ir.informed_cases(hit, m, seed)
            assert idx.tolist() == exp_idx.tolist(), (cases, eps, m)
            assert ev.last_informed_distances.tolist() == exp_dist.tolist(), (cases, eps, m)
        # e == eps is a hit, a nan or inf never, also at eps = inf
        assert ir.threshold(E, HIT_EPS)[0, 5] and not ir.threshold(E, np.inf)[1:3, 9].any()
        assert ir.threshold(E, HIT_EPS)[0].sum() != ir.threshold(E, 0.0)[0].sum()
        # the matrix still serves selection, and the fitness is what it was
        assert lexicase_outcome(ev, trees, 11) == picks
        again = ev.evaluate(trees)
        assert np.array_equal(np.array(fit), np.array(again), equal_nan=True)
    finally:
        ev.close()


def test_apply_on_the_f_machine():
    ps, trees, X, y = regression()
    E = host_matrix()
    ev = reg_evaluator("host")
    try:
        ev.evaluate(trees[:30])
        random.seed(31)
        seed, _ = replayed_seed(random.getstate())
        idx = ev.informed_subsample(50)
        assert idx.tolist() == ir.informed_cases(ir.threshold(E[:30], HIT_EPS), 50, seed)[0].tolist()
        assert ev.case_subset.tolist() == idx.tolist() and ev.n_cases == 50
        with pytest.raises(ValueError, match="left no per-case matrix on the GPU"):
            ev.select_lexicase(trees[:30], 3)
        with pytest.raises(_lib.GpeError, match="no per-case values on the device"):
            ev.ctx.informed_cases(None, 0, 0, HIT_EPS, 1, 3)           # (stale)
        fit = ev.evaluate(trees)
        fresh = reg_evaluator("host", np.ascontiguousarray(X[:, idx]), y[idx])
        try:
            want = fresh.evaluate(trees)
        finally:
            fresh.close()
        assert np.array(fit).shape == (len(trees), 50)
        assert np.array_equal(np.array(fit), np.array(want), equal_nan=True)
        assert np.array_equal(np.array(fit), E[:, idx], equal_nan=True)
        assert lexicase_outcome(ev, trees, 12)[0]          # (a matrix is there again)
        with pytest.raises(ValueError, match=r"subsample\(None\) and evaluate the parent sample"):
            ev.informed_subsample(10)
    finally:
        ev.close()


# ------------------------------------------------------ the library's refusals --
def _refused(ctx, code, match, *args):
    with pytest.raises(_lib.GpeError, match=match) as info:
        ctx.informed_cases(*args)
    assert "(%d)" % code in str(info.value)


def test_the_library_refuses(mux_ev):
    from deap_amd.evaluator import pack_bitplanes
    ps, pop, ins, outs = mux()
    planes = pack_bitplanes(np.ones((3, 40), dtype=bool))
    c = mux_ev.ctx
    _refused(c, _lib.GPE_E_INVALID, "m = 0 ", planes, 3, 40, 0.0, 1, 0)
    _refused(c, _lib.GPE_E_INVALID, r"m = 41 \(need 1 .. n_cases = 40\)", planes, 3, 40, 0.0, 1, 41)
    out = (np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32))
    rc = c.lib.gpe_informed_cases(c.h, _lib._ptr(planes), 0, 40, 0.0, 1, 2, _lib._ptr(out[0]),
                                  _lib._ptr(out[1]))
    assert rc == _lib.GPE_E_INVALID and b"n = 0 individuals" in c.lib.gpe_last_error(c.h)
    mux_ev.subsample(None)
    mux_ev.evaluate(pop[:5])
    _refused(c, _lib.GPE_E_INVALID, "m = 0 ", None, 0, 0, 0.0, 1, 0)
    _refused(c, _lib.GPE_E_INVALID, "m = 2049 ", None, 0, 0, 0.0, 1, 2049)
    assert len(c.informed_cases(None, 0, 0, 0.0, 1, 2048)[0]) == 2048
    c.select_cases(np.arange(100))                         # the planes are the full set's
    try:
        _refused(c, -3, "no hit planes of the loaded programs", None, 0, 0, 0.0, 1, 5)
    finally:
        c.select_cases(None)
    _refused(c, -3, "no hit planes of the loaded programs", None, 0, 0, 0.0, 1, 5)
    # the F machine: nothing resident, a bad eps, a stale matrix
    ps, trees, X, y = regression()
    ev = reg_evaluator("device")
    try:
        fc = ev.ctx
        _refused(fc, -3, "no per-case values on the device", None, 0, 0, HIT_EPS, 1, 5)
        ev.evaluate(trees)
        for eps in (-0.5, float("nan")):
            _refused(fc, _lib.GPE_E_ARG, "eps must be >= 0", None, 0, 0, eps, 1, 5)
        _refused(fc, _lib.GPE_E_INVALID, "m = 258 ", None, 0, 0, HIT_EPS, 1, N_REG + 1)
        assert len(fc.informed_cases(None, 0, 0, HIT_EPS, 1, 5)[0]) == 5
        ev.predict(trees[:10], errors="nan")               # another batch: the matrix has 48 rows
        _refused(fc, -3, "another batch was loaded since the per-case run", None, 0, 0, HIT_EPS,
                 1, 5)
        ev.evaluate(trees)
        assert len(fc.informed_cases(None, 0, 0, HIT_EPS, 1, 5)[0]) == 5
        fc.select_cases(np.arange(20))
        _refused(fc, -3, "no per-case values on the device", None, 0, 0, HIT_EPS, 1, 5)
        fc.select_cases(None)
        _refused(fc, -3, "no per-case values on the device", None, 0, 0, HIT_EPS, 1, 5)
    finally:
        ev.close()
