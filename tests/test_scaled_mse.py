"""``SymbRegScaledMSE`` without a GPU: the host twin of the formula the device
applies (``gpe_host_scaled_from_moments``) against the exact-rational
reference (``scaled_ref``) on moments built exactly from random data, the
ABI, what the spec refuses, its exact target sums, and the recorded reference
of the GPU suite recomputed on a sample."""
import math
from fractions import Fraction

import numpy as np
import pytest

import scaled_ref as sr
from deap_amd import _lib, build, configs, distributed
from deap_amd.evaluator import (GPUEvaluator, SymbRegMSE, SymbRegScaledMSE,
                                exact_dd_sums)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _moments(f, y):
    """The exact moments of f against y as the six words of a moments run."""
    Sf, Sff, Sfy = sr.exact_sum(f.tolist()), sr.exact_dot(f, f), sr.exact_dot(f, y)
    return [w for S in (Sf, Sff, Sfy) for w in sr.dd(S)]


def _target(rng, n):
    y = rng.normal(0.0, 1.5, n)
    return y - (y.mean() if n > 2 else 0.0)


def _host(f, y, flags=None):
    n = len(y)
    m6 = [0.0] * 6 if flags else _moments(f, y)
    mse, a, b = _lib.host_scaled_from_moments(
        [m6], n, sr.dd(sr.exact_sum(y.tolist())), sr.dd(sr.exact_dot(y, y)),
        None if flags is None else [flags])
    return float(mse[0]), float(a[0]), float(b[0])


def _check(f, y, flags=None):
    """The host twin within the tolerances of ``scaled_ref.record`` (which
    asserts the conditioning of its own numbers first); returns both."""
    ref = dict(zip(sr.FIELDS, sr.record(f, y)))
    got = _host(f, y, flags)
    assert bool(ref["flagged"]) == bool(flags)
    if ref["flagged"]:
        assert got[0] == math.inf and got[2] == 0.0
    else:
        assert abs(got[0] - ref["mse"]) <= ref["tol_mse"], (got, ref)
    assert abs(got[1] - ref["a"]) <= ref["tol_a"], (got, ref)
    assert abs(got[2] - ref["b"]) <= ref["tol_b"], (got, ref)
    return got, ref


@pytest.mark.parametrize("n", [3, 64, 1000, 4097])
def test_ordinary_programs(lib, n):
    rng = np.random.default_rng(n)
    y = _target(rng, n)
    for k in range(20):
        f = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-3, 4) + \
            rng.uniform(-0.9, 0.9) * y + rng.normal()
        got, ref = _check(f, y)
        assert ref["tol_b"] > 0.0 and got[0] > 0.0


def test_a_constant_has_the_targets_variance(lib):
    rng = np.random.default_rng(1)
    y = _target(rng, 500)
    got, ref = _check(np.full(500, 3.25), y)
    vy_n = float((sr.exact_dot(y, y) - sr.exact_sum(y.tolist()) ** 2 / 500) / 500)
    assert got[2] == 0.0 and abs(got[0] - vy_n) <= 1e-12 * vy_n
    assert abs(got[1] - float(sr.exact_sum(y.tolist()) / 500)) <= ref["tol_a"]
    _check(np.zeros(500), y)


def test_an_exact_affine_image_fits(lib):
    rng = np.random.default_rng(2)
    y = np.round(_target(rng, 300) * 1024.0) / 1024.0      # few bits: 4 y + 1 exact
    f = 4.0 * y + 1.0
    got, ref = _check(f, y)
    assert ref["mse"] == 0.0
    vy_n = float((sr.exact_dot(y, y) - sr.exact_sum(y.tolist()) ** 2 / 300) / 300)
    assert 0.0 <= got[0] <= 1e-12 * vy_n
    assert abs(got[2] - 0.25) <= 1e-12 and abs(got[1] + 0.25) <= 1e-12


def test_an_anticorrelated_program_has_a_negative_slope(lib):
    rng = np.random.default_rng(3)
    y = _target(rng, 777)
    got, ref = _check(-2.0 * y + 0.01 * rng.normal(size=777), y)
    assert got[2] < 0.0 and abs(got[2] + 0.5) < 1e-2


def test_one_and_two_cases(lib):
    got, ref = _check(np.array([1.75]), np.array([-0.5]))
    assert got == (0.0, -0.5, 0.0)                        # n = 1: a constant, no error
    got, ref = _check(np.array([1.0, 3.0]), np.array([-0.5, 0.75]))
    assert got[0] == 0.0 and ref["mse"] == 0.0            # two points: a line through both
    assert abs(got[2] - 0.625) <= 1e-15 and abs(got[1] + 1.125) <= 1e-15
    got, ref = _check(np.array([2.0, 2.0]), np.array([-0.5, 0.75]))
    assert got[2] == 0.0 and got[0] == ref["mse"] == 0.390625


def test_the_flag_gives_inf_and_the_targets_mean(lib):
    rng = np.random.default_rng(4)
    y = _target(rng, 200)
    f = rng.normal(size=200)
    f[17] = 2.0 ** 500
    got, ref = _check(f, y, flags=_lib.GPE_FLAG_MOMENT_RANGE)
    assert got[0] == math.inf and got[2] == 0.0 and got[1] == ref["a"]
    f[17] = math.nan
    _check(f, y, flags=_lib.GPE_FLAG_MOMENT_RANGE)
    f[17] = 2.0 ** 499                # below the bound: Sff near 2**998, no flag
    got, ref = _check(f, y)
    assert not ref["flagged"] and math.isfinite(got[0])


def test_conditioning_inside_and_far_outside_the_threshold(lib):
    """Sff / (n vf) just under 2**20: fitted; 2**62: constant by the rule."""
    rng = np.random.default_rng(5)
    n = 1024
    y = _target(rng, n)
    u = 0.5 * y + rng.normal(size=n)
    u = (u - u.mean()) / u.std()
    f = u + 2.0 ** 14.9
    got, ref = _check(f, y)
    cond = sr.exact_dot(f, f) / (n * (sr.exact_dot(f, f) - sr.exact_sum(f.tolist()) ** 2 / n))
    assert 2 ** 19 < cond < 2 ** 20 and ref["b"] != 0.0 and got[2] != 0.0
    f = u + 2.0 ** 36
    got, ref = _check(f, y)
    cond = sr.exact_dot(f, f) / (n * (sr.exact_dot(f, f) - sr.exact_sum(f.tolist()) ** 2 / n))
    assert cond > 2 ** 60 and ref["b"] == 0.0 and got[2] == 0.0
    assert abs(got[0] - ref["mse"]) <= 1e-12 * ref["mse"]


def test_the_abi_is_declared_bound_and_exported(lib):
    for name in ("gpe_run_moments", "gpe_run_scaled", "gpe_run_scaled_device",
                 "gpe_host_scaled_from_moments"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert _lib.GPE_FLAG_MOMENT_RANGE == 8 and _lib.GPE_E_ARG == -6
    for m in ("run_moments", "run_scaled", "run_scaled_device"):
        assert callable(getattr(_lib.Context, m))


# -------------------------------------------------------------- refusals --
def _spec(n=8):
    rng = np.random.default_rng(6)
    return SymbRegScaledMSE(rng.uniform(-1, 1, (10, n)), rng.normal(size=n))


def test_fp32_is_refused():
    with pytest.raises(ValueError, match="fp64 only"):
        GPUEvaluator(configs.pset_for("symreg10"), _spec(), device=0, precision="fp32")


def test_a_numpy_semantics_set_is_refused():
    rng = np.random.default_rng(7)
    spec = SymbRegScaledMSE(rng.uniform(-1, 1, (1, 8)), rng.normal(size=8))
    with pytest.raises(NotImplementedError, match="numpy-semantics"):
        GPUEvaluator(configs.pset_for("symbreg_numpy"), spec, device=0)


def test_a_typed_set_is_refused():
    ps = configs.pset_for("spambase")
    rng = np.random.default_rng(8)
    spec = SymbRegScaledMSE(rng.uniform(0, 1, (len(ps.arguments), 8)), rng.normal(size=8))
    with pytest.raises(NotImplementedError, match="typed primitive set"):
        GPUEvaluator(ps, spec, device=0)


class _Local(object):
    def __init__(self):
        self.spec = _spec()


@pytest.mark.parametrize("wrap", [
    lambda loc: distributed.PopulationSharded(loc),
    lambda loc: distributed.CaseSharded(loc, 16, 0)])
def test_the_distributed_wrappers_refuse(wrap):
    with pytest.raises(NotImplementedError, match="one GPU"):
        wrap(_Local()).evaluate([])


def test_two_target_columns_are_refused():
    with pytest.raises(ValueError, match="one target column"):
        SymbRegScaledMSE(np.zeros((2, 4)), np.zeros((2, 4)))


def test_predict_scaled_needs_the_scaled_spec():
    ev = GPUEvaluator.__new__(GPUEvaluator)          # (no device context needed)
    ev.spec = SymbRegMSE(np.zeros((1, 4)), np.zeros(4))
    with pytest.raises(ValueError, match="SymbRegScaledMSE"):
        ev.predict([], scaled=True)


# ------------------------------------------------------ exact target sums --
def test_the_targets_sums_are_exact():
    """A column whose left-to-right sum (and numpy's pairwise one) is wrong
    in the last bits, and whose squares do not fit a double."""
    rng = np.random.default_rng(9)
    y = np.concatenate([rng.normal(size=4000) * 1e8, rng.normal(size=4000) * 1e-8,
                        [1e16, 1.0, -1e16, 3.0 ** -20]])
    rng.shuffle(y)
    Sy = sum(map(Fraction, y.tolist()))
    Syy = sum(Fraction(v) ** 2 for v in y.tolist())
    naive = 0.0
    for v in y.tolist():
        naive += v
    assert naive != float(Sy) and float(np.sum(y)) != float(Sy)
    spec = SymbRegScaledMSE(np.zeros((1, len(y))), y)
    assert spec.sy == sr.dd(Sy) and spec.syy == sr.dd(Syy)
    assert spec.terms.shape == (1, len(y))
    # magnitudes past the exact product's range take the rational path
    y = np.array([2.0 ** 450, -2.0 ** 450 + 2.0 ** 400, 3.0 ** -300, 0.1])
    sy, syy = exact_dd_sums(y)
    assert sy == sr.dd(sum(map(Fraction, y.tolist())))
    assert syy == sr.dd(sum(Fraction(v) ** 2 for v in y.tolist()))
    with pytest.raises(ValueError, match="finite"):
        exact_dd_sums(np.array([1.0, math.inf]))


# ------------------------------------------------- the recorded reference --
def test_the_recorded_reference_is_the_reference():
    """tests/golden/scaled_mse_n*.npz on every hand-written tree and every
    100th seeded one, recomputed from gp.compile's outputs (the 24,575-node
    tree of the rows route on up to 257 cases: it takes 2 ms per case)."""
    ps, trees = sr.population()
    X, y = sr.data()
    key = sr.cells_key(trees, X, y)
    gold = {n: sr.load_golden(n, key) for n in sr.CASES}
    assert all(g.shape == (len(trees), len(sr.FIELDS)) for g in gold.values())
    pick = list(range(len(sr.HAND))) + list(range(len(sr.HAND), len(trees), 100))
    for i in pick:
        cases = sr.CASES if len(trees[i]) < 5000 else [n for n in sr.CASES if n <= 257]
        for n, rec in sr.reference(ps, trees[i], X, y, cases).items():
            exp = gold[n][i]
            same = (np.array(rec) == exp) | (np.isnan(rec) & np.isnan(exp))
            assert same.all(), (i, n, rec, exp.tolist())
    st = gold[10243][:, 0]
    assert (st == 1).sum() > 100 and (gold[10243][:, 2] == 1).sum() > 100   # the inf case
    assert (gold[10240][:len(sr.HAND), 0] == [0, 0, 0, 0, 0, 0, 1, 1, 0, 2, 0, 0, 0, 0, 0,
                                              0]).all()
