"""``SymbRegAbsError`` without a GPU: the recorded reference of the GPU suite
recomputed on a sample, the host twin of the rows reduction
(``gpe_host_abserr``) against it, the spec's ``finish`` / ``finish_all`` on
synthetic words, what the spec refuses, and the ABI."""
import math
from fractions import Fraction

import numpy as np
import pytest

import abs_error_ref as ar
import scaled_ref as sr
from deap_amd import _lib, build, configs, distributed
from deap_amd.evaluator import GPUEvaluator, SymbRegAbsError

NONF, NAN, INF = (_lib.GPE_FLAG_NONFINITE_TERM, _lib.GPE_FLAG_NAN_TERM,
                  _lib.GPE_FLAG_INF_TERM)
OK = _lib.GPE_NO_ERROR
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def cells():
    if not _CACHE:
        ps, trees, n_base = ar.population()
        X, y = sr.data()
        key = sr.cells_key(trees, X, y)
        _CACHE.update(ps=ps, trees=trees, n_base=n_base, X=X, y=y, key=key,
                      gold={n: ar.load_golden(n, key) for n in ar.CASES})
    return _CACHE


def sample():
    """Every hand-written tree (scaled_ref's and this suite's) and every
    100th seeded one."""
    c = cells()
    return list(range(len(sr.HAND))) + list(range(len(sr.HAND), c["n_base"], 100)) + \
        list(range(c["n_base"], len(c["trees"])))


def test_the_recorded_reference_is_the_reference():
    """tests/golden/abs_error_n*.npz on the sample, recomputed from
    gp.compile's outputs (the 24,575-node tree on up to 257 cases)."""
    c = cells()
    trees, gold = c["trees"], c["gold"]
    assert all(g.shape == (len(trees), len(ar.FIELDS)) for g in gold.values())
    for i in sample():
        cases = ar.CASES if len(trees[i]) < 5000 else [n for n in ar.CASES if n <= 257]
        for n, rec in ar.reference(c["ps"], trees[i], c["X"], c["y"], cases).items():
            exp = gold[n][i]
            same = (np.array(rec) == exp) | (np.isnan(rec) & np.isnan(exp))
            assert same.all(), (i, n, rec, exp.tolist())


def test_the_hand_written_trees_pin_the_threshold():
    """The figures the definition gives for this suite's own trees."""
    c = cells()
    G = {n: {k: c["gold"][n][c["n_base"]:, j] for j, k in enumerate(ar.FIELDS)}
         for n in ar.CASES}
    for n in ar.CASES:
        g = G[n]
        assert g["mae"][0] == 0.0 and g["max"][0] == 0.0 and g["hits"][0] == n
        assert g["hits0"][0] == n
        assert g["hits"][1] == n and g["hits0"][1] == 0
    assert [G[n]["hits"][2] for n in (1, 2, 128, 10243)] == [0, 1, 33, 2706]
    assert [G[n]["hits"][3] for n in (1, 2, 128, 10243)] == [0, 1, 31, 2744]
    assert G[10243]["hits"][4] == 2588
    # finite and near 1e308 on every case: a value at n = 1, fsum's
    # OverflowError from n = 2
    assert G[1]["status"][5] == 0 and 9e307 < G[1]["mae"][5] < 1.1e308
    assert all(G[n]["status"][5] == ar.FSUM_OVERFLOW for n in ar.CASES if n > 1)
    # the population is not trivially all-zero: of scaled_ref's hand-written
    # trees and the first 300 seeded ones (316) on 1,000 cases, 289 have at
    # least one hit (282 of the 300 seeded)
    h = c["gold"][1000][:len(sr.HAND) + 300, ar.FIELDS.index("hits")]
    assert (h > 0).sum() == 289 and (h[len(sr.HAND):] > 0).sum() == 282
    # nan and inf cells exist (the inf column of the last case)
    g = c["gold"][10243]
    assert (g[:, ar.FIELDS.index("any_inf")] == 1).sum() > 20


@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])
def test_the_host_twin_against_the_reference(lib, n):
    """``gpe_host_abserr`` (the rows kernel's order) on the sample's per-case
    values: hits and max equal, the flags, the raw double-double sum within
    ``n 2**-100 sum e`` of the exact sum."""
    c = cells()
    gold = c["gold"][n]
    rows = list(zip(*c["X"][:, :n].tolist()))
    y = c["y"][:n]
    bound = Fraction(n, 2 ** 100)
    checked = 0
    for i in sample():
        if len(c["trees"][i]) >= 5000 and n > 257:
            continue
        g = dict(zip(ar.FIELDS, gold[i]))
        if g["status"] in (1, 2):
            continue                               # raises at a case: no values
        f, first, kind = sr.outputs(c["ps"], c["trees"][i], rows)
        assert first is None
        out4, flags = _lib.host_abserr(f, y, ar.HIT_EPS)
        assert bool(flags & NAN) == bool(g["any_nan"]), (i, flags)
        assert bool(flags & INF) == bool(g["any_inf"]), (i, flags)
        assert bool(flags & NONF) == bool(g["any_nan"] or g["any_inf"])
        if g["status"] == ar.FSUM_OVERFLOW:
            assert out4[0] == math.inf and not flags
            continue
        assert out4[3] == g["hits"], (i, out4, g)
        if g["any_nan"]:
            assert math.isnan(g["max"])
            continue
        assert out4[2] == g["max"], (i, out4, g)
        if g["any_inf"]:
            assert out4[0] == math.inf and g["mae"] == math.inf
            continue
        got = Fraction(float(out4[0])) + Fraction(float(out4[1]))
        exact = Fraction(g["Se_hi"]) + Fraction(g["Se_lo"])
        assert abs(got - exact) <= bound * exact, (i, float(got), float(exact))
        assert abs(out4[0] / n - g["mae"]) <= ar.TOL * g["mae"]
        # other thresholds: 0 counts the exact cases, inf every finite one
        assert _lib.host_abserr(f, y, 0.0)[0][3] == g["hits0"]
        assert _lib.host_abserr(f, y, math.inf)[0][3] == g["hits_finite"]
        checked += 1
    assert checked >= 25


def test_the_host_twin_with_two_term_columns_and_bad_arguments(lib):
    rng = np.random.default_rng(11)
    n = 700
    f = rng.normal(size=n)
    t = rng.normal(size=(2, n))
    f[5] = t[0, 5] + t[1, 5]                        # (not exactly 0 after two roundings,
    t[1, 6] = 0.0                                   #  unless the second term is 0)
    f[6] = t[0, 6]
    e = [abs(a - b - c) for a, b, c in zip(f.tolist(), t[0].tolist(), t[1].tolist())]
    mae, mx, hits = ar.figures(e, 0.25)
    out4, flags = _lib.host_abserr(f, t, 0.25)
    assert flags == 0 and out4[2] == mx and out4[3] == hits and e[6] == 0.0
    assert abs(out4[0] / n - mae) <= 1e-15 * mae
    for eps in (-1.0, math.nan):
        with pytest.raises(_lib.GpeError, match=r"\(-6\)"):
            _lib.host_abserr(f, t, eps)


# ------------------------------------------------------------- the spec --
def _spec(fitness=("mae",), n=8, **kw):
    rng = np.random.default_rng(6)
    return SymbRegAbsError(rng.uniform(-1, 1, (10, n)), rng.normal(size=n),
                           fitness=fitness, **kw)


WORDS = np.array([[4.0, 1e-17, 1.5, 3.0],            # 0 ordinary
                  [math.inf, 0.0, 1e308, 0.0],       # 1 finite terms, overflowing sum
                  [math.inf, 0.0, math.inf, 2.0],    # 2 an inf term
                  [math.nan, 0.0, 7.0, 1.0],         # 3 a nan term (the device max ignores it)
                  [math.nan, 0.0, math.inf, 1.0],    # 4 nan and inf terms
                  [1.0, 0.0, 1.0, 0.0],              # 5 a first error at case 3
                  [0.0, 0.0, 0.0, 8.0]])             # 6 the target itself
ERR = np.array([OK, OK, OK, OK, OK, (3 << 2) | _lib.GPE_ERR_VALUE, OK], dtype=np.uint64)
FLAGS = np.array([0, 0, NONF | INF, NONF | NAN, NONF | NAN | INF, 0, 0], dtype=np.uint32)


@pytest.mark.parametrize("fitness", [("mae",), ("max",), ("hits",), ("hits", "mae"),
                                     ("mae", "max", "hits"), ("max", "hits", "mae")])
def test_finish_and_finish_all_on_synthetic_words(fitness):
    spec = _spec(fitness)
    exp = [{"mae": 0.5, "max": 1.5, "hits": 3}, OverflowError,
           {"mae": math.inf, "max": math.inf, "hits": 2},
           {"mae": math.nan, "max": math.nan, "hits": 1},
           {"mae": math.nan, "max": math.nan, "hits": 1}, ValueError,
           {"mae": 0.0, "max": 0.0, "hits": 8}]
    both = [spec.finish_all(WORDS, None, ERR, FLAGS),
            [spec.finish(i, WORDS[i], 0.0, ERR[i], FLAGS[i]) for i in range(len(WORDS))]]
    for got in both:
        assert len(got) == len(exp)
        for r, e in zip(got, exp):
            if isinstance(e, type):
                assert isinstance(r, e), (r, e)
                continue
            assert isinstance(r, tuple) and len(r) == len(fitness)
            for name, v in zip(fitness, r):
                assert type(v) is (int if name == "hits" else float), (name, v)
                assert v == e[name] or (math.isnan(v) and math.isnan(e[name])), (name, v, e)
    assert str(both[0][1]) == "intermediate overflow in fsum"
    mae, mx, hits = spec.figures(WORDS, ERR, FLAGS)
    assert hits.dtype == np.int64 and mae.dtype == mx.dtype == np.float64
    assert hits.tolist() == [3, -1, 2, 1, 1, -1, 8]
    assert np.isnan(mae[[1, 3, 4, 5]]).all() and np.isnan(mx[[1, 3, 4, 5]]).all()


def test_the_spec_checks_its_arguments():
    for bad in ((), ("mse",), ("mae", "hit")):
        with pytest.raises(ValueError, match="fitness"):
            _spec(bad)
    for eps in (-0.01, math.nan):
        with pytest.raises(ValueError, match="hit_eps"):
            _spec(hit_eps=eps)
    s = _spec()
    assert s.hit_eps == 0.01 and s.fitness == ("mae",)
    assert _spec(hit_eps=math.inf).hit_eps == math.inf and _spec(hit_eps=0).hit_eps == 0.0
    two = SymbRegAbsError(np.zeros((2, 4)), np.zeros((3, 4)))
    assert two.terms.shape == (3, 4)
    import deap_amd.evaluator as evm
    assert "SymbRegAbsError" in evm.__all__


# -------------------------------------------------------------- refusals --
def test_fp32_is_refused():
    with pytest.raises(ValueError, match="SymbRegAbsError is fp64 only"):
        GPUEvaluator(configs.pset_for("symreg10"), _spec(), device=0, precision="fp32")


def test_a_numpy_semantics_set_is_refused():
    rng = np.random.default_rng(7)
    spec = SymbRegAbsError(rng.uniform(-1, 1, (1, 8)), rng.normal(size=8))
    with pytest.raises(NotImplementedError, match="SymbRegAbsError needs Python-semantics"):
        GPUEvaluator(configs.pset_for("symbreg_numpy"), spec, device=0)


def test_a_typed_set_is_refused():
    ps = configs.pset_for("spambase")
    rng = np.random.default_rng(8)
    spec = SymbRegAbsError(rng.uniform(0, 1, (len(ps.arguments), 8)), rng.normal(size=8))
    with pytest.raises(NotImplementedError,
                       match="SymbRegAbsError does not take a typed primitive set"):
        GPUEvaluator(ps, spec, device=0)


class _Local(object):
    def __init__(self):
        self.spec = _spec()


@pytest.mark.parametrize("wrap", [
    lambda loc: distributed.PopulationSharded(loc),
    lambda loc: distributed.CaseSharded(loc, 16, 0)])
def test_the_distributed_wrappers_refuse(wrap):
    with pytest.raises(NotImplementedError, match="SymbRegAbsError runs on one GPU"):
        wrap(_Local()).evaluate([])


# ------------------------------------------------------------------- ABI --
def test_the_abi_is_declared_bound_and_exported(lib):
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "gpeval.h")).read()
    P, I, I64, D = _lib._P, _lib._I, _lib._I64, __import__("ctypes").c_double
    want = {"gpe_run_abserr": [P, D, P, P, P],
            "gpe_run_abserr_device": [P, D, P, P, P],
            "gpe_host_abserr": [P, P, I64, I64, D, P, P]}
    ctype = {"double": D, "int64_t": I64, "int": I}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args)
        assert getattr(lib, name).argtypes == args
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, name
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        got = [P if "*" in a else ctype[a.rsplit(" ", 1)[0].strip()] for a in decl]
        assert got == args, (name, decl)
    for k, v in (("GPE_LAUNCH_ABSERR", 9), ("GPE_LAUNCH_ABSERR_DEEP", 10)):
        assert re.search(r"#define %s %d\b" % (k, v), header)
    assert _lib.Context.LAUNCHES.index("abserr") == 9
    assert _lib.Context.LAUNCHES.index("abserr_deep") == 10
    for m in ("run_abserr", "run_abserr_device"):
        assert callable(getattr(_lib.Context, m))
    assert "abserr.h" in build.LIB_HEADERS
