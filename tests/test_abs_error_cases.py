"""``SymbRegCaseAbsErrors`` without a GPU: the host twin of the per-case value
(``gpe_host_abserr_cases``) against Python's ``abs(f - t0 - t1)`` on IEEE edge
operands, a sample of the GPU suite's population whose rows must sum to the
recorded ``mae``, the spec's ``finish`` / ``finish_all`` in both ``cases=``
modes, what it refuses, ``select_lexicase``'s checks on a stub context, and
the ABI."""
import math
import random

import numpy as np
import pytest

import abs_error_ref as ar
import predict_ref as pr
import scaled_ref as sr
from deap_amd import _lib, build, configs, distributed
from deap_amd.evaluator import (GPUEvaluator, SymbRegAbsError, SymbRegCaseAbsErrors,
                                SymbRegCaseErrors)

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
        _CACHE.update(ps=ps, trees=trees, n_base=n_base, X=X, y=y,
                      key=sr.cells_key(trees, X, y))
    return _CACHE


def sample():
    """The six EXTRA trees, scaled_ref's hand-written ones and every 64th of
    the seeded ones."""
    c = cells()
    return list(range(c["n_base"], len(c["trees"]))) + list(range(len(sr.HAND))) + \
        list(range(len(sr.HAND), c["n_base"], 64))


# --------------------------------------------------------- the host twin --
SUB = 5e-324
EDGES = [0.0, -0.0, SUB, -SUB, 2.5e-310, -2.5e-310, 2.2250738585072014e-308, 1.0, -1.0,
         0.1, 1e308, -1e308, 1.7976931348623157e308, -1.7976931348623157e308,
         math.inf, -math.inf, math.nan, -math.nan]


def test_the_host_twin_on_ieee_edge_operands(lib):
    """Every pair (and triple) of ±0.0, subnormals, ±1e308 and ±max (whose
    differences overflow), ±inf (``inf - inf``) and a nan of either sign,
    against Python's own ``abs(f - t0 - t1)``: equal bits, any nan for a
    nan."""
    assert math.copysign(1.0, EDGES[-1]) == -1.0 and math.copysign(1.0, EDGES[-2]) == 1.0
    f1, t1 = zip(*[(a, b) for a in EDGES for b in EDGES])
    exp1 = np.array([abs(a - b) for a, b in zip(f1, t1)])
    got1 = _lib.host_abserr_cases(np.array(f1), np.array(t1))
    pr.assert_same_bits(got1, exp1, "one term column")
    f2, t2a, t2b = zip(*[(a, b, c) for a in EDGES for b in EDGES for c in EDGES])
    exp2 = np.array([abs(a - b - c) for a, b, c in zip(f2, t2a, t2b)])
    got2 = _lib.host_abserr_cases(np.array(f2), np.array([t2a, t2b]))
    pr.assert_same_bits(got2, exp2, "two term columns")
    # what the table holds: zeros of the absolute value are +0.0, inf - inf is
    # nan, 1e308 - -1e308 is inf, a subnormal difference stays exact
    k = {v: i for i, v in enumerate(EDGES[:16])}
    n = len(EDGES)
    assert math.copysign(1.0, got1[k[-0.0] * n + k[0.0]]) == 1.0
    assert math.isnan(got1[k[math.inf] * n + k[math.inf]])
    assert got1[k[1e308] * n + k[-1e308]] == math.inf
    assert got1[k[SUB] * n + k[-SUB]] == 2 * SUB
    assert np.isnan(got1[-2 * n:]).all() and np.isnan(got1[n - 2::n]).all()
    # left to right: (-max - max) - -max is inf, where -max - (max + -max)
    # would be max
    m = 1.7976931348623157e308
    assert _lib.host_abserr_cases(np.array([-m]), np.array([[m], [-m]]))[0] == math.inf


def test_the_host_twin_refuses_bad_arguments(lib):
    f = np.zeros(4)
    out = np.zeros(4)
    P = _lib._ptr
    assert lib.gpe_host_abserr_cases(None, P(f), 1, 4, P(out)) == _lib.GPE_E_INVALID
    assert lib.gpe_host_abserr_cases(P(f), None, 1, 4, P(out)) == _lib.GPE_E_INVALID
    assert lib.gpe_host_abserr_cases(P(f), P(f), -1, 4, P(out)) == _lib.GPE_E_INVALID
    assert lib.gpe_host_abserr_cases(P(f), P(f), 1, 0, P(out)) == _lib.GPE_E_INVALID
    assert lib.gpe_host_abserr_cases(P(f), P(f), 1, 4, None) == _lib.GPE_E_INVALID
    # no term column at all: |f|
    f = np.array([-1.5, 0.0, -0.0, math.inf])
    assert lib.gpe_host_abserr_cases(P(f), None, 0, 4, P(out)) == 0
    assert out.tolist() == [1.5, 0.0, 0.0, math.inf]
    with pytest.raises(ValueError):
        _lib.host_abserr_cases(np.zeros(3), np.zeros((1, 4)))


@pytest.mark.parametrize("n", [129, 257])
def test_rows_of_the_sample_sum_to_the_recorded_mae(lib, n):
    """The rows a cases run must produce, from ``gp.compile``'s outputs through
    the host twin: equal to Python's ``abs(f - y)`` bit for bit, and
    ``math.fsum(row) / n`` equal to the ``mae`` recorded in
    tests/golden/abs_error_n*.npz wherever that record holds a value."""
    c = cells()
    gold = ar.load_golden(n, c["key"])
    rows = list(zip(*c["X"][:, :n].tolist()))
    y = c["y"][:n]
    values = 0
    for i in sample():
        g = dict(zip(ar.FIELDS, gold[i]))
        f, first, kind = sr.outputs(c["ps"], c["trees"][i], rows)
        if g["status"] in (1, 2):
            assert first == g["first"] and sr.STATUS[kind] == g["status"]
            continue
        assert first is None
        e = _lib.host_abserr_cases(f, y)
        pr.assert_same_bits(e, np.array([abs(a - b) for a, b in zip(f.tolist(), y.tolist())]),
                            "tree %d" % i)
        if g["status"] == ar.FSUM_OVERFLOW:
            with pytest.raises(OverflowError):
                math.fsum(e.tolist())
            continue
        mae = math.fsum(e.tolist()) / n
        assert pr.same_bits(np.array([mae]), np.array([g["mae"]])).all(), (i, mae, g["mae"])
        values += 1
    assert values >= 40


# ------------------------------------------------------------- the spec --
def _spec(cases="host", fitness=("mae",), n=3, cls=SymbRegCaseAbsErrors, **kw):
    rng = np.random.default_rng(6)
    if cls is SymbRegCaseAbsErrors:
        kw["cases"] = cases
    return cls(rng.uniform(-1, 1, (10, n)), rng.normal(size=n), fitness=fitness, **kw)


WORDS = np.array([[4.5, 1e-17, 3.0, 1.0],            # 0 ordinary
                  [math.inf, 0.0, 1e308, 0.0],       # 1 finite terms, overflowing sum
                  [math.inf, 0.0, math.inf, 2.0],    # 2 an inf term
                  [math.nan, 0.0, 7.0, 1.0],         # 3 a nan term
                  [1.0, 0.0, 1.0, 0.0],              # 4 a first error at case 1
                  [0.0, 0.0, 0.0, 3.0]])             # 5 the target itself
ROWS = np.array([[0.5, 3.0, 1.0], [1e308, 1e308, 1e308], [math.inf, 0.0, 0.0],
                 [math.nan, 7.0, 0.0], [1.0, math.nan, math.nan], [0.0, 0.0, 0.0]])
ERR = np.array([OK, OK, OK, OK, (1 << 2) | _lib.GPE_ERR_VALUE, OK], dtype=np.uint64)
FLAGS = np.array([0, 0, NONF | INF, NONF | NAN, 0, 0], dtype=np.uint32)


def _same_result(r, e):
    if isinstance(e, type):
        return isinstance(r, e)
    return type(r) is tuple and len(r) == len(e) and all(
        type(a) is type(b) and (a == b or (a != a and b != b)) for a, b in zip(r, e))


@pytest.mark.parametrize("fitness", [("mae",), ("hits", "mae")])
def test_finish_and_finish_all_in_both_modes(fitness):
    """``cases="host"``: the row as a tuple of floats; ``cases="device"``:
    the summary tuple of SymbRegAbsError.  The exceptions are SymbRegAbsError's
    in both, fsum's overflow included whatever the fitness names."""
    plain = _spec(cls=SymbRegAbsError, fitness=fitness)
    summary = plain.finish_all(WORDS, None, ERR, FLAGS)
    host, dev = _spec("host", fitness), _spec("device", fitness)
    exp_host = [tuple(r) for r in ROWS.tolist()]
    for i in (1, 4):
        exp_host[i] = type(summary[i])
    assert isinstance(summary[1], OverflowError) and isinstance(summary[4], ValueError)
    got = {"host all": host.finish_all(WORDS, None, ERR, FLAGS, cases=ROWS),
           "host one": [host.finish(i, WORDS[i], 0.0, ERR[i], FLAGS[i], ROWS[i])
                        for i in range(len(WORDS))],
           "dev all": dev.finish_all(WORDS, None, ERR, FLAGS, cases=None),
           "dev all 4": dev.finish_all(WORDS, None, ERR, FLAGS),
           "dev one": [dev.finish(i, WORDS[i], 0.0, ERR[i], FLAGS[i])
                       for i in range(len(WORDS))]}
    for name, res in got.items():
        exp = exp_host if name.startswith("host") else \
            [type(s) if isinstance(s, BaseException) else s for s in summary]
        assert len(res) == len(exp)
        for i, (r, e) in enumerate(zip(res, exp)):
            assert _same_result(r, e), (name, i, r, e)
    assert str(got["host all"][1]) == "intermediate overflow in fsum"
    assert str(got["host all"][4]) == "math domain error"
    assert all(type(v) is float for v in got["host all"][0])
    # the three figures are SymbRegAbsError's
    for a, b in zip(host.figures(WORDS, ERR, FLAGS), plain.figures(WORDS, ERR, FLAGS)):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def test_the_spec_checks_its_arguments():
    s = SymbRegCaseAbsErrors(np.zeros((2, 4)), np.zeros((3, 4)))
    assert s.cases == "host" and s.hit_eps == 0.01 and s.fitness == ("mae",)
    assert s.terms.shape == (3, 4) and s.abs_error and s.abs_cases
    assert isinstance(s, SymbRegAbsError) and not getattr(s, "per_case", False)
    for bad in ("gpu", None, "Host"):
        with pytest.raises(ValueError, match="cases must be 'host' or 'device'"):
            _spec(bad)
    with pytest.raises(ValueError, match="fitness"):
        _spec(fitness=("mse",))
    with pytest.raises(ValueError, match="hit_eps"):
        _spec(hit_eps=-1.0)
    import deap_amd.evaluator as evm
    assert "SymbRegCaseAbsErrors" in evm.__all__


# -------------------------------------------------------------- refusals --
def test_fp32_is_refused():
    with pytest.raises(ValueError, match="SymbRegCaseAbsErrors is fp64 only"):
        GPUEvaluator(configs.pset_for("symreg10"), _spec(), device=0, precision="fp32")


def test_a_numpy_semantics_set_is_refused():
    rng = np.random.default_rng(7)
    spec = SymbRegCaseAbsErrors(rng.uniform(-1, 1, (1, 8)), rng.normal(size=8))
    with pytest.raises(NotImplementedError,
                       match="SymbRegCaseAbsErrors needs Python-semantics"):
        GPUEvaluator(configs.pset_for("symbreg_numpy"), spec, device=0)


def test_a_typed_set_is_refused():
    ps = configs.pset_for("spambase")
    rng = np.random.default_rng(8)
    spec = SymbRegCaseAbsErrors(rng.uniform(0, 1, (len(ps.arguments), 8)),
                                rng.normal(size=8), cases="device")
    with pytest.raises(NotImplementedError,
                       match="SymbRegCaseAbsErrors does not take a typed primitive set"):
        GPUEvaluator(ps, spec, device=0)


class _Local(object):
    def __init__(self):
        self.spec = _spec()


@pytest.mark.parametrize("wrap", [
    lambda loc: distributed.PopulationSharded(loc),
    lambda loc: distributed.CaseSharded(loc, 16, 0)])
def test_the_distributed_wrappers_refuse(wrap):
    with pytest.raises(NotImplementedError, match="SymbRegCaseAbsErrors runs on one GPU"):
        wrap(_Local()).evaluate([])


# ------------------------------------------------------- select_lexicase --
class _StubContext(object):
    """What select_lexicase reads of a context: the program count, and
    ``lexicase`` (which records its call and picks the first k)."""

    def __init__(self, n_prog):
        self.n_prog = n_prog
        self.calls = []

    def lexicase(self, values, maximise, k, rng, mode=0, epsilon=0.0):
        self.calls.append((values, np.asarray(maximise).copy(), k, rng, mode, epsilon))
        return np.arange(k, dtype=np.int32) % self.n_prog, -1


class _Ind(object):
    pass


def _stub_evaluator(results, spec=None):
    ev = GPUEvaluator.__new__(GPUEvaluator)
    ev.spec = spec or _spec(n=5)
    pop = [_Ind() for _ in results]
    ev.ctx = _StubContext(len(pop))
    ev._lex_batch = (list(pop), list(results))
    return ev, pop


def test_select_lexicase_takes_the_last_batch_only():
    ev, pop = _stub_evaluator([(0.0,)] * 4)
    got = ev.select_lexicase(pop, 3, "epsilon", 0.05)
    assert [id(x) for x in got] == [id(x) for x in pop[:3]]
    values, maximise, k, rng, mode, eps = ev.ctx.calls[0]
    assert values is None and k == 3 and mode == 1 and eps == 0.05
    assert rng is random._inst                     # the module stream, as the drop-ins
    assert maximise.dtype == np.uint8 and maximise.tolist() == [0] * 5     # minimised
    assert [ev.select_lexicase(pop, 1, m) and ev.ctx.calls[-1][4]
            for m in ("plain", "epsilon", "automatic")] == [0, 1, 2]
    assert ev.select_lexicase(tuple(pop), 2) == pop[:2]          # (any sequence of them)
    n_calls = len(ev.ctx.calls)
    msg = "must be the batch of this evaluator's last evaluate / map"
    for other in (pop[:3], pop + [pop[0]], pop[::-1], [_Ind() for _ in pop], []):
        with pytest.raises(ValueError, match=msg):
            ev.select_lexicase(other, 2)
    with pytest.raises(ValueError, match="mode must be"):
        ev.select_lexicase(pop, 2, "auto")
    assert ev.select_lexicase(pop, 0) == []
    assert len(ev.ctx.calls) == n_calls            # none of these reached the device
    # other programs loaded since (a predict of another population)
    ev.ctx.n_prog = 7
    with pytest.raises(ValueError, match="now holds 7 programs, not the 4"):
        ev.select_lexicase(pop, 2)


def test_select_lexicase_without_a_matrix_and_with_a_raising_individual():
    ev, pop = _stub_evaluator([(0.0,)] * 3, spec=_spec(cls=SymbRegAbsError, n=5))
    ev._lex_batch = None
    with pytest.raises(ValueError, match="left no per-case matrix on the GPU .*SymbRegAbsError"):
        ev.select_lexicase(pop, 1)
    first, second = ValueError("math domain error"), OverflowError("later")
    ev, pop = _stub_evaluator([(0.0,), first, (1.0,), second])
    with pytest.raises(ValueError) as info:
        ev.select_lexicase(pop, 1)
    assert info.value is first and not ev.ctx.calls


def test_a_failed_selection_is_the_references_index_error():
    ev, pop = _stub_evaluator([(0.0,)] * 3)
    ev.ctx.lexicase = lambda *a, **k: (np.zeros(0, dtype=np.int32), 0)
    with pytest.raises(IndexError, match="Cannot choose from an empty sequence"):
        ev.select_lexicase(pop, 2)


# ------------------------------------------------------------------- ABI --
def test_the_abi_is_declared_bound_and_exported(lib):
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "gpeval.h")).read()
    P, I, I64, D = _lib._P, _lib._I, _lib._I64, __import__("ctypes").c_double
    want = {"gpe_run_abserr_cases": [P, D, P, P, P, P],
            "gpe_host_abserr_cases": [P, P, I64, I64, P]}
    ctype = {"double": D, "int64_t": I64, "int": I}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args)
        assert getattr(lib, name).argtypes == args
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, name
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        got = [P if "*" in a else ctype[a.rsplit(" ", 1)[0].strip()] for a in decl]
        assert got == args, (name, decl)
    assert callable(_lib.Context.run_abserr_cases) and callable(_lib.host_abserr_cases)
    assert callable(GPUEvaluator.select_lexicase)
    # the squared-error spec keeps its own flag; the two are told apart
    assert getattr(SymbRegCaseErrors, "per_case", False)
    assert not getattr(SymbRegCaseErrors, "abs_cases", False)
