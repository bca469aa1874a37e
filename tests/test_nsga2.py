"""NSGA-II without a GPU: the host mirrors of ``tools`` against the
reference's recorded results (``tests/golden/nsga2.json.gz``), the library's
host twin ``gpe_host_nd_sort`` against the golden fronts and against the
mirror on random small problems, the vectorised crowding distance against the
mirror's loop bit for bit, argument errors, the build lists and the shaping of
``size_objective`` tuples."""
import os
import random

import numpy as np
import pytest

import nsga2_cases as nc
from conftest import REPO
from deap_amd import _lib, build, tools
from deap_amd.evaluator import BooleanCaseHits, GPUEvaluator, SymbRegCaseErrors


@pytest.mark.parametrize("name", nc.case_names())
def test_host_mirrors_equal_the_reference(name):
    case = nc.case_by_name(name)
    k = case["k"]
    pop = nc.case_population(case)
    assert nc.idx_fronts(tools.sortNondominated(pop, k)) == case["fronts"]
    assert nc.idx_fronts(tools.sortNondominated(pop, k, first_front_only=True)) \
        == case["first_front"]
    pop = nc.case_population(case)
    random.seed(case["seed"])
    assert [ind.idx for ind in tools.selNSGA2(pop, k)] == case["selected"]
    assert random.getrandbits(32) == case["canary"]
    assert nc.crowding_hex(pop) == case["crowding"]
    if "dcd_k" in case:
        pop = nc.case_population(case)
        tools.selNSGA2(pop, len(pop))
        random.seed(case["seed"] + 1)
        got = tools.selTournamentDCD(pop, case["dcd_k"])
        assert [ind.idx for ind in got] == case["dcd_selected"]
        assert random.getrandbits(32) == case["dcd_canary"]


@pytest.mark.parametrize("name", nc.case_names())
def test_pareto_front_equals_the_reference(name):
    case = nc.case_by_name(name)
    pop = nc.case_population(case)
    third = max(1, len(pop) // 3)
    chunks = [pop[:third], pop[third:2 * third], pop[:third], pop[2 * third:]]
    for key, args in (("pareto_eq", ()),
                      ("pareto_idx", (lambda a, b: a.idx == b.idx,))):
        pf = tools.ParetoFront(*args)
        states = []
        for chunk in chunks:
            pf.update(chunk)
            states.append([ind.idx for ind in pf])
        assert states == case[key], key


def _distinct_rows(pop):
    """The grouping of sortNondominatedGPU: distinct wvalues in first
    appearance order, their members."""
    groups = {}
    for ind in pop:
        groups.setdefault(ind.fitness.wvalues, []).append(ind.idx)
    return np.asarray(list(groups.keys()), dtype=np.float64), list(groups.values())


@pytest.mark.parametrize("name", nc.case_names())
def test_host_twin_equals_the_golden_fronts(name):
    case = nc.case_by_name(name)
    pop = nc.case_population(case)
    w, members = _distinct_rows(pop)
    mult = [len(g) for g in members]
    for ffo, key in ((False, "fronts"), (True, "first_front")):
        rows = _lib.host_nd_sort(w, case["k"], mult, first_front_only=ffo)
        got = [[i for r in front.tolist() for i in members[r]] for front in rows]
        assert got == case[key]


def test_host_twin_equals_the_mirror_on_random_problems():
    rng = np.random.default_rng(20021)
    for trial in range(300):
        values, weights, k = nc.random_problem(rng)
        pop = nc.population(values, weights)
        ffo = trial % 7 == 0
        want = nc.idx_fronts(tools.sortNondominated(pop, k, first_front_only=ffo))
        w, members = _distinct_rows(pop)
        rows = _lib.host_nd_sort(w, k, [len(g) for g in members], first_front_only=ffo)
        got = [[i for r in front.tolist() for i in members[r]] for front in rows]
        assert got == want, (trial, values.tolist(), weights, k)


def test_host_twin_on_equal_rows_and_without_multiplicities():
    """Equal rows do not dominate each other: they share a front, in
    ascending row index, for m = 1 (the sort shortcut) as for m = 2."""
    for m in (1, 2):
        w = np.repeat(np.asarray([[1.0], [3.0], [1.0], [3.0], [2.0]]), m, axis=1)
        rows = nc.fronts_as_lists(_lib.host_nd_sort(w, 5))
        assert rows == [[1, 3], [4], [0, 2]]
        assert nc.fronts_as_lists(_lib.host_nd_sort(w, 2)) == [[1, 3]]
        assert nc.fronts_as_lists(_lib.host_nd_sort(w, 3)) == [[1, 3], [4]]
        assert nc.fronts_as_lists(_lib.host_nd_sort(w, 3, [1, 2, 1, 1, 1])) == [[1, 3]]
    assert _lib.host_nd_sort(np.zeros((4, 2)), 0) == []


def test_vectorised_crowding_distance_has_the_mirrors_bits():
    rng = np.random.default_rng(5)
    for trial in range(200):
        n, m = int(rng.integers(1, 40)), int(rng.integers(1, 5))
        values = rng.integers(0, 6, size=(n, m)) / 3.0
        if trial % 5 == 0:
            values[rng.integers(0, n), rng.integers(0, m)] = np.inf
        if trial % 9 == 0:
            values[rng.integers(0, n), rng.integers(0, m)] = -np.inf
        pop = nc.population(values, [1.0] * m)
        tools.assignCrowdingDist(pop)
        want = np.asarray([ind.fitness.crowding_dist for ind in pop])
        got = tools._crowding_dist(np.asarray([ind.fitness.values for ind in pop]))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (trial, values)


def test_argument_errors():
    with pytest.raises(ValueError, match="objectives"):
        _lib.host_nd_sort(np.zeros((3, 33)), 3)
    with pytest.raises(ValueError, match="objectives"):
        _lib.host_nd_sort(np.zeros((3, 0)), 3)
    with pytest.raises(ValueError, match="rows"):
        _lib.host_nd_sort(np.zeros((0, 2)), 3)
    with pytest.raises(ValueError, match="k ="):
        _lib.host_nd_sort(np.zeros((3, 2)), -1)
    with pytest.raises(ValueError, match="one entry per row"):
        _lib.host_nd_sort(np.zeros((3, 2)), 3, [1, 1])
    w = np.zeros((3, 2))
    w[1, 1] = np.nan
    with pytest.raises(ValueError, match="nan"):
        _lib.host_nd_sort(w, 3)
    with pytest.raises(ValueError):
        _lib.host_nd_sort(np.zeros((3, 2)), 3, [1, 0, 1])
    # the library's own codes, below the Python checks
    lib = _lib.load()
    order = np.zeros(3, dtype=np.int32)
    ends = np.zeros(3, dtype=np.int64)
    import ctypes
    nf, nr = ctypes.c_int64(), ctypes.c_int64()
    args = (1, 0, _lib._ptr(order), _lib._ptr(ends), ctypes.byref(nf), ctypes.byref(nr))
    z = np.zeros((3, 40))
    assert lib.gpe_host_nd_sort(_lib._ptr(z), None, 3, 33, *args) == _lib.GPE_E_INVALID
    assert lib.gpe_host_nd_sort(_lib._ptr(z), None, 3, 0, *args) == _lib.GPE_E_INVALID
    assert lib.gpe_host_nd_sort(_lib._ptr(z), None, 0, 2, *args) == _lib.GPE_E_INVALID
    assert lib.gpe_host_nd_sort(_lib._ptr(w), None, 3, 2, *args) == _lib.GPE_E_ARG
    with pytest.raises(NotImplementedError):
        tools.selNSGA2(nc.population([[1.0, 2.0]], [1.0, 1.0]), 1, nd="log")


def test_nd_sort_header_is_in_the_build_lists():
    assert "nd_sort.h" in build.LIB_HEADERS
    assert os.path.exists(os.path.join(REPO, "deap_amd", "csrc", "nd_sort.h"))
    with open(os.path.join(REPO, "scripts", "build_variant.sh")) as fh:
        assert "deap_amd/csrc/nd_sort.h" in fh.read()
    with open(os.path.join(REPO, "deap_amd", "csrc", "gpeval.hip")) as fh:
        assert '#include "nd_sort.h"' in fh.read()


class _Tree(list):
    pass


def _stub_evaluator(size_objective, adf=False):
    """A GPUEvaluator whose spec results are canned (no device): only
    evaluate's shaping of the tuples runs."""
    ev = GPUEvaluator.__new__(GPUEvaluator)
    ev.size_objective = size_objective
    ev.pset = [None, None] if adf else None
    ev._lex_batch = None

    def canned(individuals):
        out = [(float(i),) for i in range(len(individuals))]
        if len(out) > 1:
            out[1] = ZeroDivisionError("float division by zero")
        ev._lex_batch = (list(individuals), out)
        return out
    ev._evaluate_spec = canned
    return ev


def test_size_objective_appends_the_size_after_the_record():
    pop = [_Tree([0] * 3), _Tree([0] * 5), _Tree([0] * 1)]
    plain = _stub_evaluator(False).evaluate(pop)
    assert plain[0] == (0.0,) and plain[2] == (2.0,)
    ev = _stub_evaluator(True)
    got = ev.evaluate(pop)
    assert got[0] == (0.0, 3) and got[2] == (2.0, 1)
    assert isinstance(got[1], ZeroDivisionError)          # passes through
    assert ev._lex_batch[1][0] == (0.0,)                  # the spec's own tuple
    assert list(ev.map(pop[:1])) == [(0.0, 3)] and ev(pop[0]) == (0.0, 3)
    with pytest.raises(ZeroDivisionError):
        list(ev.map(pop))
    adf = [[_Tree([0] * 3), _Tree([0] * 4)], [_Tree([0] * 2), _Tree([0] * 2)]]
    got = _stub_evaluator(True, adf=True).evaluate(adf)
    assert got[0] == (0.0, 7) and isinstance(got[1], ZeroDivisionError)


def test_size_objective_refuses_per_case_specs():
    """The refusal comes before any device is opened."""
    from deap_amd import configs
    pset = configs.pset_for("symbreg")
    X = np.linspace(-1, 1, 8)[None, :]
    with pytest.raises(ValueError, match="size_objective"):
        GPUEvaluator(pset, SymbRegCaseErrors(X, [X[0] ** 2]), size_objective=True)
    bits = np.asarray([[0, 1, 0, 1], [0, 0, 1, 1]], dtype=np.uint8)
    with pytest.raises(ValueError, match="size_objective"):
        GPUEvaluator(pset, BooleanCaseHits(bits, bits[0] ^ bits[1], cases="host"),
                     size_objective=True)
