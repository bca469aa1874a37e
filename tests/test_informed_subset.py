"""Informed down-sampling without a GPU: the host twin
(``gpe_host_informed_cases``) against the definition restated in
``informed_ref``, the properties of the distances, the thresholding twin
(``gpe_host_hit_threshold``) against numpy, the ABI, what
``GPUEvaluator.informed_subsample`` refuses (on a stub context) and its one
draw from the ``random`` stream."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import informed_ref as ir
from deap_amd import _lib, build, distributed
from deap_amd.evaluator import (BooleanCaseHits, GPUEvaluator, SymbRegCaseAbsErrors,
                                SymbRegCaseErrors, pack_bitplanes)

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0x1234567, (1 << 64) - 1)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def sizes(n_cases):
    return sorted({1, min(2, n_cases), max(1, n_cases // 2), n_cases})


# ------------------------------------------------------------ the oracle --
def test_the_oracles_keys_are_splitmix64():
    # SplitMix64 seeded with 0: its first outputs (Steele, Lea & Flood 2014;
    # the generator java.util.SplittableRandom and xoshiro's seeding use)
    assert [int(k) for k in ir.splitmix_keys(0, 3)] == [
        0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for seed in SEEDS + (0,):
        assert (ir.splitmix_keys(seed, 70) == ir.splitmix_keys_np(seed, 70)).all()


def test_the_oracle_on_a_case_worked_by_hand():
    # columns: a = 000, b = 111, c = 001, d = 000 (a's duplicate)
    hit = np.array([[0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 1, 0]], dtype=bool)
    for seed in range(12):
        key = [int(k) for k in ir.splitmix_keys(seed, 4)]
        first = min(range(4), key=lambda c: (key[c], c))
        chosen, dist = ir.informed_cases(hit, 4, seed)
        assert chosen[0] == first and dist[0] == -1 and sorted(chosen.tolist()) == [0, 1, 2, 3]
        if first in (0, 3):                                # from 000: 111 (3), 001 (1), twin (0)
            assert chosen.tolist()[1:3] == [1, 2] and dist.tolist() == [-1, 3, 1, 0]
        elif first == 1:                                   # from 111: a 000 (3), 001 (1), twin
            other = min((0, 3), key=lambda c: (key[c], c))
            assert chosen.tolist()[1:3] == [other, 2] and dist.tolist() == [-1, 3, 1, 0]
        else:                                              # from 001: 111 (2), a 000 (1), twin
            assert chosen[1] == 1 and dist.tolist() == [-1, 2, 1, 0]


# --------------------------------------------------------- the host twin --
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_the_host_twin_against_the_oracle(lib, n):
    shapes = [(c, n) for c in (1, 31, 32, 33, 513)]
    seen_equal = 0
    for kind, hit in ir.matrices(shapes, seed=n):
        n_cases = hit.shape[1]
        planes = pack_bitplanes(hit)
        for m in sizes(n_cases):
            for seed in SEEDS:
                exp_idx, exp_dist = ir.informed_cases(hit, m, seed)
                idx, dist = _lib.host_informed_cases(planes, n_cases, seed, m)
                assert idx.dtype == np.int64 and dist.dtype == np.int32
                assert idx.tolist() == exp_idx.tolist(), (kind, n_cases, m, seed)
                assert dist.tolist() == exp_dist.tolist(), (kind, n_cases, m, seed)
                # the properties the definition promises
                assert dist[0] == -1 and len(set(idx.tolist())) == m
                assert (np.diff(dist[1:]) <= 0).all() and (dist[1:] >= 0).all()
                assert 0 <= idx.min() and idx.max() < n_cases
                if kind == "equal":                        # pure key order
                    key = ir.splitmix_keys(seed, n_cases)
                    order = sorted(range(n_cases), key=lambda c: (int(key[c]), c))
                    assert idx.tolist() == order[:m] and not dist[1:].any()
                    seen_equal += 1
    assert seen_equal


def test_the_matrices_hold_what_the_traversal_must_cope_with():
    for kind, hit in ir.matrices([(513, 65), (33, 63)]):
        if kind == "mixed":
            cols = {c.tobytes() for c in hit.T}
            assert len(cols) < hit.shape[1]                # duplicated columns
            assert (~hit).all(axis=0).any() and hit.all(axis=0).any()
        else:
            assert (hit == hit[:, :1]).all()


def test_distances_stop_at_zero_when_only_duplicates_remain(lib):
    rng = np.random.default_rng(3)
    pool = rng.integers(0, 2, (40, 5)).astype(bool)
    hit = pool[:, rng.integers(0, 5, 60)]
    distinct = len({c.tobytes() for c in hit.T})
    idx, dist = _lib.host_informed_cases(pack_bitplanes(hit), 60, 99, 60)
    assert (dist[1:distinct] > 0).all() and not dist[distinct:].any()
    assert len({hit[:, c].tobytes() for c in idx[:distinct]}) == distinct
    key = ir.splitmix_keys(99, 60)
    rest = idx[distinct:].tolist()
    assert rest == sorted(rest, key=lambda c: (int(key[c]), c))     # "then at random"


def test_the_host_twin_refuses_what_it_cannot_index(lib):
    planes = pack_bitplanes(np.ones((2, 5), dtype=bool))
    for m in (0, 6, -1):
        with pytest.raises(_lib.GpeError, match="gpe_host_informed_cases failed"):
            _lib.host_informed_cases(planes, 5, 1, m)
    with pytest.raises(_lib.GpeError):
        _lib.host_informed_cases(np.zeros((0, 1), dtype=np.uint32), 5, 1, 2)       # n < 1
    with pytest.raises(ValueError, match=r"planes must be uint32 \[n, 1\] for 5 cases"):
        _lib.host_informed_cases(np.zeros((2, 2), dtype=np.uint32), 5, 1, 2)


# ----------------------------------------------------- the threshold twin --
@pytest.mark.parametrize("n_cases", [1, 32, 33, 65])
def test_the_threshold_twin_is_finite_and_at_most_eps(lib, n_cases):
    rng = np.random.default_rng(n_cases)
    n = 7
    e = np.abs(rng.normal(size=(n, n_cases)))
    e[rng.random((n, n_cases)) < 0.15] = 0.5               # e == eps
    e[rng.random((n, n_cases)) < 0.1] = np.nan
    e[rng.random((n, n_cases)) < 0.1] = np.inf
    e[rng.random((n, n_cases)) < 0.1] = 0.0
    e[0, 0], e[1, 0], e[2, 0], e[3, 0] = 0.5, np.nan, np.inf, 0.0
    for eps in (0.5, 0.0, np.inf, np.nextafter(0.5, 0.0)):
        with np.errstate(invalid="ignore"):
            exp = np.isfinite(e) & (e <= eps)
        assert (ir.threshold(e, eps) == exp).all()
        got = _lib.host_hit_threshold(e, eps)
        assert got.dtype == np.uint32 and got.shape == (n, (n_cases + 31) // 32)
        assert (got == pack_bitplanes(exp)).all(), eps     # (pad bits 0)
    assert ir.threshold(e, 0.5)[0, 0] and not ir.threshold(e, np.nextafter(0.5, 0.0))[0, 0]
    assert not ir.threshold(e, np.inf)[1:3, 0].any() and ir.threshold(e, 0.0)[3, 0]


# ------------------------------------------------------------------- ABI --
def test_the_abi_is_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpeval.h")).read()
    P, I, I64 = _lib._P, _lib._I, _lib._I64
    D, U64 = ctypes.c_double, ctypes.c_uint64
    want = {"gpe_informed_cases": [P, P, I64, I64, D, U64, I64, P, P],
            "gpe_host_informed_cases": [P, I64, I64, U64, I64, P, P],
            "gpe_host_hit_threshold": [P, I64, I64, D, P]}
    ctype = {"int64_t": I64, "int": I, "double": D, "uint64_t": U64}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args)
        assert getattr(lib, name).argtypes == args
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, name
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        got = [P if "*" in a else ctype[a.rsplit(" ", 1)[0].strip()] for a in decl]
        assert got == args, (name, decl)
    assert callable(_lib.Context.informed_cases) and callable(GPUEvaluator.informed_subsample)
    assert callable(_lib.host_informed_cases) and callable(_lib.host_hit_threshold)
    out = np.zeros(1, dtype=np.int64)
    assert lib.gpe_host_informed_cases(None, 1, 1, 0, 1, _lib._ptr(out), None) == \
        _lib.GPE_E_INVALID
    assert lib.gpe_host_hit_threshold(None, 1, 1, 0.0, None) == _lib.GPE_E_INVALID


# ------------------------------------------------- the evaluator's checks --
class _StubContext(object):
    """What informed_subsample reads of a context: the program count and
    ``informed_cases``, which records its call and picks the first m cases."""

    def __init__(self, n_prog):
        self.n_prog = n_prog
        self.calls = []
        self.selected = []

    def informed_cases(self, planes, n, n_cases, eps, seed, m):
        self.calls.append((planes, n, n_cases, eps, seed, m))
        return np.arange(m, dtype=np.int64), np.full(m, -1, dtype=np.int32)

    def select_cases(self, idx):
        self.selected.append(idx)


class _Ind(object):
    pass


def _bool_spec(cases="device", n_cases=37):
    rng = np.random.default_rng(5)
    return BooleanCaseHits(rng.integers(0, 2, (3, n_cases)), rng.integers(0, 2, n_cases), cases)


def _reg_spec(cls=SymbRegCaseAbsErrors, n_cases=37, **kw):
    x = np.linspace(-1, 1, n_cases)
    return cls(x[None, :], x ** 2, **kw)


def _stub(results, spec):
    ev = GPUEvaluator.__new__(GPUEvaluator)
    ev.spec = ev._full_spec = spec
    ev.full_n_cases = spec.n_cases
    ev.case_subset = None
    pop = [_Ind() for _ in results]
    ev.ctx = _StubContext(len(pop))
    ev._lex_batch = (list(pop), list(results))
    ev.last_informed_distances = np.zeros(0, dtype=np.int32)
    return ev


WHAT_TO_DO = r"subsample\(None\) and evaluate the parent sample first"


def test_the_call_reaches_the_library_with_the_specs_epsilon():
    ev = _stub([(1,)] * 4, _bool_spec())
    idx = ev.informed_subsample(5, apply=False)
    assert idx.tolist() == [0, 1, 2, 3, 4] and ev.last_informed_distances.tolist() == [-1] * 5
    planes, n, n_cases, eps, seed, m = ev.ctx.calls[-1]
    assert planes is None and m == 5 and eps == 0.0 and 0 <= seed < 1 << 64
    assert not ev.ctx.selected and ev._lex_batch is not None and ev.case_subset is None
    for cases in ("host", "device"):
        ev = _stub([(1.0,)] * 4, _reg_spec(hit_eps=0.125, cases=cases))
        ev.informed_subsample(37, apply=False)
        assert ev.ctx.calls[-1][3] == 0.125 and ev.ctx.calls[-1][5] == 37
        ev.informed_subsample(1, eps=2.5, apply=False)
        assert ev.ctx.calls[-1][3] == 2.5
    # apply=True: subsample(idx) follows, which drops the per-case matrix
    idx = ev.informed_subsample(3)
    assert ev.case_subset.tolist() == idx.tolist() == [0, 1, 2]
    assert ev.ctx.selected[-1].tolist() == [0, 1, 2] and ev._lex_batch is None
    assert ev.spec.n_cases == 3 and ev.n_cases == 3
    with pytest.raises(ValueError, match=WHAT_TO_DO):      # a second one, subset active
        ev.informed_subsample(2)


def test_what_is_refused():
    ev = _stub([(1,)] * 4, _bool_spec())
    ev._lex_batch = None                                   # no per-case matrix
    with pytest.raises(ValueError, match="no per-case matrix is on the GPU.*" + WHAT_TO_DO):
        ev.informed_subsample(3)
    ev = _stub([(1,)] * 4, _bool_spec())
    ev.case_subset = np.arange(5)                          # an active subset
    with pytest.raises(ValueError, match="a case subset is active.*" + WHAT_TO_DO):
        ev.informed_subsample(3)
    ev = _stub([(1.0,) * 37] * 4, _reg_spec(SymbRegCaseErrors))     # squared errors
    with pytest.raises(ValueError, match="the spec is SymbRegCaseErrors.*" + WHAT_TO_DO):
        ev.informed_subsample(3)
    ev = _stub([(1,)] * 4, _bool_spec())
    with pytest.raises(ValueError, match="eps applies to SymbRegCaseAbsErrors"):
        ev.informed_subsample(3, eps=0.5)
    for m in (0, 38, -1):
        with pytest.raises(ValueError, match=r"m must be in \[1, 37\]"):
            ev.informed_subsample(m)
    ev = _stub([(1.0,)] * 4, _reg_spec())
    for eps in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="eps must be >= 0"):
            ev.informed_subsample(3, eps=eps)
    ev.ctx.n_prog = 7
    with pytest.raises(ValueError, match="now holds 7 programs, not the 4"):
        ev.informed_subsample(3)
    first, second = SyntaxError("too many nested parentheses"), ValueError("later")
    ev = _stub([(1,), first, (2,), second], _bool_spec())
    state = random.getstate()
    with pytest.raises(SyntaxError) as info:
        ev.informed_subsample(3)
    assert info.value is first
    assert random.getstate() == state and not ev.ctx.calls and not ev.ctx.selected


class _Local(object):
    def __init__(self):
        self.spec = _bool_spec()


@pytest.mark.parametrize("wrap, name", [
    (lambda loc: distributed.PopulationSharded(loc), "PopulationSharded"),
    (lambda loc: distributed.CaseSharded(loc, 16, 0), "CaseSharded")])
def test_the_distributed_wrappers_refuse(wrap, name):
    with pytest.raises(NotImplementedError, match=name + " does not take a case subset"):
        wrap(_Local()).informed_subsample(4)
    with pytest.raises(NotImplementedError, match="does not take a case subset"):
        wrap(_Local()).informed_subsample(4, eps=0.1, apply=False)


def test_exactly_one_draw_of_64_bits_from_the_random_stream():
    ev = _stub([(1,)] * 4, _bool_spec())
    for apply in (False, True):
        ev = _stub([(1,)] * 4, _bool_spec())
        random.seed(77)
        twin = random.Random(77)
        ev.informed_subsample(4, apply=apply)
        assert ev.ctx.calls[-1][4] == twin.getrandbits(64)
        assert random.getstate() == twin.getstate()
    # a refused call draws nothing
    random.seed(78)
    state = random.getstate()
    with pytest.raises(ValueError):
        ev.informed_subsample(4)                           # (the subset is active now)
    assert random.getstate() == state
