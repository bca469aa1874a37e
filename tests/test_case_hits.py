"""``BooleanCaseHits`` without a GPU: the spec's validation and both ``cases=``
modes, what it refuses, the host twin of the plane arithmetic
(``gpe_host_hit_planes``) against numpy, ``select_lexicase``'s checks on a stub
context, the argument the bit kernel rests on — on 0/1 values the three
lexicase variants make the same draws — with ``deap_amd.tools``, the recorded
reference selections (``tests/golden/lexicase_bits.json.gz``) reproduced by
``tools.selLexicase`` and by a Python mirror of the kernel's word-wide filter,
and the ABI."""
import gzip
import json
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

from deap_amd import _lib, build, configs, distributed, tools
from deap_amd.evaluator import (BooleanCaseHits, BooleanHits, GPUEvaluator, pack_bitplanes,
                                unpack_bitplanes)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def fixture_cases():
    with gzip.open(os.path.join(HERE, "golden", "lexicase_bits.json.gz"), "rt") as fh:
        return json.load(fh)


def _bits(case):
    return np.array([[int(ch) for ch in row] for row in case["rows"]], dtype=np.uint8)


def _spec(cases="host", n_vars=3, n_cases=37, seed=5, cls=BooleanCaseHits):
    rng = np.random.default_rng(seed)
    ins, outs = rng.integers(0, 2, (n_vars, n_cases)), rng.integers(0, 2, n_cases)
    return cls(ins, outs, cases) if cls is BooleanCaseHits else cls(ins, outs)


# ------------------------------------------------------------------ spec --
def test_the_spec_is_a_boolean_hits_with_a_cases_mode():
    s = _spec()
    assert isinstance(s, BooleanHits) and s.hit_planes and s.cases == "host"
    assert s.machine == BooleanHits.machine and s.mode == _lib.GPE_MODE_HITS_BITS
    assert not getattr(s, "per_case", False) and not getattr(s, "abs_cases", False)
    assert not getattr(BooleanHits, "hit_planes", False)
    plain = _spec(cls=BooleanHits)
    assert (s.planes == plain.planes).all() and (s.out_plane == plain.out_plane).all()
    assert s.n_cases == 37 and _spec("device").cases == "device"
    for bad in ("gpu", None, "Host"):
        with pytest.raises(ValueError, match="cases must be 'host' or 'device'"):
            _spec(bad)
    import deap_amd.evaluator as evm
    assert "BooleanCaseHits" in evm.__all__


def test_non_binary_data_and_bad_shapes_are_refused():
    with pytest.raises(NotImplementedError, match="0/1 data"):
        BooleanCaseHits([[0, 1, 2]], [0, 1, 0])
    with pytest.raises(NotImplementedError, match="0/1 data"):
        BooleanCaseHits([[0, 1, 1]], [0, 1, 3], cases="device")
    with pytest.raises(ValueError, match="inputs must be"):
        BooleanCaseHits([[0, 1, 1]], [0, 1])


def test_from_rows_and_subset_keep_the_class_and_the_mode():
    rng = np.random.default_rng(6)
    ins, outs = rng.integers(0, 2, (4, 70)), rng.integers(0, 2, 70)
    a = BooleanCaseHits(ins, outs, "device")
    b = BooleanCaseHits.from_rows(ins.T.tolist(), outs.tolist(), cases="device")
    assert type(b) is BooleanCaseHits and b.cases == "device" and b.n_cases == 70
    assert (a.planes == b.planes).all() and (a.out_plane == b.out_plane).all()
    assert BooleanCaseHits.from_rows(ins.T, outs).cases == "host"
    idx = np.array([69, 0, 0, 33, 32, 31] * 7)
    sub = a.subset(idx)
    assert type(sub) is BooleanCaseHits and sub.cases == "device" and sub.n_cases == 42
    assert (unpack_bitplanes(sub.planes, 42) == ins[:, idx].astype(bool)).all()
    assert (unpack_bitplanes(sub.out_plane, 42)[0] == outs[idx].astype(bool)).all()
    assert a.n_cases == 70                                 # (the spec itself is left alone)


def test_finish_gives_case_tuples_on_the_host_and_counts_on_the_device():
    rng = np.random.default_rng(7)
    n, nc = 6, 37
    hit = rng.integers(0, 2, (n, nc))
    planes = pack_bitplanes(hit)
    hits = hit.sum(axis=1).astype(np.float64)
    host, dev = _spec("host"), _spec("device")
    out = host.finish_all(hits, None, None, None, cases=planes)
    assert out == [tuple(row) for row in hit.tolist()]
    assert all(type(v) is int for v in out[0]) and len(out[0]) == nc
    assert host.finish(2, hits[2], None, None, None, cases=planes[2]) == out[2]
    assert dev.finish_all(hits, None, None, None, cases=None) == [(int(h),) for h in hits]
    assert type(dev.finish_all(hits, None, None, None)[0][0]) is int
    assert dev.finish(1, hits[1], None, None, None) == (int(hits[1]),)
    assert host.finish_all(np.zeros(0), None, None, None,
                           cases=np.zeros((0, 2), dtype=np.uint32)) == []


# -------------------------------------------------------------- refusals --
def test_a_typed_set_is_refused():
    ps = configs.pset_for("spambase")
    rng = np.random.default_rng(8)
    spec = BooleanCaseHits(rng.integers(0, 2, (len(ps.arguments), 8)), rng.integers(0, 2, 8))
    with pytest.raises(NotImplementedError,
                       match="BooleanCaseHits does not take a typed primitive set"):
        GPUEvaluator(ps, spec, device=0)


class _Local(object):
    def __init__(self):
        self.spec = _spec()


@pytest.mark.parametrize("wrap", [
    lambda loc: distributed.PopulationSharded(loc),
    lambda loc: distributed.CaseSharded(loc, 16, 0)])
def test_the_distributed_wrappers_refuse(wrap):
    with pytest.raises(NotImplementedError, match="BooleanCaseHits runs on one GPU"):
        wrap(_Local()).evaluate([])


# ------------------------------------------------------- select_lexicase --
class _StubContext(object):
    """What select_lexicase reads of a context: the program count,
    ``lexicase_bits`` (which records its call and picks the first k) and a
    ``lexicase`` that must not be reached."""

    def __init__(self, n_prog):
        self.n_prog = n_prog
        self.calls = []

    def lexicase_bits(self, planes, n, n_cases, k, rng):
        self.calls.append((planes, n, n_cases, k, rng))
        return np.arange(k, dtype=np.int32) % self.n_prog, -1

    def lexicase(self, *a, **kw):
        raise AssertionError("the double kernel was asked to select on hit planes")


class _Ind(object):
    pass


def _stub_evaluator(results, spec=None):
    ev = GPUEvaluator.__new__(GPUEvaluator)
    ev.spec = spec or _spec("device")
    pop = [_Ind() for _ in results]
    ev.ctx = _StubContext(len(pop))
    ev._lex_batch = (list(pop), list(results))
    return ev, pop


def test_every_mode_runs_the_bit_kernel_on_the_resident_matrix():
    ev, pop = _stub_evaluator([(3,)] * 4)
    for args in (("plain",), ("automatic",), ("epsilon", 0.0), ("epsilon", 0.5),
                 ("epsilon", 0.999999), ()):
        got = ev.select_lexicase(pop, 3, *args)
        assert [id(x) for x in got] == [id(x) for x in pop[:3]]
        planes, n, n_cases, k, rng = ev.ctx.calls[-1]
        assert planes is None and k == 3 and rng is random._inst
    assert len(ev.ctx.calls) == 6
    assert ev.select_lexicase(pop, 0) == [] and len(ev.ctx.calls) == 6
    assert ev.select_lexicase(pop, 6) == pop + pop[:2]            # k > n


@pytest.mark.parametrize("eps, why", [(1.0, "from 1 on every candidate survives"),
                                       (2.5, "random.choice"),
                                       (float("inf"), "from 1 on"),
                                       (-0.25, "a negative epsilon"),
                                       (float("nan"), r"must be in \[0, 1\)")])
def test_an_epsilon_outside_zero_to_one_is_refused_with_the_reason(eps, why):
    ev, pop = _stub_evaluator([(3,)] * 4)
    with pytest.raises(ValueError, match=why):
        ev.select_lexicase(pop, 2, "epsilon", eps)
    assert not ev.ctx.calls
    # (the other modes ignore the argument, as the reference's signatures do)
    assert len(ev.select_lexicase(pop, 2, "plain", eps)) == 2


def test_the_batch_checks_are_those_of_the_other_per_case_specs():
    ev, pop = _stub_evaluator([(3,)] * 4)
    msg = "must be the batch of this evaluator's last evaluate / map"
    for other in (pop[:3], pop + [pop[0]], pop[::-1], [_Ind() for _ in pop], []):
        with pytest.raises(ValueError, match=msg):
            ev.select_lexicase(other, 2)
    with pytest.raises(ValueError, match="mode must be"):
        ev.select_lexicase(pop, 2, "auto")
    ev.ctx.n_prog = 7
    with pytest.raises(ValueError, match="now holds 7 programs, not the 4"):
        ev.select_lexicase(pop, 2)
    assert not ev.ctx.calls
    ev._lex_batch = None                                   # (what subsample leaves)
    with pytest.raises(ValueError, match="left no per-case matrix on the GPU .*BooleanCaseHits"):
        ev.select_lexicase(pop, 1)
    with pytest.raises(ValueError, match="left no hit planes on the GPU"):
        ev.last_case_hits()
    first, second = SyntaxError("too many nested parentheses"), ValueError("later")
    ev, pop = _stub_evaluator([(1,), first, (2,), second])
    with pytest.raises(SyntaxError) as info:
        ev.select_lexicase(pop, 1)
    assert info.value is first and not ev.ctx.calls
    ev, pop = _stub_evaluator([])
    assert ev.select_lexicase([], 0) == []
    with pytest.raises(IndexError, match="list index out of range"):
        ev.select_lexicase([], 2)
    ev, pop = _stub_evaluator([(1,)] * 3)
    ev.ctx.lexicase_bits = lambda *a, **k: (np.zeros(0, dtype=np.int32), 0)
    with pytest.raises(IndexError, match="Cannot choose from an empty sequence"):
        ev.select_lexicase(pop, 2)


# --------------------------------------------------------- the host twin --
@pytest.mark.parametrize("n_cases", [1, 31, 32, 33, 64, 2049])
def test_the_host_twin_is_xnor_and_the_last_words_mask(lib, n_cases):
    rng = np.random.default_rng(100 + n_cases)
    n = 9
    res = rng.integers(0, 2, (n, n_cases))
    res[0], res[1] = 0, 1
    outs = rng.integers(0, 2, n_cases)
    units = (n_cases + 31) // 32
    planes = pack_bitplanes(res)
    # the twin must mask whatever the pad bits hold: set them in its inputs
    pad = np.uint32(0) if n_cases % 32 == 0 else \
        np.uint32((0xFFFFFFFF << (n_cases % 32)) & 0xFFFFFFFF)
    dirty = planes.copy()
    dirty[:, -1] |= pad
    oplane = pack_bitplanes(outs)[0]
    got = _lib.host_hit_planes(dirty, oplane | np.where(np.arange(units) == units - 1, pad, 0)
                               .astype(np.uint32), n_cases)
    assert got.dtype == np.uint32 and got.shape == (n, units)
    exp = (res == outs[None, :])
    assert (unpack_bitplanes(got, n_cases) == exp).all()
    assert (got == pack_bitplanes(exp)).all()              # (pad bits 0)
    assert (_lib.host_hit_planes(planes, oplane, n_cases) == got).all()
    assert (np.array([bin(int(w)).count("1") for w in got.ravel()]).reshape(n, units).sum(axis=1)
            == exp.sum(axis=1)).all()
    with pytest.raises(ValueError, match="planes are"):
        _lib.host_hit_planes(planes[:, :-1] if units > 1 else np.zeros((n, 2), np.uint32),
                             oplane, n_cases)


# ------------------------------------------- the equivalence of the modes --
def _pop(bits):
    w = (1.0,) * bits.shape[1]
    return [SimpleNamespace(fitness=SimpleNamespace(values=tuple(row), weights=w), idx=i)
            for i, row in enumerate(bits.tolist())]


def _run(fn, pop, k, seed, *args):
    random.seed(seed)
    picks = [ind.idx for ind in fn(pop, k, *args)]
    return picks, random.getstate()


def _matrices():
    rng = np.random.default_rng(4242)
    for t in range(24):
        n, c = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        base = rng.integers(0, 2, (max(1, n // 3), c))
        bits = base[rng.integers(0, len(base), n)]         # duplicated rows
        if t % 3 == 0:
            bits = (rng.random((n, c)) < rng.random()).astype(np.int64)
        if c >= 3:
            bits[:, 0] = 0                                 # a case nobody passes
            bits[:, c - 1] = 1                             # a case everybody passes
        yield bits


def test_the_three_modes_make_the_same_draws_on_zero_one_values():
    """The bit kernel has no mode: this is why.  (It runs no library code; it
    guards the argument.)"""
    for t, bits in enumerate(_matrices()):
        pop, k, seed = _pop(bits), len(bits) + 3, 900 + t
        exp = _run(tools.selLexicase, pop, k, seed)
        assert _run(tools.selAutomaticEpsilonLexicase, pop, k, seed) == exp, t
        for eps in (0.0, 0.25, 0.5, 0.999):
            assert _run(tools.selEpsilonLexicase, pop, k, seed, eps) == exp, (t, eps)
    # ... and where it ends: from epsilon 1 on nobody is ever filtered
    bits = np.array([[1, 0], [0, 0], [0, 0]])
    pop = _pop(bits)
    a = _run(tools.selEpsilonLexicase, pop, 40, 3, 1.0)
    assert a != _run(tools.selLexicase, pop, 40, 3)
    assert set(a[0]) == {0, 1, 2}


# ------------------------------------------------ the reference's fixture --
def bit_lexicase(bits, k, rng):
    """The kernel's selection in Python ints: case-major planes (program i at
    bit i), ``cand & plane`` kept when not empty, the r-th set bit chosen."""
    n, n_cases = bits.shape
    planes = [sum(1 << i for i in np.flatnonzero(bits[:, c]).tolist()) for c in range(n_cases)]
    out = []
    for _ in range(k):
        cases = list(range(n_cases))
        rng.shuffle(cases)
        cand, count = (1 << n) - 1, n
        for c in cases:
            if count <= 1:
                break
            keep = cand & planes[c]
            if keep:
                cand, count = keep, bin(keep).count("1")
        r = rng._randbelow(count)
        members = [i for i in range(n) if cand >> i & 1]
        out.append(members[r])
    return out


def test_the_fixture_is_reproduced_by_the_cpu_restatement_and_the_bit_mirror():
    cases = fixture_cases()
    assert [c["name"] for c in cases] == [
        "duplicates_dead_and_full_case_k_over_n", "one_individual", "pop130_cases70",
        "cases700_one_selection_past_624_words"]
    for c in cases:
        bits = _bits(c)
        assert bits.shape[1] == c["n_cases"] and set(np.unique(bits)) <= {0, 1}
        picks, state = _run(tools.selLexicase, _pop(bits), c["k"], c["seed"])
        assert picks == c["selected"], c["name"]
        assert list(state[1]) == c["state"], c["name"]
        rng = random.Random(c["seed"])
        assert bit_lexicase(bits, c["k"], rng) == c["selected"], c["name"]
        assert list(rng.getstate()[1]) == c["state"], c["name"]
    first = _bits(cases[0])
    assert len(np.unique(first, axis=0)) < len(first) // 2           # mostly duplicates
    assert not first[:, 3].any() and first[:, 7].all() and cases[0]["k"] > len(first)
    assert len(cases[1]["rows"]) == 1 and cases[3]["n_cases"] > 624


# ------------------------------------------------------------------- ABI --
def test_the_abi_is_declared_bound_and_exported(lib):
    import ctypes
    import re
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpeval.h")).read()
    P, I, I64 = _lib._P, _lib._I, _lib._I64
    want = {"gpe_run_hit_planes": [P, P, P, P, P],
            "gpe_read_hit_planes": [P, P],
            "gpe_host_hit_planes": [P, P, I64, I64, P],
            "gpe_lexicase_bits": [P, P, I64, I64, P, I64, P, ctypes.POINTER(I64)]}
    ctype = {"int64_t": I64, "int": I}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args)
        assert getattr(lib, name).argtypes == args
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, name
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        got = [P if "*" in a else ctype[a.rsplit(" ", 1)[0].strip()] for a in decl]
        assert got == [P if issubclass(a, ctypes._Pointer) else a for a in args], (name, decl)
    for meth in ("run_hit_planes", "lexicase_bits", "hit_planes"):
        assert callable(getattr(_lib.Context, meth))
    assert callable(_lib.host_hit_planes) and callable(GPUEvaluator.last_case_hits)
    # no GPU: the twin refuses what it cannot index
    assert lib.gpe_host_hit_planes(None, None, 1, 1, None) == _lib.GPE_E_INVALID
