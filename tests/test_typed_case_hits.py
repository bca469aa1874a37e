"""``TypedCaseHits`` without a GPU: the spec and both ``cases=`` modes, what it
refuses, the host twin of the word arithmetic (``gpe_host_typed_hit_planes``)
against the plain-Python reference ``bool(func(*row)) is bool(label)``,
``select_lexicase`` / ``informed_subsample`` / ``last_case_hits`` plumbing on a
stub context, the generated hit-planes core beside the count-only one, and the
ABI."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from deap_amd import _lib, build, configs, datasets, distributed, gp
from deap_amd.evaluator import (BooleanCaseHits, GPUEvaluator, TypedBoolHits, TypedCaseHits,
                                pack_bitplanes, unpack_bitplanes)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "deap_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _spec(cases="host", n_cases=37, seed=5):
    rng = np.random.default_rng(seed)
    return TypedCaseHits(rng.random((3, n_cases)), rng.integers(0, 2, n_cases), cases)


# ------------------------------------------------------------------ spec --
def test_the_spec_is_a_typed_bool_hits_with_a_cases_mode():
    s = _spec()
    assert isinstance(s, TypedBoolHits) and s.hit_planes and s.typed_planes
    assert s.cases == "host" and _spec("device").cases == "device"
    assert s.machine == TypedBoolHits.machine and s.mode == _lib.GPE_MODE_HITS_BOOL
    assert not getattr(TypedBoolHits, "hit_planes", False)
    assert not getattr(BooleanCaseHits, "typed_planes", False)
    assert not getattr(s, "per_case", False) and not getattr(s, "abs_cases", False)
    assert s.n_cases == 37 and s.labels.shape == (1, 37) and s.X.shape == (3, 37)
    for bad in ("gpu", None, "Host"):
        with pytest.raises(ValueError, match="cases must be 'host' or 'device'"):
            _spec(bad)
    import deap_amd.evaluator as evm
    assert "TypedCaseHits" in evm.__all__


def test_subset_keeps_the_class_and_the_mode():
    a = _spec("device", 70)
    idx = np.array([69, 0, 0, 33, 32, 31] * 7)
    sub = a.subset(idx)
    assert type(sub) is TypedCaseHits and sub.cases == "device" and sub.n_cases == 42
    assert (sub.X == a.X[:, idx]).all() and (sub.labels == a.labels[:, idx]).all()
    assert a.n_cases == 70                                 # (the spec itself is left alone)


def test_finish_gives_case_tuples_on_the_host_and_counts_on_the_device():
    rng = np.random.default_rng(7)
    n, nc = 6, 37
    hit = rng.integers(0, 2, (n, nc))
    planes = pack_bitplanes(hit)
    hits = hit.sum(axis=1).astype(np.float64)
    ok = np.full(n, _lib.GPE_NO_ERROR, dtype=np.uint64)
    host, dev = _spec("host"), _spec("device")
    out = host.finish_all(hits, None, ok, None, cases=planes)
    assert out == [tuple(row) for row in hit.tolist()]
    assert all(type(v) is int for v in out[0]) and len(out[0]) == nc
    assert host.finish(2, hits[2], None, ok[2], None, cases=planes[2]) == out[2]
    assert dev.finish_all(hits, None, ok, None, cases=None) == [(int(h),) for h in hits]
    assert type(dev.finish_all(hits, None, ok, None)[0][0]) is int
    assert dev.finish(1, hits[1], None, ok[1], None) == (int(hits[1]),)
    assert host.finish_all(np.zeros(0), None, np.zeros(0, np.uint64), None,
                           cases=np.zeros((0, 2), dtype=np.uint32)) == []
    # an erroring individual (the exact pass's first error word) is returned in
    # its place, in both modes, as TypedBoolHits returns it
    bad = ok.copy()
    bad[3] = np.uint64((5 << 2) | _lib.GPE_ERR_OVERFLOW)
    want = TypedBoolHits(host.X, host.labels[0]).finish_all(hits, None, bad, None)
    for spec, cases in ((host, planes), (dev, None)):
        got = spec.finish_all(hits, None, bad, None, cases=cases)
        assert type(got[3]) is type(want[3]) and isinstance(got[3], BaseException)
        assert str(got[3]) == str(want[3])
        assert [g for i, g in enumerate(got) if i != 3] == \
            [g for i, g in enumerate(spec.finish_all(hits, None, ok, None, cases=cases))
             if i != 3]
        one = spec.finish(3, hits[3], None, bad[3], None,
                          cases=None if cases is None else cases[3])
        assert type(one) is type(want[3])


# -------------------------------------------------------------- refusals --
def test_fp32_is_refused_naming_the_spec():
    ps = configs.pset_for("spambase")
    rng = np.random.default_rng(8)
    spec = TypedCaseHits(rng.random((len(ps.arguments), 8)), rng.integers(0, 2, 8))
    with pytest.raises(NotImplementedError, match="TypedCaseHits needs precision='fp64'"):
        GPUEvaluator(ps, spec, device=0, precision="fp32")


def test_boolean_case_hits_still_refuses_a_typed_set():
    ps = configs.pset_for("spambase")
    rng = np.random.default_rng(8)
    spec = BooleanCaseHits(rng.integers(0, 2, (len(ps.arguments), 8)), rng.integers(0, 2, 8))
    with pytest.raises(NotImplementedError,
                       match="BooleanCaseHits does not take a typed primitive set .*typed "
                             "programs run on the F machine's typed core, which stores no "
                             "hit planes"):
        GPUEvaluator(ps, spec, device=0)


class _Local(object):
    def __init__(self):
        self.spec = _spec()


@pytest.mark.parametrize("wrap", [
    lambda loc: distributed.PopulationSharded(loc),
    lambda loc: distributed.CaseSharded(loc, 16, 0)])
def test_the_distributed_wrappers_refuse_naming_the_spec(wrap):
    with pytest.raises(NotImplementedError, match="TypedCaseHits runs on one GPU"):
        wrap(_Local()).evaluate([])


# --------------------------------------------------------- the host twin --
def reference_hits(pset, trees, X, lab):
    """hit[i, c] = ``bool(func(*row)) is bool(label)`` in plain Python, and the
    programs' outputs as doubles."""
    rows = list(zip(*X.tolist()))
    labels = [bool(v) for v in lab.tolist()]
    hit = np.zeros((len(trees), len(rows)), dtype=bool)
    vals = np.zeros((len(trees), len(rows)), dtype=np.float64)
    for i, tree in enumerate(trees):
        func = gp.compile(tree, pset)
        outs = [func(*r) for r in rows]
        hit[i] = [bool(o) is b for o, b in zip(outs, labels)]
        vals[i] = [float(o) for o in outs]
    return hit, vals


@pytest.mark.parametrize("n_cases", [1, 31, 32, 33, 63, 65, 129, 200])
def test_the_host_twin_matches_the_python_reference(lib, n_cases):
    ps = configs.pset_for("spambase")
    X, lab = datasets.spambase_like(200, 57)
    X, lab = X[:, :n_cases], lab[:n_cases]
    trees = configs.population(ps, "half", 24, 57, 2, 4)
    trees += [gp.PrimitiveTree.from_string(s, ps) for s in
              ("True", "False", "lt(IN0, IN1)", "not_(eq(IN2, IN2))")]
    hit, vals = reference_hits(ps, trees, X, lab)
    got = _lib.host_typed_hit_planes(vals, lab)
    units = (n_cases + 31) // 32
    assert got.dtype == np.uint32 and got.shape == (len(trees), units)
    assert (unpack_bitplanes(got, n_cases) == hit).all()
    assert (got == pack_bitplanes(hit)).all()              # (pad bits 0)
    pop = np.array([bin(int(w)).count("1") for w in got.ravel()]).reshape(got.shape)
    assert (pop.sum(axis=1) == hit.sum(axis=1)).all()
    assert hit[-4].tolist() == [bool(v) for v in lab.tolist()]        # "True"
    assert hit[-3].tolist() == [not bool(v) for v in lab.tolist()]    # "False"


def test_the_host_twin_counts_nan_as_true_and_masks_the_pad(lib):
    nan, inf = float("nan"), float("inf")
    vals = np.array([[0.0, -0.0, nan, -nan, inf, -inf, 5e-324, 1.0, 2.5] * 5], dtype=np.float64)
    truth = [False, False, True, True, True, True, True, True, True] * 5
    assert [bool(v) for v in vals[0].tolist()] == truth    # bool(nan) is True
    n_cases = vals.shape[1]                                # 45: not a multiple of 32
    for lab in (np.ones(n_cases), np.zeros(n_cases), np.arange(n_cases) % 2,
                np.where(np.arange(n_cases) % 3 == 0, nan, 0.0)):
        got = _lib.host_typed_hit_planes(vals, lab)
        exp = np.array([t is bool(v) for t, v in zip(truth, lab.tolist())])
        assert (unpack_bitplanes(got, n_cases)[0] == exp).all()
        assert int(got[0, 1]) >> (n_cases - 32) == 0       # pad bits 0
    with pytest.raises(ValueError, match="values are"):
        _lib.host_typed_hit_planes(vals, np.ones(n_cases + 1))
    assert lib.gpe_host_typed_hit_planes(None, None, 1, 1, None) == _lib.GPE_E_INVALID


# ------------------------------------ select_lexicase / informed plumbing --
class _StubContext(object):
    """What the evaluator's per-case methods read of a context."""

    def __init__(self, n_prog, n_cases):
        self.n_prog, self.n_cases = n_prog, n_cases
        self.calls = []
        self.selected = []

    def lexicase_bits(self, planes, n, n_cases, k, rng):
        self.calls.append(("bits", planes, n, n_cases, k, rng))
        return np.arange(k, dtype=np.int32) % self.n_prog, -1

    def lexicase_bits_par(self, planes, n, n_cases, k, seed):
        self.calls.append(("bits_par", planes, n, n_cases, k, seed))
        return np.arange(k, dtype=np.int32) % self.n_prog, -1

    def lexicase(self, *a, **kw):
        raise AssertionError("the double kernel was asked to select on hit planes")

    lexicase_par = lexicase

    def informed_cases(self, planes, n, n_cases, eps, seed, m):
        self.calls.append(("informed", planes, n, n_cases, eps, seed, m))
        return np.arange(m, dtype=np.int64)[::-1].copy(), np.full(m, 3, dtype=np.int32)

    def select_cases(self, idx):
        self.selected.append(idx)

    def hit_planes(self, n):
        self.calls.append(("read", n))
        return np.full((n, (self.n_cases + 31) // 32), 1, dtype=np.uint32)


class _Ind(object):
    pass


def _stub_evaluator(results, cases="device"):
    ev = GPUEvaluator.__new__(GPUEvaluator)
    ev.spec = ev._full_spec = _spec(cases)
    ev.case_subset = None
    ev.full_n_cases = ev.spec.n_cases
    pop = [_Ind() for _ in results]
    ev.ctx = _StubContext(len(pop), ev.spec.n_cases)
    ev._lex_batch = (list(pop), list(results))
    return ev, pop


def test_every_lexicase_mode_runs_the_bit_kernels_on_the_resident_matrix():
    ev, pop = _stub_evaluator([(3,)] * 4)
    for args in (("plain",), ("automatic",), ("epsilon", 0.0), ("epsilon", 0.999999), ()):
        got = ev.select_lexicase(pop, 3, *args)
        assert [id(x) for x in got] == [id(x) for x in pop[:3]]
        kind, planes, n, n_cases, k, rng = ev.ctx.calls[-1]
        assert kind == "bits" and planes is None and k == 3 and rng is random._inst
    random.seed(11)
    want_seed = random.Random(11).getrandbits(64)
    assert ev.select_lexicase(pop, 6, parallel=True) == pop + pop[:2]
    kind, planes, n, n_cases, k, seed = ev.ctx.calls[-1]
    assert kind == "bits_par" and planes is None and k == 6 and seed == want_seed
    assert ev.last_lexicase_seed == want_seed
    for eps in (1.0, -0.25, float("nan")):
        with pytest.raises(ValueError, match=r"epsilon must be in \[0, 1\)"):
            ev.select_lexicase(pop, 2, "epsilon", eps)


def test_a_raising_individual_is_raised_with_the_random_state_untouched():
    first = SyntaxError("too many nested parentheses")
    ev, pop = _stub_evaluator([(1,), first, (2,), OverflowError("later")])
    random.seed(3)
    state = random.getstate()
    for kw in ({}, {"parallel": True}):
        with pytest.raises(SyntaxError) as info:
            ev.select_lexicase(pop, 1, **kw)
        assert info.value is first
    with pytest.raises(SyntaxError):
        ev.informed_subsample(4)
    assert random.getstate() == state and not ev.ctx.calls


def test_informed_subsample_takes_the_planes_and_applies_the_subset():
    ev, pop = _stub_evaluator([(3,)] * 4)
    random.seed(21)
    want_seed = random.Random(21).getrandbits(64)
    with pytest.raises(ValueError, match="eps applies to"):
        ev.informed_subsample(5, eps=0.5)
    with pytest.raises(ValueError, match=r"m must be in \[1, 37\]"):
        ev.informed_subsample(38)
    idx = ev.informed_subsample(5)
    assert idx.tolist() == [4, 3, 2, 1, 0]
    kind, planes, n, n_cases, eps, seed, m = ev.ctx.calls[-1]
    assert kind == "informed" and planes is None and eps == 0.0 and seed == want_seed and m == 5
    assert ev.last_informed_distances.tolist() == [3] * 5
    assert len(ev.ctx.selected) == 1 and ev.ctx.selected[0].tolist() == idx.tolist()
    assert type(ev.spec) is TypedCaseHits and ev.spec.n_cases == 5
    assert ev._lex_batch is None                           # (subsample drops the planes)
    with pytest.raises(ValueError, match="left no per-case matrix on the GPU"):
        ev.select_lexicase(pop, 1)
    with pytest.raises(ValueError, match="left no hit planes on the GPU"):
        ev.last_case_hits()


def test_last_case_hits_reads_the_planes_back_in_either_mode():
    for cases in ("host", "device"):
        ev, pop = _stub_evaluator([(3,)] * 4, cases)
        got = ev.last_case_hits()
        assert got.dtype == bool and got.shape == (4, 37)
        assert got[:, 0].all() and got[:, 32].all() and got.sum() == 8
        assert ev.ctx.calls[-1] == ("read", 4)


# ------------------------------------------------- the generated core --
def test_the_hit_planes_core_is_a_file_of_its_own_beside_the_typed_core():
    build.generate()
    inc, lay = build.ASM_HITS_OUT
    assert os.path.basename(inc) == "gp_asm_core_typed_hits.inc"
    assert not set(build.ASM_HITS_OUT) & set(build.ASM_OUT + build.ASM32_OUT)
    typed = open(os.path.join(CSRC, "gp_asm_core_typed.inc")).read()
    hits = open(inc).read()
    assert "GP_ASM_CORE_TYPED_HITS" in hits and "GP_ASM_CORE_TYPED_HITS" not in typed
    # the count-only core names none of the plane operands; the variant names
    # each of the four exactly once
    for op in ("hp0lo", "hp0hi", "hp1lo", "hp1hi"):
        assert "%%[%s]" % op not in typed
        assert hits.count("%%[%s]" % op) == 1
    # the same handlers in the same order: one translator layout
    ids = re.compile(r"constexpr int (H_\w+|N_FAMS|SGPR_BASE|WINDOW) = (-?\d+);")
    a = ids.findall(open(os.path.join(CSRC, "gp_asm_layout_typed.h")).read())
    assert a and a == ids.findall(open(lay).read())


# ------------------------------------------------------------------- ABI --
def test_the_abi_is_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpeval.h")).read()
    P, I, I64 = _lib._P, _lib._I, _lib._I64
    want = {"gpe_run_typed_hit_planes": [P, P, P, P, P],
            "gpe_host_typed_hit_planes": [P, P, I64, I64, P]}
    ctype = {"int64_t": I64, "int": I}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args)
        assert getattr(lib, name).argtypes == args
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, name
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        got = [P if "*" in a else ctype[a.rsplit(" ", 1)[0].strip()] for a in decl]
        assert got == [P if issubclass(a, ctypes._Pointer) else a for a in args], (name, decl)
    assert callable(_lib.Context.run_typed_hit_planes) and callable(_lib.host_typed_hit_planes)
    assert lib.gpe_run_typed_hit_planes(None, None, None, None, None) == _lib.GPE_E_INVALID
