"""Case subsampling without a GPU: ``subsample``'s argument checks
(``check_case_subset``), the host side of the spec swap (``subset``: counts,
exact target sums, gathered planes, the user's spec untouched), the refusals
of the sharded evaluators and the two C ABI calls' binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from deap_amd import _lib, build
from deap_amd.evaluator import (BooleanHits, SymbRegAbsError,
                                SymbRegCaseAbsErrors, SymbRegCaseErrors,
                                SymbRegMSE, SymbRegNumpySSE, SymbRegScaledMSE,
                                SymbRegSumSSE, TypedBoolHits,
                                check_case_subset, exact_dd_sums,
                                pack_bitplanes)

N = 301


def _data(seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, size=(4, N))
    y = rng.normal(size=N) * 10.0 ** rng.integers(-3, 4, size=N)
    return X, y


def _idx(seed=11, m=77):
    idx = np.random.default_rng(seed).integers(0, N, m)
    idx[:4] = (5, 5, N - 1, 0)          # a duplicate, a descending pair, both ends
    return idx


# ------------------------------------------------------------ validation --
def test_validator_accepts_sequences_and_arrays():
    for idx in ([3, 1, 1, 0], (2,), range(5), np.array([4, 0], dtype=np.int32),
                np.array([4, 0], dtype=np.uint8), np.arange(5)[::-1]):
        out = check_case_subset(idx, 5)
        assert out.dtype == np.int64 and out.ndim == 1
        assert out.tolist() == list(idx)
    a = np.array([1, 2, 3])
    out = check_case_subset(a, 4)
    out[0] = 0
    assert a.tolist() == [1, 2, 3]                       # a copy
    assert len(check_case_subset([0] * 40, 3)) == 40     # longer than the set


@pytest.mark.parametrize("idx", [[], np.zeros(0, dtype=np.int64), [[1, 2]], 3,
                                 np.zeros((2, 2), dtype=np.int64), [0.0, 1.0],
                                 [1.5], ["a"], [True, False], [None]])
def test_validator_value_errors(idx):
    with pytest.raises(ValueError):
        check_case_subset(idx, 5)


@pytest.mark.parametrize("idx, pos, val", [([0, 5], 1, 5), ([-1], 0, -1),
                                           ([2, 3, -7, 9], 2, -7),
                                           (np.array([4, 2 ** 40]), 1, 2 ** 40)])
def test_validator_index_errors_name_the_first_bad_entry(idx, pos, val):
    with pytest.raises(IndexError) as info:
        check_case_subset(idx, 5)
    assert "idx[%d] = %d" % (pos, val) in str(info.value)
    assert "[0, 5)" in str(info.value)


# ------------------------------------------------------------- spec swap --
F_SPECS = [SymbRegMSE, SymbRegNumpySSE, SymbRegSumSSE, SymbRegScaledMSE, SymbRegAbsError,
           SymbRegCaseAbsErrors, SymbRegCaseErrors]


@pytest.mark.parametrize("cls", F_SPECS, ids=lambda c: c.__name__)
def test_f_spec_subset_gathers_and_leaves_the_spec_alone(cls):
    X, y = _data()
    idx = _idx()
    spec = cls(X, y)
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v)
              for k, v in vars(spec).items()}
    sub = spec.subset(idx)
    assert type(sub) is cls and sub is not spec
    assert sub.n_cases == len(idx) and spec.n_cases == N
    assert np.array_equal(sub.X, X[:, idx]) and sub.X.flags.c_contiguous
    assert np.array_equal(sub.terms, y[None, idx]) and sub.terms.flags.c_contiguous
    fresh = cls(X[:, idx], y[idx])
    for k, v in vars(fresh).items():
        got = getattr(sub, k)
        if isinstance(v, np.ndarray):
            assert np.array_equal(got, v), k
        else:
            assert got == v, k
    assert set(vars(spec)) == set(before)
    for k, v in before.items():
        got = getattr(spec, k)
        assert np.array_equal(got, v) if isinstance(v, np.ndarray) else got == v, k
    assert spec.X is not sub.X and np.array_equal(spec.X, X)


def test_scaled_subset_sums_are_the_exact_sums_of_the_gathered_target():
    X, y = _data()
    spec = SymbRegScaledMSE(X, y)
    full = (spec.sy, spec.syy)
    for seed in (1, 2):
        idx = _idx(seed)
        sub = spec.subset(idx)
        sy, syy = exact_dd_sums(y[idx])
        for got, exp in ((sub.sy, sy), (sub.syy, syy)):
            assert np.array(got).view(np.uint64).tolist() == \
                np.array(exp).view(np.uint64).tolist()
        assert (sub.sy, sub.syy) != full
    assert (spec.sy, spec.syy) == full


def test_two_term_columns_and_options_survive():
    X, y = _data()
    T = np.stack([y, 0.5 * y])
    spec = SymbRegCaseAbsErrors(X, T, hit_eps=0.25, cases="device", fitness=("hits", "max"))
    sub = spec.subset(_idx())
    assert np.array_equal(sub.terms, T[:, _idx()])
    assert (sub.hit_eps, sub.cases, sub.fitness) == (0.25, "device", ("hits", "max"))
    assert len(sub.finish_all(np.zeros((2, 4)), None, np.full(2, _lib.GPE_NO_ERROR, np.uint64),
                              np.zeros(2, np.uint32))) == 2


def test_typed_spec_subset():
    X, _ = _data()
    lab = (np.arange(N) % 3 == 0).astype(int)
    spec = TypedBoolHits(X, lab)
    idx = _idx()
    sub = spec.subset(idx)
    assert sub.n_cases == len(idx) and spec.n_cases == N
    assert np.array_equal(sub.X, X[:, idx])
    assert np.array_equal(sub.labels, (lab[idx] != 0).astype(np.float64)[None, :])
    assert spec.labels.shape == (1, N)


@pytest.mark.parametrize("m", [1, 31, 32, 33, 64, 100])
def test_boolean_spec_subset_planes(m):
    rng = np.random.default_rng(m)
    ins = rng.integers(0, 2, size=(6, 64))
    outs = ins.sum(axis=0) % 2
    spec = BooleanHits(ins, outs)
    planes, out_plane = spec.planes.copy(), spec.out_plane.copy()
    idx = rng.integers(0, 64, m)
    sub = spec.subset(idx)
    assert sub.n_cases == m and spec.n_cases == 64
    assert sub.planes.dtype == np.uint32 and sub.planes.shape == (6, (m + 31) // 32)
    assert np.array_equal(sub.planes, pack_bitplanes(ins[:, idx]))
    assert np.array_equal(sub.out_plane, pack_bitplanes(outs[idx])[0])
    assert np.array_equal(spec.planes, planes) and np.array_equal(spec.out_plane, out_plane)


# -------------------------------------------------------------- refusals --
def test_sharded_evaluators_refuse_a_subset():
    from deap_amd import distributed

    class Local(object):
        spec = None

    for ev in (distributed.PopulationSharded(Local()),
               distributed.CaseSharded(Local(), 10, 0)):
        with pytest.raises(NotImplementedError) as info:
            ev.subsample([0, 1])
        assert "case offsets are global" in str(info.value)


# ------------------------------------------------------------- the C ABI --
def test_lib_binds_the_two_calls():
    I, P, I64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert _lib.SIGNATURES["gpe_select_cases"] == (I, [P, P, I64])
    assert _lib.SIGNATURES["gpe_case_subset"] == \
        (I, [P, ctypes.POINTER(I64), ctypes.POINTER(I64)])
    header = open(os.path.join(REPO, "include", "gpeval.h")).read()
    assert re.search(r"int gpe_select_cases\(gpe_ctx\* ctx, const int64_t\* idx, int64_t m\);",
                     header)
    assert re.search(r"int gpe_case_subset\(const gpe_ctx\* ctx, int64_t\* m, "
                     r"int64_t\* n_full\);", header)
    build.build()
    lib = _lib.load()
    for name in ("gpe_select_cases", "gpe_case_subset"):
        assert getattr(lib, name).argtypes is not None
    assert lib.gpe_select_cases(None, None, 0) == _lib.GPE_E_INVALID
    assert lib.gpe_case_subset(None, None, None) == _lib.GPE_E_INVALID
    assert "case_subset.h" in build.LIB_HEADERS
    assert callable(_lib.Context.select_cases) and callable(_lib.Context.case_subset)
