"""Parallel lexicase selection without a GPU: the keys, the host twin
(``gpe_host_lexicase_par``) against the rule restated in ``lexicase_par_ref``,
the frequencies the rule selects with, the argument errors and the ABI."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import lexicase_par_ref as lr
from deap_amd import _lib, build, tools
from deap_amd.evaluator import GPUEvaluator

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0x1234567, (1 << 64) - 1)
MODES = ((0, 0.0), (1, 0.75), (2, 0.0))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_the_keys_are_splitmix64():
    assert lr.key(0, 0) == 0xE220A8397B1DCDAF
    assert lr.key(0, 1) == 0x6E789E6AA1B965F4


def test_the_librarys_keys_are_those_keys(lib):
    """65,536 clones on one case all survive, so selection s picks survivor
    (K(i0 + C) * 2^16) >> 64 with i0 + C = 2 s + 1: the top 16 bits of K(1),
    K(3), K(5) of the library's own key function.  And on two specialists the
    case that comes first decides: K(1) < K(0) for seed 0 puts case 1 first."""
    clones = np.zeros((1 << 16, 1))
    got, failed = _lib.host_lexicase_par(clones, [0], 3, 0, 0)
    assert failed == -1 and got[0] == 0x6E789E6AA1B965F4 >> 48 == 0x6E78
    assert got.tolist() == [lr.key(0, 2 * s + 1) >> 48 for s in range(3)]
    got, failed = _lib.host_lexicase_par(clones, [0], 2, SEEDS[1], 0)
    assert got.tolist() == [lr.key(SEEDS[1], 2 * s + 1) >> 48 for s in range(2)]
    assert 0x6E789E6AA1B965F4 < 0xE220A8397B1DCDAF
    got, failed = _lib.host_lexicase_par([[0.0, 1.0], [1.0, 0.0]], [0, 0], 1, 0, 0)
    assert failed == -1 and got.tolist() == [1]


def check(values, maximise, k, seed, mode, eps):
    got, gf = _lib.host_lexicase_par(values, maximise, k, seed, mode, eps)
    ref, rf = lr.lexicase_par(values, maximise, k, seed, mode, eps)
    assert got.dtype == np.int32 and got.shape == (k,)
    assert gf == rf and (got == ref).all(), (gf, rf, got[:8], ref[:8])
    return got, gf


@pytest.mark.parametrize("C", (1, 2, 33))
@pytest.mark.parametrize("n", (1, 2, 3, 64, 65))
def test_the_host_twin_is_the_rule(lib, n, C):
    """Every matrix, mode and maximise setting at odd and even population
    sizes; the nan matrices make selections fail (failed >= 0, -1 entries)."""
    failures = 0
    for name, values in lr.matrices(n, C).items():
        for mx in lr.maximise_settings(C).values():
            for mode, eps in MODES:
                got, failed = check(values, mx, 7, SEEDS[(n + C + mode) % 2], mode, eps)
                assert (failed >= 0) == bool((got < 0).any())
                if failed >= 0:
                    assert name == "nan" and got[failed] == -1 and (got[:failed] >= 0).all()
                    failures += 1
                if name == "clones":           # every candidate survives every case
                    assert failed < 0 and (n < 3 or len(set(got.tolist())) > 1)
    assert n == 1 or failures > 0


def test_many_selections_and_none(lib):
    values = lr.matrices(65, 5)["ties"]
    mx = lr.maximise_settings(5)["mixed"]
    for mode, eps in MODES:
        got, failed = check(values, mx, 300, SEEDS[1], mode, eps)
        assert failed == -1 and got.min() >= 0 and got.max() < 65
        got, failed = _lib.host_lexicase_par(values, mx, 0, 5, mode, eps)
        assert got.shape == (0,) and failed == -1


def test_odd_and_even_candidate_counts_in_automatic_mode(lib):
    """Two-level columns leave candidate sets of either parity for the next
    case's medians (the even ones take (a + b) / 2)."""
    rng = np.random.default_rng(3)
    for n in (6, 7, 10, 11):
        values = np.concatenate([rng.integers(0, 2, (n, 1)).astype(np.float64),
                                 rng.normal(size=(n, 4))], axis=1)
        check(values, np.zeros(5, dtype=np.uint8), 40, 99, 2, 0.0)


def test_the_rule_selects_what_lexicase_selects(lib):
    """Individuals 0 and 3 are clones and win case 0, individual 1 wins case
    1, individual 2 is dominated: lexicase picks 1 half of the time and 0 or 3
    a quarter each.  Bounds: 400 is more than five standard deviations of the
    binomial (sqrt(20000 / 4) = 71 at p = 1/2), and the seed is fixed."""
    values = np.array([[0, 1], [1, 0], [2, 2], [0, 1]], dtype=np.float64)
    got, failed = _lib.host_lexicase_par(values, [0, 0], 20000, 12345, 0)
    ref, _ = lr.lexicase_par(values, [0, 0], 20000, 12345, 0)
    assert failed == -1 and (got == ref).all()
    counts = np.bincount(got, minlength=4)
    print("picks per individual:", counts.tolist())
    assert abs(counts[1] - 10000) <= 400
    assert abs(counts[0] - 5000) <= 400 and abs(counts[3] - 5000) <= 400
    assert counts[2] == 0


def test_argument_errors_of_the_host_twin(lib):
    v = np.zeros((3, 2))
    mx = np.zeros(2, dtype=np.uint8)
    with pytest.raises(ValueError, match=r"n = 0 individuals \(need 1 \.\. 2\^31 - 1\)"):
        _lib.host_lexicase_par(np.zeros((0, 2)), mx, 1, 0)
    with pytest.raises(ValueError, match=r"n_cases = 0 \(need 1 \.\. 2\^31 - 1\)"):
        _lib.host_lexicase_par(np.zeros((3, 0)), np.zeros(0, dtype=np.uint8), 1, 0)
    with pytest.raises(ValueError, match=r"k = -1 selections \(need >= 0\)"):
        _lib.host_lexicase_par(v, mx, -1, 0)
    with pytest.raises(ValueError, match=r"mode must be 0, 1 or 2 \(got 3\)"):
        _lib.host_lexicase_par(v, mx, 1, 0, mode=3)
    with pytest.raises(ValueError, match=r"maximise must have one entry per case \(2\)"):
        _lib.host_lexicase_par(v, np.zeros(3, dtype=np.uint8), 1, 0)
    with pytest.raises(ValueError, match=r"values must be \[n, n_cases\]"):
        _lib.host_lexicase_par(np.zeros(3), mx, 1, 0)
    # the library itself refuses the same (no context: no message)
    out = np.zeros(4, dtype=np.int32)
    failed = ctypes.c_int64(0)
    P = _lib._ptr
    call = lib.gpe_host_lexicase_par
    for args in ((None, 3, 2, P(mx), 0, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 3, 2, None, 0, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 0, 2, P(mx), 0, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 1 << 31, 2, P(mx), 0, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 3, 0, P(mx), 0, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 3, 1 << 31, P(mx), 0, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 3, 2, P(mx), 3, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 3, 2, P(mx), -1, 0.0, 0, 1, P(out), ctypes.byref(failed)),
                 (P(v), 3, 2, P(mx), 0, 0.0, 0, -1, P(out), ctypes.byref(failed)),
                 (P(v), 3, 2, P(mx), 0, 0.0, 0, 1, None, ctypes.byref(failed))):
        assert call(*args) == _lib.GPE_E_INVALID, args[1:8]
    assert call(P(v), 3, 2, P(mx), 0, 0.0, 0, 0, None, None) == 0      # k == 0: nothing
    assert lib.gpe_lexicase_par(None, None, 1, 1, None, 0, 0.0, 0, 1, None, None) == \
        _lib.GPE_E_INVALID
    assert lib.gpe_lexicase_bits_par(None, None, 1, 1, 0, 1, None, None) == _lib.GPE_E_INVALID


def test_the_abi_is_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpeval.h")).read()
    P, I, I64 = _lib._P, _lib._I, _lib._I64
    D, U64 = ctypes.c_double, ctypes.c_uint64
    want = {"gpe_lexicase_par": [P, P, I64, I64, P, I, D, U64, I64, P, P],
            "gpe_lexicase_bits_par": [P, P, I64, I64, U64, I64, P, P],
            "gpe_host_lexicase_par": [P, I64, I64, P, I, D, U64, I64, P, P]}
    ctype = {"int64_t": I64, "int": I, "double": D, "uint64_t": U64}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args)
        assert getattr(lib, name).argtypes == args
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, name
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        got = [P if "*" in a else ctype[a.rsplit(" ", 1)[0].strip()] for a in decl]
        assert got == args, (name, decl)
    assert re.search(r"\bint64_t gpe_lexicase_par_lds_values\(void\);", header)
    assert _lib.SIGNATURES["gpe_lexicase_par_lds_values"] == (I64, [])
    assert _lib.lexicase_par_lds_values() >= 64
    # the rule is in the header with its constants
    for text in ("0x9E3779B97F4A7C15", "0xE220A8397B1DCDAF", "0x6E789E6AA1B965F4",
                 "i0 = s * (C + 1)", "(K(i0 + C) * count) >> 64"):
        assert text in header, text
    assert "lexicase_par.h" in build.LIB_HEADERS
    for meth in ("lexicase_par", "lexicase_bits_par"):
        assert callable(getattr(_lib.Context, meth))
    assert inspect.signature(GPUEvaluator.select_lexicase).parameters["parallel"].default is False
    for fn in (tools.selLexicaseGPU, tools.selEpsilonLexicaseGPU,
               tools.selAutomaticEpsilonLexicaseGPU):
        assert inspect.signature(fn).parameters["parallel"].default is False
