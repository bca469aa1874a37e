"""``GPUEvaluator.predict`` without a GPU: the chunk planner, the mapping from
a values run's error words to the reference's exceptions, the B machine's
bit-plane unpacking, and the reference helper of the GPU tests
(``predict_ref``) on bool, int and large-int results."""
import math
import operator

import numpy as np
import pytest

import predict_ref as pr
from deap_amd import _lib, gp
from deap_amd.configs import protectedDiv
from deap_amd.evaluator import (first_error_cases, pack_bitplanes,
                                plan_predict_chunks, predict_error,
                                unpack_bitplanes)

NO = _lib.GPE_NO_ERROR


# ---------------------------------------------------------- chunk planner --
@pytest.mark.parametrize("budget, runs", [(700, 1), (10 ** 9, 1), (300, 3),
                                          (399, 3), (100, 7), (199, 7)])
def test_chunks_split_seven_individuals(budget, runs):
    chunks = plan_predict_chunks(7, 100, budget)
    assert len(chunks) == runs
    # in order, without a gap or an overlap, each within the budget
    assert chunks[0][0] == 0 and chunks[-1][1] == 7
    for (a, b), (c, d) in zip(chunks, chunks[1:]):
        assert b == c
    assert all(0 < b - a and (b - a) * 100 <= budget for a, b in chunks)
    sizes = [b - a for a, b in chunks]
    assert sizes == {1: [7], 3: [3, 3, 1], 7: [1] * 7}[runs]


def test_a_budget_below_one_row_runs_single_rows():
    assert plan_predict_chunks(3, 100, 50) == [(0, 1), (1, 2), (2, 3)]
    assert plan_predict_chunks(3, 100, 0) == [(0, 1), (1, 2), (2, 3)]
    assert plan_predict_chunks(0, 100, 50) == []


# ------------------------------------------------- error words -> errors --
def _word(case, kind):
    return (case << 2) | kind


def test_first_error_cases():
    err = np.array([NO, _word(0, _lib.GPE_ERR_VALUE), _word(385, _lib.GPE_ERR_OVERFLOW),
                    NO], dtype=np.uint64)
    assert first_error_cases(err).tolist() == [-1, 0, 385, -1]
    assert first_error_cases(err).dtype == np.int64


def test_the_first_erroring_individual_raises_its_exception():
    err = np.array([NO, NO, _word(128, _lib.GPE_ERR_VALUE),
                    _word(3, _lib.GPE_ERR_OVERFLOW)], dtype=np.uint64)
    exc = predict_error(err)
    assert type(exc) is ValueError
    assert "individual 2" in str(exc) and "case 128" in str(exc)
    assert "math domain error" in str(exc)
    # a chunk's offset names the individual in the caller's order
    assert "individual 12," in str(predict_error(err, 10))
    # individual order, not case order
    err[2] = NO
    exc = predict_error(err)
    assert type(exc) is OverflowError
    assert "individual 3" in str(exc) and "case 3" in str(exc)
    err[3] = NO
    assert predict_error(err) is None


def test_an_error_kind_the_library_must_not_leak_is_loud():
    err = np.array([_word(5, _lib.GPE_ERR_XINT_RANGE)], dtype=np.uint64)
    with pytest.raises(_lib.GpeError):
        predict_error(err)


# ------------------------------------------------------------- bit planes --
def test_bit_planes_unpack_at_a_partial_word():
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=(5, 40)).astype(np.uint8)
    planes = pack_bitplanes(bits)
    assert planes.shape == (5, 2)
    got = unpack_bitplanes(planes, 40)
    assert got.dtype == bool and got.shape == (5, 40)
    assert (got == bits.astype(bool)).all()
    # pad bits are dropped, whatever they hold
    dirty = planes.copy()
    dirty[:, 1] |= np.uint32(0xffffff00)
    assert (unpack_bitplanes(dirty, 40) == got).all()
    # case c is bit c % 32 of word c // 32
    one = np.zeros((1, 2), dtype=np.uint32)
    one[0, 1] = 1 << 7
    assert np.flatnonzero(unpack_bitplanes(one, 40)[0]).tolist() == [39]
    assert unpack_bitplanes(planes[0], 40).shape == (1, 40)


# ------------------------------------------------------- reference helper --
def _pset():
    ps = gp.PrimitiveSet("PRED", 1)
    ps.addPrimitive(operator.add, 2)
    ps.addPrimitive(operator.sub, 2)
    ps.addPrimitive(operator.mul, 2)
    ps.addPrimitive(protectedDiv, 2)
    ps.addPrimitive(operator.lt, 2)
    ps.addPrimitive(math.sqrt, 1)
    ps.renameArguments(ARG0="x")
    return ps


ONE = "protectedDiv(x, sub(x, x))"           # the int 1 of protectedDiv


def test_reference_helper_converts_as_numpy_does():
    ps = _pset()
    exprs = ["lt(x, 0.5)",                                   # bool
             "add(1, %s)" % ONE,                             # int 2
             "add(9007199254740992, %s)" % ONE,              # 2**53 + 1
             "add(9007199254740994, %s)" % ONE,              # 2**53 + 3
             "mul(%d, %s)" % (10 ** 400, ONE),               # past the float range
             "sqrt(x)", "sub(x, x)", "mul(x, sub(x, x))"]
    pop = [gp.PrimitiveTree.from_string(e, ps) for e in exprs]
    X = np.array([[0.25, 0.75, -1.0]])
    F, exc = pr.values(ps, pop, X)
    assert F.dtype == np.float64 and F.shape == (8, 3)
    assert F[0].tolist() == [1.0, 0.0, 1.0] and not exc[0]
    assert F[1].tolist() == [2.0, 2.0, 2.0]
    # float(2**53 + 1) is a tie: to even, 2**53; 2**53 + 3 to 2**53 + 4
    assert float(2 ** 53 + 1) == 2.0 ** 53
    assert F[2].tolist() == [2.0 ** 53] * 3
    assert F[3].tolist() == [2.0 ** 53 + 4] * 3
    assert exc[4] == {0: "OverflowError", 1: "OverflowError", 2: "OverflowError"}
    assert np.isnan(F[4]).all()
    assert exc[5] == {2: "ValueError"} and F[5, 0] == 0.5 and math.isnan(F[5, 2])
    assert pr.first_errors(exc).tolist() == [-1, -1, -1, -1, 0, 2, -1, -1]
    # signed zeros: x - x is +0.0, x * (x - x) is -0.0 for the negative x
    assert math.copysign(1.0, F[6, 2]) == 1.0 and math.copysign(1.0, F[7, 2]) == -1.0
    with pytest.raises(OverflowError):
        pr.to_float64(10 ** 400)
    assert pr.to_float64(True) == 1.0 and pr.to_float64(7) == 7.0


def test_bit_compare_knows_nan_and_signed_zero():
    a = np.array([0.0, -0.0, math.nan, 1.0, math.inf])
    other_nan = np.array([0x7ff0000000000001], dtype=np.uint64).view(np.float64)[0]
    b = np.array([0.0, -0.0, other_nan, 1.0, math.inf])
    assert pr.same_bits(a, b).all()
    pr.assert_same_bits(a, b)
    c = np.array([-0.0, 0.0, 0.0, np.nextafter(1.0, 2.0), -math.inf])
    assert not pr.same_bits(a, c).any()
    with pytest.raises(AssertionError):
        pr.assert_same_bits(a, c, "signed zero")
