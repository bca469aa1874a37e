"""Test helper for ``GPUEvaluator.predict``: the reference expression

    numpy.array([[gp.compile(t, pset)(*row) for row in rows] for t in pop],
                dtype=numpy.float64)

case by case, so that the case an exception comes from is known, and a bit
compare in which a nan equals a nan and -0.0 differs from +0.0.  Not product
code.
"""
import numpy as np

from abs_sqrt_ref import ERRORS
from deap_amd import gp


def to_float64(v):
    """One result as ``numpy.array([v], dtype=numpy.float64)`` converts it: a
    bool 1.0 / 0.0, a Python int ``float(int)`` (correctly rounded;
    OverflowError past the float range), a float itself."""
    return float(np.array([v], dtype=np.float64)[0])


def values(pset, pop, X):
    """``(F, exc)``: ``F[n_prog, n_cases]`` float64 with nan where the case
    raised, and per program ``{case: exception type name}`` (from
    ``func(*row)`` or from the conversion of its result)."""
    rows = list(zip(*np.asarray(X).tolist()))
    F = np.full((len(pop), len(rows)), np.nan)
    exc = [dict() for _ in pop]
    for i, tree in enumerate(pop):
        func = gp.compile(tree, pset)
        for c, row in enumerate(rows):
            try:
                F[i, c] = to_float64(func(*row))
            except ERRORS as e:
                exc[i][c] = type(e).__name__
    return F, exc


def first_errors(exc):
    """``int64[n]``: each program's first raising case, -1 for none."""
    return np.array([min(e) if e else -1 for e in exc], dtype=np.int64)


def bits(a):
    """float64 → uint64 bit patterns, every nan as one pattern."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    return b


def same_bits(got, exp):
    """True where got and exp hold the same float64 bits (nan == nan,
    -0.0 != +0.0), elementwise."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    return bits(got) == bits(exp)


def assert_same_bits(got, exp, what=""):
    ok = same_bits(got, exp)
    if not ok.all():
        idx = np.argwhere(~ok)
        i = tuple(idx[0])
        raise AssertionError("%s: %d of %d values differ, first at %r: got %r, expected %r"
                             % (what, len(idx), ok.size, i, np.asarray(got)[i],
                                np.asarray(exp)[i]))
