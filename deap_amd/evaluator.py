"""GPU population evaluator — the drop-in behind ``toolbox.map``/``evaluate``.

Reference hot path (chris-chambers/deap):

    toolbox.register("evaluate", evalSymbReg, points=...)   examples/gp/symbreg.py:63
    fitnesses = toolbox.map(toolbox.evaluate, invalid_ind)   deap/algorithms.py:172
      evalSymbReg: func = gp.compile(ind, pset)              deap/gp.py:462-487
                   math.fsum((func(x) - ...)**2 ...) / n     symbreg.py:55-61

Drop-in replacement (the EA loop, PrimitiveSet and PrimitiveTree unchanged):

    ev = GPUEvaluator(pset, SymbRegMSE.quartic())
    toolbox.register("evaluate", ev)
    toolbox.register("map", gpu_map)

``gpu_map(func, individuals)`` recognises a (``functools.partial``-wrapped)
:class:`GPUEvaluator`, flattens all individuals (:mod:`deap_amd.flatten`),
evaluates them in one call of the HIP library and returns the fitness tuples
in order.  Any other function goes to the builtin ``map`` — exactly the
reference's default (``deap/base.py:50``).  Like the reference's lazy ``map``
consumed by ``zip`` (``algorithms.py:173``), the result iterator yields the
individuals before the first failing one and then raises that individual's
exception (``ValueError`` from ``math.sin/cos(inf)``, ``OverflowError`` from
``d**2`` or ``fsum``, ``SyntaxError`` for trees over 200 levels, or whatever a
constant subtree raised).
"""
import copy
import math
import os
import random
import sys
import time
import warnings
from functools import partial

import numpy as np

from . import _lib
from .flatten import (ADFFlattener, ERR_CONST, ERR_SYNTAX, Flattener,
                      Machine, ProgramBatch)


def _tuples1(values, as_int):
    """``[(v,), ...]`` for a float64 array (hit counts as ints), built by
    the native module in one pass."""
    from . import _flatnative
    return _flatnative.tuples1(np.ascontiguousarray(values, dtype=np.float64),
                               as_int)


__all__ = ["SymbRegMSE", "SymbRegNumpySSE", "SymbRegSumSSE",
           "SymbRegScaledMSE", "SymbRegAbsError", "SymbRegCaseErrors",
           "SymbRegCaseAbsErrors",
           "BooleanHits", "BooleanCaseHits",
           "exact_dd_sums", "check_case_subset",
           "TypedBoolHits", "TypedCaseHits", "GPUEvaluator", "gpu_map",
           "TypedConfusion", "BooleanConfusion", "confusion_figures",
           "pack_bitplanes", "unpack_bitplanes", "plan_predict_chunks", "first_error_cases",
           "predict_error"]


def _case_error(err):
    """The exception of a program's first erroring case (out_err's type)."""
    kind = int(err) & 3
    if kind == _lib.GPE_ERR_VALUE:
        return ValueError("math domain error")
    if kind == _lib.GPE_ERR_OVERFLOW:
        return OverflowError(34, "Numerical result out of range")
    # the device exact pass's range end (GPE_ERR_XINT_RANGE) never reaches
    # the caller: the library re-runs such programs on its host evaluator.
    # One that leaks is a library bug, not the reference's OverflowError
    raise _lib.GpeError("internal: per-case error kind %d (first error word "
                        "0x%x) reached the evaluator" % (kind, int(err)))


# --------------------------------------------------------- fitness specs --
class SymbRegMSE(object):
    """``(math.fsum((f(*row) - t0 - t1 - ...)**2 for each case) / n,)``.

    ``X``: float64 ``[n_vars, n_cases]``; ``terms``: float64
    ``[n_terms, n_cases]`` subtracted left to right (symbreg.py:60)."""
    machine = Machine.F
    mode = _lib.GPE_MODE_MSE

    def __init__(self, X, terms):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        if self.X.ndim == 1:
            self.X = self.X[None, :]
        t = np.ascontiguousarray(terms, dtype=np.float64)
        self.terms = t[None, :] if t.ndim == 1 else t
        self.n_cases = self.X.shape[1]
        assert self.terms.shape[1] == self.n_cases

    @classmethod
    def quartic(cls):
        """symbreg.py's ``x**4 + x**3 + x**2 + x`` on ``x/10.``, x in
        [-10, 10) — terms computed with Python ``**`` like the reference."""
        from .datasets import symbreg_points
        X, T = symbreg_points()
        return cls(X, T)

    def upload(self, ctx):
        ctx.set_cases(_lib.GPE_MACHINE_F, self.X, self.terms)

    def subset(self, idx):
        """The spec of cases *idx* (:meth:`GPUEvaluator.subsample`): a
        shallow copy with the gathered host arrays and the numbers that
        depend on them (``n_cases``; :class:`SymbRegScaledMSE`'s ``sy``,
        ``syy``).  It is never uploaded, and this spec is left as it is."""
        sub = copy.copy(self)
        sub.X = np.ascontiguousarray(self.X[:, idx])
        sub.terms = np.ascontiguousarray(self.terms[:, idx])
        sub.n_cases = sub.X.shape[1]
        if getattr(self, "scaled", False):
            sub.sy, sub.syy = exact_dd_sums(sub.terms[0])
        return sub

    def finish(self, i, hi, lo, err, flags):
        if err != _lib.GPE_NO_ERROR:
            return _case_error(err)
        sse = float(hi) + float(lo)
        if math.isinf(sse) and not (flags & _lib.GPE_FLAG_NONFINITE_TERM):
            return OverflowError("intermediate overflow in fsum")
        return (sse / self.n_cases,)

    def finish_all(self, hi, lo, err, flags):
        """:meth:`finish` for a whole batch (vectorised; the same IEEE
        operations, per-individual only where an exception is possible)."""
        sse = hi + lo
        with np.errstate(all="ignore"):
            out = _tuples1(sse / self.n_cases, False)          # 1-tuples, in C
        bad = (err != np.uint64(_lib.GPE_NO_ERROR)) | (
            np.isinf(sse) & ((flags & _lib.GPE_FLAG_NONFINITE_TERM) == 0))
        for i in np.flatnonzero(bad).tolist():
            out[i] = self.finish(i, hi[i], lo[i], err[i], flags[i])
        return out


class SymbRegNumpySSE(SymbRegMSE):
    """``(numpy.sum((func(samples) - values)**2),)`` — the vectorised
    evaluation of ``examples/gp/symbreg_numpy.py:62-68``.

    numpy semantics throughout: ``numpy.sin/cos(+-inf)`` is nan (no
    ``ValueError``), ``**2`` of a large finite value is inf (no
    ``OverflowError``), the protected division of ``symbreg_numpy.py:28-36``
    maps inf/nan quotients to 1 (``Op.NPDIV``), and the sum is not divided
    by n.  The device writes every squared term and sums each program's row
    in numpy.sum's own order (GPE_MODE_SSE_NUMPY: pairwise blocks of 128
    inside 8192-element chunks), so the sum is bit-identical to numpy's
    for identical terms; nan and inf propagate as they do there."""
    mode = _lib.GPE_MODE_SSE_NUMPY
    outputs = ("hi",)            # what finish_all reads (gpe_run copies)

    @classmethod
    def linspace(cls, n=10000):
        """The reference example's ``samples``/``values``."""
        from .datasets import symbreg_numpy_points
        X, V = symbreg_numpy_points(n)
        return cls(X, V)

    def finish(self, i, hi, lo, err, flags):
        return (float(hi),)

    def finish_all(self, hi, lo, err, flags):
        return _tuples1(hi, False)


class SymbRegSumSSE(SymbRegMSE):
    """``(sum((f(x) - target)**2 for each case),)`` with Python's builtin
    ``sum`` (left to right from 0, no division) — the evaluation of
    ``examples/gp/adf_symbreg.py:117-125``.  Exceptions as in
    :class:`SymbRegMSE` (``math.sin/cos(inf)``, ``d**2`` overflow); an
    overflowing sum is ``inf`` (no ``fsum`` error).  The device sums each
    program's terms in the same order (GPE_MODE_SSE_SEQ), bit for bit."""
    mode = _lib.GPE_MODE_SSE_SEQ

    @classmethod
    def adf_quartic(cls):
        from .datasets import adf_symbreg_points
        X, T = adf_symbreg_points()
        return cls(X, T)

    def finish(self, i, hi, lo, err, flags):
        if err != _lib.GPE_NO_ERROR:
            return SymbRegMSE.finish(self, i, hi, lo, err, flags)
        return (float(hi),)

    def finish_all(self, hi, lo, err, flags):
        out = _tuples1(hi, False)
        for i in np.flatnonzero(err != np.uint64(_lib.GPE_NO_ERROR)).tolist():
            out[i] = self.finish(i, hi[i], lo[i], err[i], flags[i])
        return out


def _two_prod_squares(y):
    """``(p, e)`` with ``p + e == y * y`` exactly (Dekker's product on
    Veltkamp halves; *y* within 2**-400 .. 2**400 in magnitude, or 0)."""
    p = y * y
    c = 134217729.0 * y
    yh = c - (c - y)
    yl = y - yh
    e = ((yh * yh - p) + yh * yl + yl * yh) + yl * yl
    return p, e


def exact_dd_sums(y):
    """``((Sy hi, lo), (Syy hi, lo))``: the exact ``sum(y)`` and
    ``sum(y * y)`` of a float64 column as double-doubles — hi the correctly
    rounded sum (``math.fsum``), lo the correctly rounded residual."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if not np.isfinite(y).all():
        raise ValueError("the target column must be finite")
    vals = y.tolist()
    sy = math.fsum(vals)
    sy_lo = math.fsum(vals + [-sy])
    mag = np.abs(y[y != 0.0])
    if len(mag) and (mag.min() < 2.0 ** -400 or mag.max() > 2.0 ** 400):
        from fractions import Fraction
        exact = sum(Fraction(v) ** 2 for v in vals)
        with np.errstate(over="ignore"):
            syy = float(exact) if exact < Fraction(2) ** 1024 else math.inf
        if math.isinf(syy):
            raise ValueError("the target column's sum of squares overflows")
        return (sy, sy_lo), (syy, float(exact - Fraction(syy)))
    p, e = _two_prod_squares(y)
    parts = p.tolist() + e.tolist()
    syy = math.fsum(parts)
    return (sy, sy_lo), (syy, math.fsum(parts + [-syy]))


class SymbRegScaledMSE(SymbRegMSE):
    """Linear-scaling fitness (Keijzer 2003): ``(mse,)`` of the best affine
    fit ``a + b * f(x)`` to the target ``y``, from one moments run
    (``gpe_run_scaled``).

    With ``Sf = sum f``, ``Sff = sum f*f``, ``Sfy = sum f*y`` (the device's
    double-double sums), ``Sy``, ``Syy`` (exact, from the host) and
    ``vf = Sff - Sf**2/n``, ``vy = Syy - Sy**2/n``, ``cfy = Sfy - Sf*Sy/n``:
    ``b = cfy/vf``, ``a = (Sy - b*Sf)/n``, ``mse = (vy - cfy**2/vf)/n``.  Two
    rules belong to the definition: an individual with an inf, nan or
    ``|f| >= 2**500`` output has fitness ``inf`` (``b = 0``, ``a = Sy/n``, no
    exception), and one with ``n*vf <= 2**-40 * Sff`` counts as constant
    (``b = 0``, ``a = Sy/n``, ``mse = vy/n``).  A case whose call raises
    (``math.sin(inf)``, ``math.sqrt(-1)``, ``float(int)`` overflow) raises for
    that individual, as in :class:`SymbRegMSE`.  The coefficients of the last
    evaluation are ``GPUEvaluator.last_scaling``.

    fp64, one target column, Python-semantics untyped primitive sets, one
    GPU.  The library reduces the programs' per-case values in chunks of
    programs that fit its scratch budget (``GPE_MOMENTS_MB``, 16 GiB)."""
    scaled = True

    def __init__(self, X, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim == 2 and y.shape[0] != 1:
            raise ValueError("SymbRegScaledMSE takes one target column")
        SymbRegMSE.__init__(self, X, y)
        self.sy, self.syy = exact_dd_sums(self.terms[0])

    def finish(self, i, hi, lo, err, flags):
        if err != _lib.GPE_NO_ERROR:
            return _case_error(err)
        return (float(hi),)

    def finish_all(self, hi, lo, err, flags):
        out = _tuples1(hi, False)
        for i in np.flatnonzero(err != np.uint64(_lib.GPE_NO_ERROR)).tolist():
            out[i] = _case_error(err[i])
        return out


class SymbRegAbsError(SymbRegMSE):
    """Absolute-error fitness from one GPU pass (``gpe_run_abserr``).  With
    ``e_i = abs(f(*row_i) - t0_i - t1_i - ...)`` (the terms subtracted left to
    right, as :class:`SymbRegMSE` without the square):

    * ``"mae"``: ``math.fsum(e) / n``;
    * ``"max"``: ``float(numpy.max(e))`` — nan if any ``e_i`` is nan, else the
      largest (inf included);
    * ``"hits"``: Koza's hits, ``sum(1 for v in e if v <= hit_eps)`` as an
      ``int``; a nan or inf ``e_i`` is never a hit, also with
      ``hit_eps = inf``.

    *fitness* is a non-empty tuple drawn from those names: the fitness tuple's
    entries, in that order.  A case whose call raises (``math.sin(inf)``,
    ``math.sqrt(-1)``, ``float(int)`` overflow) raises for that individual, as
    in :class:`SymbRegMSE`; there is no ``d**2``, so no ``OverflowError`` from
    a large difference.  ``fsum`` as :meth:`SymbRegMSE.finish` states it: all
    ``e_i`` finite and the sum overflows: ``OverflowError("intermediate
    overflow in fsum")`` (whatever *fitness* names: the reference computes
    all three); some ``e_i`` inf and none nan: ``mae = inf``; some nan:
    ``mae = nan``.  After an evaluation ``GPUEvaluator.last_mae``,
    ``last_max_error`` (float64) and ``last_hits`` (int64) hold all three per
    individual (nan / -1 for one that raised).

    fp64, Python-semantics untyped primitive sets, one GPU."""
    abs_error = True
    NAMES = ("mae", "max", "hits")

    def __init__(self, X, terms, hit_eps=0.01, fitness=("mae",)):
        SymbRegMSE.__init__(self, X, terms)
        hit_eps = float(hit_eps)
        if not hit_eps >= 0.0:
            raise ValueError("hit_eps must be >= 0 (got %r)" % hit_eps)
        if isinstance(fitness, str):
            fitness = (fitness,)
        fitness = tuple(fitness)
        if not fitness or any(k not in self.NAMES for k in fitness):
            raise ValueError("fitness must be a non-empty tuple drawn from "
                             "%r (got %r)" % (self.NAMES, fitness))
        self.hit_eps = hit_eps
        self.fitness = fitness

    def figures(self, w4, err, flags):
        """``(mae, max, hits)`` arrays (float64, float64, int64) of a batch's
        abs-error words ``[n, 4]``; nan / -1 where the individual raises (a
        first error, or an fsum overflow)."""
        w4 = np.asarray(w4, dtype=np.float64).reshape(-1, 4)
        flags = np.asarray(flags)
        nan_t = (flags & _lib.GPE_FLAG_NAN_TERM) != 0
        inf_t = ((flags & _lib.GPE_FLAG_INF_TERM) != 0) & ~nan_t
        with np.errstate(all="ignore"):
            mae = w4[:, 0] / self.n_cases
        mx = w4[:, 2].copy()
        mae[inf_t] = mx[inf_t] = math.inf
        mae[nan_t] = mx[nan_t] = math.nan
        hits = w4[:, 3].astype(np.int64)
        raised = (np.asarray(err) != np.uint64(_lib.GPE_NO_ERROR)) | (
            ~np.isfinite(w4[:, 0]) & ~nan_t & ~inf_t)
        mae[raised] = mx[raised] = math.nan
        hits[raised] = -1
        return mae, mx, hits

    def finish(self, i, w4, lo, err, flags):
        if err != _lib.GPE_NO_ERROR:
            return _case_error(err)
        mae, mx, hits = self.figures(w4, [err], [flags])
        if hits[0] < 0:
            return OverflowError("intermediate overflow in fsum")
        vals = {"mae": float(mae[0]), "max": float(mx[0]), "hits": int(hits[0])}
        return tuple(vals[k] for k in self.fitness)

    def finish_all(self, w4, lo, err, flags):
        mae, mx, hits = self.figures(w4, err, flags)
        cols = {"mae": mae.tolist(), "max": mx.tolist(), "hits": hits.tolist()}
        out = list(zip(*[cols[k] for k in self.fitness]))
        for i in np.flatnonzero(hits < 0).tolist():
            out[i] = self.finish(i, w4[i], None, err[i], flags[i])
        return out


class SymbRegCaseAbsErrors(SymbRegAbsError):
    """Per-case absolute errors ``e_c = abs(f(*row_c) - t0_c - t1_c - ...)``
    for epsilon-lexicase selection, with :class:`SymbRegAbsError`'s summaries
    from the same GPU pass (``gpe_run_abserr_cases``).  Automatic
    epsilon-lexicase takes its epsilon from the median absolute deviation of a
    case's errors, which does not commute with squaring: selection on these
    differs from selection on :class:`SymbRegCaseErrors`' squared errors.

    *cases* ``"host"`` (default): an individual's fitness is
    ``tuple(e_0 ... e_{n-1})``, one value per case (weights
    ``(-1.0,) * n_cases``), as :class:`SymbRegCaseErrors` returns squared
    ones; ``tools.selLexicase*`` and ``tools.sel*LexicaseGPU`` select on it
    unchanged.  ``"device"``: no ``n x n_cases`` copy is made; the matrix
    stays on the GPU for :meth:`GPUEvaluator.select_lexicase` and the fitness
    tuple is the summary *fitness* names, as in :class:`SymbRegAbsError`.
    Either way ``last_mae``, ``last_max_error`` and ``last_hits`` are filled,
    :meth:`GPUEvaluator.select_lexicase` works, and exceptions and refusals
    are :class:`SymbRegAbsError`'s."""
    abs_cases = True

    def __init__(self, X, terms, hit_eps=0.01, cases="host",
                 fitness=("mae",)):
        SymbRegAbsError.__init__(self, X, terms, hit_eps, fitness)
        if cases not in ("host", "device"):
            raise ValueError("cases must be 'host' or 'device' (got %r)"
                             % (cases,))
        self.cases = cases

    def finish(self, i, w4, lo, err, flags, cases=None):
        res = SymbRegAbsError.finish(self, i, w4, lo, err, flags)
        if self.cases == "device" or isinstance(res, BaseException):
            return res
        return tuple(np.asarray(cases, dtype=np.float64).tolist())

    def finish_all(self, w4, lo, err, flags, cases=None):
        out = SymbRegAbsError.finish_all(self, w4, lo, err, flags)
        if self.cases == "device":
            return out
        rows = np.asarray(cases, dtype=np.float64).tolist()
        return [res if isinstance(res, BaseException) else tuple(row)
                for res, row in zip(out, rows)]


def _check_scaled_setup(spec, pset, flattener, precision):
    """A moments-route spec's evaluator (linear scaling, absolute error): what
    it refuses, and why."""
    name = type(spec).__name__
    if precision == "fp32":
        raise ValueError(
            "%s is fp64 only: %s" % (name, "a one-pass variance has no digits "
                                     "to spare in precision='fp32'"
                                     if getattr(spec, "scaled", False) else
                                     "its kernels are the exact fp64 cores' "
                                     "(no precision='fp32')"))
    sems = set(flattener.spec.prim_ops.values())
    np_sems = sorted(s for s in sems if s.startswith("np"))
    if np_sems:
        raise NotImplementedError(
            "%s needs Python-semantics primitives; this set has "
            "numpy-semantics ones (%s), whose sin/cos(inf) and division are "
            "values, not errors" % (name, ", ".join(np_sems)))
    for p in (pset if isinstance(pset, (list, tuple)) else [pset]):
        if getattr(p, "ret", object) is not object:
            raise NotImplementedError(
                "%s does not take a typed primitive set (%s "
                "returns %r): the %s run covers float programs only"
                % (name, getattr(p, "name", "pset"), p.ret,
                   "moments" if getattr(spec, "scaled", False) else "abs-error"))


class SymbRegCaseErrors(SymbRegMSE):
    """``tuple((f(*row) - t0 - ...)**2 for each case)`` — one fitness value
    per case, for lexicase selection (reference ``selLexicase`` and its
    epsilon variants, ``deap/tools/selection.py:214-320``, read
    ``fitness.values[case]``; the individual's weights are one per case).
    The device writes the per-case terms of the same reduction
    (``gpe_run_cases``)."""
    per_case = True

    def finish(self, i, hi, lo, err, flags, cases=None):
        if err != _lib.GPE_NO_ERROR:
            return SymbRegMSE.finish(self, i, hi, lo, err, flags)
        return tuple(cases.tolist())


def pack_bitplanes(bits):
    """``bits[n_rows, n_cases]`` in {0,1} → ``uint32[n_rows, ceil(n/32)]``,
    case c at bit c % 32 of word c // 32."""
    bits = np.asarray(bits, dtype=np.uint8)
    if bits.ndim == 1:
        bits = bits[None, :]
    n_rows, n = bits.shape
    n_words = (n + 31) // 32
    padded = np.zeros((n_rows, n_words * 32), dtype=np.uint64)
    padded[:, :n] = bits
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    words = (padded.reshape(n_rows, n_words, 32) * weights).sum(axis=2)
    return words.astype(np.uint32)


def unpack_bitplanes(planes, n_cases):
    """The inverse of :func:`pack_bitplanes`: ``uint32[n_rows, ceil(n/32)]``
    → ``bool[n_rows, n_cases]`` (the pad bits of the last word dropped)."""
    planes = np.ascontiguousarray(planes, dtype=np.uint32)
    if planes.ndim == 1:
        planes = planes[None, :]
    if sys.byteorder == "little":
        # a word's bytes in memory order are cases 0-7, 8-15, ...: one byte
        # per case at once, with no uint32 per case in between (the host
        # side of last_case_hits at 16,384 x 4,601 is this function)
        bits = np.unpackbits(planes.view(np.uint8), axis=1, bitorder="little")
        return bits[:, :n_cases].astype(bool)
    shifts = np.arange(32, dtype=np.uint32)
    bits = (planes[:, :, None] >> shifts) & np.uint32(1)
    return bits.reshape(planes.shape[0], -1)[:, :n_cases].astype(bool)


# ------------------------------------------------------ predict helpers --
def plan_predict_chunks(n, row_bytes, max_bytes):
    """``[(lo, hi), ...]`` covering ``range(n)`` in order: as many
    individuals per run as keep its output (``row_bytes`` each) within
    ``max_bytes``, but at least one (a single row past the budget runs
    alone)."""
    per = max(1, int(max_bytes) // max(1, int(row_bytes)))
    return [(lo, min(n, lo + per)) for lo in range(0, n, per)]


def first_error_cases(err):
    """``int64[n]``: each program's first erroring case from a values run's
    error words (``(case << 2) | type``), -1 where it has none."""
    err = np.asarray(err, dtype=np.uint64)
    out = (err >> np.uint64(2)).astype(np.int64)
    out[err == np.uint64(_lib.GPE_NO_ERROR)] = -1
    return out


def predict_error(err, offset=0):
    """The reference's exception for the first individual (in order) whose
    error word says a case raised, its message naming the individual
    (``offset`` + position) and the case; None when no case raised."""
    err = np.asarray(err, dtype=np.uint64)
    bad = np.flatnonzero(err != np.uint64(_lib.GPE_NO_ERROR))
    if not len(bad):
        return None
    i = int(bad[0])
    exc = _case_error(err[i])
    where = "individual %d, case %d: " % (offset + i, int(err[i]) >> 2)
    if isinstance(exc, OverflowError):
        return OverflowError(where + "int too large to convert to float")
    return type(exc)(where + str(exc))


class BooleanHits(object):
    """``(sum(func(*in_) == out for in_, out in zip(inputs, outputs)),)``
    (multiplexer.py:75, parity.py:68) on 0/1 inputs, bit-sliced."""
    machine = Machine.B
    mode = _lib.GPE_MODE_HITS_BITS
    outputs = ("hi",)

    def __init__(self, inputs, outputs):
        ins = np.asarray(inputs)
        outs = np.asarray(outputs)
        if ins.ndim != 2 or outs.shape != (ins.shape[1],):
            raise ValueError("inputs must be [n_vars, n_cases], outputs "
                             "[n_cases]")
        if not (np.isin(ins, (0, 1)).all() and np.isin(outs, (0, 1)).all()):
            raise NotImplementedError("bit-sliced evaluation needs 0/1 data")
        self.n_cases = ins.shape[1]
        self.planes = pack_bitplanes(ins)
        self.out_plane = pack_bitplanes(outs)[0]

    @classmethod
    def from_rows(cls, inputs, outputs):
        """Reference layout: ``inputs[case][var]``, ``outputs[case]``."""
        return cls(np.asarray(inputs).T, np.asarray(outputs))

    def upload(self, ctx):
        ctx.set_bitplanes(self.planes, self.out_plane, self.n_cases)

    def subset(self, idx):
        """As :meth:`SymbRegMSE.subset`: the planes of cases *idx*."""
        sub = copy.copy(self)
        sub.n_cases = len(idx)
        sub.planes = pack_bitplanes(
            unpack_bitplanes(self.planes, self.n_cases)[:, idx])
        sub.out_plane = pack_bitplanes(
            unpack_bitplanes(self.out_plane, self.n_cases)[:, idx])[0]
        return sub

    def finish(self, i, hi, lo, err, flags):
        return (int(hi),)

    def finish_all(self, hi, lo, err, flags):
        return _tuples1(hi, True)


class BooleanCaseHits(BooleanHits):
    """Per-case hits ``int(func(*in_) == out)`` of a boolean problem, for
    lexicase selection, with :class:`BooleanHits`' count from the same GPU
    pass (``gpe_run_hit_planes``): one bit per individual and case, stored by
    the bit-sliced kernels next to the popcount.

    *cases* ``"host"`` (default): an individual's fitness is
    ``tuple(int(func(*in_) == out) for in_, out in zip(inputs, outputs))``,
    ``n_cases`` ints 0/1 (weights ``(1.0,) * n_cases``); ``tools.selLexicase``
    and ``tools.selLexicaseGPU`` select on it unchanged.  ``"device"``: no
    ``n x n_cases`` matrix is allocated or copied; the fitness is ``(hits,)``
    as :class:`BooleanHits` gives it and the bit matrix stays on the GPU for
    :meth:`GPUEvaluator.select_lexicase`.  Either way ``last_hits`` (int64) is
    filled, :meth:`GPUEvaluator.last_case_hits` reads the matrix back on
    request and :meth:`GPUEvaluator.select_lexicase` works.  Validation,
    :meth:`from_rows` and :meth:`subset` are :class:`BooleanHits`'; typed
    primitive sets (spambase runs on the F machine's typed core) are
    refused."""
    hit_planes = True

    def __init__(self, inputs, outputs, cases="host"):
        BooleanHits.__init__(self, inputs, outputs)
        if cases not in ("host", "device"):
            raise ValueError("cases must be 'host' or 'device' (got %r)"
                             % (cases,))
        self.cases = cases

    @classmethod
    def from_rows(cls, inputs, outputs, cases="host"):
        """Reference layout: ``inputs[case][var]``, ``outputs[case]``."""
        return cls(np.asarray(inputs).T, np.asarray(outputs), cases)

    def finish(self, i, hi, lo, err, flags, cases=None):
        if self.cases == "device":
            return (int(hi),)
        return tuple(unpack_bitplanes(cases, self.n_cases)[0]
                     .astype(np.int64).tolist())

    def finish_all(self, hi, lo, err, flags, cases=None):
        if self.cases == "device":
            return _tuples1(hi, True)
        if not len(hi):
            return []
        rows = unpack_bitplanes(cases, self.n_cases).astype(np.int64).tolist()
        return [tuple(row) for row in rows]


class TypedBoolHits(object):
    """``(sum(bool(func(*row)) is bool(label) for row, label ...),)``
    (spambase.py:86) evaluated on every row."""
    machine = Machine.F
    mode = _lib.GPE_MODE_HITS_BOOL
    outputs = ("hi", "err")
    # with no exact-integer pass and no sin/cos or sqrt (ValueError) no case
    # can error: the counts alone
    outputs_plain = ("hi",)

    def __init__(self, X, labels):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.labels = (np.asarray(labels) != 0).astype(np.float64)[None, :]
        self.n_cases = self.X.shape[1]

    def upload(self, ctx):
        ctx.set_cases(_lib.GPE_MACHINE_F, self.X, self.labels)

    def subset(self, idx):
        """As :meth:`SymbRegMSE.subset`: the rows and labels of cases *idx*."""
        sub = copy.copy(self)
        sub.X = np.ascontiguousarray(self.X[:, idx])
        sub.labels = np.ascontiguousarray(self.labels[:, idx])
        sub.n_cases = sub.X.shape[1]
        return sub

    def finish(self, i, hi, lo, err, flags):
        # (errors only from the exact-integer pass: float(int) overflow)
        if err != _lib.GPE_NO_ERROR:
            return _case_error(err)
        return (int(hi),)

    def finish_all(self, hi, lo, err, flags):
        out = _tuples1(hi, True)
        if err is not None:
            for i in np.flatnonzero(err != np.uint64(_lib.GPE_NO_ERROR)).tolist():
                out[i] = _case_error(err[i])
        return out


class TypedCaseHits(TypedBoolHits):
    """Per-case hits ``bool(func(*row)) is bool(label)`` of a typed
    classifier (spambase.py:70), for lexicase selection and informed
    down-sampling, with :class:`TypedBoolHits`' count from the same GPU pass
    (``gpe_run_typed_hit_planes``): one bit per individual and case, stored
    by the typed core's hit-planes variant, by the C++ kernels (programs past
    the core's five stack slots), by a fill (one-constant programs) and by the
    exact-integer pass, each next to its count.

    *cases* ``"host"`` (default): an individual's fitness is
    ``tuple(int(bool(func(*row)) is bool(label)) for row, label in ...)``,
    ``n_cases`` ints 0/1 (weights ``(1.0,) * n_cases``) for
    ``tools.selLexicase*``.  ``"device"``: no ``n x n_cases`` matrix is
    allocated or copied; the fitness is ``(hits,)`` as :class:`TypedBoolHits`
    gives it and the bit matrix stays on the GPU.  Either way ``last_hits``
    (int64) is filled and :meth:`GPUEvaluator.last_case_hits`,
    :meth:`GPUEvaluator.select_lexicase` (every mode, *parallel* too),
    :meth:`GPUEvaluator.informed_subsample` and
    :meth:`GPUEvaluator.subsample` work as for :class:`BooleanCaseHits`.  An
    individual that raises (the exact pass's ``OverflowError``, a tree taller
    than the parser allows) is returned in its place.  fp64, one GPU."""
    hit_planes = True
    typed_planes = True

    def __init__(self, X, labels, cases="host"):
        TypedBoolHits.__init__(self, X, labels)
        if cases not in ("host", "device"):
            raise ValueError("cases must be 'host' or 'device' (got %r)"
                             % (cases,))
        self.cases = cases

    def finish(self, i, hi, lo, err, flags, cases=None):
        if err is not None and err != _lib.GPE_NO_ERROR:
            return _case_error(err)
        if self.cases == "device":
            return (int(hi),)
        return tuple(unpack_bitplanes(cases, self.n_cases)[0]
                     .astype(np.int64).tolist())

    def finish_all(self, hi, lo, err, flags, cases=None):
        if self.cases == "device":
            return TypedBoolHits.finish_all(self, hi, lo, err, flags)
        if not len(hi):
            return []
        rows = unpack_bitplanes(cases, self.n_cases).astype(np.int64).tolist()
        out = [tuple(row) for row in rows]
        if err is not None:
            for i in np.flatnonzero(err != np.uint64(_lib.GPE_NO_ERROR)).tolist():
                out[i] = _case_error(err[i])
        return out


CONFUSION_NAMES = ("tp", "fp", "fn", "tn", "hits", "accuracy", "recall",
                   "specificity", "precision", "balanced_accuracy", "f1",
                   "mcc")


def confusion_figures(conf, names=CONFUSION_NAMES):
    """The class-aware figures of confusion counts ``int64[n, 4]`` in the
    order tp, fp, fn, tn → ``{name: array[n]}`` for *names* (int64 for the
    five counts, float64 for the rest).  With ``P = tp + fn`` and
    ``N = fp + tn``, every operation an IEEE double one on the integers:

    * ``hits = tp + tn``; ``accuracy = (tp + tn) / (P + N)``;
    * ``recall = tp / P``, ``0.0`` when ``P == 0``;
    * ``specificity = tn / N``, ``0.0`` when ``N == 0``;
    * ``precision = tp / (tp + fp)``, ``0.0`` when that sum is 0;
    * ``balanced_accuracy = (recall + specificity) / 2``; specificity alone
      when ``P == 0``, recall alone when ``N == 0``;
    * ``f1 = (2 * tp) / (2 * tp + fp + fn)``, ``0.0`` when the denominator
      is 0;
    * ``mcc = float(tp * tn - fp * fn) / (math.sqrt(float((tp + fp) *
      (tp + fn))) * math.sqrt(float((tn + fp) * (tn + fn))))``, ``0.0`` when
      either product is 0 (the products are exact integers: the counts are
      below 2^31).

    A row of ``-1`` (an individual that raised) gives figures without
    meaning; the caller replaces them."""
    conf = np.asarray(conf, dtype=np.int64).reshape(-1, 4)
    tp, fp, fn, tn = conf[:, 0], conf[:, 1], conf[:, 2], conf[:, 3]
    P, N = tp + fn, fp + tn
    zeros = np.zeros(len(conf))
    cols = {}
    with np.errstate(all="ignore"):
        def ratio(num, den):
            return np.where(den == 0, zeros, num / den)
        for name in names:
            if name in cols:
                continue
            if name in ("tp", "fp", "fn", "tn"):
                cols[name] = conf[:, ("tp", "fp", "fn", "tn").index(name)]
            elif name == "hits":
                cols[name] = tp + tn
            elif name == "accuracy":
                cols[name] = (tp + tn) / (P + N)
            elif name == "recall":
                cols[name] = ratio(tp, P)
            elif name == "specificity":
                cols[name] = ratio(tn, N)
            elif name == "precision":
                cols[name] = ratio(tp, tp + fp)
            elif name == "balanced_accuracy":
                rec, spe = ratio(tp, P), ratio(tn, N)
                cols[name] = np.where(P == 0, spe,
                                      np.where(N == 0, rec, (rec + spe) / 2))
            elif name == "f1":
                cols[name] = ratio(2 * tp, 2 * tp + fp + fn)
            elif name == "mcc":
                a, b = (tp + fp) * (tp + fn), (tn + fp) * (tn + fn)
                num = (tp * tn - fp * fn).astype(np.float64)
                den = np.sqrt(a.astype(np.float64)) * \
                    np.sqrt(b.astype(np.float64))
                cols[name] = np.where((a == 0) | (b == 0), zeros, num / den)
            else:
                raise ValueError("unknown confusion figure %r (the names are "
                                 "%r)" % (name, CONFUSION_NAMES))
    return cols


class _Confusion(object):
    """What :class:`TypedConfusion` and :class:`BooleanConfusion` share: the
    *fitness* names, the confusion counts from the hits and the label-plane
    count, and the vectorised fitness tuples."""
    confusion = True
    NAMES = CONFUSION_NAMES
    cases = "device"

    def _set_fitness(self, fitness):
        if isinstance(fitness, str):
            fitness = (fitness,)
        fitness = tuple(fitness)
        if not fitness or any(k not in self.NAMES for k in fitness):
            raise ValueError("fitness must be a non-empty tuple drawn from "
                             "%r (got %r)" % (self.NAMES, fitness))
        self.fitness = fitness

    def confusion_counts(self, hits, tp, err=None):
        """``int64[n, 4]`` (tp, fp, fn, tn) from the hit counts, the hits on
        the positive cases (the label plane's masked count) and the error
        words; ``-1`` rows where the individual raised."""
        hits = np.asarray(hits).astype(np.int64).reshape(-1)
        tp = np.asarray(tp, dtype=np.int64).reshape(-1)
        P = int(self.positives())
        N = self.n_cases - P
        tn = hits - tp
        conf = np.stack([tp, N - tn, P - tp, tn], axis=1)
        if err is not None:
            conf[np.asarray(err) != np.uint64(_lib.GPE_NO_ERROR)] = -1
        return conf

    def finish(self, i, hi, lo, err, flags, cases=None):
        return self.finish_all(np.asarray([hi]), None,
                               None if err is None else
                               np.asarray([err], dtype=np.uint64), None,
                               cases=np.asarray([cases]).reshape(-1))[0]

    def finish_all(self, hi, lo, err, flags, cases=None):
        # (cases: the label plane's masked counts, the true positives)
        if not len(hi):
            return []
        conf = self.confusion_counts(hi, cases, err)
        cols = confusion_figures(conf, self.fitness)
        out = list(zip(*[cols[k].tolist() for k in self.fitness]))
        if err is not None:
            for i in np.flatnonzero(err != np.uint64(_lib.GPE_NO_ERROR)).tolist():
                out[i] = _case_error(err[i])
        return out


class TypedConfusion(_Confusion, TypedCaseHits):
    """Class-aware fitness of a typed classifier (spambase.py) from the hit
    planes :class:`TypedCaseHits` leaves on the GPU: after the hit-planes run
    one masked count (``gpe_hit_group_counts`` with the label plane) gives
    each individual's hits on the positive rows.  With ``P`` the number of
    positive labels, ``N = n_cases - P`` and ``hits`` the count
    :class:`TypedBoolHits` returns: ``tp`` is that count, ``tn = hits - tp``,
    ``fn = P - tp``, ``fp = N - tn``.

    *fitness* is a non-empty tuple drawn from ``"tp" "fp" "fn" "tn" "hits"``
    (ints) and ``"accuracy" "recall" "specificity" "precision"
    "balanced_accuracy" "f1" "mcc"`` (floats): the fitness tuple's entries in
    that order, by the definitions of :func:`confusion_figures`:

    * ``accuracy = (tp + tn) / (P + N)``
    * ``recall = tp / P``, ``0.0`` when ``P == 0``
    * ``specificity = tn / N``, ``0.0`` when ``N == 0``
    * ``precision = tp / (tp + fp)``, ``0.0`` when that sum is 0
    * ``balanced_accuracy = (recall + specificity) / 2``; when ``P == 0``
      specificity alone, when ``N == 0`` recall alone
    * ``f1 = (2 * tp) / (2 * tp + fp + fn)``, ``0.0`` when the denominator
      is 0
    * ``mcc = float(tp * tn - fp * fn) / (math.sqrt(float((tp + fp) *
      (tp + fn))) * math.sqrt(float((tn + fp) * (tn + fn))))``, ``0.0`` when
      either product is 0

    each an IEEE double operation on Python ints.  There is no *cases*
    argument: the matrix stays on the GPU as with ``cases="device"``, and
    :meth:`GPUEvaluator.select_lexicase` (every mode, *parallel* too),
    :meth:`GPUEvaluator.informed_subsample`, :meth:`GPUEvaluator.subsample`,
    :meth:`GPUEvaluator.last_case_hits`, :meth:`GPUEvaluator.group_hits` and
    ``last_hits`` work as for :class:`TypedCaseHits`.
    ``GPUEvaluator.last_confusion`` is ``int64[n, 4]`` in the order tp, fp,
    fn, tn (a row of ``-1`` where the individual raised).  Exceptions and
    setup refusals are :class:`TypedCaseHits`'.  fp64, one GPU."""

    def __init__(self, X, labels, fitness=("balanced_accuracy",)):
        TypedCaseHits.__init__(self, X, labels, "device")
        self._set_fitness(fitness)

    def label_plane(self):
        """``uint32[ceil(n_cases / 32)]``: bit c set where label c is true."""
        return pack_bitplanes(self.labels[0] != 0)[0]

    def positives(self):
        return int(np.count_nonzero(self.labels[0]))


class BooleanConfusion(_Confusion, BooleanCaseHits):
    """:class:`TypedConfusion`'s figures for a boolean problem (the positive
    cases are those whose output is 1), from :class:`BooleanCaseHits`' hit
    planes and one masked count with the output plane.  *fitness*, the
    definitions, ``last_confusion`` and what keeps working are
    :class:`TypedConfusion`'s; validation, :meth:`from_rows` and the refusal
    of typed primitive sets are :class:`BooleanCaseHits`'."""

    def __init__(self, inputs, outputs, fitness=("balanced_accuracy",)):
        BooleanCaseHits.__init__(self, inputs, outputs, "device")
        self._set_fitness(fitness)

    @classmethod
    def from_rows(cls, inputs, outputs, fitness=("balanced_accuracy",)):
        """Reference layout: ``inputs[case][var]``, ``outputs[case]``."""
        return cls(np.asarray(inputs).T, np.asarray(outputs), fitness)

    def label_plane(self):
        """``uint32[ceil(n_cases / 32)]``: bit c set where output c is 1."""
        return self.out_plane

    def positives(self):
        return int(unpack_bitplanes(self.out_plane, self.n_cases).sum())


# ------------------------------------------------------------- evaluator --
def trig_leaf_columns(pset_spec, spec, precision="fp64"):
    """Argument indices whose sin/cos leaves may be read from device columns:
    an F-machine spec whose case matrix holds one row per pset argument, and
    a finite column (math.sin/cos(+-inf) raises, so such leaves stay in the
    program where the error is reported at its first case) — in fp32 mode
    finite after the float cast the fp32 machine applies."""
    X = getattr(spec, "X", None)
    if not pset_spec.has_trig or spec.machine != Machine.F or X is None \
            or X.shape[0] != len(pset_spec.arg_index):
        return ()
    if precision == "fp32":
        with np.errstate(over="ignore"):
            X = X.astype(np.float32)
    return tuple(int(v) for v in np.flatnonzero(np.isfinite(X).all(axis=1)))


class _Rows(object):
    """The rows of ``predict(X=...)`` as trig_leaf_columns reads a spec."""
    machine = Machine.F

    def __init__(self, X):
        self.X = X


def check_case_subset(idx, full_n_cases):
    """The index vector of :meth:`GPUEvaluator.subsample` as an int64 copy:
    1-D, at least one entry, integers in ``[0, full_n_cases)`` in any order,
    duplicates allowed.  ``ValueError`` for an empty, not 1-D or non-integer
    *idx*; ``IndexError`` naming the first entry out of range (a negative one
    included: no wrap-around)."""
    a = np.asarray(idx)
    if a.ndim != 1:
        raise ValueError("subsample: idx must be 1-D (got %d-D)" % a.ndim)
    if a.size == 0:
        raise ValueError("subsample: idx must name at least one case")
    if a.dtype.kind not in "iu":
        raise ValueError("subsample: idx must hold integers (got dtype %s)"
                         % a.dtype)
    bad = np.flatnonzero((a < 0) | (a >= full_n_cases))
    if len(bad):
        raise IndexError("subsample: idx[%d] = %d is outside [0, %d)"
                         % (bad[0], a[bad[0]], full_n_cases))
    return a.astype(np.int64)


def _default_device():
    return int(os.environ.get("LOCAL_RANK", "0"))


class GPUEvaluator(object):
    """Evaluates populations of one primitive set on one fitness spec.

    Calling it on a single individual evaluates a batch of one (the
    reference's direct ``toolbox.evaluate(ind)`` calls); :func:`gpu_map`
    routes whole populations through :meth:`map`.

    *pset* may be a list of primitive sets ``[main, adf_1, ...]`` — the
    ``psets`` of ``gp.compileADF`` (gp.py:490-513) — for individuals that
    are lists of trees (``examples/gp/adf_symbreg.py``).
    """

    def __init__(self, pset, spec, device=None, machine=None,
                 trig_leaves=True, precision="fp64", size_objective=False):
        """*precision* ``"fp64"`` (default) matches the reference (1e-12
        relative MSE); ``"fp32"`` evaluates the trees in single precision
        for throughput, with the agreement DESIGN.md §4 states.

        *size_objective* True appends ``len(individual)`` (an ADF
        individual: the sum of its trees' lengths) to every fitness tuple
        :meth:`evaluate`, :meth:`map` and a call return — the second
        objective of a parsimony run under ``tools.selNSGA2GPU``.  Exception
        entries pass through unchanged.  Specs whose tuple is one value per
        case (``cases="host"``, :class:`SymbRegCaseErrors`) refuse it."""
        if precision not in ("fp64", "fp32"):
            raise ValueError("precision must be 'fp64' or 'fp32'")
        if size_objective and (getattr(spec, "per_case", False) or
                               getattr(spec, "cases", None) == "host"):
            raise ValueError(
                "size_objective: the fitness tuple of %s is one value per "
                "case (lexicase selection reads it as such); a size has no "
                "place in it" % type(spec).__name__)
        self.size_objective = bool(size_objective)
        if getattr(spec, "typed_planes", False) and precision != "fp64":
            raise NotImplementedError(
                "%s needs precision='fp64': the typed core's hit planes are "
                "the fp64 machine's (gpe_run_typed_hit_planes)"
                % type(spec).__name__)
        if getattr(spec, "hit_planes", False) and \
                not getattr(spec, "typed_planes", False):
            for p in (pset if isinstance(pset, (list, tuple)) else [pset]):
                if getattr(p, "ret", object) is not object:
                    raise NotImplementedError(
                        "%s does not take a typed primitive set (%s returns "
                        "%r): typed programs run on the F machine's typed "
                        "core, which stores no hit planes"
                        % (type(spec).__name__, getattr(p, "name", "pset"),
                           p.ret))
        self.pset = pset
        self.spec = spec
        self.precision = precision
        machine = machine if machine is not None else spec.machine
        adf = isinstance(pset, (list, tuple))
        self.flattener = ADFFlattener(pset, machine) if adf else \
            Flattener(pset, machine)
        if self.flattener.machine != spec.machine:
            raise ValueError("fitness spec and primitive set need different "
                             "machines")
        if getattr(spec, "scaled", False) or getattr(spec, "abs_error", False):
            _check_scaled_setup(spec, pset, self.flattener, precision)
        self.ctx = _lib.Context(_default_device() if device is None
                                else device)
        spec.upload(self.ctx)
        # case subsampling (subsample): the spec the user passed (never
        # mutated; self.spec is it, or its subset() while one is active), the
        # active index vector, and how often case data left the host
        self._full_spec = spec
        self.case_subset = None
        self.full_n_cases = spec.n_cases
        self.case_uploads = 1
        if precision == "fp32":
            if spec.machine != Machine.F:
                raise ValueError("fp32 mode applies to the F machine only")
            self.ctx.set_precision(_lib.GPE_PREC_F32)
        # sin/cos of a bare argument: evaluated once per case on the device
        # (same function, same value) and read by every program
        leaves = trig_leaf_columns(self.flattener.spec, spec, precision) \
            if trig_leaves and not adf else ()
        if leaves:
            self.ctx.set_trig_leaves(True)
            self.flattener = Flattener(pset, machine, trig_leaves=leaves)
        self.stats = {"calls": 0, "individuals": 0, "node_evals": 0,
                      "flatten_s": 0.0, "device_s": 0.0, "kernel_ms": 0.0,
                      "device_lowered": 0}
        self._warned_inexact = False
        self._exact_flattener = None
        # device lowering (gpe_lower_programs): the host only reads each
        # node's pset entry; the register-machine words are built on the GPU
        self.device_lowering = not adf and \
            os.environ.get("GPE_DEVICE_LOWERING", "1") != "0"
        self._lowering_set = False
        # output arrays reused across evaluate calls (_lib.ResultBuffers)
        self._run_out = _lib.ResultBuffers()
        self._lw_out = _lib.LoweringBuffers()
        # the node offsets of a chunked lowering, reused when the batch
        # does not outlive the next lowering (keep=False: evaluate)
        self._lw_off = np.zeros(0, dtype=np.int64)
        # trees per chunk of a chunked device lowering (populations larger
        # than this are read and lowered in overlapping chunks)
        self.lower_chunk = int(os.environ.get("GPE_LOWER_CHUNK", 1 << 18))
        # predict(X=...): the sibling context holding the held-out rows, the
        # rows it holds, and how often rows were uploaded to it
        self._predict_ctx = None
        self._predict_X = None
        self._predict_leaves = False
        self.predict_uploads = 0
        self.last_predict_first_error = np.zeros(0, dtype=np.int64)
        # SymbRegScaledMSE: (a, b) float64 [n] of the last evaluation
        self.last_scaling = (np.zeros(0), np.zeros(0))
        # SymbRegAbsError: all three figures of the last evaluation
        self.last_mae = np.zeros(0)
        self.last_max_error = np.zeros(0)
        self.last_hits = np.zeros(0, dtype=np.int64)
        # TypedConfusion / BooleanConfusion: (tp, fp, fn, tn) per individual
        self.last_confusion = np.zeros((0, 4), dtype=np.int64)
        # select_lexicase: the individuals (kept, so that their identities
        # stay theirs) and results of the last evaluation that left a
        # per-case matrix on the GPU
        self._lex_batch = None
        # select_lexicase(parallel=True): the seed its last call drew
        self.last_lexicase_seed = None
        # select_dalex: the seed its last call drew
        self.last_dalex_seed = None
        # informed_subsample: each pick's distance to the nearest earlier one
        self.last_informed_distances = np.zeros(0, dtype=np.int32)
        # shared_hits: how many individuals solve each case
        self.last_solve_counts = np.zeros(0, dtype=np.int64)

    def close(self):
        """Release the device contexts (the evaluator's and predict's)."""
        if self._predict_ctx is not None:
            self._predict_ctx.close()
            self._predict_ctx = None
            self._predict_X = None
        self.ctx.close()

    @property
    def n_cases(self):
        """The active case count (``full_n_cases`` with no subset)."""
        return self.spec.n_cases

    def subsample(self, idx):
        """Evaluate on cases *idx* of the resident set from now on, or on the
        whole set again (*idx* None): down-sampled lexicase, mini-batch
        fitness, bootstrap resampling.  *idx*: a 1-D integer sequence or
        array, values in ``[0, full_n_cases)``, any order, duplicates allowed,
        at least one entry, possibly more than ``full_n_cases``
        (:func:`check_case_subset`: ``IndexError`` out of range,
        ``ValueError`` empty, not 1-D or non-integer).

        The rows are gathered on the GPU (``gpe_select_cases``: no case data
        leaves the host, ``case_uploads`` stays 1).  Afterwards
        :meth:`evaluate` / :meth:`map`, ``predict(X=None)``,
        ``predict(scaled=True)``, ``last_scaling``, ``last_mae``,
        ``last_max_error``, ``last_hits``, :meth:`select_lexicase` and
        ``tools.selTournamentGPU`` on the resident fitness give what a fresh
        evaluator built on ``X[:, idx]``, ``terms[:, idx]`` gives — in fp64
        bit for bit, exceptions included.  A first-error case is a position
        in *idx* (``case_subset`` maps it back), the MSE / MAE divisor is
        ``len(idx)``.  ``predict(X=rows)`` is untouched.

        The loaded programs, their exact-int pass and the lowering tables are
        kept (one population can be run on several subsets without
        flattening again); the per-case matrix of the last evaluation is
        dropped, so :meth:`select_lexicase` needs an :meth:`evaluate`
        first.  The flattener's trig-leaf choice stays the full set's (a
        column finite on all cases is finite on any subset)."""
        if idx is None:
            self.ctx.select_cases(None)
            self.spec = self._full_spec
            self.case_subset = None
        else:
            idx = check_case_subset(idx, self.full_n_cases)
            sub = self._full_spec.subset(idx)
            self.ctx.select_cases(idx)
            self.spec = sub
            self.case_subset = idx
        self._lex_batch = None

    def informed_subsample(self, m, eps=None, apply=True):
        """Informed down-sampling (Boldi et al. 2023): choose *m* cases by a
        farthest-first traversal of the per-case matrix the last
        :meth:`evaluate` / :meth:`map` left on the GPU, and (with *apply*)
        :meth:`subsample` to them.  Returns the cases, ``int64[m]`` in pick
        order, no duplicates.

        Evaluate a sample of the parents on all cases first
        (``subsample(None)``; :class:`BooleanCaseHits`, :class:`TypedCaseHits`
        or :class:`SymbRegCaseAbsErrors`, either *cases* mode).  Two cases are
        as far apart as the number of those individuals that pass one and fail
        the other; for the regression spec a case is passed when its absolute
        error is finite and ``<= eps`` (default ``spec.hit_eps``; *eps* with
        :class:`BooleanCaseHits` is a ``ValueError``).  The first case is
        drawn at random, every further one is the case farthest from all
        chosen so far, so cases that the same individuals solve stop crowding
        the subset; once only duplicates of chosen cases remain, they follow
        in random order.  The exact rule, with its SplitMix64 tie-break keys,
        is ``gpe_informed_cases``' (include/gpeval.h); no ``n x n_cases`` copy
        leaves the GPU.

        ``seed = random.getrandbits(64)`` is the only draw from the module
        ``random`` stream.  ``last_informed_distances`` (int32 ``[m]``) holds
        each pick's distance to the nearest case picked before it (-1 for the
        first).  *apply* False changes nothing else: the per-case matrix still
        serves :meth:`select_lexicase`.  ``ValueError``: no per-case matrix of
        the full case set (or :class:`SymbRegCaseErrors`' squared errors), *m*
        outside ``[1, full_n_cases]``.  If an individual of the batch raised,
        its exception is raised here, the first in order."""
        def own():
            if not 1 <= m <= self.full_n_cases:
                raise ValueError("informed_subsample: m must be in [1, %d] "
                                 "(got %r)" % (self.full_n_cases, m))
        bits = getattr(self.spec, "hit_planes", False)
        last, results = self._last_batch(
            "informed_subsample", self.case_subset is None and
            (bits or getattr(self.spec, "abs_cases", False)),
            "it needs the per-case matrix of a BooleanCaseHits or "
            "SymbRegCaseAbsErrors evaluation on the full case set (the spec "
            "is %%s, %s, %s): subsample(None) and evaluate the parent sample "
            "first" % ("no per-case matrix is on the GPU"
                       if self._lex_batch is None else "a per-case matrix is "
                       "on the GPU", "no case subset is active"
                       if self.case_subset is None else "a case subset is "
                       "active"),
            eps=eps, hits_eps="BooleanCaseHits' cases are hits already",
            own=own)
        for res in results:
            if isinstance(res, BaseException):
                raise res
        if not last:
            raise ValueError("informed_subsample: the last evaluate / map "
                             "held no individuals")
        eps = self._hit_eps("informed_subsample", eps)
        seed = random.getrandbits(64)
        idx, dist = self.ctx.informed_cases(None, 0, 0, eps, seed, int(m))
        self.last_informed_distances = dist
        if apply:
            self.subsample(idx)
        return idx

    # the evaluator is used as toolbox.evaluate
    def __call__(self, individual):
        res = self.evaluate([individual])[0]
        if isinstance(res, BaseException):
            raise res
        return res

    def flatten(self, individuals):
        t0 = time.perf_counter()
        batch = self.flattener.flatten(individuals)
        self.stats["flatten_s"] += time.perf_counter() - t0
        self._warn_inexact(batch)
        return batch

    def lower_on_device(self, individuals, keep=True, lo=0, hi=None):
        """Read the trees' node codes on the host and lower them into the
        context's program buffers on the GPU.  Returns a :class:`ProgramBatch`
        without host words (``code`` None, already loaded), or None when the
        batch needs the host flattener (a node the native reader declines, a
        constant fold only Python can do, a pset of 255+ entries).  *keep*
        False: the batch is used only until the next lowering (its arrays
        stay in the evaluator's reused buffers).  *lo*, *hi*: lower only
        ``individuals[lo:hi]`` (read in place, no slice)."""
        hi = len(individuals) if hi is None else hi
        n = hi - lo
        if n > self.lower_chunk:
            return self._lower_chunked(individuals, keep, lo, hi)
        t0 = time.perf_counter()
        r = self.flattener.read_codes(individuals, lo, hi)
        self.stats["flatten_s"] += time.perf_counter() - t0
        if r is None:
            return None
        t0 = time.perf_counter()
        self._set_lowering()
        codes, node_off, evals, eph_off = r
        depth, err, status = self.ctx.lower_programs(codes, node_off, evals,
                                                     eph_off, out=self._lw_out)
        self.stats["device_s"] += time.perf_counter() - t0
        off = np.frombuffer(node_off, dtype=np.int64)
        return self._lowered_batch(off, depth, err, status, keep)

    def _set_lowering(self):
        if not self._lowering_set:
            self.ctx.set_lowering(*self.flattener.lowering_tables())
            self._lowering_set = True

    @staticmethod
    def _chunk_bounds(n, chunk, tail=None):
        """Chunk ends of a chunked lowering: equal chunks of at most
        ``chunk`` trees; with *tail*, the last ones halving (chunk / 2,
        chunk / 4, ... down to ``tail``).  Halving was meant to leave little
        device work after the host's last read, but each lower_trees launch
        has a ~0.4 ms floor (one wave lowering its 64 trees through
        dependent scratch accesses), so the small chunks cost more than they
        saved (C3 at pop 1M, same box: 9.4-10.9 ms without, 11.5-13.8 with
        a 2^14 tail).  ``GPE_LOWER_TAIL=N`` (N >= 1024) restores a tail."""
        env = os.environ.get("GPE_LOWER_TAIL", "")
        if tail is None and env.isdigit() and int(env) >= 1024:
            tail = int(env)
        halves = []
        c = chunk // 2 if tail else 0
        while tail and c >= tail and sum(halves) + c < n // 2:
            halves.append(c)
            c //= 2
        head = n - sum(halves)
        k = -(-head // chunk)
        ends = [head * (i + 1) // k for i in range(k)]
        for h in halves:
            ends.append(ends[-1] + h)
        return ends

    def _lower_chunked(self, individuals, keep=True, lo=0, hi=None):
        """lower_on_device in chunks of ``lower_chunk`` trees: the device
        uploads and lowers chunk i (gpe_lower_add, asynchronous) while the
        host reads chunk i + 1 (read_codes in place, no slices)."""
        hi = len(individuals) if hi is None else hi
        n = hi - lo
        self._set_lowering()
        if keep:
            off = np.empty(n + 1, dtype=np.int64)
        else:
            # (a fresh 8 MB array per call at pop 1M is fresh pages: their
            # first-touch faults and the unmapping)
            if len(self._lw_off) < n + 1:
                self._lw_off = np.empty(n + 1, dtype=np.int64)
            off = self._lw_off[:n + 1]
        off[0] = 0
        self.ctx.lower_begin(n, out=self._lw_out)
        ends = [lo + e for e in self._chunk_bounds(n, self.lower_chunk)]
        if os.environ.get("GPE_READ_LOWER", "1") != "0":
            # the pipeline in native code: the next chunk's read overlaps
            # the previous one's staging and launch (gpe_lower_add)
            t0 = time.perf_counter()
            rc = self.flattener.read_lower(individuals, ends,
                                           self.ctx.lower_add_addr(),
                                           self.ctx.handle_addr(), off, lo)
            self.stats["flatten_s"] += time.perf_counter() - t0
            if rc is None:
                return None            # (the next lowering or load resets)
            self.ctx.check_rc(rc, "gpe_lower_add")
            t0 = time.perf_counter()
            depth, err, status = self.ctx.lower_end(out=self._lw_out)
            self.stats["device_s"] += time.perf_counter() - t0
            return self._lowered_batch(off, depth, err, status, keep)
        a = lo
        for b in ends:
            t0 = time.perf_counter()
            r = self.flattener.read_codes(individuals, a, b)
            self.stats["flatten_s"] += time.perf_counter() - t0
            if r is None:
                return None            # (the next lowering or load resets)
            t0 = time.perf_counter()
            codes, node_off, evals, eph_off = r
            self.ctx.lower_add(codes, node_off, evals, eph_off)
            # the population's node offsets, chunk by chunk
            np.add(np.frombuffer(node_off, dtype=np.int64)[1:], off[a - lo],
                   out=off[a - lo + 1:b - lo + 1])
            self.stats["device_s"] += time.perf_counter() - t0
            a = b
        t0 = time.perf_counter()
        depth, err, status = self.ctx.lower_end(out=self._lw_out)
        self.stats["device_s"] += time.perf_counter() - t0
        return self._lowered_batch(off, depth, err, status, keep)

    def _lowered_batch(self, off, depth, err, status, keep=True):
        """The ProgramBatch of a device lowering (None: the batch needs the
        host flattener).  *keep*: the batch outlives this call (its depth
        and error arrays are copied out of the reused output buffers)."""
        verr = None
        inexact = []
        # (the library counted the flagged trees while decoding: no scan of
        # a million zeros in the common case)
        n_err, n_status = self.ctx.lower_flags()
        if n_status:                          # rare: any flag at all
            verr = (status & 4) != 0
            if (status & 1).any():
                return None
            inexact = np.flatnonzero(status & 2).tolist()
        if n_err and ((err == ERR_CONST) & (True if verr is None else ~verr)).any():
            return None
        batch = ProgramBatch(None, off, depth.copy() if keep else depth, None,
                             err.copy() if keep else err,
                             {} if verr is None else
                             {int(i): ValueError("math domain error")
                              for i in np.flatnonzero(verr)},
                             inexact)
        batch.node_offsets = off
        batch.any_err = n_err > 0
        self.ctx.resident = batch
        self._warn_inexact(batch)
        self.stats["device_lowered"] += 1
        return batch

    def _warn_inexact(self, batch):
        """fp32 mode has no exact-integer pass: say so once."""
        if batch.inexact and self.precision == "fp32" and \
                not self._warned_inexact:
            self._warned_inexact = True
            warnings.warn("%d individual(s) may compute integers beyond "
                          "2**53; fp32 mode evaluates them in floating point "
                          "(fp64 mode keeps Python's exact ints)"
                          % len(batch.inexact), RuntimeWarning)

    def _load_exact(self, batch, individuals, ctx=None):
        """Programs that can compute Python ints beyond 2**53 (the batch's
        ``inexact`` candidates, decided exactly by the host flattener) are
        re-evaluated with Python-int semantics after each run
        (gpe_load_exact_v: on the device, and on the host where an int
        outgrows the device's 1088 bits); the pass reports the reference's
        exceptions (OverflowError for float(int) past 2**1024)."""
        if not batch.inexact:
            return 0
        if self.precision != "fp64" or \
                self.spec.mode not in (_lib.GPE_MODE_MSE, _lib.GPE_MODE_HITS_BOOL,
                                       _lib.GPE_MODE_SSE_SEQ):
            # no exact pass: an int constant past the float range is
            # converted, as the reference's mixed arithmetic would, and raises
            for i, exc in getattr(batch, "big_const", {}).items():
                if batch.err[i] == 0:
                    batch.err[i] = ERR_CONST
                    batch.const_exc[i] = exc
                    batch.any_err = True
            return 0
        cand = [i for i in batch.inexact if batch.err[i] == 0]
        if not cand:
            return 0
        fl = self.flattener
        if getattr(fl, "trig_leaves", None):
            # the exact pass takes sin/cos from glibc, not the leaf columns
            if self._exact_flattener is None:
                self._exact_flattener = Flattener(self.pset, self.spec.machine)
            fl = self._exact_flattener
        idx, code, off, depth, ints, _ = fl.exact_programs(
            [individuals[i] for i in cand])
        if idx:
            # kept on the batch: a reload of its programs (gpe_load_programs
            # clears the exact pass) loads the pass again (_make_resident)
            batch.exact_pass = ([cand[j] for j in idx], code, off, depth, ints)
            (self.ctx if ctx is None else ctx).load_exact(*batch.exact_pass)
        self.stats["exact_programs"] = self.stats.get("exact_programs", 0) + len(idx)
        return len(idx)

    def prepare(self, batch, individuals):
        """Load *batch* (the programs of *individuals*) into the context and
        set up its exact-integer pass; run_batch then evaluates it."""
        self._make_resident(batch)
        if getattr(batch, "exact_pass", None) is None:
            self._load_exact(batch, individuals)

    def _make_resident(self, batch):
        # (the context tracks which batch it holds by identity: a flag on the
        # batch would not say which context, or whether another batch
        # replaced it since)
        if self.ctx.resident is batch:
            return
        if batch.code is None:
            raise RuntimeError("this device-lowered batch is no longer the "
                               "context's programs; lower or flatten it again")
        self.ctx.load_programs(batch)
        if getattr(batch, "exact_pass", None) is not None:
            self.ctx.load_exact(*batch.exact_pass)

    def run_batch(self, batch, reuse=False, want=None, out=None):
        """Device evaluation of a flattened batch → raw arrays (and the
        per-case matrix for per-case specs, else None).  *reuse*: write into
        the evaluator's kept output arrays (valid until its next call);
        *want*: the outputs to copy back (the others are None); *out*: the
        arrays to write into instead (``views(n)``, as ResultBuffers)."""
        t0 = time.perf_counter()
        self._make_resident(batch)
        cases = None
        if getattr(self.spec, "scaled", False):
            # (mse in hi's place; the coefficients beside it)
            hi, a, b, err, flags = self.ctx.run_scaled(self.spec.sy,
                                                       self.spec.syy)
            lo = np.zeros_like(hi)
            self.last_scaling = (a, b)
        elif getattr(self.spec, "abs_error", False):
            # (the four words per program in hi's place)
            if getattr(self.spec, "abs_cases", False):
                cases, hi, err, flags = self.ctx.run_abserr_cases(
                    self.spec.hit_eps, self.spec.n_cases,
                    want_cases=self.spec.cases == "host")
            else:
                hi, err, flags = self.ctx.run_abserr(self.spec.hit_eps)
            lo = np.zeros(len(err))
            self.last_mae, self.last_max_error, self.last_hits = \
                self.spec.figures(hi, err, flags)
        elif getattr(self.spec, "hit_planes", False):
            # (the hit planes in cases' place; the counts alone come back)
            lo = err = flags = None
            if getattr(self.spec, "typed_planes", False):
                # (the error words only where a program can raise: _want)
                cases, hi, err = self.ctx.run_typed_hit_planes(
                    want_planes=self.spec.cases == "host",
                    want_err=want is None or "err" in want)
            else:
                cases, hi = self.ctx.run_hit_planes(
                    want_planes=self.spec.cases == "host")
            self.last_hits = np.asarray(hi).astype(np.int64)
            if getattr(self.spec, "confusion", False):
                # (the true positives in cases' place: one masked count of
                # the resident planes with the active spec's label plane)
                cases = self.ctx.hit_group_counts(
                    None, 0, 0, self.spec.label_plane()[None, :])[:, 0] \
                    if len(self.last_hits) else np.zeros(0, dtype=np.int64)
                conf = self.spec.confusion_counts(hi, cases, err)
                if getattr(batch, "any_err", True):
                    conf[np.flatnonzero(batch.err)] = -1
                self.last_confusion = conf
        elif getattr(self.spec, "per_case", False):
            cases, hi, lo, err, flags = self.ctx.run_cases(
                self.spec.mode, self.spec.n_cases)
        else:
            hi, lo, err, flags = self.ctx.run(
                self.spec.mode, out=out if out is not None else
                self._run_out if reuse else None, want=want)
        self.stats["device_s"] += time.perf_counter() - t0
        self.stats["kernel_ms"] += self.ctx.timing()["total_ms"]
        return hi, lo, err, flags, cases

    def _want(self, batch):
        """The outputs finish_all reads (B-machine hits: the counts alone, a
        quarter of the copy at pop 1M; no error words where no program can
        raise), or None (all)."""
        want = getattr(self.spec, "outputs", None) \
            if hasattr(self.spec, "finish_all") else None
        if want is not None and getattr(batch, "exact_pass", None) is None \
                and not getattr(getattr(self.flattener, "spec", None), "raises_value", True):
            want = getattr(self.spec, "outputs_plain", want)
        return want

    def evaluate(self, individuals):
        """Fitness tuple, or the exception instance the reference would raise,
        for every individual (in order).  With ``size_objective`` the tuples
        end with the individual's size."""
        out = self._evaluate_spec(individuals)
        if not self.size_objective:
            return out
        # (a new list: select_lexicase's record keeps the spec's own tuples)
        adf = isinstance(self.pset, (list, tuple))
        return [res if isinstance(res, BaseException) else
                tuple(res) + (sum(len(t) for t in ind) if adf else len(ind),)
                for ind, res in zip(individuals, out)]

    def _evaluate_spec(self, individuals):
        """:meth:`evaluate` without the size objective: the spec's tuples."""
        batch = self.lower_on_device(individuals, keep=False) \
            if self.device_lowering else None
        if batch is None:
            batch = self.flatten(individuals)
        self.prepare(batch, individuals)
        want = self._want(batch)
        hi, lo, err, flags, cases = self.run_batch(batch, reuse=True, want=want)
        self.stats["calls"] += 1
        self.stats["individuals"] += len(individuals)
        self.stats["node_evals"] += batch.n_nodes() * \
            self.spec.n_cases
        abs_cases = getattr(self.spec, "abs_cases", False) or \
            getattr(self.spec, "hit_planes", False)
        if (cases is None or abs_cases) and hasattr(self.spec, "finish_all"):
            args = [None if x is None else np.asarray(x)
                    for x in (hi, lo, err, flags)]
            out = self.spec.finish_all(*args, cases=cases) if abs_cases \
                else self.spec.finish_all(*args)
            if getattr(batch, "any_err", True):
                for i in np.flatnonzero(batch.err).tolist():
                    out[i] = SyntaxError("too many nested parentheses") \
                        if batch.err[i] == ERR_SYNTAX else batch.const_exc[i]
            if abs_cases:
                self._lex_batch = (list(individuals), out)
            return out
        out = []
        for i in range(len(individuals)):
            code = batch.err[i]
            if code == ERR_SYNTAX:
                out.append(SyntaxError("too many nested parentheses"))
            elif code == ERR_CONST:
                out.append(batch.const_exc[i])
            elif cases is not None:
                out.append(self.spec.finish(i, hi[i], lo[i], err[i],
                                            flags[i], cases[i]))
            else:
                out.append(self.spec.finish(i, hi[i], lo[i], err[i],
                                            flags[i]))
        if cases is not None:
            self._lex_batch = (list(individuals), out)
        return out

    LEXICASE_MODES = {"plain": 0, "epsilon": 1, "automatic": 2}

    def select_lexicase(self, individuals, k, mode="automatic", epsilon=0.0,
                        parallel=False):
        """Lexicase selection of *k* individuals straight from the per-case
        matrix the last :meth:`evaluate` / :meth:`map` left on the GPU
        (:class:`SymbRegCaseAbsErrors` in either *cases* mode,
        :class:`SymbRegCaseErrors`): ``gpe_lexicase`` without a host round
        trip.  *mode* ``"plain"``, ``"epsilon"`` (with *epsilon*) or
        ``"automatic"``: ``tools.selLexicase``, ``selEpsilonLexicase`` and
        ``selAutomaticEpsilonLexicase`` with every case minimised; the draws
        come from the module ``random`` stream as theirs do, so a seeded run
        selects the same individuals and leaves the same state.

        *individuals* must be the batch of that last evaluation: the same
        objects in the same order (``ValueError`` otherwise).  If an
        individual of the batch raised, its exception is raised here, the
        first in order.  The device selection's limits (16,384 individuals
        for ``"automatic"``; ``n/32 + n_cases`` words within 48 KiB of LDS)
        are raised as the library words them.

        After a :class:`BooleanCaseHits` or :class:`TypedCaseHits` evaluation
        the values are 0/1 hits
        and every case is maximised.  On such values ``selLexicase``,
        ``selEpsilonLexicase`` with ``0 <= epsilon < 1`` and
        ``selAutomaticEpsilonLexicase`` select the same individuals with the
        same draws and leave the same ``random`` state: a case keeps the
        candidates that hit it when some do and everybody otherwise, whatever
        an epsilon below 1 subtracts, and a 0/1 sample's median absolute
        deviation is 0 or 0.5.  All three modes therefore run one bit kernel
        (``gpe_lexicase_bits``), which has neither of the limits above.
        ``epsilon >= 1`` raises ``ValueError``: past 1 every candidate
        survives every case and the selection is ``random.choice``; a
        negative epsilon raises too.

        *parallel* True selects with ``gpe_lexicase_par`` /
        ``gpe_lexicase_bits_par``: the *k* selections run side by side, one
        workgroup each, with neither of the limits above.  Each is still the
        reference's loop body (a uniformly shuffled case order, the
        reference's survivors, a uniform final pick), but the shuffles and
        picks are SplitMix64 keys of one ``seed = random.getrandbits(64)``,
        the only draw from ``random`` (kept in ``last_lexicase_seed``; the
        rule is in include/gpeval.h, ``_lib.host_lexicase_par`` is its host
        twin).  A seeded run is reproducible; its picks are not DEAP's for
        the same ``random.seed``.  The checks above are made first, in the
        same order, and ``k == 0`` returns ``[]`` before any draw."""
        if mode not in self.LEXICASE_MODES:
            raise ValueError("mode must be 'plain', 'epsilon' or 'automatic' "
                             "(got %r)" % (mode,))
        individuals = list(individuals)
        bits = getattr(self.spec, "hit_planes", False)
        if bits and mode == "epsilon":
            if not 0.0 <= epsilon < 1.0:      # (a nan is refused as well)
                raise ValueError(
                    "select_lexicase: epsilon must be in [0, 1) on 0/1 hits "
                    "(got %r): %s" % (epsilon,
                                      "a negative epsilon leaves a case no "
                                      "candidate" if epsilon < 0 else
                                      "from 1 on every candidate survives "
                                      "every case and the selection is "
                                      "random.choice(individuals)"))
        def own():
            last = self._lex_batch[0]
            if len(individuals) != len(last) or \
                    any(a is not b for a, b in zip(individuals, last)):
                raise ValueError(
                    "select_lexicase: individuals must be the batch of this "
                    "evaluator's last evaluate / map, the same objects in "
                    "the same order: the GPU holds that batch's per-case "
                    "errors")
        last, results = self._last_batch(
            "select_lexicase", True,
            "this evaluator's last evaluate / map left no per-case matrix on "
            "the GPU (its spec is %s; evaluate with SymbRegCaseAbsErrors, "
            "SymbRegCaseErrors or BooleanCaseHits first)", own=own)
        for res in results:
            if isinstance(res, BaseException):
                raise res
        if k == 0:                        # the reference's loop runs 0 times
            return []
        if not individuals:               # individuals[0] in the reference
            raise IndexError("list index out of range")
        if parallel:
            # the only draw: case orders and choices are keys of this seed
            seed = random.getrandbits(64)
            self.last_lexicase_seed = seed
            if bits:
                idx, failed = self.ctx.lexicase_bits_par(None, 0, 0, k, seed)
            else:
                idx, failed = self.ctx.lexicase_par(
                    None, np.zeros(self.spec.n_cases, dtype=np.uint8), k,
                    seed, self.LEXICASE_MODES[mode], epsilon)
        elif bits:
            idx, failed = self.ctx.lexicase_bits(None, 0, 0, k, random._inst)
        else:
            idx, failed = self.ctx.lexicase(
                None, np.zeros(self.spec.n_cases, dtype=np.uint8), k,
                random._inst, self.LEXICASE_MODES[mode], epsilon)
        if failed >= 0:                   # random.choice([]) in the reference
            raise IndexError("Cannot choose from an empty sequence")
        return [individuals[i] for i in idx.tolist()]

    def select_dalex(self, individuals, k, pressure, standardize=True):
        """DALex selection (Ni, Ding and Spector 2024) of *k* individuals
        from the per-case matrix the last :meth:`evaluate` / :meth:`map` left
        on the GPU (``gpe_dalex`` / ``gpe_dalex_bits``): every selection draws
        one normal importance score per case (standard deviation *pressure*,
        the "particularity pressure"), turns the scores into weights with a
        softmax and picks the individual with the smallest weighted sum of its
        per-case errors.  A large *pressure* behaves like lexicase, a small
        one like selection on the mean error.  With *standardize* every case
        is divided by its standard deviation over the population first (a
        constant case gets weight 0).  The *k* selections are one fp64 matrix
        product on the GPU with a fused argmin; the cost grows as
        ``n * n_cases * k``.

        It works after :class:`SymbRegCaseAbsErrors` (either *cases* mode),
        :class:`SymbRegCaseErrors` and the four hit-plane specs (a case's
        error is then ``1 - hit``), and under :meth:`subsample`.  The checks
        are :meth:`select_lexicase`'s, in its order: *individuals* must be the
        batch of that last evaluation (``ValueError``), the first exception an
        individual raised is raised here, ``k == 0`` returns ``[]`` before any
        draw.  The only draw from ``random`` is ``seed =
        random.getrandbits(64)``, kept in ``last_dalex_seed``; weights and
        tie-breaks are SplitMix64 keys of it (the rule is in
        include/gpeval.h, ``_lib.host_dalex`` is its host twin), so a seeded
        run is reproducible.  An individual with an error that is not finite
        is never picked; when nobody is left, ``IndexError`` as
        ``random.choice([])``.  Nothing resident changes."""
        pressure = float(pressure)
        if not (pressure >= 0.0 and math.isfinite(pressure)):
            raise ValueError("select_dalex: pressure must be finite and >= 0 "
                             "(got %r)" % (pressure,))
        individuals = list(individuals)
        bits = getattr(self.spec, "hit_planes", False)

        def own():
            last = self._lex_batch[0]
            if len(individuals) != len(last) or \
                    any(a is not b for a, b in zip(individuals, last)):
                raise ValueError(
                    "select_dalex: individuals must be the batch of this "
                    "evaluator's last evaluate / map, the same objects in "
                    "the same order: the GPU holds that batch's per-case "
                    "errors")
        last, results = self._last_batch(
            "select_dalex", True,
            "this evaluator's last evaluate / map left no per-case matrix on "
            "the GPU (its spec is %s; evaluate with SymbRegCaseAbsErrors, "
            "SymbRegCaseErrors or BooleanCaseHits first)", own=own)
        for res in results:
            if isinstance(res, BaseException):
                raise res
        if k == 0:
            return []
        if not individuals:
            raise IndexError("list index out of range")
        seed = random.getrandbits(64)     # the only draw
        self.last_dalex_seed = seed
        if bits:
            idx, failed = self.ctx.dalex_bits(None, 0, 0, k, seed, pressure,
                                              standardize)
        else:
            idx, failed = self.ctx.dalex(None, k, seed, pressure, standardize)
        if failed >= 0:                   # nobody is fit: random.choice([])
            raise IndexError("Cannot choose from an empty sequence")
        return [individuals[i] for i in idx.tolist()]

    def weighted_errors(self, weights):
        """Each individual's weighted sum of its per-case errors,
        ``sum_c weights[c] * e[i, c]`` (``gpe_weighted_errors``, the DALex
        product kernel with a store epilogue): ``float64[n]`` for 1-D
        *weights* ``[n_cases]``, ``float64[n, G]`` for 2-D ``[G, n_cases]``
        (one column per boosting round or sample-weight vector; any *G*).
        The matrix is the one the last :meth:`evaluate` / :meth:`map` left on
        the GPU with :class:`SymbRegCaseAbsErrors` or
        :class:`SymbRegCaseErrors` (for hit planes see :meth:`weighted_hits`).
        Every weight must be finite and ``>= 0`` (``ValueError``).  The sum
        is within ``(n_cases + 1) * 2^-53`` relative of the exact one.  An
        individual whose result is an exception, or with an error that is not
        finite, gets ``nan``.  ``ValueError`` when the last evaluate / map
        left no such matrix or another batch has been loaded since."""
        last, results = self._last_batch(
            "weighted_errors",
            not getattr(self.spec, "hit_planes", False),
            "this evaluator's last evaluate / map left no per-case errors on "
            "the GPU (its spec is %s; evaluate with SymbRegCaseAbsErrors or "
            "SymbRegCaseErrors first)")
        one = np.ndim(weights) == 1
        w = _lib.check_case_weights("weighted_errors", weights,
                                    self.spec.n_cases)
        n, G = len(last), w.shape[0]
        out = np.zeros((n, G), dtype=np.float64)
        if n and G:
            out[:] = self.ctx.weighted_errors(None, w)
            out[self._raised(results)] = np.nan
        return out[:, 0] if one else out

    def last_case_hits(self):
        """``bool[n, n_cases]``: the hit matrix of the last
        :class:`BooleanCaseHits` / :class:`TypedCaseHits` evaluation, read
        back from the device's bit matrix on request (either *cases* mode).  ``ValueError`` when the
        last evaluate / map left none (as :meth:`select_lexicase`)."""
        last, _ = self._last_batch(
            "last_case_hits", getattr(self.spec, "hit_planes", False),
            "this evaluator's last evaluate / map left no hit planes on the "
            "GPU (its spec is %s; evaluate with BooleanCaseHits first)",
            loaded=False)
        n = len(last)
        if n == 0:
            return np.zeros((0, self.spec.n_cases), dtype=bool)
        return unpack_bitplanes(self.ctx.hit_planes(n), self.spec.n_cases)

    def _last_batch(self, what, served, missing, eps=None, hits_eps=None,
                    own=None, loaded=True):
        """The batch of the last :meth:`evaluate` / :meth:`map` and its
        results → ``(last, results)``, for the methods that read the
        per-case matrix it left on the GPU.  ``ValueError``, in this order:
        no such matrix — none at all, or not *served*: one of the kind the
        caller reads — in the caller's words *missing*; an *eps* for hit
        planes, which are thresholded already (*hits_eps*: the caller's
        clause); *own*, the caller's own checks; with *loaded*, another batch
        in the context since.  ``%s`` in the caller's words is the spec's
        name."""
        if self._lex_batch is None or not served:
            raise ValueError("%s: %s" % (what, missing.replace(
                "%s", type(self.spec).__name__)))
        if eps is not None and getattr(self.spec, "hit_planes", False):
            raise ValueError("%s: eps applies to SymbRegCaseAbsErrors; %s "
                             "(got eps=%r)" % (what, hits_eps.replace(
                                 "%s", type(self.spec).__name__), eps))
        if own is not None:
            own()
        last, results = self._lex_batch
        if loaded and self.ctx.n_prog != len(last):
            raise ValueError(
                "%s: the context now holds %d programs, not the %d of the "
                "last evaluate / map; evaluate the batch again"
                % (what, self.ctx.n_prog, len(last)))
        return last, results

    def _hit_eps(self, what, eps):
        """The threshold a call on the hit matrix passes on: 0.0 for hit
        planes, else *eps* (default ``spec.hit_eps``), ``>= 0``."""
        if getattr(self.spec, "hit_planes", False):
            return 0.0
        eps = self.spec.hit_eps if eps is None else float(eps)
        if not eps >= 0.0:
            raise ValueError("%s: eps must be >= 0 (got %r)" % (what, eps))
        return eps

    def _raised(self, results):
        """The indices of the individuals whose result is an exception
        (found once per evaluation: a pass over a million results costs more
        than a count on the GPU)."""
        cache = getattr(self, "_group_raised", None)
        if cache is None or cache[0] is not results:
            cache = self._group_raised = (results, [
                i for i, res in enumerate(results)
                if isinstance(res, BaseException)])
        return cache[1]

    def _group_masks(self, groups):
        """*groups* of :meth:`group_hits` as ``bool[G, n_cases]``."""
        n_cases = self.spec.n_cases
        arr = groups if isinstance(groups, np.ndarray) else None
        if arr is None:
            try:
                arr = np.asarray(groups)
            except ValueError:          # (ragged index lists)
                arr = None
        if arr is not None and arr.dtype == bool and arr.ndim == 2:
            if arr.shape[1] != n_cases:
                raise ValueError("group_hits: a boolean groups array must be "
                                 "[G, %d] (got %r)" % (n_cases, arr.shape))
            return arr
        masks = np.zeros((len(groups), n_cases), dtype=bool)
        for g, members in enumerate(groups):
            a = np.asarray(members)
            if a.size == 0:
                continue
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError("group_hits: groups[%d] must be a 1-D "
                                 "sequence of integer case indices" % g)
            bad = np.flatnonzero((a < 0) | (a >= n_cases))
            if len(bad):
                raise IndexError("group_hits: groups[%d][%d] = %d is outside "
                                 "[0, %d)" % (g, bad[0], a[bad[0]], n_cases))
            masks[g, a] = True
        return masks

    def group_hits(self, groups):
        """``int64[n, G]``: each individual's hits inside each of *G* case
        groups, counted on the GPU from the hit matrix the last
        :meth:`evaluate` / :meth:`map` left there (``gpe_hit_group_counts``;
        :class:`BooleanCaseHits`, :class:`TypedCaseHits`,
        :class:`BooleanConfusion` or :class:`TypedConfusion`, either *cases*
        mode): per-fold, per-stratum or train / validation counts from one
        evaluation, with no ``n x n_cases`` copy.

        *groups*: ``bool[G, n_cases]``, or a sequence of *G* integer index
        sequences over the active cases (positions in ``case_subset`` while a
        subset is active, as first-error cases are); duplicates inside a
        group count once, an index out of range raises ``IndexError`` (a
        negative one included).  More than 8 groups are counted in slices of
        8.  An individual whose result is an exception gets a row of ``-1``.
        ``ValueError`` when the last evaluate / map left no hit planes (as
        :meth:`last_case_hits`) or another batch has been loaded since (as
        :meth:`select_lexicase`)."""
        last, results = self._last_batch(
            "group_hits", getattr(self.spec, "hit_planes", False),
            "this evaluator's last evaluate / map left no hit planes on the "
            "GPU (its spec is %s; evaluate with BooleanCaseHits, "
            "TypedCaseHits, BooleanConfusion or TypedConfusion first)")
        masks = self._group_masks(groups)
        n, G = len(last), len(masks)
        out = np.zeros((n, G), dtype=np.int64)
        if n == 0 or G == 0:
            return out
        planes = pack_bitplanes(masks)
        for s in range(0, G, _lib.HIT_GROUPS_MAX):
            e = min(G, s + _lib.HIT_GROUPS_MAX)
            out[:, s:e] = self.ctx.hit_group_counts(None, 0, 0, planes[s:e])
        out[self._raised(results)] = -1
        return out

    def _case_weights_batch(self, what, eps):
        """The checks the case-weight calls share → ``(n, eps, raised,
        live)``: the batch's size, the threshold to pass on, the indices of
        the individuals whose result is an exception and the live mask
        (None when nobody raised)."""
        last, results = self._last_batch(
            what, getattr(self.spec, "hit_planes", False) or
            getattr(self.spec, "abs_cases", False),
            "this evaluator's last evaluate / map left no hit planes and no "
            "per-case absolute errors on the GPU (its spec is %s; evaluate "
            "with BooleanCaseHits, TypedCaseHits, BooleanConfusion, "
            "TypedConfusion or SymbRegCaseAbsErrors first)",
            eps=eps, hits_eps="the cases of %s are hits already")
        eps = self._hit_eps(what, eps)
        raised = self._raised(results)
        live = None
        if raised:
            alive = np.ones(len(last), dtype=bool)
            alive[raised] = False
            live = _lib.pack_live_mask(alive)
        return len(last), eps, raised, live

    def case_solve_counts(self, eps=None):
        """``int64[n_cases]``: how many individuals of the last
        :meth:`evaluate` / :meth:`map` solve each case, counted on the GPU
        from the per-case matrix that evaluation left there
        (``gpe_case_solve_counts``): the hit planes of
        :class:`BooleanCaseHits`, :class:`TypedCaseHits`,
        :class:`BooleanConfusion` or :class:`TypedConfusion`, or
        :class:`SymbRegCaseAbsErrors`' absolute errors, where a case is
        solved when its error is finite and ``<= eps`` (default
        ``spec.hit_eps``; *eps* with a hit-plane spec is a ``ValueError``).
        An individual whose result is an exception is not counted.  While a
        case subset is active the positions are those of the active cases.
        Nothing is drawn from ``random`` and nothing resident changes.
        ``ValueError`` when the last evaluate / map left no such matrix or
        another batch has been loaded since (as :meth:`group_hits`)."""
        n, eps, _, live = self._case_weights_batch("case_solve_counts", eps)
        if n == 0:
            return np.zeros(self.spec.n_cases, dtype=np.int64)
        return self.ctx.case_solve_counts(None, 0, 0, eps, live)

    def weighted_hits(self, weights, eps=None):
        """Each individual's sum of *weights* over the cases it solves
        (``gpe_hit_weighted_sums``): ``float64[n]`` for 1-D *weights*
        ``[n_cases]``, ``float64[n, G]`` for 2-D ``[G, n_cases]`` (one column
        per boosting round, fold or cost vector; more than 8 rows go in slices
        of 8).  The matrix, *eps* and the ``ValueError`` s of the batch are
        :meth:`case_solve_counts`'.  Every weight must be finite and ``>= 0``
        (``-0.0`` is ``0.0``) and ``math.fsum`` of every row finite, else
        ``ValueError`` before the GPU is touched.  The sum is a
        double-double sum in one fixed order: within 1e-12
        relative of ``math.fsum``, equal to it whenever the partial sums are
        representable; no hits give ``+0.0``.  An individual whose result is
        an exception gets ``nan`` (where :meth:`group_hits` gives -1)."""
        n, eps, raised, _ = self._case_weights_batch("weighted_hits", eps)
        one = np.ndim(weights) == 1
        w = _lib.check_case_weights("weighted_hits", weights,
                                    self.spec.n_cases)
        G = w.shape[0]
        out = np.zeros((n, G), dtype=np.float64)
        if n and G:
            for s in range(0, G, _lib.HIT_WEIGHTS_MAX):
                e = min(G, s + _lib.HIT_WEIGHTS_MAX)
                out[:, s:e] = self.ctx.hit_weighted_sums(None, 0, 0, w[s:e],
                                                         eps)
            out[raised] = np.nan
        return out[:, 0] if one else out

    def shared_hits(self, eps=None):
        """``float64[n]``: implicit fitness sharing (Smith et al. 1993;
        McKay 2000) — a case is worth ``1 / (the number of individuals that
        solve it)`` and an individual's value is the sum of the worth of the
        cases it solves (``gpe_hit_shared_sums``: counts, weights and sums
        stay on the GPU).  ``last_solve_counts`` (``int64[n_cases]``) holds
        the counts.  The matrix, *eps*, the accuracy and the ``ValueError`` s
        are :meth:`weighted_hits`'; an individual whose result is an
        exception is left out of the counts and gets ``nan``."""
        n, eps, raised, live = self._case_weights_batch("shared_hits", eps)
        if n == 0:
            self.last_solve_counts = np.zeros(self.spec.n_cases,
                                              dtype=np.int64)
            return np.zeros(0, dtype=np.float64)
        self.last_solve_counts, out = self.ctx.hit_shared_sums(
            None, 0, 0, eps, live)
        out = np.array(out)
        out[raised] = np.nan
        return out

    def map(self, individuals):
        return _yield_until_error(self.evaluate(list(individuals)))

    # ------------------------------------------------------------ predict --
    def _predict_context(self, X):
        """The sibling context of ``predict(X=...)``: the evaluator's
        machine, precision and trig-leaf setting, no target column; created
        on first use, the rows uploaded again only when they change."""
        bits = self.spec.machine == Machine.B
        X = np.ascontiguousarray(X, dtype=np.uint8 if bits else np.float64)
        if X.ndim == 1:
            X = X[None, :]
        n_vars = self.spec.planes.shape[0] if bits else self.spec.X.shape[0]
        if X.ndim != 2 or X.shape[0] != n_vars:
            raise ValueError("X must be [n_vars, n_cases] with n_vars = %d"
                             % n_vars)
        if self._predict_X is not None and self._predict_X.shape == X.shape \
                and np.array_equal(self._predict_X, X, equal_nan=not bits):
            return self._predict_ctx
        if self._predict_ctx is None:
            self._predict_ctx = _lib.Context(self.ctx.device)
            if self.precision == "fp32":
                self._predict_ctx.set_precision(_lib.GPE_PREC_F32)
        ctx = self._predict_ctx
        if bits:
            if not np.isin(X, (0, 1)).all():
                raise NotImplementedError("bit-sliced evaluation needs 0/1 data")
            planes = pack_bitplanes(X)
            # (the B machine's cases carry an output plane; a values run
            # never compares with it)
            ctx.set_bitplanes(planes, np.zeros(planes.shape[1], np.uint32),
                              X.shape[1])
        else:
            ctx.set_cases(_lib.GPE_MACHINE_F, X, None)
            # sin/cos leaf columns as the evaluator's, where these rows allow
            # them (a leaf of a column with an inf must stay in the program,
            # which reports the ValueError); else the plain flattener
            leaves = getattr(self.flattener, "trig_leaves", None) or ()
            ok = set(trig_leaf_columns(self.flattener.spec, _Rows(X),
                                       self.precision))
            self._predict_leaves = bool(leaves) and set(leaves) <= ok
            if self._predict_leaves:
                ctx.set_trig_leaves(True)
        self._predict_X = X.copy()
        self.predict_uploads += 1
        return ctx

    def _predict_load(self, chunk, ctx):
        """Flatten / lower *chunk* with the evaluator's own code and load it
        (and its exact-integer pass) into *ctx*; returns the batch."""
        if ctx is self.ctx:
            batch = self.lower_on_device(chunk, keep=False) \
                if self.device_lowering else None
            if batch is None:
                batch = self.flatten(chunk)
            self.prepare(batch, chunk)
            return batch
        fl = self.flattener
        if getattr(fl, "trig_leaves", None) and not self._predict_leaves:
            if self._exact_flattener is None:
                self._exact_flattener = Flattener(self.pset, self.spec.machine)
            fl = self._exact_flattener
        t0 = time.perf_counter()
        batch = fl.flatten(chunk)
        self.stats["flatten_s"] += time.perf_counter() - t0
        self._warn_inexact(batch)
        ctx.load_programs(batch)
        self._load_exact(batch, chunk, ctx=ctx)
        return batch

    def predict(self, individuals, X=None, errors="raise", max_bytes=1 << 30,
                scaled=False):
        """What each individual computes on each case:
        ``numpy.array([[gp.compile(t, pset)(*row) for row in rows] for t in
        individuals], dtype=float64)``, bit for bit in fp64 mode (a bool is
        1.0 / 0.0, a Python int ``float(int)``); a :class:`BooleanHits`
        evaluator returns ``bool[n, n_cases]``.

        *X* None: the evaluator's own resident cases; else the rows to
        predict on, ``[n_vars, n_cases]`` like the spec's, held in a sibling
        context (uploaded again only when they change; the training cases
        stay in place).  The individuals are evaluated in chunks whose output
        stays within *max_bytes* (at least one individual per run).

        *errors* ``"raise"``: the reference's exception of the first
        individual (in order) with an erroring case (``ValueError`` of
        ``math.sin(inf)`` / ``math.sqrt(-1)``, ``OverflowError`` of an int
        past the float range), naming the individual and the case.
        ``"nan"``: no per-case exception; every erroring case of the fp64 /
        fp32 cores (for exact-int programs at least the first) holds NaN and
        ``last_predict_first_error`` (``int64[n]``, -1 for none) tells an
        error from a computed NaN.  Compile-time errors (a tree past 200
        levels, a constant subtree that raises) are raised either way.

        *scaled* True (a :class:`SymbRegScaledMSE` evaluator only, else
        ``ValueError``): ``a[:, None] + b[:, None] * predict(...)`` with each
        individual's coefficients fitted on the training cases — held-out
        *X* rows are scaled by the training coefficients.  The coefficients
        come from an evaluation of *individuals* on the training cases made
        by this call: it counts in ``stats``, leaves ``last_scaling`` holding
        these individuals' ``(a, b)``, and an individual whose training
        evaluation raises has no coefficients, so its exception is raised
        whatever *errors* says (*errors* governs the predicted rows only).

        Out of scope: numpy-semantics specs (:class:`SymbRegNumpySSE`, whose
        sin/cos(inf) is a value, not an error), and case-sharded or
        population-sharded prediction (``distributed.py``)."""
        if errors not in ("raise", "nan"):
            raise ValueError("errors must be 'raise' or 'nan'")
        if scaled:
            if not getattr(self.spec, "scaled", False):
                raise ValueError("predict(scaled=True) needs a "
                                 "SymbRegScaledMSE evaluator: %s fits no "
                                 "scaling" % type(self.spec).__name__)
            individuals = list(individuals)
            # the coefficients of the training cases (an individual with an
            # erroring training case has none: its exception is raised)
            for res in self.evaluate(individuals):
                if isinstance(res, BaseException):
                    raise res
            a, b = self.last_scaling
            vals = self.predict(individuals, X=X, errors=errors,
                                max_bytes=max_bytes)
            with np.errstate(invalid="ignore"):     # (0 * inf of a flagged one)
                return a[:, None] + b[:, None] * vals
        if self.spec.mode == _lib.GPE_MODE_SSE_NUMPY:
            raise NotImplementedError("predict: numpy-semantics specs are not "
                                      "supported")
        individuals = list(individuals)
        n = len(individuals)
        bits = self.spec.machine == Machine.B
        ctx = self.ctx if X is None else self._predict_context(X)
        n_cases = ctx.n_cases
        row_bytes = ((n_cases + 31) // 32) * 4 if bits else n_cases * 8
        out = np.empty((n, n_cases), dtype=bool if bits else np.float64)
        first = np.full(n, -1, dtype=np.int64)
        self.last_predict_first_error = first
        for lo, hi in plan_predict_chunks(n, row_bytes, max_bytes):
            chunk = individuals[lo:hi]
            batch = self._predict_load(chunk, ctx)
            if getattr(batch, "any_err", True):
                for i in np.flatnonzero(batch.err).tolist():
                    raise SyntaxError("too many nested parentheses") \
                        if batch.err[i] == ERR_SYNTAX else batch.const_exc[i]
            t0 = time.perf_counter()
            if bits:
                out[lo:hi] = unpack_bitplanes(ctx.run_values_bits(), n_cases)
            else:
                _, err = ctx.run_values(out=out[lo:hi])
                first[lo:hi] = first_error_cases(err)
                if errors == "raise":
                    exc = predict_error(err, lo)
                    if exc is not None:
                        raise exc
            self.stats["device_s"] += time.perf_counter() - t0
        return out


def _yield_until_error(results):
    for res in results:
        if isinstance(res, BaseException):
            raise res
        yield res


def _unwrap(func):
    while isinstance(func, partial):
        if func.args or func.keywords:
            return None
        func = func.func
    return func if isinstance(func, GPUEvaluator) else None


def gpu_map(func, *iterables):
    """Drop-in for ``toolbox.map`` (reference default: builtin ``map``,
    ``deap/base.py:50``)."""
    ev = _unwrap(func)
    if ev is None or len(iterables) != 1:
        return map(func, *iterables)
    return ev.map(iterables[0])
