"""Test helper for the abs / sqrt primitives: the numpy interpreter of
``bytecode_ref`` extended by the two opcodes, and the reference evaluation
(``gp.compile`` per case, ``math.fsum``) of the GPU tests.  Not product code.
"""
import math

import numpy as np

import bytecode_ref as ref
from deap_amd import gp
from deap_amd.flatten import Op

ERRORS = (ValueError, OverflowError, ZeroDivisionError, TypeError)


def run_f(code, X, trig_args=None):
    """``(T, valueerror_mask)`` of one F program over all cases: the words of
    ``bytecode_ref.run_f`` plus ABS and SQRT.  *trig_args* (a list) receives
    every sin/cos node's argument vector, in word order."""
    n = X.shape[1]
    T = np.zeros(n)
    R = {}
    verr = np.zeros(n, dtype=bool)
    pc = 0
    with np.errstate(all="ignore"):
        while True:
            w = int(code[pc])
            pc += 1
            op, d, x = w & 0xff, (w >> 8) & 0xff, w >> 16
            if op == Op.END:
                return T, verr
            fam = Op.ADD <= op < Op.NEG or Op.NPDIV <= op < Op.NPDIV + 6
            b0 = Op.NPDIV if op >= Op.NPDIV else Op.ADD
            form = (op - b0) % 3 if fam else -1
            const = None
            if op in (Op.LDC, Op.PUSHC) or form == 2:
                const = ref._f64(code[pc], code[pc + 1])
                pc += 2
            if op in (Op.PUSH, Op.PUSHV, Op.PUSHC):
                R[d] = T
            if op in (Op.LDV, Op.PUSHV):
                T = X[x].copy()
            elif op in (Op.LDC, Op.PUSHC):
                T = np.full(n, const)
            elif op == Op.PUSH:
                pass
            elif fam:
                a = R[d] if form == 0 else X[x] if form == 1 else const
                T = ref._fbin(ref._FAMS[b0 + 3 * ((op - b0) // 3)], a, T)
            elif op == Op.NEG:
                T = -T
            elif op == Op.ABS:
                T = np.abs(T)
            elif op == Op.SQRT:
                verr |= T < 0
                T = np.sqrt(T)                     # IEEE, correctly rounded
            elif op in (Op.SIN, Op.COS):
                if trig_args is not None:
                    trig_args.append(T.copy())
                verr |= np.isinf(T)
                fn = math.sin if op == Op.SIN else math.cos
                T = np.array([fn(v) if math.isfinite(v) else math.nan
                              for v in T.tolist()])
            else:
                raise ValueError(op)


def values(pset, pop, X):
    """``func(*row)`` of every program at every case and the exceptions'
    type names by case: ``(F[n_prog, n_cases], [dict(case -> name)])``."""
    rows = list(zip(*X.tolist()))
    F = np.full((len(pop), len(rows)), np.nan)
    exc = [dict() for _ in pop]
    for i, tree in enumerate(pop):
        func = gp.compile(tree, pset)
        for c, row in enumerate(rows):
            try:
                F[i, c] = func(*row)
            except ERRORS as e:
                exc[i][c] = type(e).__name__
    return F, exc


def squares(F, exc, i, y, n=None):
    """Program *i*'s ``(f - y)**2`` over the first *n* cases as Python
    computes them (a list up to the first exception), and that exception's
    name (or None)."""
    n = len(y) if n is None else n
    first = min((c for c in exc[i] if c < n), default=None)
    out = []
    for c, (f, t) in enumerate(zip(F[i, :n].tolist(), y[:n].tolist())):
        if c == first:
            return out, exc[i][c]
        try:
            out.append((f - t) ** 2)
        except OverflowError:
            return out, "OverflowError"
    return out, None


def mse_reference(F, exc, y, n=None):
    """The reference's fitness per program over the first *n* cases:
    ``math.fsum(squares) / n`` or the first exception's type name."""
    n = len(y) if n is None else n
    out = []
    for i in range(F.shape[0]):
        sq, err = squares(F, exc, i, y, n)
        if err is None:
            try:
                out.append(math.fsum(sq) / n)
                continue
            except OverflowError:
                err = "OverflowError"
        out.append(err)
    return out


REL = 1e-12                       # the project's stated fp64 bound


def check_mse(pop, got, exp, what):
    """Exception type, nan, inf and 0.0 exact, else 1e-12 relative."""
    assert len(got) == len(exp) == len(pop)
    for tree, res, e in zip(pop, got, exp):
        s = str(tree)[:120]
        if isinstance(e, str):
            assert isinstance(res, BaseException) and type(res).__name__ == e, \
                (what, s, res, e)
            continue
        assert not isinstance(res, BaseException), (what, s, res, e)
        v = res[0]
        if math.isnan(e):
            assert math.isnan(v), (what, s, v)
        elif math.isinf(e) or e == 0.0:
            assert v == e, (what, s, v, e)
        else:
            assert abs(v - e) <= REL * abs(e), (what, s, v, e)
