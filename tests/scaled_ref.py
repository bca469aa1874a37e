"""Test helper for ``SymbRegScaledMSE``: the definition of linear scaling in
exact rational arithmetic over the doubles ``gp.compile(tree, pset)(*row)``
returns.  Not product code.

    Sf = sum f   Sff = sum f*f   Sfy = sum f*y   Sy = sum y   Syy = sum y*y
    vf = Sff - Sf**2/n     vy = Syy - Sy**2/n     cfy = Sfy - Sf*Sy/n
    constant (vf == 0):  b = 0,      a = Sy/n,           mse = vy/n
    otherwise:           b = cfy/vf, a = (Sy - b*Sf)/n,  mse = (vy - cfy**2/vf)/n

with the two rules (an inf, nan or ``|f| >= 2**500`` output: fitness inf,
``b = 0``, ``a = Sy/n``; ``n*vf <= 2**-40 * Sff``: constant) and the
exceptions (the individual raises what its first erroring case raises).  Only
the results are rounded to double.

The exact sums are formed without a Fraction per term: ``math.fsum`` is the
correctly rounded sum, so the sum of the terms and of the negated parts found
so far is the exact remainder, and the parts add up to the exact sum when it
reaches zero; a product enters as Dekker's exact pair.

The GPU suite's population (2,000 seeded trees of the headline primitive set
and the hand-written ones) on its cases costs two and a half minutes of
``gp.compile`` calls and exact sums, so its reference is recorded in ``tests/golden/scaled_mse_n*.npz`` —
written by :func:`write_golden` (``python tests/golden/_ref_scaled_mse.py``) —
and ``tests/test_scaled_mse.py`` recomputes a sample of it here on every run.
"""
import math
import os
from fractions import Fraction

import numpy as np

from abs_sqrt_ref import ERRORS
from deap_amd import configs, gp

RANGE = 2.0 ** 500               # the range rule's bound
CONST = Fraction(1, 2 ** 40)     # the constant rule's
TOL = 1e-12                      # the project's tolerance (README)
# what keeps the comparison meaningful: the target's
# Syy / vy, and each program's Sff / (n vf) on either side of 2**40
Y_COND = 2 ** 10
F_COND_LO, F_COND_HI = 2 ** 20, 2 ** 60

CASES = (1, 2, 127, 128, 129, 257, 1000, 10243, 10240)
N_MAX = max(CASES)
N_RANDOM, POP_SEED, DATA_SEED = 2000, 2024, 5
INF_CASE = N_MAX - 1             # ARG9 is inf there: only the 10,243-case set
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATUS = {None: 0, "ValueError": 1, "OverflowError": 2}
FIELDS = ("status", "first", "flagged", "mse", "a", "b", "tol_mse", "tol_a",
          "tol_b", "Sf_hi", "Sf_lo", "Sff_hi", "Sff_lo", "Sfy_hi", "Sfy_lo",
          "Af", "Afy")


# ----------------------------------------------------------- exact sums --
def exact_sum(vals):
    """The exact sum of finite floats, as a Fraction."""
    vals = list(vals)
    total = Fraction(0)
    while True:
        s = math.fsum(vals)
        if s == 0.0:
            return total
        total += Fraction(s)
        vals.append(-s)


def _dekker_ok(x):
    m = np.abs(x[x != 0.0])
    return not len(m) or (m.min() > 2.0 ** -400 and m.max() < 2.0 ** 400)


def exact_dot(x, y):
    """The exact ``sum(x * y)`` of two float64 arrays, as a Fraction."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if not (_dekker_ok(x) and _dekker_ok(y)):
        return sum(Fraction(a) * Fraction(b) for a, b in zip(x.tolist(), y.tolist()))
    p = x * y
    c = 134217729.0 * x
    xh = c - (c - x)
    xl = x - xh
    c = 134217729.0 * y
    yh = c - (c - y)
    yl = y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return exact_sum(p.tolist() + e.tolist())


def dd(fr):
    """A Fraction as (hi, lo) doubles: hi the rounded value, lo the rounded
    remainder."""
    hi = float(fr)
    return hi, float(fr - Fraction(hi))


# ----------------------------------------------------------- definition --
def scaled(Sf, Sff, Sfy, Sy, Syy, n, flagged=False):
    """``(mse, a, b, constant)`` as Fractions (mse ``inf`` when flagged) from
    exact sums."""
    vy = Syy - Sy * Sy / n
    if flagged:
        return math.inf, Sy / n, Fraction(0), True
    vf = Sff - Sf * Sf / n
    if vf == 0 or n * vf <= CONST * Sff:
        return vy / n, Sy / n, Fraction(0), True
    cfy = Sfy - Sf * Sy / n
    b = cfy / vf
    return (vy - cfy * cfy / vf) / n, (Sy - b * Sf) / n, b, False


def sqrt_fr(fr):
    return math.sqrt(fr) if fr < 2 ** 1000 else math.inf


def record(f, y, first=None, kind=None):
    """The reference of one program on one case set as the FIELDS of the
    golden file: *f*, *y* float64 arrays of the same length; *first*, *kind*:
    its first erroring case within them and that exception's type name.
    Asserts the conditioning the comparison needs (module docstring)."""
    n = len(y)
    Sy, Syy = exact_sum(y.tolist()), exact_dot(y, y)
    vy = Syy - Sy * Sy / n
    assert n == 1 or Syy <= Y_COND * vy, "target conditioning %r" % float(Syy / vy)
    out = dict.fromkeys(FIELDS, 0.0)
    out["first"] = -1.0
    if first is not None:
        out["status"], out["first"] = float(STATUS[kind]), float(first)
        out["mse"] = out["a"] = out["b"] = math.nan
        return [out[k] for k in FIELDS]
    flagged = not bool((np.abs(f) < RANGE).all())          # inf, nan, huge
    if flagged:
        Sf = Sff = Sfy = Fraction(0)
    else:
        Sf, Sff, Sfy = exact_sum(f.tolist()), exact_dot(f, f), exact_dot(f, y)
        out["Af"] = float(exact_sum(np.abs(f).tolist()))
        out["Afy"] = float(exact_sum(np.abs(f * y).tolist()))
        vf = Sff - Sf * Sf / n
        assert vf == 0 or Sff <= F_COND_LO * n * vf or Sff >= F_COND_HI * n * vf, \
            "program conditioning 2**%.1f" % math.log2(Sff / (n * vf))
    mse, a, b, const = scaled(Sf, Sff, Sfy, Sy, Syy, n, flagged)
    out["flagged"] = float(flagged)
    out["mse"], out["a"], out["b"] = float(mse), float(a), float(b)
    # |mse - ref| <= TOL max(ref, vy / n); b to TOL max(|ref|, sqrt(vy / vf)),
    # a to TOL max(|ref|, sqrt(vy / vf) |Sf / n|); a constant program's b is
    # 0 and its a the target's mean
    out["tol_mse"] = 0.0 if flagged else TOL * max(float(mse), float(vy / n))
    if const:
        out["tol_a"], out["tol_b"] = TOL * abs(float(a)), 0.0
    else:
        s = sqrt_fr(vy / vf)
        out["tol_b"] = TOL * max(abs(float(b)), s)
        out["tol_a"] = TOL * max(abs(float(a)), s * abs(float(Sf / n)))
    for name, S in (("Sf", Sf), ("Sff", Sff), ("Sfy", Sfy)):
        out[name + "_hi"], out[name + "_lo"] = dd(S)
    return [out[k] for k in FIELDS]


# -------------------------------------------------- the GPU suite's cells --
def _level(k, j=[0]):
    """A balanced tree needing k + 1 stack slots (no sin/cos, no ARG9)."""
    if k == 0:
        j[0] += 1
        return "add(abs(ARG%d), psqrt(ARG%d))" % (j[0] % 9, (j[0] + 3) % 9)
    return "%s(%s, %s)" % ("sub" if k % 2 else "add", _level(k - 1), _level(k - 1))


def _chain(e, k):
    for _ in range(k):
        e = "mul(%s, %s)" % (e, e)
    return e


# the target's generator, as a tree: y is its value case by case
GENERATOR = "sub(add(mul(ARG0, ARG1), sin(mul(ARG2, ARG3))), mul(ARG4, cos(ARG5)))"
ONE = "protectedDiv(ARG0, sub(ARG0, ARG0))"          # the int 1
A = "add(1073741824, %s)" % ONE                       # the int 2**30 + 1
E25 = "add(1e25, ARG1)"                               # about 1e25, a float
E200 = _chain(E25, 3)                                 # 1e200: past 2**500
HAND = [
    "1",                                              # 0 a constant
    "ARG0",                                           # 1 x0
    "add(mul(%s, 3), 1)" % GENERATOR,                 # 2 an affine image of y
    "sub(1, mul(%s, 2))" % GENERATOR,                 # 3 ... anticorrelated
    E200,                                             # 4 the range rule
    "mul(%s, add(1e109, ARG1))" % E200,               # 5 past 1e308: inf
    "sin(mul(%s, %s))" % (E200, E200),                # 6 sin(inf): ValueError
    "sqrt(ARG6)",                                     # 7 ARG6 < 0 from case 3 on
    # 8 exact int: (2**30 + 1)**2 - 2**60 = 2**31 + 1 (in floats 2**31)
    "mul(ARG1, sub(mul(%s, %s), mul(1073741824, 1073741824)))" % (A, A),
    "mul(ARG1, %s)" % _chain(A, 6),                   # 9 float(int) past 2**1024
    _level(7),                                        # 10 8 slots: the deep core
    _level(12),                                       # 11 13 slots: the rows route
    "sin(ARG9)",                                      # 12 ValueError at INF_CASE
    "add(ARG9, ARG0)",                                # 13 inf at INF_CASE
    "add(mul(ARG0, 1000000), 1)",                     # 14 large mean, well conditioned
    "add(ARG1, 1000000000000000)",                    # 15 numerically constant
]
NEG_FROM = 3
# The first two cases.  With two cases a program's Sff / (n vf) is
# (f0^2 + f1^2) / (f0 - f1)^2, so any tree whose two outputs agree to three
# digits falls between the bounds above; of 2,000 trees a handful do at any
# two random points.  At these two none of the population's trees does
# (record() asserts it for every tree).
FIRST_TWO = [[0.047, 1.279, -0.318, 1.498, 1.829, -0.892, 1.148, -0.878, -0.309, -1.91],
             [1.014, 0.153, 1.053, 0.167, -0.787, -1.902, 0.88, -0.388, 1.542, -1.319]]


def data():
    """``(X[10, N_MAX], y[N_MAX])``: U(-2, 2) variables; ARG6 positive before
    case NEG_FROM and negative from it on; ARG9 inf in the last case; y the
    generator tree's values (a mean near zero)."""
    rng = np.random.default_rng(DATA_SEED)
    X = np.ascontiguousarray(rng.uniform(-2.0, 2.0, size=(N_MAX, 10)).T)
    X[:, :2] = np.array(FIRST_TWO).T
    X[6] = -np.abs(X[6])
    X[6, :NEG_FROM] = np.abs(X[6, :NEG_FROM])
    X[9, INF_CASE] = math.inf
    ps = configs.pset_for("symreg10_sqrt")
    func = gp.compile(gp.PrimitiveTree.from_string(GENERATOR, ps), ps)
    y = np.array([func(*row) for row in zip(*X.tolist())], dtype=np.float64)
    return X, y


def population():
    """``(pset, trees)``: the hand-written trees, then the 2,000 seeded ones
    of the headline primitive set (parsed into the set that also has sqrt)."""
    ps = configs.pset_for("symreg10_sqrt")
    rand = configs.population(configs.pset_for("symreg10"), "half", N_RANDOM,
                              POP_SEED, 4, 8)
    return ps, [gp.PrimitiveTree.from_string(s, ps) for s in HAND] + \
        [gp.PrimitiveTree.from_string(str(t), ps) for t in rand]


def outputs(ps, tree, rows):
    """``(f, first, kind)``: the tree's float64 value per row up to its
    first erroring case (nan from there on), that case and its exception's
    type name (None, None without one)."""
    func = gp.compile(tree, ps)
    f = np.full(len(rows), np.nan)
    for c, row in enumerate(rows):
        try:
            f[c] = float(func(*row))
        except ERRORS as e:
            return f, c, type(e).__name__
    return f, None, None


def reference(ps, tree, X, y, cases=CASES):
    """``{n: record}`` of one tree on the first n cases, for every n."""
    rows = list(zip(*X[:, :max(cases)].tolist()))
    f, first, kind = outputs(ps, tree, rows)
    out = {}
    for n in cases:
        err = first is not None and first < n
        out[n] = record(f[:n], y[:n], first if err else None, kind if err else None)
    return out


def cells_key(trees, X, y):
    """sha256 over the cases and the trees' strings: what a recorded
    reference belongs to."""
    import hashlib
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(X).tobytes())
    h.update(np.ascontiguousarray(y).tobytes())
    for t in trees:
        h.update(str(t).encode() + b"\n")
    return h.hexdigest()


def golden_path(n):
    return os.path.join(GOLDEN, "scaled_mse_n%d.npz" % n)


def load_golden(n, key=None):
    """float64 ``[n_trees, len(FIELDS)]`` of the recorded reference; *key*
    (``cells_key``): asserted to be the one it was recorded for."""
    with np.load(golden_path(n)) as z:
        assert key is None or str(z["key"]) == key, \
            "tests/golden/scaled_mse_n%d.npz was recorded for other trees or cases: run " \
            "tests/golden/_ref_scaled_mse.py" % n
        return z["ref"]


def write_golden():
    ps, trees = population()
    X, y = data()
    tab = {n: np.zeros((len(trees), len(FIELDS))) for n in CASES}
    for i, t in enumerate(trees):
        for n, rec in reference(ps, t, X, y).items():
            tab[n][i] = rec
    for n in CASES:
        np.savez_compressed(golden_path(n), ref=tab[n], key=np.array(cells_key(trees, X, y)))
