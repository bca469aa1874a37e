"""The handler matrix on the GPU: the trees of tests/handler_ref.py, which
between them execute every reachable handler of the exact D = 5 core, the
exact deep core and the typed core (tests/test_handler_matrix.py proves that
on the CPU), on IEEE edge operands, through every kernel that includes the
cores with a jump table of its own:

    values kernels      predict(errors="nan")           reference bits, first errors
    the same, permuted  cases reversed, rotated by 64   the unpermuted run's bits
    MSE kernels         SymbRegCaseErrors, zero target  f * f of the reference, bits;
                                                        the reference's exception type
    C++ kernels only    GPE_ASM=0                       reference bits
    moments kernels     SymbRegScaledMSE, run_moments   exact sums, n 2**-100 sum|term|
    typed core          TypedBoolHits                   exact hit counts
    ndiv / nrdiv        the numpy-flavoured set         reference bits

The reference is the vectorised twin, which the CPU test proves bit-identical
to ``gp.compile`` called per case on every small tree.  A failure names the
tree, its handlers, the core, the route, the case and both bit patterns.
"""
from fractions import Fraction

import numpy as np
import pytest

import handler_ref as hr
import scaled_ref as sr
from deap_amd import _lib

pytestmark = pytest.mark.gpu
LAUNCHES = ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep")


# -------------------------------------------------------------- references --
def cell(which):
    """``(pset, strings, X)`` of a cell's programs and cases."""
    if which in ("X", "Xodd"):
        X = hr.data()
        return hr.arith_pset(), hr.arith_small()[0], X if which == "X" else X[:, :hr.N - 1]
    if which == "Xb":
        return hr.arith_pset(), hr.arith_small()[0] + hr.arith_big(), hr.benign()
    if which == "X32":
        return hr.arith_pset(), hr.arith_small()[0], hr.data32()
    if which == "X40":
        return hr.arith_pset(40), hr.trees40(), hr.data40()
    if which == "npX":
        return hr.numpy_pset(), hr.numpy_trees(), hr.data()
    assert which == "npXb"
    return hr.numpy_pset(), hr.numpy_trees() + hr.numpy_big(), hr.benign()


def reference(which, dtype=np.float64):
    """``(trees, route, hits, X, F, first, masks)``, once per cell; *dtype*
    float32: the float32 twin's values, widened (exactly) to float64."""
    def make():
        pset, strings, X = cell(which)
        trees, route, hits = hr.programs(pset, strings)
        twin = hr.Twin(pset, dtype=dtype, numpy_sem=which.startswith("np"))
        F, first = twin.values(trees, X)
        return (trees, route, hits, np.ascontiguousarray(X), F.astype(np.float64), first,
                twin.masks)
    return hr.cached(("gpu_ref", which, dtype), make)


def evaluator(which, spec_cls=None, X=None, y=None, **kw):
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    pset, _, X0 = cell(which)
    X = np.ascontiguousarray(X0 if X is None else X)
    y = np.zeros((1, X.shape[1])) if y is None else y
    return GPUEvaluator(pset, (spec_cls or SymbRegMSE)(X, y), device=0, **kw)


def check_routing(ev, route, where):
    shapes = {k: ev.ctx.launch_shape(k)["programs"] for k in LAUNCHES}
    want = [int((route == r).sum()) for r in range(3)]
    assert shapes["asm_fast"] == want[0] and shapes["asm_deep"] == want[1] and \
        shapes["cpp_fast"] + shapes["cpp_deep"] == want[2], (where, shapes, want)


def check_values(which, got, first, route_name, dtype=np.float64):
    trees, route, hits, X, F, ref_first, _ = reference(which, dtype)
    strings = cell(which)[1]
    for r, core in enumerate(("exact D = 5 core", "exact deep core", "C++ kernels")):
        idx = np.flatnonzero(route == r)
        if not len(idx):
            continue
        msg = hr.mismatch(got[idx], F[idx], [strings[i] for i in idx],
                          [hits[i] for i in idx], core, route_name + " " + which)
        assert msg is None, msg
    assert first.tolist() == ref_first.tolist()


# ------------------------------------------------------------------ values --
@pytest.mark.parametrize("which", ["X", "Xodd", "Xb", "X40"])
def test_values_kernels(which):
    """predict(errors="nan"): the values kernels of the exact D = 5 and deep
    cores (X: 1354 cases, two tile buffers; Xodd: 1353, one) and the C++
    kernels (Xb: the 13-slot tree; X40: columns past 32)."""
    trees, route, hits, X, F, ref_first, _ = reference(which)
    ev = evaluator(which)
    try:
        got = ev.predict(trees, errors="nan")
        first = ev.last_predict_first_error.copy()
        if which != "X40":
            check_routing(ev, route, which)
        else:                                  # every tree reads a column past 32
            geo = ev.ctx.geometry()
            assert geo["asm"] == 0 and geo["fast"] + geo["deep"] == len(trees), geo
    finally:
        ev.close()
    check_values(which, got, first, "values kernels")
    if which == "Xb":
        assert (route == 2).sum() == 1 and (route == 1).sum() > 300


def test_values_kernels_with_the_cases_permuted():
    """The cases reversed and rotated by 64 (another lane, chain and tile for
    every case): bit-identical to the unpermuted run, column for column."""
    trees, route, hits, X, F, ref_first, _ = reference("X")
    perm = np.roll(np.arange(hr.N)[::-1], 64)
    ev = evaluator("X", X=X[:, perm])
    try:
        got = ev.predict(trees, errors="nan")
        check_routing(ev, route, "permuted")
    finally:
        ev.close()
    ev = evaluator("X")
    try:
        plain = ev.predict(trees, errors="nan")
    finally:
        ev.close()
    strings = cell("X")[1]
    msg = hr.mismatch(got, plain[:, perm], strings, hits, "exact cores", "values, permuted")
    assert msg is None, msg


# --------------------------------------------------------------- MSE kernels --
def case_expectation(F, masks):
    """Per program: the squares ``f * f`` (Python's ``(f - 0.0) ** 2``), or
    the name of the exception of its first raising case — ValueError where
    math.sqrt raised, OverflowError where a finite f squares to inf."""
    with np.errstate(all="ignore"):
        sq = F * F
        ovf = np.isfinite(F) & np.isinf(sq)
    out = []
    for i in range(len(F)):
        verr = masks.get(i)
        bad = ovf[i] | verr if verr is not None else ovf[i]
        if bad.any():
            c = int(np.argmax(bad))
            out.append("ValueError" if verr is not None and verr[c] else "OverflowError")
        else:
            out.append(sq[i])
    return out


@pytest.mark.parametrize("which", ["X", "Xb", "npX", "npXb"])
def test_mse_kernels_per_case_output(which):
    """SymbRegCaseErrors with a zero target: the MSE kernels' own inclusion
    of the cores.  On X nearly every program meets a value that squares past
    the float range (its exception type is compared); on Xb few do.  np: the
    numpy-flavoured set, which the library accepts with this spec."""
    from deap_amd.evaluator import SymbRegCaseErrors
    trees, route, hits, X, F, ref_first, masks = reference(which)
    strings = cell(which)[1]
    exp = case_expectation(F, masks)
    ev = evaluator(which, SymbRegCaseErrors)
    try:
        res = ev.evaluate(trees)
        check_routing(ev, route, which)
    finally:
        ev.close()
    n_val = 0
    got = np.full(F.shape, np.nan)
    want = np.full(F.shape, np.nan)
    for i, (r, e) in enumerate(zip(res, exp)):
        if isinstance(e, str):
            assert isinstance(r, BaseException) and type(r).__name__ == e, \
                (which, strings[i][:200], r, e)
            continue
        assert not isinstance(r, BaseException), (which, strings[i][:200], r)
        got[i], want[i] = r, e
        n_val += 1
    msg = hr.mismatch(got, want, strings, hits, "exact cores", "MSE kernels " + which)
    assert msg is None, msg
    print("HM|MSE kernels %s: %d of %d programs compared by value" % (which, n_val, len(res)))
    if which.endswith("Xb"):
        assert n_val >= 0.9 * len(res)


# ---------------------------------------------------------- C++ kernels only --
def test_cpp_kernels_alone(monkeypatch):
    """GPE_ASM=0 (read when the context is created): every tree on the C++
    kernels, the same bits."""
    trees, route, hits, X, F, ref_first, _ = reference("X")
    monkeypatch.setenv("GPE_ASM", "0")
    ev = evaluator("X")
    try:
        got = ev.predict(trees, errors="nan")
        first = ev.last_predict_first_error.copy()
        shapes = {k: ev.ctx.launch_shape(k)["programs"] for k in LAUNCHES}
    finally:
        ev.close()
    assert shapes["asm_fast"] == shapes["asm_deep"] == 0 and \
        shapes["cpp_fast"] + shapes["cpp_deep"] == len(trees), shapes
    msg = hr.mismatch(got, F, cell("X")[1], hits, "C++ kernels", "GPE_ASM=0 values")
    assert msg is None, msg
    assert first.tolist() == ref_first.tolist()


# ----------------------------------------------------------------- fp32 mode --
@pytest.mark.parametrize("which", ["X32", "Xb"])
def test_fp32_cores_values(which):
    """precision="fp32": add, sub, mul, div, neg, abs and sqrt are IEEE-exact
    in float32, so numpy float32 on float32 columns and constants gives the
    bits (the values come back widened to float64)."""
    trees, route, hits, X, F, ref_first, _ = reference(which, np.float32)
    ev = evaluator(which, precision="fp32")
    try:
        got = ev.predict(trees, errors="nan")
        first = ev.last_predict_first_error.copy()
        check_routing(ev, route, which + " fp32")
    finally:
        ev.close()
    assert (got.astype(np.float32).astype(np.float64) == got)[~np.isnan(got)].all()
    check_values(which, got, first, "fp32 values kernels", np.float32)


@pytest.mark.parametrize("which", ["X32", "Xb"])
def test_fp32_cores_per_case_output(which):
    """The fp32 MSE kernels' per-case terms: ``f * f`` in float32, widened;
    a finite f whose square is inf in float32 is the program's OverflowError."""
    from deap_amd.evaluator import SymbRegCaseErrors
    trees, route, hits, X, F, ref_first, masks = reference(which, np.float32)
    strings = cell(which)[1]
    F32 = F.astype(np.float32)
    exp = case_expectation(F32, masks)
    ev = evaluator(which, SymbRegCaseErrors, precision="fp32")
    try:
        res = ev.evaluate(trees)
        check_routing(ev, route, which + " fp32")
    finally:
        ev.close()
    got = np.full(F.shape, np.nan)
    want = np.full(F.shape, np.nan)
    n_val = 0
    for i, (r, e) in enumerate(zip(res, exp)):
        if isinstance(e, str):
            assert isinstance(r, BaseException) and type(r).__name__ == e, \
                (which, strings[i][:200], r, e)
            continue
        assert not isinstance(r, BaseException), (which, strings[i][:200], r)
        got[i], want[i] = r, e.astype(np.float64)
        n_val += 1
    msg = hr.mismatch(got, want, strings, hits, "fp32 cores", "fp32 MSE kernels " + which)
    assert msg is None, msg
    print("HM|fp32 MSE kernels %s: %d of %d programs compared by value"
          % (which, n_val, len(res)))


# ----------------------------------------------------------- moments kernels --
def test_moments_kernels():
    """SymbRegScaledMSE on Xb: the moments kernels (their own jump tables)
    run every program; each sum against the exact sum of the reference's
    values within ``n 2**-100 sum|term|`` (test_scaled_mse_gpu's bound).
    Programs under the range rule carry no sums and are skipped.

    The sums are double-doubles, and a double holds no value below 2**-1074:
    a product ``f * f`` or ``f * y`` below 2**-1022 (the constant trees'
    ``mul(ARGv, 5e-324)`` and their like) reaches its sum rounded to that
    grid, twice at most (the product and its error term), whatever the
    kernel does.  For the programs whose reference has such a product, known
    from the reference alone, the bound gains that floor, ``n 2**-1074``;
    for every other program it is the bound above, unchanged.  30 of the 929
    programs have such a product (3 %)."""
    from deap_amd.evaluator import SymbRegScaledMSE
    trees, route, hits, X, F, ref_first, _ = reference("Xb")
    strings = cell("Xb")[1]
    n = X.shape[1]
    y = np.random.default_rng(hr.SEED + 9).uniform(-2.0, 2.0, size=n)
    assert (ref_first == -1).all()
    ev = evaluator("Xb", SymbRegScaledMSE, y=y)
    try:
        batch = ev.flatten(trees)
        ev.prepare(batch, trees)
        m6, err, flags = ev.ctx.run_moments()
        shapes = {k: ev.ctx.launch_shape(k)["programs"]
                  for k in ("moments", "moments_deep") + LAUNCHES}
    finally:
        ev.close()
    print("HM|moments launches %r" % shapes)
    assert shapes["moments"] == (route == 0).sum() and \
        shapes["moments_deep"] == (route == 1).sum(), shapes
    assert (err == np.uint64(_lib.GPE_NO_ERROR)).all()
    with np.errstate(invalid="ignore"):
        ranged = ~(np.abs(F) < sr.RANGE).all(axis=1)
    assert ranged.mean() < 0.10
    bound = Fraction(n, 2 ** 100)
    floor = Fraction(n, 2 ** 1074)
    tiny = lambda t: bool(((t != 0) & (np.abs(t) < 2.0 ** -1022)).any())
    worst, n_floor = 0.0, 0
    for i in range(len(trees)):
        flagged = bool(flags[i] & _lib.GPE_FLAG_MOMENT_RANGE)
        assert flagged == bool(ranged[i]), (strings[i][:200], flagged)
        if flagged:
            continue
        f = F[i]
        with np.errstate(all="ignore"):
            under = tiny(f * f) or tiny(f * y) or \
                bool(((f != 0) & (f * f == 0)).any() or ((f != 0) & (y != 0) & (f * y == 0)).any())
        n_floor += under
        sums = (("Sf", sr.exact_sum(f.tolist()), sr.exact_sum(np.abs(f).tolist())),
                ("Sff", sr.exact_dot(f, f), None),
                ("Sfy", sr.exact_dot(f, y), sr.exact_sum(np.abs(f * y).tolist())))
        for k, (what, exact, mag) in enumerate(sums):
            got = Fraction(float(m6[i, 2 * k])) + Fraction(float(m6[i, 2 * k + 1]))
            lim = bound * (exact if mag is None else mag)
            if under and what != "Sf":
                lim += floor
            assert abs(got - exact) <= lim, \
                ("moments kernels on the %s core: %s of %s (handlers %s): got %r + %r, exact %r"
                 % (hr.ROUTES[route[i]], what, strings[i][:200],
                    " ".join(sorted(hr.name(h) for h in (hits[i] or ()))[:40]),
                    float(m6[i, 2 * k]), float(m6[i, 2 * k + 1]), float(exact)))
            if lim:
                worst = max(worst, float(abs(got - exact) / lim))
    print("HM|moments: worst error / bound %.3g, %d programs under the range rule, %d with "
          "a product below 2**-1022" % (worst, ranged.sum(), n_floor))
    assert n_floor < 0.05 * len(trees)


# ----------------------------------------------------------------- typed core --
def test_typed_core():
    from deap_amd.evaluator import GPUEvaluator, TypedBoolHits
    pset = hr.typed_pset()
    strings = hr.typed_trees()
    trees = hr.parse(strings, pset)
    Xt, labels = hr.typed_data()
    exp = hr.typed_hits_twin(pset, trees, Xt, labels).sum(axis=1)
    from deap_amd.flatten import Flattener
    hits = hr.word_hits(Flattener(pset).flatten(trees))
    ev = GPUEvaluator(pset, TypedBoolHits(np.ascontiguousarray(Xt), labels), device=0)
    try:
        res = ev.evaluate(trees)
        geo = ev.ctx.geometry()
    finally:
        ev.close()
    assert geo["asm_typed"] == len(trees), geo
    bad = [i for i, (r, e) in enumerate(zip(res, exp)) if r != (float(e),)]
    assert not bad, ("typed core, hit counts: %d of %d trees differ; first %s (handlers %s): "
                     "got %r, expected %d"
                     % (len(bad), len(trees), strings[bad[0]][:200],
                        " ".join(sorted(hr.name(h) for h in hits[bad[0]])),
                        res[bad[0]], exp[bad[0]]))


# --------------------------------------------------------- ndiv and nrdiv --
@pytest.mark.parametrize("which", ["npX", "npXb"])
def test_numpy_division_families(which):
    """The numpy-flavoured set's protected division (inf and nan quotients
    are 1) through the values kernels of both cores."""
    trees, route, hits, X, F, ref_first, _ = reference(which)
    ev = evaluator(which)
    try:
        got = ev.predict(trees, errors="nan")
        first = ev.last_predict_first_error.copy()
        check_routing(ev, route, which)
    finally:
        ev.close()
    check_values(which, got, first, "values kernels")
    assert (route == 0).any() and (route == 1).any()
