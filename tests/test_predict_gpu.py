"""``GPUEvaluator.predict`` on the GPU against the reference expression

    numpy.array([[gp.compile(t, pset)(*row) for row in rows] for t in pop],
                dtype=numpy.float64)

bit for bit (``predict_ref``): hand trees through every route a per-case run
takes (the exact D = 5 and deep cores, the C++ kernels, the pair pass,
constants), a seeded population, the cross-check with the per-case squared
errors, ``errors="nan"``, the exact-integer pass, held-out rows, chunking,
device output, the ``GPE_EXACT_ALL=0`` / ``GPE_TILE_LOOP=0`` knobs in fresh
child processes (a child is this file run as a script), the B machine and a
typed primitive set.

F-machine case counts: 129 (a full 128-case tile and one case) and 386 (three
full tiles and a 2-case one).
"""
import itertools
import json
import math
import operator
import os
import subprocess
import sys

import numpy as np
import pytest

import predict_ref as pr
from deap_amd import configs, datasets, gp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASES = (129, 386)
N = max(CASES)
SEED = 41             # every value of the 300 seeded trees finite (checked on the CPU)
INF_CASE, BIG_CASE, NEG_CASE = 3, 130, 128


def _level(k, j=[0]):
    """A balanced tree needing k + 1 stack slots (no sin/cos)."""
    if k == 0:
        j[0] += 1
        cols = (0, 1, 2, 3, 4, 5, 7, 8, 9)          # (ARG6 holds the inf and 1e200)
        return "add(abs(ARG%d), psqrt(ARG%d))" % (cols[j[0] % 9], cols[(j[0] + 3) % 9])
    return "%s(%s, %s)" % ("sub" if k % 2 else "add", _level(k - 1), _level(k - 1))


HAND = ["ARG3",                                              # 0 a lone variable
        "1",                                                 # 1 a lone constant
        "protectedDiv(sin(ARG1), cos(ARG2))",                # 2 D <= 5, sin/cos
        "add(sin(mul(ARG1, ARG5)), protectedDiv(ARG4, ARG5))",   # 3 ... a zero divisor
        _level(5),                                           # 4 6 slots: the deep core
        _level(12),                                          # 5 13 slots: the C++ kernel
        "neg(neg(neg(ARG5)))",                               # 6 NEG chains, signed zeros
        "neg(mul(ARG5, neg(ARG3)))",                         # 7
        "sub(neg(ARG5), ARG5)",                              # 8
        "protectedDiv(sin(ARG6), sub(ARG0, ARG0))",          # 9 sin(inf) hidden by the 1
        "sqrt(ARG0)",                                        # 10 one negative value
        "mul(ARG6, ARG6)",                                   # 11 inf, no error
        "sin(ARG6)",                                         # 12 sin(inf), sin(1e200)
        "cos(add(ARG6, ARG1))"]                              # 13
TRIG = [i for i, s in enumerate(HAND) if "sin(" in s or "cos(" in s]
DEEP, CPP = 4, 5


def hand_data():
    X, Y = datasets.symreg10_cases(N, 11)
    X = X.copy()
    X[0] = np.abs(X[0])
    X[0, NEG_CASE] = -0.25
    X[5, 7], X[5, 200] = 0.0, -0.0
    X[6, INF_CASE], X[6, BIG_CASE] = math.inf, 1e200
    return X, Y


def _prefix(X, Y, n):
    return np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(Y[:, :n])


def populations():
    ps = configs.pset_for("symreg10_sqrt")
    hand = [gp.PrimitiveTree.from_string(s, ps) for s in HAND]
    seeded = configs.population(configs.pset_for("symreg10_abs"), "half", 300, SEED, 2, 5)
    seeded = [gp.PrimitiveTree.from_string(str(t), ps) for t in seeded]
    return ps, hand, seeded


_REF = {}


def reference(which):
    """``(pop, X, Y, F, exc)``: the reference's values at all 386 cases, once
    (a prefix of the cases is a prefix of the columns)."""
    if which not in _REF:
        ps, hand, seeded = populations()
        if which == "hand":
            pop, (X, Y) = hand, hand_data()
        else:
            pop, (X, Y) = seeded, datasets.symreg10_cases(N, 11)
        F, exc = pr.values(ps, pop, X)
        _REF[which] = (pop, X, Y, F, exc)
    return _REF[which]


def _first(exc, n):
    return pr.first_errors([{c: k for c, k in e.items() if c < n} for e in exc])


def evaluator(which, n, spec_cls=None, **kw):
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    pop, X, Y, _, _ = reference(which)
    return GPUEvaluator(configs.pset_for("symreg10_sqrt"),
                        (spec_cls or SymbRegMSE)(*_prefix(X, Y, n)), device=0, **kw)


def predict(which, n, **kw):
    """``(values, first errors, launch shapes)`` of ``predict(errors="nan")``."""
    pop = reference(which)[0]
    ev = evaluator(which, n)
    try:
        got = ev.predict(pop, errors="nan", **kw)
        first = ev.last_predict_first_error.copy()
        shapes = {k: ev.ctx.launch_shape(k)["programs"]
                  for k in ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep")}
    finally:
        ev.close()
    return got, first, shapes


# ------------------------------------------------------------ 1 hand trees --
def test_reference_of_the_hand_trees_is_what_the_cells_are_for():
    """(CPU part) the planted cases raise where the tests below say."""
    pop, X, Y, F, exc = reference("hand")
    assert exc[9] == {INF_CASE: "ValueError"} and (np.delete(F[9], INF_CASE) == 1.0).all()
    assert exc[10] == {NEG_CASE: "ValueError"}
    assert exc[12] == {INF_CASE: "ValueError"} and exc[13] == {INF_CASE: "ValueError"}
    assert not exc[11] and math.isinf(F[11, INF_CASE]) and math.isinf(F[11, BIG_CASE])
    assert not any(exc[i] for i in (0, 1, 2, 3, 4, 5, 6, 7, 8))
    # the signed zeros reach the NEG chains
    assert math.copysign(1, F[6, 7]) == -1 and math.copysign(1, F[6, 200]) == 1
    assert math.isfinite(F[12, BIG_CASE]) and (F[1] == 1.0).all()


@pytest.mark.parametrize("n", CASES)
def test_hand_trees_are_bit_identical_through_every_route(n):
    pop, X, Y, F, exc = reference("hand")
    got, first, shapes = predict("hand", n)
    assert got.shape == (len(pop), n) and got.dtype == np.float64
    for i, s in enumerate(HAND):
        pr.assert_same_bits(got[i], F[i, :n], "%s @%d" % (s[:40], n))
    assert first.tolist() == _first(exc, n).tolist()
    # routing: only the 13-slot tree ran on the C++ kernels (the pair pass of
    # the inf / 1e200 lanes is no launch of its own), the 6-slot one on the
    # deep core, everything else on the D = 5 core
    print("PREDICT|routing@%d|%r" % (n, shapes))
    assert shapes["cpp_fast"] + shapes["cpp_deep"] == 1, shapes
    assert shapes["asm_deep"] >= 1 and \
        shapes["asm_fast"] + shapes["asm_deep"] == len(pop) - 1, shapes
    from deap_amd.flatten import Flattener
    depth = Flattener(configs.pset_for("symreg10_sqrt")).flatten(pop).depth.tolist()
    assert 6 <= depth[DEEP] <= 12 < depth[CPP], depth


# ------------------------------------------------------ 2 seeded population --
def test_reference_of_the_seeded_population_is_finite():
    pop, X, Y, F, exc = reference("seeded")
    assert len(pop) == 300 and not any(exc) and np.isfinite(F).all()


@pytest.mark.parametrize("n", CASES)
def test_seeded_population_is_bit_identical(n):
    pop, X, Y, F, exc = reference("seeded")
    got, first, shapes = predict("seeded", n)
    pr.assert_same_bits(got, F[:, :n], "seeded @%d" % n)
    assert (first == -1).all()
    assert shapes["asm_fast"] + shapes["asm_deep"] == len(pop), shapes


# --------------------------------------------- 3 against the per-case errors --
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_squared_residuals_equal_the_per_case_errors(precision):
    """``(predict - y) ** 2`` is SymbRegCaseErrors' per-case matrix bit for
    bit; in fp32 mode the expression in numpy float32, widened (how the
    kernels' epilogue forms the term)."""
    from deap_amd.evaluator import SymbRegCaseErrors
    pop, X, Y, F, exc = reference("seeded")
    n = 386
    ev = evaluator("seeded", n, SymbRegCaseErrors, precision=precision)
    try:
        batch = ev.flatten(pop)
        ev.prepare(batch, pop)
        cases = ev.run_batch(batch)[4].copy()
        got = ev.predict(pop, errors="nan")
    finally:
        ev.close()
    if precision == "fp64":
        pr.assert_same_bits(got, F[:, :n], "fp64 values")
        d = got - Y[0, :n]
        exp = d * d
    else:
        g32 = got.astype(np.float32)
        assert (g32.astype(np.float64) == got).all()      # fp32 values, widened
        d = g32 - Y[0, :n].astype(np.float32)
        with np.errstate(over="ignore"):
            exp = (d * d).astype(np.float64)
    pr.assert_same_bits(cases, exp, precision + " terms")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_hand_trees_agree_with_the_per_case_errors(precision):
    """The same identity on the hand trees and their planted cases, which in
    fp32 mode take the fp32 cores, the fp32 C++ kernel (13 slots) and the pair
    pass of arguments past 2**30: at every case that does not raise, and the
    first raising case is the fitness run's."""
    from deap_amd import _lib
    from deap_amd.evaluator import SymbRegCaseErrors, first_error_cases
    pop, X, Y, F, exc = reference("hand")
    n = 386
    ev = evaluator("hand", n, SymbRegCaseErrors, precision=precision)
    try:
        batch = ev.flatten(pop)
        ev.prepare(batch, pop)
        _, _, err, _, cases = ev.run_batch(batch)
        err, cases = err.copy(), cases.copy()
        got = ev.predict(pop, errors="nan")
        first = ev.last_predict_first_error.copy()
    finally:
        ev.close()
    y = Y[0, :n]
    with np.errstate(all="ignore"):
        if precision == "fp64":
            exp = (got - y) * (got - y)
        else:
            d = got.astype(np.float32) - y.astype(np.float32)
            exp = (d * d).astype(np.float64)
    for i, s in enumerate(HAND):
        ok = ~np.isnan(got[i])
        pr.assert_same_bits(cases[i][ok], exp[i][ok], "%s %s" % (precision, s[:40]))
        # (d * d overflowing is the fitness run's error alone: nothing is squared here)
        if int(err[i]) & 3 != _lib.GPE_ERR_OVERFLOW or err[i] == np.uint64(_lib.GPE_NO_ERROR):
            assert first[i] == first_error_cases(err[i:i + 1])[0], (precision, s)
    assert first[9] == INF_CASE and first[10] == NEG_CASE and first[0] == -1
    if precision == "fp32":                      # float(1e200) is inf in fp32
        assert first[12] == INF_CASE and np.isnan(got[12, BIG_CASE])


# ---------------------------------------------------------- 4 errors="nan" --
@pytest.mark.parametrize("n", CASES)
def test_nan_sits_at_the_raising_cases_and_raise_raises(n):
    pop, X, Y, F, exc = reference("hand")
    got, first, _ = predict("hand", n)
    for i, e in enumerate(exc):
        bad = sorted(c for c in e if c < n)
        assert np.isnan(got[i, bad]).all(), (HAND[i], bad)
        # no other nan than the reference's own
        assert (np.isnan(got[i]) == np.isnan(F[i, :n])).all(), HAND[i]
    assert first.tolist() == _first(exc, n).tolist()
    assert first[9] == INF_CASE and first[10] == (NEG_CASE if n > NEG_CASE else -1)
    ev = evaluator("hand", n)
    try:
        with pytest.raises(ValueError) as info:
            ev.predict(pop)
        assert "individual 9" in str(info.value) and "case %d" % INF_CASE in str(info.value)
        # the trees before the first erroring one raise nothing
        pr.assert_same_bits(ev.predict(pop[:9]), F[:9, :n], "errors=raise")
        with pytest.raises(ValueError):
            ev.predict(pop, errors="ignore")
    finally:
        ev.close()


# ---------------------------------------------------------- 5 exact ints --
ONE = "protectedDiv(x, sub(x, x))"                  # the int 1
A = "add(1073741824, %s)" % ONE                     # the int 2**30 + 1


def _sq(e):
    return "mul(%s, %s)" % (e, e)


def _pow(k):
    """A ** k as a tree of muls (k's binary expansion)."""
    e, out = A, None
    while k:
        if k & 1:
            out = e if out is None else "mul(%s, %s)" % (out, e)
        e, k = _sq(e), k >> 1
    return out


EXACT = [_pow(2),                                   # 2**60: past 2**53, rounds
         "sub(%s, x)" % _pow(2),                    # ... meeting a float
         _pow(33),                                  # 2**990
         "neg(%s)" % _pow(34),                      # -(2**1020): the device's ints
         "sub(%s, sub(%s, %s))" % (_pow(37), _pow(37), A),   # past 1088 bits: the host
         _pow(35),                                  # 2**1050: OverflowError (device)
         _pow(37)]                                  # 2**1110: OverflowError (host)


def test_exact_int_programs_give_float_of_the_python_int():
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    ps = configs.pset_for("symbreg")
    pop = [gp.PrimitiveTree.from_string(e, ps) for e in EXACT]
    n = 129
    X = np.linspace(-3.0, 3.0, n)[None, :].copy()
    X[0, 5] = 0.0
    F, exc = pr.values(ps, pop, X)
    a = 2 ** 30 + 1
    assert F[0, 0] == float(a * a) and float(a * a) != a * a      # rounded
    assert F[2, 0] == float(a ** 33) and F[3, 0] == -float(a ** 34) and F[4, 0] == float(a)
    assert all(exc[i] == {c: "OverflowError" for c in range(n)} for i in (5, 6))
    assert not any(exc[:5])
    ev = GPUEvaluator(ps, SymbRegMSE(X, np.zeros((1, n))), device=0)
    try:
        got = ev.predict(pop, errors="nan")
        first = ev.last_predict_first_error.copy()
        assert ev.stats["exact_programs"] == len(pop)
        assert ev.ctx.exact_host_runs() >= 2
        pr.assert_same_bits(got[:5], F[:5], "exact ints")
        assert first.tolist() == [-1] * 5 + [0, 0]
        assert math.isnan(got[5, 0]) and math.isnan(got[6, 0])
        with pytest.raises(OverflowError) as info:
            ev.predict(pop)
        assert "individual 5" in str(info.value) and "case 0" in str(info.value)
        with pytest.raises(OverflowError):
            ev.predict(pop[6:])
    finally:
        ev.close()


# ---------------------------------------------------------- 6 held-out rows --
def _mixed():
    ps, hand, seeded = populations()
    return ps, hand + seeded[:40]


def _fit(results):
    return [type(r).__name__ if isinstance(r, BaseException) else [float(v).hex() for v in r]
            for r in results]


def test_held_out_rows_through_the_sibling_context():
    ps, pop = _mixed()
    X2 = datasets.symreg10_cases(193, 99)[0].copy()
    X2[6, 100] = -math.inf
    F2, exc2 = pr.values(ps, pop, X2)
    ev = evaluator("hand", 129)
    try:
        before = _fit(ev.evaluate(pop))
        got = ev.predict(pop, X=X2, errors="nan")
        assert got.shape == (len(pop), 193)
        pr.assert_same_bits(got, F2, "held-out rows")
        assert ev.last_predict_first_error.tolist() == pr.first_errors(exc2).tolist()
        assert ev.predict_uploads == 1
        # the training cases and their fitness are as they were
        assert _fit(ev.evaluate(pop)) == before
        pr.assert_same_bits(ev.predict(pop, X=X2.copy(), errors="nan"), got, "again")
        assert ev.predict_uploads == 1                 # the same rows: no upload
        # the evaluator's own cases, then other rows
        F1 = reference("hand")[3]
        pr.assert_same_bits(ev.predict(pop[:9], errors="nan"), F1[:9, :129], "X=None")
        X3 = np.ascontiguousarray(X2[:, :50])
        pr.assert_same_bits(ev.predict(pop, X=X3, errors="nan"), F2[:, :50], "other rows")
        assert ev.predict_uploads == 2
        assert _fit(ev.evaluate(pop)) == before
        with pytest.raises(ValueError):
            ev.predict(pop, X=X2[:5])
    finally:
        ev.close()


# --------------------------------------------------------------- 7 chunking --
def test_chunked_runs_give_the_same_bits():
    ps, pop = _mixed()
    n = 129
    ev = evaluator("hand", n)
    try:
        whole = ev.predict(pop, errors="nan")
        first = ev.last_predict_first_error.copy()
        from deap_amd.evaluator import plan_predict_chunks
        budget = n * 8 * -(-len(pop) // 3)
        assert len(plan_predict_chunks(len(pop), n * 8, budget)) == 3
        parts = ev.predict(pop, errors="nan", max_bytes=budget)
        pr.assert_same_bits(parts, whole, "3 runs")
        assert ev.last_predict_first_error.tolist() == first.tolist()
        pr.assert_same_bits(ev.predict(pop, errors="nan", max_bytes=1), whole, "single rows")
        # errors="raise" names the individual in the caller's order
        with pytest.raises(ValueError) as info:
            ev.predict(pop, max_bytes=n * 8 * 4)
        assert "individual 9" in str(info.value)
    finally:
        ev.close()


# ---------------------------------------------------------- 8 device output --
def test_device_output_equals_the_host_output():
    import torch
    from deap_amd import _lib
    ps, pop = _mixed()
    n = 386
    ev = evaluator("hand", n)
    try:
        batch = ev.flatten(pop)
        ev.prepare(batch, pop)
        vals, err = ev.ctx.run_values()
        t = torch.full((len(pop), n), 7.0, dtype=torch.float64, device="cuda:0")
        e = torch.zeros(len(pop), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ev.ctx.run_values_device(t.data_ptr(), e.data_ptr())
        pr.assert_same_bits(t.cpu().numpy(), vals, "device output")
        assert (e.cpu().numpy().view(np.uint64) == err).all()
        ev.ctx.run_values_device(t.data_ptr())           # no error array
        pr.assert_same_bits(t.cpu().numpy(), vals, "device output, no errors")
        # what the entry points refuse
        with pytest.raises(_lib.GpeError, match="null output"):
            ev.ctx.run_values_device(0)
        with pytest.raises(_lib.GpeError, match="B machine"):
            ev.ctx.run_values_bits()
        fresh = _lib.Context(0)
        try:
            fresh.set_cases(_lib.GPE_MACHINE_F, np.zeros((1, 4)), None)
            with pytest.raises(_lib.GpeError, match="no programs"):
                fresh.run_values()
        finally:
            fresh.close()
    finally:
        ev.close()


def test_a_values_run_leaves_the_resident_fitness_to_the_tournament():
    import random
    from deap_amd import _lib
    pop = reference("seeded")[0]
    ev = evaluator("seeded", 129)
    try:
        batch = ev.flatten(pop)
        ev.prepare(batch, pop)
        hi, lo, err, flags = ev.ctx.run(_lib.GPE_MODE_MSE)
        r1, r2 = random.Random(5), random.Random(5)
        a = ev.ctx.tournament(None, 500, 3, r1, weight=-1.0)
        ev.ctx.run_values()
        b = ev.ctx.tournament(None, 500, 3, r2, weight=-1.0)
        assert a.tolist() == b.tolist()
        hi2, lo2, err2, flags2 = ev.ctx.run(_lib.GPE_MODE_MSE)
        assert (hi2.view(np.uint64) == hi.view(np.uint64)).all() and (lo2 == lo).all()
    finally:
        ev.close()


# ------------------------------------------------------------------ 9 knobs --
def child(out):
    res = {}
    for n in CASES:
        got, first, _ = predict("hand", n)
        res[str(n)] = {"bits": [[int(v) for v in row] for row in pr.bits(got).tolist()],
                       "first": first.tolist()}
    with open(out, "w") as fh:
        json.dump(res, fh)


# the table cores' sin/cos is within 1 ulp of the reference's; the
# hand trees' sin/cos terms are O(1) and well conditioned, so their values are
# held to the project's stated fp64 bound, 1e-12, relative to max(|value|, 1)
TABLE_REL = 1e-12


@pytest.mark.parametrize("knob", ["GPE_EXACT_ALL", "GPE_TILE_LOOP"])
def test_knobs_off_give_the_reference_too(tmp_path, knob):
    out = str(tmp_path / "out.json")
    env = dict(os.environ)
    for k in ("GPE_EXACT_ALL", "GPE_TILE_LOOP", "GPE_ASM", "GPE_DIAG"):
        env.pop(k, None)
    env[knob] = "0"
    env["PYTHONPATH"] = os.pathsep.join([REPO, HERE] + env.get("PYTHONPATH", "").split(os.pathsep))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), out],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (knob, p.stdout[-2000:], p.stderr[-2000:])
    with open(out) as fh:
        res = json.load(fh)
    pop, X, Y, F, exc = reference("hand")
    for n in CASES:
        got = np.array(res[str(n)]["bits"], dtype=np.uint64).view(np.float64)
        assert res[str(n)]["first"] == _first(exc, n).tolist(), (knob, n)
        for i, s in enumerate(HAND):
            if knob == "GPE_TILE_LOOP" or i not in TRIG:
                pr.assert_same_bits(got[i], F[i, :n], "%s=0 %s @%d" % (knob, s[:40], n))
                continue
            ref = F[i, :n]
            assert (np.isnan(got[i]) == np.isnan(ref)).all(), (knob, s)
            ok = ~np.isnan(ref)
            with np.errstate(invalid="ignore"):
                d = np.abs(got[i][ok] - ref[ok])
            same = got[i][ok] == ref[ok]                  # (inf == inf)
            print("PREDICT|%s=0|%s@%d|max abs diff %.3g" % (knob, s[:40], n, d[~same].max(initial=0)))
            assert (same | (d <= TABLE_REL * np.maximum(np.abs(ref[ok]), 1.0))).all(), (knob, s)


# -------------------------------------------------------------- 10 B machine --
def _mux6():
    ps = gp.PrimitiveSet("MUX6", 6, "IN")
    ps.addPrimitive(operator.and_, 2)
    ps.addPrimitive(operator.or_, 2)
    ps.addPrimitive(operator.not_, 1)
    ps.addPrimitive(configs.if_then_else, 3)
    ps.addTerminal(1)
    ps.addTerminal(0)
    ins = datasets._bits_msb_first(6).astype(np.uint8)
    outs = ins[2 + ins[0] + 2 * ins[1], np.arange(64)]
    return ps, ins, outs


def _b_cells():
    ps6, ins6, outs6 = _mux6()
    pins, pouts = datasets.parity6_table()
    mins, mouts = datasets.mux11_table()
    return {"mux6@64": (ps6, ins6, outs6),
            "parity6@40": (configs.pset_for("parity6"), pins[:, :40], pouts[:40]),
            # (past 16 words: b_eval, one word per lane; 1000 = 31 words + 8 bits)
            "mux11@1000": (configs.pset_for("mux11"), mins[:, :1000], mouts[:1000])}


@pytest.mark.parametrize("cell", ["mux6@64", "parity6@40", "mux11@1000"])
def test_b_machine_outputs(cell):
    from deap_amd.evaluator import BooleanHits, GPUEvaluator
    ps, ins, outs = _b_cells()[cell]
    ins, outs = np.ascontiguousarray(ins), np.ascontiguousarray(outs)
    n = ins.shape[1]
    pop = configs.population(ps, "half", 200, 17, 2, 5)
    rows = list(zip(*ins.tolist()))
    exp = np.array([[bool(f(*row)) for row in rows]
                    for f in (gp.compile(t, ps) for t in pop)])
    assert 0.2 < exp.mean() < 0.8
    ev = GPUEvaluator(ps, BooleanHits(ins, outs), device=0)
    try:
        fit = ev.evaluate(pop)
        got = ev.predict(pop)
        assert got.dtype == bool and got.shape == (200, n)
        assert (got == exp).all(), np.argwhere(got != exp)[:5]
        planes = ev.ctx.run_values_bits()
        assert planes.shape == (200, (n + 31) // 32)
        if n % 32:
            assert (planes[:, -1] >> np.uint32(n % 32) == 0).all()
        assert planes.any()
        # the hits the outputs imply, and the fitness after the values run
        assert [(int((g == outs.astype(bool)).sum()),) for g in got] == fit
        assert ev.evaluate(pop) == fit
        # other rows: the cases in reverse order
        rev = np.ascontiguousarray(ins[:, ::-1])
        assert (ev.predict(pop, X=rev) == exp[:, ::-1]).all()
        assert ev.evaluate(pop) == fit
    finally:
        ev.close()


# ---------------------------------------------------------------- 11 typed --
def _typed():
    ps = gp.PrimitiveSetTyped("TYPED8", itertools.repeat(float, 8), bool, "IN")
    ps.addPrimitive(operator.and_, [bool, bool], bool)
    ps.addPrimitive(operator.or_, [bool, bool], bool)
    ps.addPrimitive(operator.not_, [bool], bool)
    ps.addPrimitive(operator.add, [float, float], float)
    ps.addPrimitive(operator.sub, [float, float], float)
    ps.addPrimitive(operator.mul, [float, float], float)
    ps.addPrimitive(configs.protectedDiv, [float, float], float)
    ps.addPrimitive(operator.lt, [float, float], bool)
    ps.addPrimitive(operator.eq, [float, float], bool)
    ps.addPrimitive(configs.if_then_else, [bool, float, float], float)
    ps.addTerminal(False, bool)
    ps.addTerminal(True, bool)
    return ps


TYPED = ["and_(lt(IN0, IN1), eq(IN2, IN3))",
         "or_(not_(eq(IN1, IN1)), lt(IN4, IN5))",
         "if_then_else(lt(IN4, IN5), IN6, mul(IN0, IN7))",
         "if_then_else(and_(lt(IN0, IN4), not_(eq(IN1, IN2))), add(IN4, IN5), "
         "protectedDiv(IN6, IN2))",
         "lt(add(IN0, IN1), mul(IN2, IN4))",
         "and_(True, or_(False, eq(IN3, IN0)))",
         "sub(if_then_else(eq(IN0, IN1), IN5, IN6), IN7)"]


def test_typed_trees_give_bools_as_one_and_zero():
    from deap_amd.evaluator import GPUEvaluator, TypedBoolHits
    ps = _typed()
    X57, labels = datasets.spambase_like(129, 7)
    X = np.ascontiguousarray(X57[[0, 1, 2, 3, 54, 55, 56, 4]])
    pop = [gp.PrimitiveTree.from_string(s, ps) for s in TYPED]
    F, exc = pr.values(ps, pop, X)
    assert not any(exc)
    for i in (0, 1, 4, 5):                               # the bool-rooted trees
        assert set(np.unique(F[i])) <= {0.0, 1.0}
    assert len(np.unique(F[0])) == 2 and len(np.unique(F[2])) > 2
    ev = GPUEvaluator(ps, TypedBoolHits(X, labels), device=0)
    try:
        fit = ev.evaluate(pop)
        got = ev.predict(pop)
        pr.assert_same_bits(got, F, "typed")
        # (typed programs run on the C++ F kernels in a values run)
        assert ev.ctx.launch_shape("cpp_fast")["programs"] + \
            ev.ctx.launch_shape("cpp_deep")["programs"] == len(pop)
        assert ev.evaluate(pop) == fit                   # the hits, by the typed core again
    finally:
        ev.close()


if __name__ == "__main__":
    child(sys.argv[1])
