"""abs and sqrt on the GPU, end to end against the reference's own evaluate
body in plain Python (``gp.compile`` per case, ``math.fsum``): fp64 MSE at 129
and 386 cases (a partial tile; a full stretch followed by a partial tile),
per-case outputs, the numpy flavour, fp32 mode, the exact-integer pass, the
device lowering, and ``GPE_EXACT_ALL=0`` / ``GPE_TILE_LOOP=0`` in fresh child
processes (the knobs are read once per context; a child is this file run as a
script).

fp64 criterion: exception type, nan, inf and 0.0 exact, else 1e-12 relative.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import abs_sqrt_ref as asr
from deap_amd import configs, datasets, gp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASES = (129, 386)
N = max(CASES)
SEED = 41                          # 300 of 300 seeded programs finite (CPU run)


def _level(k, j=[0]):
    """A balanced tree needing k + 1 stack slots, abs and psqrt at its leaves."""
    if k == 0:
        j[0] += 1
        cols = (0, 1, 2, 3, 4, 5, 7, 8, 9)          # (ARG6 holds the 1e200)
        return "add(abs(ARG%d), psqrt(ARG%d))" % (cols[j[0] % 9], cols[(j[0] + 3) % 9])
    return "%s(%s, %s)" % ("sub" if k % 2 else "add", _level(k - 1), _level(k - 1))


HAND = ["sqrt(ARG0)", "sqrt(abs(ARG0))", "psqrt(ARG0)", "sin(psqrt(ARG1))",
        "abs(sub(ARG2, ARG3))", "protectedDiv(ARG4, sqrt(abs(ARG5)))",
        "sqrt(mul(ARG6, ARG6))", "sqrt(neg(ARG0))", "abs(neg(cos(ARG7)))",
        _level(5),                 # 6 slots: the deep cores' range (6..12)
        _level(12)]                # 13 slots: the C++ deep kernel only
NEG_CASE = 128                     # ARG0's one negative value: tile 1's first


def hand_data():
    X, Y = datasets.symreg10_cases(N, 11)
    X = X.copy()
    X[0] = np.abs(X[0])
    X[0, NEG_CASE] = -0.25
    X[5, 7], X[5, 200] = 0.0, -0.0
    X[6, 3], X[6, 130] = 1e200, 1e-200     # inf (no error); underflow to 0
    return X, Y


def _prefix(X, Y, n):
    return np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(Y[:, :n])


def populations():
    ps = configs.pset_for("symreg10_sqrt")
    hand = [gp.PrimitiveTree.from_string(s, ps) for s in HAND]
    seeded = configs.population(configs.pset_for("symreg10_abs"), "half", 300, SEED, 2, 5)
    # (the same trees over symreg10_sqrt's nodes: one evaluator runs both)
    seeded = [gp.PrimitiveTree.from_string(str(t), ps) for t in seeded]
    return ps, hand, seeded


_REF = {}


def reference(which):
    """``(pop, X, Y, F, exc)``: the programs' values at every case, once."""
    if which not in _REF:
        ps, hand, seeded = populations()
        if which == "hand":
            pop, (X, Y) = hand, hand_data()
        else:
            pop, (X, Y) = seeded, datasets.symreg10_cases(N, 11)
        F, exc = asr.values(ps, pop, X)
        _REF[which] = (pop, X, Y, F, exc)
    return _REF[which]


def evaluate(which, n, spec_cls=None, **kw):
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    pop, X, Y, _, _ = reference(which)
    ev = GPUEvaluator(configs.pset_for("symreg10_sqrt"),
                      (spec_cls or SymbRegMSE)(*_prefix(X, Y, n)), device=0, **kw)
    try:
        return ev.evaluate(pop), ev
    finally:
        ev.ctx.close()


# -------------------------------------------------------- fp64 MSE cells --
@pytest.mark.parametrize("n", CASES)
def test_hand_trees_match_the_reference(n):
    pop, X, Y, F, exc = reference("hand")
    depth = _depths(pop)
    assert 6 <= depth[-2] <= 12 < depth[-1], depth
    got, ev = evaluate("hand", n)
    exp = asr.mse_reference(F, exc, Y[0], n)
    for s, g, e in zip(HAND, got, exp):
        print("ASGPU|%d|%s|%r|%r" % (n, s[:50], g if isinstance(g, BaseException) else g[0], e))
    asr.check_mse(pop, got, exp, "hand@%d" % n)
    # what the cells are for: the ValueError of tile 1, inf without an
    # error, and finite values elsewhere
    assert exp[0] == "ValueError" and exp[7] == "ValueError"
    assert math.isinf(exp[6]) and all(
        isinstance(e, float) and math.isfinite(e) for e in exp[1:6] + exp[8:])


def test_routing_only_the_tree_past_12_slots_runs_on_the_cpp_kernels():
    """After the MSE run the C++ launches count one program, the 13-slot
    tree; the sqrt(ARG0) programs' negative lane sends them through the
    cores' leave-for-the-C++-finish exit (a pair pass, not a launch of
    their own): everything else ran on the asm cores.  Without this a
    C++-only implementation would pass."""
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    for which, n_cpp in (("hand", 1), ("seeded", 0)):
        pop, X, Y, _, _ = reference(which)
        for n in CASES:
            ev = GPUEvaluator(configs.pset_for("symreg10_sqrt"),
                              SymbRegMSE(*_prefix(X, Y, n)), device=0)
            try:
                ev.evaluate(pop)
                fast = ev.ctx.launch_shape("cpp_fast")["programs"]
                deep = ev.ctx.launch_shape("cpp_deep")["programs"]
                asm = ev.ctx.launch_shape("asm_fast")["programs"] + \
                    ev.ctx.launch_shape("asm_deep")["programs"]
            finally:
                ev.ctx.close()
            assert fast + deep == n_cpp, (which, n, fast, deep)
            print("ASGPU|routing|%s@%d|asm=%d cpp_fast=%d cpp_deep=%d of %d"
                  % (which, n, asm, fast, deep, len(pop)))
            assert asm == len(pop) - n_cpp, (which, n, asm)


def _depths(pop):
    from deap_amd.flatten import Flattener
    return Flattener(configs.pset_for("symreg10_sqrt")).flatten(pop).depth.tolist()


def test_first_error_case_is_the_references():
    """sqrt(ARG0): the reference raises at ARG0's one negative case, in the
    second tile; the device reports that case as the program's first error."""
    from deap_amd import _lib
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    pop, X, Y, F, exc = reference("hand")
    assert min(exc[0]) == NEG_CASE and exc[0][NEG_CASE] == "ValueError"
    ev = GPUEvaluator(configs.pset_for("symreg10_sqrt"), SymbRegMSE(X, Y), device=0)
    try:
        batch = ev.flatten(pop[:3])
        ev.prepare(batch, pop[:3])
        hi, lo, err, flags, _ = ev.run_batch(batch)
        err = [int(e) for e in err]
    finally:
        ev.ctx.close()
    assert err[0] >> 2 == NEG_CASE and err[0] & 3 == _lib.GPE_ERR_VALUE
    assert err[1] == err[2] == _lib.GPE_NO_ERROR


@pytest.mark.parametrize("n", CASES)
def test_seeded_programs_match_the_reference(n):
    pop, X, Y, F, exc = reference("seeded")
    exp = asr.mse_reference(F, exc, Y[0], n)
    finite = sum(isinstance(e, float) and math.isfinite(e) for e in exp)
    assert finite >= 0.9 * len(pop), finite          # a bad seed is loud
    text = "".join(str(t) for t in pop)
    assert text.count("abs(") > 50 and text.count("psqrt(") > 50
    got, ev = evaluate("seeded", n)
    asr.check_mse(pop, got, exp, "seeded@%d" % n)


def test_per_case_outputs_are_bit_identical():
    """SymbRegCaseErrors, 386 cases, 40 programs: every case's squared
    residual is Python's ``d * d``, bit for bit."""
    from deap_amd.evaluator import GPUEvaluator, SymbRegCaseErrors
    ps, hand, seeded = populations()
    pop = hand[:-1] + seeded[:30]
    X, Y = hand_data()
    F, exc = asr.values(ps, pop, X)
    ev = GPUEvaluator(ps, SymbRegCaseErrors(X, Y), device=0)
    try:
        got = ev.evaluate(pop)
    finally:
        ev.ctx.close()
    n_val = 0
    for i, (tree, res) in enumerate(zip(pop, got)):
        sq, err = asr.squares(F, exc, i, Y[0])
        if err is not None:
            assert type(res).__name__ == err, (str(tree)[:80], res)
            continue
        assert not isinstance(res, BaseException), (str(tree)[:80], res)
        d = F[i] - Y[0]                     # (Python's d * d: one IEEE product;
        with np.errstate(over="ignore"):    # its d ** 2 is libm's pow)
            a, b = np.array(res), d * d
        assert a.shape == b.shape == (N,)
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), (str(tree)[:80], np.flatnonzero(~same)[:5])
        n_val += 1
    assert n_val >= 30


def test_device_sqrt_is_correctly_rounded():
    """gpe_math_probe 15 / 16 (C++) and 17 / 18 (the exact and the fp32 asm
    cores' SQRT handlers: the authority on the hardware's v_rsq_f64 /
    v_sqrt_f32 seeds) on 2**18 arguments: every binade from 2**-1074
    to 2**1023, subnormals, k * k and its two neighbours, +-0, inf, nan and
    negatives — the fp64 square root of the C++ kernels has math.sqrt's bits
    (nan for a negative argument), the fp32 one numpy's on float32."""
    from deap_amd import _lib
    rng = np.random.default_rng(17)
    n = 1 << 18
    x = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-1073, 1025, n))
    e = np.arange(-1074, 1024)
    x[:len(e)] = np.ldexp(1.0, e)
    k = rng.integers(1, 1 << 26, 20000).astype(np.float64)
    sq = k * k                                            # exact below 2**53
    x[3000:23000] = sq
    x[23000:43000] = np.nextafter(sq, 0.0)
    x[43000:63000] = np.nextafter(sq, np.inf)
    x[63000:64000] = rng.integers(1, 1 << 52, 1000).astype(np.uint64).view(np.float64)
    x[64000:64008] = [0.0, -0.0, np.inf, np.nan, 5e-324, 2.2250738585072014e-308,
                      1.7976931348623157e308, 4.0]
    x[70000:80000] = -x[70000:80000]
    x[80000:80003] = [-np.inf, -5e-324, -1.0]
    ctx = _lib.Context(0)
    try:
        y64 = ctx.math_probe(15, x)
        y32 = ctx.math_probe(16, x)
        h64 = ctx.math_probe(17, x)          # the exact core's SQRT handler
        h32 = ctx.math_probe(18, x)          # the fp32 core's
    finally:
        ctx.close()
    # the handlers: the C++ path's bits in every lane, nan where it is nan
    for a, b in ((h64, y64), (h32, y32)):
        assert (np.isnan(a) == np.isnan(b)).all()
        fin = ~np.isnan(b)
        assert np.array_equal(a[fin].view(np.uint64), b[fin].view(np.uint64))
    exp = np.array([math.sqrt(v) if not v < 0 else math.nan for v in x.tolist()])
    neg = x < 0
    assert np.isnan(y64[neg]).all() and neg.sum() > 9000
    ok = ~neg & ~np.isnan(x)
    assert np.array_equal(y64[ok].view(np.uint64), exp[ok].view(np.uint64))
    assert np.isnan(y64[np.isnan(x)]).all()
    with np.errstate(all="ignore"):
        x32 = x.astype(np.float32)
        e32 = np.sqrt(x32)
    ok = ~(x32 < 0) & ~np.isnan(x32)
    assert np.array_equal(y32[ok].astype(np.float32).view(np.uint32), e32[ok].view(np.uint32))
    assert np.isnan(y32[x32 < 0]).all()


# ------------------------------------------------------------ other modes --
def numpy_pset():
    ps = gp.PrimitiveSet("NPAS10", 10)
    ps.addPrimitive(np.add, 2, name="add")
    ps.addPrimitive(np.subtract, 2, name="sub")
    ps.addPrimitive(np.multiply, 2, name="mul")
    ps.addPrimitive(configs.np_protectedDiv, 2, name="protectedDiv")
    ps.addPrimitive(np.negative, 1, name="neg")
    ps.addPrimitive(np.cos, 1, name="cos")
    ps.addPrimitive(np.sin, 1, name="sin")
    ps.addPrimitive(np.abs, 1, name="abs")
    ps.addPrimitive(np.sqrt, 1, name="sqrt")
    ps.addPrimitive(lambda x: np.sqrt(np.abs(x)), 1, name="psqrt")
    return ps


def test_numpy_flavour_gives_nan_and_numpy_sum():
    """np.sqrt / np.abs, 129 cases: a negative argument gives nan and no
    error.  The trees without sin/cos (every operation IEEE-exact; at least 25
    of the 60) must give numpy.sum's bits; a tree with sin/cos is held to 1e-12
    relative only, because numpy's own vectorised sin/cos are not the
    reference libm's to the last bit."""
    from deap_amd.evaluator import GPUEvaluator, SymbRegNumpySSE
    from deap_amd.flatten import Flattener
    ps = numpy_pset()
    assert Flattener(ps).spec.prim_ops["sqrt"] == "npsqrt"
    _, hand, seeded = populations()
    pop = [gp.PrimitiveTree.from_string(str(t), ps) for t in hand[:-1] + seeded[:50]]
    X, Y = _prefix(*hand_data(), 129)
    ev = GPUEvaluator(ps, SymbRegNumpySSE(X, Y[0]), device=0)
    try:
        got = ev.evaluate(pop)
    finally:
        ev.ctx.close()
    n_nan = n_exact = 0
    for tree, res in zip(pop, got):
        with np.errstate(all="ignore"):
            exp = float(np.sum((gp.compile(tree, ps)(*X) - Y[0]) ** 2))
        assert not isinstance(res, BaseException), (str(tree)[:80], res)
        text = str(tree)
        if "sin(" in text or "cos(" in text:
            # (numpy's own vectorised sin/cos are not glibc's to the last bit)
            ok = res[0] == exp or (math.isfinite(exp) and
                                   abs(res[0] - exp) <= asr.REL * abs(exp))
        else:
            ok = res[0] == exp
            n_exact += 1
        assert ok or (math.isnan(exp) and math.isnan(res[0])), (text[:80], res[0], exp)
        n_nan += math.isnan(exp)
    assert math.isnan(got[0][0]) and n_nan >= 2          # sqrt(ARG0), sqrt(neg(ARG0))
    # the bit-identical cell: the trees without sin/cos, most with abs / sqrt
    assert n_exact >= 25, n_exact


def test_fp32_mode_within_its_stated_tolerance():
    """fp32 mode, the bounds test_gpu.py asserts for C4: median
    <= 1e-5, >= 80 % within 1e-4 and >= 90 % within 1e-3 relative to the
    reference's fp64 fitness; the exceptions' types are the reference's
    where fp32 can represent the argument."""
    rel, mixed, n_small = [], [], 0
    for which in ("hand", "seeded"):
        pop, X, Y, F, exc = reference(which)
        exp = asr.mse_reference(F, exc, Y[0], 129)
        got, _ = evaluate(which, 129, precision="fp32")
        for tree, res, e in zip(pop, got, exp):
            # an exception on one side only.  Counted where fp32 cannot
            # differ by range: the seeded data lie in [-1, 1], and a
            # reference MSE below 1e30 keeps every |d| below 1.2e16, far
            # from float's 1.8e19 where d * d overflows
            small = which == "seeded" and not isinstance(e, str) and e < 1e30
            n_small += small
            if isinstance(e, str) != isinstance(res, BaseException):
                if small:
                    mixed.append(str(tree)[:80])
                continue
            if isinstance(e, str):
                assert type(res).__name__ == e or which == "hand", (str(tree)[:80], res, e)
                continue
            if math.isfinite(e) and math.isfinite(res[0]):
                rel.append(abs(res[0] - e) / max(abs(e), 1e-300))
        if which == "hand":
            assert isinstance(got[0], ValueError) and isinstance(got[7], ValueError)
    rel = np.array(rel)
    print("ASGPU|fp32|n=%d median=%.3g within1e-4=%.3f within1e-3=%.3f"
          % (len(rel), np.median(rel), (rel <= 1e-4).mean(), (rel <= 1e-3).mean()))
    print("ASGPU|fp32|exception on one side only: %d of %d %r" % (len(mixed), n_small, mixed[:3]))
    # (what is left: an intermediate past float's 3.4e38 that the final
    # value does not show, sin/cos of it raising in fp32 only)
    assert n_small > 250 and len(mixed) <= n_small // 100
    assert len(rel) > 250
    assert np.median(rel) <= 1e-5 and (rel <= 1e-4).mean() >= 0.80 \
        and (rel <= 1e-3).mean() >= 0.90


def test_exact_integer_pass_on_the_device():
    """The CPU suite's int cases through the evaluator: abs keeps ints past
    2**53 exact, fabs / sqrt convert (OverflowError past 2**1024), sqrt of a
    negative int raises ValueError."""
    import test_abs_sqrt as cpu
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    ps = cpu._pset(abs, math.fabs, math.sqrt, psqrt=configs.psqrt)
    exprs = [e.format(one=cpu.ONE, b=b) for e in cpu.EXACT_EXPRS
             for b in (cpu.B53, cpu.B1023, cpu.B1024, cpu.B1088)]
    pop = [gp.PrimitiveTree.from_string(e, ps) for e in exprs]
    X = np.array([[0.5, -3.0, 0.0, 1.25, -0.75, 2.0, 7.5],
                  [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]])
    Y = np.array([[float(cpu.B53), 0.0, 1.0, -1.0, 2.0 ** 60, 3.0, 5.0]])
    F_exc = [asr.values(ps, [t], X) for t in pop]
    ev = GPUEvaluator(ps, SymbRegMSE(X, Y), device=0)
    try:
        got = ev.evaluate(pop)
        assert ev.stats["exact_programs"] == len(pop)
    finally:
        ev.ctx.close()
    exp = [asr.mse_reference(F, exc, Y[0])[0] for F, exc in F_exc]
    asr.check_mse(pop, got, exp, "exact")
    kinds = {e if isinstance(e, str) else "value" for e in exp}
    assert kinds == {"value", "OverflowError", "ValueError"}, kinds


def test_device_lowering_matches_the_host_flattener():
    """2,000 seeded symreg10_sqrt trees lowered on the GPU: the host
    flattener's depths, errors and exceptions, and bit-identical fitness."""
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    ps = configs.pset_for("symreg10_sqrt")
    pop = configs.population(ps, "half", 2000, 1234, 1, 7)
    X, Y = _prefix(*datasets.symreg10_cases(N, 11), 129)
    ev = GPUEvaluator(ps, SymbRegMSE(X, Y), device=0)
    try:
        dev = ev.lower_on_device(pop)
        assert dev is not None, "device lowering declined the batch"
        host = ev.flattener.flatten(pop)
        assert np.array_equal(dev.depth, host.depth)
        assert np.array_equal(dev.err, host.err)
        assert sorted(dev.const_exc) == sorted(host.const_exc) and dev.const_exc
        got_dev = ev.evaluate(pop)
        ev.device_lowering = False
        got_host = ev.evaluate(pop)
    finally:
        ev.ctx.close()
    for tree, a, b in zip(pop, got_dev, got_host):
        if isinstance(a, BaseException) or isinstance(b, BaseException):
            assert type(a) is type(b), (str(tree)[:80], a, b)
        else:
            assert a == b or (math.isnan(a[0]) and math.isnan(b[0])), (str(tree)[:80], a, b)
    assert any(isinstance(a, ValueError) for a in got_dev)


# ------------------------------------------------------- child processes --
def _fit(results):
    return [type(r).__name__ if isinstance(r, BaseException) else [float(v).hex() for v in r]
            for r in results]


def _unfit(fit):
    return [{"ValueError": ValueError, "OverflowError": OverflowError,
             "ZeroDivisionError": ZeroDivisionError}[f]() if isinstance(f, str)
            else tuple(float.fromhex(v) for v in f) for f in fit]


def child(out):
    res = {which: _fit(evaluate(which, 129)[0]) for which in ("hand", "seeded")}
    with open(out, "w") as fh:
        json.dump(res, fh)


@pytest.mark.parametrize("knob", ["GPE_EXACT_ALL", "GPE_TILE_LOOP"])
def test_knobs_off_give_the_reference_too(tmp_path, knob):
    """``GPE_EXACT_ALL=0`` and ``GPE_TILE_LOOP=0``, each in a fresh process:
    the reference's results by the same criterion; without the resident tile
    loop also the default run's bits."""
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
    for which in ("hand", "seeded"):
        pop, X, Y, F, exc = reference(which)
        asr.check_mse(pop, _unfit(res[which]), asr.mse_reference(F, exc, Y[0], 129),
                      "%s=0 %s" % (knob, which))
        if knob == "GPE_TILE_LOOP":
            assert res[which] == _fit(evaluate(which, 129)[0]), which


if __name__ == "__main__":
    child(sys.argv[1])
