"""abs and sqrt with Python semantics, on the host (no GPU): what the
flattener accepts and refuses, its folding and NEG peephole, the native
flattener's words against the Python specification, the exact-integer pass's
two interpreters against Python's own numbers, and the range pass's model of
the two opcodes against sampled evaluation."""
import math
import operator

import numpy as np
import pytest

import abs_sqrt_ref as asr
from deap_amd import _lib, configs, gp
from deap_amd.flatten import (ERR_CONST, ExactIntRangeError, Flattener, Op,
                              analyse_pset)


def _pset(*fns, **named):
    ps = gp.PrimitiveSet("AS", 2)
    ps.addPrimitive(operator.add, 2)
    ps.addPrimitive(operator.sub, 2)
    ps.addPrimitive(operator.mul, 2)
    ps.addPrimitive(operator.neg, 1)
    ps.addPrimitive(configs.protectedDiv, 2)
    for fn in fns:
        ps.addPrimitive(fn, 1)
    for name, fn in named.items():
        ps.addPrimitive(fn, 1, name=name)
    return ps


def _words(fl, expr, py=False):
    tree = gp.PrimitiveTree.from_string(expr, fl.pset)
    b = (fl.flatten_py if py else fl.flatten)([tree])
    return [int(w) for w in b.code], b


def _ops(words):
    return [w & 0xff for w in words]


# ------------------------------------------------------------- flattener --
def test_every_callable_of_the_table_is_accepted():
    table = [(abs, "abs"), (operator.abs, "abs"), (math.fabs, "fabs"),
             (np.abs, "npabs"), (np.absolute, "npabs"), (np.fabs, "npabs"),
             (math.sqrt, "sqrt"), (np.sqrt, "npsqrt"),
             (configs.psqrt, "psqrt"),
             (lambda x: math.sqrt(abs(x)), "psqrt"),
             (lambda x: math.sqrt(math.fabs(x)), "psqrt")]
    for fn, sem in table:
        spec = analyse_pset(_pset(f=fn))
        assert spec.prim_ops["f"] == sem, (fn, spec.prim_ops)
    assert Op.ABS == 53 and Op.SQRT == 54


def test_other_primitives_and_protected_variants_stay_refused():
    """The set with abs and math.sqrt is accepted; the same set with one more
    primitive that has no GPU implementation is refused, by that name."""
    eps = 1e-12
    spec = Flattener(_pset(abs, math.sqrt)).spec
    assert spec.raises_value and not spec.has_trig
    assert not Flattener(_pset(abs)).spec.raises_value
    for fn in (max, np.minimum, math.exp, math.log, math.tanh):
        ps = gp.PrimitiveSet("R", 2)
        ps.addPrimitive(fn, 2 if fn in (max, np.minimum) else 1, name="f")
        with pytest.raises(NotImplementedError, match="f"):
            Flattener(ps)
    for fn in (lambda x: math.sqrt(x) if x > 0 else 0,
               lambda x: math.sqrt(abs(x) + eps),
               lambda x: math.sqrt(abs(x)) if abs(x) > 1e-6 else 0.0):
        with pytest.raises(NotImplementedError, match="f"):
            Flattener(_pset(f=fn))


def test_folding_uses_the_callables_own_semantics():
    ps = _pset(abs, math.fabs, math.sqrt)
    for fl_py in (False, True):
        fl = Flattener(ps)
        for expr, want in (("add(ARG0, abs(-3))", 3), ("add(ARG0, fabs(-3))", 3.0),
                           ("add(ARG0, sqrt(4))", 2.0),
                           ("add(ARG0, sqrt(abs(-2)))", math.sqrt(2.0))):
            w, b = _words(fl, expr, fl_py)
            assert _ops(w)[:2] == [Op.LDV, Op.ADD + 2] and b.err[0] == 0
            assert asr.ref._f64(w[2], w[3]) == want
        # the folded constant's type, from the specification's own record
        for expr, typ in (("abs(-3)", int), ("fabs(-3)", float), ("sqrt(4)", float)):
            rec = fl._build(gp.PrimitiveTree.from_string(expr, ps))
            assert rec[0] == "c" and type(rec[1].value) is typ, expr
        for expr in ("sqrt(-1.0)", "add(ARG0, sqrt(-1.0))", "sqrt(neg(4))"):
            w, b = _words(fl, expr, fl_py)
            assert b.err[0] == ERR_CONST and w == [Op.END]
            assert type(b.const_exc[0]) is ValueError


def test_psqrt_is_two_words_for_one_node():
    fl = Flattener(configs.pset_for("symreg10_abs"))
    for py in (False, True):
        w, b = _words(fl, "psqrt(ARG3)", py)
        assert w == [Op.LDV | 3 << 16, Op.ABS, Op.SQRT, Op.END]
        assert b.length[0] == 2 and b.depth[0] == 0      # the tree's length
    w, _ = _words(Flattener(_pset(math.fabs)), "fabs(ARG1)")
    assert w == [Op.LDV | 1 << 16, Op.ABS | 1 << 16, Op.END]


def test_neg_peephole_before_sqrt_and_abs():
    fl = Flattener(configs.pset_for("symreg10_sqrt"))
    X = np.array([[4.0, -4.0, 0.0, -0.0, 2.25, math.nan, math.inf, -math.inf]] * 10)
    for py in (False, True):
        w, _ = _words(fl, "sqrt(neg(ARG0))", py)
        assert _ops(w) == [Op.LDV, Op.NEG, Op.SQRT, Op.END]
        w, _ = _words(fl, "sqrt(neg(neg(ARG0)))", py)
        assert _ops(w) == [Op.LDV, Op.SQRT, Op.END]
        # a NEG that an add absorbed or a mul carried is written before SQRT
        w, _ = _words(fl, "sqrt(mul(ARG1, neg(ARG0)))", py)
        assert _ops(w)[-3:] == [Op.NEG, Op.SQRT, Op.END]
        T, verr = asr.run_f(w, X)
        # -(x * x) < 0 except for the zeros and the nan
        assert verr.tolist() == [True, True, False, False, True, False, True, True]
        # before abs the NEG is dropped or written: the same values
        w, _ = _words(fl, "abs(neg(ARG0))", py)
        assert _ops(w) in ([Op.LDV, Op.ABS, Op.END], [Op.LDV, Op.NEG, Op.ABS, Op.END])
        T, verr = asr.run_f(w, X)
        exp = np.abs(X[0])
        assert not verr.any() and np.array_equal(T.view(np.uint64), exp.view(np.uint64))
        w, _ = _words(fl, "sub(ARG1, abs(neg(ARG0)))", py)
        T, _ = asr.run_f(w, X)
        with np.errstate(invalid="ignore"):
            exp = X[1] - exp
        assert np.array_equal(T.view(np.uint64), exp.view(np.uint64))


def test_native_words_equal_the_python_flattener_on_seeded_trees():
    """2,000 seeded symreg10_sqrt trees: the native flattener (lower_core.h,
    which the device lowering compiles too) emits the specification's words,
    depths, errors and exceptions."""
    ps = configs.pset_for("symreg10_sqrt")
    pop = configs.population(ps, "half", 2000, 1234, 1, 7)
    fl = Flattener(ps)
    a, b = fl.flatten(pop), fl.flatten_py(pop)
    assert np.array_equal(a.offsets, b.offsets)
    assert np.array_equal(a.code, b.code)
    assert np.array_equal(a.depth, b.depth) and np.array_equal(a.err, b.err)
    assert np.array_equal(a.length, b.length)
    assert {i: type(e) for i, e in a.const_exc.items()} == \
        {i: type(e) for i, e in b.const_exc.items()}
    ops = set(_ops(a.code.tolist()))
    assert Op.ABS in ops and Op.SQRT in ops
    assert any(type(e) is ValueError for e in b.const_exc.values())
    # the numpy flavour: nan instead of the exception, the same words
    nps = gp.PrimitiveSet("NPAS", 1)
    nps.addPrimitive(np.add, 2, name="vadd")
    nps.addPrimitive(np.sqrt, 1, name="vsqrt")
    nps.addPrimitive(np.abs, 1, name="vabs")
    nfl = Flattener(nps)
    for expr in ("vadd(ARG0, vsqrt(-1.0))", "vsqrt(vabs(ARG0))", "vadd(ARG0, vabs(-2))"):
        wa, ba = _words(nfl, expr)
        wb, bb = _words(nfl, expr, True)
        assert wa == wb and ba.err[0] == bb.err[0] == 0, expr


# ------------------------------------------------------------ exact pass --
def _same(a, b):
    if isinstance(a, BaseException) or isinstance(b, BaseException):
        return type(a) is type(b)
    if isinstance(a, bool):
        a = int(a)
    if isinstance(a, int) or isinstance(b, int):
        return isinstance(a, int) and isinstance(b, int) and a == b
    if math.isnan(a):
        return math.isnan(b)
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


def _host(fn, code, ints, x):
    try:
        return fn(code, ints, [x, 0.0])
    except (ValueError, OverflowError, ExactIntRangeError) as exc:
        return exc


# a per-case Python int: protectedDiv's int 1 where ARG0 - ARG0 divides
ONE = "protectedDiv(ARG0, sub(ARG0, ARG0))"
B53, B1023, B1024, B1088 = 2 ** 53 + 1, 2 ** 1023 + 12345, 2 ** 1024, 2 ** 1090 + 7
EXACT_EXPRS = [
    "abs(sub({one}, {b}))", "abs(neg(add({one}, {b})))", "abs(mul({one}, -{b}))",
    "sub(abs(sub({one}, {b})), {b})", "fabs(sub({one}, {b}))",
    "sqrt(add({one}, {b}))", "sqrt(sub({one}, {b}))", "sqrt(abs(sub({one}, {b})))",
    "psqrt(sub({one}, {b}))", "add(fabs(mul({one}, -{b})), ARG0)",
    "mul(sqrt(mul(add({one}, {b}), add({one}, {b}))), ARG0)",
]


def test_exact_pass_matches_python_numbers():
    ps = _pset(abs, math.fabs, math.sqrt, psqrt=configs.psqrt)
    fl = Flattener(ps)
    exprs = [e.format(one=ONE, b=b) for e in EXACT_EXPRS
             for b in (B53, B1023, B1024, B1088)]
    trees = [gp.PrimitiveTree.from_string(e, ps) for e in exprs]
    idx, code, off, depth, ints, refused = fl.exact_programs(trees)
    assert not refused
    # every tree that computes with an int past 2**53 goes to the pass (a
    # sqrt or fabs of one converts it at once: those need it for the int
    # arithmetic below them)
    assert len(idx) == len(trees), [exprs[j] for j in set(range(len(trees))) - set(idx)]
    seen = set()
    n_dev = 0
    for k, j in enumerate(idx):
        prog = code[off[k]:off[k + 1]]
        for x in (0.5, -3.0, 0.0):
            try:
                exp = gp.compile(trees[j], ps)(x, 0.0)
            except (ValueError, OverflowError) as exc:
                exp = exc
            big = _host(_lib.host_bigint_eval, prog, ints, x)
            assert _same(exp, big), (exprs[j][:80], x, exp, big)
            dev = _host(_lib.host_exact_eval, prog, ints, x)
            if isinstance(dev, ExactIntRangeError):     # past 1088 bits: host only
                assert "%d" % B1088 in exprs[j] or "mul(add(" in exprs[j]
                continue
            assert _same(exp, dev), (exprs[j][:80], x, exp, dev)
            n_dev += 1
            seen.add(type(exp).__name__)
    assert {"int", "float", "OverflowError", "ValueError"} <= seen, seen
    assert n_dev >= 3 * len(trees) // 2


# ------------------------------------------------------------ range pass --
GENERAL, MID, SMALL = 0, 1, 2
T_SMALL, T_MID = 0.85546875, 2.4262657165527344
RANGE_BOUNDS = {"half": (-0.5, 0.5), "unit": (-1.0, 1.0), "pos": (0.0, 4.0),
                "wide": (-50.0, 50.0)}


def _classes(fl, expr, lo, hi, nv=10):
    w, _ = _words(fl, expr)
    return list(_lib.debug_trig_classes(np.array(w, dtype=np.uint32),
                                        np.full(nv, lo), np.full(nv, hi)))


def test_range_pass_models_abs_and_sqrt():
    fl = Flattener(configs.pset_for("symreg10_sqrt"))
    # sqrt(|x|) of [-0.5, 0.5] is within [0, 0.7072]: small
    assert _classes(fl, "sin(psqrt(ARG0))", -0.5, 0.5) == [SMALL]
    assert _classes(fl, "sin(sqrt(abs(ARG0)))", -0.5, 0.5) == [SMALL]
    assert _classes(fl, "cos(psqrt(ARG0))", -1.0, 1.0) == [MID]
    assert _classes(fl, "sin(abs(add(ARG0, ARG1)))", -0.4, 0.4) == [SMALL]
    assert _classes(fl, "sin(abs(add(ARG0, ARG1)))", -1.0, 1.0) == [MID]
    assert _classes(fl, "sin(sqrt(ARG0))", 0.0, 4.0) == [MID]
    # a lower bound below 0: nan (and ValueError) downstream
    assert _classes(fl, "sin(sqrt(ARG0))", -0.5, 0.5) == [GENERAL]
    assert _classes(fl, "sin(sqrt(sub(ARG0, ARG1)))", 0.0, 0.5) == [GENERAL]
    # abs bounds a value away from 0 when its interval excludes 0
    assert _classes(fl, "sin(protectedDiv(ARG0, abs(add(ARG1, 2))))", -1.0, 1.0) \
        in ([MID], [SMALL])
    assert _classes(fl, "sin(protectedDiv(ARG0, abs(ARG1)))", -1.0, 1.0) == [GENERAL]


@pytest.mark.parametrize("name", list(RANGE_BOUNDS))
def test_range_classes_hold_for_every_sampled_case(name):
    """Sampled soundness on trees with abs and sqrt: wherever the pass proves
    a range, every sampled argument (corners and 0.0 included) is finite and
    inside glibc's own threshold for that class."""
    ps = configs.pset_for("symreg10_sqrt")
    pop = configs.population(ps, "half", 1500, 99, 1, 7)
    pop += [gp.PrimitiveTree.from_string(s, ps) for s in (
        "sin(psqrt(ARG0))", "cos(sqrt(abs(sub(ARG1, ARG2))))",
        "sin(abs(mul(ARG0, ARG1)))", "sin(sqrt(mul(ARG3, ARG3)))",
        "cos(protectedDiv(ARG0, add(1, psqrt(ARG1))))")]
    lo, hi = RANGE_BOUNDS[name]
    rng = np.random.default_rng(3)
    X = rng.uniform(lo, hi, (10, 256))
    X[:, 0], X[:, 1], X[:, 2] = lo, hi, 0.0
    for c in range(3, 43):                     # corner combinations
        X[:, c] = [(lo, hi)[(c >> (v % 5)) & 1] for v in range(10)]
    batch = Flattener(ps).flatten(pop)
    count = [0, 0, 0]
    through = 0                                # proven past an abs / a sqrt
    for i, tree in enumerate(pop):
        if batch.err[i]:
            continue
        w = batch.code[batch.offsets[i]:batch.offsets[i + 1]]
        cls = _lib.debug_trig_classes(w, np.full(10, min(lo, 0.0)), np.full(10, max(hi, 0.0)))
        args = []
        asr.run_f(w, X, args)
        assert len(cls) == len(args), str(tree)
        ops = _ops(w.tolist())
        for c, arg in zip(cls, args):
            count[c] += 1
            if c == GENERAL:
                continue
            assert np.all(np.isfinite(arg)), (name, str(tree)[:160])
            assert np.abs(arg).max() < (T_SMALL if c == SMALL else T_MID), \
                (name, str(tree)[:160])
            through += Op.ABS in ops or Op.SQRT in ops
    print("ASRANGE|%s|general=%d mid=%d small=%d through=%d" % ((name,) + tuple(count) + (through,)))
    assert sum(count) > 1000
    if name != "wide":
        assert through > 0
