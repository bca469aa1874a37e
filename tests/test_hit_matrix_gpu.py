"""The hit matrix of a call is resolved in one place (csrc/hit_matrix.h) for
all of its consumers: ``lexicase_bits_par``, ``lexicase_bits``,
``informed_cases``, ``hit_group_counts`` and the case-weight calls.  What a
shared resolver could get wrong is what these tests pin: whichever consumer
comes first after a run makes the cached case-major transpose and the others
must find it right; a call on a caller's matrix of another shape in between
must not touch the resident one; the F machine's thresholded scratch is shared
between calls that name different ``eps``; and the calls without an ``eps``
keep refusing an F context that has no hit planes.

The shapes are those around the 32-case plane word and the 64-program word of
the transpose: n in {1, 64, 65, 130}, n_cases in {1, 32, 33, 97}."""
import itertools
import random

import numpy as np
import pytest

from deap_amd import _lib, configs, gp
from deap_amd.evaluator import (BooleanCaseHits, GPUEvaluator, SymbRegCaseAbsErrors,
                                unpack_bitplanes)

pytestmark = pytest.mark.gpu

NS = (1, 64, 65, 130)
CASES = (1, 32, 33, 97)
SEED = 0x9E3779B97F4A7C15
HIT_EPS = 0.25
NAMES = ("bits_par", "bits", "informed", "groups", "weights")
_CACHE = {}


@pytest.fixture(scope="module")
def plain():
    """A context of its own for the calls on explicit planes: what they give
    is what the resident routes of another context must give."""
    c = _lib.Context(0)
    yield c
    c.close()


def call_inputs(n, n_cases, seed):
    """The other arguments of the five consumers for an [n, n_cases] matrix:
    masks with pad bits set, dyadic weights (any order of the sum gives the
    same bits), a live mask with dead programs where there is more than one."""
    rng = np.random.default_rng(seed)
    units = (n_cases + 31) // 32
    masks = rng.integers(0, 1 << 32, size=(3, units), dtype=np.uint64).astype(np.uint32)
    w = rng.integers(0, 1 << 20, size=(2, n_cases)).astype(np.float64) / 1024.0
    alive = rng.random(n) < 0.7
    alive[0] = True
    return dict(masks=masks, w=w, live=_lib.pack_live_mask(alive) if n > 1 else None,
                m=min(n_cases, 5), k=6)


def flat(x):
    """A call's result as a list of arrays, floats by their bits."""
    out = []
    for a in x if isinstance(x, tuple) else (x,):
        a = np.ascontiguousarray(a)
        out.append(a.view(np.uint64) if a.dtype == np.float64 else a)
    return out


def same(a, b):
    a, b = flat(a), flat(b)
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y)
                                    for x, y in zip(a, b))


def consume(c, name, matrix, inp, eps=0.0):
    """Consumer *name* of context *c* on *matrix*: ``(planes, n, n_cases)`` or
    ``(None, 0, 0)``, the resident one."""
    if name == "bits_par":
        idx, failed = c.lexicase_bits_par(*matrix, inp["k"], SEED)
        return idx, np.int64(failed)
    if name == "bits":
        rng = random.Random(5)
        idx, failed = c.lexicase_bits(*matrix, inp["k"], rng)
        return idx, np.int64(failed), np.array(rng.getstate()[1], dtype=np.uint64)
    if name == "informed":
        return c.informed_cases(*matrix, eps, SEED, inp["m"])
    if name == "groups":
        return c.hit_group_counts(*matrix, inp["masks"])
    return (c.case_solve_counts(*matrix, eps, inp["live"]),
            c.hit_weighted_sums(*matrix, inp["w"], eps))


def twin(name, planes, n_cases, inp):
    """The host twin's result, or None where the library has none (the
    replaying ``lexicase_bits`` follows Python's ``random``)."""
    if name == "bits_par":
        hit = unpack_bitplanes(planes, n_cases).astype(np.float64)
        idx, failed = _lib.host_lexicase_par(hit, np.ones(n_cases, dtype=np.uint8), inp["k"],
                                             SEED, 0)
        return idx, np.int64(failed)
    if name == "informed":
        return _lib.host_informed_cases(planes, n_cases, SEED, inp["m"])
    if name == "groups":
        return _lib.host_hit_group_counts(planes, n_cases, inp["masks"])
    if name == "weights":
        return (_lib.host_case_solve_counts(planes, n_cases, inp["live"]),
                _lib.host_hit_weighted_sums(planes, n_cases, inp["w"]))
    return None


def expected(plain, planes, n_cases, inp):
    """Every consumer on the explicit *planes*, checked against its twin."""
    exp = {}
    for name in NAMES:
        exp[name] = consume(plain, name, (planes, len(planes), n_cases), inp)
        t = twin(name, planes, n_cases, inp)
        assert t is None or same(exp[name], t), name
    return exp


def other_matrix(plain):
    """A caller's matrix of another shape (7 programs, 45 cases: other W, other
    units) and what the consumers give on it."""
    if "other" not in _CACHE:
        rng = np.random.default_rng(45)
        planes = rng.integers(0, 1 << 32, size=(7, 2), dtype=np.uint64).astype(np.uint32)
        inp = call_inputs(7, 45, 7)
        _CACHE["other"] = (planes, inp, expected(plain, planes, 45, inp))
    return _CACHE["other"]


# ---------------------------------------------------------------- B machine --
def parity_pop():
    if "parity" not in _CACHE:
        ps = configs.pset_for("parity6")
        _CACHE["parity"] = (ps, configs.population(ps, "half", max(NS), 13, 2, 5))
    return _CACHE["parity"]


@pytest.mark.parametrize("n, n_cases", list(itertools.product(NS, CASES)))
def test_every_consumer_may_be_the_first_after_a_run(plain, n, n_cases):
    ps, pop = parity_pop()
    pop = pop[:n]
    rng = np.random.default_rng(n * 1000 + n_cases)
    ins = rng.integers(0, 2, (6, n_cases)).astype(np.uint8)
    outs = rng.integers(0, 2, n_cases).astype(np.uint8)
    inp = call_inputs(n, n_cases, n + n_cases)
    o_planes, o_inp, o_exp = other_matrix(plain)
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, "device"), device=0)
    try:
        c = ev.ctx
        exp = None
        for first in range(len(NAMES)):
            ev.evaluate(pop)                               # (run_hit_planes: no transpose yet)
            planes = c.hit_planes(n)
            if exp is None:
                exp = expected(plain, planes, n_cases, inp)
            for j in range(len(NAMES)):
                name = NAMES[(first + j) % len(NAMES)]
                assert same(consume(c, name, (None, 0, 0), inp), exp[name]), (first, name)
                # a caller's matrix of another shape in between, by another consumer
                o_name = NAMES[(first + j + 2) % len(NAMES)]
                assert same(consume(c, o_name, (o_planes, 7, 45), o_inp), o_exp[o_name]), o_name
            assert np.array_equal(c.hit_planes(n), planes)
    finally:
        ev.close()


# ---------------------------------------------------------------- F machine --
HAND = ["ARG0", "ARG3", "sub(ARG3, ARG3)", "mul(ARG0, ARG1)", "add(ARG0, 1)",
        "add(mul(ARG0, ARG1), ARG2)", "neg(ARG2)", "mul(ARG3, ARG4)"]


def regression():
    """``(pset, 130 trees without sin/cos, X [10, 97], y)``: small integers, so
    that many errors are exactly 0, 1, 2 ...; an error of exactly HIT_EPS (tree
    ``ARG0`` at case 5), an inf and a nan (ARG3 at case 9)."""
    if "reg" not in _CACHE:
        ps = configs.pset_for("symreg10_notrig")
        rng = np.random.default_rng(97)
        X = rng.integers(-2, 3, (10, max(CASES))).astype(np.float64)
        y = X[0] * X[1] + X[2]
        y[5] = X[0, 5] + HIT_EPS
        X[3, 9] = np.inf
        trees = [gp.PrimitiveTree.from_string(s, ps) for s in HAND] + \
            configs.population(ps, "half", max(NS) - len(HAND), 29, 1, 4)
        _CACHE["reg"] = (ps, trees, X, y)
    return _CACHE["reg"]


def refused(call):
    with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs") as info:
        call()
    assert "(-3)" in str(info.value)


@pytest.mark.parametrize("n, n_cases", list(itertools.product(NS, CASES)))
def test_the_f_machine_thresholds_for_the_calls_with_an_eps_only(plain, n, n_cases):
    ps, trees, X, y = regression()
    trees = trees[:n]
    spec = SymbRegCaseAbsErrors(np.ascontiguousarray(X[:, :n_cases]), y[:n_cases],
                                hit_eps=HIT_EPS, cases="host")
    inp = call_inputs(n, n_cases, 3 * n + n_cases)
    ev = GPUEvaluator(ps, spec, device=0)
    try:
        fit = ev.evaluate(trees)                           # (run_abserr_cases)
        assert not any(isinstance(f, BaseException) for f in fit)
        E = np.array(fit, dtype=np.float64).reshape(n, n_cases)
        c = ev.ctx
        H = {eps: _lib.host_hit_threshold(E, eps) for eps in (HIT_EPS, 1.0)}
        if n_cases > 9 and n > 2:
            assert not same(H[HIT_EPS], H[1.0]) and np.isinf(E[1, 9]) and np.isnan(E[2, 9])
        # two thresholds in alternation: the thresholded scratch is one
        steps = list(zip(("informed", "counts", "shared") * 2, (HIT_EPS, 1.0) * 3))
        for what, eps in steps + steps[::-1]:
            if what == "informed":
                got = c.informed_cases(None, 0, 0, eps, SEED, inp["m"])
                exp = _lib.host_informed_cases(H[eps], n_cases, SEED, inp["m"])
            elif what == "counts":
                got = c.case_solve_counts(None, 0, 0, eps, inp["live"])
                exp = _lib.host_case_solve_counts(H[eps], n_cases, inp["live"])
            else:
                got = c.hit_shared_sums(None, 0, 0, eps, inp["live"])
                exp = _lib.host_hit_shared_sums(H[eps], n_cases, inp["live"])
            assert same(got, exp), (what, eps)
        # no eps to threshold by: no hit planes, as before
        refused(lambda: c.lexicase_bits(None, 0, 0, 2, random.Random(1)))
        refused(lambda: c.lexicase_bits_par(None, 0, 0, 2, SEED))
        refused(lambda: c.hit_group_counts(None, 0, 0, inp["masks"]))
        # a typed hit-planes run of the same programs: all five serve its planes
        planes, hits, err = c.run_typed_hit_planes()
        assert np.array_equal(c.hit_planes(n), planes)
        exp = expected(plain, planes, n_cases, inp)
        for name in NAMES[2:] + NAMES[:2]:
            assert same(consume(c, name, (None, 0, 0), inp, eps=1.0), exp[name]), name
        assert np.array_equal(c.hit_planes(n), planes)
    finally:
        ev.close()
