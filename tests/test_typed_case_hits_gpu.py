"""``TypedCaseHits`` on the GPU: the hit planes of typed classifiers
(``gpe_run_typed_hit_planes``) bit for bit against the plain-Python reference
``bool(gp.compile(tree, pset)(*row)) is bool(label)``, on every route — the
typed core's hit-planes variant, the C++ kernels (programs past five stack
slots), the constant fill and the exact-integer pass — at ragged case counts
and launch geometries, and the selections, the informed subsets and the
residency rules that rest on the matrix."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from deap_amd import _lib, configs, datasets, gp, tools
from deap_amd.evaluator import GPUEvaluator, TypedBoolHits, TypedCaseHits, unpack_bitplanes

pytestmark = pytest.mark.gpu

N_MAX = 300
KNOBS = ("GPE_TYPED_WAVES", "GPE_TYPED_PMAX", "GPE_TYPED_TARGET_BLOCKS", "GPE_MIN_GROUP_TILES",
         "GPE_TYPED_ASM", "GPE_ASM", "GPE_TARGET_BLOCKS", "GPE_F_WAVES")
_CACHE = {}


def _full(depth, leaf):
    """A full binary tree of add / mul over distinct columns: *depth* + 1
    values live at once, more than the typed core's five stack slots."""
    if depth == 0:
        return "IN%d" % (next(leaf) % 57)
    return "%s(%s, %s)" % ("add" if depth % 2 else "mul", _full(depth - 1, leaf),
                           _full(depth - 1, leaf))


def inputs():
    """(pset, trees, X, labels, hit): about 600 generated classifiers (more
    than one 64-program wave, more than one 512-program block) and hand-built
    trees for every route; hit[i, c] is the reference, computed once."""
    if "data" in _CACHE:
        return _CACHE["data"]
    ps = configs.pset_for("spambase")
    X, lab = datasets.spambase_like(N_MAX, 57)
    trees = configs.population(ps, "half", 600, 57, 2, 4)
    one = "protectedDiv(IN0, sub(IN1, IN1))"               # the int 1 (a zero divisor)
    big = "add(%s, %s)" % (one, one)
    for _ in range(6):
        big = "mul(%s, %s)" % (big, big)                   # the int 2 ** 64: the exact pass
    hand = ["True", "False", "lt(1.0, 2.0)", "not_(eq(3.0, 3.0))",         # constants
            "lt(IN0, IN1)", "and_(lt(IN3, IN4), not_(eq(IN5, IN6)))",
            "lt(%s, %s)" % (_full(7, iter(range(10 ** 6))), _full(6, iter(range(7, 10 ** 6)))),
            "lt(if_then_else(lt(IN1, IN2), %s, IN3), 1.5)" % _full(7, iter(range(3, 10 ** 6))),
            "lt(%s, IN0)" % big]
    trees = trees + [gp.PrimitiveTree.from_string(s, ps) for s in hand]
    rows = list(zip(*X.tolist()))
    labels = [bool(v) for v in lab.tolist()]
    hit = np.zeros((len(trees), N_MAX), dtype=bool)
    for i, tree in enumerate(trees):
        func = gp.compile(tree, ps)
        hit[i] = [bool(func(*r)) is b for r, b in zip(rows, labels)]
    _CACHE["data"] = (ps, trees, X, lab, hit)
    return _CACHE["data"]


def make(monkeypatch, n_cases, cases="device", knobs=None, cls=TypedCaseHits):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (knobs or {}).items():
        monkeypatch.setenv(k, str(v))
    ps, trees, X, lab, hit = inputs()
    spec = cls(X[:, :n_cases], lab[:n_cases], cases) if cls is TypedCaseHits \
        else cls(X[:, :n_cases], lab[:n_cases])
    return GPUEvaluator(ps, spec, device=0)


def check_routes(ev, got):
    """Every route held a program and nobody was skipped."""
    geo = ev.ctx.geometry()
    assert geo["asm_typed"] >= 1 and geo["typed_const"] >= 1, geo
    assert geo["fast"] + geo["deep"] >= 1, geo             # the C++ kernels
    assert ev.stats.get("exact_programs", 0) >= 1          # the exact-integer pass
    assert len(got) == ev.ctx.n_prog
    assert geo["asm_typed"] + geo["typed_const"] + geo["fast"] + geo["deep"] == len(got), geo
    assert all(type(r) is tuple for r in got), [r for r in got if type(r) is not tuple][:1]
    return geo


def raw_planes(ev, n):
    return ev.ctx.hit_planes(n)


def counts(monkeypatch, n_cases, knobs=None):
    """TypedBoolHits' counts of the batch (the count-only kernels)."""
    ps, trees, X, lab, hit = inputs()
    ev = make(monkeypatch, n_cases, knobs=knobs, cls=TypedBoolHits)
    try:
        return [h for (h,) in ev.evaluate(trees)]
    finally:
        ev.close()


# ------------------------------------------------------------------ bits --
@pytest.mark.parametrize("n_cases", [1, 63, 64, 65, 127, 128, 129, 200, 300])
def test_the_planes_are_the_reference_bit_for_bit(monkeypatch, n_cases):
    ps, trees, X, lab, hit = inputs()
    exp = hit[:, :n_cases]
    plain = counts(monkeypatch, n_cases)
    assert plain == exp.sum(axis=1).tolist()
    for cases in ("device", "host"):
        ev = make(monkeypatch, n_cases, cases)
        try:
            got = ev.evaluate(trees)
            check_routes(ev, got)
            mat = ev.last_case_hits()
            assert mat.dtype == bool and mat.shape == exp.shape
            assert np.array_equal(mat, exp), np.argwhere(mat != exp)[:5]
            raw = raw_planes(ev, len(trees))
            units = (n_cases + 31) // 32
            assert raw.shape == (len(trees), units)
            if n_cases % 32:                               # the pad bits of the raw words
                assert not (raw[:, -1] >> np.uint32(n_cases % 32)).any()
            assert np.array_equal(unpack_bitplanes(raw, n_cases), exp)
            assert ev.last_hits.dtype == np.int64
            assert ev.last_hits.tolist() == exp.sum(axis=1).tolist() == plain
            if cases == "device":
                assert got == [(h,) for h in plain]
            else:
                assert got == [tuple(r) for r in exp.astype(np.int64).tolist()]
                assert all(type(v) is int for v in got[0])
        finally:
            ev.close()


# -------------------------------------------------------------- geometry --
# the planner takes P = min(GPE_TYPED_PMAX, programs * tiles / (4 * GPE_TARGET_BLOCKS)):
# the batch repeated REP times (the same rows REP times) reaches P >= 38 at two tiles
REP = 64
GEO_BASE = {"GPE_TARGET_BLOCKS": 256}


def default_planes(monkeypatch, n_cases, rep=1):
    key = ("default", n_cases, rep)
    if key not in _CACHE:
        ps, trees, X, lab, hit = inputs()
        ev = make(monkeypatch, n_cases)
        try:
            ev.evaluate(trees * rep)
            _CACHE[key] = raw_planes(ev, len(trees) * rep)
        finally:
            ev.close()
    return _CACHE[key]


@pytest.mark.parametrize("n_cases", [129, 300])
@pytest.mark.parametrize("waves, pmax", [(1, 1), (1, 38), (1, 64), (8, 1), (8, 38), (8, 64)])
def test_the_matrix_does_not_depend_on_the_typed_launch_geometry(monkeypatch, n_cases, waves,
                                                                 pmax):
    ps, trees, X, lab, hit = inputs()
    base = default_planes(monkeypatch, n_cases, REP)
    ev = make(monkeypatch, n_cases,
              knobs=dict(GEO_BASE, GPE_TYPED_WAVES=waves, GPE_TYPED_PMAX=pmax))
    try:
        got = ev.evaluate(trees * REP)
        geo = check_routes(ev, got)
        s = ev.ctx.launch_shape("typed")
        tiles = -(-n_cases // 128)
        assert s["programs"] == geo["asm_typed"] and s["n_tiles"] == tiles, s
        assert s["wpb"] == waves and s["P"] == min(pmax, s["programs"] * tiles // 1024), s
        assert s["P"] == pmax or s["P"] >= 38, s           # (lane 37 and beyond hold programs)
        raw = raw_planes(ev, len(trees) * REP)
        assert np.array_equal(raw, base)
        assert np.array_equal(unpack_bitplanes(raw, n_cases), np.tile(hit[:, :n_cases], (REP, 1)))
    finally:
        ev.close()


@pytest.mark.parametrize("knobs, groups, tiles_per_group", [
    # every tile a group of its own: two blocks write neighbouring words of a row
    ({"GPE_TYPED_TARGET_BLOCKS": 32768}, 3, 1),
    # one group walks all three tiles: the lanes' plane registers are reused
    ({"GPE_TYPED_TARGET_BLOCKS": 256, "GPE_TYPED_WAVES": 1, "GPE_TYPED_PMAX": 1}, 1, 3)])
def test_tile_groups_and_tile_loops_write_the_same_words(monkeypatch, knobs, groups,
                                                         tiles_per_group):
    ps, trees, X, lab, hit = inputs()
    base = default_planes(monkeypatch, 300)
    ev = make(monkeypatch, 300, knobs=knobs)
    try:
        got = ev.evaluate(trees)
        check_routes(ev, got)
        s = ev.ctx.launch_shape("typed")
        assert s["groups"] == groups and s["tiles_per_group"] == tiles_per_group, s
        if groups > 1:
            assert s["groups"] >= 2
        assert np.array_equal(raw_planes(ev, len(trees)), base)
    finally:
        ev.close()


# ------------------------------------------------------------- selection --
def _wrapped(values):
    w = (1.0,) * len(values[0])
    return [SimpleNamespace(fitness=SimpleNamespace(values=v, weights=w), idx=i)
            for i, v in enumerate(values)]


def test_select_lexicase_replays_tools_sellexicase_and_the_parallel_twin(monkeypatch):
    ps, trees, X, lab, hit = inputs()
    n_cases = 200
    host = make(monkeypatch, n_cases, "host")
    try:
        values = host.evaluate(trees)
    finally:
        host.close()
    random.seed(77)
    want = [ind.idx for ind in tools.selLexicase(_wrapped(values), 50)]
    want_state = random.getstate()
    ev = make(monkeypatch, n_cases, "device")
    try:
        got = ev.evaluate(trees)
        check_routes(ev, got)
        index = {id(t): i for i, t in enumerate(trees)}
        for args in ((), ("plain",), ("epsilon", 0.5)):
            random.seed(77)
            picks = [index[id(t)] for t in ev.select_lexicase(trees, 50, *args)]
            assert picks == want, args
            assert random.getstate() == want_state, args
        for eps in (1.0, -0.5):
            with pytest.raises(ValueError, match=r"epsilon must be in \[0, 1\)"):
                ev.select_lexicase(trees, 5, "epsilon", eps)
        random.seed(78)
        picks = [index[id(t)] for t in ev.select_lexicase(trees, 50, parallel=True)]
        seed = ev.last_lexicase_seed
        assert seed == random.Random(78).getrandbits(64)
        mat = ev.last_case_hits().astype(np.float64)
        exp, failed = _lib.host_lexicase_par(mat, np.ones(n_cases, dtype=np.uint8), 50, seed)
        assert failed == -1 and picks == exp.tolist()
    finally:
        ev.close()


# -------------------------------------------------------------- informed --
def test_informed_subsample_is_the_host_twin_and_the_subset_a_fresh_evaluator(monkeypatch):
    ps, trees, X, lab, hit = inputs()
    ev = make(monkeypatch, N_MAX, "device")
    try:
        got = ev.evaluate(trees)
        check_routes(ev, got)
        planes = raw_planes(ev, len(trees))
        random.seed(5)
        seed = random.Random(5).getrandbits(64)
        idx = ev.informed_subsample(32)
        exp_idx, exp_dist = _lib.host_informed_cases(planes, N_MAX, seed, 32)
        assert idx.tolist() == exp_idx.tolist() and len(set(idx.tolist())) == 32
        assert ev.last_informed_distances.tolist() == exp_dist.tolist()
        assert ev.n_cases == 32
        sub = ev.evaluate(trees)
        sub_mat = ev.last_case_hits()
        sub_hits = ev.last_hits.tolist()
    finally:
        ev.close()
    assert np.array_equal(sub_mat, hit[:, idx])
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    fresh = GPUEvaluator(ps, TypedCaseHits(X[:, idx], lab[idx], "device"), device=0)
    try:
        assert fresh.evaluate(trees) == sub
        assert np.array_equal(fresh.last_case_hits(), sub_mat)
        assert fresh.last_hits.tolist() == sub_hits
    finally:
        fresh.close()


# ------------------------------------------------------------- residency --
def test_subsample_and_a_reload_drop_or_refuse_the_planes(monkeypatch):
    ps, trees, X, lab, hit = inputs()
    ev = make(monkeypatch, 129, "device")
    try:
        ev.evaluate(trees)
        assert len(ev.select_lexicase(trees, 3)) == 3
        ev.subsample(np.arange(0, 129, 2))
        with pytest.raises(ValueError, match="left no per-case matrix on the GPU"):
            ev.select_lexicase(trees, 3)
        with pytest.raises(_lib.GpeError, match="no hit planes"):
            ev.ctx.hit_planes(len(trees))
        with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs"):
            ev.ctx.lexicase_bits(None, 0, 0, 1, random.Random(1))
        ev.evaluate(trees)
        assert np.array_equal(ev.last_case_hits(), hit[:, 0:129:2])
        assert len(ev.select_lexicase(trees, 3)) == 3
        # another batch is loaded (not run): the NULL routes refuse its count
        few = trees[:10]
        ev.prepare(ev.flatten(few), few)
        assert ev.ctx.n_prog == 10
        with pytest.raises(ValueError, match="now holds 10 programs"):
            ev.select_lexicase(trees, 3)
        for call in (lambda: ev.ctx.lexicase_bits(None, 0, 0, 1, random.Random(1)),
                     lambda: ev.ctx.lexicase_bits_par(None, 0, 0, 1, 9),
                     lambda: ev.ctx.informed_cases(None, 0, 0, 0.0, 9, 4)):
            with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs"):
                call()
    finally:
        ev.close()


# -------------------------------------------------------- unchanged path --
def test_the_count_only_run_is_the_same_before_and_after(monkeypatch):
    ps, trees, X, lab, hit = inputs()
    n_cases = 300
    plain = make(monkeypatch, n_cases, cls=TypedBoolHits)
    try:
        before = plain.evaluate(trees)
        ev = make(monkeypatch, n_cases, "device")
        try:
            assert ev.evaluate(trees) == before
        finally:
            ev.close()
        after = plain.evaluate(trees)
        again = make(monkeypatch, n_cases, cls=TypedBoolHits)
        try:
            fresh = again.evaluate(trees)
        finally:
            again.close()
    finally:
        plain.close()
    assert before == after == fresh == [(int(h),) for h in hit.sum(axis=1)]


def test_the_library_refuses_the_b_machine_fp32_and_two_columns(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    ctx = _lib.Context(0)
    try:
        ctx.set_bitplanes(np.zeros((2, 1), dtype=np.uint32), np.zeros(1, dtype=np.uint32), 20)
        with pytest.raises(_lib.GpeError, match="needs the F machine"):
            ctx.run_typed_hit_planes()
        rng = np.random.default_rng(1)
        ctx.set_cases(_lib.GPE_MACHINE_F, rng.random((2, 20)), rng.random((2, 20)))
        with pytest.raises(_lib.GpeError, match="exactly one target column"):
            ctx.run_typed_hit_planes()
        ctx.set_cases(_lib.GPE_MACHINE_F, rng.random((2, 20)), rng.random((1, 20)))
        ctx.set_precision(_lib.GPE_PREC_F32)
        with pytest.raises(_lib.GpeError, match="needs fp64"):
            ctx.run_typed_hit_planes()
    finally:
        ctx.close()
