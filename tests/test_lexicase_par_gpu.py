"""Parallel lexicase selection on the GPU: ``gpe_lexicase_par`` and
``gpe_lexicase_bits_par`` against the host twin (``gpe_host_lexicase_par``,
which the CPU suite checks against the rule's restatement) on host matrices
and on the resident matrices of the three per-case specs; the picks are equal
exactly."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import lexicase_par_ref as lr
import test_abs_error_cases_gpu as tg
from deap_amd import _lib, configs, datasets, gp, tools

pytestmark = pytest.mark.gpu
SEEDS = (0x1234567, (1 << 64) - 1)
MODES = {"plain": (0, 0.0), "epsilon": (1, 0.75), "automatic": (2, 0.0)}
_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same(ctx, values, maximise, k, seed, mode, eps):
    got, gf = ctx.lexicase_par(values, maximise, k, seed, mode, eps)
    ref, rf = _lib.host_lexicase_par(values, maximise, k, seed, mode, eps)
    assert got.shape == (k,) and gf == rf and (got == ref).all(), \
        (gf, rf, np.flatnonzero(got != ref)[:5], got[:8], ref[:8])
    return got, gf


# -------------------------------------------------------- host matrices --
@pytest.mark.parametrize("n, C", [(1, 5), (2, 1), (63, 2), (64, 33), (65, 257), (257, 3),
                                  (16385, 3)])
def test_host_matrices_against_the_twin(ctx, n, C):
    """W crosses one word per thread at 16,385 individuals, C the block width
    at 257 cases; ties, clones and nan / inf matrices, every mode, both seeds."""
    mats = lr.matrices(n, C)
    mixed = lr.maximise_settings(C)["mixed"]
    failures = 0
    for name in ("ties", "clones", "nan"):
        for mode, eps in MODES.values():
            for seed in SEEDS:
                got, failed = same(ctx, mats[name], mixed, 64, seed, mode, eps)
                failures += failed >= 0
                assert (failed >= 0) == bool((got < 0).any())
    same(ctx, mats["random"], np.zeros(C, dtype=np.uint8), 64, SEEDS[0], 2, 0.0)
    assert n == 1 or failures > 0


def test_candidate_sets_beyond_the_lds_capacity(ctx):
    """40,000 individuals on a 2-level alphabet: the second case's candidate
    set (about half of them) does not fit the compacted values' LDS and its
    medians run on the block's device scratch; more than 32,768 individuals
    put the candidate words there too.  The serial route refuses this shape."""
    n, C, k, seed = 40000, 3, 16, 7
    cap = _lib.lexicase_par_lds_values()
    values = np.random.default_rng(40).integers(0, 2, (n, C)).astype(np.float64)
    mx = np.zeros(C, dtype=np.uint8)
    # the candidates left by each selection's opening case: a 0/1 column's
    # MAD is 0 (or 0.5 on an exactly even one), so min + MAD keeps the zeros
    firsts = [min(range(C), key=lambda c: (lr.key(seed, s * (C + 1) + c), c)) for s in range(k)]
    largest = max(int((values[:, c] == 0).sum()) for c in set(firsts))
    assert largest > cap and largest < n
    same(ctx, values, mx, k, seed, 2, 0.0)
    with pytest.raises(_lib.GpeError, match="at most 16384 individuals"):
        ctx.lexicase(values, mx, 1, random.Random(1), 2)


def test_blocks_loop_over_several_selections(ctx):
    values = lr.matrices(65, 5)["ties"]
    for mode, eps in MODES.values():
        got, failed = same(ctx, values, lr.maximise_settings(5)["mixed"], 5000, SEEDS[1], mode,
                           eps)
        assert failed == -1 and len(set(got.tolist())) > 5


def test_failing_selections(ctx):
    values = lr.matrices(65, 5)["nan"]
    mx = np.zeros(5, dtype=np.uint8)
    for mode, eps in MODES.values():
        got, failed = same(ctx, values, mx, 300, 11, mode, eps)
        assert failed >= 0 and got[failed] == -1 and (got[:failed] >= 0).all()
        # (a nan anywhere in a column makes its median nan: nobody survives)
        assert (got >= 0).any() == (mode != 2)
    # no selection: nothing is written, nothing fails
    got, failed = ctx.lexicase_par(values, mx, 0, 11, 0)
    assert got.shape == (0,) and failed == -1


def test_argument_errors(ctx):
    v = np.zeros((3, 2))
    mx = np.zeros(2, dtype=np.uint8)
    with pytest.raises(_lib.GpeError, match=r"lexicase_par: k = -1 selections"):
        ctx.lexicase_par(v, mx, -1, 0)
    with pytest.raises(_lib.GpeError, match=r"lexicase_par: mode must be 0, 1 or 2"):
        ctx.lexicase_par(v, mx, 1, 0, mode=3)
    with pytest.raises(_lib.GpeError, match=r"lexicase_par: n = 0 individuals"):
        ctx.lexicase_par(np.zeros((0, 2)), mx, 1, 0)
    with pytest.raises(_lib.GpeError, match=r"lexicase_bits_par: n_cases = 0"):
        ctx.lexicase_bits_par(np.zeros((3, 0), dtype=np.uint32), 3, 0, 1, 0)
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.GpeError, match="no per-case values on the device"):
            fresh.lexicase_par(None, mx, 1, 0)
        with pytest.raises(_lib.GpeError, match="no hit planes"):
            fresh.lexicase_bits_par(None, 0, 0, 1, 0)
    finally:
        fresh.close()


# ------------------------------------------------------ resident doubles --
def regression_pop():
    """The abs-error tests' trees that neither raise nor leave a non-finite
    error on the first 257 cases, and their matrix from a cases="host"
    evaluation (computed once): of the last 400 seeded trees (the
    hand-written ones around them hold the target itself, which wins every
    case)."""
    if "reg" not in _CACHE:
        ps, trees, X, y = tg.cells()
        trees = trees[tg._CACHE["n_base"] - 400:tg._CACHE["n_base"]]
        ev = tg.evaluator(tg.N_SMALL, cases="host")
        try:
            res = ev.evaluate(trees)
        finally:
            ev.close()
        kept = [(t, r) for t, r in zip(trees, res)
                if not isinstance(r, BaseException) and np.isfinite(r).all()]
        assert len(kept) >= 200, len(kept)
        _CACHE["reg"] = ([gp.PrimitiveTree(t) for t, _ in kept],
                         np.array([r for _, r in kept], dtype=np.float64))
    return _CACHE["reg"]


@pytest.mark.parametrize("subset", [False, True])
def test_selection_from_the_resident_matrix(subset):
    pop, full = regression_pop()
    idx = np.random.default_rng(33).integers(0, tg.N_SMALL, 33) if subset else None
    matrix = full[:, idx] if subset else full
    C = matrix.shape[1]
    ev = tg.evaluator(tg.N_SMALL, cases="device")
    try:
        if subset:
            ev.subsample(idx)
        ev.evaluate(pop)
        mae, hits = ev.last_mae.copy(), ev.last_hits.copy()
        random.seed(5)
        random.getrandbits(64)
        after_one_draw = random.getstate()
        for mode, (m, eps) in MODES.items():
            random.seed(5)
            got = ev.select_lexicase(pop, 100, mode, eps, parallel=True)
            assert random.getstate() == after_one_draw
            ref, failed = _lib.host_lexicase_par(matrix, np.zeros(C, dtype=np.uint8), 100,
                                                 ev.last_lexicase_seed, m, eps)
            assert failed == -1 and [id(x) for x in got] == [id(pop[i]) for i in ref]
            print(mode, "distinct picks:", len(set(ref.tolist())))
            assert (ev.last_mae == mae).all() and (ev.last_hits == hits).all()
            # the matrix is where it was: the replaying route still selects
            random.seed(9)
            serial = ev.select_lexicase(pop, 5, mode, eps)
            random.seed(9)
            assert serial == ev.select_lexicase(pop, 5, mode, eps)
        state = random.getstate()
        assert ev.select_lexicase(pop, 0, "plain", parallel=True) == []
        assert random.getstate() == state
        with pytest.raises(ValueError, match="last evaluate / map"):
            ev.select_lexicase(pop[:4], 3, parallel=True)
        assert random.getstate() == state
    finally:
        ev.close()


def test_more_than_16384_individuals_in_automatic_mode():
    """One past the replaying kernel's automatic-epsilon limit, the shape
    ``test_select_lexicase_surfaces_the_librarys_limits`` builds."""
    ps, trees, X, y = tg.cells()
    many = [trees[20 + i % 100] for i in range(16385)]
    host = tg.evaluator(2, cases="host")
    try:
        matrix = np.array(host.evaluate(many[:100]), dtype=np.float64)
    finally:
        host.close()
    assert matrix.shape == (100, 2) and np.isfinite(matrix).all()
    matrix = matrix[np.arange(16385) % 100]
    ev = tg.evaluator(2, cases="device")
    try:
        ev.evaluate(many)
        random.seed(5)
        got = ev.select_lexicase(many, 40, "automatic", parallel=True)
        ref, failed = _lib.host_lexicase_par(matrix, np.zeros(2, dtype=np.uint8), 40,
                                             ev.last_lexicase_seed, 2)
        assert failed == -1 and [id(x) for x in got] == [id(many[i]) for i in ref]
        assert ref.max() > 8192
    finally:
        ev.close()


# --------------------------------------------------------- resident bits --
def mux6():
    """The 6-multiplexer (2 address lines, 4 data lines; 64 cases) over the
    6-input boolean primitive set: ``(pset, 128 seeded trees, ins, outs)``."""
    if "mux6" not in _CACHE:
        ps = configs.pset_for("parity6")
        ins = datasets.parity6_table()[0]
        sel = 2 + ins[0].astype(np.int64) + 2 * ins[1].astype(np.int64)
        outs = ins[sel, np.arange(64)]
        _CACHE["mux6"] = (ps, configs.population(ps, "half", 128, 21, 2, 6), ins,
                          outs.astype(np.uint8))
    return _CACHE["mux6"]


@pytest.mark.parametrize("n", [65, 16385])
@pytest.mark.parametrize("subset", [False, True])
def test_selection_from_the_resident_hit_planes(n, subset):
    from deap_amd.evaluator import BooleanCaseHits, GPUEvaluator
    ps, trees, ins, outs = mux6()
    pop = [gp.PrimitiveTree(trees[i % 128]) for i in range(n)]
    ev = GPUEvaluator(ps, BooleanCaseHits(ins, outs, "device"), device=0)
    try:
        if subset:
            ev.subsample(np.random.default_rng(6).integers(0, 64, 33))
        ev.evaluate(pop)
        hit = ev.last_case_hits().astype(np.float64)
        C = 33 if subset else 64
        assert hit.shape == (n, C)
        random.seed(5)
        random.getrandbits(64)
        after_one_draw = random.getstate()
        for mode, eps in (("plain", 0.0), ("epsilon", 0.5), ("automatic", 0.0)):
            random.seed(5)
            got = ev.select_lexicase(pop, 100, mode, eps, parallel=True)
            assert random.getstate() == after_one_draw
            ref, failed = _lib.host_lexicase_par(hit, np.ones(C, dtype=np.uint8), 100,
                                                 ev.last_lexicase_seed, 0)
            assert failed == -1 and [id(x) for x in got] == [id(pop[i]) for i in ref]
            print(mode, "distinct picks:", len(set(ref.tolist())))
        if n > 8192:
            assert ref.max() > 8192                         # (picks from the far words too)
        for eps in (1.0, -0.5):
            with pytest.raises(ValueError, match=r"epsilon must be in \[0, 1\)"):
                ev.select_lexicase(pop, 2, "epsilon", eps, parallel=True)
        # the planes are where they were: the replaying route still selects
        random.seed(9)
        serial = ev.select_lexicase(pop, 5)
        random.seed(9)
        assert serial == ev.select_lexicase(pop, 5)
    finally:
        ev.close()


def test_host_planes_against_the_twin(ctx):
    from deap_amd.evaluator import pack_bitplanes
    rng = np.random.default_rng(8)
    for n, C in ((1, 5), (65, 33), (300, 257)):
        hit = rng.integers(0, 2, (n, C)).astype(np.uint8)
        hit[n // 2:] = hit[:n - n // 2]                     # clone groups
        for seed in SEEDS:
            got, gf = ctx.lexicase_bits_par(pack_bitplanes(hit), n, C, 64, seed)
            ref, rf = _lib.host_lexicase_par(hit.astype(np.float64), np.ones(C, dtype=np.uint8),
                                             64, seed, 0)
            assert gf == rf == -1 and (got == ref).all()


# -------------------------------------------------------------- drop-ins --
def test_the_drop_ins_pick_what_select_lexicase_picks():
    pop, full = regression_pop()
    C = full.shape[1]
    w = (-1.0,) * C
    inds = [SimpleNamespace(fitness=SimpleNamespace(values=tuple(r), weights=w), idx=i)
            for i, r in enumerate(full.tolist())]
    ev = tg.evaluator(tg.N_SMALL, cases="device")
    try:
        ev.evaluate(pop)
        k, eps = 50, 0.75
        calls = {"plain": lambda: tools.selLexicaseGPU(inds, k, device=0, parallel=True),
                 "epsilon": lambda: tools.selEpsilonLexicaseGPU(inds, k, eps, device=0,
                                                                parallel=True),
                 "automatic": lambda: tools.selAutomaticEpsilonLexicaseGPU(inds, k, device=0,
                                                                           parallel=True)}
        for mode, call in calls.items():
            random.seed(5)
            drop = [x.idx for x in call()]
            state = random.getstate()
            random.seed(5)
            res = ev.select_lexicase(pop, k, mode, eps, parallel=True)
            where = {id(x): j for j, x in enumerate(pop)}
            assert drop == [where[id(x)] for x in res] and random.getstate() == state
    finally:
        ev.close()
