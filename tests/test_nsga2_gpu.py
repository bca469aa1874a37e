"""NSGA-II on the GPU: ``gpe_nd_sort`` against its host twin (identical
fronts and order required) at the shapes where the kernels can go wrong, the
reference's recorded results through ``tools.sortNondominatedGPU`` /
``selNSGA2GPU``, what the call must leave alone, and a seeded evolution with
the size objective selected on the GPU against the same run selected by the
host mirror.

The register kernels own 256 rows a block and stream tiles of 256 candidates
(m = 2, 3, 4); the generic kernels 128 rows and tiles of 64 (m = 5 .. 32);
m = 1 is one radix sort.  n = 63 .. 65 and 255 .. 257 straddle the wave, the
tiles and the blocks, 1,025 leaves one row in the fifth block."""
import math
import operator
import random

import numpy as np
import pytest

import nsga2_cases as nc
from deap_amd import _lib, algorithms, base, configs, creator, datasets, gp, tools
from deap_amd.evaluator import GPUEvaluator, SymbRegCaseAbsErrors, SymbRegMSE, gpu_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def both(ctx, w, k, mult=None, ffo=False):
    """The device's fronts, required identical to the host twin's."""
    dev = nc.fronts_as_lists(ctx.nd_sort(w, k, mult, first_front_only=ffo))
    host = nc.fronts_as_lists(_lib.host_nd_sort(w, k, mult, first_front_only=ffo))
    assert dev == host
    assert ctx.nd_sort_fronts() == len(dev) and ctx.nd_sort_ms() >= 0.0
    return dev


def distinct_grid(rng, n, m, levels=8):
    """n distinct rows on a grid (ties in every objective), one objective of
    each row nudged by a distinct amount below the grid step.  With many
    objectives independent values would leave every row non-dominated, so
    past m = 3 a row is a common level plus half steps per objective."""
    if m > 3:
        w = rng.integers(0, levels, size=(n, 1)) + rng.integers(0, 3, size=(n, m)) / 2.0
    else:
        w = rng.integers(0, levels, size=(n, m)).astype(np.float64)
    w[np.arange(n), np.arange(n) % m] += (np.arange(n) + 1.0) / (4.0 * n)
    return w


# ------------------------------------------------------------- golden --
@pytest.mark.parametrize("name", nc.case_names())
def test_gpu_selection_equals_the_reference(name):
    case = nc.case_by_name(name)
    k = case["k"]
    pop = nc.case_population(case)
    random.seed(case["seed"])
    state = random.getstate()
    assert nc.idx_fronts(tools.sortNondominatedGPU(pop, k, device=0)) == case["fronts"]
    assert nc.idx_fronts(tools.sortNondominatedGPU(pop, k, first_front_only=True,
                                                   device=0)) == case["first_front"]
    assert all(not hasattr(ind.fitness, "crowding_dist") for ind in pop)
    chosen = tools.selNSGA2GPU(pop, k, device=0)
    assert [ind.idx for ind in chosen] == case["selected"]
    assert all(a is pop[a.idx] for a in chosen)               # identities
    assert nc.crowding_hex(pop) == case["crowding"]
    assert random.getstate() == state                          # nothing drawn
    assert random.getrandbits(32) == case["canary"]


# ------------------------------------------------- device == host twin --
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 32])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_device_equals_host_twin_at_ragged_shapes(ctx, n, m):
    rng = np.random.default_rng(n * 131 + m)
    w = distinct_grid(rng, n, m)
    assert len({tuple(r) for r in w.tolist()}) == n
    mult = rng.integers(1, 4, size=n).astype(np.int32)
    total = int(mult.sum())
    full = both(ctx, w, total, mult)
    assert sorted(r for f in full for r in f) == list(range(n))
    both(ctx, w, max(1, (3 * total) // 5), mult)
    both(ctx, w, max(1, n // 2))
    assert both(ctx, w, total, mult, ffo=True) == full[:1]


@pytest.mark.parametrize("n", [257, 1025])
def test_mutually_non_dominated_rows_are_one_front(ctx, n):
    x = np.arange(n, dtype=np.float64)
    w = np.stack([x, -x], axis=1)
    assert both(ctx, w, n) == [list(range(n))]
    assert both(ctx, w, 3) == [list(range(n))]


@pytest.mark.parametrize("m", [2, 5])
def test_a_peel_scans_a_front_of_several_tiles(ctx, m):
    """Two fronts of 700 rows, shuffled: row (x - 0.5, -x - 0.5) is dominated
    by (x, -x) alone, so the second front's order follows the first's
    positions across three tiles of 256 (eleven of 64)."""
    x = np.arange(700, dtype=np.float64)
    w = np.zeros((1400, m))
    w[:700, 0], w[:700, 1] = x, -x
    w[700:, 0], w[700:, 1] = x - 0.5, -x - 0.5
    perm = np.random.default_rng(6).permutation(1400)
    w = w[perm]
    fronts = both(ctx, w, 1400)
    first = [i for i in range(1400) if perm[i] < 700]
    assert fronts[0] == first and len(fronts) == 2
    below = {int(perm[i]) - 700: i for i in range(1400) if perm[i] >= 700}
    assert fronts[1] == [below[int(perm[i])] for i in first]
    assert both(ctx, w, 701) == fronts and both(ctx, w, 700) == fronts[:1]


def test_a_total_chain_is_300_fronts_of_one_row(ctx):
    x = np.random.default_rng(4).permutation(300).astype(np.float64)
    w = np.stack([x, 2.0 * x], axis=1)
    fronts = both(ctx, w, 300)
    assert fronts == [[i] for i in np.argsort(-x).tolist()]
    assert len(both(ctx, w, 17)) == 17
    # m = 1: the same chain from one sort
    assert both(ctx, x[:, None], 300) == fronts


@pytest.mark.parametrize("m", [1, 2, 5])
def test_equal_rows_share_one_front(ctx, m):
    assert both(ctx, np.full((130, m), 2.5), 130) == [list(range(130))]
    assert both(ctx, np.full((130, m), 2.5), 1, np.full(130, 3)) == [list(range(130))]


def test_duplicates_through_mult_count_as_individuals(ctx):
    rng = np.random.default_rng(12)
    w = distinct_grid(rng, 200, 2, levels=5)
    plain = both(ctx, w, 200)
    assert len(plain) > 3
    mult = np.ones(200, dtype=np.int32)
    mult[plain[0]] = 40                       # front 0 alone covers k
    assert both(ctx, w, 40 * len(plain[0]), mult) == plain[:1]
    assert both(ctx, w, 40 * len(plain[0]) + 1, mult) == plain[:2]


@pytest.mark.parametrize("m", [2, 5])
def test_k_at_a_front_boundary_one_below_and_one_above(ctx, m):
    rng = np.random.default_rng(77 + m)
    w = distinct_grid(rng, 300, m, levels=6 if m == 2 else 3)
    full = both(ctx, w, 300)
    assert len(full) >= 3
    ends = np.cumsum([len(f) for f in full]).tolist()

    def prefix(k):          # the fronts up to the one that covers k rows
        return full[:next(r for r, e in enumerate(ends) if e >= k) + 1] if k else []

    for r in (0, 1, len(full) - 2):
        assert both(ctx, w, ends[r]) == full[:r + 1]
        assert both(ctx, w, ends[r] - 1) == prefix(ends[r] - 1)
        assert both(ctx, w, ends[r] + 1) == full[:r + 2]
    assert both(ctx, w, 1) == full[:1]
    assert both(ctx, w, 10 ** 6) == full                      # k > n: all
    assert both(ctx, w, 300, ffo=True) == full[:1]


def test_infinities_and_signed_zeros_compare_as_ieee(ctx):
    inf = float("inf")
    w = np.asarray([[inf, 0.0], [1.0, inf], [inf, inf], [-inf, 5.0], [-inf, -inf],
                    [1.0, 1.0], [inf, -inf]])
    # (front 2: row 6 leaves with row 0 at position 0, rows 3 and 5 with row 1)
    assert both(ctx, w, 7) == [[2], [0, 1], [6, 3, 5], [4]]
    z = np.asarray([[0.0, -0.0], [-0.0, 0.0], [0.0, 0.0], [-1.0, -0.0]])
    assert both(ctx, z, 4) == [[0, 1, 2], [3]]
    assert both(ctx, np.asarray([[-0.0], [0.0], [-1.0], [0.0]]), 4) == [[0, 1, 3], [2]]
    rng = np.random.default_rng(8)
    w = rng.integers(0, 5, size=(260, 3)).astype(np.float64)
    w[rng.integers(0, 260, 30), rng.integers(0, 3, 30)] = inf
    w[rng.integers(0, 260, 30), rng.integers(0, 3, 30)] = -inf
    both(ctx, w, 260)


def test_nan_raises_and_k_zero_gives_nothing(ctx):
    w = np.zeros((70, 2))
    assert ctx.nd_sort(w, 0) == [] and ctx.nd_sort_fronts() == 0
    w[69, 1] = np.nan
    with pytest.raises(ValueError, match="nan at row 69, objective 1"):
        ctx.nd_sort(w, 5)
    with pytest.raises(ValueError, match="objectives"):
        ctx.nd_sort(np.zeros((3, 33)), 3)
    with pytest.raises(ValueError, match="mult"):
        ctx.nd_sort(np.zeros((3, 2)), 3, [1, 0, 2])
    pop = nc.population([[1.0, 2.0], [float("nan"), 1.0], [0.5, 3.0]], [-1.0, -1.0])
    for fn in (tools.sortNondominatedGPU, tools.selNSGA2GPU):
        with pytest.raises(ValueError):
            fn(pop, 2, device=0)
        assert fn(pop, 0, device=0) == []
    # the context still works after a refusal
    assert both(ctx, np.asarray([[1.0, 2.0], [2.0, 1.0], [0.0, 0.0]]), 3) == [[0, 1], [2]]


def test_a_repeated_call_gives_the_identical_result(ctx):
    rng = np.random.default_rng(31)
    w = distinct_grid(rng, 1500, 2, levels=40)
    first = both(ctx, w, 900)
    small = both(ctx, w[:100], 100)                # smaller, then larger again
    assert both(ctx, w, 900) == first and both(ctx, w[:100], 100) == small


# ------------------------------------------------- nothing resident moves --
def test_nothing_resident_is_disturbed():
    pset = configs.pset_for("symbreg")
    X, T = datasets.symbreg_points()
    random.seed(5)
    trees = configs.population(pset, "half", 120, 5, 1, 4)
    ev = GPUEvaluator(pset, SymbRegCaseAbsErrors(X, T, cases="device"), device=0)
    try:
        fit = ev.evaluate(trees)

        def lexicase():
            random.seed(8)
            return [id(t) for t in ev.select_lexicase(trees, 30, "epsilon", 0.5, parallel=True)]

        before = lexicase()
        rng = np.random.default_rng(3)
        w = distinct_grid(rng, 700, 3)
        # on the evaluator's own context, and through tools on the same device
        assert nc.fronts_as_lists(ev.ctx.nd_sort(w, 400)) == \
            nc.fronts_as_lists(_lib.host_nd_sort(w, 400))
        pop = nc.population(w[:, :2], [-1.0, 1.0])
        assert [i.idx for i in tools.selNSGA2GPU(pop, 300, device=0)] == \
            [i.idx for i in tools.selNSGA2(nc.population(w[:, :2], [-1.0, 1.0]), 300)]
        assert lexicase() == before and repr(ev.evaluate(trees)) == repr(fit)
        assert lexicase() == before
    finally:
        ev.close()


# ----------------------------------------------------------- end to end --
def _toolbox(tag, select):
    pset = configs.pset_for("symbreg")
    if not hasattr(creator, "FitnessMulti" + tag):
        creator.create("FitnessMulti" + tag, base.Fitness, weights=(-1.0, -1.0))
        creator.create("Individual" + tag, gp.PrimitiveTree,
                       fitness=getattr(creator, "FitnessMulti" + tag))
    tb = base.Toolbox()
    tb.register("expr", gp.genHalfAndHalf, pset=pset, min_=1, max_=2)
    tb.register("individual", tools.initIterate, getattr(creator, "Individual" + tag), tb.expr)
    tb.register("population", tools.initRepeat, list, tb.individual)
    ev = GPUEvaluator(pset, SymbRegMSE.quartic(), device=0, size_objective=True)
    tb.register("evaluate", ev)
    tb.register("map", gpu_map)
    tb.register("select", select)
    tb.register("mate", gp.cxOnePoint)
    tb.register("expr_mut", gp.genFull, min_=0, max_=2)
    tb.register("mutate", gp.mutUniform, expr=tb.expr_mut, pset=pset)
    for op in ("mate", "mutate"):
        tb.decorate(op, gp.staticLimit(key=operator.attrgetter("height"), max_value=17))
    return tb, ev


def test_evolution_with_the_size_objective_selects_as_the_host_mirror():
    runs = []
    for tag, select in (("NsgaGpu", tools.selNSGA2GPU), ("NsgaHost", tools.selNSGA2)):
        tb, ev = _toolbox(tag, select)
        try:
            random.seed(23)
            pop = tb.population(n=64)
            st = tools.Statistics(lambda ind: ind.fitness.values)
            st.register("min", lambda v: np.min(v, axis=0).tolist())
            st.register("avg", lambda v: np.mean(v, axis=0).tolist())
            pop, log = algorithms.eaMuPlusLambda(pop, tb, 64, 64, 0.5, 0.2, 5, stats=st,
                                                 verbose=False)
        finally:
            ev.close()
        for ind in pop:
            assert len(ind.fitness.values) == 2 and ind.fitness.values[1] == len(ind)
            assert not math.isnan(ind.fitness.values[0])
        runs.append(([dict(rec) for rec in log], [str(ind) for ind in pop],
                     [ind.fitness.values for ind in pop]))
    assert runs[0] == runs[1]
    assert len(runs[0][0]) == 6 and len(runs[0][1]) == 64
