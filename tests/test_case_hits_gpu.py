"""``BooleanCaseHits`` on the GPU: the hit planes a hit-planes run stores against
the values run's planes XNOR the outputs at the case counts where the B
machine changes kernel or tile and the program counts where the transposition
has ragged groups; the counts against ``BooleanHits``; device lexicase on the
bit matrix against ``tools.selLexicase`` on the unpacked matrix (picks and
``random`` state) in all three modes, at the shapes the double kernel refuses,
and on the reference's recorded matrices; residency and the order of errors."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from deap_amd import _lib, configs, datasets, gp, tools
from test_case_hits import _bits, bit_lexicase, fixture_cases

pytestmark = pytest.mark.gpu

# (cases, programs): 1, 33, 512 run the lane-packed kernel, 513 is the first
# count past its 16 words; 2048 is one 64-word tile, 2049 a second, partial one,
# 4097 a partial third; the program counts are the transposition's 64-program
# groups: one program, one short of a group, a full one, one past, two and one
SHAPES = [(1, 129), (33, 63), (512, 64), (513, 65), (2048, 129), (2049, 1), (4097, 65)]
HAND = ["0", "and_(IN0, IN1)", "and_(IN0, and_(IN1, IN2))", "and_(IN2, IN3)", "xor(IN0, IN0)",
        "and_(IN4, or_(IN0, IN1))", "and_(xor(IN0, IN1), IN2)"]
_CACHE = {}


def mux():
    """``(pset, population of 129, inputs, outputs)``: a tree of 7 stack slots
    first (the deep kernel; every program count holds it), then seeded
    half-and-half trees, some of them deep as well."""
    if "mux" not in _CACHE:
        ps = configs.pset_for("mux11")
        deep = configs.population(ps, "full", 2, 3, 7, 7)[1:]
        pop = deep + configs.population(ps, "half", 128, 17, 2, 6)
        ins, outs = datasets.mux11_table()
        _CACHE["mux"] = (ps, pop, ins, outs)
    return _CACHE["mux"]


def make(kind, which="mux", cases="device"):
    from deap_amd.evaluator import BooleanCaseHits, BooleanHits, GPUEvaluator
    if which == "mux":
        ps, _, ins, outs = mux()
    else:
        ps = configs.pset_for("parity6")
        ins, outs = datasets.parity6_table()
    spec = BooleanHits(ins, outs) if kind == "plain" else BooleanCaseHits(ins, outs, cases)
    return GPUEvaluator(ps, spec, device=0)


@pytest.fixture(scope="module")
def evs():
    """One evaluator per (problem, spec kind), shared by the tests."""
    made = {}

    def get(kind, which="mux", cases="device"):
        key = (kind, which, cases)
        if key not in made:
            made[key] = make(kind, which, cases)
        return made[key]
    yield get
    for ev in made.values():
        ev.close()


def subset_idx(m):
    idx = np.random.default_rng(m).integers(0, 2048, m)
    idx[:min(m, 3)] = (2047, 0, 2047)[:min(m, 3)]          # the ends, a duplicate
    return idx


def namespace_pop(hit):
    w = (1.0,) * hit.shape[1]
    return [SimpleNamespace(fitness=SimpleNamespace(values=tuple(r), weights=w), idx=i)
            for i, r in enumerate(hit.astype(np.int64).tolist())]


def reference_picks(hit, k, seed):
    random.seed(seed)
    picks = [x.idx for x in tools.selLexicase(namespace_pop(hit), k)]
    return picks, random.getstate()


# ------------------------------------------------------------ hit planes --
@pytest.mark.parametrize("m, n", SHAPES)
def test_hit_planes_and_counts(evs, m, n):
    ps, pop, ins, outs = mux()
    pop = pop[:n]
    idx = subset_idx(m)
    host, dev, plain = evs("case", cases="host"), evs("case"), evs("plain")
    for ev in (host, dev, plain):
        ev.subsample(idx)
    assert host.flatten(pop).depth.max() > 6               # (the deep kernel runs too)
    fit = host.evaluate(pop)
    units = (m + 31) // 32
    # the values run's planes XNOR the gathered output plane
    vals = host.ctx.run_values_bits()
    assert vals.shape == (n, units)
    exp = _lib.host_hit_planes(vals, host.spec.out_plane, m)
    got = host.ctx.hit_planes(n)
    assert (got == exp).all(), np.argwhere(got != exp)[:5]
    if m % 32:
        assert (got[:, -1] >> np.uint32(m % 32) == 0).all()            # pad bits
    hit = host.last_case_hits()
    assert hit.dtype == bool and hit.shape == (n, m)
    from deap_amd.evaluator import unpack_bitplanes
    assert (hit == unpack_bitplanes(exp, m)).all()
    # the same thing from the data: predict against the gathered outputs
    assert (hit == (host.predict(pop) == outs[idx].astype(bool)[None, :])).all()
    if m >= 512 and n > 1:
        assert 0.2 < hit.mean() < 0.9 and len(np.unique(hit, axis=0)) > 1
    # cases="host": tuples of n_cases ints
    assert fit == [tuple(r) for r in hit.astype(np.int64).tolist()]
    assert all(type(v) is int for v in fit[0]) and len(fit[0]) == m
    # counts: BooleanHits on the same batch, bit for bit, from every spec
    want = plain.evaluate(pop)
    assert want == [(int(r.sum()),) for r in hit]
    assert dev.evaluate(pop) == want
    for ev in (host, dev):
        assert ev.last_hits.dtype == np.int64 and ev.last_hits.tolist() == [h for h, in want]
    assert (dev.last_case_hits() == hit).all()


# -------------------------------------------------------------- selection --
def parity_pop(n):
    ps = configs.pset_for("parity6")
    base = [gp.PrimitiveTree.from_string(s, ps) for s in HAND]
    order = np.random.default_rng(n).integers(0, len(base), n)
    return [gp.PrimitiveTree(base[i]) for i in order.tolist()]


@pytest.fixture(scope="module")
def duplicates(evs):
    """130 individuals that are copies of 7 trees (6 behaviours), none of which
    passes the all-zero case, evaluated once; their hit matrix."""
    ev = evs("case", "parity")
    pop = parity_pop(130)
    fit = ev.evaluate(pop)
    hit = ev.last_case_hits()
    assert hit.shape == (130, 64) and len(np.unique(hit, axis=0)) == 6
    assert (hit.sum(axis=0) == 0).any() and (hit.sum(axis=0) == 130).any()
    assert fit == [(int(r.sum()),) for r in hit]
    return ev, pop, hit


@pytest.mark.parametrize("mode, eps", [("plain", 0.0), ("automatic", 0.0), ("epsilon", 0.0),
                                       ("epsilon", 0.5)])
def test_selection_matches_the_reference_loop_in_every_mode(duplicates, mode, eps):
    ev, pop, hit = duplicates
    for k, seed in ((150, 21), (1, 22)):                   # (k > n; a single selection)
        exp, state = reference_picks(hit, k, seed)
        random.seed(seed)
        got = ev.select_lexicase(pop, k, mode, eps)
        assert [id(x) for x in got] == [id(pop[i]) for i in exp], (mode, k)
        assert random.getstate() == state, (mode, k)
    assert len(set(exp_i for exp_i in reference_picks(hit, 150, 21)[0])) > 20   # choice among many
    random.seed(23)
    state = random.getstate()
    assert ev.select_lexicase(pop, 0, mode, eps) == [] and random.getstate() == state


def test_one_individual_and_the_epsilon_refusal(evs):
    ev = evs("case", "parity")
    pop = parity_pop(130)[:1]
    ev.evaluate(pop)
    exp, state = reference_picks(ev.last_case_hits(), 5, 31)
    random.seed(31)
    assert ev.select_lexicase(pop, 5, "automatic") == [pop[i] for i in exp] == pop * 5
    assert random.getstate() == state
    for eps in (1.0, -0.5):
        with pytest.raises(ValueError, match=r"epsilon must be in \[0, 1\)"):
            ev.select_lexicase(pop, 2, "epsilon", eps)


def test_the_references_recorded_selections_through_a_host_matrix(evs):
    from deap_amd.evaluator import pack_bitplanes
    ctx = evs("case", "parity").ctx
    for c in fixture_cases():
        bits = _bits(c)
        rng = random.Random(c["seed"])
        idx, failed = ctx.lexicase_bits(pack_bitplanes(bits), len(bits), c["n_cases"], c["k"],
                                        rng)
        assert failed == -1 and idx.tolist() == c["selected"], c["name"]
        assert list(rng.getstate()[1]) == c["state"], c["name"]
    # nobody to choose from: the first selection fails, nothing is drawn
    rng = random.Random(1)
    before = rng.getstate()
    idx, failed = ctx.lexicase_bits(np.zeros((0, 1), dtype=np.uint32), 0, 5, 3, rng)
    assert failed == 0 and len(idx) == 0 and rng.getstate() == before


def test_16385_individuals_select_in_automatic_mode(evs):
    """One past the double kernel's automatic-epsilon limit (which its own
    tests pin): no values are held per candidate here."""
    ev = evs("case", "parity")
    pop = parity_pop(16385)
    fit = ev.evaluate(pop)
    hit = ev.last_case_hits()
    assert hit.shape == (16385, 64) and fit[16384] == (int(hit[16384].sum()),)
    ref = random.Random(41)
    exp = bit_lexicase(hit.astype(np.uint8), 12, ref)
    random.seed(41)
    got = ev.select_lexicase(pop, 12, "automatic")
    assert [id(x) for x in got] == [id(pop[i]) for i in exp]
    assert random.getstate() == ref.getstate()
    assert max(exp) > 8192                                  # (picks from the far words too)


def test_12289_cases_take_the_device_scratch(evs):
    """5 programs on 12,289 cases: ceil(5 / 32) + 12289 words are 8 bytes past
    48 KiB, so candidates and permutation live in device memory."""
    ps, pop, ins, outs = mux()
    pop = pop[10:15]                                       # (five behaviours)
    ev = evs("case")
    idx = np.random.default_rng(12289).integers(0, 2048, 12289)
    ev.subsample(idx)
    try:
        ev.evaluate(pop)
        hit = ev.last_case_hits()
        assert hit.shape == (5, 12289) and len(np.unique(hit, axis=0)) == 5
        exp, state = reference_picks(hit, 6, 51)
        random.seed(51)
        got = ev.select_lexicase(pop, 6, "plain")
        assert [id(x) for x in got] == [id(pop[i]) for i in exp]
        assert random.getstate() == state
    finally:
        ev.subsample(None)


# ---------------------------------------------------- residency and order --
def test_other_runs_leave_the_matrix_and_other_batches_do_not(evs, duplicates):
    ev, pop, hit = duplicates
    ev.evaluate(pop)
    exp, state = reference_picks(hit, 40, 61)
    # a values run, a plain hits run and a reload of the same programs in between
    assert (ev.predict(pop) == ev.predict(pop)).all()
    hi = ev.ctx.run(_lib.GPE_MODE_HITS_BITS)[0]
    assert hi.tolist() == hit.sum(axis=1).tolist()
    random.seed(61)
    assert [id(x) for x in ev.select_lexicase(pop, 40)] == [id(pop[i]) for i in exp]
    assert random.getstate() == state
    assert (ev.last_case_hits() == hit).all()
    # the resident fitness is a BooleanHits run's
    plain = evs("plain", "parity")
    plain.evaluate(pop)
    ev.evaluate(pop)
    r1, r2 = random.Random(5), random.Random(5)
    a = ev.ctx.tournament(None, 200, 3, r1)
    b = plain.ctx.tournament(None, 200, 3, r2)
    assert a.tolist() == b.tolist() and r1.getstate() == r2.getstate()
    # another batch, other objects, another program count
    msg = "must be the batch of this evaluator's last evaluate / map"
    with pytest.raises(ValueError, match=msg):
        ev.select_lexicase(parity_pop(130), 3)
    with pytest.raises(ValueError, match=msg):
        ev.select_lexicase(pop[:-1], 3)
    ev.predict(pop[:10])
    with pytest.raises(ValueError, match="now holds 10 programs, not the 130"):
        ev.select_lexicase(pop, 3)
    # a subsample drops the matrix, in the evaluator and in the library
    ev.evaluate(pop)
    ev.subsample(np.arange(10))
    try:
        with pytest.raises(ValueError, match="last evaluate / map left no per-case matrix"):
            ev.select_lexicase(pop, 3)
        with pytest.raises(_lib.GpeError, match="no hit planes of the loaded programs"):
            ev.ctx.lexicase_bits(None, 0, 0, 3, random.Random(1))
        ev.evaluate(pop)
        assert ev.last_case_hits().shape == (130, 10)
        assert (ev.last_case_hits() == hit[:, :10]).all()
        assert len(ev.select_lexicase(pop, 3)) == 3
    finally:
        ev.subsample(None)


def test_a_too_tall_tree_raises_from_select_lexicase_first(evs):
    ev = evs("case", "parity")
    ps = configs.pset_for("parity6")
    pop = parity_pop(6)
    pop[2] = gp.PrimitiveTree([ps.mapping["not_"]] * 201 + [ps.mapping["IN0"]])
    fit = ev.evaluate(pop)
    assert isinstance(fit[2], SyntaxError) and type(fit[1]) is tuple
    state = random.getstate()
    with pytest.raises(SyntaxError, match="too many nested parentheses"):
        ev.select_lexicase(pop, 2)
    assert random.getstate() == state


def test_the_f_machine_is_refused_by_the_library():
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    ev = GPUEvaluator(configs.pset_for("symbreg"), SymbRegMSE.quartic(), device=0)
    try:
        pop = configs.population(configs.pset_for("symbreg"), "half", 4, 7, 1, 3)
        ev.evaluate(pop)
        rc = ev.ctx.lib.gpe_run_hit_planes(ev.ctx.h, None, None, None, None)
        assert rc == _lib.GPE_E_ARG
        assert b"needs the B machine" in ev.ctx.lib.gpe_last_error(ev.ctx.h)
    finally:
        ev.close()
