"""Case subsampling on the GPU: after ``GPUEvaluator.subsample(idx)`` every
result is what a fresh evaluator built on ``X[:, idx]``, ``terms[:, idx]``
gives, bit for bit — for every F spec at the edges of the 128-case tile,
against ``gp.compile`` directly, in fp32, on the typed and the boolean
machine; the programs stay resident across subsets and nothing of a previous
subset survives; selection from the gathered set; the C ABI."""
import ctypes
import random
import warnings

import numpy as np
import pytest

import abs_error_ref as ar
import predict_ref as pr
import scaled_ref as sr
from deap_amd import _lib, base, configs, creator, datasets, gp, tools

pytestmark = pytest.mark.gpu
ALL3 = ("mae", "max", "hits")
MS = (1, 2, 127, 128, 129, 257, 1000)
N = sr.N_MAX
INF_ROW = sr.INF_CASE
SHAPES = ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep", "moments", "moments_deep",
          "abserr", "abserr_deep")
# sin(ARG9) raises only at the inf row, sqrt(ARG0) only where ARG0 < 0
EXTRA = ["sin(ARG9)", "sqrt(ARG0)"]
# an exact-int program whose int outgrows the device's 1088 bits and cancels
# back: ARG1 * ((2**30 + 1)**64 - ((2**30 + 1)**64 - (2**30 + 1))), evaluated
# by the host pass on the cases it copies back from the device
_P64 = sr._chain(sr.A, 6)
HUGE = "mul(ARG1, sub(%s, sub(%s, %s)))" % (_P64, _P64, sr.A)
_CACHE = {}


def cells():
    """``(pset, trees, X, y)``, once: abs_error_ref's population with EXTRA
    appended, scaled_ref's data at its full 10,243 cases."""
    if "cells" not in _CACHE:
        ps, trees, _ = ar.population()
        trees = trees + [gp.PrimitiveTree.from_string(s, ps) for s in EXTRA]
        X, y = sr.data()
        assert X.shape == (10, N) and np.isinf(X[9, INF_ROW]) and (X[6, sr.NEG_FROM:] < 0).all()
        _CACHE["cells"] = (ps, trees, X, y)
    return _CACHE["cells"]


def make_spec(name, X, y, cases="host"):
    from deap_amd import evaluator as E
    X, y = np.ascontiguousarray(X), np.ascontiguousarray(y)
    return {"mse": lambda: E.SymbRegMSE(X, y),
            "numpy_sse": lambda: E.SymbRegNumpySSE(X, y),
            "sum_sse": lambda: E.SymbRegSumSSE(X, y),
            "scaled": lambda: E.SymbRegScaledMSE(X, y),
            "abs_error": lambda: E.SymbRegAbsError(X, y, hit_eps=ar.HIT_EPS, fitness=ALL3),
            "case_abs_errors": lambda: E.SymbRegCaseAbsErrors(
                X, y, hit_eps=ar.HIT_EPS, cases=cases, fitness=ALL3),
            "case_errors": lambda: E.SymbRegCaseErrors(X, y)}[name]()


F_SPECS = ("mse", "numpy_sse", "sum_sse", "scaled", "abs_error", "case_abs_errors",
           "case_errors")


def make_ev(name, X, y, ps=None, **kw):
    from deap_amd.evaluator import GPUEvaluator
    cases = kw.pop("cases", "host")
    return GPUEvaluator(ps or cells()[0], make_spec(name, X, y, cases), device=0, **kw)


@pytest.fixture(scope="module")
def full_ev():
    """One evaluator per spec holding the full 10,243 cases, shared by the
    subset sizes (and so run on one subset after another)."""
    made = {}

    def get(name):
        if name not in made:
            ps, trees, X, y = cells()
            made[name] = make_ev(name, X, y)
        return made[name]
    yield get
    for ev in made.values():
        ev.close()


def subset_idx(m, seed=0):
    """A seeded draw of m cases, forced to hold case 0 and the inf row, a
    duplicate and a descending pair as far as m has room for them (m = 1: the
    inf row alone; m = 2: the inf row, then case 0)."""
    idx = np.random.default_rng(1000 * seed + m).integers(0, N, m)
    if m == 1:
        idx[:] = INF_ROW
    elif m < 5:
        idx[:2] = (INF_ROW, 0)
    else:
        idx[:5] = (7, 7, INF_ROW, 0, 5000)
    return idx


def assert_same_results(got, exp, what):
    """Fitness tuples by bits, exceptions by type and args."""
    assert len(got) == len(exp), what
    rows_g, rows_e = [], []
    for i, (a, b) in enumerate(zip(got, exp)):
        if isinstance(a, BaseException) or isinstance(b, BaseException):
            assert type(a) is type(b) and a.args == b.args, (what, i, a, b)
            continue
        assert type(a) is tuple and type(b) is tuple and len(a) == len(b), (what, i)
        k = min(len(a), 4)
        assert [type(v) for v in a[:k]] == [type(v) for v in b[:k]], (what, i, a[:k], b[:k])
        rows_g.append(a)
        rows_e.append(b)
    if rows_g:
        pr.assert_same_bits(np.array(rows_g, dtype=np.float64),
                            np.array(rows_e, dtype=np.float64), what)
    return len(rows_g)


def snapshot(ev, pop, name):
    """One evaluation of *pop* and everything the contract names."""
    out = {"res": ev.evaluate(pop)}
    out["shapes"] = {k: ev.ctx.launch_shape(k)["programs"] for k in SHAPES}
    out["last"] = [np.array(a).copy() for a in
                   (ev.last_scaling[0], ev.last_scaling[1], ev.last_mae, ev.last_max_error,
                    ev.last_hits)]
    out["vals"], out["err"] = ev.ctx.run_values()          # what predict() returns, all rows
    if name != "numpy_sse":
        out["predict"] = ev.predict(pop[:24], errors="nan")
        out["first"] = ev.last_predict_first_error.copy()
    return out


def assert_same_snapshot(got, exp, what):
    n_values = assert_same_results(got["res"], exp["res"], what)
    for a, b in zip(got["last"], exp["last"]):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        if a.dtype.kind == "f":
            pr.assert_same_bits(a, b, what + " last_*")
        else:
            assert np.array_equal(a, b), what
    pr.assert_same_bits(got["vals"], exp["vals"], what + " values")
    assert np.array_equal(got["err"], exp["err"]), what + " error words"
    if "predict" in exp:
        pr.assert_same_bits(got["predict"], exp["predict"], what + " predict")
        assert np.array_equal(got["first"], exp["first"]), what
    return n_values


def assert_every_route_ran(shapes, name, what):
    """The exact D = 5, the exact deep and the C++ launches each held a
    program (the moments / abs-error specs: their kernels' two launches and
    the rows route)."""
    rows = sum(shapes[k] for k in ("asm_fast", "asm_deep", "cpp_fast", "cpp_deep"))
    if name == "scaled":
        assert shapes["moments"] > 0 and shapes["moments_deep"] > 0 and rows > 0, (what, shapes)
    elif name in ("abs_error", "case_abs_errors"):
        assert shapes["abserr"] > 0 and shapes["abserr_deep"] > 0 and rows > 0, (what, shapes)
    else:
        assert shapes["asm_fast"] > 0 and shapes["asm_deep"] > 0 and \
            shapes["cpp_fast"] + shapes["cpp_deep"] > 0, (what, shapes)


# ------------------------------------- 1. equivalence with a fresh evaluator --
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", F_SPECS)
def test_subset_equals_a_fresh_evaluator(full_ev, name, m):
    ps, trees, X, y = cells()
    idx = subset_idx(m)
    assert INF_ROW in idx and (m == 1 or 0 in idx)
    assert m < 5 or (len(set(idx.tolist())) < m and (np.diff(idx) < 0).any())
    ev = full_ev(name)
    ev.subsample(idx)
    assert ev.n_cases == m and ev.full_n_cases == N and ev.case_uploads == 1
    assert ev.case_subset.dtype == np.int64 and np.array_equal(ev.case_subset, idx)
    assert ev.ctx.case_subset() == (m, N, True)
    what = "%s, m = %d" % (name, m)
    got = snapshot(ev, trees, name)
    assert got["vals"].shape == (len(trees), m)
    fresh = make_ev(name, X[:, idx], y[idx])
    try:
        exp = snapshot(fresh, trees, name)
    finally:
        fresh.close()
    n_values = assert_same_snapshot(got, exp, what)
    # (every subset holds the inf row, where each tree that takes sin / cos of
    # something built on ARG9 raises: 4 in 10 of the seeded trees; the rest
    # keeps the comparison of values from being vacuous)
    assert n_values > len(trees) // 2, (what, n_values)
    assert_every_route_ran(got["shapes"], name, what)
    assert ev.case_uploads == 1


def test_errors_follow_the_rows_of_the_subset(full_ev):
    """sin(ARG9) raises only at the inf row and sqrt(ARG0) only where ARG0 is
    negative: a subset without such rows raises for neither, and one with the
    row at position p reports case p."""
    ps, trees, X, y = cells()
    pop = trees[-2:] + [trees[1]]
    assert [str(t) for t in pop[:2]] == EXTRA
    ok = np.flatnonzero((X[0] >= 0) & (np.arange(N) != INF_ROW))
    neg = np.flatnonzero(X[0] < 0)
    clean = np.random.default_rng(4).permutation(ok)[:130]
    ev = full_ev("mse")
    ev.subsample(clean)
    res = ev.evaluate(pop)
    assert all(type(r) is tuple for r in res), res
    ev.predict(pop)                                       # raises nothing
    assert ev.last_predict_first_error.tolist() == [-1, -1, -1]
    p, q = 77, 50                      # (q < p: ARG0 may be negative at the inf row too)
    dirty = clean.copy()
    dirty[p], dirty[q] = INF_ROW, neg[3]
    ev.subsample(dirty)
    res = ev.evaluate(pop)
    assert type(res[0]) is ValueError and type(res[1]) is ValueError and type(res[2]) is tuple
    ev.predict(pop, errors="nan")
    assert ev.last_predict_first_error.tolist() == [p, q, -1]
    with pytest.raises(ValueError) as info:
        ev.predict(pop)
    assert "individual 0, case %d:" % p in str(info.value)
    assert ev.case_subset[p] == INF_ROW and ev.case_subset[q] == neg[3]
    with pytest.raises(ValueError) as info:
        ev.predict(pop[1:])
    assert "individual 0, case %d:" % q in str(info.value)


# -------------------------------------------- 2. against gp.compile directly --
@pytest.mark.parametrize("m", [1, 129])
def test_per_case_errors_against_the_reference(full_ev, m):
    ps, trees, X, y = cells()
    idx = subset_idx(m, seed=2)
    pick = sorted(set(range(len(sr.HAND))) | set(range(len(trees) - 8, len(trees))) |
                  set(range(16, len(trees), 40)))
    pick = [i for i in pick if len(trees[i]) < 3000][:64]
    assert len(pick) >= 48
    pop = [trees[i] for i in pick]
    rows = list(zip(*X[:, idx].tolist()))
    ev = full_ev("case_abs_errors")
    ev.subsample(idx)
    res = ev.evaluate(pop)
    raised = values = 0
    for i, tree, r in zip(pick, pop, res):
        f, first, kind = sr.outputs(ps, tree, rows)
        w = (m, i, str(tree)[:80])
        if first is not None:
            assert type(r).__name__ == kind, (w, r)
            raised += 1
            continue
        e = np.array([abs(a - b) for a, b in zip(f.tolist(), y[idx].tolist())])
        if isinstance(r, BaseException):              # fsum's overflow: finite rows
            assert type(r) is OverflowError and "fsum" in str(r) and np.isfinite(e).all(), w
            continue
        assert type(r) is tuple and len(r) == m
        pr.assert_same_bits(np.array(r), e, repr(w))
        values += 1
    assert raised >= 3 and values >= 30, (raised, values)


# ------------------------------------------------------- 3. other machines --
def test_fp32_subset_equals_a_fresh_fp32_evaluator():
    ps, trees, X, y = cells()
    pop = trees[:400] + trees[-2:]
    idx = subset_idx(129, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # (no exact-int pass in fp32)
        ev = make_ev("mse", X, y, precision="fp32")
        fresh = make_ev("mse", X[:, idx], y[idx], precision="fp32")
        try:
            full = ev.evaluate(pop)
            ev.subsample(idx)
            got = snapshot(ev, pop, "mse")
            exp = snapshot(fresh, pop, "mse")
            assert assert_same_snapshot(got, exp, "fp32") > len(pop) // 2
            ev.subsample(None)
            assert_same_results(ev.evaluate(pop), full, "fp32, the full set again")
        finally:
            ev.close()
            fresh.close()


def test_typed_bool_hits_recounts_the_labels():
    from deap_amd.evaluator import GPUEvaluator, TypedBoolHits
    ps = configs.pset_for("spambase")
    pop = configs.population(ps, "half", 300, 7, 1, 2)
    X, lab = datasets.spambase_like(1000, 1234)
    lab = np.asarray(lab)
    ones, zeros = np.flatnonzero(lab != 0), np.flatnonzero(lab == 0)
    idx = np.random.default_rng(5).permutation(np.concatenate([ones[:100], zeros[:29], ones[:3]]))
    assert abs((lab[idx] != 0).mean() - (lab != 0).mean()) > 0.1
    ev = GPUEvaluator(ps, TypedBoolHits(X, lab), device=0)
    fresh = GPUEvaluator(ps, TypedBoolHits(np.ascontiguousarray(X[:, idx]), lab[idx]), device=0)
    try:
        full = ev.evaluate(pop)
        assert ev.ctx.geometry()["typed_const"] > 0
        ev.subsample(idx)
        got = ev.evaluate(pop)
        assert ev.ctx.geometry()["typed_const"] > 0          # constant programs: label_true
        exp = fresh.evaluate(pop)
        assert got == exp and all(type(r) is tuple and type(r[0]) is int for r in got)
        assert got != full
        ev.subsample(None)
        assert ev.evaluate(pop) == full and ev.case_uploads == 1
    finally:
        ev.close()
        fresh.close()


@pytest.mark.parametrize("m", [1, 31, 32, 33, 64])
def test_boolean_hits_subset(m):
    from deap_amd.evaluator import BooleanHits, GPUEvaluator
    ins, outs = (np.ascontiguousarray(a) for a in datasets.parity6_table())
    ps = configs.pset_for("parity6")
    pop = configs.population(ps, "half", 300, 5, 3, 5)
    idx = np.random.default_rng(m).integers(0, ins.shape[1], m)
    if m > 2:
        idx[:3] = (63, 63, 0)
    ev = GPUEvaluator(ps, BooleanHits(ins, outs), device=0)
    fresh = GPUEvaluator(ps, BooleanHits(ins[:, idx], outs[idx]), device=0)
    try:
        full = ev.evaluate(pop)
        ev.subsample(idx)
        assert ev.n_cases == m and ev.full_n_cases == 64
        got, exp = ev.evaluate(pop), fresh.evaluate(pop)
        assert got == exp and max(r[0] for r in got) <= m
        a, b = ev.predict(pop), fresh.predict(pop)
        assert a.dtype == bool and a.shape == (len(pop), m) and np.array_equal(a, b)
        ev.subsample(None)
        assert ev.evaluate(pop) == full and ev.case_uploads == 1
    finally:
        ev.close()
        fresh.close()


# ------------------------------------------------------------ 4. residency --
def _batch(ev, pop):
    """A kept batch of *pop*, loaded with its exact pass."""
    batch = ev.lower_on_device(pop, keep=True) if ev.device_lowering else None
    if batch is None:
        batch = ev.flatten(pop)
    ev.prepare(batch, pop)
    return batch


def _raw(ev, batch):
    hi, lo, err, flags, _ = ev.run_batch(batch)
    return [np.array(a).copy() for a in (hi, lo, err, flags)]


def _same_raw(a, b, what):
    pr.assert_same_bits(a[0], b[0], what + " hi")
    pr.assert_same_bits(a[1], b[1], what + " lo")
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), what


def test_programs_stay_resident_and_nothing_stale_survives():
    ps, trees, X, y = cells()
    pop = trees[:300] + trees[-2:] + [gp.PrimitiveTree.from_string(HUGE, ps)]
    huge = len(pop) - 1
    rng = np.random.default_rng(8)
    idx_a, idx_b = rng.integers(0, N, 129), rng.integers(0, N, 129)
    ev = make_ev("mse", X, y)
    try:
        full = ev.evaluate(pop)
        assert ev.ctx.exact_host_runs() >= 1 and type(full[huge]) is tuple
        ev.subsample(idx_a)
        sub_a = ev.evaluate(pop)
        ev.subsample(None)
        assert ev.case_subset is None and ev.n_cases == N
        assert ev.ctx.case_subset() == (N, N, False)
        assert_same_results(ev.evaluate(pop), full, "the full set again")
        assert ev.case_uploads == 1
        # a kept batch on two subsets of the same size: lowered and flattened
        # once, each subset's own results
        batch = _batch(ev, pop)
        lowered, flatten_s = ev.stats["device_lowered"], ev.stats["flatten_s"]
        raws = []
        for idx in (idx_a, idx_b):
            ev.subsample(idx)
            raws.append(_raw(ev, batch))
            assert ev.ctx.resident is batch and ev.ctx.exact_host_runs() >= 1
            fresh = make_ev("mse", X[:, idx], y[idx])
            try:
                _same_raw(raws[-1], _raw(fresh, _batch(fresh, pop)), "kept batch")
                if idx is idx_a:
                    assert_same_results(sub_a, fresh.evaluate(pop), "subset a")
            finally:
                fresh.close()
        assert ev.stats["device_lowered"] == lowered and ev.stats["flatten_s"] == flatten_s
        assert raws[0][0][huge] != raws[1][0][huge]        # (the host pass saw each set)
        assert ev.case_uploads == 1
    finally:
        ev.close()


# ------------------------------------------------------------ 5. selection --
def test_selection_on_the_gathered_cases():
    ps, trees, X, y = cells()
    m, k, eps = 129, 300, 0.05
    idx = subset_idx(m, seed=5)
    idx[idx == INF_ROW] = 11                               # (no inf row: finite errors)
    if not hasattr(creator, "FitnessSubsetCases"):
        creator.create("FitnessSubsetCases", base.Fitness, weights=(-1.0,) * m)
        creator.create("IndividualSubsetCases", gp.PrimitiveTree,
                       fitness=creator.FitnessSubsetCases)
        creator.create("FitnessSubsetMin", base.Fitness, weights=(-1.0,))
        creator.create("IndividualSubsetMin", gp.PrimitiveTree, fitness=creator.FitnessSubsetMin)
    host = make_ev("case_abs_errors", X[:, idx], y[idx])
    dev = make_ev("case_abs_errors", X, y, cases="device")
    mse, mse_fresh = make_ev("mse", X, y), make_ev("mse", X[:, idx], y[idx])
    try:
        with np.errstate(over="ignore"):
            kept = [(t, r) for t, r in zip(trees, host.evaluate(trees))
                    if not isinstance(r, BaseException) and
                    np.isfinite(np.array(r) ** 2).all()][:300]
        assert len(kept) == 300
        pop = [creator.IndividualSubsetCases(t) for t, _ in kept]
        for ind, (_, r) in zip(pop, kept):
            ind.fitness.values = r
        dev.subsample(idx)
        with pytest.raises(ValueError, match="no per-case matrix"):
            dev.select_lexicase(pop, k)
        res = dev.evaluate(pop)
        assert all(type(r) is tuple and len(r) == 3 for r in res)
        where = {id(x): j for j, x in enumerate(pop)}
        for mode, ref in (("plain", lambda: tools.selLexicase(pop, k)),
                          ("epsilon", lambda: tools.selEpsilonLexicase(pop, k, eps)),
                          ("automatic", lambda: tools.selAutomaticEpsilonLexicase(pop, k))):
            random.seed(31)
            exp = [where[id(x)] for x in ref()]
            state = random.getstate()
            random.seed(31)
            got = [where[id(x)] for x in dev.select_lexicase(pop, k, mode, eps)]
            assert got == exp and random.getstate() == state, mode
            assert len(set(got)) > 5
        dev.subsample(subset_idx(m, seed=6))
        with pytest.raises(ValueError, match="no per-case matrix"):
            dev.select_lexicase(pop, k)
        # the resident MSE after a subset: the tournament on the device
        # against selTournament on a fresh evaluator's fitnesses
        plain = [creator.IndividualSubsetMin(t) for t, _ in kept]
        for ind, fit in zip(plain, mse_fresh.evaluate(plain)):
            ind.fitness.values = fit
        mse.subsample(idx)
        got_fit = mse.evaluate(plain)
        assert_same_results(got_fit, [ind.fitness.values for ind in plain], "mse")
        random.seed(9)
        exp = [id(x) for x in tools.selTournament(plain, 200, 3)]
        state = random.getstate()
        random.seed(9)
        sel = mse.ctx.tournament(None, 200, 3, random._inst, weight=-1.0)
        assert [id(plain[i]) for i in sel.tolist()] == exp and random.getstate() == state
        random.seed(9)
        assert [id(x) for x in tools.selTournamentGPU(plain, 200, 3, device=0)] == exp
        mse.subsample(None)                               # nothing resident any more
        with pytest.raises(_lib.GpeError):
            mse.ctx.tournament(None, 200, 3, random._inst, weight=-1.0)
    finally:
        for ev in (host, dev, mse, mse_fresh):
            ev.close()


# ------------------------------------------------------------ 6. the C ABI --
def test_the_c_abi_by_raw_ctypes():
    ps, trees, X, y = cells()
    n = 64
    ev = make_ev("case_abs_errors", X[:, :n], y[:n])
    lib, P = ev.ctx.lib, _lib._ptr
    h = ev.ctx.h
    I64 = ctypes.c_int64

    def subset():
        m, full = I64(), I64()
        assert lib.gpe_case_subset(h, ctypes.byref(m), ctypes.byref(full)) == 0
        return m.value, full.value
    try:
        pop = trees[16:48]
        base_res = ev.evaluate(pop)
        assert subset() == (-1, n)
        idx = np.array([5, 5, 63, 0, 17], dtype=np.int64)
        assert lib.gpe_select_cases(h, P(idx), len(idx)) == 0
        assert subset() == (5, n)
        # the matrix and the resident fitness belong to the previous set
        mx = np.zeros(5, dtype=np.uint8)
        with pytest.raises(_lib.GpeError, match="no per-case values"):
            ev.ctx.lexicase(None, mx, 4, random.Random(3), 0)
        with pytest.raises(_lib.GpeError):
            ev.ctx.tournament(None, 4, 3, random.Random(3), weight=-1.0)
        ev.ctx.n_cases = 5
        cases, w4, err, flags = ev.ctx.run_abserr_cases(ar.HIT_EPS, 5)
        assert cases.shape == (len(pop), 5)
        pr.assert_same_bits(cases[:, 0], cases[:, 1], "a duplicate case")
        assert ev.ctx.lexicase(None, mx, 4, random.Random(3), 0)[1] == -1
        # refusals: the active set stays as it was
        for bad, where in (([1, 64], "idx[1] = 64"), ([-1, 2], "idx[0] = -1"),
                           ([0, 1, 2, 1 << 40], "idx[3] = %d" % (1 << 40))):
            b = np.array(bad, dtype=np.int64)
            assert lib.gpe_select_cases(h, P(b), len(b)) == _lib.GPE_E_INVALID
            msg = lib.gpe_last_error(h).decode()
            assert where in msg and "[0, 64)" in msg, msg
            assert subset() == (5, n)
        for m in (0, -3):
            assert lib.gpe_select_cases(h, P(idx), m) == _lib.GPE_E_INVALID
            assert subset() == (5, n)
        again = ev.ctx.run_abserr_cases(ar.HIT_EPS, 5)
        pr.assert_same_bits(again[0], cases, "after the refusals")
        assert lib.gpe_select_cases(None, P(idx), 5) == _lib.GPE_E_INVALID
        # NULL: the full set; its results are the first evaluation's
        assert lib.gpe_select_cases(h, None, 0) == 0
        assert subset() == (-1, n)
        ev.ctx.n_cases = n
        assert_same_results(ev.evaluate(pop), base_res, "the full set again")
        # gpe_set_cases while a subset is active leaves none
        assert lib.gpe_select_cases(h, P(idx), len(idx)) == 0
        assert subset() == (5, n)
        ev.ctx.set_cases(_lib.GPE_MACHINE_F, np.ascontiguousarray(X[:, :40]),
                         np.ascontiguousarray(y[None, :40]))
        assert subset() == (-1, 40)
        # ... and so does gpe_set_trig_leaves
        idx40 = np.array([5, 5, 39, 0, 17], dtype=np.int64)
        assert lib.gpe_select_cases(h, P(idx), len(idx)) == _lib.GPE_E_INVALID     # (63 >= 40)
        assert lib.gpe_select_cases(h, P(idx40), len(idx40)) == 0
        assert subset() == (5, 40)
        ev.ctx.set_trig_leaves(False)
        assert subset() == (-1, 40) and ev.ctx.n_cases == 40
    finally:
        ev.close()
