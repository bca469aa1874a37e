"""Confusion figures without a GPU: the host twin of the masked counts
(``gpe_host_hit_group_counts``) against numpy on unpacked bits, the twelve
figures against a pure-Python restatement on ints, the validation and the
ABI."""
import itertools
import math
import os
import re

import numpy as np
import pytest

from deap_amd import _lib, build, datasets
from deap_amd import evaluator as evm
from deap_amd.evaluator import (BooleanCaseHits, BooleanConfusion, GPUEvaluator, TypedCaseHits,
                                TypedConfusion, confusion_figures, pack_bitplanes,
                                unpack_bitplanes)

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("tp", "fp", "fn", "tn", "hits", "accuracy", "recall", "specificity", "precision",
         "balanced_accuracy", "f1", "mcc")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def figures_ref(tp, fp, fn, tn):
    """The issue's definitions on Python ints."""
    P, N = tp + fn, fp + tn
    recall = tp / P if P else 0.0
    specificity = tn / N if N else 0.0
    if P == 0:
        balanced = specificity
    elif N == 0:
        balanced = recall
    else:
        balanced = (recall + specificity) / 2
    a, b = (tp + fp) * (tp + fn), (tn + fp) * (tn + fn)
    mcc = 0.0 if a == 0 or b == 0 else \
        float(tp * tn - fp * fn) / (math.sqrt(float(a)) * math.sqrt(float(b)))
    den = 2 * tp + fp + fn
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "hits": tp + tn,
            "accuracy": (tp + tn) / (P + N), "recall": recall, "specificity": specificity,
            "precision": tp / (tp + fp) if tp + fp else 0.0, "balanced_accuracy": balanced,
            "f1": (2 * tp) / den if den else 0.0, "mcc": mcc}


def random_planes(rng, n, n_cases, pad):
    """uint32[n, units] of random bits; *pad*: the pad bits random too."""
    units = (n_cases + 31) // 32
    words = rng.integers(0, 1 << 32, size=(n, units), dtype=np.uint64).astype(np.uint32)
    if not pad and n_cases % 32:
        words[:, -1] &= np.uint32((1 << (n_cases % 32)) - 1)
    return words


# ------------------------------------------------------------- host twin --
@pytest.mark.parametrize("n_cases", [1, 31, 32, 33, 64, 65, 4601])
@pytest.mark.parametrize("G", [1, 2, 8])
def test_the_host_twin_is_numpy_on_the_unpacked_bits(lib, n_cases, G):
    rng = np.random.default_rng(n_cases * 10 + G)
    n = 37
    for pad in (False, True):
        planes = random_planes(rng, n, n_cases, pad)
        masks = random_planes(rng, G, n_cases, pad)
        masks[0] = 0                                          # an all-zero mask
        masks[-1] = 0xFFFFFFFF                                # an all-one mask, pad bits too
        rows, sel = unpack_bitplanes(planes, n_cases), unpack_bitplanes(masks, n_cases)
        exp = (rows[:, None, :] & sel[None]).sum(-1)
        got = _lib.host_hit_group_counts(planes, n_cases, masks)
        assert got.dtype == np.int64 and got.shape == (n, G)
        assert np.array_equal(got, exp)
        # a mask with pad bits set is the same mask with them cleared
        clean = pack_bitplanes(sel)
        assert np.array_equal(_lib.host_hit_group_counts(planes, n_cases, clean), exp)
        assert (got[:, -1] == rows.sum(1)).all()
        if G > 1:
            assert not got[:, 0].any()
    none = _lib.host_hit_group_counts(np.zeros((0, (n_cases + 31) // 32), dtype=np.uint32),
                                      n_cases, masks)
    assert none.shape == (0, G)


def test_the_library_refuses_bad_arguments(lib):
    planes = np.zeros((3, 2), dtype=np.uint32)
    for G in (0, 9):
        with pytest.raises(_lib.GpeError, match=r"gpe_host_hit_group_counts failed \(-6\)"):
            _lib.host_hit_group_counts(planes, 40, np.zeros((G, 2), dtype=np.uint32))
    with pytest.raises(ValueError, match=r"masks must be uint32 \[G, 2\]"):
        _lib.host_hit_group_counts(planes, 40, np.zeros((1, 3), dtype=np.uint32))
    with pytest.raises(ValueError, match=r"planes must be uint32 \[n, 2\]"):
        _lib.host_hit_group_counts(np.zeros((3, 1), dtype=np.uint32), 40,
                                   np.zeros((1, 2), dtype=np.uint32))
    P = _lib._ptr
    masks, out = np.zeros((1, 2), dtype=np.uint32), np.zeros((3, 1), dtype=np.int32)
    call = lib.gpe_host_hit_group_counts
    assert call(P(planes), 3, 40, P(masks), 1, P(out)) == 0
    for args in ((P(planes), -1, 40, P(masks), 1, P(out)),
                 (P(planes), 3, 0, P(masks), 1, P(out)),
                 (P(planes), 3, 40, None, 1, P(out)),
                 (P(planes), 3, 40, P(masks), 1, None),
                 (None, 3, 40, P(masks), 1, P(out))):
        assert call(*args) == _lib.GPE_E_ARG, args[1:5]
    assert call(None, 0, 40, P(masks), 1, None) == 0          # n == 0: nothing written
    assert lib.gpe_hit_group_counts(None, None, 0, 0, P(masks), 1, None) == _lib.GPE_E_INVALID


# --------------------------------------------------------------- figures --
def grid():
    small = (0, 1, 2, 7)
    cells = [c for c in itertools.product(small, repeat=4) if sum(c) > 0]
    big = 1 << 30
    cells += [(big, 5, 7, big - 100), (big, 0, 0, big - 1), (0, big, big - 1, 0),
              (big - 3, big - 1, 0, 0), (0, 0, big - 1, big - 3), (big, big, big, big),
              (big, 0, big, 0), (0, big, 0, big), (3, big, big, 5), (big, 3, 5, big)]
    return cells


def test_the_twelve_figures_are_the_definitions_on_python_ints():
    cells = grid()
    # every zero denominator is in the grid
    assert any(tp + fn == 0 for tp, fp, fn, tn in cells)              # P == 0
    assert any(fp + tn == 0 for tp, fp, fn, tn in cells)              # N == 0
    assert any(tp + fp == 0 for tp, fp, fn, tn in cells)
    assert any(tn + fn == 0 for tp, fp, fn, tn in cells)
    assert any(2 * tp + fp + fn == 0 for tp, fp, fn, tn in cells)
    for i in range(4):                                                # mcc's four sums
        assert any([tp + fp, tp + fn, tn + fp, tn + fn][i] == 0 for tp, fp, fn, tn in cells)
    cols = confusion_figures(np.array(cells, dtype=np.int64), NAMES)
    assert tuple(cols) == NAMES
    for name in NAMES:
        got = cols[name].tolist()
        kind = int if name in NAMES[:5] else float
        assert all(type(v) is kind for v in got), name
        for cell, v in zip(cells, got):
            assert v == figures_ref(*cell)[name], (name, cell, v, figures_ref(*cell)[name])


def test_finish_all_builds_the_tuples_from_hits_and_true_positives():
    X, lab = datasets.spambase_like(300, 57)
    spec = TypedConfusion(X, lab, fitness=NAMES)
    P = int(np.count_nonzero(lab))
    assert spec.positives() == P and spec.cases == "device" and spec.hit_planes
    plane = spec.label_plane()
    assert plane.dtype == np.uint32 and plane.shape == (10,)
    assert np.array_equal(unpack_bitplanes(plane, 300)[0], lab != 0)
    rng = np.random.default_rng(3)
    tp = rng.integers(0, P + 1, size=50)
    tn = rng.integers(0, 300 - P + 1, size=50)
    tp[:2], tn[:2] = (0, P), (300 - P, 0)                             # "False" and "True"
    hits = (tp + tn).astype(np.float64)
    err = np.full(50, _lib.GPE_NO_ERROR, dtype=np.uint64)
    err[7] = np.uint64((3 << 2) | _lib.GPE_ERR_OVERFLOW)
    out = spec.finish_all(hits, None, err, None, cases=tp)
    conf = spec.confusion_counts(hits, tp, err)
    assert conf.dtype == np.int64 and conf.shape == (50, 4) and conf[7].tolist() == [-1] * 4
    assert isinstance(out[7], OverflowError)
    for i in range(50):
        if i == 7:
            continue
        cell = (int(tp[i]), 300 - P - int(tn[i]), P - int(tp[i]), int(tn[i]))
        assert conf[i].tolist() == list(cell)
        assert out[i] == tuple(figures_ref(*cell)[k] for k in NAMES)
    assert spec.finish_all(hits, None, None, None, cases=tp)[7] == \
        tuple(figures_ref(int(tp[7]), 300 - P - int(tn[7]), P - int(tp[7]), int(tn[7]))[k]
              for k in NAMES)
    assert spec.finish_all(np.zeros(0), None, None, None, cases=np.zeros(0)) == []
    # a subset carries its own labels
    idx = np.array([5, 5, 299, 0, 17])
    sub = spec.subset(idx)
    assert sub.n_cases == 5 and sub.positives() == int(np.count_nonzero(lab[idx]))
    assert np.array_equal(unpack_bitplanes(sub.label_plane(), 5)[0], lab[idx] != 0)
    assert sub.fitness == NAMES


def test_the_prefixes_of_the_gpu_tests_have_the_stated_positives():
    X, lab = datasets.spambase_like(300, 57)
    assert [int(np.count_nonzero(lab[:n])) for n in (1, 2, 33, 64, 65, 129, 300)] == \
        [0, 1, 11, 21, 22, 48, 112]


def test_the_boolean_spec_counts_the_ones_of_the_output_plane():
    rows = [[(c >> v) & 1 for v in range(6)] for c in range(64)]
    outs = [sum(r) % 2 for r in rows]
    spec = BooleanConfusion.from_rows(rows, outs, fitness=("tp", "mcc"))
    assert isinstance(spec, BooleanCaseHits) and spec.cases == "device"
    assert spec.n_cases == 64 and spec.positives() == 32 and spec.fitness == ("tp", "mcc")
    assert np.array_equal(unpack_bitplanes(spec.label_plane(), 64)[0], np.array(outs) == 1)
    sub = spec.subset(np.array([1, 2, 3, 3]))
    assert sub.positives() == sum(outs[c] for c in (1, 2, 3, 3))
    assert BooleanConfusion(np.array(rows).T, outs).fitness == ("balanced_accuracy",)


# ------------------------------------------------------------ validation --
def test_fitness_is_validated_like_the_abs_error_spec():
    X, lab = datasets.spambase_like(8, 57)
    rows = [[0, 1], [1, 1]]
    for bad in ((), ("auc",), ("tp", "nope"), "kappa"):
        with pytest.raises(ValueError, match="fitness must be a non-empty tuple drawn from"):
            TypedConfusion(X, lab, fitness=bad)
        with pytest.raises(ValueError, match="fitness must be a non-empty tuple drawn from"):
            BooleanConfusion.from_rows(rows, [0, 1], fitness=bad)
    assert TypedConfusion(X, lab).fitness == ("balanced_accuracy",)
    assert TypedConfusion(X, lab, fitness="f1").fitness == ("f1",)
    assert TypedConfusion.NAMES == NAMES == evm.CONFUSION_NAMES
    with pytest.raises(ValueError, match="unknown confusion figure"):
        confusion_figures(np.zeros((1, 4), dtype=np.int64), ("auc",))
    with pytest.raises(NotImplementedError, match="bit-sliced evaluation needs 0/1 data"):
        BooleanConfusion.from_rows([[0, 2]], [1])


def test_setup_refusals_are_the_parents(lib):
    from deap_amd import configs, distributed
    X, lab = datasets.spambase_like(8, 57)
    with pytest.raises(NotImplementedError, match="TypedConfusion needs precision='fp64'"):
        GPUEvaluator(configs.pset_for("spambase"), TypedConfusion(X, lab), precision="fp32")
    rows = [[(c >> v) & 1 for v in range(57)] for c in range(4)]
    with pytest.raises(NotImplementedError,
                       match="BooleanConfusion does not take a typed primitive set"):
        GPUEvaluator(configs.pset_for("spambase"), BooleanConfusion.from_rows(rows, [0, 1, 1, 0]))
    for spec in (TypedConfusion(X, lab), BooleanConfusion.from_rows(rows, [0, 1, 1, 0])):
        with pytest.raises(NotImplementedError, match="%s runs on one GPU" % type(spec).__name__):
            distributed._check_shardable(spec, False)


# ------------------------------------------------------ group_hits plumbing --
class _StubContext(object):
    """What group_hits reads of a context, the counts by the host twin."""

    def __init__(self, planes, n_cases):
        self.planes, self.n_cases, self.n_prog = planes, n_cases, len(planes)
        self.calls = []

    def hit_group_counts(self, planes, n, n_cases, masks):
        assert planes is None and n == 0 and n_cases == 0
        self.calls.append(np.array(masks))
        return _lib.host_hit_group_counts(self.planes, self.n_cases, masks)


def _stub_evaluator(hit, results, cls=TypedCaseHits):
    X, lab = datasets.spambase_like(hit.shape[1], 57)
    ev = GPUEvaluator.__new__(GPUEvaluator)
    ev.spec = ev._full_spec = cls(X, lab, "device") if cls is TypedCaseHits else cls(X, lab)
    ev.case_subset = None
    ev.ctx = _StubContext(pack_bitplanes(hit), hit.shape[1])
    ev._lex_batch = ([object() for _ in results], list(results))
    return ev


def test_group_hits_takes_masks_or_index_lists_and_slices_past_eight_groups(lib):
    rng = np.random.default_rng(8)
    hit = rng.random((6, 70)) < 0.5
    results = [(1,), (2,), OverflowError("x"), (3,), (4,), (5,)]
    for cls in (TypedCaseHits, TypedConfusion):
        ev = _stub_evaluator(hit, results, cls)
        folds = [list(range(0, 20)), list(range(20, 50)), list(range(50, 70))]
        got = ev.group_hits(folds)
        assert got.dtype == np.int64 and got.shape == (6, 3)
        assert got[2].tolist() == [-1] * 3                     # the one that raised
        keep = [0, 1, 3, 4, 5]
        exp = np.stack([hit[:, f].sum(1) for f in folds], axis=1)
        assert np.array_equal(got[keep], exp[keep])
        assert np.array_equal(got[keep].sum(1), hit.sum(1)[keep])
        masks = np.zeros((3, 70), dtype=bool)
        for g, f in enumerate(folds):
            masks[g, f] = True
        assert np.array_equal(ev.group_hits(masks), got)
        assert np.array_equal(ev.group_hits(masks.tolist()), got)
        # duplicates count once; ragged and empty groups
        got2 = ev.group_hits([[3, 3, 3, 69], [], np.array([0])])
        assert np.array_equal(got2[keep], np.stack(
            [hit[:, 3] * 1 + hit[:, 69], np.zeros(6, dtype=int), hit[:, 0] * 1], axis=1)[keep])
        # eleven groups: slices of eight and three
        many = rng.random((11, 70)) < 0.3
        ev.ctx.calls.clear()
        got11 = ev.group_hits(many)
        assert [len(m) for m in ev.ctx.calls] == [8, 3]
        assert np.array_equal(got11[keep], (hit[:, None, :] & many[None]).sum(-1)[keep])
        assert ev.group_hits([]).shape == (6, 0)
        for bad in ([[0, 70]], [[-1]]):
            with pytest.raises(IndexError, match=r"group_hits: groups\[0\]\[\d\] = -?\d+ is outside"):
                ev.group_hits(bad)
        with pytest.raises(ValueError, match="1-D sequence of integer case indices"):
            ev.group_hits([[0.5, 1.0]])
        with pytest.raises(ValueError, match=r"boolean groups array must be \[G, 70\]"):
            ev.group_hits(np.zeros((2, 69), dtype=bool))
        ev.ctx.n_prog = 4
        with pytest.raises(ValueError, match="group_hits: the context now holds 4 programs"):
            ev.group_hits(folds)
        ev._lex_batch = None
        with pytest.raises(ValueError, match="group_hits: .* left no hit planes on the GPU"):
            ev.group_hits(folds)
    ev = _stub_evaluator(hit, results)
    ev.spec = evm.TypedBoolHits(*datasets.spambase_like(70, 57))
    with pytest.raises(ValueError, match="its spec is TypedBoolHits"):
        ev.group_hits([[0]])


# ------------------------------------------------------------------- ABI --
def test_the_abi_is_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpeval.h")).read()
    P, I, I64 = _lib._P, _lib._I, _lib._I64
    want = {"gpe_hit_group_counts": [P, P, I64, I64, P, I, P],
            "gpe_host_hit_group_counts": [P, I64, I64, P, I, P]}
    ctype = {"int64_t": I64, "int": I}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args)
        assert getattr(lib, name).argtypes == args
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, name
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        got = [P if "*" in a else ctype[a.rsplit(" ", 1)[0].strip()] for a in decl]
        assert got == args, (name, decl)
    assert re.search(r"\bint gpe_last_hit_group_ms\(const gpe_ctx\* ctx, float\* ms\);", header)
    assert _lib.SIGNATURES["gpe_last_hit_group_ms"][0] is I and callable(_lib.Context.hit_group_ms)
    assert lib.gpe_last_hit_group_ms(None, None) == _lib.GPE_E_INVALID
    assert "hit_groups.h" in build.LIB_HEADERS
    variant = open(os.path.join(os.path.dirname(HERE), "scripts", "build_variant.sh")).read()
    assert "deap_amd/csrc/hit_groups.h" in variant
    assert callable(_lib.Context.hit_group_counts) and callable(_lib.host_hit_group_counts)
    assert callable(GPUEvaluator.group_hits)
    for name in ("TypedConfusion", "BooleanConfusion"):
        assert name in evm.__all__
    assert issubclass(TypedConfusion, TypedCaseHits)
    assert issubclass(BooleanConfusion, BooleanCaseHits)
    assert _lib.HIT_GROUPS_MAX == 8
