"""Case weights on the CPU: the host twins (``gpe_host_case_solve_counts``,
``gpe_host_hit_weighted_sums``, ``gpe_host_hit_shared_sums``) against the
definitions of ``case_weights_ref`` — counts equal, sums bit-equal to
``math.fsum`` where every partial sum is representable, within 1e-12 relative
on random weights, and the double-double pair within ``n_cases * 2**-100`` of
the exact sum in ``fractions.Fraction``."""
import math
from fractions import Fraction

import numpy as np
import pytest

import case_weights_ref as ref
from deap_amd import _lib
from deap_amd.evaluator import pack_bitplanes, unpack_bitplanes


def random_words(rng, n, units):
    return rng.integers(0, 1 << 32, size=(n, units), dtype=np.uint64).astype(np.uint32)


def dyadic_weights(rng, G, n_cases):
    """Multiples of 2**-20 in [0, 1024], a fifth of them zero."""
    w = rng.integers(0, (1 << 30) + 1, size=(G, n_cases)).astype(np.float64) / float(1 << 20)
    w[rng.random((G, n_cases)) < 0.2] = 0.0
    return w


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------- counts --
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_the_counts_are_the_column_sums_of_the_live_rows(n):
    for n_cases in (1, 31, 32, 33, 64, 65, 300):
        rng = np.random.default_rng(n * 1009 + n_cases)
        planes = random_words(rng, n, (n_cases + 31) // 32)       # (pad bits set)
        H = unpack_bitplanes(planes, n_cases)
        W = (n + 63) // 64
        ones = np.full(W, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        alive = rng.random(n) < 0.7
        ragged = _lib.pack_live_mask(alive)
        if n % 64:
            ragged[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)   # (pad bits set)
        for live, rows in ((None, np.ones(n, dtype=bool)), (ones, np.ones(n, dtype=bool)),
                           (ragged, alive)):
            got = _lib.host_case_solve_counts(planes, n_cases, live)
            assert got.dtype == np.int64 and got.shape == (n_cases,)
            assert np.array_equal(got, H[rows].sum(0)), (n, n_cases)
        if n <= 129 and n_cases <= 65:
            assert got.tolist() == ref.solve_counts(H.tolist(), alive.tolist())


def test_the_live_mask_packs_bit_i_of_word_i_div_64():
    alive = np.zeros(130, dtype=bool)
    alive[[0, 63, 64, 129]] = True
    assert _lib.pack_live_mask(alive).tolist() == [1 | 1 << 63, 1, 2]
    assert _lib.pack_live_mask(np.ones(64, dtype=bool)).tolist() == [2 ** 64 - 1]


# ------------------------------------------------------- weighted: exact --
@pytest.mark.parametrize("n, n_cases, G", [
    (40, 1, 1), (40, 33, 3), (40, 64, 8), (40, 65, 2), (30, 129, 3), (20, 2049, 2),
    (12, 4601, 8), (3, 65536, 1)])
def test_exactly_representable_sums_are_fsum_bit_for_bit(n, n_cases, G):
    rng = np.random.default_rng(n_cases * 31 + G)
    planes = random_words(rng, n, (n_cases + 31) // 32)           # (pad bits set)
    w = dyadic_weights(rng, G, n_cases)
    got = _lib.host_hit_weighted_sums(planes, n_cases, w)
    H = unpack_bitplanes(planes, n_cases)
    exp = np.array(ref.weighted_hits(H.tolist(), w.tolist()))
    assert got.shape == (n, G) and bits_equal(got, exp)
    # (exact sums do not depend on the order: numpy's matrix product agrees)
    assert bits_equal(got, H.astype(np.float64) @ w.T)
    one = _lib.host_hit_weighted_sums(planes, n_cases, w[0])      # 1-D weights: G = 1
    assert bits_equal(one[:, 0], exp[:, 0])


# ------------------------------------------------------ weighted: random --
def test_uniform_weights_are_within_1e_12_of_fsum(capsys):
    same = total = 0
    for n, n_cases, G in ((200, 300, 3), (100, 4601, 2), (300, 65, 8)):
        rng = np.random.default_rng(n_cases)
        planes = random_words(rng, n, (n_cases + 31) // 32)
        w = rng.random((G, n_cases))
        got = _lib.host_hit_weighted_sums(planes, n_cases, w)
        exp = np.array(ref.weighted_hits(unpack_bitplanes(planes, n_cases).tolist(), w.tolist()))
        assert (np.abs(got - exp) <= 1e-12 * exp).all(), np.abs(got / exp - 1).max()
        same += int((got.view(np.uint64) == exp.view(np.uint64)).sum())
        total += got.size
    with capsys.disabled():
        print("\nuniform weights: %d of %d sums bit-identical to fsum (%.2f %%)"
              % (same, total, 100.0 * same / total))


@pytest.mark.parametrize("n_cases", [65, 500, 4601])
def test_the_pair_is_within_the_double_double_bound_of_the_exact_sum(n_cases, capsys):
    rng = np.random.default_rng(n_cases + 7)
    n = 200
    planes = random_words(rng, n, (n_cases + 31) // 32)
    w = (1.0 + rng.random((1, n_cases))) * np.exp2(rng.integers(-60, 61, size=(1, n_cases)))
    hi, lo = _lib.host_hit_weighted_sums(planes, n_cases, w, pair=True)
    H = unpack_bitplanes(planes, n_cases)
    fr = [Fraction(v) for v in w[0].tolist()]
    bound = Fraction(n_cases, 2 ** 100)
    same = 0
    for i in range(n):
        exact = sum((fr[c] for c in np.flatnonzero(H[i]).tolist()), Fraction(0))
        pair = Fraction(float(hi[i, 0])) + Fraction(float(lo[i, 0]))
        assert abs(pair - exact) <= bound * exact, (i, float(abs(pair - exact) / exact))
        fs = math.fsum(w[0, c] for c in np.flatnonzero(H[i]).tolist())
        assert abs(hi[i, 0] - fs) <= 1e-12 * fs
        same += hi[i, 0] == fs
    with capsys.disabled():
        print("\nweights over 2^-60 .. 2^60, %d cases: %d of %d sums bit-identical to fsum"
              % (n_cases, same, n))


# ---------------------------------------------------------------- shared --
@pytest.mark.parametrize("n, n_cases", [(1, 1), (1, 40), (63, 33), (130, 64), (200, 300)])
def test_shared_sums_follow_the_definition(n, n_cases):
    rng = np.random.default_rng(n * 7 + n_cases)
    H = rng.random((n, n_cases)) < rng.random(n_cases)[None, :]   # easy and hard cases
    if n_cases > 2:
        H[:, 1] = False                                           # a case nobody solves
        H[:, 2] = True                                            # a case everyone solves
    planes = pack_bitplanes(H)
    if n_cases % 32:
        planes[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(n_cases % 32)     # (pad bits set)
    alive = np.ones(n, dtype=bool)
    if n > 3:
        alive[[0, n - 1]] = False
    for rows, live in ((np.ones(n, dtype=bool), None), (alive, _lib.pack_live_mask(alive))):
        cnt, (hi, lo) = _lib.host_hit_shared_sums(planes, n_cases, live, pair=True)
        s, sh = ref.shared_hits(H.tolist(), None if live is None else rows.tolist())
        assert cnt.tolist() == s == H[rows].sum(0).tolist()
        exp = np.array(sh)
        assert (np.abs(hi[rows] - exp[rows]) <= 1e-12 * exp[rows]).all()
        ws = np.array([1.0 / c if c else 0.0 for c in s])
        # the same sum as the weighted twin under the counts' weights
        assert bits_equal(hi, _lib.host_hit_weighted_sums(planes, n_cases, ws)[:, 0])
        frs = [Fraction(v) for v in ws.tolist()]
        for i in np.flatnonzero(rows)[:50].tolist():
            exact = sum((frs[c] for c in np.flatnonzero(H[i]).tolist()), Fraction(0))
            pair = Fraction(float(hi[i])) + Fraction(float(lo[i]))
            assert abs(pair - exact) <= Fraction(n_cases, 2 ** 100) * exact
    if n_cases > 2:
        assert cnt[1] == 0 and cnt[2] == alive.sum()
    if n == 1:                                                    # alone: every solved case is 1
        assert hi.tolist() == [float(H[0].sum())]


def test_dead_rows_change_the_counts_and_are_left_out_of_them():
    H = np.array([[1, 1, 0], [1, 0, 0], [1, 1, 1]], dtype=bool)
    planes = pack_bitplanes(H)
    cnt, sh = _lib.host_hit_shared_sums(planes, 3)
    assert cnt.tolist() == [3, 2, 1] and sh.tolist() == [1 / 3 + 1 / 2, 1 / 3, 1 / 3 + 1 / 2 + 1.0]
    live = _lib.pack_live_mask(np.array([True, True, False]))
    cnt, sh = _lib.host_hit_shared_sums(planes, 3, live)
    assert cnt.tolist() == [2, 1, 0] and sh[:2].tolist() == [1 / 2 + 1.0, 1 / 2]
    assert _lib.host_case_solve_counts(planes, 3, live).tolist() == [2, 1, 0]


# ------------------------------------------------------------ edge cases --
def test_zero_weights_empty_rows_and_full_rows():
    n_cases = 100
    H = np.zeros((3, n_cases), dtype=bool)
    H[1] = True
    H[2, ::3] = True
    planes = pack_bitplanes(H)
    planes[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(n_cases % 32)         # (pad bits set)
    rng = np.random.default_rng(5)
    w = np.stack([dyadic_weights(rng, 1, n_cases)[0], np.full(n_cases, -0.0), np.ones(n_cases)])
    hi, lo = _lib.host_hit_weighted_sums(planes, n_cases, w, pair=True)
    zero = np.zeros(1).view(np.uint64)[0]
    assert (hi[0].view(np.uint64) == zero).all() and (lo[0].view(np.uint64) == zero).all()
    assert (hi[:, 1].view(np.uint64) == zero).all()               # -0.0 weights: +0.0
    assert hi[1, 0] == math.fsum(w[0].tolist()) and hi[1, 2] == 100.0
    assert hi[2].tolist() == [math.fsum(w[0, ::3].tolist()), 0.0, 34.0]
    assert hi.shape == (3, 3)


def test_the_python_wrappers_refuse_bad_weights():
    planes = np.zeros((2, 2), dtype=np.uint32)
    good = np.ones(40)
    for bad, text in ((np.ones(39), r"weights must be float64 \[40\] or \[G, 40\]"),
                      (np.ones((2, 3, 40)), "weights must be float64"),
                      (np.where(np.arange(40) == 3, np.nan, good), "finite"),
                      (np.where(np.arange(40) == 3, np.inf, good), "finite"),
                      (np.where(np.arange(40) == 3, -1e-300, good), ">= 0"),
                      (np.full(40, 1e308), r"sum of weights\[0\] overflows")):
        with pytest.raises(ValueError, match=text):
            _lib.host_hit_weighted_sums(planes, 40, bad)
    top = np.zeros(40)
    top[:2] = 8e307                                               # 1.6e308: still a float
    assert _lib.check_case_weights("t", top, 40).shape == (1, 40)
    assert _lib.HIT_WEIGHTS_MAX == 8


def test_the_twins_answer_gpe_e_arg_where_the_header_says():
    lib = _lib.load()
    P = _lib._ptr
    planes = np.zeros((3, 2), dtype=np.uint32)
    w = np.ones((9, 40))
    out, lo = np.zeros((3, 9)), np.zeros((3, 9))
    cnt = np.zeros(40, dtype=np.int32)
    ARG = _lib.GPE_E_ARG
    ws = lib.gpe_host_hit_weighted_sums
    assert ws(P(planes), 3, 40, P(w), 1, P(out), P(lo)) == 0
    assert ws(P(planes), 3, 40, P(w), 8, P(out), None) == 0       # (out_lo is optional)
    for args in ((P(planes), 3, 40, P(w), 0, P(out), None), (P(planes), 3, 40, P(w), 9, P(out), None),
                 (P(planes), -1, 40, P(w), 1, P(out), None), (P(planes), 3, 0, P(w), 1, P(out), None),
                 (P(planes), 3, 2 ** 31, P(w), 1, P(out), None),
                 (P(planes), 3, 40, None, 1, P(out), None), (P(planes), 3, 40, P(w), 1, None, None),
                 (None, 3, 40, P(w), 1, P(out), None)):
        assert ws(*args) == ARG, args[1:5]
    for bad in (np.nan, np.inf, -1.0):
        wb = np.ones((1, 40))
        wb[0, 39] = bad
        assert ws(P(planes), 3, 40, P(wb), 1, P(out), None) == ARG
    assert ws(None, 0, 40, P(w), 1, None, None) == 0              # n == 0
    sc = lib.gpe_host_case_solve_counts
    assert sc(P(planes), 3, 40, None, P(cnt)) == 0
    for args in ((P(planes), -1, 40, None, P(cnt)), (P(planes), 3, 0, None, P(cnt)),
                 (P(planes), 2 ** 31, 40, None, P(cnt)), (P(planes), 3, 40, None, None),
                 (None, 3, 40, None, P(cnt))):
        assert sc(*args) == ARG, args[1:3]
    cnt[:] = 7
    assert sc(None, 0, 40, None, P(cnt)) == 0 and not cnt.any()   # n == 0: nobody solves anything
    sh = lib.gpe_host_hit_shared_sums
    assert sh(P(planes), 3, 40, None, None, P(out), None) == 0    # (the counts are optional)
    for args in ((P(planes), -1, 40, None, P(cnt), P(out), None),
                 (P(planes), 3, 0, None, P(cnt), P(out), None),
                 (P(planes), 2 ** 31, 40, None, P(cnt), P(out), None),
                 (P(planes), 3, 40, None, P(cnt), None, None),
                 (None, 3, 40, None, P(cnt), P(out), None)):
        assert sh(*args) == ARG, args[1:3]
