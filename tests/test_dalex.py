"""DALex selection without a GPU: the host twins (``_lib.host_dalex``,
``host_dalex_weights``, ``host_dalex_sigma``) against the pure-Python
restatement of the rule in ``dalex_ref`` — keys, weights, standardisation,
ties, unfit rows — and the arguments they refuse."""
import math

import numpy as np
import pytest

import dalex_ref as ref
from deap_amd import _lib, tools


def errors(seed, n, n_cases):
    rng = np.random.default_rng(seed)
    return np.abs(rng.normal(size=(n, n_cases))) * rng.uniform(0.1, 10.0, n_cases)


def test_the_keys_of_the_header_hold_through_the_new_entry_points():
    assert ref.key(0, 0) == 0xE220A8397B1DCDAF and ref.key(0, 1) == 0x6E789E6AA1B965F4
    # two cases, one selection, seed 0: case 0's score is made of K(0) and
    # K(1), case 1's of K(2) and K(3), and w_0 / w_1 = exp(I_0 - I_1)
    u1 = float((0xE220A8397B1DCDAF >> 11) + 1) * 2.0 ** -53
    u2 = float(0x6E789E6AA1B965F4 >> 11) * 2.0 ** -53
    i0 = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
    i1 = ref.importance(0, 1, 1.0)
    assert i0 == ref.importance(0, 0, 1.0)
    wt = _lib.host_dalex_weights(2, 1, 0, 1.0)
    assert wt[0, 0] / wt[1, 0] == pytest.approx(math.exp(i0 - i1), rel=1e-13)
    # a 64-bit seed and its reduction mod 2^64 are one seed
    assert np.array_equal(_lib.host_dalex_weights(5, 3, (1 << 64) + 7, 2.0),
                          _lib.host_dalex_weights(5, 3, 7, 2.0))


@pytest.mark.parametrize("pressure", [0.0, 0.25, 1.0, 3.0, 20.0, 200.0])
@pytest.mark.parametrize("n_cases, k", [(1, 1), (3, 17), (33, 15), (257, 5)])
def test_the_weights_agree_with_the_restatement(n_cases, k, pressure):
    seed = 0x9E3779B97F4A7C15 ^ (n_cases * 1000 + k)
    got = _lib.host_dalex_weights(n_cases, k, seed, pressure)
    exp = ref.weights(n_cases, k, seed, pressure)
    assert got.shape == (n_cases, k) and got.dtype == np.float64
    assert ref.weights_close(got, exp, pressure), np.abs(got - exp).max()
    assert np.all(np.abs(got.sum(axis=0) - 1.0) <= n_cases * 2.0 ** -53)
    assert np.all(got >= 0.0)
    if pressure == 0.0:
        assert np.all(got == 1.0 / n_cases)
    if pressure == 200.0 and n_cases > 3:
        assert got.max(axis=0).min() > 0.5            # (close to one case each: lexicase-like)


def test_the_weights_under_a_sigma():
    sigma = np.array([2.0, 0.0, 0.5, 1.0, 3.0])
    plain = _lib.host_dalex_weights(5, 9, 11, 1.5)
    got = _lib.host_dalex_weights(5, 9, 11, 1.5, sigma)
    assert np.all(got[1] == 0.0)                      # a constant case
    keep = [0, 2, 3, 4]
    assert np.array_equal(got[keep], plain[keep] / sigma[keep, None])
    assert ref.weights_close(got, ref.weights(5, 9, 11, 1.5, sigma), 1.5)


@pytest.mark.parametrize("n, n_cases", [(1, 1), (2, 3), (15, 5), (130, 33), (600, 7)])
def test_sigma_agrees_with_numpy(n, n_cases):
    E = errors(n, n, n_cases)
    E[:, 0] = 3.5                                     # a constant case
    got = _lib.host_dalex_sigma(E)
    exp = E.std(axis=0)
    assert got[0] == 0.0
    assert np.all(np.abs(got - exp) <= 1e-12 * exp)
    if n > 4:                                         # unfit rows change nothing
        F = np.vstack([E[:2], np.full((1, n_cases), np.inf), E[2:], np.full((1, n_cases), np.nan)])
        F[2, 1:] = 1.0                                # (one bad error is enough)
        assert np.array_equal(_lib.host_dalex_sigma(F), got)


@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("n, n_cases, k, pressure", [
    (1, 1, 15, 1.0), (15, 3, 17, 0.5), (17, 5, 300, 3.0), (130, 33, 300, 3.0),
    (130, 257, 40, 1.0), (200, 33, 300, 20.0)])
def test_the_selection_against_the_restatement(n, n_cases, k, pressure, standardize):
    E = errors(n * 7 + n_cases, n, n_cases)
    seed = 1234567 + n
    out, failed = _lib.host_dalex(E, k, seed, pressure, standardize)
    assert failed == -1 and out.shape == (k,) and out.dtype == np.int32
    sigma = _lib.host_dalex_sigma(E) if standardize else None
    wt = _lib.host_dalex_weights(n_cases, k, seed, pressure, sigma)
    S = ref.scores(E, wt)
    ref.check(out, S, seed, n_cases)
    # ... and the whole restatement (numpy's sigma, math's weights) picks the same
    picks = ref.select(E, k, seed, pressure, standardize)[0]
    ref.check(picks, S, seed, n_cases)
    if pressure >= 3.0 and n >= 17 and n_cases >= 5:
        assert len(set(out.tolist())) > 1             # (the weights differ by selection)


@pytest.mark.parametrize("n_cases", [1, 4, 32, 256])
def test_the_selection_on_exact_data_bit_for_bit(n_cases):
    """pressure = 0, no standardisation, C a power of two: every weight is
    exactly 1 / C and every score of small integers is exact."""
    rng = np.random.default_rng(n_cases)
    E = rng.integers(1, 5, size=(130, n_cases)).astype(np.float64)
    E[7] = E[90] = E[41] = 0.0                        # three winners that tie
    out, failed = _lib.host_dalex(E, 300, 5, 0.0, False)
    wt = _lib.host_dalex_weights(n_cases, 300, 5, 0.0)
    assert np.all(wt == 1.0 / n_cases)
    S = (E.sum(axis=1) / n_cases)[:, None].repeat(300, axis=1)
    assert np.array_equal(S, ref.scores(E, wt))
    assert out.tolist() == [ref.pick(S, 5, s) for s in range(300)]
    assert set(out.tolist()) == {7, 41, 90}


def test_constant_cases_get_weight_zero_and_ties_follow_the_keys():
    E = errors(3, 40, 6)
    E[:, 2] = 1e6                                     # would decide everything
    out, _ = _lib.host_dalex(E, 100, 8, 2.0, True)
    sigma = _lib.host_dalex_sigma(E)
    wt = _lib.host_dalex_weights(6, 100, 8, 2.0, sigma)
    assert sigma[2] == 0.0 and np.all(wt[2] == 0.0)
    S = ref.scores(E, wt)
    assert np.array_equal(S, ref.scores(np.delete(E, 2, axis=1), np.delete(wt, 2, axis=0)))
    ref.check(out, S, 8, 6)
    # every case constant: every score is 0 and the keys pick
    G = np.tile(np.arange(1.0, 6.0), (50, 1))
    out, failed = _lib.host_dalex(G, 200, 9, 1.0, True)
    assert failed == -1
    zero = np.zeros((50, 200))
    assert out.tolist() == [ref.pick(zero, 9, s) for s in range(200)]
    assert len(set(out.tolist())) > 20


def test_identical_rows_are_picked_by_key_and_not_by_position():
    E = np.tile(errors(1, 1, 9), (64, 1))
    for standardize in (True, False):
        out, failed = _lib.host_dalex(E, 64, 2024, 1.5, standardize)
        assert failed == -1
        S = np.zeros((64, 64))                        # (equal scores: any constant)
        assert out.tolist() == [ref.pick(S, 2024, s) for s in range(64)]
        assert len(set(out.tolist())) > 1


def test_unfit_rows_are_never_picked():
    E = errors(5, 60, 7)
    best = E.sum(axis=1).argsort()[:6]
    F = E.copy()
    F[best[0], 3] = np.inf
    F[best[1], 0] = np.nan
    F[best[2], 6] = -np.inf
    out, failed = _lib.host_dalex(F, 300, 77, 1.0, True)
    assert failed == -1 and not set(out.tolist()) & set(best[:3].tolist())
    fit = ref.fit_rows(F)
    assert fit.sum() == 57
    # sigma, and with it every pick, is that of the fit rows alone
    assert np.array_equal(_lib.host_dalex_sigma(F), _lib.host_dalex_sigma(F[fit]))
    S = ref.scores(F, _lib.host_dalex_weights(7, 300, 77, 1.0, _lib.host_dalex_sigma(F)))
    assert np.isnan(S[~fit]).all()
    ref.check(out, S, 77, 7)
    # nobody fit
    F[:, 1] = np.nan
    out, failed = _lib.host_dalex(F, 5, 77, 1.0, True)
    assert out.tolist() == [-1] * 5 and failed == 0
    assert np.all(_lib.host_dalex_sigma(F) == 0.0)


def test_k_zero_and_the_refusals_by_their_words():
    E = errors(0, 4, 3)
    out, failed = _lib.host_dalex(E, 0, 1, 1.0)
    assert out.shape == (0,) and failed == -1
    assert _lib.host_dalex_weights(3, 0, 1, 1.0).shape == (3, 0)
    with pytest.raises(ValueError, match=r"host_dalex: k selections = -1 \(need 0 \.\. 2\^31 - 1\)"):
        _lib.host_dalex(E, -1, 1, 1.0)
    with pytest.raises(ValueError, match=r"host_dalex: n = 0 individuals \(need 1 \.\. 2\^31 - 1\)"):
        _lib.host_dalex(np.zeros((0, 3)), 1, 1, 1.0)
    with pytest.raises(ValueError, match=r"host_dalex: n_cases = 0 \(need 1 \.\. 2\^31 - 1\)"):
        _lib.host_dalex(np.zeros((3, 0)), 1, 1, 1.0)
    with pytest.raises(ValueError, match=r"values must be \[n, n_cases\] \(got 1 dimensions\)"):
        _lib.host_dalex(np.zeros(3), 1, 1, 1.0)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="host_dalex: pressure must be finite and >= 0"):
            _lib.host_dalex(E, 1, 1, bad)
        with pytest.raises(ValueError, match="host_dalex_weights: pressure must be finite and >= 0"):
            _lib.host_dalex_weights(3, 1, 1, bad)
    with pytest.raises(ValueError, match=r"host_dalex_weights: n_cases = 0"):
        _lib.host_dalex_weights(0, 1, 1, 1.0)
    with pytest.raises(ValueError, match=r"sigma must have one entry per case \(3\)"):
        _lib.host_dalex_weights(3, 1, 1, 1.0, np.ones(4))
    # the C twins refuse the same without the Python checks in front
    lib = _lib.load()
    o = np.zeros(4, dtype=np.int32)
    for args in ((None, 4, 3, 1, 1.0, 1, 1), (E, 0, 3, 1, 1.0, 1, 1), (E, 4, 0, 1, 1.0, 1, 1),
                 (E, 4, 3, 1, -1.0, 1, 1), (E, 4, 3, 1, float("nan"), 1, 1),
                 (E, 4, 3, 1, 1.0, 1, -1)):
        v = None if args[0] is None else _lib._ptr(args[0])
        assert lib.gpe_host_dalex(v, *args[1:], _lib._ptr(o), None) == _lib.GPE_E_INVALID
    assert lib.gpe_host_dalex(_lib._ptr(E), 4, 3, 1, 1.0, 1, 1, None, None) == _lib.GPE_E_INVALID


def test_the_drop_in_is_exported_and_returns_nothing_for_k_zero():
    assert "selDALexGPU" in tools.__all__
    assert tools.selDALexGPU([], 0, 1.0) == []
    with pytest.raises(IndexError):
        tools.selDALexGPU([], 3, 1.0)
