"""The DALex rule of include/gpeval.h restated in pure Python (``math.log``,
``math.cos``, ``math.exp``, ``math.fsum``), and the criteria the tests hold a
selection to.  Nothing here calls the library."""
import math

import numpy as np

M64 = (1 << 64) - 1
TIE_SALT = 0xD1B54A32D192ED03
U = 2.0 ** -53


def key(seed, i):
    """K(i): the (i + 1)-th output of SplitMix64 seeded with *seed*."""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def importance(seed, j, pressure):
    u1 = float((key(seed, (2 * j) & M64) >> 11) + 1) * U
    u2 = float(key(seed, (2 * j + 1) & M64) >> 11) * U
    z = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
    return pressure * z


def weights(n_cases, k, seed, pressure, sigma=None):
    """Steps 1, 2 and 4 → ``float64[n_cases, k]`` (case-major)."""
    out = np.zeros((n_cases, k), dtype=np.float64)
    for s in range(k):
        imp = [importance(seed, s * n_cases + c, pressure) for c in range(n_cases)]
        m = max(imp)
        x = [math.exp(v - m) for v in imp]
        t = 0.0
        for v in x:                                   # ascending c, fp64
            t += v
        for c in range(n_cases):
            w = x[c] / t
            if sigma is not None:
                w = 0.0 if sigma[c] == 0.0 else w / sigma[c]
            out[c, s] = w
    return out


def weight_bound(pressure):
    """The relative bound of the issue between two faithful evaluations of
    steps 1 - 2: 16 * 2^-53 * (1 + 8.6 pressure); |I| <= 8.6 pressure because
    |z| <= sqrt(2 * 53 * ln 2)."""
    return 16.0 * U * (1.0 + 8.6 * pressure)


def weights_close(a, b, pressure):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= weight_bound(pressure) * np.abs(b) + 1e-300))


def fit_rows(E):
    return np.isfinite(np.asarray(E)).all(axis=1)


def gamma(n_cases):
    g = (n_cases + 1) * U
    return g / (1.0 - g)


def scores(E, wt):
    """``S_ref[i, s]`` by math.fsum of w'[c, s] * e[i, c] (each product rounded
    to fp64); nan for an unfit row."""
    E = np.asarray(E, dtype=np.float64)
    n, C = E.shape
    fit = fit_rows(E)
    out = np.full((n, wt.shape[1]), np.nan)
    cols = [wt[:, s].tolist() for s in range(wt.shape[1])]
    for i in np.flatnonzero(fit):
        row = E[i].tolist()
        for s, w in enumerate(cols):
            out[i, s] = math.fsum(w[c] * row[c] for c in range(C))
    return out


def tie_less(seed, n, s, a, b):
    ka = key(seed ^ TIE_SALT, (s * n + a) & M64)
    kb = key(seed ^ TIE_SALT, (s * n + b) & M64)
    return (ka, a) < (kb, b)


def pick(S, seed, s):
    """The rule's pick of selection s from exact scores S[:, s]: the smallest
    (S, K2(s n + i), i) over the fit rows; -1 with none."""
    n = S.shape[0]
    best = -1
    for i in range(n):
        v = S[i, s]
        if v != v:
            continue
        if best < 0 or v < S[best, s] or (v == S[best, s] and tie_less(seed, n, s, i, best)):
            best = i
    return best


def select(E, k, seed, pressure, standardize=True):
    """The whole rule with fsum scores and numpy's sigma → (picks, S, wt)."""
    E = np.asarray(E, dtype=np.float64)
    fit = fit_rows(E)
    sigma = None
    if standardize:
        sigma = E[fit].std(axis=0) if fit.any() else np.zeros(E.shape[1])
    wt = weights(E.shape[1], k, seed, pressure, sigma)
    S = scores(E, wt)
    return [pick(S, seed, s) for s in range(k)], S, wt


def check(picks, S, seed, n_cases, min_decided=0.99):
    """The gap criterion on reference scores S[n, k] (``scores``): every pick p
    has S[p] <= min S * (1 + 2 gamma), which any summation order of
    non-negative terms stays inside; where the reference's runner-up lies
    outside that margin, p is the reference's argmin.  Such decided selections
    must be at least *min_decided* of all: a condition on the inputs, asserted
    on the reference alone.  Returns their number."""
    g = gamma(n_cases)
    n, k = S.shape
    decided = 0
    for s in range(k):
        col = S[:, s]
        live = np.flatnonzero(col == col)
        p = int(picks[s])
        if len(live) == 0:
            assert p == -1, (s, p)
            decided += 1
            continue
        lo = col[live].min()
        lim = lo * (1.0 + 2.0 * g)
        assert p >= 0 and col[p] == col[p] and col[p] <= lim, (s, p, col[p], lo)
        near = [int(i) for i in live if col[i] <= lim]
        if len(near) == 1:
            decided += 1
            assert p == near[0], (s, p, near[0])
    assert decided >= min_decided * k, (decided, k)
    return decided
