"""The rule of ``gpe_lexicase_par`` (include/gpeval.h) restated in plain
Python / numpy, as the tests' reference: SplitMix64 keys in Python ints, the
filter as the ``survive`` functions of ``deap_amd.tools._lexicase`` with
``numpy.median``, the choice as ``(K * count) >> 64``."""
import numpy as np

M64 = (1 << 64) - 1


def key(seed, i):
    """K(i): the (i + 1)-th output of SplitMix64 seeded with *seed*."""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def survive_plain(vals, maximise):
    best = max(vals) if maximise else min(vals)
    return lambda v: v == best


def survive_epsilon(epsilon):
    def survive(vals, maximise):
        if maximise:
            lim = max(vals) - epsilon
            return lambda v: v >= lim
        lim = min(vals) + epsilon
        return lambda v: v <= lim
    return survive


def survive_automatic(vals, maximise):
    with np.errstate(invalid="ignore"):
        med = np.median(vals)
        mad = np.median([abs(v - med) for v in vals])
    if maximise:
        lim = max(vals) - mad
        return lambda v: v >= lim
    lim = min(vals) + mad
    return lambda v: v <= lim


def lexicase_par(values, maximise, k, seed, mode=0, epsilon=0.0):
    """``(out int32[k], failed)`` of the rule on ``values`` [n, C]."""
    values = np.asarray(values, dtype=np.float64)
    n, C = values.shape
    rows = values.tolist()                    # Python floats, as fitness.values
    survive = (survive_plain, survive_epsilon(epsilon), survive_automatic)[mode]
    seed &= M64
    out = np.zeros(k, dtype=np.int32)
    failed = -1
    for s in range(k):
        i0 = s * (C + 1)
        cases = sorted(range(C), key=lambda c: (key(seed, i0 + c), c))
        candidates = list(range(n))
        while cases and len(candidates) > 1:
            c = cases.pop(0)
            vals = [rows[i][c] for i in candidates]
            keep = survive(vals, bool(maximise[c]))
            candidates = [i for i, v in zip(candidates, vals) if keep(v)]
        if not candidates:
            out[s] = -1
            if failed < 0:
                failed = s
            continue
        out[s] = candidates[(key(seed, i0 + C) * len(candidates)) >> 64]
    return out, failed


def matrices(n, C, seed=0):
    """The test matrices [n, C] by name: continuous values, a 4-level
    alphabet (heavy ties), a population of clones (every selection ends with
    count = n) and ties with nan / +-inf entries, a nan in row 0 among them
    (selections that meet it as the best value fail)."""
    rng = np.random.default_rng([seed, n, C])
    ties = rng.integers(0, 4, (n, C)).astype(np.float64)
    bad = ties.copy()
    m = rng.random((n, C))
    bad[m < 0.08] = np.nan
    bad[(m >= 0.08) & (m < 0.14)] = np.inf
    bad[(m >= 0.14) & (m < 0.20)] = -np.inf
    bad[0, 0] = np.nan
    return {"random": rng.normal(size=(n, C)),
            "ties": ties,
            "clones": np.tile(rng.integers(0, 4, (1, C)).astype(np.float64), (n, 1)),
            "nan": bad}


def maximise_settings(C):
    mixed = (np.arange(C) % 3 == 1).astype(np.uint8)
    return {"min": np.zeros(C, dtype=np.uint8), "max": np.ones(C, dtype=np.uint8),
            "mixed": mixed}
