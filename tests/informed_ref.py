"""The definition of informed down-sampling in numpy / Python: the oracle of
``gpe_informed_cases`` and its host twin (DEAP has no such operator).

Given ``hit`` bool ``[n, C]``, ``1 <= m <= C`` and a 64-bit ``seed``:
``key[c]`` is the ``(c + 1)``-th output of SplitMix64 seeded with ``seed``; the
cases are totally ordered by ``(key[c], c)``.  ``chosen[0]`` is the smallest
case in that order and ``dist[0] = -1``; ``mind[c]`` is the Hamming distance of
columns ``c`` and ``chosen[0]``.  Step ``t = 1 .. m - 1`` takes, among the cases
not yet chosen, the largest ``mind``, ties to the smallest ``(key, c)``;
``dist[t]`` is its ``mind``; then ``mind = minimum(mind, hamming to it)``."""
import numpy as np

MASK = (1 << 64) - 1


def splitmix_keys(seed, n_cases):
    """``key[c]``, uint64 ``[n_cases]``, in Python ints (mod 2^64)."""
    out = np.zeros(n_cases, dtype=np.uint64)
    for c in range(n_cases):
        z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        out[c] = z ^ (z >> 31)
    return out


def splitmix_keys_np(seed, n_cases):
    """The same keys in wrapping uint64 arithmetic (large case counts)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + \
            np.arange(1, n_cases + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def informed_cases(hit, m, seed):
    """``(chosen int64[m], dist int32[m])`` of the definition above."""
    hit = np.asarray(hit).astype(bool)
    n, n_cases = hit.shape
    assert n >= 1 and 1 <= m <= n_cases
    key = splitmix_keys_np(seed, n_cases)
    # rank[c]: the position of c in the (key, c) order (lexsort: last key first)
    order = np.lexsort((np.arange(n_cases), key))
    rank = np.empty(n_cases, dtype=np.int64)
    rank[order] = np.arange(n_cases)
    cols = np.ascontiguousarray(hit.T, dtype=np.float64)   # [C, n] of 0.0 / 1.0

    def hamming(c):
        # x != p is x + p - 2 x p on 0/1: summed over the individuals, one
        # matrix-vector product (counts below 2^53 are exact in float64)
        p = cols[c]
        return (cols @ (1.0 - 2.0 * p) + p.sum()).astype(np.int64)

    chosen = np.zeros(m, dtype=np.int64)
    dist = np.zeros(m, dtype=np.int32)
    taken = np.zeros(n_cases, dtype=bool)
    first = int(order[0])
    chosen[0], dist[0] = first, -1
    taken[first] = True
    mind = hamming(first)
    for t in range(1, m):
        best = np.where(taken, -1, mind).max()
        cand = np.flatnonzero(~taken & (mind == best))
        c = int(cand[np.argmin(rank[cand])])
        chosen[t], dist[t] = c, best
        taken[c] = True
        mind = np.minimum(mind, hamming(c))
    return chosen, dist


def threshold(cases, eps):
    """The hit matrix of a matrix of absolute errors: finite and ``<= eps``
    (a nan or inf never hits, also with ``eps = inf``)."""
    e = np.asarray(cases, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(e) & (e <= eps)


def matrices(shapes, seed=7):
    """Hit matrices ``[n, C]`` for *shapes* ``(C, n)``: random columns drawn
    from a small pool (duplicated columns), an all-0 and an all-1 column where
    there is room, and per shape a second matrix whose columns are all equal."""
    rng = np.random.default_rng(seed)
    for n_cases, n in shapes:
        pool = rng.integers(0, 2, (n, max(1, n_cases // 3))).astype(bool)
        hit = pool[:, rng.integers(0, pool.shape[1], n_cases)]
        fresh = rng.random(n_cases) < 0.3                  # some columns of their own
        hit[:, fresh] = rng.integers(0, 2, (n, int(fresh.sum()))).astype(bool)
        if n_cases >= 3:
            hit[:, n_cases // 2] = False
            hit[:, n_cases - 1] = True
        yield "mixed", hit
        yield "equal", np.repeat(rng.integers(0, 2, (n, 1)).astype(bool), n_cases, axis=1)
