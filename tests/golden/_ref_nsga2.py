#!/usr/bin/env python3
"""Golden results of the REFERENCE's NSGA-II operators (deap/tools/emo.py:
``sortNondominated`` :53-117, ``assignCrowdingDist`` :119-143, ``selNSGA2``
:15-50, ``selTournamentDCD`` :145-195) and of its ``ParetoFront``
(deap/tools/support.py:591-641) on committed fitness matrices.  The
individuals' ``fitness`` are the reference's own ``base.Fitness`` subclasses,
so dominance, hashing and equality are the reference's.

Per case: the values as hex floats, the weights, ``k``; the fronts of
``sortNondominated(pop, k)`` and of ``first_front_only`` as index lists; after
``selNSGA2(pop, k)`` every assigned ``crowding_dist`` as hex (null where none
was assigned), the selected indices and a ``random.getrandbits(32)`` canary
(selNSGA2 must leave the stream alone); after crowding distances for the whole
population, a seeded ``selTournamentDCD`` with its canary; and the contents of
a ``ParetoFront`` after each of a sequence of updates.

Build container only: ``python3 tests/golden/_ref_nsga2.py`` (needs the 2to3
copy from ``make_oracle_copy.sh``; writes ``nsga2.json.gz``).
"""
import gzip
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_COPY = os.environ.get("DEAP_ORACLE_COPY", "/tmp/deap_oracle")
sys.path.insert(0, ORACLE_COPY)

from deap import base  # noqa: E402  (the reference)
from deap.tools import emo, support  # noqa: E402


class Ind(object):
    def __init__(self, idx, fitness):
        self.idx = idx
        self.fitness = fitness


def population(values, weights):
    fit_cls = type("Fit", (base.Fitness,), {"weights": tuple(weights)})
    pop = []
    for i, row in enumerate(values):
        f = fit_cls()
        f.values = tuple(float(v) for v in row)
        pop.append(Ind(i, f))
    return pop


def same_idx(a, b):
    return a.idx == b.idx


def case(name, values, weights, k, seed):
    values = np.asarray(values, dtype=np.float64)
    n = len(values)
    out = {"name": name,
           "values": [[float(v).hex() for v in row] for row in values],
           "weights": list(weights), "k": k, "seed": seed}
    pop = population(values, weights)
    out["fronts"] = [[ind.idx for ind in front]
                     for front in emo.sortNondominated(pop, k)]
    out["first_front"] = [[ind.idx for ind in front] for front in
                          emo.sortNondominated(pop, k, first_front_only=True)]
    pop = population(values, weights)
    random.seed(seed)
    out["selected"] = [ind.idx for ind in emo.selNSGA2(pop, k)]
    out["canary"] = random.getrandbits(32)
    out["crowding"] = [float(ind.fitness.crowding_dist).hex()
                       if hasattr(ind.fitness, "crowding_dist") else None
                       for ind in pop]
    # selTournamentDCD on crowding distances of the whole population
    pop = population(values, weights)
    emo.selNSGA2(pop, n)
    kd = min(n, max(4, k)) // 4 * 4
    if kd >= 4:
        random.seed(seed + 1)
        out["dcd_k"] = kd
        out["dcd_selected"] = [ind.idx
                               for ind in emo.selTournamentDCD(pop, kd)]
        out["dcd_canary"] = random.getrandbits(32)
    # a ParetoFront through four updates (the first chunk twice)
    pop = population(values, weights)
    third = max(1, n // 3)
    chunks = [pop[:third], pop[third:2 * third], pop[:third], pop[2 * third:]]
    for key, similar in (("pareto_eq", None), ("pareto_idx", same_idx)):
        pf = support.ParetoFront() if similar is None else \
            support.ParetoFront(similar)
        states = []
        for chunk in chunks:
            pf.update(chunk)
            states.append([ind.idx for ind in pf])
        out[key] = states
    return out


def main():
    rng = np.random.default_rng(2002)
    inf = float("inf")
    out = []
    v = np.stack([rng.integers(0, 40, 300) / 8.0,
                  rng.integers(3, 30, 300).astype(float)], axis=1)
    out.append(case("error_size_ties", v, [-1.0, -1.0], 150, 11))
    v = rng.integers(0, 25, size=(200, 1)).astype(float)
    out.append(case("one_objective_ties", v, [1.0], 77, 12))
    v = rng.normal(size=(400, 3))
    out.append(case("three_objectives_mixed_weights", v, [-1.0, 1.0, -0.5],
                    200, 13))
    v = rng.integers(0, 4, size=(500, 4)).astype(float)
    out.append(case("four_objectives_heavy_duplicates", v,
                    [2.0, -1.0, 1.0, -0.5], 250, 14))
    v = rng.integers(0, 12, size=(257, 2)).astype(float)
    out.append(case("k_equals_n", v, [1.0, -1.0], 257, 15))
    out.append(case("k_above_n", v[:90], [1.0, 1.0], 500, 16))
    out.append(case("k_one", v[:64], [-1.0, -1.0], 1, 17))
    v = rng.integers(0, 6, size=(120, 2)).astype(float)
    v[rng.integers(0, 120, 9), rng.integers(0, 2, 9)] = inf
    v[rng.integers(0, 120, 9), rng.integers(0, 2, 9)] = -inf
    out.append(case("infinities", v, [-1.0, 1.0], 60, 18))
    v = rng.integers(-1, 2, size=(60, 2)).astype(float)
    v[::3] *= -1.0          # 0.0 against -0.0
    out.append(case("signed_zeros", v, [1.0, -1.0], 30, 19))
    out.append(case("all_equal", np.full((33, 2), 1.5), [-1.0, -1.0], 10, 20))
    x = np.arange(65, dtype=float)
    out.append(case("one_front", np.stack([x, -x], axis=1), [1.0, 1.0], 40, 21))
    out.append(case("chain", np.stack([x, x], axis=1), [1.0, 1.0], 40, 22))
    out.append(case("single_individual", [[2.0, 3.0]], [-1.0, -1.0], 1, 23))
    v = rng.normal(size=(1500, 2))
    out.append(case("n_1500_continuous", v, [-1.0, -1.0], 750, 24))
    path = os.path.join(HERE, "nsga2.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as gz:
        gz.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, os.path.getsize(path), [c["name"] for c in out])


if __name__ == "__main__":
    main()
