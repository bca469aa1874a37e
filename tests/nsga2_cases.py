"""Shared by test_nsga2.py and test_nsga2_gpu.py: the golden cases of
``tests/golden/nsga2.json.gz`` (the reference's NSGA-II operators, written by
``tests/golden/_ref_nsga2.py``) as populations of this project's ``Fitness``,
and small helpers to compare results by identity and by bits."""
import numpy as np

from conftest import load_golden
from deap_amd import base

_GOLDEN = []


def golden_cases():
    if not _GOLDEN:
        _GOLDEN.extend(load_golden("nsga2"))
    return _GOLDEN


def case_names():
    return [c["name"] for c in golden_cases()]


def case_by_name(name):
    return next(c for c in golden_cases() if c["name"] == name)


class Ind(object):
    def __init__(self, idx, fitness):
        self.idx = idx
        self.fitness = fitness

    def __repr__(self):
        return "Ind(%d)" % self.idx


def population(values, weights):
    """One individual per row of *values* (fitness.values), in order."""
    fit_cls = type("Fit", (base.Fitness,), {"weights": tuple(weights)})
    pop = []
    for i, row in enumerate(values):
        f = fit_cls()
        f.values = tuple(float(v) for v in row)
        pop.append(Ind(i, f))
    return pop


def case_population(case):
    values = [[float.fromhex(v) for v in row] for row in case["values"]]
    return population(values, case["weights"])


def idx_fronts(fronts):
    return [[ind.idx for ind in front] for front in fronts]


def crowding_hex(pop):
    return [float(ind.fitness.crowding_dist).hex()
            if hasattr(ind.fitness, "crowding_dist") else None for ind in pop]


def fronts_as_lists(rows):
    return [np.asarray(f).tolist() for f in rows]


def random_problem(rng, n_max=90):
    """A small problem on an integer grid, so that ties and duplicates abound:
    ``(wvalues float64[n, m], weights, k)``."""
    n = int(rng.integers(1, n_max + 1))
    m = int(rng.integers(1, 5))
    weights = rng.choice([-1.0, 1.0, -0.5, 2.0], size=m)
    values = rng.integers(0, int(rng.integers(2, 7)), size=(n, m)).astype(float)
    k = int(rng.integers(1, n + 3))
    return values, weights.tolist(), k
