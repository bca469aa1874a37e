#!/usr/bin/env python3
"""Golden selections of the REFERENCE's ``selLexicase`` on 0/1 fitness
matrices with every case maximised — what ``gpe_lexicase_bits`` replays.

Runs ``selLexicase`` (deap/tools/selection.py:214-244, the 2to3 copy made by
``make_oracle_copy.sh``) on a few seeded 0/1 matrices under fixed
``random.seed``s and records each matrix (one string of 0/1 per row), the
seed, ``k``, the selected indices and ``random.getstate()[1]`` afterwards
(the 624 MT19937 words and the position), which pins every draw.  The
matrices hold duplicated rows, a case nobody passes, a case everybody passes,
a population of one, ``k > n`` and a case count past 624 (one selection's
shuffle crosses a state block).

Build container only: ``python3 tests/golden/_ref_lexicase_bits.py``
(writes ``lexicase_bits.json.gz``).
"""
import gzip
import json
import os
import random
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_COPY = os.environ.get("DEAP_ORACLE_COPY", "/tmp/deap_oracle")
sys.path.insert(0, ORACLE_COPY)

from deap.tools import selection  # noqa: E402  (the reference)


def case(name, bits, k, seed):
    bits = np.asarray(bits, dtype=np.int64)
    n_cases = bits.shape[1]
    pop = [SimpleNamespace(fitness=SimpleNamespace(values=tuple(row.tolist()),
                                                   weights=(1.0,) * n_cases),
                           idx=i) for i, row in enumerate(bits)]
    random.seed(seed)
    got = [ind.idx for ind in selection.selLexicase(pop, k)]
    return {"name": name, "rows": ["".join(map(str, row.tolist())) for row in bits],
            "n_cases": n_cases, "k": k, "seed": seed, "selected": got,
            "state": list(random.getstate()[1])}


def main():
    rng = np.random.default_rng(20261)
    out = []
    base = rng.integers(0, 2, size=(8, 12))
    v = base[rng.integers(0, 8, size=40)]         # mostly duplicated rows
    v[:, 3] = 0                                   # nobody passes
    v[:, 7] = 1                                   # everybody passes
    out.append(case("duplicates_dead_and_full_case_k_over_n", v, 50, 11))
    out.append(case("one_individual", rng.integers(0, 2, size=(1, 5)), 3, 12))
    base = rng.integers(0, 2, size=(30, 70))
    v = base[rng.integers(0, 30, size=130)]       # 3 words of 64 programs
    out.append(case("pop130_cases70", v, 64, 13))
    v = (rng.random(size=(20, 700)) < 0.9).astype(np.int64)
    v[5] = v[4]
    out.append(case("cases700_one_selection_past_624_words", v, 4, 14))
    path = os.path.join(HERE, "lexicase_bits.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, [(c["name"], c["selected"][:5]) for c in out])


if __name__ == "__main__":
    main()
