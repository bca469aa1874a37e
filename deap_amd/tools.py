"""Population initialisers, selection and bookkeeping used around the GP path.

Behavioural restatement of the parts of the reference's ``deap/tools`` that the
GP examples wire around the evaluation hot path:

* initialisers ``initRepeat``/``initIterate``/``initCycle``
  (reference ``deap/tools/init.py:3-75``);
* selection ``selRandom``/``selBest``/``selWorst``/``selTournament``
  (reference ``deap/tools/selection.py:12-69``) and the lexicase family
  (``:214-320``, fed by per-case fitness from ``SymbRegCaseErrors``) —
  consumers of the fitness the GPU evaluator produces;
* NSGA-II: ``selNSGA2``/``sortNondominated``/``assignCrowdingDist``/
  ``selTournamentDCD`` (reference ``deap/tools/emo.py:15-195``), with
  ``sortNondominatedGPU``/``selNSGA2GPU`` doing the N^2 dominance tests on
  the GPU and returning the same lists;
* ``Statistics``/``MultiStatistics``/``Logbook``/``HallOfFame``/
  ``ParetoFront`` (reference ``deap/tools/support.py:154-641``).
"""
import random
from bisect import bisect_right
from collections import defaultdict
from copy import deepcopy
from functools import partial
from itertools import chain
from operator import attrgetter, eq

__all__ = ["initRepeat", "initIterate", "initCycle", "selRandom", "selBest",
           "selWorst", "selTournament", "selLexicase", "selEpsilonLexicase",
           "selAutomaticEpsilonLexicase", "selLexicaseGPU", "selEpsilonLexicaseGPU", "selDALexGPU",
           "selAutomaticEpsilonLexicaseGPU", "selTournamentGPU",
           "selNSGA2", "sortNondominated", "assignCrowdingDist",
           "selTournamentDCD", "sortNondominatedGPU", "selNSGA2GPU",
           "Statistics", "MultiStatistics",
           "Logbook", "HallOfFame", "ParetoFront", "identity"]


# ----------------------------------------------------------------- init ----
def initRepeat(container, func, n):
    """``container(func() for _ in range(n))`` (reference init.py:3-25)."""
    return container(func() for _ in range(n))


def initIterate(container, generator):
    """``container(generator())`` (reference init.py:27-52)."""
    return container(generator())


def initCycle(container, seq_func, n=1):
    """Cycle through *seq_func* n times (reference init.py:54-75)."""
    return container(f() for _ in range(n) for f in seq_func)


# ------------------------------------------------------------ selection ----
def selRandom(individuals, k):
    return [random.choice(individuals) for _ in range(k)]


def selBest(individuals, k, fit_attr="fitness"):
    return sorted(individuals, key=attrgetter(fit_attr), reverse=True)[:k]


def selWorst(individuals, k, fit_attr="fitness"):
    return sorted(individuals, key=attrgetter(fit_attr))[:k]


def selTournament(individuals, k, tournsize, fit_attr="fitness"):
    """k tournaments of *tournsize* uniformly drawn aspirants; the first best
    aspirant wins each (reference selection.py:51-69)."""
    key = attrgetter(fit_attr)
    return [max(selRandom(individuals, tournsize), key=key)
            for _ in range(k)]


def _lexicase(individuals, k, survive):
    """Shared loop of the lexicase family (reference selection.py:214-320):
    per selection, shuffle the case indices, keep the candidates that
    ``survive(values, case, weight)`` case by case until one candidate or no
    case is left, then draw one candidate.  Same RNG calls, same order."""
    chosen = []
    for _ in range(k):
        weights = individuals[0].fitness.weights
        candidates = individuals
        cases = list(range(len(individuals[0].fitness.values)))
        random.shuffle(cases)
        while cases and len(candidates) > 1:
            c = cases[0]
            vals = [x.fitness.values[c] for x in candidates]
            keep = survive(vals, weights[c] > 0)
            candidates = [x for x, v in zip(candidates, vals) if keep(v)]
            cases.pop(0)
        chosen.append(random.choice(candidates))
    return chosen


def selLexicase(individuals, k):
    """Lexicase selection (reference selection.py:214-244): survivors of
    each case equal its best value."""
    def survive(vals, maximise):
        best = max(vals) if maximise else min(vals)
        return lambda v: v == best
    return _lexicase(individuals, k, survive)


def selEpsilonLexicase(individuals, k, epsilon):
    """epsilon-lexicase (reference selection.py:247-281): survivors are
    within *epsilon* of the best value of the case."""
    def survive(vals, maximise):
        if maximise:
            lim = max(vals) - epsilon
            return lambda v: v >= lim
        lim = min(vals) + epsilon
        return lambda v: v <= lim
    return _lexicase(individuals, k, survive)


def selAutomaticEpsilonLexicase(individuals, k):
    """Automatic epsilon-lexicase (reference selection.py:283-316): epsilon
    is the median absolute deviation of the case's values."""
    import numpy as np

    def survive(vals, maximise):
        med = np.median(vals)
        mad = np.median([abs(v - med) for v in vals])
        if maximise:
            lim = max(vals) - mad
            return lambda v: v >= lim
        lim = min(vals) + mad
        return lambda v: v <= lim
    return _lexicase(individuals, k, survive)


_LEX_CTX = {}


def _lexicase_gpu(individuals, k, mode, epsilon=0.0, device=None,
                  parallel=False):
    """gpe_lexicase: the reference's selection loop on the GPU, drawing from
    the module ``random`` stream exactly as the reference does (its MT19937
    state goes to the device and comes back advanced), so a seeded run
    selects the same individuals and continues with the same stream.

    *parallel*: gpe_lexicase_par instead — the k selections side by side,
    their case orders and picks keyed by one ``random.getrandbits(64)`` (the
    only draw; the rule is in include/gpeval.h).  Reproducible from the seed,
    but not the reference's picks."""
    import numpy as np
    from . import _lib
    from .evaluator import _default_device
    if k == 0:                            # the reference's loop runs 0 times
        return []
    if not individuals:                   # individuals[0] in the reference
        raise IndexError("list index out of range")
    dev = _default_device() if device is None else device
    if dev not in _LEX_CTX:
        _LEX_CTX[dev] = _lib.Context(dev)
    values = np.asarray([ind.fitness.values for ind in individuals],
                        dtype=np.float64)
    maximise = np.asarray(individuals[0].fitness.weights) > 0
    if parallel:
        idx, failed = _LEX_CTX[dev].lexicase_par(
            values, maximise, k, random.getrandbits(64), mode, epsilon)
    else:
        idx, failed = _LEX_CTX[dev].lexicase(values, maximise, k,
                                             random._inst, mode, epsilon)
    if failed >= 0:                       # random.choice([]) in the reference
        raise IndexError("Cannot choose from an empty sequence")
    return [individuals[i] for i in idx.tolist()]


def selLexicaseGPU(individuals, k, device=None, parallel=False):
    """Drop-in for :func:`selLexicase` (reference selection.py:214-244) that
    filters on the GPU; same selections, same ``random`` consumption.
    *parallel* True: the selections run side by side from one drawn seed
    (:func:`_lexicase_gpu`); lexicase selections, but not the same picks."""
    return _lexicase_gpu(individuals, k, 0, device=device, parallel=parallel)


def selEpsilonLexicaseGPU(individuals, k, epsilon, device=None,
                          parallel=False):
    """Drop-in for :func:`selEpsilonLexicase` (selection.py:247-281);
    *parallel* as :func:`selLexicaseGPU`."""
    return _lexicase_gpu(individuals, k, 1, epsilon, device=device,
                         parallel=parallel)


# the device kernel keeps a case's values for the medians in LDS
AUTO_EPSILON_DEVICE_MAX = 16384


def selAutomaticEpsilonLexicaseGPU(individuals, k, device=None,
                                   parallel=False):
    """Drop-in for :func:`selAutomaticEpsilonLexicase`
    (selection.py:283-320).  Above AUTO_EPSILON_DEVICE_MAX individuals the
    selection runs as :func:`selAutomaticEpsilonLexicase` on the host (same
    selections, same ``random`` consumption; selection is not on the
    evaluation path).  *parallel* as :func:`selLexicaseGPU`; that route has
    no such limit and never falls back to the host."""
    if parallel:
        return _lexicase_gpu(individuals, k, 2, device=device, parallel=True)
    if len(individuals) > AUTO_EPSILON_DEVICE_MAX:
        return selAutomaticEpsilonLexicase(individuals, k)
    return _lexicase_gpu(individuals, k, 2, device=device)


def selDALexGPU(individuals, k, pressure, standardize=True, device=None):
    """DALex selection (Ni, Ding and Spector 2024) on the individuals'
    fitness tuples, one fitness value per case: ``gpe_dalex`` on the GPU
    (:meth:`GPUEvaluator.select_dalex` is the same selection straight from
    the resident per-case matrix).  Every selection draws a normal importance
    score per case with standard deviation *pressure*, weights the cases by
    the scores' softmax and picks the individual with the smallest weighted
    error sum; with *standardize* each case is first divided by its standard
    deviation over the population.  The error of a case is the negated
    wvalue: a fitness weight of -1 minimises the value, +1 maximises it.  The
    only draw from ``random`` is one ``getrandbits(64)``; ``k == 0`` returns
    ``[]`` before it.  An individual with a value that is not finite is never
    picked; when nobody is left, ``IndexError`` as ``random.choice([])``."""
    import numpy as np
    from . import _lib
    from .evaluator import _default_device
    if k == 0:
        return []
    if not individuals:
        raise IndexError("list index out of range")
    dev = _default_device() if device is None else device
    if dev not in _LEX_CTX:
        _LEX_CTX[dev] = _lib.Context(dev)
    errors = -np.asarray([ind.fitness.wvalues for ind in individuals],
                         dtype=np.float64)
    idx, failed = _LEX_CTX[dev].dalex(errors, k, random.getrandbits(64),
                                      pressure, standardize)
    if failed >= 0:
        raise IndexError("Cannot choose from an empty sequence")
    return [individuals[i] for i in idx.tolist()]


# round 1's name of selLexicaseGPU, kept for callers written against it
selLexicaseDevice = selLexicaseGPU


def selTournamentGPU(individuals, k, tournsize, fit_attr="fitness",
                     device=None):
    """Drop-in for :func:`selTournament` (reference selection.py:51-69):
    the aspirants' ``random.choice`` draws are replayed on the GPU from the
    module ``random`` state (which comes back advanced), the winners picked
    there by ``Fitness`` order (wvalues); same selections, same stream."""
    import numpy as np
    from . import _lib
    from .evaluator import _default_device
    dev = _default_device() if device is None else device
    if dev not in _LEX_CTX:
        _LEX_CTX[dev] = _lib.Context(dev)
    if not individuals:                   # random.choice([]) in the reference
        if k > 0:
            raise IndexError("Cannot choose from an empty sequence")
        return []
    wv = np.asarray([getattr(ind, fit_attr).wvalues for ind in individuals],
                    dtype=np.float64)
    idx = _LEX_CTX[dev].tournament(wv, k, tournsize, random._inst)
    return [individuals[i] for i in idx.tolist()]


# --------------------------------------------------------------- NSGA-II ----
def _nsga2_cut(fronts, k):
    """All fronts but the last, then the last one's most isolated members
    (descending crowding distance, Python's stable ``sorted``) up to *k*."""
    chosen = [ind for front in fronts[:-1] for ind in front]
    room = k - len(chosen)
    if room > 0:
        by_distance = sorted(fronts[-1], reverse=True,
                             key=attrgetter("fitness.crowding_dist"))
        chosen.extend(by_distance[:room])
    return chosen


def selNSGA2(individuals, k, nd="standard"):
    """NSGA-II selection (reference emo.py:15-50): the non-dominated fronts
    that cover *k* individuals, every front given its crowding distances, the
    last front cut by descending distance.  Draws nothing from ``random``.
    ``nd='log'`` (the reference's ``sortLogNondominated``) is not restated."""
    if nd == "log":
        raise NotImplementedError("selNSGA2: nd='log' is not implemented")
    if nd != "standard":
        raise Exception("selNSGA2: unknown non-dominated sorting method %r" % (nd,))
    fronts = sortNondominated(individuals, k)
    for front in fronts:
        assignCrowdingDist(front)
    return _nsga2_cut(fronts, k)


def sortNondominated(individuals, k, first_front_only=False):
    """Fast non-dominated sorting (reference emo.py:53-117): O(M N^2) calls
    of ``Fitness.dominates`` over the distinct fitnesses, taken in the order
    they first appear; fronts until ``min(len(individuals), k)`` individuals
    are ranked.  Inside a front the fitnesses stand in the order in which
    their last dominator of the previous front, in that front's order,
    released them (front 0: first-appearance order)."""
    if k == 0:
        return []
    members = {}               # fitness -> its individuals, in input order
    for ind in individuals:
        members.setdefault(ind.fitness, []).append(ind)
    fits = list(members)
    n = len(fits)
    dominators = [0] * n                  # how many fitnesses dominate a
    dominated = [[] for _ in range(n)]    # whom a dominates, ascending
    for a in range(n):
        for b in range(a + 1, n):
            if fits[a].dominates(fits[b]):
                dominators[b] += 1
                dominated[a].append(b)
            elif fits[b].dominates(fits[a]):
                dominators[a] += 1
                dominated[b].append(a)

    def expand(front):
        return [ind for a in front for ind in members[fits[a]]]

    front = [a for a in range(n) if dominators[a] == 0]
    fronts = [expand(front)]
    ranked = len(fronts[0])
    if first_front_only:
        return fronts
    target = min(len(individuals), k)
    while ranked < target:
        released = []
        for p in front:
            for d in dominated[p]:
                dominators[d] -= 1
                if dominators[d] == 0:
                    released.append(d)
        front = released
        fronts.append(expand(front))
        ranked += len(fronts[-1])
    return fronts


def assignCrowdingDist(individuals):
    """Set ``fitness.crowding_dist`` on every individual of one front
    (reference emo.py:119-143): per objective, a stable sort of the order the
    previous objective left, ``inf`` for the two ends, ``(next - prev) /
    (nobj * (max - min))`` added for the others; an objective whose ends are
    equal adds nothing."""
    n = len(individuals)
    if n == 0:
        return
    values = [ind.fitness.values for ind in individuals]
    nobj = len(values[0])
    dist = [0.0] * n
    order = list(range(n))
    for j in range(nobj):
        order.sort(key=lambda i: values[i][j])
        low, high = values[order[0]][j], values[order[-1]][j]
        dist[order[0]] = float("inf")
        dist[order[-1]] = float("inf")
        if high == low:
            continue
        norm = nobj * float(high - low)
        for pos in range(1, n - 1):
            dist[order[pos]] += (values[order[pos + 1]][j]
                                 - values[order[pos - 1]][j]) / norm
    for ind, d in zip(individuals, dist):
        ind.fitness.crowding_dist = d


def selTournamentDCD(individuals, k):
    """Dominance / crowding-distance tournaments (reference emo.py:145-195):
    two ``random.sample`` permutations of the individuals, per step of four
    two pairs of each; the dominating one of a pair wins, else the one with
    the larger ``crowding_dist``, else ``random.random() <= 0.5`` picks the
    first."""
    n = len(individuals)
    if k > n:
        raise ValueError("selTournamentDCD: k = %d exceeds the %d individuals"
                         % (k, n))
    if k == n and k % 4 != 0:
        raise ValueError("selTournamentDCD: k == len(individuals) must be a "
                         "multiple of four (got %d)" % k)

    def winner(a, b):
        if a.fitness.dominates(b.fitness):
            return a
        if b.fitness.dominates(a.fitness):
            return b
        da, db = a.fitness.crowding_dist, b.fitness.crowding_dist
        if da < db:
            return b
        if da > db:
            return a
        return a if random.random() <= 0.5 else b

    perms = (random.sample(individuals, n), random.sample(individuals, n))
    chosen = []
    for i in range(0, k, 4):
        for perm in perms:
            chosen.append(winner(perm[i], perm[i + 1]))
            chosen.append(winner(perm[i + 2], perm[i + 3]))
    return chosen


def _nd_fronts_gpu(individuals, k, first_front_only, device):
    """The fronts of :func:`sortNondominatedGPU` and the weighted values
    float64 ``[len(individuals), nobj]`` they were ranked by."""
    import numpy as np
    from . import _lib
    from .evaluator import _default_device
    groups = {}                # wvalues -> members, in first-appearance order
    for i, ind in enumerate(individuals):
        groups.setdefault(ind.fitness.wvalues, []).append(i)
    if not groups:
        return [[]], np.zeros((0, 0))
    w = np.asarray(list(groups.keys()), dtype=np.float64)
    if w.ndim != 2 or np.isnan(w).any():
        raise ValueError("sortNondominatedGPU: a fitness value is nan (or the "
                         "fitnesses differ in length)")
    members = list(groups.values())
    mult = np.asarray([len(g) for g in members], dtype=np.int32)
    dev = _default_device() if device is None else device
    if dev not in _LEX_CTX:
        _LEX_CTX[dev] = _lib.Context(dev)
    rows = _LEX_CTX[dev].nd_sort(w, k, mult, first_front_only)
    fronts = [[i for r in front.tolist() for i in members[r]]
              for front in rows]
    wall = np.empty((len(individuals), w.shape[1]), dtype=np.float64)
    for r, g in enumerate(members):
        wall[g] = w[r]
    return fronts, wall


def sortNondominatedGPU(individuals, k, first_front_only=False, device=None):
    """Drop-in for :func:`sortNondominated` (reference emo.py:53-117) with
    the dominance tests on the GPU (``gpe_nd_sort``; the rule is in
    include/gpeval.h): the same list of fronts, the same order inside each.
    The individuals are grouped by their ``wvalues`` in a dict (``0.0`` and
    ``-0.0`` fall together, as under ``Fitness.__hash__`` / ``__eq__``), the
    distinct rows ranked in one call and expanded again, each group's members
    in input order.  A nan fitness value raises ``ValueError`` (the
    reference's order there depends on its sort's internals)."""
    if k == 0:
        return []
    fronts, _ = _nd_fronts_gpu(individuals, k, first_front_only, device)
    return [[individuals[i] for i in front] for front in fronts]


def _crowding_dist(values):
    """:func:`assignCrowdingDist`'s distances of one front, vectorised:
    *values* float64 ``[n, nobj]`` (``fitness.values``, nan-free) →
    float64 ``[n]`` with the same bits."""
    import numpy as np
    n, nobj = values.shape
    dist = np.zeros(n, dtype=np.float64)
    perm = np.arange(n)
    with np.errstate(all="ignore"):
        for i in range(nobj):
            # the stable sort of the order the previous objective left
            perm = perm[np.argsort(values[perm, i], kind="stable")]
            col = values[perm, i]
            dist[perm[0]] = np.inf
            dist[perm[-1]] = np.inf
            if col[-1] == col[0]:
                continue
            norm = nobj * float(col[-1] - col[0])
            if n > 2:
                dist[perm[1:-1]] += (col[2:] - col[:-2]) / norm
    return dist


def selNSGA2GPU(individuals, k, device=None):
    """Drop-in for :func:`selNSGA2` (reference emo.py:15-50) with the
    non-dominated sorting on the GPU (:func:`sortNondominatedGPU`): the same
    *k* individuals in the same order, the same ``fitness.crowding_dist`` on
    every individual of the fronts it went through.  The crowding distances
    are computed per front on the host in numpy (O(M N log N), off the N^2
    path) and the last front is cut with Python's own stable ``sorted``, so
    ties and nan distances (from infinite values) order as in the reference.
    Nothing is drawn from ``random``; a nan fitness value raises
    ``ValueError``; ``k == 0`` returns ``[]``."""
    import numpy as np
    if k == 0:
        return []
    fronts, wall = _nd_fronts_gpu(individuals, k, False, device)
    if not individuals:
        return []
    with np.errstate(all="ignore"):     # Fitness.values: wvalues / weights
        values = wall / np.asarray(individuals[0].fitness.weights,
                                   dtype=np.float64)
    pareto_fronts = []
    for front in fronts:
        dist = _crowding_dist(values[front]).tolist()
        members = [individuals[i] for i in front]
        for ind, d in zip(members, dist):
            ind.fitness.crowding_dist = d
        pareto_fronts.append(members)
    return _nsga2_cut(pareto_fronts, k)


# -------------------------------------------------------------- support ----
def identity(obj):
    return obj


class Statistics(object):
    """Apply registered reductions to ``key(item)`` over a population
    (reference support.py:154-210)."""

    def __init__(self, key=identity):
        self.key = key
        self.functions = dict()
        self.fields = []

    def register(self, name, function, *args, **kargs):
        self.functions[name] = partial(function, *args, **kargs)
        self.fields.append(name)

    def compile(self, data):
        values = tuple(self.key(elem) for elem in data)
        return {name: fn(values) for name, fn in self.functions.items()}


class MultiStatistics(dict):
    """Named group of :class:`Statistics` (reference support.py:212-259)."""

    def compile(self, data):
        return {name: stats.compile(data) for name, stats in self.items()}

    @property
    def fields(self):
        return sorted(self.keys())

    def register(self, name, function, *args, **kargs):
        for stats in self.values():
            stats.register(name, function, *args, **kargs)


class Logbook(list):
    """Chronological list of record dicts; dict-valued entries become chapters
    (reference support.py:261-488)."""

    def __init__(self):
        self.buffindex = 0
        self.chapters = defaultdict(Logbook)
        self.columns_len = None
        self.header = None
        self.log_header = True

    def record(self, **infos):
        scalars = {k: v for k, v in infos.items() if not isinstance(v, dict)}
        for key, value in list(infos.items()):
            if isinstance(value, dict):
                sub = dict(value)
                sub.update(scalars)
                self.chapters[key].record(**sub)
                del infos[key]
        self.append(infos)

    def select(self, *names):
        if len(names) == 1:
            return [entry.get(names[0], None) for entry in self]
        return tuple([entry.get(n, None) for entry in self] for n in names)

    @property
    def stream(self):
        start, self.buffindex = self.buffindex, len(self)
        return self.__str__(start)

    def __delitem__(self, key):
        if isinstance(key, slice):
            for i in range(*key.indices(len(self))):
                self.pop(i)
                for chapter in self.chapters.values():
                    chapter.pop(i)
        else:
            self.pop(key)
            for chapter in self.chapters.values():
                chapter.pop(key)

    def pop(self, index=0):
        if index < self.buffindex:
            self.buffindex -= 1
        return super(Logbook, self).pop(index)

    def _lines(self, start):
        columns = self.header or (sorted(self[0].keys())
                                  + sorted(self.chapters.keys()))
        if not self.columns_len or len(self.columns_len) != len(columns):
            self.columns_len = [len(c) for c in columns]
        chapter_lines = {}
        offsets = defaultdict(int)
        for name, chapter in self.chapters.items():
            chapter_lines[name] = chapter._lines(start)
            if start == 0:
                offsets[name] = len(chapter_lines[name]) - len(self)
        rows = []
        for i, entry in enumerate(self[start:]):
            row = []
            for j, name in enumerate(columns):
                if name in chapter_lines:
                    cell = chapter_lines[name][i + offsets[name]]
                else:
                    value = entry.get(name, "")
                    cell = ("{0:n}" if isinstance(value, float)
                            else "{0}").format(value)
                self.columns_len[j] = max(self.columns_len[j], len(cell))
                row.append(cell)
            rows.append(row)
        if start == 0 and self.log_header:
            n_head = 1
            if len(self.chapters) > 0:
                n_head += max(len(v) for v in chapter_lines.values()) \
                    - len(self) + 1
            head = [[] for _ in range(n_head)]
            for j, name in enumerate(columns):
                if name in chapter_lines:
                    width = max(len(line.expandtabs())
                                for line in chapter_lines[name])
                    blanks = n_head - 2 - offsets[name]
                    for i in range(blanks):
                        head[i].append(" " * width)
                    head[blanks].append(name.center(width))
                    head[blanks + 1].append("-" * width)
                    for i in range(offsets[name]):
                        head[blanks + 2 + i].append(chapter_lines[name][i])
                else:
                    width = max([len(r[j].expandtabs()) for r in rows]
                                or [len(name)])
                    for line in head[:-1]:
                        line.append(" " * width)
                    head[-1].append(name)
            rows = list(chain(head, rows))
        template = "\t".join("{%d:<%d}" % (i, w)
                             for i, w in enumerate(self.columns_len))
        return [template.format(*row) for row in rows]

    def __str__(self, startindex=0):
        return "\n".join(self._lines(startindex))


class HallOfFame(object):
    """Best-ever individuals, kept sorted; ties keep the older entry first
    (reference support.py:490-589)."""

    def __init__(self, maxsize, similar=eq):
        self.maxsize = maxsize
        self.keys = list()
        self.items = list()
        self.similar = similar

    def update(self, population):
        for ind in population:
            if len(self) == 0 and self.maxsize != 0:
                self.insert(population[0])
                continue
            if ind.fitness > self[-1].fitness or len(self) < self.maxsize:
                if any(self.similar(ind, h) for h in self):
                    continue
                if len(self) >= self.maxsize:
                    self.remove(-1)
                self.insert(ind)

    def insert(self, item):
        item = deepcopy(item)
        i = bisect_right(self.keys, item.fitness)
        self.items.insert(len(self) - i, item)
        self.keys.insert(i, item.fitness)

    def remove(self, index):
        del self.keys[len(self) - (index % len(self) + 1)]
        del self.items[index]

    def clear(self):
        del self.items[:]
        del self.keys[:]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def __iter__(self):
        return iter(self.items)

    def __reversed__(self):
        return reversed(self.items)

    def __str__(self):
        return str(self.items)


class ParetoFront(HallOfFame):
    """Every non-dominated individual that ever lived, sorted
    lexicographically as a :class:`HallOfFame` without a size limit
    (reference support.py:591-641).  A newcomer is scanned against the
    members in order: a member that dominates it ends the scan (unless it has
    already beaten one), members it dominates leave, and a member of equal
    fitness that is ``similar`` makes it a twin, which stays out."""

    def __init__(self, similar=eq):
        HallOfFame.__init__(self, None, similar)

    def update(self, population):
        for ind in population:
            dominated = twin = False
            beaten = []
            for i, member in enumerate(self):
                if not beaten and member.fitness.dominates(ind.fitness):
                    dominated = True
                    break
                if ind.fitness.dominates(member.fitness):
                    beaten.append(i)
                elif ind.fitness == member.fitness and self.similar(ind, member):
                    twin = True
                    break
            for i in reversed(beaten):
                self.remove(i)
            if not (dominated or twin):
                self.insert(ind)
