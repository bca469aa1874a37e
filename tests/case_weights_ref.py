"""The definitions of the case weights in plain Python (``math.fsum``): solve
counts, weighted hits and implicit fitness sharing of a ``bool[n][n_cases]``
hit matrix.  The tests hold the host twins and the GPU to these."""
import math


def solve_counts(H, live=None):
    """s[c]: the live rows that hit case c."""
    n = len(H)
    n_cases = len(H[0]) if n else 0
    return [sum(1 for i in range(n) if (live is None or live[i]) and H[i][c])
            for c in range(n_cases)]


def weighted_hits(H, W):
    """wh[i][g]: fsum of W[g][c] over the cases row i hits."""
    out = []
    for row in H:
        solved = [c for c in range(len(row)) if row[c]]
        out.append([math.fsum(w[c] for c in solved) for w in W])
    return out


def shared_hits(H, live=None):
    """(s, sh): sh[i] is the fsum of 1 / s[c] over the cases row i hits, nan
    for a row that is not live."""
    s = solve_counts(H, live)
    out = []
    for i, row in enumerate(H):
        if live is not None and not live[i]:
            out.append(math.nan)
        else:
            out.append(math.fsum(1.0 / s[c] for c in range(len(row)) if row[c]))
    return s, out
