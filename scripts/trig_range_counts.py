#!/usr/bin/env python3
"""Executed instructions per sin/cos call of the exact cores' handlers, with
and without the range-specialised ones, on headline trees and their own
arguments (tests/asm_emu.py on the CPU; no GPU).

The first ``trees`` trees of the headline population (bench.py's seed and
depths) are flattened; the range pass (csrc/trig_ranges.h, through
gpe_debug_trig_picks) classifies every sin/cos node from the columns' bounds
[-1, 1]; the words are evaluated on the first ``tiles`` 128-case tiles of the
headline cases, and every sin/cos call's 128 arguments (chain k = cases
64k .. 64k + 63) run through the general handler and through the handler of
the node's class, three times: with the base classes (GPE_TRIG_RANGES=1),
with all of them (2), and with the static-role MID / MIDLO bodies (3, the
default).  Prints, per mode and handler, the executed VALU (of them fp64),
SALU and LDS instructions per wave-call, the class shares, and the weighted
per-call totals of the specialised mix against the general handler alone,
then the per-call totals of modes 1 -> 2 and 2 -> 3 side by side.  Every
result is checked bit for bit against the host libm, and every argument
against its class's range.

Usage: python scripts/trig_range_counts.py [trees=192] [tiles=2]
"""
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(1, REPO)

import asm_emu                                   # noqa: E402
from deap_amd import _lib, configs              # noqa: E402
from deap_amd.flatten import Flattener, Op       # noqa: E402

CLASS = ("general", "mid", "small", "midlo", "wide")
LIMIT = (math.inf, 2.42, 0.855, 1.44, 1e8)


def handler(kind, c, mode=2):
    """The handler of a node's class (modes 1 and 2: midlo is a cos class, a
    sin node never gets it; mode 3: sin too, and mid and midlo are the bodies
    with static lane roles)."""
    assert mode == 3 or not (kind == "sin" and c == 3)
    return kind.upper() if c == 0 else "%s_%s%s" % (
        kind.upper(), CLASS[c].upper(), "3" if mode == 3 and c in (1, 3) else "")


def handlers(mode):
    """Every handler a node can get in `mode` (mode 1 picks a subset of mode
    2's: the list is mode 2's there, the unused ones print no row)."""
    return sorted({handler(k, c, mode) for k in ("sin", "cos") for c in range(5)
                   if mode == 3 or not (k == "sin" and c == 3)})


def f64(lo, hi):
    return np.array([int(lo) | (int(hi) << 32)], dtype=np.uint64).view(np.float64)[0]


def pdiv(num, den):
    z = den == 0.0
    return np.where(z, 1.0, num / np.where(z, 1.0, den))


def trig_calls(words, X):
    """(kind, arguments per case) of every sin/cos word, in word order."""
    n = X.shape[1]
    T, R, out, pc = np.zeros(n), {}, [], 0
    with np.errstate(all="ignore"):
        while True:
            w = int(words[pc])
            pc += 1
            op, d, x = w & 0xff, (w >> 8) & 0xff, w >> 16
            if op == Op.END:
                return out
            form = (op - Op.ADD) % 3 if Op.ADD <= op < Op.NEG else -1
            c = None
            if op in (Op.LDC, Op.PUSHC) or form == 2:
                c = f64(words[pc], words[pc + 1])
                pc += 2
            if op in (Op.PUSH, Op.PUSHV, Op.PUSHC):
                R[d] = T
            if op in (Op.LDV, Op.PUSHV):
                T = X[x].copy()
            elif op in (Op.LDC, Op.PUSHC):
                T = np.full(n, c)
            elif op == Op.NEG:
                T = -T
            elif op in (Op.SIN, Op.COS):
                out.append(("sin" if op == Op.SIN else "cos", T.copy()))
                fn = math.sin if op == Op.SIN else math.cos
                T = np.array([fn(v) if math.isfinite(v) else math.nan for v in T.tolist()])
            elif form >= 0:
                a = R[d] if form == 0 else X[x] if form == 1 else np.full(n, c)
                fam = (op - Op.ADD) // 3        # add sub rsub mul div rdiv
                T = [a + T, a - T, T - a, a * T, pdiv(a, T), pdiv(T, a)][fam] \
                    if fam < 6 else None
                assert T is not None, "an op outside the symreg10 set"
            elif op != Op.PUSH:
                raise ValueError(op)


def count_mode(mode, n_trees, tiles, code, off, pop, calls_of, lo, hi, lines):
    """One GPE_TRIG_RANGES mode on the same calls: prints its table, returns
    (results that are not the host libm's, weighted totals per call)."""
    names = handlers(mode)
    spec = {h: {} for h in names}                # the node's class handler
    gen = {h: {} for h in names}                 # the general one, same calls
    calls = {h: 0 for h in names}
    bad = nan_calls = 0
    for i in range(n_trees):
        w = code[off[i]:off[i + 1]]
        cls = _lib.debug_trig_picks(w, lo, hi, mode=mode)
        got = calls_of[i]
        assert len(cls) == len(got)
        for c, (kind, arg) in zip(cls.tolist(), got):
            h = handler(kind, c, mode)
            f = math.sin if kind == "sin" else math.cos
            for t in range(tiles):
                x = np.ascontiguousarray(arg[t * 128:(t + 1) * 128])
                fin = np.isfinite(x)
                if not fin.all():
                    # general, or (mode 2) a NaN lane of a "bounded or NaN"
                    # value in mid / small / midlo: never an inf, never wide
                    assert c == 0 or (mode >= 2 and c in (1, 2, 3) and not np.isinf(x).any())
                    if c == 0:
                        continue
                    nan_calls += 1
                assert np.abs(x[fin]).max(initial=0.0) < LIMIT[c], (str(pop[i]), CLASS[c])
                ref = np.array([f(v) if math.isfinite(v) else math.nan
                                for v in x.tolist()]).view(np.uint64)
                y, _ = asm_emu.run_handler(h, x, lines=lines[h], counts=spec[h])
                bad += int((y.view(np.uint64)[fin] != ref[fin]).sum() + (~np.isnan(y[~fin])).sum())
                g = handler(kind, 0)
                if c:
                    y, _ = asm_emu.run_handler(g, x, lines=lines[g], counts=gen[h])
                    bad += int((y.view(np.uint64)[fin] != ref[fin]).sum())
                calls[h] += 1
    total = sum(calls.values())
    print("GPE_TRIG_RANGES=%d: %d trees, %d tiles: %d sin/cos wave-calls (%d with NaN lanes "
          "in a specialised handler); results not the host libm's: %d"
          % (mode, n_trees, tiles, total, nan_calls, bad))
    print("| handler | share of calls | VALU | of them fp64 | SALU | LDS | "
          "general handler on the same calls: VALU / fp64 / SALU |")
    print("|---|---|---|---|---|---|---|")
    tot_s = {"valu": 0, "valu_f64": 0, "salu": 0, "lds": 0}
    tot_g = dict(tot_s)
    for h in sorted(calls, key=lambda s: (s[4:] or "0", s)):
        n = calls[h]
        if not n:
            continue
        s = spec[h]
        g = gen[h] if "_" in h else s
        for k in tot_s:
            tot_s[k] += s.get(k, 0)
            tot_g[k] += g.get(k, 0)
        print("| %s | %.1f %% | %.1f | %.1f | %.1f | %.1f | %s |"
              % (h, 100.0 * n / total, s.get("valu", 0) / n, s.get("valu_f64", 0) / n,
                 s.get("salu", 0) / n, s.get("lds", 0) / n,
                 "—" if "_" not in h else "%.1f / %.1f / %.1f"
                 % (g.get("valu", 0) / n, g.get("valu_f64", 0) / n, g.get("salu", 0) / n)))
    print("| weighted, specialised mix | 100 %% | %.1f | %.1f | %.1f | %.1f | "
          "%.1f / %.1f / %.1f |"
          % (tot_s["valu"] / total, tot_s["valu_f64"] / total, tot_s["salu"] / total,
             tot_s["lds"] / total, tot_g["valu"] / total, tot_g["valu_f64"] / total,
             tot_g["salu"] / total))
    print("VALU per average call: %.1f -> %.1f (%.1f %% fewer); SALU %.1f -> %.1f"
          % (tot_g["valu"] / total, tot_s["valu"] / total,
             100.0 * (1 - tot_s["valu"] / tot_g["valu"]),
             tot_g["salu"] / total, tot_s["salu"] / total))
    return bad, {k: v / total for k, v in tot_s.items()}


def main():
    n_trees = int(sys.argv[1]) if len(sys.argv) > 1 else 192
    tiles = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    pset = configs.pset_for("symreg10")
    pop = configs.population(pset, "half", n_trees, 2024, 4, 8)
    batch = Flattener(pset).flatten(pop)
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    X = np.ascontiguousarray(np.random.default_rng(2024).uniform(
        -1.0, 1.0, size=(tiles * 128, 10)).T)
    lo, hi = -np.ones(10), np.ones(10)
    calls_of = [trig_calls(code[off[i]:off[i + 1]], X) for i in range(n_trees)]
    lines = {h: asm_emu.handler_lines(h) for mode in (1, 2, 3) for h in handlers(mode)}
    bad = 0
    per_call = {}
    for mode in (1, 2, 3):
        b, per_call[mode] = count_mode(mode, n_trees, tiles, code, off, pop, calls_of,
                                       lo, hi, lines)
        bad += b
        print()
    for a, b in ((1, 2), (2, 3)):
        print("per average call, GPE_TRIG_RANGES=%d -> %d: VALU %.2f -> %.2f, fp64 %.2f -> "
              "%.2f, SALU %.2f -> %.2f"
              % (a, b, per_call[a]["valu"], per_call[b]["valu"], per_call[a]["valu_f64"],
                 per_call[b]["valu_f64"], per_call[a]["salu"], per_call[b]["salu"]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
