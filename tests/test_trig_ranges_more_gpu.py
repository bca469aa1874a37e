"""The exact cores' later range-specialised sin/cos handlers (COS_MIDLO,
SIN_WIDE, COS_WIDE, the "bounded or NaN" state, the SMALL bodies without da)
on the GPU: ``GPE_TRIG_RANGES`` = 1 (the handlers before them) and 2 (all,
the default), each in a fresh child process, give hi, lo, err and flags that
are equal in every bit; the classes the device translation picked are the
host pass's and every new class is in use; the programs that run into an inf
raise the reference's ValueError in both.

512 seeded symreg10 trees of depth 2-5 plus hand-written ones, over 1,100
cases (eight full 128-case tiles and a partial one) and over 129.  Ten columns
of five kinds, two each: U(-1, 1), U(0.9, 1.4), U(-3, 3), U(0, 0.1) and
U(-1, 1) holding one inf.

Run as a script (the child): ``python test_trig_ranges_more_gpu.py N_CASES
LEAVES OUT.npz`` evaluates the same population under the environment's
``GPE_TRIG_RANGES`` and stores the raw outputs.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path.insert(0, REPO)

from deap_amd import _lib, configs, gp                    # noqa: E402

pytestmark = pytest.mark.gpu
NV = 10
KINDS = [(-1.0, 1.0), (0.9, 1.4), (-3.0, 3.0), (0.0, 0.1), None] * 2
INF_PROGRAMS = [
    "cos(sin(mul(mul(protectedDiv(ARG0, ARG3), 1e300), 1e300)))",
    "sin(cos(mul(mul(protectedDiv(ARG1, ARG8), 1e300), 1e300)))",
    "cos(mul(ARG2, sin(mul(mul(protectedDiv(1.0, ARG3), 1e300), 1e300))))",
    "cos(sin(ARG4))", "sin(cos(ARG9))", "cos(mul(0.5, sin(add(ARG4, ARG0))))",
    "cos(protectedDiv(sin(ARG4), add(ARG1, 2.0)))",
]
HAND = INF_PROGRAMS + [
    "cos(ARG0)", "cos(ARG1)", "cos(ARG6)", "cos(mul(ARG0, ARG5))", "cos(add(ARG0, ARG5))",
    "cos(ARG3)", "sin(ARG3)", "sin(ARG8)", "cos(mul(ARG3, ARG8))", "sin(ARG1)",
    "sin(ARG2)", "cos(ARG2)", "sin(mul(ARG2, ARG7))", "cos(mul(mul(ARG2, ARG7), ARG2))",
    "sin(mul(1e6, ARG0))", "cos(mul(1e7, ARG2))", "sin(mul(1e9, ARG0))",
    "cos(sub(ARG1, ARG6))", "cos(neg(ARG1))", "sin(cos(protectedDiv(ARG0, ARG3)))",
    "cos(sin(protectedDiv(ARG0, ARG2)))", "cos(cos(protectedDiv(ARG1, ARG0)))",
    "sin(sin(sin(protectedDiv(ARG2, ARG0))))", "cos(add(ARG1, sin(protectedDiv(1.0, ARG5))))",
    "add(cos(ARG3), cos(mul(ARG1, ARG1)))", "sub(sin(mul(ARG2, 30.0)), cos(ARG6))",
]


def population():
    pset = configs.pset_for("symreg10")
    pop = [gp.PrimitiveTree.from_string(s, pset) for s in HAND]
    return pset, pop + configs.population(pset, "half", 512, 1440, 2, 5)


def data(n_cases):
    rng = np.random.default_rng(n_cases)
    X = np.array([rng.uniform(*(k or (-1.0, 1.0)), size=n_cases) for k in KINDS])
    X[4, n_cases - 3] = math.inf                # (1,100: in the partial last tile)
    X[9, 5] = -math.inf
    Y = rng.uniform(-2, 2, size=(1, n_cases))
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def column_bounds(X, leaves):
    """gpe_set_cases' bounds: [min, max] hulled with 0.0, unbounded for a
    column with a nan or an inf; the trig leaves' columns [-1, 1]."""
    ok = [bool(np.isfinite(col).all()) for col in X]
    lo = [min(col.min(), 0.0) if f else -math.inf for col, f in zip(X, ok)]
    hi = [max(col.max(), 0.0) if f else math.inf for col, f in zip(X, ok)]
    if leaves:
        lo += 2 * [-1.0 if f else -math.inf for f in ok]
        hi += 2 * [1.0 if f else math.inf for f in ok]
    return np.array(lo), np.array(hi)


def child(n_cases, leaves, out):
    from deap_amd.evaluator import GPUEvaluator, SymbRegMSE
    pset, pop = population()
    X, Y = data(n_cases)
    ev = GPUEvaluator(pset, SymbRegMSE(X, Y), device=0, trig_leaves=leaves)
    raw = {}
    inner = ev.run_batch

    def spy(batch, *a, **k):
        k["want"] = None                        # every output, copied back
        r = inner(batch, *a, **k)
        raw["out"] = [np.array(v, copy=True) for v in r[:4]]
        return r
    ev.run_batch = spy
    try:
        got = ev.evaluate(pop)
        base = ev.ctx.trig_classes()
        picked = ev.ctx.trig_classes(picked=True)
        geo = ev.ctx.geometry()
        batch = ev.flattener.flatten(pop)
    finally:
        ev.ctx.close()
    fit = [type(r).__name__ if isinstance(r, BaseException) else float(r[0]).hex()
           for r in got]
    # the host pass over the words this evaluator loaded and the same columns
    lo, hi = column_bounds(X, leaves)
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    host1, host2 = np.zeros(3, dtype=np.int64), np.zeros(5, dtype=np.int64)
    for i in range(len(pop)):
        if batch.err[i]:
            continue
        w = code[off[i]:off[i + 1]]
        host1 += np.bincount(_lib.debug_trig_classes(w, lo, hi), minlength=3)
        host2 += np.bincount(_lib.debug_trig_classes(w, lo, hi, mode=2), minlength=5)
    meta = {"fit": fit, "base": base, "picked": picked, "asm": int(geo["asm"]),
            "valid": int(sum(1 for e in batch.err if not e)),
            "host1": host1.tolist(), "host2": host2.tolist()}
    np.savez(out, hi=raw["out"][0], lo=raw["out"][1], err=raw["out"][2],
             flags=raw["out"][3], meta=np.array(json.dumps(meta)))


def run_child(tmp_path, n_cases, leaves, mode):
    out = str(tmp_path / ("mode%s_%d.npz" % (mode, n_cases)))
    env = dict(os.environ, GPE_TRIG_RANGES=str(mode))
    env["PYTHONPATH"] = os.pathsep.join([REPO, HERE] + env.get("PYTHONPATH", "").split(os.pathsep))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), str(n_cases),
                                                  str(int(leaves)), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (mode, p.stdout[-2000:], p.stderr[-2000:])
    z = np.load(out)
    return {k: z[k] for k in ("hi", "lo", "err", "flags")}, json.loads(str(z["meta"]))


_REF = {}


def hand_reference(n_cases):
    """The reference's fitness of the hand-written programs (the seeded trees
    are compared between the modes only)."""
    if n_cases not in _REF:
        from test_launch_geometry import Values, mse_reference
        pset, pop = population()
        X, Y = data(n_cases)
        _REF[n_cases] = mse_reference(Values(pset, pop[:len(HAND)], X), Y, n_cases)
    return _REF[n_cases]


@pytest.mark.parametrize("n_cases,leaves", [(1100, False), (1100, True), (129, False)],
                         ids=["1100-inline", "1100-trig_leaves", "129-inline"])
def test_modes_1_and_2_agree_bit_for_bit(tmp_path, n_cases, leaves):
    from test_launch_geometry import check_mse
    pset, pop = population()
    raw1, m1 = run_child(tmp_path, n_cases, leaves, 1)
    raw2, m2 = run_child(tmp_path, n_cases, leaves, 2)
    host1, host2 = m2["host1"], m2["host2"]
    assert (host1, host2) == (m1["host1"], m1["host2"]) and sum(host1) == sum(host2) > 500
    print("TRIGCLS2|gpu n_cases=%d leaves=%d|mode1=%s mode2=%s host1=%s host2=%s"
          % (n_cases, leaves, m1["picked"], m2["picked"], host1, host2))
    # every valid program ran on an exact core, in both modes
    assert m1["asm"] == m1["valid"] == m2["asm"] == m2["valid"] > 500
    # the classes: the base ones in both modes, the picked ones per mode
    for m in (m1, m2):
        assert [m["base"][k] for k in _lib.TRIG_CLASSES] == host1
    assert [m1["picked"][k] for k in _lib.TRIG_PICKED] == host1 + [0, 0]
    assert [m2["picked"][k] for k in _lib.TRIG_PICKED] == host2
    assert all(m2["picked"][k] > 0 for k in _lib.TRIG_PICKED), m2["picked"]
    assert m2["picked"]["general"] < m1["picked"]["general"]
    # hi, lo, err, flags: the same bits, program for program
    for name in ("hi", "lo", "err", "flags"):
        a, b = np.ascontiguousarray(raw1[name]), np.ascontiguousarray(raw2[name])
        assert a.dtype == b.dtype and a.shape == b.shape == (len(pop),)
        same = a.view(np.uint8).reshape(len(pop), -1) == b.view(np.uint8).reshape(len(pop), -1)
        bad = np.flatnonzero(~same.all(axis=1))
        assert len(bad) == 0, (name, [(int(i), str(pop[i])[:100]) for i in bad[:3]])
    assert m1["fit"] == m2["fit"]
    # the inf programs raise the reference's ValueError, the other
    # hand-written ones give its value (1e-12)
    assert m2["fit"][:len(INF_PROGRAMS)] == ["ValueError"] * len(INF_PROGRAMS)
    got = [ValueError() if f == "ValueError" else OverflowError() if f == "OverflowError"
           else (float.fromhex(f),) for f in m2["fit"][:len(HAND)]]
    check_mse(pop[:len(HAND)], got, hand_reference(n_cases), ("modes", n_cases))


if __name__ == "__main__":
    child(int(sys.argv[1]), bool(int(sys.argv[2])), sys.argv[3])
