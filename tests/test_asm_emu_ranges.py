"""The exact cores' range-specialised sin/cos handlers (SIN_MID, COS_MID,
SIN_SMALL, COS_SMALL: gen_asm.py glibc_seq4(rng=...)), executed on the CPU
(tests/asm_emu.py) on waves confined to their range, against the host libm
bit for bit.  They run the general handler's operations for a lane of that
range without the range tests, so VRED (the general handler's running max of
|x|.hi) must stay untouched.
"""
import math
import os

import numpy as np
import pytest

import asm_emu

T0855 = 0.85546875                       # glibc's threshold (hx < 0x3feb6000)
LIMIT = {"SMALL": 0.855, "MID": 2.42}    # trig_ranges.h's class bounds
ULP = 2.0 ** -52


def _signs(rng, x):
    return x * np.where(rng.random(len(x)) < 0.5, -1.0, 1.0)


def _waves(rng, rng_name):
    lim = np.nextafter(LIMIT[rng_name], 0.0)        # the largest argument
    out = []
    # uniform fill
    out.append(rng.uniform(-lim, lim, 128))
    out.append(np.full(128, 0.5))
    out.append(np.full(128, -lim))
    # all TAYLOR_SIN lanes (|a| < 0.126), and none
    out.append(rng.uniform(-0.1259, 0.1259, 128))
    out.append(_signs(rng, rng.uniform(0.127, min(lim, 0.85), 128)))
    # chains that differ
    out.append(np.concatenate([rng.uniform(-0.12, 0.12, 64),
                               _signs(rng, rng.uniform(0.2, min(lim, 0.85), 64))]))
    out.append(np.concatenate([_signs(rng, rng.uniform(0.2, min(lim, 0.85), 64)),
                               rng.uniform(-0.12, 0.12, 64)]))
    # +-0, denormals, 2^-26, 2^-27, 0.126 +- ulps, the range's end
    edges = [0.0, 5e-324, 2.2e-308, 1e-310, 2.0 ** -26, 2.0 ** -27, 2.0 ** -28,
             np.nextafter(2.0 ** -26, 0), np.nextafter(2.0 ** -26, 1), lim,
             np.nextafter(lim, 0), 0.78539816339744828, 0.5, 0.25]
    edges += [0.126 * (1 + k * ULP) for k in range(-4, 5)]
    e = np.array(edges)
    x = _signs(rng, e[rng.integers(0, len(e), 128)])
    x[:len(e)] = e
    x[len(e):2 * len(e)] = -e
    out.append(x)
    if rng_name == "MID":
        d_lo, d_hi = T0855, lim
        # one chain all small, one all d (0.85546875 <= |x| < 2.42)
        out.append(np.concatenate([rng.uniform(-0.85, 0.85, 64),
                                   _signs(rng, rng.uniform(d_lo, d_hi, 64))]))
        out.append(np.concatenate([_signs(rng, rng.uniform(d_lo, d_hi, 64)),
                                   rng.uniform(-0.85, 0.85, 64)]))
        out.append(_signs(rng, rng.uniform(d_lo, d_hi, 128)))    # no small lane
        # both sides of 0.85546875 by ulps, pi/2 (y = hp0 - |x| changes sign)
        t = [T0855 * (1 + k * ULP) for k in range(-6, 7)]
        t += [np.nextafter(0.855, 0), 0.855, math.pi / 2,
              np.nextafter(math.pi / 2, 0), np.nextafter(math.pi / 2, 2),
              math.pi / 2 - 0.126, math.pi / 2 + 0.126, math.pi / 2 + 1e-9]
        t = np.array(t)
        x = _signs(rng, t[rng.integers(0, len(t), 128)])
        x[:len(t)] = t
        x[len(t):2 * len(t)] = -t
        out.append(x)
        # everything shuffled
        x = np.concatenate([rng.uniform(-0.12, 0.12, 32), rng.uniform(-0.85, 0.85, 32),
                            _signs(rng, rng.uniform(d_lo, d_hi, 64))])
        rng.shuffle(x)
        out.append(x)
    for _ in range(6):
        out.append(rng.uniform(-lim, lim, 128))
    return out


@pytest.mark.parametrize("suffix", ["_exact", "_exact_deep"])
@pytest.mark.parametrize("which", ["SIN_MID", "COS_MID", "SIN_SMALL", "COS_SMALL"])
def test_range_handler_is_the_host_libm(which, suffix):
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core%s.inc" % suffix)):
        pytest.skip("cores not generated (python -m deap_amd.build)")
    want, rng_name = which.split("_")
    f = math.sin if want == "SIN" else math.cos
    rng = np.random.default_rng(909 + len(which) + 2 * (suffix == "_exact_deep"))
    lines = asm_emu.handler_lines(which, suffix)
    # a body of its own: no branch to the general handler, no |x|.hi
    assert len(lines) > 30 and not any("0x7fffffff" in l for l in lines)
    for x in _waves(rng, rng_name):
        assert np.abs(x).max() < LIMIT[rng_name]
        y, vred = asm_emu.run_handler(which, x, suffix, lines)
        ref = np.array([f(v) for v in x.tolist()])
        bad = y.view(np.uint64) != ref.view(np.uint64)
        assert not bad.any(), (x[bad][:4], y[bad][:4], ref[bad][:4])
        assert not vred.any()


@pytest.mark.parametrize("suffix", ["_exact", "_exact_deep"])
def test_range_handlers_execute_fewer_valu(suffix):
    """The point of the handlers: on the same in-range wave each runs fewer
    VALU instructions than the general one, and no more fp64 ones."""
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core%s.inc" % suffix)):
        pytest.skip("cores not generated (python -m deap_amd.build)")
    rng = np.random.default_rng(3)
    for rng_name, lim in LIMIT.items():
        x = rng.uniform(-lim, lim, 128)
        for want in ("SIN", "COS"):
            g, s = {}, {}
            a, _ = asm_emu.run_handler(want, x, suffix, counts=g)
            b, _ = asm_emu.run_handler("%s_%s" % (want, rng_name), x, suffix, counts=s)
            assert (a.view(np.uint64) == b.view(np.uint64)).all()
            assert s["valu"] < g["valu"] and s["salu"] <= g["salu"], (want, rng_name, g, s)
            assert s["valu_f64"] <= g["valu_f64"] + 2, (want, rng_name, g, s)
            assert s["lds"] == g["lds"]
