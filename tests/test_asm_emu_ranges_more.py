"""The exact cores' further range-specialised sin/cos handlers (COS_MIDLO,
SIN_WIDE, COS_WIDE, and the SMALL bodies without their da terms: gen_asm.py
glibc_seq4(rng=...)), executed on the CPU (tests/asm_emu.py) against the host
libm bit for bit, and the specialised handlers fed NaN lanes (the range
pass's "nanable" state, trig_ranges.h): every table address stays inside the
glibc table block, EXEC is restored and the lane comes out NaN.
"""
import math
import os

import numpy as np
import pytest

import asm_emu

T0855 = 0.85546875                       # glibc's threshold (hx < 0x3feb6000)
T2426 = float(np.array([0x400368fd << 32], dtype=np.uint64).view(np.float64)[0])
LIMIT = {"SMALL": 0.855, "MID": 2.42, "MIDLO": 1.44, "WIDE": 1e8}
ULP = 2.0 ** -52
SUFFIXES = ["_exact", "_exact_deep"]


def _need(suffix):
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core%s.inc" % suffix)):
        pytest.skip("cores not generated (python -m deap_amd.build)")


def _signs(rng, x):
    return x * np.where(rng.random(len(x)) < 0.5, -1.0, 1.0)


def _fill(rng, vals):
    """Waves of 128 lanes holding every value of `vals` with both signs."""
    v = np.concatenate([np.asarray(vals, dtype=np.float64), -np.asarray(vals, dtype=np.float64)])
    pad = (-len(v)) % 128
    v = np.concatenate([v, v[rng.integers(0, len(v), pad)]])
    return [v[i:i + 128] for i in range(0, len(v), 128)]


def _check(which, suffix, waves, limit):
    want = which.split("_")[0]
    f = math.sin if want == "SIN" else math.cos
    lines = asm_emu.handler_lines(which, suffix)
    # a body of its own: no branch into the general handler
    assert len(lines) > 30 and not any(".Lalias" in l for l in lines)
    for x in waves:
        assert np.abs(x).max() < limit
        y, vred = asm_emu.run_handler(which, x, suffix, lines)
        ref = np.array([f(v) for v in x.tolist()])
        bad = y.view(np.uint64) != ref.view(np.uint64)
        assert not bad.any(), (which, x[bad][:4], y[bad][:4], ref[bad][:4])
        assert not vred.any()
    return lines


def _small_edge_waves(rng):
    """The edge set of the SMALL bodies: +-0, +-denormals down to the
    smallest (2^-1074; 2^-1075 is not a double: it is +-0, in the set), the
    0.126 and 0.855 edges by ulps, every binade with both signs (a power of
    two, a full mantissa and a random one), chains that differ."""
    lim = np.nextafter(LIMIT["SMALL"], 0.0)
    vals = [0.0, 5e-324, 1e-323, 2.0 ** -1074, 2.0 ** -1073, 2.2250738585072014e-308,
            np.nextafter(2.2250738585072014e-308, 0), 1e-310, 2.0 ** -1075,
            2.0 ** -26, np.nextafter(2.0 ** -26, 0), np.nextafter(2.0 ** -26, 1),
            2.0 ** -27, lim, np.nextafter(lim, 0), 0.5, 0.25, math.pi / 4]
    vals += [0.126 * (1 + k * ULP) for k in range(-4, 5)]
    vals += [np.nextafter(0.126, 0), np.nextafter(0.126, 1)]
    for e in range(-1074, 0):
        p = math.ldexp(1.0, e)
        vals.append(p)
        if e >= -1022:
            for m in (np.nextafter(2.0, 1.0), 1.0 + rng.random()):
                v = math.ldexp(m, e)
                if v < lim:
                    vals.append(v)
        else:
            vals.append(math.ldexp(1.0 + math.floor(rng.random() * 2 ** (e + 1074))
                                   * 2.0 ** -(e + 1074), e))
    waves = _fill(rng, [v for v in vals if v <= lim])
    # chains that differ: TAYLOR_SIN lanes in one chain only, and tiny against big
    waves.append(np.concatenate([rng.uniform(-0.12, 0.12, 64),
                                 _signs(rng, rng.uniform(0.2, 0.85, 64))]))
    waves.append(np.concatenate([_signs(rng, rng.uniform(0.2, 0.85, 64)),
                                 rng.uniform(-0.12, 0.12, 64)]))
    waves.append(np.concatenate([np.full(64, -0.0), _signs(rng, rng.uniform(0.127, 0.85, 64))]))
    waves.append(np.concatenate([_signs(rng, rng.uniform(0.127, 0.85, 64)),
                                 _signs(rng, np.full(64, 5e-324))]))
    waves.append(np.full(128, -0.0))
    waves.append(np.full(128, 0.0))
    for _ in range(4):
        waves.append(rng.uniform(-lim, lim, 128))
    return waves


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("which", ["SIN_SMALL", "COS_SMALL"])
def test_small_without_da_is_the_host_libm_on_the_edge_set(which, suffix):
    _need(suffix)
    rng = np.random.default_rng(4100 + len(which) + (suffix == "_exact_deep"))
    lines = _check(which, suffix, _small_edge_waves(rng), LIMIT["SMALL"])
    # the da path is gone: no 64-bit move, no 0.5 da
    assert not any(l.startswith("v_mov_b64") for l in lines)
    assert not any(l.startswith("v_mul_f64") and l.endswith(", 0.5") for l in lines)


def _midlo_waves(rng):
    lim = np.nextafter(LIMIT["MIDLO"], 0.0)
    out = [rng.uniform(-lim, lim, 128), np.full(128, lim), np.full(128, -lim),
           np.full(128, 0.0), np.full(128, -0.0),
           rng.uniform(-0.85, 0.85, 128),                        # no d lane
           _signs(rng, rng.uniform(T0855, lim, 128))]            # no small lane
    # one chain all small, one all d (0.85546875 <= |x| < 1.44)
    out.append(np.concatenate([rng.uniform(-0.85, 0.85, 64),
                               _signs(rng, rng.uniform(T0855, lim, 64))]))
    out.append(np.concatenate([_signs(rng, rng.uniform(T0855, lim, 64)),
                               rng.uniform(-0.85, 0.85, 64)]))
    # both sides of 0.85546875 by ulps, the 1.44 end by ulps (where the
    # do_sin argument pi/2 - |x| is nearest 0.126), zeros and denormals
    t = [T0855 * (1 + k * ULP) for k in range(-6, 7)]
    t += [lim * (1 - k * ULP) for k in range(0, 8)]
    t += [0.0, 5e-324, 2.2e-308, 2.0 ** -27, 0.126, 0.855, np.nextafter(0.855, 0),
          1.0, 1.25, 1.4, 1.43, math.pi / 4]
    out += _fill(rng, t)
    for _ in range(6):
        out.append(rng.uniform(-lim, lim, 128))
    return out


@pytest.mark.parametrize("suffix", SUFFIXES)
def test_cos_midlo_is_the_host_libm(suffix):
    _need(suffix)
    rng = np.random.default_rng(1440 + (suffix == "_exact_deep"))
    lines = _check("COS_MIDLO", suffix, _midlo_waves(rng), LIMIT["MIDLO"])
    # no 0.126 compare (the only v_cmpx of the bodies), no |x|.hi
    assert not any(l.startswith("v_cmpx") for l in lines)
    assert not any("0x7fffffff" in l for l in lines)


def test_midlo_margin():
    """The do_sin argument of a d lane below 1.44 is above TAYLOR_SIN's
    0.126 with room for the roundings of (hp0 - |x|) + hp1."""
    hp0 = asm_emu.glibc_constants()["HP0"]
    hp1 = asm_emu.glibc_constants()["HP1"]
    a = (hp0 - np.nextafter(LIMIT["MIDLO"], 0.0)) + hp1
    assert a > 0.126 + 0.004


def _wide_waves(rng):
    lim = np.nextafter(LIMIT["WIDE"], 0.0)
    out = [rng.uniform(-lim, lim, 128), rng.uniform(-1e3, 1e3, 128),
           rng.uniform(-3.0, 3.0, 128), rng.uniform(-0.85, 0.85, 128),
           np.full(128, lim), np.full(128, -lim), np.full(128, -0.0)]
    # both sides of 2.426265 and of 0.85546875, chains that differ
    t = [T2426 * (1 + k * ULP) for k in range(-6, 7)]
    t += [T0855 * (1 + k * ULP) for k in range(-6, 7)]
    t += [0.0, 5e-324, 2.0 ** -27, 0.126, math.pi / 2, math.pi, 2 * math.pi, 1e4, 16384.0,
          1e6, 99999999.0, lim, 105414350.0 * 0.9]
    out += _fill(rng, t)
    out.append(np.concatenate([rng.uniform(-0.85, 0.85, 64), _signs(rng, rng.uniform(3, lim, 64))]))
    out.append(np.concatenate([_signs(rng, rng.uniform(T0855, 2.4, 64)),
                               _signs(rng, rng.uniform(2.43, 1e5, 64))]))
    out.append(np.concatenate([_signs(rng, rng.uniform(2.43, 1e5, 64)),
                               rng.uniform(-0.12, 0.12, 64)]))
    for _ in range(4):
        out.append(_signs(rng, np.exp(rng.uniform(math.log(1e-3), math.log(lim), 128))))
    return out


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("want", ["SIN", "COS"])
def test_wide_agrees_with_the_general_handler(want, suffix):
    _need(suffix)
    rng = np.random.default_rng(10 ** 8 % 977 + len(want) + (suffix == "_exact_deep"))
    which = want + "_WIDE"
    waves = _wide_waves(rng)
    lines = _check(which, suffix, waves, LIMIT["WIDE"])
    assert not any("v_max3_u32" in l for l in lines)             # no VRED update
    assert not any("Lslow" in l for l in lines)                  # no __branred
    glines = asm_emu.handler_lines(want, suffix)
    for x in waves:
        g, s = {}, {}
        a, _ = asm_emu.run_handler(want, x, suffix, glines, counts=g)
        b, _ = asm_emu.run_handler(which, x, suffix, lines, counts=s)
        assert (a.view(np.uint64) == b.view(np.uint64)).all()
        assert s["valu"] == g["valu"] - 2 and s["salu"] <= g["salu"], (g, s)
        assert s["valu_f64"] == g["valu_f64"] and s["lds"] == g["lds"]


@pytest.mark.parametrize("suffix", SUFFIXES)
def test_new_bodies_execute_fewer_instructions(suffix):
    """COS_MIDLO against COS_MID, and the SMALL bodies against the general
    handler, on the same in-range waves: fewer VALU and SALU, no more fp64."""
    _need(suffix)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.43, 1.43, 128)
    m, lo = {}, {}
    a, _ = asm_emu.run_handler("COS_MID", x, suffix, counts=m)
    b, _ = asm_emu.run_handler("COS_MIDLO", x, suffix, counts=lo)
    assert (a.view(np.uint64) == b.view(np.uint64)).all()
    assert lo["valu"] == m["valu"] - 2 and lo["salu"] <= m["salu"] - 4, (m, lo)
    assert lo["valu_f64"] == m["valu_f64"] - 2                   # (the two compares)
    x = rng.uniform(-0.85, 0.85, 128)
    for want, fewer in (("SIN", 6), ("COS", 8)):
        g, s = {}, {}
        asm_emu.run_handler(want, x, suffix, counts=g)
        asm_emu.run_handler(want + "_SMALL", x, suffix, counts=s)
        assert s["valu"] <= g["valu"] - fewer and s["valu_f64"] <= g["valu_f64"], (want, g, s)


# --------------------------------------------------------------- NaN lanes --
@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("want", ["SIN", "COS"])
def test_general_handler_turns_inf_and_nan_into_flagged_zero_payload_nans(want, suffix):
    """Where nanable values are born: the general handler gives NaN with a
    zero low word for an inf or nan lane, and leaves |x|.hi >= 0x7ff00000 in
    that lane of VRED (END then leaves the program's tile to the C++ pass)."""
    _need(suffix)
    rng = np.random.default_rng(7)
    x = rng.uniform(-3.0, 3.0, 128)
    x[3], x[40], x[64 + 3], x[64 + 9], x[100] = np.inf, -np.inf, np.nan, -np.nan, np.inf
    y, vred = asm_emu.run_handler(want, x, suffix)
    bad = ~np.isfinite(x)
    assert np.isnan(y[bad]).all() and np.isfinite(y[~bad]).all()
    assert not (y[bad].view(np.uint64) & 0xffffffff).any()
    lanes = bad[:64] | bad[64:]
    assert (vred[lanes] >= 0x7ff00000).all() and (vred[~lanes] < 0x7ff00000).all()


def _nan_waves(rng, lim):
    lim = np.nextafter(lim, 0.0)
    out = []
    x = rng.uniform(-lim, lim, 128)
    x[::3] = np.nan
    out.append(x)
    out.append(np.full(128, np.nan))
    out.append(np.concatenate([np.full(64, np.nan), rng.uniform(-lim, lim, 64)]))
    out.append(np.concatenate([rng.uniform(-min(lim, 0.12), min(lim, 0.12), 64),
                               np.full(64, -np.nan)]))
    x = _signs(rng, np.full(128, lim))
    x[5] = x[70] = -np.nan
    out.append(x)
    return out


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("which", ["SIN_MID", "COS_MID", "SIN_SMALL", "COS_SMALL",
                                   "COS_MIDLO"])
def test_nan_lanes_stay_inside_the_table_and_come_out_nan(which, suffix, monkeypatch):
    """A NaN whose low word is zero (every NaN of the machine: trig_ranges.h)
    in a specialised handler: u = |x| + BIG keeps the low word, so the lane
    gathers entry 0.  The finite lanes' results are untouched by their
    neighbours.  (run_handler asserts EXEC restored.)"""
    _need(suffix)
    lay = asm_emu.read_layout(suffix)
    seen = []
    orig = asm_emu.Wave._ds

    def spy(self, o, mods, nbytes):
        addr = self.u32(o[1]).astype(np.int64) + mods.get("offset", 0)
        seen.append((addr[self.lanes()], nbytes))
        return orig(self, o, mods, nbytes)

    monkeypatch.setattr(asm_emu.Wave, "_ds", spy)
    want, rng_name = which.split("_")
    f = math.sin if want == "SIN" else math.cos
    rng = np.random.default_rng(77 + len(which))
    lines = asm_emu.handler_lines(which, suffix)
    for x in _nan_waves(rng, LIMIT[rng_name]):
        # canonical NaNs: low word zero (either sign)
        assert not (x[np.isnan(x)].view(np.uint64) & 0xffffffff).any()
        del seen[:]
        y, vred = asm_emu.run_handler(which, x, suffix, lines)
        nan = np.isnan(x)
        assert np.isnan(y[nan]).all()
        ref = np.array([f(v) for v in x[~nan].tolist()])
        assert (y[~nan].view(np.uint64) == ref.view(np.uint64)).all()
        assert seen and not vred.any()
        for addr, nbytes in seen:
            assert addr.min() >= 0 and addr.max() + nbytes <= lay["GLIBC_BRANRED_OFF"], \
                (which, int(addr.min()), int(addr.max()))
