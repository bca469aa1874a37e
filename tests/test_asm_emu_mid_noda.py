"""The exact cores' MID / MIDLO sin/cos bodies with static lane roles
(SIN_MID3, COS_MID3, SIN_MIDLO3, COS_MIDLO3: gen_asm.py glibc_seq4(rng="mid3"
/ "midlo3"), GPE_TRIG_RANGES=3), executed on the CPU (tests/asm_emu.py): every
result is the host libm's in every bit and the mode-2 body's on the same
wave, with the temporaries poisoned (a lane that read a da it never wrote
would show), NaN lanes of the "bounded or NaN" state come out NaN with every
gather inside the table, EXEC is restored (run_handler asserts it), and the
range pass picks midlo for a sin node only below 1.44.  No GPU.
"""
import math
import os

import numpy as np
import pytest

import asm_emu
from deap_amd import _lib, configs, gp
from deap_amd.flatten import Flattener

T0855 = 0.85546875                       # glibc's threshold (hx < 0x3feb6000)
T2426 = float(np.array([0x400368fd << 32], dtype=np.uint64).view(np.float64)[0])
ULP = 2.0 ** -52
SUFFIXES = ["_exact", "_exact_deep"]
# body: (the bound its arguments stay below, the mode-2 body of the same node).
# MID3 is run up to glibc's own 2.426265 (|x|.hi < 0x400368fd), the last
# double below it included: the range pass stops at 2.42, inside that.  At
# and past 2.426265 a lane is reduce_sincos's, which no MID body has, so that
# edge has one side here
BODIES = {"SIN_MID3": (T2426, "SIN_MID"), "COS_MID3": (T2426, "COS_MID"),
          "SIN_MIDLO3": (1.44, "SIN_MID"), "COS_MIDLO3": (1.44, "COS_MIDLO")}
GENERAL, MID, SMALL, MIDLO, WIDE = range(5)


def _need(suffix):
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core%s.inc" % suffix)):
        pytest.skip("cores not generated (python -m deap_amd.build)")


@pytest.fixture
def poisoned(monkeypatch):
    """Every VGPR a handler may use as a temporary (the pool after VRED and
    VINF, up to the named operands) starts as a NaN with a payload, not as
    0: da is written in the d lanes only, and a small lane that still read
    it would no longer get the +0 it used to hold."""
    init = asm_emu.Wave.__init__

    def arm(suffix):
        lay = asm_emu.read_layout(suffix)
        pool = 32 + 2 * lay["K"] + 2 * lay["K"] * lay["D"] + 2     # gen_asm Gen.POOL0

        def poison(self, lds, named):
            init(self, lds, named)
            self.v[pool:200, :] = 0x7ff4dead

        monkeypatch.setattr(asm_emu.Wave, "__init__", poison)
    return arm


def _signs(rng, x):
    return x * np.where(rng.random(len(x)) < 0.5, -1.0, 1.0)


def _fill(rng, vals):
    """Waves of 128 lanes holding every value of `vals` with both signs."""
    v = np.asarray(vals, dtype=np.float64)
    v = np.concatenate([v, -v])
    pad = (-len(v)) % 128
    v = np.concatenate([v, v[rng.integers(0, len(v), pad)]])
    return [v[i:i + 128] for i in range(0, len(v), 128)]


def _edge_waves(rng, limit):
    """+-0, +-denormals down to 2^-1074, every binade up to the class bound,
    the 0.126, 0.85546875, pi/2, 1.44 and 2.42 edges by ulps on both sides and
    2.426265 by ulps from below (whatever of them lies below the bound),
    chains that differ, chains without a d lane and chains of d lanes only."""
    lim = float(np.nextafter(limit, 0.0))
    vals = [0.0, 5e-324, 1e-323, 2.0 ** -1073, 2.2250738585072014e-308,
            float(np.nextafter(2.2250738585072014e-308, 0)), 1e-310, 2.0 ** -26,
            float(np.nextafter(2.0 ** -26, 0)), 2.0 ** -27, lim, 0.5, 1.0, 1.25, 1.4, math.pi / 4]
    for edge in (0.126, T0855, math.pi / 2, 1.44, 2.42, T2426, lim,
                 math.pi / 2 - 0.126, math.pi / 2 + 0.126):
        vals += [edge * (1 + k * ULP) for k in range(-6, 7)]
        vals += [float(np.nextafter(edge, 0)), float(np.nextafter(edge, 4))]
    for e in range(-1074, 2):
        p = math.ldexp(1.0, e)
        vals.append(p)
        if e >= -1022:
            vals += [math.ldexp(float(np.nextafter(2.0, 1.0)), e),
                     math.ldexp(1.0 + rng.random(), e)]
        else:
            vals.append(p + math.ldexp(math.floor(rng.random() * 2 ** (e + 1074)), -1074))
    waves = _fill(rng, [v for v in vals if v <= lim])
    small = lambda n: rng.uniform(-0.85, 0.85, n)
    tiny = lambda n: rng.uniform(-0.12, 0.12, n)
    d = lambda n: _signs(rng, rng.uniform(T0855, lim, n))
    waves += [small(128), d(128), tiny(128),                      # no d lane / d lanes only
              np.concatenate([small(64), d(64)]), np.concatenate([d(64), small(64)]),
              np.concatenate([tiny(64), d(64)]), np.concatenate([d(64), tiny(64)]),
              np.concatenate([np.full(64, -0.0), d(64)]),
              np.concatenate([d(64), _signs(rng, np.full(64, 5e-324))]),
              np.full(128, 0.0), np.full(128, -0.0), np.full(128, lim), np.full(128, -lim)]
    # one d lane among small ones, one small lane among d ones
    x = small(128)
    x[7], x[64 + 40] = lim, -T0855
    waves.append(x)
    x = d(128)
    x[3], x[64 + 63] = 0.1, -0.0
    waves.append(x)
    for _ in range(6):
        waves.append(rng.uniform(-lim, lim, 128))
    return waves


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("which", list(BODIES))
def test_body_is_the_host_libm_and_the_mode_2_body(which, suffix, poisoned):
    _need(suffix)
    poisoned(suffix)
    limit, twin = BODIES[which]
    f = math.sin if which.startswith("SIN") else math.cos
    rng = np.random.default_rng(3000 + len(which) + 7 * (suffix == "_exact_deep"))
    lines = asm_emu.handler_lines(which, suffix)
    old = asm_emu.handler_lines(twin, suffix)
    # a body of its own
    assert len(lines) > 30 and not any(".Lalias" in l for l in lines)
    waves = _edge_waves(rng, limit)
    # the bound's own edge is in: the last double below it, with both signs
    top = float(np.nextafter(limit, 0.0))
    assert any((x == top).any() for x in waves) and any((x == -top).any() for x in waves)
    if limit == T2426:                   # ... and both sides of the pass's 2.42
        assert any(((np.abs(x) > 2.42) & (np.abs(x) < 2.4200001)).any() for x in waves)
    for x in waves:
        assert np.abs(x).max() < limit
        n, o = {}, {}
        y, vred = asm_emu.run_handler(which, x, suffix, lines, counts=n)
        z, _ = asm_emu.run_handler(twin, x, suffix, old, counts=o)
        ref = np.array([f(v) for v in x.tolist()])
        bad = _bits(y) != _bits(ref)
        assert not bad.any(), (which, x[bad][:4], y[bad][:4], ref[bad][:4])
        assert (_bits(y) == _bits(z)).all()
        assert not vred.any()
        # fewer instructions, and no fp64 operation added
        assert n["valu"] < o["valu"] and n["valu_f64"] <= o["valu_f64"], (n, o)
        assert n["salu"] <= o["salu"] + 1 and n["lds"] == o["lds"], (n, o)


@pytest.mark.parametrize("suffix", SUFFIXES)
def test_the_da_plumbing_is_gone(suffix):
    """No zeroing move of da, no copy da := v; the sin bodies have no 0.5 da;
    SIN_MIDLO3 has no 64-bit move at all (hp1 is an SGPR operand) and no sign
    operation on da; COS_MIDLO3 no sign operation on da either."""
    _need(suffix)
    for which in BODIES:
        lines = asm_emu.handler_lines(which, suffix)
        mov64 = [l for l in lines if l.startswith("v_mov_b64")]
        # (cos: the one zeroing move left is n's pair)
        assert sum(l.endswith(", 0") for l in mov64) == (1 if which.startswith("COS") else 0)
        assert not any(re_v(l) for l in mov64), mov64
        if which.startswith("SIN"):
            assert not any(l.startswith("v_mul_f64") and l.endswith(", 0.5") for l in lines)
    assert not any(l.startswith("v_mov_b64") for l in asm_emu.handler_lines("SIN_MIDLO3", suffix))
    # sign operations (v_bitop3): mid3 signs da per chain; sin also has the
    # result's two, cos n's fold and the result's (four)
    nb = {w: sum(l.startswith("v_bitop3") for l in asm_emu.handler_lines(w, suffix))
          for w in BODIES}
    assert nb == {"SIN_MID3": 4, "SIN_MIDLO3": 2, "COS_MID3": 6, "COS_MIDLO3": 4}, nb


def re_v(line):
    """A 64-bit move whose source is a VGPR pair (the copy da := v)."""
    return line.split(",")[-1].strip().startswith("v[")


def test_static_counts():
    """The VALU lines of the generated text: 6 / 10 fewer than SIN_MID, 4
    fewer than COS_MID, 6 fewer than COS_MIDLO."""
    _need("_exact")
    n = {w: sum(l.startswith("v_") for l in asm_emu.handler_lines(w, "_exact"))
         for w in list(BODIES) + ["SIN_MID", "COS_MID", "COS_MIDLO"]}
    assert n["SIN_MID3"] == n["SIN_MID"] - 6 and n["SIN_MIDLO3"] == n["SIN_MID"] - 10, n
    assert n["COS_MID3"] == n["COS_MID"] - 4 and n["COS_MIDLO3"] == n["COS_MIDLO"] - 6, n


def _nan_waves(rng, lim):
    lim = float(np.nextafter(lim, 0.0))
    out = []
    x = rng.uniform(-lim, lim, 128)
    x[::3] = np.nan
    out.append(x)
    out.append(np.full(128, np.nan))
    out.append(np.concatenate([np.full(64, np.nan), rng.uniform(-lim, lim, 64)]))
    out.append(np.concatenate([rng.uniform(-0.12, 0.12, 64), np.full(64, -np.nan)]))
    x = _signs(rng, np.full(128, lim))
    x[5] = x[70] = -np.nan
    out.append(x)
    x = rng.uniform(-0.8, 0.8, 128)              # NaN the only d lanes
    x[9] = x[64 + 1] = np.nan
    out.append(x)
    return out


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("which", list(BODIES))
def test_nan_lanes_stay_inside_the_table_and_come_out_nan(which, suffix, monkeypatch, poisoned):
    _need(suffix)
    poisoned(suffix)
    lay = asm_emu.read_layout(suffix)
    seen = []
    orig = asm_emu.Wave._ds

    def spy(self, o, mods, nbytes):
        addr = self.u32(o[1]).astype(np.int64) + mods.get("offset", 0)
        seen.append((addr[self.lanes()], nbytes))
        return orig(self, o, mods, nbytes)

    monkeypatch.setattr(asm_emu.Wave, "_ds", spy)
    limit, twin = BODIES[which]
    f = math.sin if which.startswith("SIN") else math.cos
    rng = np.random.default_rng(91 + len(which))
    lines = asm_emu.handler_lines(which, suffix)
    for x in _nan_waves(rng, limit):
        assert not (_bits(x[np.isnan(x)]) & 0xffffffff).any()
        del seen[:]
        y, vred = asm_emu.run_handler(which, x, suffix, lines)
        nan = np.isnan(x)
        assert np.isnan(y[nan]).all()
        ref = np.array([f(v) for v in x[~nan].tolist()])
        assert (_bits(y[~nan]) == _bits(ref)).all()
        assert seen and not vred.any()
        for addr, nbytes in seen:
            assert addr.min() >= 0 and addr.max() + nbytes <= lay["GLIBC_BRANRED_OFF"], \
                (which, int(addr.min()), int(addr.max()))


def test_mode_2_bodies_are_still_there():
    """GPE_TRIG_RANGES=2's handlers keep bodies of their own (the A/B
    control), and every core's layout has the four new ids after COS_WIDE."""
    _need("_exact")
    for w in ("SIN_MID", "COS_MID", "COS_MIDLO"):
        lines = asm_emu.handler_lines(w, "_exact")
        assert len(lines) > 30 and not any(".Lalias" in l for l in lines)
    for suffix in SUFFIXES:
        lay = asm_emu.read_layout(suffix)
        assert [lay[k] - lay["H_COS_WIDE"] for k in
                ("H_SIN_MID3", "H_COS_MID3", "H_SIN_MIDLO3", "H_COS_MIDLO3")] == [1, 2, 3, 4]
        assert lay["H_COUNT"] == lay["H_COS_MIDLO3"] + 1


# -------------------------------------------------------------- range pass --
@pytest.fixture(scope="module")
def pset():
    return configs.pset_for("symreg10")


def _classes(pset, expr, bounds, mode=3):
    b = Flattener(pset).flatten([gp.PrimitiveTree.from_string(expr, pset)])
    lo, hi = zip(*bounds)
    return list(_lib.debug_trig_picks(b.code, np.array(lo), np.array(hi), mode=mode))


def test_sin_midlo_rules(pset):
    from test_trig_ranges import BOUNDS, NV

    def col(lo, hi):
        return [(lo, hi)] * NV
    below = float(np.nextafter(1.44, 0))
    assert _classes(pset, "sin(ARG0)", col(0.0, below)) == [MIDLO]
    assert _classes(pset, "sin(ARG0)", col(0.0, 1.44)) == [MID]
    assert _classes(pset, "sin(ARG0)", col(-below, 0.0)) == [MIDLO]
    assert _classes(pset, "sin(ARG0)", col(-1.44, 0.0)) == [MID]
    assert _classes(pset, "sin(ARG0)", col(0.0, 0.8)) == [SMALL]
    assert _classes(pset, "sin(ARG0)", col(0.0, 2.0)) == [MID]
    assert _classes(pset, "sin(ARG0)", col(0.0, 3.0)) == [WIDE]
    assert _classes(pset, "sin(mul(ARG0, ARG1))", BOUNDS["unit"]) == [MIDLO]
    assert _classes(pset, "sin(add(ARG0, ARG1))", BOUNDS["unit"]) == [MID]
    # nanable arguments are allowed, as for COS_MIDLO
    assert _classes(pset, "sin(cos(ARG3))", BOUNDS["unbounded3"]) == [GENERAL, MIDLO]
    # modes 1 and 2 are what they were, through either entry point
    assert _classes(pset, "sin(ARG0)", col(0.0, 1.0), mode=2) == [MID]
    assert _classes(pset, "cos(ARG0)", col(0.0, 1.0), mode=2) == [MIDLO]
    assert _classes(pset, "cos(ARG0)", col(0.0, 1.0), mode=1) == [MID]
    # mode 4, SIN_MIDLO3's A/B control: mode 2's classes
    assert _classes(pset, "sin(ARG0)", col(0.0, 1.0), mode=4) == [MID]
    assert _classes(pset, "cos(ARG0)", col(0.0, 1.0), mode=4) == [MIDLO]
    assert _classes(pset, "sin(cos(ARG3))", BOUNDS["unbounded3"], mode=4) == [GENERAL, MID]
    for mode in (0, 5):
        with pytest.raises(_lib.GpeError):
            _classes(pset, "sin(ARG0)", col(0.0, 1.0), mode=mode)


@pytest.mark.parametrize("name", ["unit", "offset", "wide", "unbounded3"])
def test_mode_3_differs_from_mode_2_in_sin_midlo_only_and_it_holds(pset, name):
    """Sampled evaluation, as test_trig_ranges_more.py does for COS_MIDLO:
    every sin node picked midlo has |x| < 1.44 (or NaN, downstream of a
    possible inf) in every sampled case; nothing else changes."""
    from test_trig_ranges import BOUNDS, HAND, cases, trig_arguments
    from test_trig_ranges_more import INF_PROGRAMS, check_node, words_of
    pop = configs.population(pset, "half", 600, 1441, 1, 8)
    pop += [gp.PrimitiveTree.from_string(s, pset) for s in HAND + INF_PROGRAMS]
    lo = np.array([b[0] for b in BOUNDS[name]])
    hi = np.array([b[1] for b in BOUNDS[name]])
    unbounded = {v for v, b in enumerate(BOUNDS[name]) if math.isinf(b[0])}
    X = cases(name)
    sin_midlo = 0
    for tree, w in zip(pop, words_of(pset, pop)):
        c2 = list(_lib.debug_trig_classes(w, lo, hi, mode=2))
        assert c2 == list(_lib.debug_trig_picks(w, lo, hi, mode=2))
        c3 = list(_lib.debug_trig_picks(w, lo, hi, mode=3))
        args = trig_arguments(w, X, unbounded)
        assert len(c2) == len(c3) == len(args), str(tree)
        for a, b, (arg, dirty) in zip(c2, c3, args):
            check_node(b, arg, dirty, (name, str(tree)[:200]))
            if a != b:
                assert (a, b) == (MID, MIDLO), str(tree)
                sin_midlo += 1
    print("TRIGCLS3|%s|sin nodes mid -> midlo: %d" % (name, sin_midlo))
    if name in ("unit", "offset"):
        assert sin_midlo > 0


def test_translation_picks_the_static_role_handlers(pset):
    """gpe_debug_translate in mode 3: the same word count, only sin/cos words
    differ, mid and midlo words are the new handlers' (sin midlo:
    SIN_MIDLO3), and mode 2 picks what it did."""
    from test_trig_ranges import HAND, NV
    try:
        lay = asm_emu.read_layout("_exact")
    except OSError:
        pytest.skip("asm cores not generated")
    pop = configs.population(pset, "half", 300, 79, 1, 6)
    pop += [gp.PrimitiveTree.from_string(s, pset) for s in HAND]
    pop += [gp.PrimitiveTree.from_string(s, pset) for s in
            ("sin(ARG0)", "cos(ARG0)", "sin(mul(ARG0, ARG1))", "cos(add(ARG0, ARG1))",
             "sin(add(ARG0, ARG1))", "sin(ARG3)")]
    batch = Flattener(pset).flatten(pop)
    table = np.arange(lay["H_COUNT"], dtype=np.uint32) * 4 + 0x1000
    lo = np.array([-1.0] * 3 + [-50.0] + [-1.0] * (NV - 4))
    hi = -lo
    plain, s0 = _lib.debug_translate(batch, NV, table)
    m2, s2 = _lib.debug_translate(batch, NV, table, bounds=(lo, hi), mode=2)
    m3, s3 = _lib.debug_translate(batch, NV, table, bounds=(lo, hi), mode=3)
    m4, s4 = _lib.debug_translate(batch, NV, table, bounds=(lo, hi), mode=4)
    assert len(plain) == len(m2) == len(m3) == len(m4) and np.array_equal(s0, s3)
    name2 = {("H_SIN", GENERAL): "H_SIN", ("H_SIN", MID): "H_SIN_MID",
             ("H_SIN", SMALL): "H_SIN_SMALL", ("H_SIN", WIDE): "H_SIN_WIDE",
             ("H_COS", GENERAL): "H_COS", ("H_COS", MID): "H_COS_MID",
             ("H_COS", SMALL): "H_COS_SMALL", ("H_COS", MIDLO): "H_COS_MIDLO",
             ("H_COS", WIDE): "H_COS_WIDE"}
    name3 = dict(name2)
    name3.update({("H_SIN", MID): "H_SIN_MID3", ("H_COS", MID): "H_COS_MID3",
                  ("H_SIN", MIDLO): "H_SIN_MIDLO3", ("H_COS", MIDLO): "H_COS_MIDLO3"})
    word = {k: int(table[lay[k]]) for k in set(name2.values()) | set(name3.values())}
    code = np.asarray(batch.code, dtype=np.uint32)
    off = np.asarray(batch.offsets, dtype=np.int64)
    seen = set()
    for i in range(len(pop)):
        if s0[i] < 0:
            continue
        end = s0[i + 1:][s0[i + 1:] >= 0]
        a, b = int(s0[i]), int(end[0]) if len(end) else len(plain)
        w = code[off[i]:off[i + 1]]
        c2 = list(_lib.debug_trig_picks(w, lo, hi, mode=2))
        c3 = list(_lib.debug_trig_picks(w, lo, hi, mode=3))
        trig = [j for j in range(a, b) if plain[j] in (word["H_SIN"], word["H_COS"])]
        assert len(trig) == len(c2) == len(c3), str(pop[i])
        for j in np.nonzero(plain[a:b] != m3[a:b])[0]:
            assert a + j in trig, str(pop[i])
        for j, p, q in zip(trig, c2, c3):
            kind = "H_SIN" if plain[j] == word["H_SIN"] else "H_COS"
            assert m2[j] == word[name2[(kind, p)]], str(pop[i])
            assert m3[j] == word[name3[(kind, q)]], str(pop[i])
            # mode 4: mode 2's class, mode 3's handler of it
            assert m4[j] == word[name3[(kind, p)]], str(pop[i])
            seen.add(name3[(kind, q)])
    assert seen == set(name3.values())
