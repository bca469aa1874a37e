"""The exact cores' ABS and SQRT handlers (gen_asm.py deferred_bodies /
sqrt_all), executed on the CPU (tests/asm_emu.py, extended here by subclass)
on one wave, against ``math.sqrt`` bit for bit: every binade from 2^-1074 to
2^1023, subnormals, k * k and its two neighbours, +-0, inf, nan, chains that
differ, and a negative lane, which must put its high word into VRED (the
cores' leave-for-the-C++-finish condition of an infinite sin/cos argument).

``v_rsq_f64`` is not correctly rounded on the hardware; the handler's
refinement must absorb its error.  It is modelled three ways: the rounded
1 / sqrt(x), and that value times (1 +- 2^-27).  All three must give
math.sqrt's bits.  (The GPU probe, gpe_math_probe 17, is the authority on
the hardware's own seed.)
"""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import asm_emu

L = asm_emu.L


class SqrtWave(asm_emu.Wave):
    """asm_emu.Wave plus the instructions only the ABS / SQRT handlers use."""
    seed_scale = 1.0                   # the v_rsq_f64 model's relative error

    def op_v_rsq_f64_e32(self, o, _):
        x = self.f64(o[1])
        with np.errstate(all="ignore"):
            y = 1.0 / np.sqrt(x)       # within an ulp of 1 / sqrt(x)
        self.write_v(o[0], y * self.seed_scale, True)

    def op_v_cmp_class_f64_e64(self, o, _):
        x = self.f64(o[1])
        mask = int(self.sval(o[2]))
        bits = x.view(np.uint64)
        neg = (bits >> np.uint64(63)).astype(bool)
        ex = (bits >> np.uint64(52)) & np.uint64(0x7ff)
        man = bits & np.uint64((1 << 52) - 1)
        cls = np.where(ex == 0x7ff, np.where(man == 0, np.where(neg, 2, 9),
                                             np.where((man >> np.uint64(51)) == 1, 1, 0)),
                       np.where(ex == 0, np.where(man == 0, np.where(neg, 5, 6),
                                                  np.where(neg, 4, 7)),
                                np.where(neg, 3, 8)))
        self.cmp_out(o[0], ((mask >> cls) & 1).astype(bool))

    def op_v_max_u32_e32(self, o, _):
        self._w(o, np.maximum(self.u32(o[1]), self.u32(o[2])))


def run(which, x, suffix, seed_scale=1.0):
    """The handler on 128 values (chains 0, 1): (results, VRED)."""
    lay = asm_emu.read_layout(suffix)
    w = SqrtWave(np.zeros(8), {"one": 0x3ff00000})
    w.seed_scale = seed_scale
    for k in range(2):
        u = asm_emu._f2u(x[64 * k:64 * (k + 1)])
        w.v[32 + 2 * k], w.v[33 + 2 * k] = u[:, 0], u[:, 1]
    lines = asm_emu.handler_lines(which, suffix)
    # no branch, no EXEC write, no barrier: one straight body to its jump
    assert lines[-1].startswith("s_setpc_b64") and not any(
        l.startswith(("s_cbranch", "s_branch", "s_barrier", "v_cmpx")) or "exec" in l
        for l in lines), lines
    w.run(lines)
    assert w.exec == (1 << 64) - 1
    out = np.empty(128)
    for k in range(2):
        out[64 * k:64 * (k + 1)] = (w.v[32 + 2 * k].astype(np.uint64) |
                                    (w.v[33 + 2 * k].astype(np.uint64) << 32)).view(np.float64)
    vred = 32 + 2 * lay["K"] + 2 * lay["K"] * lay["D"]
    return out, w.v[vred].copy(), lines


def arguments():
    rng = np.random.default_rng(23)
    xs = [np.ldexp(1.0, np.arange(-1074, 1024))]                    # every binade
    xs.append(np.ldexp(rng.uniform(0.5, 1.0, 4096), rng.integers(-1073, 1025, 4096)))
    xs.append(rng.integers(1, 1 << 52, 512).astype(np.uint64).view(np.float64))  # subnormals
    k = rng.integers(1, 1 << 26, 1024).astype(np.float64)
    xs += [k * k, np.nextafter(k * k, 0.0), np.nextafter(k * k, np.inf)]
    k = rng.integers(1 << 26, 1 << 53, 512).astype(np.float64)        # inexact squares
    xs += [k * k]
    xs.append(np.array([0.0, -0.0, np.inf, np.nan, 5e-324, 2.2250738585072014e-308,
                        2.225073858507201e-308, 1.7976931348623157e308, 1.0, 2.0, 4.0,
                        0.25, float.fromhex("0x1p-767"), float.fromhex("0x1.fffffffffffffp-768"),
                        float.fromhex("0x1.0000000000001p-767")]))
    x = np.concatenate(xs)
    pad = (-len(x)) % 128
    return np.concatenate([x, np.full(pad, 3.0)])


@pytest.mark.parametrize("suffix", ["_exact", "_exact_deep"])
@pytest.mark.parametrize("seed", [1.0, 1.0 + 2.0 ** -27, 1.0 - 2.0 ** -27])
def test_sqrt_handler_is_math_sqrt(suffix, seed):
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core%s.inc" % suffix)):
        pytest.skip("cores not generated (python -m deap_amd.build)")
    x = arguments()
    rng = np.random.default_rng(5)
    x = x[rng.permutation(len(x))]               # the two chains differ
    ref = np.array([math.sqrt(v) for v in x.tolist()])
    n_f64 = None
    for i in range(0, len(x), 128):
        y, vred, lines = run("SQRT", x[i:i + 128], suffix, seed)
        r = ref[i:i + 128]
        same = (y.view(np.uint64) == r.view(np.uint64)) | (np.isnan(y) & np.isnan(r))
        assert same.all(), (seed, x[i:i + 128][~same][:4], y[~same][:4], r[~same][:4])
        # +0 keeps VRED clear; only -0.0 (its sign bit) sets it here
        neg0 = (x[i:i + 128].view(np.uint64) >> np.uint64(63)).astype(bool)
        assert ((vred >= 0x80000000) == (neg0[:64] | neg0[64:])).all()
        n_f64 = sum("_f64" in l for l in lines)
    # the compiler's sequence per value: 14 fp64 instructions (two compares,
    # two ldexp, the seed, two products, seven fma) and four selects
    assert n_f64 == 2 * 14, n_f64


@pytest.mark.parametrize("suffix", ["_exact", "_exact_deep"])
def test_negative_lane_trips_the_leave_condition(suffix):
    """A negative argument gives nan and raises VRED past every redo
    threshold (the exact cores leave at |x|.hi >= 0x7ff00000 at the latest):
    END then hands the (program, tile) to the C++ finish, whose f_run reports
    ValueError at that case.  The other lanes keep math.sqrt's bits."""
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core%s.inc" % suffix)):
        pytest.skip("cores not generated (python -m deap_amd.build)")
    lay = asm_emu.read_layout(suffix)
    x = np.linspace(0.5, 900.0, 128)
    x[7], x[64 + 40], x[64 + 41] = -4.0, -np.inf, -5e-324
    y, vred, _ = run("SQRT", x, suffix)
    neg = x < 0
    assert np.isnan(y[neg]).all()
    ok = ~neg
    ref = np.array([math.sqrt(v) for v in x[ok].tolist()])
    assert (y[ok].view(np.uint64) == ref.view(np.uint64)).all()
    hit = neg[:64] | neg[64:]
    assert (vred[hit] >= 0x80000000).all() and (vred[~hit] == 0).all()
    assert 0x80000000 > lay.get("EXACT_REDO_HI", 0x7ff00000) > 0


@pytest.mark.parametrize("suffix", ["_exact", "_exact_deep"])
def test_abs_handler_clears_the_sign(suffix):
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core%s.inc" % suffix)):
        pytest.skip("cores not generated (python -m deap_amd.build)")
    rng = np.random.default_rng(9)
    x = np.ldexp(rng.uniform(-1.0, 1.0, 128), rng.integers(-1070, 1024, 128))
    x[:6] = [0.0, -0.0, -np.inf, np.inf, -5e-324, -1.5]
    x[6] = np.uint64(0xfff8000000000000).view(np.float64)          # -nan
    y, vred, lines = run("ABS", x, suffix)
    assert (y.view(np.uint64) == (x.view(np.uint64) & np.uint64((1 << 63) - 1))).all()
    assert not vred.any()
    assert sum(l.startswith("v_") for l in lines) == 2             # one v_and_b32 per case


def test_sqrt_refinement_basis():
    """The reasoning behind the seed models, checked exactly on a few values:
    with a seed within 2^-26 of 1 / sqrt(x), g after the Goldschmidt step is
    within 2^-50 of sqrt(x) and each residual correction (d = x - g g, exact
    in the fma; g += d h) at least squares the error before the final
    rounding.  Here: the emulated handler's result equals the correctly
    rounded root decided with exact rationals."""
    if not os.path.exists(os.path.join(asm_emu.CSRC, "gp_asm_core_exact.inc")):
        pytest.skip("cores not generated (python -m deap_amd.build)")
    rng = np.random.default_rng(77)
    x = np.ldexp(rng.uniform(0.5, 1.0, 128), rng.integers(-1000, 1000, 128))
    for seed in (1.0, 1.0 + 2.0 ** -27, 1.0 - 2.0 ** -27):
        y, _, _ = run("SQRT", x, "_exact", seed)
        for v, r in zip(x.tolist(), y.tolist()):
            lo, hi = np.nextafter(r, 0.0), np.nextafter(r, np.inf)
            fx = Fraction(v)
            # r is nearest: (r + lo) / 2 < sqrt(x) < (r + hi) / 2
            assert ((Fraction(r) + Fraction(float(lo))) / 2) ** 2 < fx < \
                ((Fraction(r) + Fraction(float(hi))) / 2) ** 2


def test_exact_core_kernel_resources():
    """The exact D = 5 kernel (f_eval_asm<false, false, true>) with the two
    handlers: at or below 128 VGPRs (4 waves per SIMD) and no scratch, read
    from the built code object (scripts/kernel_resources.sh; the listing is
    profiles/abs_sqrt_kernel_resources.txt)."""
    import re
    import subprocess
    from deap_amd import build
    build.build()
    out = subprocess.run(["bash", os.path.join(asm_emu.REPO, "scripts", "kernel_resources.sh"),
                          "f_eval_asmILb0ELb0ELb1E"], check=True, capture_output=True,
                         text=True).stdout
    m = re.search(r"vgpr\s+(\d+) spill\s+(\d+) .* scratch\s+(\d+)", out)
    assert m, out
    vgpr, spill, scratch = map(int, m.groups())
    print("ASEMU|exact D=5 kernel: vgpr %d spill %d scratch %d" % (vgpr, spill, scratch))
    assert vgpr <= 128 and spill == 0 and scratch == 0, out
