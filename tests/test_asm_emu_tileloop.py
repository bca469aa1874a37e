"""The exact core's resident tile loop (gen_asm.py Gen.tile_next) on the CPU.

The whole generated D = 5 exact core — prologue, program loop, handlers, the
lean MSE epilogue of END and the tile change — is executed for one wave by an
extension of tests/asm_emu.py's emulator: SMEM window loads, the threaded
dispatch (s_movrels / s_setpc), lane reads, the LDS accumulators, s_barrier
(counted) and the tile's LDS-DMA (global_load_lds_dwordx4, done at issue).

Three lean tiles with different column values, two tile buffers, three
programs per wave:
* the accumulators after one resident run over the three tiles equal those
  of three single-tile entries (the per-tile C++ loop's), bit for bit, and a
  program without sin/cos equals numpy's own Fast2Sum accumulation;
* a program that meets an inf in the middle tile leaves for the caller's
  ``finish`` with the tile it stopped in, and the re-entry at the next
  program goes on from there: one barrier per tile change in all;
* the generation-time barrier / EXEC check (gen_asm.check_tile_loop) accepts
  the emitted text and rejects broken variants of it.
"""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import asm_emu
from asm_emu import L, M32, Wave

CODE_BASE = 0x00007F0010000000      # the core's (emulated) address
CODE_MEM = 0x0000000100000000       # program words
CST_MEM = 0x0000000200000000        # the two SGPR constant blocks
COL_MEM = 0x0000000300000000        # the case columns (X rows, then y)
NV, NT, K = 3, 1, 2
NTILES = 3
TILE_BYTES = (NV + NT) * K * 64 * 8
P = 3                                # programs of the wave

# operand -> register of the emulated call (SGPRs below s40, VGPRs below v32)
SREG = {"jio": "s0", "tio": "s1", "bflip": "s2", "tend": "s3", "probe": "s4",
        "nmine": "s5", "done": "s6", "rhi": "s7", "lean": "s8", "code_lo": "s9",
        "code_hi": "s10", "cst": "s[12:13]", "probe_out": "s[14:15]"}
VREG = {"xa": "v10", "vts": "v11", "vacc": "v12", "vstart": "v13", "dlo": "v14",
        "dhi": "v15", "ddst": "v16", "one": "v17", "mg": "v[18:19]",
        "g_sn5": "v[20:21]", "g_cs6": "v[22:23]", "g_s5": "v[24:25]"}


def _gen_asm():
    spec = importlib.util.spec_from_file_location(
        "gen_asm_tileloop", os.path.join(asm_emu.CSRC, "gen_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """The exact core generated afresh (the product's settings)."""
    out = str(tmp_path_factory.mktemp("core"))
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("GEN_ASM")}
    try:
        gen = _gen_asm()
        gen.emit(K, 5, 32, "_exact", out_dir=out)
        g = gen.Gen(K, 5, 32, exact=True, loop=True, tile_loop=True).build()
    finally:
        os.environ.update(saved)
    src = open(os.path.join(out, "gp_asm_core_exact.inc")).read()
    assert "#define GP_ASM_TILE_LOOP_EXACT 1" in src
    body = src[src.index("#define GP_ASM_CORE_EXACT"):src.index("#define GP_ASM_CLOBBERS")]
    lines = [l.strip().strip("\\").strip().strip('"').replace("\\n", "")
             for l in body.split("\n")[1:]]
    lines = [l for l in lines if l]
    assert lines == g.lines
    return {"gen": gen, "g": g, "lines": lines, "layout": asm_emu.read_layout("_exact", out)}


class CoreWave(Wave):
    """asm_emu.Wave with what the core uses outside its sin/cos handlers."""

    def __init__(self, lds, mem):
        Wave.__init__(self, lds, {})
        self.mem = mem                      # base address -> uint8 array
        self.barriers = 0
        self.dma = []                       # (global address, LDS address) per copy

    def load(self, addr, n):
        for base, buf in self.mem.items():
            if base <= addr and addr + n <= base + len(buf):
                return buf[addr - base:addr - base + n]
        raise AssertionError("global read outside the buffers: 0x%x + %d" % (addr, n))

    def pair(self, op):
        return self.get_mask(op)

    def set_s(self, op, v):
        if op == "m0":
            self.m0 = v & M32
        else:
            self.s[self._reg(op)[1]] = v & M32

    def run_core(self, lines, max_steps=400000):
        labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
        pc = steps = 0
        with np.errstate(all="ignore"):
            while pc < len(lines):
                steps += 1
                assert steps < max_steps, "runaway"
                line = lines[pc]
                pc += 1
                if line.endswith(":"):
                    continue
                mn, _, rest = line.partition(" ")
                mods = {}
                m = re.search(r"\s(offset|bitop3):(0x[0-9a-f]+|\d+)$", rest)
                if m:
                    mods[m.group(1)] = int(m.group(2), 0)
                    rest = rest[:m.start()]
                o = [x.strip() for x in rest.split(",")] if rest else []
                if mn in ("s_waitcnt", "s_setprio", "s_nop"):
                    continue
                if mn == "s_barrier":
                    assert self.exec == (1 << 64) - 1
                    self.barriers += 1
                elif mn == "s_branch":
                    pc = labels[o[0]] + 1
                elif mn.startswith("s_cbranch_"):
                    take = {"execz": self.exec == 0, "execnz": self.exec != 0,
                            "scc0": self.scc == 0, "scc1": self.scc == 1,
                            "vccz": self.vcc == 0, "vccnz": self.vcc != 0}[mn[10:]]
                    if take:
                        pc = labels[o[0]] + 1
                elif mn == "s_getpc_b64":
                    self.set_mask(o[0], CODE_BASE + 4 * pc)
                elif mn == "s_setpc_b64":
                    tgt = self.pair(o[0]) - CODE_BASE
                    assert tgt % 4 == 0 and lines[tgt // 4].startswith(".Lh_"), hex(tgt)
                    pc = tgt // 4
                elif mn == "s_movrels_b32":
                    self.set_s(o[0], int(self.s[self._reg(o[1])[1] + self.m0]))
                elif mn == "s_load_dwordx16":
                    w = np.frombuffer(self.load(self.pair(o[1]) + int(o[2], 0), 64).tobytes(),
                                      dtype="<u4")
                    r = self._reg(o[0])[1]
                    self.s[r:r + 16] = w
                elif mn in ("s_add_u32", "s_addc_u32", "s_sub_u32"):
                    a, b = self.sval(o[1]), self.sval(o[2])
                    r = a - b if mn == "s_sub_u32" else a + b + (self.scc if mn == "s_addc_u32" else 0)
                    self.scc = int(r < 0 or r > M32)
                    self.set_s(o[0], r)
                elif mn in ("s_lshl_b32", "s_lshr_b32"):
                    a, b = self.sval(o[1]), self.sval(o[2]) & 31
                    r = (a << b) & M32 if mn == "s_lshl_b32" else a >> b
                    self.scc = int(r != 0)
                    self.set_s(o[0], r)
                elif mn == "s_max_i32":
                    a, b = (v - (1 << 32) if v >> 31 else v
                            for v in (self.sval(o[1]), self.sval(o[2])))
                    self.scc = int(a >= b)
                    self.set_s(o[0], max(a, b))
                elif mn in ("s_cmp_ge_u32", "s_cmp_lt_u32", "s_cmp_eq_u32"):
                    a, b = self.sval(o[0]), self.sval(o[1])
                    self.scc = int({"ge": a >= b, "lt": a < b, "eq": a == b}[mn[6:8]])
                elif mn == "s_cmp_eq_u64":
                    self.scc = int(self.pair(o[0]) == int(o[1], 0))
                elif mn == "s_bitcmp1_b32":
                    self.scc = (self.sval(o[0]) >> (self.sval(o[1]) & 31)) & 1
                elif mn == "v_readlane_b32":
                    self.set_s(o[0], int(self.v[self._reg(o[1])[1], self.sval(o[2]) & 63]))
                elif mn == "v_writelane_b32":
                    self.v[self._reg(o[0])[1], self.sval(o[2]) & 63] = self.sval(o[1])
                else:
                    getattr(self, "op_" + mn)(o, mods)
        return steps

    # VALU / LDS / VMEM the base emulator has no use for
    def op_v_cmp_le_u32_e64(self, o, _):
        self.cmp_out(o[0], self.u32(o[1]).astype(np.int64) <= self.u32(o[2]).astype(np.int64))

    def op_v_cmp_class_f64_e64(self, o, _):
        assert self.sval(o[2]) == 0x207              # nan, -inf, +inf
        self.cmp_out(o[0], ~np.isfinite(self.f64(o[1])))

    def op_v_max_f64(self, o, _):
        self.write_v(o[0], np.fmax(self.f64(o[1]), self.f64(o[2])), True)

    def op_v_min_f64(self, o, _):
        self.write_v(o[0], np.fmin(self.f64(o[1]), self.f64(o[2])), True)

    def op_v_mbcnt_lo_u32_b32(self, o, _):
        assert o[1] == "-1"
        self.write_v(o[0], np.minimum(np.arange(L), 32) + self.u32(o[2]))

    def op_v_mbcnt_hi_u32_b32(self, o, _):
        assert o[1] == "-1"
        self.write_v(o[0], np.maximum(np.arange(L) - 32, 0) + self.u32(o[2]))

    def op_ds_write_b64(self, o, mods):
        addr = self.u32(o[0]).astype(np.int64) + mods.get("offset", 0)
        n = self._reg(o[1])[1]
        for i in np.nonzero(self.lanes())[0]:
            a = int(addr[i])
            assert a + 8 <= len(self.lds), "LDS write past the allocation at %d" % a
            self.lds[a:a + 8] = np.array([self.v[n, i], self.v[n + 1, i]],
                                         dtype="<u4").view(np.uint8)

    def op_global_load_lds_dwordx4(self, o, _):
        assert self.exec == (1 << 64) - 1
        base, off = self.pair(o[1]), self.u32(o[0]).astype(np.int64)
        for i in range(L):
            a = self.m0 + 16 * i
            assert a + 16 <= len(self.lds)
            self.lds[a:a + 16] = self.load(base + int(off[i]), 16)
        self.dma.append((base, self.m0))


def f2u(x):
    return np.frombuffer(np.asarray(x, dtype="<f8").tobytes(), dtype="<u4")


class Setup(object):
    """One wave's world: three programs, the columns of three tiles in
    global memory, the LDS (tables | two tile buffers | accumulators)."""

    # program -> handler names (window of 16 words, END-terminated)
    PROGRAMS = [["LDV0", "PUSH0", "LDV1", "add_S0", "END"],             # x0 + x1
                ["LDV2", "SIN", "PUSH0", "LDV0", "mul_S0", "END"],      # sin(x2) * x0
                ["LDV1", "PUSH0", "LDV2", "add_S0", "COS", "END"]]      # cos(x1 + x2)

    def __init__(self, core, inf_case=None):
        self.core = core
        lines = core["lines"]
        sub = dict(SREG, **VREG)
        self.lines = [re.sub(r"%\[(\w+)\]", lambda m: sub[m.group(1)], l) for l in lines]
        self.lay = core["layout"]
        self.ktab = self.lay["GLIBC_LDS_BYTES"]
        rng = np.random.default_rng(31)
        n = NTILES * K * 64
        self.cols = rng.uniform(-3.0, 3.0, size=(NV + NT, n))      # x0, x1, x2, y
        if inf_case is not None:
            self.cols[2, inf_case] = math.inf
        lab = {l[:-1]: i for i, l in enumerate(self.lines) if l.endswith(":")}
        words = []
        for prog in self.PROGRAMS:
            w = [(CODE_BASE + 4 * lab[".Lh_%s_%%=" % h]) & M32 for h in prog]
            words += w + [0] * (16 - len(w))
        c = asm_emu.glibc_constants()
        ks = [c["HPINV"], c["MP1"], c["MP2"], c["PP3"], c["PP4"], c["BIG"], c["HP0"],
              c["HP1"], c["SN3"], c["CS4"], c["CS2"], c["S4"], c["S3"], c["S2"], c["S1"], 0.126]
        self.mem = {CODE_MEM: np.array(words, dtype="<u4").view(np.uint8),
                    CST_MEM: np.array(ks, dtype="<f8").view(np.uint8),
                    COL_MEM: np.ascontiguousarray(self.cols).view(np.uint8).reshape(-1)}
        self.acc0 = self.ktab + 2 * TILE_BYTES
        self.lds_doubles = (self.acc0 + P * 1024) // 8

    def tile(self, t):
        """Tile t as it lies in a tile buffer: [column][K][64]."""
        return self.cols[:, t * K * 64:(t + 1) * K * 64].reshape(-1)

    def wave(self, lds=None):
        img = np.zeros(self.lds_doubles)
        img[:self.ktab // 8] = asm_emu.lds_image(self.lay)
        w = CoreWave(img, self.mem)
        if lds is not None:
            w.lds[:] = lds
        c = asm_emu.glibc_constants()
        for name, val in (("mg", float.fromhex("0x1.8p52")), ("g_sn5", c["SN5"]),
                          ("g_cs6", c["CS6"]), ("g_s5", c["S5"])):
            r = int(re.match(r"v\[(\d+)", VREG[name]).group(1))
            w.v[r, :], w.v[r + 1, :] = f2u([val])
        lane = np.arange(L, dtype=np.uint32)
        w.v[17, :] = 0x3ff00000
        w.v[12, :] = self.acc0 + 8 * lane                       # vacc
        w.v[13, :P] = [16 * j for j in range(P)]                # vstart: first words
        # this wave copies every column: lane i, column i
        col_addr = [COL_MEM + 8 * i * self.cols.shape[1] for i in range(NV + NT)]
        w.v[14, :NV + NT] = [a & M32 for a in col_addr]
        w.v[15, :NV + NT] = [a >> 32 for a in col_addr]
        w.v[16, :NV + NT] = [self.ktab + 1024 * i for i in range(NV + NT)]
        w.m0 = 0x1234                                            # the caller's
        for name, v in (("probe", 0), ("nmine", P), ("done", 0), ("rhi", 0x7ff00000),
                        ("lean", 1), ("code_lo", CODE_MEM & M32), ("code_hi", CODE_MEM >> 32)):
            w.s[int(SREG[name][1:])] = v
        w.s[12], w.s[13] = CST_MEM & M32, CST_MEM >> 32
        return w

    def put_tile(self, w, t, b):
        a = self.ktab + b * TILE_BYTES
        w.lds[a:a + TILE_BYTES] = np.ascontiguousarray(self.tile(t)).view(np.uint8)

    def enter(self, w, t, b, tend, j=0):
        lane = np.arange(L, dtype=np.uint32)
        w.v[10, :] = self.ktab + b * TILE_BYTES + 8 * lane                   # xa
        w.v[11, :] = w.v[10, :] + NV * K * 64 * 8                           # vts
        w.s[0], w.s[1], w.s[3] = j, t, tend
        w.s[2] = (-TILE_BYTES if b else TILE_BYTES) & M32
        w.run_core(self.lines)
        assert w.exec == (1 << 64) - 1 and w.m0 == 0x1234, "EXEC / M0 not restored"
        return int(w.s[0]), int(w.s[1])

    def acc(self, w):
        """(hi, lo)[program][lane] of the LDS accumulators."""
        a = w.lds[self.acc0:self.acc0 + P * 1024].view("<f8").reshape(P, 2, 64)
        return a.copy()

    def per_tile(self, skip=()):
        """The per-tile loop: one core entry per tile (TEND = 0), the tile
        staged in buffer t & 1, the accumulators carried in LDS."""
        w = self.wave()
        for t in range(NTILES):
            self.put_tile(w, t, t & 1)
            j = 0
            while True:
                j, tt = self.enter(w, t, t & 1, 0, j)
                assert tt == t
                if j >= P:
                    break
                assert (t, j) in skip, (t, j)       # the caller's finish: redo pair
                j += 1
        assert w.barriers == 0 and not w.dma
        return self.acc(w)


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)).all()


def test_resident_stretch_equals_three_single_tile_entries(core):
    s = Setup(core)
    ref = s.per_tile()
    w = s.wave()
    s.put_tile(w, 0, 0)
    s.put_tile(w, 1, 1)                  # the caller issued tile 1's copy before tile 0 ran
    j, t = s.enter(w, 0, 0, NTILES)
    assert (j, t) == (P, NTILES - 1)
    assert w.barriers == NTILES - 1
    # tile 2 was copied into buffer 0 (column by column) at the first change,
    # nothing after the second; XA / VTS ended in tile 2's buffer
    cols = s.cols.shape[1] * 8
    assert w.dma == [(COL_MEM + i * cols + 2 * 1024, s.ktab + 1024 * i) for i in range(NV + NT)]
    assert int(w.v[10, 5]) == s.ktab + 40 and int(w.s[2]) == TILE_BYTES
    assert int(w.v[11, 5]) == s.ktab + 40 + NV * 1024
    got = s.acc(w)
    assert same_bits(got, ref)
    # program 0 (no sin/cos) against numpy: the epilogue's Fast2Sum on (max, min)
    hi, lo = np.zeros(64), np.zeros(64)
    for t in range(NTILES):
        x = s.tile(t).reshape(NV + NT, K, 64)
        for k in range(K):
            d = (x[0, k] + x[1, k]) - x[3, k]
            sq = d * d
            ns = hi + sq
            lo = lo + (np.minimum(hi, sq) - (ns - np.maximum(hi, sq)))
            hi = ns
    assert same_bits(got[0, 0], hi) and same_bits(got[0, 1], lo)
    assert np.isfinite(got).all() and (got[:, 0] > 0).all()


def test_finish_exit_in_the_middle_tile_and_reentry(core):
    # case 1 * 128 + 70: tile 1, chain 1, lane 6 of column x2 -> program 1's sin
    s = Setup(core, inf_case=128 + 70)
    ref = s.per_tile(skip={(1, 1), (1, 2)})
    w = s.wave()
    s.put_tile(w, 0, 0)
    s.put_tile(w, 1, 1)
    j, t = s.enter(w, 0, 0, NTILES)
    # program 1 of tile 1 leaves for finish: VRED holds the inf's high word
    assert (j, t) == (1, 1) and w.barriers == 1
    vred = core["g"].VRED
    assert int(w.v[vred].max()) >= 0x7ff00000 and int(w.v[vred, 6]) >= 0x7ff00000
    # the caller's finish lists the (program, tile) pair; re-entry at program 2
    j, t = reenter(s, w, 2)
    # program 2 = cos(x1 + x2) meets the same inf: out again, same tile
    assert (j, t) == (2, 1) and w.barriers == 1
    j, t = reenter(s, w, 3)              # past the last program: straight to the tile change
    assert (j, t) == (P, NTILES - 1) and w.barriers == NTILES - 1
    got = s.acc(w)
    # (the skipped pairs added nothing: programs 1 and 2 hold tiles 0 and 2)
    assert same_bits(got, ref) and np.isfinite(got).all()


def reenter(s, w, j):
    """The caller's re-entry after finish: every in/out operand as the core
    left it, the program index moved on."""
    w.s[0] = j
    w.run_core(s.lines)
    assert w.exec == (1 << 64) - 1 and w.m0 == 0x1234
    return int(w.s[0]), int(w.s[1])


def test_single_tile_entry_takes_no_barrier(core):
    """TEND = 0 (GPE_TILE_LOOP=0, a partial or non-lean tile): the core is
    the per-tile one."""
    s = Setup(core)
    w = s.wave()
    s.put_tile(w, 1, 1)
    assert s.enter(w, 1, 1, 0) == (P, 1)
    assert w.barriers == 0 and not w.dma and int(w.s[2]) == (-TILE_BYTES) & M32
    # a wave without programs in a stretch still takes every barrier
    w = s.wave()
    w.s[int(SREG["nmine"][1:])] = 0
    s.put_tile(w, 0, 0)
    assert s.enter(w, 0, 0, NTILES) == (0, NTILES - 1)
    assert w.barriers == NTILES - 1 and len(w.dma) == NV + NT


def test_barrier_check_on_the_emitted_text(core):
    gen, g, lines = core["gen"], core["g"], core["lines"]
    saved = g.sp(g.SMASK)
    gen.check_tile_loop(lines, saved, g.SJ)
    i = lines.index("s_barrier")

    def broken(new):
        with pytest.raises(AssertionError):
            gen.check_tile_loop(new, saved, g.SJ)
    broken(lines[:i] + lines[i + 1:])                              # no barrier
    broken(lines[:i] + ["s_barrier"] + lines[i:])                  # two on the path
    broken(lines[:i] + ["s_mov_b64 exec, vcc"] + lines[i:])        # EXEC changed
    # a second barrier on one of the two ways round the DMA
    k = lines.index(".Ltile_dma_%=:")
    broken(lines[:k] + ["s_barrier"] + lines[k:])
    # leaving the core after the barrier (a wave would miss the next one)
    k = lines.index("s_cbranch_scc0 .Ltile_run_%=")
    broken(lines[:k] + ["s_cbranch_scc0 .Lend_%="] + lines[k + 1:])
    # the tile change without the program index reset
    k = lines.index("s_mov_b32 s%d, 0" % g.SJ)
    broken(lines[:k] + lines[k + 1:])
    # another way into .Ltile
    k = lines.index(".Lskip_%=:")
    broken(lines[:k + 1] + ["s_cbranch_scc1 .Ltile_%="] + lines[k + 1:])
