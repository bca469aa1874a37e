"""Test helper of the handler matrix (tests/test_handler_matrix*.py): IEEE
edge data, trees built so that every handler of every asm core is executed,
the decoder that says which handlers a tree runs, and vectorised numpy twins
of the per-case reference.  Not product code.

Data (``data()``): ``X[32, n]`` float64 in two blocks.  Block A is the ordered
pair matrix over the edge set ``E``: case ``i * |E| + j`` holds ``E[i]`` in
every even column and ``E[j]`` in every odd one.  Block B has ``N_B`` cases of
32 independent columns, each value a sign times a random 53-bit mantissa times
``2**U{-1074..1023}``; 48 of its cases are planted so that column 0 / column 1
is a subnormal non-zero quotient, and about 2 % of its cells are values of
``E``.  ``|E|`` is 29, so ``n = 841 + 513 = 1354``: ten full 128-case tiles
and one of 74; the odd prefix of 1353 cases is run too.  ``benign()`` is
``Xb[32, 257]`` uniform in [0.5, 2] for the large slot trees and the moments
route.

How the flattener lowers a tree (``Flattener._emit``; R[d]: stack slot d, T:
the accumulator), which the builders rely on and the hit sets verify:

    fam(ARGw, ARGv)               LDV w; rev_V v     (rsub, rdiv; add, mul)
    fam(ARGv, neg(neg(ARGw)))     LDV w; fwd_V v     (sub, div: the two negs
                                                      cancel in the encoder)
    fam(<subtree>, c)             ...; rev_C         fam(c, ARGv): LDC; rev_V v
    fam(L, Q), need(L) >= need(Q) L at d; PUSHV d, v of Q's first leaf; Q at
                                  d + 1; fwd_S d
    fam(Q, L), need(Q) < need(L)  L at d; PUSHV d, v; Q at d + 1; rev_S d
    fam(L, sub(1.5, ARGv))        ...; PUSHC d; rsub_V v; fwd_S d

A subtree reaches slot d only under d operators whose left operands need as
many slots as it does, so a tree that uses slot d has at least 2**(d + 1)
leaves (``at_slot``).  A PUSH is always followed by a leaf load, which the
encoder merges into PUSHV / PUSHC: the plain PUSH handlers are never emitted.
"""
import math
import os
import re
import struct
import sys

import numpy as np

import predict_ref as pr
from deap_amd import _lib, configs, gp
from deap_amd.flatten import Flattener, Op

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SEED = 20261
N_B = 513
NV = 32
NV_TYPED = 64

FAMS = ["add", "sub", "rsub", "mul", "div", "rdiv", "ndiv", "nrdiv"]
TYPED_FAMS = ["add", "sub", "rsub", "mul", "div", "rdiv", "lt", "gt", "eq", "and", "or"]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


MAXSUB = _from_bits(0x000fffffffffffff)
MAXFIN = sys.float_info.max
NAN_BITS = (0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001,
            0x7ff0000000000001)          # (the last one signalling)
_E_FINITE = [0.0, -0.0, 5e-324, -5e-324, MAXSUB, -MAXSUB, 2.0 ** -1022, -(2.0 ** -1022),
             1.0, -1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 1.5, -3.0, 1.0 / 3.0,
             2.0 ** -537, -(2.0 ** -1000), 1.4916681462400413e-154,
             -1.3407807929942597e154, 2.0 ** 512, 2.0 ** 1023, MAXFIN, -MAXFIN,
             math.inf, -math.inf]
# (as bit patterns: a NaN keeps its payload and its signalling bit)
E = np.array([struct.unpack("<Q", struct.pack("<d", v))[0] for v in _E_FINITE] +
             list(NAN_BITS), dtype=np.uint64).view(np.float64)
N_A = len(E) ** 2
N = N_A + N_B
# constants of the _C forms (no inf: 1e999 parses, but the tree prints it as
# "inf", which gp.compile cannot evaluate)
CONSTS = ["5e-324", "-0.0", "-1.7976931348623157e+308", "1.5", "-3.0", "0.3333333333333333",
          "2.2250738585072014e-308", "1.7976931348623157e+308", "8.98846567431158e+307",
          "1.4916681462400413e-154"]

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------ data --
def _draw(rng, shape):
    mant = rng.integers(2 ** 52, 2 ** 53, size=shape).astype(np.float64)
    exp = rng.integers(-1074, 1024, size=shape)
    sign = np.where(rng.integers(0, 2, size=shape) == 1, -1.0, 1.0)
    return sign * np.ldexp(mant, exp - 52)


def _block_b(rng, rows):
    B = _draw(rng, (rows, N_B))
    edge = rng.random(B.shape) < 0.02
    B[edge] = E[rng.integers(0, len(E), size=int(edge.sum()))]
    return B


def data():
    """``X[32, N]`` (module docstring); the same array at every call."""
    def make():
        rng = np.random.default_rng(SEED)
        X = np.empty((NV, N))
        i, j = np.divmod(np.arange(N_A), len(E))
        X[0::2, :N_A] = E[i]
        X[1::2, :N_A] = E[j]
        B = _block_b(rng, NV)
        # planted: column 0 / column 1 subnormal and not zero
        at = rng.choice(N_B, size=48, replace=False)
        e1 = rng.integers(0, 41, size=48)
        e0 = e1 - rng.integers(1025, 1071, size=48)
        m = rng.integers(2 ** 52, 2 ** 53, size=(2, 48)).astype(np.float64)
        B[0, at] = np.ldexp(m[0], e0 - 52)
        B[1, at] = -np.ldexp(m[1], e1 - 52)
        X[:, N_A:] = B
        X.setflags(write=False)
        return X
    return cached("X", make)


def benign():
    """``Xb[32, 257]`` uniform in [0.5, 2]."""
    def make():
        Xb = np.random.default_rng(SEED + 1).uniform(0.5, 2.0, size=(NV, 257))
        Xb.setflags(write=False)
        return Xb
    return cached("Xb", make)


def data40():
    """X and eight more columns (block A: the pair again; block B: fresh
    draws) for the 40-variable evaluator."""
    def make():
        X = data()
        more = np.empty((8, N))
        more[:, :N_A] = X[:8, :N_A]
        more[:, N_A:] = _block_b(np.random.default_rng(SEED + 2), 8)
        return np.ascontiguousarray(np.vstack([X, more]))
    return cached("X40", make)


# the float32 analogue of E (fp32 mode): every value a float32
_F32_MAXSUB = float(np.float32(2.0 ** -126) - np.float32(2.0 ** -149))
_F32_MAX = float(np.finfo(np.float32).max)
E32 = np.array([0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), _F32_MAXSUB, -_F32_MAXSUB,
                2.0 ** -126, -(2.0 ** -126), 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24,
                1.5, -3.0, float(np.float32(1.0 / 3.0)), 2.0 ** -70, -(2.0 ** -120),
                2.0 ** -63, -(2.0 ** 64), 2.0 ** 64, 2.0 ** 127, _F32_MAX, -_F32_MAX,
                math.inf, -math.inf, math.nan, -math.nan])
N32 = len(E32) ** 2 + N_B
BIG32 = (3, len(E32) ** 2 + 100)          # (column, case) of the one 1e300 cell


def data32():
    """``X32[32, N32]`` for fp32 mode: the pair matrix over E32, then 513
    cases of independent float32 values (a sign, a 24-bit mantissa, an
    exponent of U{-149..127}; 2 % values of E32), and one 1e300 cell, which
    is inf as a float32."""
    def make():
        rng = np.random.default_rng(SEED + 5)
        na = len(E32) ** 2
        X = np.empty((NV, N32))
        i, j = np.divmod(np.arange(na), len(E32))
        X[0::2, :na] = E32[i]
        X[1::2, :na] = E32[j]
        shape = (NV, N_B)
        mant = rng.integers(2 ** 23, 2 ** 24, size=shape).astype(np.float64)
        B = np.where(rng.integers(0, 2, size=shape) == 1, -1.0, 1.0) * \
            np.ldexp(mant, rng.integers(-149, 128, size=shape) - 23)
        B = B.astype(np.float32).astype(np.float64)
        edge = rng.random(shape) < 0.02
        B[edge] = E32[rng.integers(0, len(E32), size=int(edge.sum()))]
        X[:, na:] = B
        assert (X.astype(np.float32).astype(np.float64) == X)[~np.isnan(X)].all()
        X[BIG32] = 1e300
        X.setflags(write=False)
        return X
    return cached("X32", make)


R_COLS = {("add", 0): 58, ("sub", 0): 59, ("sub", 1): 60, ("mul", 0): 61,
          ("protectedDiv", 0): 62, ("protectedDiv", 1): 63}


def typed_data():
    """``(Xt[64, N], labels)``: rows 0..31 are X, 32..57 the same pair on
    block A and fresh draws on block B, 58..63 Python's own ``fam(a, b)`` and
    ``fam(b, a)`` of columns (0, 1) at every case (R_COLS)."""
    def make():
        import operator
        X = data()
        Xt = np.empty((NV_TYPED, N))
        Xt[:NV] = X
        Xt[NV:58, :N_A] = X[:26, :N_A]
        Xt[NV:58, N_A:] = _block_b(np.random.default_rng(SEED + 3), 26)
        fn = {"add": operator.add, "sub": operator.sub, "mul": operator.mul,
              "protectedDiv": configs.protectedDiv}
        a, b = X[0].tolist(), X[1].tolist()
        for (fam, rev), r in R_COLS.items():
            Xt[r] = [fn[fam](y, x) if rev else fn[fam](x, y) for x, y in zip(a, b)]
        labels = np.random.default_rng(SEED + 4).integers(0, 2, size=N).astype(np.float64)
        Xt.setflags(write=False)
        return Xt, labels
    return cached("Xt", make)


# ------------------------------------------------------------ primitive sets --
def arith_pset(n=NV):
    return cached(("pset", n), lambda: configs.arith_pset(
        n, trig=False, extra=(abs, configs.psqrt, math.sqrt)))


def typed_pset():
    """spam_pset's primitives over 64 float arguments, and neg (the typed
    core has a NEG handler that spam_pset alone cannot reach)."""
    def make():
        import itertools
        import operator
        ps = gp.PrimitiveSetTyped("TYPED64", itertools.repeat(float, NV_TYPED), bool, "ARG")
        ps.addPrimitive(operator.and_, [bool, bool], bool)
        ps.addPrimitive(operator.or_, [bool, bool], bool)
        ps.addPrimitive(operator.not_, [bool], bool)
        ps.addPrimitive(operator.add, [float, float], float)
        ps.addPrimitive(operator.sub, [float, float], float)
        ps.addPrimitive(operator.mul, [float, float], float)
        ps.addPrimitive(configs.protectedDiv, [float, float], float)
        ps.addPrimitive(operator.lt, [float, float], bool)
        ps.addPrimitive(operator.eq, [float, float], bool)
        ps.addPrimitive(configs.if_then_else, [bool, float, float], float)
        ps.addPrimitive(operator.neg, [float], float)
        ps.addEphemeralConstant("rand100_hm", configs.rand100, float)
        ps.addTerminal(False, bool)
        ps.addTerminal(True, bool)
        return ps
    return cached(("pset", "typed"), make)


def numpy_pset():
    """The numpy-flavoured set over 32 arguments (ndiv / nrdiv families)."""
    def make():
        ps = gp.PrimitiveSet("NP32", NV)
        ps.addPrimitive(np.add, 2, name="add")
        ps.addPrimitive(np.subtract, 2, name="sub")
        ps.addPrimitive(np.multiply, 2, name="mul")
        ps.addPrimitive(configs.np_protectedDiv, 2, name="protectedDiv")
        ps.addPrimitive(np.negative, 1, name="neg")
        return ps
    return cached(("pset", "numpy"), make)


# ------------------------------------------------------------ tree builders --
class Fill(object):
    """Need-1 operand subtrees ``op(ARGa, ARGb)`` over ever other columns."""

    def __init__(self, nv=NV, k=0, ops=("add", "sub")):
        self.nv, self.k, self.ops = nv, k, ops

    def p(self):
        self.k += 1
        a, b = (self.k * 7) % self.nv, (self.k * 11 + 3) % self.nv
        return "%s(ARG%d, ARG%d)" % (self.ops[self.k % len(self.ops)], a, b)


def bal(k, fill, first=None):
    """A balanced tree of ``2**k`` need-1 leaves: it needs k + 1 (the
    accumulator and k slots).  *first*: its leftmost leaf, whose load is the
    program's first word."""
    if k == 0:
        return first or fill.p()
    return "%s(%s, %s)" % ("add" if k % 2 else "sub", bal(k - 1, fill, first),
                           bal(k - 1, fill))


def at_slot(d, inner, fill, need=2, ops=("add", "sub")):
    """*inner* (needing *need*) under d operators whose left operands need as
    much as it does: the flattener emits it with R[d..] free."""
    for i in range(d):
        inner = "%s(%s, %s)" % (ops[i % len(ops)], bal(need - 1, fill), inner)
        need += 1
    return inner


def random_bushy(rnd, height, nv=NV):
    """A random tree whose binary nodes have two subtrees of one height (it
    needs about ``height`` slots), unary nodes, constants and leaves mixed in."""
    if height == 0:
        return "ARG%d" % rnd.randrange(nv) if rnd.random() < 0.85 else \
            rnd.choice(("-1", "0", "1", "0.5"))
    s = "%s(%s, %s)" % (rnd.choice(("add", "sub", "mul", "protectedDiv")),
                        random_bushy(rnd, height - 1, nv), random_bushy(rnd, height - 1, nv))
    if rnd.random() < 0.15:
        s = "%s(%s)" % (rnd.choice(("neg", "abs", "psqrt", "sqrt")), s)
    return s


# the six S-form handlers of the Python families: (primitive, operands swapped)
SFORMS = [("add", 0), ("sub", 0), ("sub", 1), ("mul", 0), ("protectedDiv", 0),
          ("protectedDiv", 1)]
PRIM = {"add": "add", "sub": "sub", "mul": "mul", "protectedDiv": "protectedDiv"}


def _q(v, k, nv=NV):
    """A need-1 subtree whose first leaf is ARGv."""
    return "%s(ARG%d, ARG%d)" % (("add", "sub", "mul")[k % 3], v, (v + 1 + 2 * (k % 7)) % nv)


def s_inner(k, v, fill, nv=NV):
    """A need-2 subtree: PUSHV d, v then the k-th S-form handler at d."""
    fam, rev = SFORMS[k % 6]
    if not rev:
        return "%s(%s, %s)" % (fam, fill.p(), _q(v, k, nv))
    return "%s(%s, add(%s, %s))" % (fam, _q(v, k, nv), fill.p(), fill.p())


def other(v, nv=NV):
    """A column of the other parity, spread over the columns."""
    return (v + 1 + 2 * ((v * 5) % (nv // 2))) % nv


def deep_wrap(s, fill, i=0):
    """*s* times ``protectedDiv(<7-slot-need filler>, 0.0)`` (the int 1): the
    same value, bit for bit, from a program the deep core runs (6 slots).  The
    filler runs first: its first load is LDV (i mod 33), or LDC at 32."""
    first = "sub(0.5, ARG%d)" % (i % NV) if i % 33 == 32 else \
        "add(ARG%d, ARG%d)" % (i % 33, (i + 5) % NV)
    return "mul(%s, protectedDiv(%s, 0.0))" % (s, bal(6, fill, first))


def pair_trees(nv=NV, cols=None):
    """(a): every ``_V`` handler of every family, both operand orders."""
    out = []
    for v in (range(nv) if cols is None else cols):
        w = other(v, NV) if cols is None else other(v % NV, NV)
        for fam in ("add", "mul"):
            out.append("%s(ARG%d, ARG%d)" % (fam, w, v))
            out.append("%s(ARG%d, ARG%d)" % (fam, v, w))
        for fam in ("sub", "protectedDiv"):
            out.append("%s(ARG%d, ARG%d)" % (fam, w, v))                 # rev_V v
            out.append("%s(ARG%d, neg(neg(ARG%d)))" % (fam, v, w))       # fwd_V v
    return out


def const_trees():
    """(a): the ``_C`` forms with constants of E on both sides, and LDC."""
    out = []
    for i, c in enumerate(CONSTS):
        for j, fam in enumerate(("add", "sub", "mul", "protectedDiv")):
            v = (3 * i + j) % NV
            out.append("%s(ARG%d, %s)" % (fam, v, c))                    # rev_C
            out.append("%s(%s, neg(neg(ARG%d)))" % (fam, c, v + 1 if v % 2 == 0 else v - 1))
            if j % 2 == i % 2:
                out.append("%s(%s, ARG%d)" % (fam, c, v))                # LDC; rev_V
    return out


def unary_trees():
    """(d)"""
    return ["%s(ARG%d)" % (f, v) for f in ("neg", "abs", "psqrt", "sqrt") for v in (0, 1)]


def slot_trees_small():
    """(b): every fam_Sd, PUSHCd and PUSHVd_v for d <= 4 (five slots: the
    D = 5 core), for the full X."""
    out = []
    fill = Fill(k=100)
    for d in range(5):
        for v in range(NV):
            out.append(at_slot(d, s_inner(v + d, v, fill), fill))
        for k in range(6):
            fam, rev = SFORMS[k]
            c = "sub(%s, ARG%d)" % (CONSTS[(k + d) % len(CONSTS)], (5 * k + d) % NV)
            inner = "%s(%s, %s)" % (fam, fill.p(), c) if not rev else \
                "%s(%s, add(%s, %s))" % (fam, c, fill.p(), fill.p())
            out.append(at_slot(d, inner, fill))
    return out


def slot_tree_big(top, t, chain=8):
    """(b), (c): one tree using slots 0..top; at every slot a chain of
    *chain* PUSHV (columns ``chain * t ...``), the S-form handlers in turn
    and one PUSHC.  For Xb only (its values stay finite there)."""
    fill = Fill(k=1000 * (t + 1), ops=("add", "sub"))
    cur = s_inner(t, chain * t % NV, fill)
    need = 2
    for d in range(top, -1, -1):
        for i in range(chain):
            v = (chain * t + i) % NV
            k = d + i + t
            fam, rev = SFORMS[k % 6]
            q = _q(v, k)
            cur = "%s(%s, %s)" % ((fam, q, cur) if rev else (fam, cur, q))
        c = "sub(%s, ARG%d)" % (("1.5", "0.75", "3.0")[(d + t) % 3], (d + 3 * t) % NV)
        fam, rev = SFORMS[(d + t) % 6]
        cur = "%s(%s, %s)" % ((fam, c, cur) if rev else (fam, cur, c))
        if d:
            cur = "%s(%s, %s)" % (("add", "sub")[d % 2], bal(need - 1, fill), cur)
            need += 1
    return cur


# ------------------------------------------------------ layouts and handlers --
def layout(core):
    """The handler ids of a generated core (gp_asm_layout<core>.h)."""
    path = os.path.join(REPO, "deap_amd", "csrc", "gp_asm_layout%s.h" % core)
    text = open(path).read()
    out = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (-?\d+);", text)}
    k, d, nv = re.search(r"constexpr int K = (\d+), D = (\d+), NV = (\d+);", text).groups()
    out.update(K=int(k), D=int(d), NV=int(nv))
    return out


def fams_of(lay):
    return TYPED_FAMS if lay.get("N_FAMS", 8) == 11 else FAMS


def universe(lay):
    """Every handler of a core the matrix is about (no sin/cos, END, RELOAD)."""
    D, nv, fams = lay["D"], lay["NV"], fams_of(lay)
    u = {("LDC",), ("NEG",)}
    for f in fams:
        u |= {("BIN", f, "S", d) for d in range(D)}
        u |= {("BIN", f, "V", v) for v in range(nv)}
        u.add(("BIN", f, "C"))
    u |= {("LDV", v) for v in range(nv)}
    u |= {("PUSH", d) for d in range(D)} | {("PUSHC", d) for d in range(D)}
    u |= {("PUSHV", d, v) for d in range(D) for v in range(nv)}
    if lay["H_ABS"] >= 0:
        u |= {("ABS",), ("SQRT",)}
    if "H_NOT" in lay:
        u.add(("NOT",))
        u |= {("ITE", d) for d in range(lay["H_COUNT"] - lay["H_ITE0"])}
    return u


def name(h):
    if h[0] == "BIN":
        return "%s_%s%s" % (h[1], h[2], "" if h[2] == "C" else h[3])
    if h[0] == "PUSHV":
        return "PUSHV%d_%d" % h[1:]
    return h[0] + "".join(str(x) for x in h[1:])


def decode(lay, hid):
    """Handler id -> key (test_asm._decode, with ABS, SQRT and the typed ids)."""
    D, nv, fams = lay["D"], lay["NV"], fams_of(lay)
    for key in ("END", "RELOAD", "LDC", "NEG", "ABS", "SQRT", "NOT"):
        if lay.get("H_" + key, -1) == hid:
            return (key,)
    if lay["H_LDV0"] <= hid < lay["H_LDV0"] + nv:
        return ("LDV", hid - lay["H_LDV0"])
    if lay["H_PUSH0"] <= hid < lay["H_PUSH0"] + D:
        return ("PUSH", hid - lay["H_PUSH0"])
    if lay["H_PUSHC0"] <= hid < lay["H_PUSHC0"] + D:
        return ("PUSHC", hid - lay["H_PUSHC0"])
    if lay["H_PUSHV0"] <= hid < lay["H_PUSHV0"] + D * nv:
        r = hid - lay["H_PUSHV0"]
        return ("PUSHV", r // nv, r % nv)
    b, st = hid - lay["H_BIN0"], lay["H_FAM_STRIDE"]
    if 0 <= b < len(fams) * st:
        fam, r = fams[b // st], b % st
        if r < D:
            return ("BIN", fam, "S", r)
        if r < D + nv:
            return ("BIN", fam, "V", r - D)
        return ("BIN", fam, "C")
    if "H_ITE0" in lay and lay["H_ITE0"] <= hid < lay["H_COUNT"]:
        return ("ITE", hid - lay["H_ITE0"])
    return ("TRIG", hid)


def _takes_const(h):
    return h[0] in ("LDC", "PUSHC") or (h[0] == "BIN" and h[2] == "C")


def translator_hits(batch, nv, lay):
    """Per program, the handlers of its threaded code: the library's own
    translator run with the identity table (a word is its handler's id),
    walked as the core walks it — RELOAD jumps to the next window, a constant
    handler skips its two data words, END ends.  None: not translated."""
    table = np.arange(lay["H_COUNT"], dtype=np.uint32)
    words, starts = _lib.debug_translate(batch, nv, table)
    out = []
    for s in starts.tolist():
        if s < 0:
            out.append(None)
            continue
        pc, hit = s, set()
        while True:
            h = decode(lay, int(words[pc]))
            pc += 1
            if h[0] == "END":
                break
            if h[0] == "RELOAD":
                pc = ((pc - 1) // lay["WINDOW"] + 1) * lay["WINDOW"]
                continue
            hit.add(h)
            if _takes_const(h):
                pc += 2
        out.append(hit)
    return out


_FAM_OF_OP = {Op.ADD: "add", Op.SUB: "sub", Op.RSUB: "rsub", Op.MUL: "mul", Op.DIV: "div",
              Op.RDIV: "rdiv", Op.LT: "lt", Op.GT: "gt", Op.EQ: "eq", Op.AND: "and",
              Op.OR: "or", Op.NPDIV: "ndiv", Op.RNPDIV: "nrdiv"}


def word_hits(batch):
    """Per program, the handlers its flattener words (op, slot, index) name:
    for the cores the host translator does not serve (the typed core maps a
    word to a handler one to one, ``translate_words``)."""
    out = []
    code = batch.code.tolist()
    for i in range(len(batch.depth)):
        pc, hit = int(batch.offsets[i]), set()
        while True:
            w = code[pc]
            op, d, x = w & 0xff, (w >> 8) & 0xff, w >> 16
            pc += 1
            if op == Op.END:
                break
            base = op - (op - Op.ADD) % 3 if Op.ADD <= op < Op.NEG or op >= Op.NPDIV else op
            if base in _FAM_OF_OP:
                form = (op - base)
                h = ("BIN", _FAM_OF_OP[base]) + ((("S", d), ("V", x), ("C",))[form])
            else:
                h = {Op.LDV: ("LDV", x), Op.LDC: ("LDC",), Op.PUSH: ("PUSH", d),
                     Op.PUSHV: ("PUSHV", d, x), Op.PUSHC: ("PUSHC", d), Op.NEG: ("NEG",),
                     Op.ABS: ("ABS",), Op.SQRT: ("SQRT",), Op.NOT: ("NOT",),
                     Op.ITE: ("ITE", d)}[op]
            hit.add(h)
            if _takes_const(h):
                pc += 2
        out.append(hit)
    return out


# ------------------------------------------------------------ the tree lists --
def parse(strings, pset):
    return [gp.PrimitiveTree.from_string(s, pset) for s in strings]


ROUTES = ("fast", "deep", "cpp")


def programs(pset, strings):
    """``(trees, route, hits)`` of a float set's trees: the kernel each runs
    on by its stack slots (0: the D = 5 core, 1: the deep core, 2: the C++
    kernels) and that core's handlers in its threaded code (None: C++)."""
    def make():
        trees = parse(strings, pset)
        batch = Flattener(pset).flatten(trees)
        assert not batch.err.any()
        route = np.where(batch.depth <= 5, 0, np.where(batch.depth <= 12, 1, 2))
        if len(pset.arguments) > NV:
            return trees, route, [None] * len(trees)
        fast = translator_hits(batch, NV, layout(""))
        deep = translator_hits(batch, NV, layout("_deep"))
        return trees, route, [(fast[i], deep[i], None)[r] for i, r in enumerate(route)]
    return cached(("programs", pset.name, len(pset.arguments), len(strings), hash(tuple(strings))),
                  make)


def arith_small():
    """``(strings, classes)``: every small tree of the arithmetic set, for the
    full X — pair, constant and unary trees as they are (the D = 5 core) and
    wrapped for the deep core, and the small slot trees."""
    def make():
        fill = Fill(k=7)
        plain = [(s, "pair") for s in pair_trees()] + \
            [(s, "const") for s in const_trees()] + [(s, "unary") for s in unary_trees()]
        out = list(plain)
        out += [(deep_wrap(s, fill, i), c + "/deep") for i, (s, c) in enumerate(plain)]
        out += [(s, "slot") for s in slot_trees_small()]
        return [s for s, _ in out], [c for _, c in out]
    return cached("arith_small", make)


BIG_TOPS = [11, 11, 11, 11, 5, 6, 7, 8, 9, 10]   # top slot: 12 slots, 6 .. 11


def arith_big():
    """The large slot trees (Xb): four of 12 slots that between them hold
    every PUSHVd_v, fam_Sd and PUSHCd of the deep core, one each of 6..11
    slots, and one of 13 slots (the C++ kernel)."""
    return cached("arith_big", lambda: [slot_tree_big(top, t) for t, top in
                                        enumerate(BIG_TOPS)] + [slot_tree_big(12, 3)])


def trees40():
    """(c): pair trees of columns 32..39 (the C++ kernels: past the cores' 32)."""
    return cached("trees40", lambda: pair_trees(40, cols=range(32, 40)))


def numpy_trees():
    """ndiv / nrdiv: their _V, _C and S forms on both cores."""
    def make():
        fill = Fill(k=50)
        out = []
        for v in range(NV):
            w = other(v)
            out.append("protectedDiv(ARG%d, ARG%d)" % (w, v))                  # nrdiv_V v
            out.append("protectedDiv(ARG%d, neg(neg(ARG%d)))" % (v, w))        # ndiv_V v
        for i, c in enumerate(CONSTS):
            out.append("protectedDiv(ARG%d, %s)" % (i, c))
            out.append("protectedDiv(%s, neg(neg(ARG%d)))" % (c, i + 1))
        plain = list(out)
        out += [deep_wrap(s, fill, i) for i, s in enumerate(plain)]
        for d in range(5):
            out.append(at_slot(d, "protectedDiv(%s, %s)" % (fill.p(), _q(d, d)), fill))
            out.append(at_slot(d, "protectedDiv(%s, add(%s, %s))"
                               % (_q(d + 8, d), fill.p(), fill.p()), fill))
        return out
    return cached("numpy_trees", make)


def numpy_big():
    """ndiv_Sd / nrdiv_Sd at every slot of both cores (Xb)."""
    return cached("numpy_big", lambda: [slot_tree_big(4, 1), slot_tree_big(11, 2)])


def typed_trees():
    """(e): every handler of the typed core that a tree can reach."""
    def make():
        nv = NV_TYPED
        out = []
        fill = Fill(nv=58, k=300, ops=("add", "sub"))
        for v in range(nv):
            w = other(v % NV) if v < 58 else (v * 3) % NV
            out.append("lt(ARG%d, ARG%d)" % (w, v))                       # gt_V v
            out.append("lt(ARG%d, neg(neg(ARG%d)))" % (v, w))             # lt_V v
            out.append("eq(ARG%d, ARG%d)" % (w, v))                       # eq_V v
            out.append("eq(ARG%d, ARG%d)" % (v, w))
            # arithmetic _V handlers; on block A columns below 58 hold the
            # pair, so Python's own result column says hit or miss
            for fam in ("add", "sub", "mul", "protectedDiv"):
                for rev in ((0,) if fam in ("add", "mul") else (0, 1)):
                    # value: fam(X[w], X[v]) (rev 0) or fam(X[v], X[w])
                    a_first = (w % 2 == 0) if not rev else (v % 2 == 0)
                    r = R_COLS[(fam, 0 if fam in ("add", "mul") or a_first else 1)]
                    if v >= 58:
                        r = (v * 5) % 32
                    e = "%s(ARG%d, ARG%d)" % (fam, w, v) if not rev else \
                        "%s(ARG%d, neg(neg(ARG%d)))" % (fam, v, w)
                    out.append("%s(%s, ARG%d)" % ("eq" if v < 58 else "lt", e, r))
        # the precision pins of the issue, columns (0, 1) at every case
        for (fam, rev), r in sorted(R_COLS.items()):
            out.append("eq(%s(ARG%d, ARG%d), ARG%d)" % (fam, rev, 1 - rev, r))
        # constants, LDC, NEG, NOT, the logic families
        for i, c in enumerate(CONSTS):
            v = 2 * i + 1
            out.append("lt(ARG%d, %s)" % (v, c))                          # gt_C
            out.append("lt(%s, neg(neg(ARG%d)))" % (c, v))                # lt_C
            out.append("eq(ARG%d, %s)" % (v, c))                          # eq_C
            fam = ("add", "sub", "mul", "protectedDiv")[i % 4]
            out.append("lt(%s(ARG%d, %s), ARG%d)" % (fam, v, c, v - 1))
            out.append("lt(%s(%s, neg(neg(ARG%d))), ARG%d)" % (fam, c, v, v - 1))
            out.append("lt(%s(%s, ARG%d), ARG%d)" % (fam, c, v, v - 1))   # LDC
            out.append("not_(lt(neg(ARG%d), %s))" % (v, c))               # NEG, NOT
        for i in range(8):
            a, b = "lt(ARG%d, ARG%d)" % (i, i + 1), "eq(ARG%d, ARG%d)" % (i + 2, i + 3)
            out.append("and_(%s, %s)" % (a, b))
            out.append("or_(%s, not_(%s))" % (a, b))
            out.append("and_(%s, True)" % a)                              # and_C
            out.append("or_(%s, False)" % b)                              # or_C
            out.append("or_(and_(%s, %s), and_(not_(%s), lt(ARG%d, 1.0)))" % (a, b, a, i))
        # S forms and pushes at every slot: a float subtree at slot d ...
        for d in range(5):
            for v in range(nv):
                out.append("lt(%s, ARG%d)" % (at_slot(d, s_inner(v + d, v, fill, 58), fill),
                                              (v + 7) % nv))
            for k in range(6):
                fam, rev = SFORMS[k]
                c = "sub(%s, ARG%d)" % (CONSTS[(k + d) % len(CONSTS)], (5 * k + d) % nv)
                inner = "%s(%s, %s)" % (fam, fill.p(), c) if not rev else \
                    "%s(%s, add(%s, %s))" % (fam, c, fill.p(), fill.p())
                out.append("lt(%s, ARG%d)" % (at_slot(d, inner, fill), k))
            # ... and a bool one: lt_S, gt_S, eq_S, and_S, or_S at slot d
            for k, inner in enumerate((
                    "lt(%s, %s)" % (fill.p(), fill.p()),
                    "lt(%s, add(%s, %s))" % (fill.p(), fill.p(), fill.p()),      # gt_S
                    "eq(%s, %s)" % (fill.p(), fill.p()),
                    "and_(lt(%s, 1.0), lt(%s, ARG3))" % (fill.p(), fill.p()),
                    "or_(lt(%s, 0.5), eq(%s, ARG0))" % (fill.p(), fill.p()))):
                cur, need = inner, 2
                for i in range(d):
                    left = "lt(%s, %s)" % (bal(need - 2, fill), bal(need - 2, fill))
                    cur = "%s(%s, %s)" % (("and_", "or_")[(i + k) % 2], left, cur)
                    need += 1
                out.append(cur)
        # if_then_else at every slot it can take (R[d], R[d + 1])
        for d in range(4):
            for i in range(4):
                v = 8 * d + 2 * i
                cond = ("lt(ARG%d, ARG%d)", "eq(ARG%d, ARG%d)", "not_(lt(ARG%d, ARG%d))",
                        "and_(lt(ARG%d, 1.0), lt(ARG%d, 1.0))")[i] % (v, v + 1)
                ite = "if_then_else(%s, ARG%d, ARG%d)" % (cond, v + 2, v + 3)
                need = 3
                cur = ite
                for j in range(d):
                    cur = "%s(%s, %s)" % (("add", "sub")[j % 2], bal(need - 1, fill), cur)
                    need += 1
                out.append("lt(%s, %s)" % (cur, ("1.0", "0.0", "ARG9", "ARG12")[i]))
        return out
    return cached("typed_trees", make)


# -------------------------------------------------------------- the twins --
def _pdiv(num, den):
    with np.errstate(all="ignore"):
        den = np.asarray(den)
        zero = den == 0
        return np.where(zero, 1.0, np.divide(num, np.where(zero, 1.0, den)))


def _np_pdiv(num, den):
    with np.errstate(all="ignore"):
        q = np.divide(num, den)
        return np.where(np.isfinite(q), q, 1.0)


class Twin(object):
    """The primitives on whole columns: ``values(trees, X)`` gives
    ``(F, first)`` like ``predict_ref.values`` and ``first_errors`` (nan at
    the cases math.sqrt raises for, and the first of them).  ``dtype``
    float32: columns, constants and every operation in float32 (a constant
    is rounded once, as the fp32 translation rounds it)."""

    def __init__(self, pset, dtype=np.float64, numpy_sem=False, typed=False):
        self.pset, self.dtype = pset, dtype
        self._err = None
        self.masks = {}           # program -> its raising cases, of the last values()
        t = dtype

        def sqrt(x):
            x = np.asarray(x, dtype=t)
            self._err |= np.broadcast_to(x < 0, self._err.shape)
            return np.sqrt(x)
        self.ctx = {"__builtins__": None, "add": np.add, "sub": np.subtract,
                    "mul": np.multiply, "neg": np.negative,
                    "protectedDiv": _np_pdiv if numpy_sem else _pdiv,
                    "abs": np.abs, "psqrt": lambda x: np.sqrt(np.abs(x)), "sqrt": sqrt}
        if typed:
            self.ctx.update({"True": True, "False": False, "and_": np.logical_and,
                             "or_": np.logical_or, "not_": np.logical_not, "lt": np.less,
                             "eq": np.equal,
                             "if_then_else": lambda c, a, b: np.where(c, a, b)})

    def _const(self, s):
        # float literals as the dtype's scalars (float32: rounded once)
        if self.dtype is np.float64:
            return s
        return re.sub(r"(?<![A-Za-z_\d.])(-?\d+\.?\d*(?:e[+-]?\d+)?)(?![\w.])",
                      lambda m: "f32(%s)" % m.group(1), s)

    def values(self, trees, X):
        X = np.asarray(X)
        n = X.shape[1]
        with np.errstate(over="ignore"):        # (1e300 as a float32 is inf)
            cols = [np.ascontiguousarray(X[i], dtype=self.dtype) for i in range(X.shape[0])]
        F = np.empty((len(trees), n), dtype=self.dtype if self.dtype is np.float32
                     else np.float64)
        first = np.full(len(trees), -1, dtype=np.int64)
        ctx = dict(self.ctx)
        ctx["f32"] = np.float32
        self.masks = {}
        # (a 13-slot tree is a few hundred levels of Python's recursive eval)
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 20000))
        try:
            with np.errstate(all="ignore"):
                for i, tree in enumerate(trees):
                    self._err = np.zeros(n, dtype=bool)
                    func = eval("lambda %s: %s" % (",".join(self.pset.arguments),
                                                   self._const(str(tree))), ctx, {})
                    F[i] = np.broadcast_to(np.asarray(func(*cols)), (n,))
                    if self._err.any():
                        F[i, self._err] = np.nan
                        first[i] = int(np.argmax(self._err))
                        self.masks[i] = self._err
        finally:
            sys.setrecursionlimit(limit)
        return F, first


def typed_hits(pset, trees, X, labels):
    """hit[program, case] = ``bool(func(*row)) is bool(label)``, per case in
    plain Python (test_launch_geometry.typed_hits' formula)."""
    rows = list(zip(*np.asarray(X).tolist()))
    lab = [bool(v) for v in np.asarray(labels).tolist()]
    hit = np.zeros((len(trees), len(rows)), dtype=bool)
    for i, tree in enumerate(trees):
        func = gp.compile(tree, pset)
        hit[i] = [bool(func(*r)) is b for r, b in zip(rows, lab)]
    return hit


def typed_hits_twin(pset, trees, X, labels):
    F, _ = Twin(pset, typed=True).values(trees, X)
    return (F != 0) == (np.asarray(labels) != 0)


# ---------------------------------------------------------------- reports --
def mismatch(got, exp, strings, hits, core, route):
    """None, or the message of the first tree whose values differ from the
    reference in any bit: the tree, its handlers, the core, the route, the
    case and both bit patterns."""
    ok = pr.same_bits(got, exp)
    if ok.all():
        return None
    bad = np.flatnonzero(~ok.all(axis=1))
    i = int(bad[0])
    c = int(np.flatnonzero(~ok[i])[0])
    hs = sorted(name(h) for h in (hits[i] or ()))
    # the handlers every differing tree runs and no agreeing tree does
    sus = None
    known = [j for j in bad if hits[j] is not None]
    if known:
        sus = set.intersection(*[set(hits[j]) for j in known])
        for j in np.flatnonzero(ok.all(axis=1)):
            sus -= hits[j] or set()
    return ("%s on %s: %d of %d trees differ; handlers that every differing tree runs and "
            "no agreeing one: %s; first tree %d %s (handlers %s), %d of its "
            "cases, first case %d: got 0x%016x, expected 0x%016x"
            % (route, core, len(bad), len(strings),
               "unknown" if sus is None else " ".join(sorted(name(h) for h in sus)[:20]) or "none",
               i, strings[i][:200],
               " ".join(hs[:40]), int((~ok[i]).sum()), c,
               int(pr.bits(np.asarray(got)[i, c:c + 1])[0]),
               int(pr.bits(np.asarray(exp)[i, c:c + 1])[0])))
