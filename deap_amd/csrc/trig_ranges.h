// The range pass over F-machine words: which glibc range every sin/cos
// argument of a program provably falls in, from the [min, max] of the case
// columns (gpe_set_cases).  Plain interval arithmetic along the postfix
// words, run by translate_words (host and device) while it emits a program
// for the exact cores, whose SIN_MID / COS_MID / SIN_SMALL / COS_SMALL /
// COS_MIDLO / SIN_WIDE / COS_WIDE handlers (gen_asm.py glibc_seq4(rng=...))
// run glibc's operations for that range without the tests that find it.
//
// The invariant the handlers rest on: a value that reaches a specialised
// handler is inside its range in EVERY lane — the pad lanes of a partial
// last tile (f_stage pads with 0.0: every column's bounds are hulled with
// 0.0 by the caller) and the lanes of a program that has already flagged an
// error elsewhere — or (MID, SMALL, MIDLO only) is a NaN whose program and
// tile are already handed to the C++ pass (below).  Hence the taint rule: a
// value that may be inf or nan in any lane (a division whose denominator may
// be 0, an unbounded column, a non-finite constant, a bound past 1e300) is
// "tainted", every arithmetic result computed from it is tainted, and a
// tainted argument is class general.
//
// The third state, "nanable" (kAll and kStatic): every lane is finite and
// inside the bounds, or NaN.  sin/cos of a tainted argument is nanable within [-1, 1]:
// the general handler returns glibc's value for a finite lane and NaN for an
// inf or nan one (x - x).  The state is closed under add, sub, mul, neg
// (a NaN operand gives NaN; finite operands inside their bounds give a
// result inside the hull, as for clean values), under protectedDiv while the
// denominator's interval excludes 0 (a NaN denominator is not == 0, the
// quotient is NaN; the numpy variant turns that NaN into 1.0, so its hull
// includes 1.0), and is tainted again by a denominator that may be 0 and by
// a bound past kHuge.  A nanable argument may take MID, SMALL and MIDLO, not
// WIDE (kept for clean values: its body drops the VRED update).
//   Why a NaN lane may run a specialised handler.  (1) Whatever it computes
// is discarded: NaN lanes are born only where a value turns nanable, in an
// inner sin/cos of the same program whose argument was tainted (the closed
// operations only pass a NaN on: their finite lanes stay inside the hull,
// below kHuge).  That node is class general, its lane held an inf or a nan,
// and the general handler has put |x|.hi >= 0x7ff00000 into VRED; END then
// leaves to the C++ `finish`, which hands that (program, tile) to
// f_eval_pairs.  (2) It is safe: the handlers' only memory accesses are the
// two table gathers at (u.lo << 4) + {0, S, 2 S}, u = |x| + BIG, and every
// NaN in the machine has a zero low word, which v_add_f64 keeps, so a NaN
// lane gathers entry 0: gpe_set_cases canonicalises the cases' NaNs to the
// default NaN (canon_nan), non-finite constants are tainted and so are the
// values computed from them up to the general handler that makes x - x, the
// default NaN (0x7ff8000000000000); every fp64 op propagates an operand's
// NaN (quieted, low word kept) or makes the default one; and the handlers'
// sign operations touch high words only.  The compares are false for NaN
// (the lane runs the d block and the table path, fp64 arithmetic only), and
// every path restores EXEC (gen_asm.py check_exec).  Both are executed in
// tests/test_asm_emu_ranges_more.py.
//
// Soundness of the bounds: add, sub, mul, div and neg are correctly rounded
// and therefore monotone in each operand, so the same round-to-nearest fp64
// operations applied to the endpoints bound every lane's result with no
// widening (mul, div: the hull of the four corners).  sin/cos of a bounded
// argument lie in [-1, 1]; tighter bounds carry an explicit margin (below).
// Both builds evaluate this header with -ffp-contract=off (no fused
// multiply-add), and IEEE fp64 division.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TR_HD __host__ __device__
#else
#define TR_HD
#endif

namespace trig_ranges {

// GENERAL, MID, SMALL: the base classes (kBase picks only these); MIDLO (cos
// only; kStatic: sin too) and WIDE: kAll's and kStatic's.  The numbering is
// the ABI's (gpe_last_trig_classes)
enum Class { GENERAL = 0, MID = 1, SMALL = 2, MIDLO = 3, WIDE = 4, kClasses = 5 };
// GPE_TRIG_RANGES: 0 general handlers only (no pass), 1 the base classes, 2 all,
// 3 (the default) all, MIDLO for sin too, and the MID / MIDLO handlers whose
// lane roles are static (gen_asm.py glibc_seq4(rng="mid3" / "midlo3")): the
// classes of a cos node and the values' intervals and states are mode 2's;
// 4: mode 3 without the sin MIDLO pick (mode 2's classes, mode 3's bodies:
// such a sin node is SIN_MID3's) — the A/B control of SIN_MIDLO3 alone
enum Mode { kOff = 0, kBase = 1, kAll = 2, kStatic = 3, kStaticMid = 4 };
constexpr int kSlots = 12;              // operand-stack slots (the deep cores' D)
// class thresholds on m = max(|lo|, |hi|): deliberately below glibc's own
// (|x| < 0.85546875: hx < 0x3feb6000; |x| < 2.426265...: hx < 0x400368fd)
constexpr double kSmall = 0.855, kMid = 2.42;
// cos, |x| < kMidLo: the do_sin lanes (0.85546875 <= |x|) have the argument
// a = (hp0 - |x|) + hp1 > pi/2 - 1.44 = 0.13080 > 0.126, TAYLOR_SIN's bound:
// a margin of 0.0048, against two roundings of 2^-53 relative.  sin (kStatic),
// |x| < kMidLo < pi/2: the do_cos lanes (0.85546875 <= |x|) have t = hp0 - |x|
// > 0.13 > 0, so do_cos(t, hp1) never negates hp1: it is an operand, not a
// register
constexpr double kMidLo = 1.44;
// |x| < kWide, clean: below __branred's 105414350 (hx < 0x419921fb) by 5 %
constexpr double kWide = 1e8;
constexpr double kHuge = 1e300;         // a bound past it: tainted

// opcodes of the flattener words this pass reads (lower_core.h / gpeval.hip)
enum : uint32_t {
  W_END = 0, W_LDV = 1, W_LDC = 2, W_PUSH = 3, W_PUSHV = 4, W_PUSHC = 5,
  W_ADD = 8, W_SUB = 11, W_RSUB = 14, W_MUL = 17, W_DIV = 20, W_RDIV = 23,
  W_LT = 26, W_NEG = 48, W_SIN = 49, W_COS = 50, W_ABS = 53, W_SQRT = 54,
  W_NPDIV = 56, W_RNPDIV = 59
};

enum State : uint8_t { TAINT = 0, CLEAN = 1, NANABLE = 2 };

struct Iv {
  double lo, hi;
  State st;                             // TAINT: may be inf / nan / anything
};

TR_HD inline double absd(double v) { return v < 0 ? -v : v; }
TR_HD inline double mind(double a, double b) { return a < b ? a : b; }
TR_HD inline double maxd(double a, double b) { return a > b ? a : b; }
TR_HD inline Iv taint() { return Iv{0.0, 0.0, TAINT}; }
// (the comparisons are false for nan: tainted)
TR_HD inline Iv mk(double lo, double hi, State st = CLEAN) {
  const bool ok = st != TAINT && lo <= hi && lo >= -kHuge && hi <= kHuge;
  return ok ? Iv{lo, hi, st} : taint();
}
// both clean: clean; a tainted one: tainted; else nanable
TR_HD inline State join(const Iv& a, const Iv& b) {
  return a.st == TAINT || b.st == TAINT ? TAINT
         : a.st == CLEAN && b.st == CLEAN ? CLEAN : NANABLE;
}
TR_HD inline Iv point(double c) { return mk(c, c); }
TR_HD inline Iv add(const Iv& a, const Iv& b) {
  return mk(a.lo + b.lo, a.hi + b.hi, join(a, b));
}
TR_HD inline Iv sub(const Iv& a, const Iv& b) {       // a - b
  return mk(a.lo - b.hi, a.hi - b.lo, join(a, b));
}
TR_HD inline Iv neg(const Iv& a) { return mk(-a.hi, -a.lo, a.st); }
// |a|: the sign bit cleared in every lane (a NaN stays a NaN: state kept)
TR_HD inline Iv abs_iv(const Iv& a) {
  if (a.st == TAINT) return taint();
  return mk(maxd(0.0, maxd(a.lo, -a.hi)), maxd(absd(a.lo), absd(a.hi)), a.st);
}
// sqrt is correctly rounded, hence monotone: exact at the endpoints.  Only a
// clean argument that cannot be negative: a negative lane gives NaN (and
// ValueError), a nanable argument is not followed further
TR_HD inline Iv sqrt_iv(const Iv& a) {
  if (a.st != CLEAN || !(a.lo >= 0.0)) return taint();
  return mk(__builtin_sqrt(a.lo), __builtin_sqrt(a.hi));
}
TR_HD inline Iv hull4(double p, double q, double r, double s, State st) {
  return mk(mind(mind(p, q), mind(r, s)), maxd(maxd(p, q), maxd(r, s)), st);
}
TR_HD inline Iv mul(const Iv& a, const Iv& b) {
  const State st = join(a, b);
  if (st == TAINT) return taint();
  return hull4(a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi, st);
}
// protectedDiv(num, den): den == 0 ? 1.0 : num / den.  The numpy variant
// (inf / nan -> 1.0) agrees wherever the quotient is finite, which the bound
// check of hull4 guarantees; where it is not, both are tainted here.  A
// nanable operand: the quotient of a NaN lane is NaN (the numpy variant:
// 1.0, hulled in); a denominator that may be 0 taints, the exact 0 too.
TR_HD inline Iv pdiv(const Iv& n, const Iv& d, bool np) {
  const State st = join(n, d);
  if (st == TAINT) return taint();
  if (st == CLEAN && d.lo == 0.0 && d.hi == 0.0) return point(1.0);
  if (d.lo <= 0.0 && d.hi >= 0.0) return taint();    // may divide by ~0: +-inf
  const Iv q = hull4(n.lo / d.lo, n.lo / d.hi, n.hi / d.lo, n.hi / d.hi, st);
  if (q.st == NANABLE && np) return mk(mind(q.lo, 1.0), maxd(q.hi, 1.0), NANABLE);
  return q;
}

// The class of a sin (cos) node from its argument; `mode` kBase, kAll or
// kStatic.
TR_HD inline int classify(const Iv& a, bool cos, int mode) {
  if (a.st == TAINT) return GENERAL;
  const double m = maxd(absd(a.lo), absd(a.hi));
  if (m < kSmall) return SMALL;
  if ((mode == kStatic || (mode >= kAll && cos)) && m < kMidLo) return MIDLO;
  if (m < kMid) return MID;
  return mode >= kAll && a.st == CLEAN && m < kWide ? WIDE : GENERAL;
}
// The class kBase gives the same node (a value is clean exactly when kBase
// calls it untainted, with the same bounds: nanable values never turn clean)
TR_HD inline int base_class(const Iv& a) {
  return a.st == CLEAN ? classify(a, false, kBase) : GENERAL;
}

// Upper bound of glibc's sin(t) for 0 <= t <= 1.5: the Taylor polynomial
// t - t^3/6 + t^5/120 is above sin t there (the next term, -t^7/5040, is
// negative and dominates the rest), glibc's sin is within one ulp (2^-52
// relative) of sin t, and this evaluation's rounding errors are a few ulps:
// the relative 2^-40 widening covers both with a margin of 2^10.  (glibc is
// not monotone to the last ulp, so the unwidened value is never used.)
TR_HD inline double sin_ub(double t) {
  const double t2 = t * t;
  const double p = t - t * t2 * (1.0 / 6.0) + t * t2 * t2 * (1.0 / 120.0);
  return mind(1.0, p * (1.0 + 0x1p-40));
}
// (a tainted argument, kAll: finite lanes give a value in [-1, 1], inf and
// nan lanes NaN — nanable; kBase: tainted)
TR_HD inline Iv sin_iv(const Iv& a, int mode) {
  if (a.st == TAINT) return mode >= kAll ? mk(-1.0, 1.0, NANABLE) : taint();
  if (a.lo < -1.5 || a.hi > 1.5) return mk(-1.0, 1.0, a.st);
  // on [-1.5, 1.5] sin is odd and has the sign of its argument (glibc's
  // too: it computes sin |x| and restores the sign)
  return mk(a.lo < 0.0 ? -sin_ub(-a.lo) : 0.0, a.hi > 0.0 ? sin_ub(a.hi) : 0.0, a.st);
}
// Lower bound of glibc's cos for |x| <= m <= 1.25: cos x >= 1 - x^2/2 >=
// 1 - m^2/2 (>= 0.21 there); narrowed by a relative 2^-40 for glibc's ulp
// and this evaluation's roundings, as above.
TR_HD inline Iv cos_iv(const Iv& a, int mode) {
  if (a.st == TAINT) return mode >= kAll ? mk(-1.0, 1.0, NANABLE) : taint();
  const double m = maxd(absd(a.lo), absd(a.hi));
  if (m > 1.25) return mk(-1.0, 1.0, a.st);
  return mk((1.0 - m * m * 0.5) * (1.0 - 0x1p-40), 1.0, a.st);
}

// The walk: T and the stack slots' intervals.  `bnd` holds (lo, hi) per
// column, nb columns; a column past nb, or a slot past kSlots, is tainted.
struct Walk {
  const double* bnd;
  int nb;
  int mode;
  int base;                             // base_class of the last sin/cos node
  Iv T;
  Iv S[kSlots];

  TR_HD Walk(const double* b, int n, int m = kBase)
      : bnd(b), nb(n), mode(m), base(GENERAL), T(taint()) {
    for (int i = 0; i < kSlots; ++i) S[i] = taint();
  }
  TR_HD Iv var(uint32_t x) const {
    return (int)x < nb ? mk(bnd[2 * x], bnd[2 * x + 1]) : taint();
  }
  TR_HD Iv slot(uint32_t d) const { return d < (uint32_t)kSlots ? S[d] : taint(); }
  TR_HD void push(uint32_t d) {
    if (d < (uint32_t)kSlots) S[d] = T;
  }
  // One instruction word (c0, c1: the two words after it, read only when the
  // op takes an inline constant).  Returns the class of a sin/cos node (and
  // sets `base`), -1 for any other op.
  TR_HD int step(uint32_t word, uint32_t c0, uint32_t c1) {
    const uint32_t op = word & 0xffu, d = (word >> 8) & 0xffu, x = word >> 16;
    const Iv K = point(__builtin_bit_cast(double, (uint64_t)c0 | ((uint64_t)c1 << 32)));
    if (op == W_LDV) {
      T = var(x);
    } else if (op == W_LDC) {
      T = K;
    } else if (op == W_PUSH) {
      push(d);
    } else if (op == W_PUSHV) {
      push(d);
      T = var(x);
    } else if (op == W_PUSHC) {
      push(d);
      T = K;
    } else if (op == W_NEG) {
      T = neg(T);
    } else if (op == W_ABS) {
      T = abs_iv(T);
    } else if (op == W_SQRT) {
      T = sqrt_iv(T);
    } else if (op == W_SIN || op == W_COS) {
      const int c = classify(T, op == W_COS, mode);
      base = base_class(T);
      T = op == W_SIN ? sin_iv(T, mode) : cos_iv(T, mode);
      return c;
    } else if ((op >= W_ADD && op < W_LT) || (op >= W_NPDIV && op < W_NPDIV + 6)) {
      // T = fam(a, T): add, sub (a - T), rsub (T - a), mul, div
      // (protectedDiv(a, T)), rdiv (protectedDiv(T, a)); the numpy pair alike
      const bool np = op >= W_NPDIV;
      const int fam = np ? 4 + (int)(op - W_NPDIV) / 3 : (int)(op - W_ADD) / 3;
      const int form = np ? (int)(op - W_NPDIV) % 3 : (int)(op - W_ADD) % 3;
      const Iv a = form == 0 ? slot(d) : form == 1 ? var(x) : K;
      T = fam == 0 ? add(a, T) : fam == 1 ? sub(a, T) : fam == 2 ? sub(T, a)
          : fam == 3 ? mul(a, T) : fam == 4 ? pdiv(a, T, np) : pdiv(T, a, np);
    } else {
      T = taint();                      // an op this pass does not model
    }
    return -1;
  }
};

}  // namespace trig_ranges
