// The range pass over F-machine words: which glibc range every sin/cos
// argument of a program provably falls in, from the [min, max] of the case
// columns (gpe_set_cases).  Plain interval arithmetic along the postfix
// words, run by translate_words (host and device) while it emits a program
// for the exact cores, whose SIN_MID / COS_MID / SIN_SMALL / COS_SMALL
// handlers (gen_asm.py glibc_seq4(rng=...)) run glibc's operations for that
// range without the tests that find it.
//
// The invariant the handlers rest on: a value that reaches a specialised
// handler is inside its range in EVERY lane — the pad lanes of a partial
// last tile (f_stage pads with 0.0: every column's bounds are hulled with
// 0.0 by the caller) and the lanes of a program that has already flagged an
// error elsewhere.  Hence the taint rule: a value that may be inf or nan in
// any lane (a division whose denominator may be 0, an unbounded column, a
// non-finite constant, a bound past 1e300) is "tainted", every result
// computed from it is tainted, and a tainted argument is class general.
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

enum Class { GENERAL = 0, MID = 1, SMALL = 2 };
constexpr int kSlots = 12;              // operand-stack slots (the deep cores' D)
// class thresholds on m = max(|lo|, |hi|): deliberately below glibc's own
// (|x| < 0.85546875: hx < 0x3feb6000; |x| < 2.426265...: hx < 0x400368fd)
constexpr double kSmall = 0.855, kMid = 2.42;
constexpr double kHuge = 1e300;         // a bound past it: tainted

// opcodes of the flattener words this pass reads (lower_core.h / gpeval.hip)
enum : uint32_t {
  W_END = 0, W_LDV = 1, W_LDC = 2, W_PUSH = 3, W_PUSHV = 4, W_PUSHC = 5,
  W_ADD = 8, W_SUB = 11, W_RSUB = 14, W_MUL = 17, W_DIV = 20, W_RDIV = 23,
  W_LT = 26, W_NEG = 48, W_SIN = 49, W_COS = 50, W_NPDIV = 56, W_RNPDIV = 59
};

struct Iv {
  double lo, hi;
  bool ok;                              // false: tainted (may be inf / nan)
};

TR_HD inline double absd(double v) { return v < 0 ? -v : v; }
TR_HD inline double mind(double a, double b) { return a < b ? a : b; }
TR_HD inline double maxd(double a, double b) { return a > b ? a : b; }
TR_HD inline Iv taint() { return Iv{0.0, 0.0, false}; }
// (the comparisons are false for nan: tainted)
TR_HD inline Iv mk(double lo, double hi) {
  const bool ok = lo <= hi && lo >= -kHuge && hi <= kHuge;
  return ok ? Iv{lo, hi, true} : taint();
}
TR_HD inline Iv point(double c) { return mk(c, c); }
TR_HD inline Iv add(const Iv& a, const Iv& b) {
  return a.ok && b.ok ? mk(a.lo + b.lo, a.hi + b.hi) : taint();
}
TR_HD inline Iv sub(const Iv& a, const Iv& b) {       // a - b
  return a.ok && b.ok ? mk(a.lo - b.hi, a.hi - b.lo) : taint();
}
TR_HD inline Iv neg(const Iv& a) { return a.ok ? mk(-a.hi, -a.lo) : taint(); }
TR_HD inline Iv hull4(double p, double q, double r, double s) {
  return mk(mind(mind(p, q), mind(r, s)), maxd(maxd(p, q), maxd(r, s)));
}
TR_HD inline Iv mul(const Iv& a, const Iv& b) {
  if (!a.ok || !b.ok) return taint();
  return hull4(a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi);
}
// protectedDiv(num, den): den == 0 ? 1.0 : num / den.  The numpy variant
// (inf / nan -> 1.0) agrees wherever the quotient is finite, which the bound
// check of hull4 guarantees; where it is not, both are tainted here.
TR_HD inline Iv pdiv(const Iv& n, const Iv& d) {
  if (!n.ok || !d.ok) return taint();
  if (d.lo == 0.0 && d.hi == 0.0) return point(1.0);
  if (d.lo <= 0.0 && d.hi >= 0.0) return taint();    // may divide by ~0: +-inf
  return hull4(n.lo / d.lo, n.lo / d.hi, n.hi / d.lo, n.hi / d.hi);
}

TR_HD inline int classify(const Iv& a) {
  if (!a.ok) return GENERAL;
  const double m = maxd(absd(a.lo), absd(a.hi));
  return m < kSmall ? SMALL : m < kMid ? MID : GENERAL;
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
TR_HD inline Iv sin_iv(const Iv& a) {
  if (!a.ok) return taint();
  if (a.lo < -1.5 || a.hi > 1.5) return mk(-1.0, 1.0);
  // on [-1.5, 1.5] sin is odd and has the sign of its argument (glibc's
  // too: it computes sin |x| and restores the sign)
  return mk(a.lo < 0.0 ? -sin_ub(-a.lo) : 0.0, a.hi > 0.0 ? sin_ub(a.hi) : 0.0);
}
// Lower bound of glibc's cos for |x| <= m <= 1.25: cos x >= 1 - x^2/2 >=
// 1 - m^2/2 (>= 0.21 there); narrowed by a relative 2^-40 for glibc's ulp
// and this evaluation's roundings, as above.
TR_HD inline Iv cos_iv(const Iv& a) {
  if (!a.ok) return taint();
  const double m = maxd(absd(a.lo), absd(a.hi));
  if (m > 1.25) return mk(-1.0, 1.0);
  return mk((1.0 - m * m * 0.5) * (1.0 - 0x1p-40), 1.0);
}

// The walk: T and the stack slots' intervals.  `bnd` holds (lo, hi) per
// column, nb columns; a column past nb, or a slot past kSlots, is tainted.
struct Walk {
  const double* bnd;
  int nb;
  Iv T;
  Iv S[kSlots];

  TR_HD Walk(const double* b, int n) : bnd(b), nb(n), T(taint()) {
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
  // op takes an inline constant).  Returns the class of a sin/cos node, -1
  // for any other op.
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
    } else if (op == W_SIN || op == W_COS) {
      const int c = classify(T);
      T = op == W_SIN ? sin_iv(T) : cos_iv(T);
      return c;
    } else if ((op >= W_ADD && op < W_LT) || (op >= W_NPDIV && op < W_NPDIV + 6)) {
      // T = fam(a, T): add, sub (a - T), rsub (T - a), mul, div
      // (protectedDiv(a, T)), rdiv (protectedDiv(T, a)); the numpy pair alike
      const bool np = op >= W_NPDIV;
      const int fam = np ? 4 + (int)(op - W_NPDIV) / 3 : (int)(op - W_ADD) / 3;
      const int form = np ? (int)(op - W_NPDIV) % 3 : (int)(op - W_ADD) % 3;
      const Iv a = form == 0 ? slot(d) : form == 1 ? var(x) : K;
      T = fam == 0 ? add(a, T) : fam == 1 ? sub(a, T) : fam == 2 ? sub(T, a)
          : fam == 3 ? mul(a, T) : fam == 4 ? pdiv(a, T) : pdiv(T, a);
    } else {
      T = taint();                      // an op this pass does not model
    }
    return -1;
  }
};

}  // namespace trig_ranges
