// Part of gpeval.hip's single translation unit (included there once, after
// select_dev.h): the moments run's device side — the row reduction
// (moments_rows), the final formula (scaled_from_moments, one function for
// the device and the host) and the kernel that applies it (scaled_rows).
//
// A program's moments over the cases are Sf = sum f, Sff = sum f^2 and
// Sfy = sum f y, each kept as a double-double (hi, lo).  With the target's own
// Sy = sum y and Syy = sum y^2 they give the error of the best affine fit
// a + b f to y (linear scaling, Keijzer 2003):
//   vf = Sff - Sf^2 / n   vy = Syy - Sy^2 / n   cfy = Sfy - Sf Sy / n
//   b = cfy / vf   a = (Sy - b Sf) / n   mse = (vy - cfy^2 / vf) / n
// and b = 0, a = Sy / n, mse = vy / n for a constant program.  Two rules are
// part of the definition: a program with a non-finite output or
// one of magnitude 2^500 or more carries GPE_FLAG_MOMENT_RANGE and has
// mse = inf, b = 0, a = Sy / n; a program with n vf <= 2^-40 Sff counts as
// constant.
#pragma once

namespace mom {

struct DD {
  double h, l;
};

HD DD two_sum(double a, double b) {
  const double s = a + b;
  const double bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}

HD DD quick_two_sum(double a, double b) {   // |a| >= |b| (or a == 0)
  const double s = a + b;
  return {s, b - (s - a)};
}

// the one fused operation of the build (-ffp-contract=off): a product's
// exact low part
HD DD two_prod(double a, double b) {
  const double p = a * b;
  return {p, __builtin_fma(a, b, -p)};
}

HD DD add(DD a, DD b) {
  DD s = two_sum(a.h, b.h);
  const DD t = two_sum(a.l, b.l);
  s.l = s.l + t.h;
  s = quick_two_sum(s.h, s.l);
  s.l = s.l + t.l;
  return quick_two_sum(s.h, s.l);
}

HD DD neg(DD a) { return {-a.h, -a.l}; }
HD DD sub(DD a, DD b) { return add(a, neg(b)); }

HD DD mul(DD a, DD b) {
  DD p = two_prod(a.h, b.h);
  p.l = p.l + (a.h * b.l + a.l * b.h);
  return quick_two_sum(p.h, p.l);
}

HD DD mul_d(DD a, double b) {
  DD p = two_prod(a.h, b);
  p.l = p.l + a.l * b;
  return quick_two_sum(p.h, p.l);
}

// long division, three quotient digits
HD DD div(DD a, DD b) {
  const double q1 = a.h / b.h;
  DD r = sub(a, mul_d(b, q1));
  const double q2 = r.h / b.h;
  r = sub(r, mul_d(b, q2));
  const double q3 = r.h / b.h;
  const DD q = quick_two_sum(q1, q2);
  return add(q, DD{q3, 0.0});
}

HD bool le(DD a, DD b) { return a.h < b.h || (a.h == b.h && a.l <= b.l); }

HD double to_double(DD a) { return a.h + a.l; }

// |f| at or past this bound (or a non-finite f) puts the program under the
// range rule: 2^500, so that sum f^2 stays finite for any case count
constexpr double kRange = 0x1p500;
// n vf <= kConst * Sff: numerically constant
constexpr double kConst = 0x1p-40;

}  // namespace mom

// The definition, in double-double, from a program's six moment words
// (Sf hi, lo, Sff hi, lo, Sfy hi, lo), the case count, the target's Sy and
// Syy (hi, lo) and the program's flags.  Only the three results are rounded
// to double.
HD void scaled_from_moments(const double* m6, double n, const double* sy, const double* syy,
                            uint32_t flags, double& mse, double& a, double& b) {
  using namespace mom;
  const DD nn{n, 0.0};
  const DD Sy = quick_two_sum(sy[0], sy[1]), Syy = quick_two_sum(syy[0], syy[1]);
  const DD mean_y = div(Sy, nn);
  b = 0.0;
  a = to_double(mean_y);
  if (flags & GPE_FLAG_MOMENT_RANGE) {
    mse = __builtin_inf();
    return;
  }
  const DD vy = sub(Syy, div(mul(Sy, Sy), nn));
  // f scaled by a power of two s that brings its mean square near 1 (exact:
  // a and mse do not change, b is s times the scaled fit's), so that Sf^2 of
  // outputs near the range bound stays finite
  double s = 1.0;
  const double ms = m6[2] / n;
  if (ms >= 0x1p-1000 && ms < __builtin_inf()) s = ::ldexp(1.0, -(::ilogb(ms) / 2));
  const DD Sf = quick_two_sum(m6[0] * s, m6[1] * s),
           Sff = quick_two_sum(m6[2] * s * s, m6[3] * s * s),
           Sfy = quick_two_sum(m6[4] * s, m6[5] * s);
  const DD vf = sub(Sff, div(mul(Sf, Sf), nn));
  // (vf == 0 falls under the same comparison: Sff >= 0)
  if (le(mul(vf, nn), DD{Sff.h * kConst, Sff.l * kConst})) {
    const double v = to_double(div(vy, nn));
    mse = v > 0.0 ? v : 0.0;
    return;
  }
  const DD cfy = sub(Sfy, div(mul(Sf, Sy), nn));
  const DD B = div(cfy, vf);
  const DD A = div(sub(Sy, mul(B, Sf)), nn);
  const double v = to_double(div(sub(vy, div(mul(cfy, cfy), vf)), nn));
  mse = v > 0.0 ? v : 0.0;      // (a perfect fit may round below zero)
  a = to_double(A);
  b = to_double(B) * s;
}

namespace {

// first errors of the listed programs from one array into another
__global__ __launch_bounds__(256) void copy_entries(const int32_t* __restrict__ list, int64_t m,
                                                    const unsigned long long* __restrict__ src,
                                                    unsigned long long* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) dst[list[i]] = src[list[i]];
}

// The moments of one row of per-case values, one block per row, in a fixed
// order (as exact_rows_sum): each thread a strided double-double part of each
// of the three sums, then a fixed tree.  A product enters with its exact low
// part.  A case under the range rule contributes nothing and raises the
// program's flag (so the sums stay finite and the same from run to run).
// Block b takes program list[b], whose row is rows[list[b] - p0] (a chunk of
// the rows route: the programs of [p0, ...) the list names).
__global__ __launch_bounds__(256) void moments_rows(const double* __restrict__ rows,
                                                    int64_t n_cases,
                                                    const double* __restrict__ y,
                                                    int64_t p0, const int32_t* __restrict__ list,
                                                    double* __restrict__ out6,
                                                    uint32_t* __restrict__ flags) {
  __shared__ double sh[6][256];
  const int64_t prog = list[blockIdx.x];
  const double* r = rows + (size_t)(prog - p0) * (size_t)n_cases;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int bad = 0;
  for (int64_t c = threadIdx.x; c < n_cases; c += 256) {
    const double f = r[c];
    if (!(__builtin_fabs(f) < mom::kRange)) {      // inf, nan, huge
      bad = 1;
      continue;
    }
    const double t = y[c];
    const mom::DD ff = mom::two_prod(f, f), ft = mom::two_prod(f, t);
    dd_add(acc[0], acc[1], f, 0.0);
    dd_add(acc[2], acc[3], ff.h, ff.l);
    dd_add(acc[4], acc[5], ft.h, ft.l);
  }
  bad = __syncthreads_or(bad);
  for (int q = 0; q < 6; ++q) sh[q][threadIdx.x] = acc[q];
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) {
      for (int q = 0; q < 6; q += 2) {
        double a = sh[q][threadIdx.x], b = sh[q + 1][threadIdx.x];
        dd_add(a, b, sh[q][threadIdx.x + m], sh[q + 1][threadIdx.x + m]);
        sh[q][threadIdx.x] = a;
        sh[q + 1][threadIdx.x] = b;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 6) out6[prog * 6 + threadIdx.x] = sh[threadIdx.x][0];
  if (threadIdx.x == 0) flags[prog] = bad ? GPE_FLAG_MOMENT_RANGE : 0u;
}

// scaled_from_moments for every program, one thread each
__global__ __launch_bounds__(256) void scaled_rows(const double* __restrict__ m6, int64_t n,
                                                   double n_cases, double sy0, double sy1,
                                                   double syy0, double syy1,
                                                   const uint32_t* __restrict__ flags,
                                                   double* __restrict__ mse,
                                                   double* __restrict__ a,
                                                   double* __restrict__ b) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double sy[2] = {sy0, sy1}, syy[2] = {syy0, syy1};
  double v, va, vb;
  scaled_from_moments(m6 + i * 6, n_cases, sy, syy, flags[i], v, va, vb);
  mse[i] = v;
  a[i] = va;
  b[i] = vb;
}

}  // namespace
