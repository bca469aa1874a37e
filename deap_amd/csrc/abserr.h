// Part of gpeval.hip's single translation unit (included there once, before
// fb_kernels.h and asm_kernels.h): the abs-error run's arithmetic — the
// per-case accumulation (abserr::accumulate, one function for the asm
// epilogue, the rows kernel and the host twin), the merge of two partial
// results, the group reduction (reduce_groups_abserr), the row reduction
// (abserr_rows) and the host twin of that row reduction (abserr::host_row).
//
// A program's abs-error words over the cases, with e = |f - t0 - t1 - ...|:
//   sum e as a double-double (hi, lo), max e, and the hits: the cases with
//   e <= hit_eps (a nan or inf e is never a hit, whatever hit_eps is).
// The max ignores nan; a nan e raises GPE_FLAG_NAN_TERM and an inf e
// GPE_FLAG_INF_TERM (both with GPE_FLAG_NONFINITE_TERM), and the caller reads
// the result's max and mean from the flags.
#pragma once

namespace abserr {

// (as two_sum / dd_add of the device and h_two_sum / h_dd_add of the host:
// the same operations in the same order)
HD void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
  if (!__builtin_isfinite(s)) e = 0.0;
}

HD void dd_add(double& hi, double& lo, double bhi, double blo) {
  double s, e;
  two_sum(hi, bhi, s, e);
  e = e + (lo + blo);
  const double h = s + e;
  double l = e - (h - s);
  if (!__builtin_isfinite(h)) l = 0.0;
  hi = h;
  lo = l;
}

// the four words of a partial result; hits is a count held as a double
// (exact to 2^53 cases), so a partial is four doubles wherever it is kept
struct Part {
  double hi, lo, mx, hits;
};

// One valid case's difference d into a partial: the caller leaves pad lanes
// out.  flag collects the GPE_FLAG_*_TERM bits.
HD void accumulate(Part& p, uint32_t& flag, double d, double hit_eps) {
  const double e = __builtin_fabs(d);
  if (!(e < __builtin_inf()))
    flag |= GPE_FLAG_NONFINITE_TERM | (e != e ? GPE_FLAG_NAN_TERM : GPE_FLAG_INF_TERM);
  double s, r;
  two_sum(p.hi, e, s, r);
  p.hi = s;
  p.lo = p.lo + r;
  if (e > p.mx) p.mx = e;
  if (e <= hit_eps && e < __builtin_inf()) p.hits += 1.0;
}

// One case's absolute error as a cases run keeps it (gpe_run_abserr_cases:
// the asm epilogue, the rows kernel and the host twin): |d|, and the default
// nan at a case whose call raised (verr: the cores' ValueError bit; a values
// row already holds nan there, so the rows route and the host pass false).
HD double case_error(double d, bool verr) {
  return verr ? __builtin_nan("") : __builtin_fabs(d);
}

// partial b into partial a (the cross-lane, cross-thread and cross-group
// steps): add, max, add
HD void merge(Part& a, const Part& b) {
  dd_add(a.hi, a.lo, b.hi, b.lo);
  if (b.mx > a.mx) a.mx = b.mx;
  a.hits += b.hits;
}

// The rows kernel's order on the host: 256 strided partials of one row of
// per-case values f (terms[n_terms][n_cases] subtracted left to right), then
// the same fixed tree.
inline void host_row(const double* f, const double* terms, int64_t n_terms, int64_t n_cases,
                     double hit_eps, double* out4, uint32_t* flags) {
  Part sh[256] = {};
  uint32_t flag = 0;
  for (int t = 0; t < 256; ++t)
    for (int64_t c = t; c < n_cases; c += 256) {
      double d = f[c];
      for (int64_t q = 0; q < n_terms; ++q) d = d - terms[q * n_cases + c];
      accumulate(sh[t], flag, d, hit_eps);
    }
  for (int m = 128; m >= 1; m >>= 1)
    for (int t = 0; t < m; ++t) merge(sh[t], sh[t + m]);
  out4[0] = sh[0].hi;
  out4[1] = sh[0].lo;
  out4[2] = sh[0].mx;
  out4[3] = sh[0].hits;
  if (flags) *flags = flag;
}

}  // namespace abserr

namespace {

// the abs-error kernels' partials [group][slot][4] into the programs' four
// words, groups in ascending order (as reduce_groups)
__global__ __launch_bounds__(256) void reduce_groups_abserr(
    const double* part, int64_t n_slots, int n_groups, const int32_t* slot_prog,
    double* out4) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const int prog = slot_prog[s];
  if (prog < 0) return;
  abserr::Part r{};
  for (int g = 0; g < n_groups; ++g) {
    const double* p = part + ((size_t)g * n_slots + s) * 4;
    abserr::merge(r, abserr::Part{p[0], p[1], p[2], p[3]});
  }
  double* o = out4 + (size_t)prog * 4;
  o[0] = r.hi;
  o[1] = r.lo;
  o[2] = r.mx;
  o[3] = r.hits;
}

// The abs-error words of one row of per-case values, one block per row, in a
// fixed order (as moments_rows): each thread a strided partial, then a fixed
// tree.  Block b takes program list[b], whose row is rows[list[b] - p0] (a
// chunk of the rows route); terms[n_terms][n_cases] are the staged term
// columns.  The program's flags are written, not or-ed: a program the asm
// kernels left for a redo tile is computed here from its first case on.
// (One body, two kernels: abserr_rows, and abserr_rows_cases for a cases run.)
template <bool CASES>
__device__ __forceinline__ void abserr_rows_body(const double* __restrict__ rows,
                                                 int64_t n_cases,
                                                 const double* __restrict__ terms,
                                                 int n_terms, double hit_eps, int64_t p0,
                                                 const int32_t* __restrict__ list,
                                                 double* __restrict__ out4,
                                                 uint32_t* __restrict__ flags,
                                                 double* __restrict__ case_out) {
  __shared__ abserr::Part sh[256];
  __shared__ uint32_t shflag;
  const int64_t prog = list[blockIdx.x];
  const double* r = rows + (size_t)(prog - p0) * (size_t)n_cases;
  if (threadIdx.x == 0) shflag = 0;
  abserr::Part acc{};
  uint32_t flag = 0;
  for (int64_t c = threadIdx.x; c < n_cases; c += 256) {
    double d = r[c];
    for (int q = 0; q < n_terms; ++q) d = d - terms[(size_t)q * (size_t)n_cases + c];
    abserr::accumulate(acc, flag, d, hit_eps);
    // (the matrix is indexed by the program's own number: only `rows` is
    // relative to the chunk)
    if constexpr (CASES)
      case_out[(size_t)prog * (size_t)n_cases + c] = abserr::case_error(d, false);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (flag) atomicOr(&shflag, flag);
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) {
      abserr::Part a = sh[threadIdx.x];
      abserr::merge(a, sh[threadIdx.x + m]);
      sh[threadIdx.x] = a;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* o = out4 + (size_t)prog * 4;
    o[0] = sh[0].hi;
    o[1] = sh[0].lo;
    o[2] = sh[0].mx;
    o[3] = sh[0].hits;
    flags[prog] = shflag;
  }
}

__global__ __launch_bounds__(256) void abserr_rows(const double* __restrict__ rows,
                                                   int64_t n_cases,
                                                   const double* __restrict__ terms,
                                                   int n_terms, double hit_eps, int64_t p0,
                                                   const int32_t* __restrict__ list,
                                                   double* __restrict__ out4,
                                                   uint32_t* __restrict__ flags) {
  abserr_rows_body<false>(rows, n_cases, terms, n_terms, hit_eps, p0, list, out4, flags,
                          nullptr);
}

// A cases run's rows kernel: the same reduction, and each case's |d| into
// case_out[n_prog][n_cases] at the program's own row.
__global__ __launch_bounds__(256) void abserr_rows_cases(
    const double* __restrict__ rows, int64_t n_cases, const double* __restrict__ terms,
    int n_terms, double hit_eps, int64_t p0, const int32_t* __restrict__ list,
    double* __restrict__ out4, uint32_t* __restrict__ flags, double* __restrict__ case_out) {
  abserr_rows_body<true>(rows, n_cases, terms, n_terms, hit_eps, p0, list, out4, flags,
                         case_out);
}

}  // namespace
