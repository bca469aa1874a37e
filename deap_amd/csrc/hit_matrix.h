// Part of gpeval.hip's single translation unit (included there once, ahead of
// case_bits.h, whose gpe_lexicase_bits is the first user): the 0/1 hit matrix
// a call means, and how it reaches the device in the layout the call's kernel
// reads.  Every consumer of the matrix —
// gpe_lexicase_bits, gpe_lexicase_bits_par, gpe_informed_cases,
// gpe_hit_group_counts, gpe_case_solve_counts, gpe_hit_weighted_sums,
// gpe_hit_shared_sums — resolves it here and nowhere else.
//
// Three routes:
//   caller       planes != NULL: the caller's host matrix uint32[n][units],
//                uploaded to d_lexb_in (Q: d_lexb_q).  A matrix of no rows is
//                still the caller's.
//   resident     planes == NULL: d_hit of the last hit-planes run of the loaded
//                programs (gpe_run_hit_planes on the B machine,
//                gpe_run_typed_hit_planes on the F machine).  Q is d_hit_t, made
//                by the first call that wants it and kept (hit_t_valid) until
//                the next run.
//   thresholded  planes == NULL on an F context without hit planes, for the
//                calls that take an eps (informed_cases and the three case-weight
//                calls): d_case_out of the last per-case run, e <= eps and
//                finite, into d_inf_hit (Q: d_inf_q) — scratch of the call, so
//                d_case_out, d_hit and hit_valid stay as they are and the next
//                call may name another eps.  The lexicase and group-count calls
//                have no eps to threshold by and take the first two routes only:
//                to them such a context has no hit planes (GPE_E_STATE).
//
// Two steps, because every entry point checks its own arguments (with its own
// codes and words) between learning the resident sizes and touching the
// device:
//   hit_matrix_which   decides the route, makes the state checks (and the eps
//                      check of the thresholded route) and fills in n / n_cases
//                      of the resident routes.  Touches nothing.
//   hit_matrix_device  after the caller's checks, for n >= 1: ensures the
//                      buffers, sends the planes (if the caller's) and the
//                      call's other host inputs in ONE staged copy (none when
//                      there is nothing to send), thresholds and / or
//                      transposes.  H is always there afterwards, Q when asked
//                      for: a call that reads H alone makes no Q and is not held
//                      to the n <= 2^31 - 1 of the calls that index programs in
//                      Q with an int32.
#pragma once
namespace {

constexpr int kInfBlock = 256;              // 4 waves (case_informed.h's kernels too)

// E double[n][C] (absolute errors) into hit planes H uint32[n][units]: bit
// c % 32 of word c / 32 is e <= eps for a finite e (nan and inf never hit, also
// with eps = inf), pad bits 0.  A wave takes one program and 32 stretches of 64
// cases: a ballot per stretch gives two words, kept by lanes 2 s and 2 s + 1,
// and the wave then stores its 64 words side by side.
__global__ __launch_bounds__(kInfBlock) void hit_threshold(const double* __restrict__ E,
                                                           int64_t n, int64_t C, int64_t units,
                                                           double eps, uint32_t* __restrict__ H) {
  const int lane = threadIdx.x & 63;
  const int64_t chunks = (units + 63) / 64;
  const int64_t total = n * chunks;
  for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < total;
       item += (int64_t)gridDim.x * 4) {
    const int64_t p = item / chunks, ch = item - p * chunks;
    const double* row = E + p * C;
    const int64_t c0 = ch * 2048;
    unsigned long long mine = 0;
    for (int s = 0; s < 32 && c0 + (int64_t)s * 64 < C; ++s) {
      const int64_t c = c0 + (int64_t)s * 64 + lane;
      bool h = false;
      if (c < C) {
        const double e = row[c];
        h = e <= eps && e - e == 0.0;               // (inf - inf and nan - nan are nan)
      }
      const unsigned long long m = __builtin_amdgcn_ballot_w64(h);
      if ((lane >> 1) == s) mine = m;
    }
    const int64_t w = ch * 64 + lane;
    if (w < units) H[p * units + w] = (uint32_t)(mine >> (32 * (lane & 1)));
  }
}

// H uint32[n][units] (device) into Q uint64[32 units][W] (case_bits.h, beside
// its kernel)
int launch_hit_transpose(gpe_ctx* ctx, const uint32_t* H, int64_t n, int64_t units,
                         unsigned long long* Q);

}  // namespace

// (gpeval.hip includes this inside its extern "C" block, where a function of
// an unnamed namespace still lands in the dynamic symbol table: the helpers
// below get C++ linkage and stay out of it)
extern "C++" {
namespace {

// E double[n][n_cases] (device) into H uint32[n][units]
int launch_hit_threshold(gpe_ctx* ctx, const double* E, int64_t n, int64_t n_cases,
                         int64_t units, double eps, uint32_t* H) {
  const int64_t items = n * ((units + 63) / 64);
  const unsigned gx = (unsigned)std::min<int64_t>((items + 3) / 4, 65536);
  hipLaunchKernelGGL(hit_threshold, dim3(gx), dim3(kInfBlock), 0, ctx->stream, E, n, n_cases,
                     units, eps, H);
  HIPCHK(hipGetLastError());
  return 0;
}

enum HitRoute { kHitCaller, kHitResident, kHitThresholded };

struct HitMatrix {
  // hit_matrix_which
  HitRoute route = kHitCaller;
  const uint32_t* planes = nullptr;          // the caller's (host)
  double eps = 0.0;                          // of the thresholded route
  int64_t n = 0, n_cases = 0;
  // hit_matrix_device
  int64_t units = 0, W = 0;                  // ceil(n_cases / 32), ceil(n / 64)
  const uint32_t* H = nullptr;               // program-major uint32[n][units]
  const unsigned long long* Q = nullptr;     // case-major uint64[32 units][W]
};

// Step 1 (see the head of this file).  allow_threshold: the call has an eps.
int hit_matrix_which(gpe_ctx* ctx, const char* what, const uint32_t* planes, int64_t n,
                     int64_t n_cases, bool allow_threshold, double eps, HitMatrix* m) {
  m->planes = planes;
  m->eps = eps;
  m->n = n;
  m->n_cases = n_cases;
  if (planes) {
    m->route = kHitCaller;
    return 0;
  }
  // (the F machine after a typed hit-planes run serves its planes, as the B
  // machine does; a later per-case run clears hit_valid and decides again)
  if (allow_threshold && ctx->machine == GPE_MACHINE_F && !ctx->hit_valid) {
    if (!ctx->d_case_out || ctx->n_prog <= 0 || ctx->case_stale)
      return fail(ctx, GPE_E_STATE, "no per-case values on the device");
    if (ctx->case_n != ctx->n_prog)          // (the matrix has case_n rows)
      return fail(ctx, GPE_E_STATE,
                  "no per-case values of the loaded programs on the device (another "
                  "batch was loaded since the per-case run)");
    if (!(eps >= 0.0)) {
      char buf[160];
      snprintf(buf, sizeof(buf), "%s: eps must be >= 0 (and not nan)", what);
      return fail(ctx, GPE_E_ARG, buf);
    }
    m->route = kHitThresholded;
    m->n = ctx->n_prog;
    m->n_cases = ctx->n_cases;
    return 0;
  }
  if (!ctx->hit_valid || ctx->n_prog <= 0 || ctx->hit_n != ctx->n_prog ||
      ctx->hit_cases != ctx->n_cases)
    return fail(ctx, GPE_E_STATE,
                "no hit planes of the loaded programs on the device (gpe_run_hit_planes "
                "first)");
  m->route = kHitResident;
  m->n = ctx->hit_n;
  m->n_cases = ctx->hit_cases;
  return 0;
}

// Step 2 (see the head of this file): m->n >= 1 and m->n_cases in
// 1 .. 2^31 - 1, checked by the caller (n <= 2^31 - 1 too when want_q).
// extra: up to two further host inputs of the call, their device buffers
// ensured by the caller; they travel with the planes (the staging buffer is not
// reused before the stream has read it).
int hit_matrix_device(gpe_ctx* ctx, HitMatrix* m, bool want_q, const HostPiece* extra = nullptr,
                      int n_extra = 0) {
  const int64_t n = m->n;
  const int64_t units = m->units = (m->n_cases + 31) / 32;
  m->W = (n + 63) / 64;
  const size_t words = (size_t)n * (size_t)units;
  const size_t qwords = want_q ? (size_t)units * 32 * (size_t)m->W : 0;
  HostPiece pc[3];
  int n_pc = 0;
  uint32_t* H = ctx->d_hit;
  unsigned long long** Q = &ctx->d_hit_t;
  size_t* q_cap = &ctx->hit_t_cap;
  bool make_q = want_q && !ctx->hit_t_valid;
  if (m->route == kHitCaller) {
    if (ensure(ctx, &ctx->d_lexb_in, &ctx->lexb_in_cap, words)) return GPE_E_HIP;
    pc[n_pc++] = {ctx->d_lexb_in, m->planes, words * sizeof(uint32_t)};
    H = ctx->d_lexb_in;
    Q = &ctx->d_lexb_q;
    q_cap = &ctx->lexb_q_cap;
    make_q = want_q;
  } else if (m->route == kHitThresholded) {
    if (ensure(ctx, &ctx->d_inf_hit, &ctx->inf_hit_cap, words)) return GPE_E_HIP;
    H = ctx->d_inf_hit;
    Q = &ctx->d_inf_q;
    q_cap = &ctx->inf_q_cap;
    make_q = want_q;
  }
  for (int k = 0; k < n_extra && k < 2; ++k) pc[n_pc++] = extra[k];
  if (int rc = h2d_staged(ctx, pc, n_pc)) return rc;
  if (m->route == kHitThresholded)
    if (int rc = launch_hit_threshold(ctx, ctx->d_case_out, n, m->n_cases, units, m->eps, H))
      return rc;
  if (make_q) {
    if (ensure(ctx, Q, q_cap, qwords)) return GPE_E_HIP;
    if (int rc = launch_hit_transpose(ctx, H, n, units, *Q)) return rc;
    if (m->route == kHitResident) ctx->hit_t_valid = true;
  }
  m->H = H;
  m->Q = want_q ? *Q : nullptr;
  return 0;
}

}  // namespace
}  // extern "C++"
