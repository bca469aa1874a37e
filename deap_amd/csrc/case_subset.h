// Part of gpeval.hip's single translation unit (included there once, in
// order): case subsampling — gpe_select_cases' gather kernels and the context
// bookkeeping around them.
//
// A case subset is an index vector idx[0..m) into the cases gpe_set_cases
// uploaded (any order, duplicates allowed, m may exceed the full count).  It
// is gathered on the device into a second pair of case buffers with column
// stride m, and the context's d_X / d_terms / n_cases / n_units are pointed at
// them: every kernel, plan and pass keeps reading those four fields and runs
// on the active set as it would on a gpe_set_cases upload of the same rows.
// The full buffers stay where they are; idx == NULL points the fields back.
//
// What the context caches per case set, and what a selection does with it:
//   planned_mode   reset: tile counts, groups and the dbuf choice (n_cases
//                  even) are the active set's;
//   last_mode      reset: the resident fitness (gpe_tournament(NULL)) belongs
//                  to the previous set;
//   case_stale     set: d_case_out's rows have the previous set's stride, so
//                  gpe_lexicase(NULL) refuses until a cases run writes it;
//   case_t_valid   cleared: d_case_t is the case-major copy of that matrix
//                  (gpe_lexicase_par(NULL) transposes again after the next run);
//   hit_valid      cleared: d_hit's planes are the previous set's cases, so
//                  gpe_lexicase_bits(NULL) refuses until a hit-planes run;
//   ex_hcases      reset: the host exact pass copies the active cases back on
//                  its next need (ex_hX / ex_hT are sized from n_cases then);
//   label_true     recounted on the device from the gathered label column
//                  (count_true): a constant HITS_BOOL program's hits;
//   np_n           keyed on the count alone (numpy.sum's plan depends on
//                  nothing else): run_numpy rebuilds it when n_cases differs;
//   the programs, their threaded code, the exact pass, the lowering tables:
//                  kept — none of them depends on the cases.
// The column bounds col_bnd / d_col_bnd stay the full set's: the hull of a
// superset still proves every range class the range pass picks from it, and
// the handlers are exact in every class they are picked for, so the class
// picked for a sin/cos word may differ from the one a fresh context on the
// same rows would pick while the result bits may not.  The trig-leaf columns
// [nv_user, 3 nv_user) are not gathered: leaf_trig recomputes them from the
// gathered variable columns at the start of every run.  The LDS checks
// depend on nv alone, which a selection leaves as it is.
//
// idx is validated on the host before any launch (gpe_select_cases): the
// kernels below are never handed an index outside [0, n_full).
#pragma once
namespace {

// F machine: column blockIdx.y of the nvu variable and nt term columns, one
// thread per output element.  idx is read coalesced, the source column
// scattered, the destination written coalesced.  The full set's NaNs are
// canonical already (canon_nan) and a copy keeps them.
__global__ __launch_bounds__(256) void gather_cases_f(
    const double* __restrict__ srcX, const double* __restrict__ srcT, int nvu,
    int64_t n_full, const int64_t* __restrict__ idx, int64_t m, double* __restrict__ dstX,
    double* __restrict__ dstT) {
  const int col = (int)blockIdx.y;
  const double* s = col < nvu ? srcX + (int64_t)col * n_full : srcT + (int64_t)(col - nvu) * n_full;
  double* d = col < nvu ? dstX + (int64_t)col * m : dstT + (int64_t)(col - nvu) * m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    d[i] = s[idx[i]];
}

// B machine: plane blockIdx.y of the nv input planes and the output plane
// (the last), one thread per output word: bit b of word w is case
// idx[32 w + b] of the source plane; the pad bits of the last word are 0.
__global__ __launch_bounds__(256) void gather_cases_b(
    const uint32_t* __restrict__ srcX, const uint32_t* __restrict__ srcT, int nv,
    int64_t units_full, const int64_t* __restrict__ idx, int64_t m, int64_t units,
    uint32_t* __restrict__ dstX, uint32_t* __restrict__ dstT) {
  const int pl = (int)blockIdx.y;
  const uint32_t* s = pl < nv ? srcX + (int64_t)pl * units_full : srcT;
  uint32_t* d = pl < nv ? dstX + (int64_t)pl * units : dstT;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < units;
       w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t out = 0u;
    const int64_t c0 = w * 32;
    const int nb = (int)(m - c0 < 32 ? m - c0 : 32);
    for (int b = 0; b < nb; ++b) {
      const int64_t j = idx[c0 + b];
      out |= ((s[j >> 5] >> (uint32_t)(j & 31)) & 1u) << b;
    }
    d[w] = out;
  }
}

// The labels' truths (gpe_set_cases counts lab[c] != 0.0 on the host; a nan
// counts): block partial sums through LDS, one atomic per block.
__global__ __launch_bounds__(256) void count_true(const double* __restrict__ lab, int64_t m,
                                                  unsigned long long* __restrict__ out) {
  __shared__ unsigned int part[256];
  unsigned int t = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    t += lab[i] != 0.0 ? 1u : 0u;
  part[threadIdx.x] = t;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && part[0]) atomicAdd(out, (unsigned long long)part[0]);
}

// The context's case fields back on the full set (no-op when none is active).
// What was cached for the subset is dropped by the caller (subset_changed).
void subset_drop(gpe_ctx* ctx) {
  if (ctx->cs_m < 0) return;
  ctx->d_X = ctx->cs_full_X;
  ctx->d_terms = ctx->cs_full_terms;
  ctx->n_cases = ctx->cs_full_cases;
  ctx->n_units = ctx->cs_full_units;
  ctx->label_true = ctx->cs_full_label_true;
  ctx->cs_m = -1;
}

// The active case set changed under loaded programs: see the audit above.
void subset_changed(gpe_ctx* ctx) {
  ctx->planned_mode = -1;
  ctx->last_mode = -1;
  ctx->case_stale = true;
  ctx->case_t_valid = false;
  ctx->hit_valid = false;
  ctx->ex_hcases = false;
}

int select_cases(gpe_ctx* ctx, const int64_t* idx, int64_t m) {
  if (ctx->machine < 0) return fail(ctx, GPE_E_STATE, "gpe_set_cases not called");
  if (!idx) {
    if (ctx->cs_m >= 0) {
      subset_drop(ctx);
      subset_changed(ctx);
    }
    return 0;
  }
  if (m <= 0) return fail(ctx, GPE_E_INVALID, "select_cases: m must be at least 1");
  const int64_t n_full = ctx->cs_m >= 0 ? ctx->cs_full_cases : ctx->n_cases;
  for (int64_t i = 0; i < m; ++i)
    if (idx[i] < 0 || idx[i] >= n_full)
      return fail(ctx, GPE_E_INVALID,
                  "select_cases: idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) +
                      " is outside [0, " + std::to_string(n_full) + ")");
  // a bad index above left the previous active set intact; from here on the
  // fields name the full set until the new one is in place, so a HIP failure
  // on the way leaves the context on the full set
  if (ctx->cs_m >= 0) {
    subset_drop(ctx);
    subset_changed(ctx);
  }
  const bool F = ctx->machine == GPE_MACHINE_F;
  const int64_t units = F ? m : (m + 31) / 32;
  const int nvu = ctx->nv_user;
  const size_t unit = F ? sizeof(double) : sizeof(uint32_t);
  // (ctx->nv columns: room for the trig leaves' 2 nv_user when they are on)
  const size_t xb = (size_t)ctx->nv * (size_t)units * unit;
  const size_t tb = (size_t)(F ? ctx->nt : 1) * (size_t)units * unit;
  if (ensure(ctx, &ctx->d_cs_X, &ctx->cs_X_cap, std::max<size_t>(xb, 8)) ||
      ensure(ctx, &ctx->d_cs_terms, &ctx->cs_terms_cap, std::max<size_t>(tb, 8)) ||
      ensure(ctx, &ctx->d_cs_idx, &ctx->cs_idx_cap, (size_t)m))
    return GPE_E_HIP;
  if (!ctx->d_cs_count) HIPCHK(hipMalloc((void**)&ctx->d_cs_count, sizeof(unsigned long long)));
  {
    const HostPiece pc[1] = {{ctx->d_cs_idx, idx, (size_t)m * sizeof(int64_t)}};
    if (int rc = h2d_staged(ctx, pc, 1)) return rc;
  }
  ctx->cs_full_X = ctx->d_X;
  ctx->cs_full_terms = ctx->d_terms;
  ctx->cs_full_cases = ctx->n_cases;
  ctx->cs_full_units = ctx->n_units;
  ctx->cs_full_label_true = ctx->label_true;
  const int cols = F ? nvu + ctx->nt : nvu + 1;
  const unsigned gx = (unsigned)std::min<int64_t>((units + 255) / 256, 65536);
  if (cols > 0 && cols <= 65535) {
    if (F)
      hipLaunchKernelGGL(gather_cases_f, dim3(gx, (unsigned)cols), dim3(256), 0, ctx->stream,
                         (const double*)ctx->cs_full_X, (const double*)ctx->cs_full_terms, nvu,
                         ctx->cs_full_cases, (const int64_t*)ctx->d_cs_idx, m,
                         (double*)ctx->d_cs_X, (double*)ctx->d_cs_terms);
    else
      hipLaunchKernelGGL(gather_cases_b, dim3(gx, (unsigned)cols), dim3(256), 0, ctx->stream,
                         (const uint32_t*)ctx->cs_full_X, (const uint32_t*)ctx->cs_full_terms,
                         nvu, ctx->cs_full_units, (const int64_t*)ctx->d_cs_idx, m, units,
                         (uint32_t*)ctx->d_cs_X, (uint32_t*)ctx->d_cs_terms);
    HIPCHK(hipGetLastError());
  } else if (cols > 65535) {
    return fail(ctx, GPE_E_INVALID, "select_cases: too many columns");
  }
  unsigned long long truths = 0;
  if (F && ctx->nt >= 1) {
    HIPCHK(hipMemsetAsync(ctx->d_cs_count, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(count_true, dim3(std::min(gx, 1024u)), dim3(256), 0, ctx->stream,
                       (const double*)ctx->d_cs_terms, m, ctx->d_cs_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&truths, ctx->d_cs_count, sizeof(truths), hipMemcpyDeviceToHost,
                          ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));   // (the idx staging is free again)
  ctx->d_X = ctx->d_cs_X;
  ctx->d_terms = ctx->d_cs_terms;
  ctx->n_cases = m;
  ctx->n_units = units;
  ctx->label_true = (int64_t)truths;
  ctx->cs_m = m;
  subset_changed(ctx);
  return 0;
}

}  // namespace
