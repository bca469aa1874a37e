// Part of gpeval.hip's single translation unit (included there once, in
// order, before the exact pass): the pieces of a typed hit-planes run
// (gpe_run_typed_hit_planes, case_bits.h) that are not an interpreter kernel.
//
// The run is a GPE_MODE_HITS_BOOL run of the F machine (fp64, one label
// column) with ctx->hits_on set: every route that counts a program's matches
// bool(T) == bool(label) also stores them, one bit per case, into ctx->d_hit,
// uint32[n_prog][n_units] (case c at bit c % 32 of word c / 32, pad bits 0 —
// the B machine's layout, so everything downstream of the matrix is shared):
//   the typed core    f_eval_asm_typed_hits (asm_kernels.h): END's masks
//   the C++ kernels   f_eval<.., HPLANES> (fb_kernels.h): the count's ballots
//   constants         const_hit_planes below: the label plane or its complement
//   the exact pass    rows_hit_planes below (the device's rows) and
//                     host_row_hit_plane (the host's terms): the 0/1 terms the
//                     pass sums, packed
// popcount(row) == hits on every route.
#pragma once
namespace {

// lp[w]: the labels' truths of cases 32 w .. 32 w + 31; lp[units + w]: their
// complement on the valid cases
__global__ __launch_bounds__(256) void label_planes(const double* terms, int64_t n_cases,
                                                    int64_t units, uint32_t* lp) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= units) return;
  uint32_t t = 0, v = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t c = w * 32 + b;
    if (c >= n_cases) break;
    v |= 1u << b;
    if (terms[c] != 0.0) t |= 1u << b;
  }
  lp[w] = t;
  lp[units + w] = ~t & v;
}

// plan_mode's class 5 (kc[i] = 2 program + truthy): bool(c) true hits the
// true labels, false the others
__global__ __launch_bounds__(256) void const_hit_planes(const uint32_t* kc, int64_t n,
                                                        const uint32_t* lp, int64_t units,
                                                        uint32_t* planes) {
  const int64_t i = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (i >= n) return;
  const uint32_t e = kc[i];
  const uint32_t* src = lp + ((e & 1u) ? 0 : units);
  uint32_t* row = planes + (size_t)(e >> 1) * (size_t)units;
  for (int64_t w = threadIdx.x; w < units; w += blockDim.x) row[w] = src[w];
}

// the exact pass's rows (rows[j][c]: 1.0 where program progs[i0 + j] matches
// case c, the terms exact_rows_sum adds) into those programs' planes
__global__ __launch_bounds__(256) void rows_hit_planes(const double* rows, int64_t n_cases,
                                                       int64_t units, const int32_t* progs,
                                                       int64_t i0, uint32_t* planes) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= units) return;
  const double* r = rows + (size_t)blockIdx.y * (size_t)n_cases;
  uint32_t t = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t c = w * 32 + b;
    if (c >= n_cases) break;
    if (r[c] != 0.0) t |= 1u << b;
  }
  planes[(size_t)progs[i0 + blockIdx.y] * (size_t)units + w] = t;
}

int launch_const_hit_planes(gpe_ctx* ctx) {
  const int64_t nk = ctx->n_kc, units = (ctx->n_cases + 31) / 32;
  if (!nk) return 0;
  if (ensure(ctx, &ctx->d_lab_planes, &ctx->lab_planes_cap, (size_t)(2 * units)))
    return GPE_E_HIP;
  hipLaunchKernelGGL(label_planes, dim3((unsigned)((units + 255) / 256)), dim3(256), 0,
                     ctx->stream, (const double*)ctx->d_terms, ctx->n_cases, units,
                     ctx->d_lab_planes);
  HIPCHK(hipGetLastError());
  const int64_t gx = std::min<int64_t>(nk, 32768);
  hipLaunchKernelGGL(const_hit_planes, dim3((unsigned)gx, (unsigned)((nk + gx - 1) / gx)),
                     dim3(256), 0, ctx->stream, (const uint32_t*)ctx->d_kc, nk,
                     (const uint32_t*)ctx->d_lab_planes, units, ctx->d_hit);
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_rows_hit_planes(gpe_ctx* ctx, int64_t i0, int64_t m) {
  const int64_t units = (ctx->n_cases + 31) / 32;
  hipLaunchKernelGGL(rows_hit_planes, dim3((unsigned)((units + 255) / 256), (unsigned)m),
                     dim3(256), 0, ctx->stream, (const double*)ctx->d_ex_rows, ctx->n_cases,
                     units, (const int32_t*)ctx->d_ex_progs, i0, ctx->d_hit);
  HIPCHK(hipGetLastError());
  return 0;
}

// one program's 0/1 terms of the host exact pass into its plane
int host_row_hit_plane(gpe_ctx* ctx, int prog, const double* term) {
  const int64_t nc = ctx->n_cases, units = (nc + 31) / 32;
  std::vector<uint32_t> row((size_t)units, 0u);
  for (int64_t c = 0; c < nc; ++c)
    if (term[c] != 0.0) row[(size_t)(c >> 5)] |= 1u << (c & 31);
  HIPCHK(hipMemcpy(ctx->d_hit + (size_t)prog * (size_t)units, row.data(),
                   (size_t)units * sizeof(uint32_t), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace
