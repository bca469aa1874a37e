// Part of gpeval.hip's single translation unit (included there once, after
// hit_groups.h): real-valued case weights on the hit matrix —
// gpe_case_solve_counts, gpe_hit_weighted_sums, gpe_hit_shared_sums, their
// host twins and gpe_last_case_weights_ms.
//
//   s[c]     = the live programs that hit case c                (solve counts)
//   wh[i][g] = the sum of W[g][c] over the cases c row i hits   (weighted hits)
//   sh[i]    = wh[i] under W[c] = s[c] > 0 ? 1 / s[c] : 0       (implicit
//              fitness sharing; the weights never leave the device)
//
// case_solve_counts works on the case-major planes Q = uint64[32 units][W64]
// (hit_transpose's; program i at bit i % 64 of word i / 64, pad programs 0):
// s[c] is the popcount of row c, ANDed word by word with the live mask
// uint64[W64] when there is one.  L lanes share a case (a power of two >= W64,
// 64 from W64 = 64 on, as informed_step), the group sums by integer xor
// shuffles and its lane 0 stores: no atomics.  The same launch writes the
// sharing weight 1.0 / (double)s[c] (one IEEE division: the translation unit
// has no fast-math and no contraction) when a weight row is given.
//
// hit_weighted_sums<G> works on the program-major planes uint32[n][units].
// The order of one sum is fixed, whatever G and the grid are (the host twin
// hw_host_row follows it):
//   1. 64 partials (hi, lo), all zero.  Partial p takes the hit cases
//      c = p, p + 64, p + 128, ... < n_cases in ascending order, each by
//      abserr::accumulate's step: two_sum(hi, w) -> (hi, r); lo = lo + r
//      (hw_two_sum: the same operations without the overflow guard, which a
//      finite sum never reaches).
//   2. The partials merge by the xor butterfly m = 32, 16, ... 1:
//      partial p becomes abserr::dd_add(partial p, partial p ^ m).
//   3. The result is hi of partial 0 (dd_add leaves a normalised pair).
// That is a wave per row: lane p keeps partial p, a step covers 64 cases (two
// words of the row, which the wave loads 64 at a time, one per lane, and hands
// round by a shuffle), lane p reads weight c0 + p (consecutive doubles:
// coalesced, conflict-free in LDS) and adds bit ? w : +0.0 (the weight ANDed
// with the bit spread over a word) — adding +0.0 leaves a non-negative pair
// as it is, so there is no branch.  The pad bits of the last word are cleared
// on load and the weight index is clamped, so a caller's pad bits never reach
// a weight.  One kernel serves every row length: a short row costs the
// butterfly, which any mapping that keeps the order has to make.
// The weights double[G][n_cases] sit in LDS when G * n_cases * 8 bytes fit
// kHwLdsBytes = 64 KiB (two 1024-thread blocks in a CU's 160 KiB: all 32 wave
// slots), else they are read through L1 / L2 — C5's 4,601 rows fit at G = 1
// only; the sums are the same bits either way.
#pragma once
extern "C++" {
namespace {

constexpr int kHwBlock = 1024;                    // 16 waves
constexpr int kHwBlocksPerCu = 2;
constexpr size_t kHwLdsBytes = 64 * 1024;         // the weights' LDS budget
constexpr int kHwMaxRows = 8;                     // weight rows of one call
constexpr int kHwCntBlock = 256;
constexpr int64_t kHwCntMaxBlocks = 4096;

__global__ __launch_bounds__(kHwCntBlock) void case_solve_counts(
    const unsigned long long* __restrict__ Q, int64_t C, int64_t W, int L,
    const unsigned long long* __restrict__ live, int32_t* __restrict__ out,
    double* __restrict__ ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (L - 1);
  const int cpw = 64 / L;
  const int64_t per_block = (int64_t)(kHwCntBlock / 64) * cpw;
  // (the bound is the block's, so every lane of a wave meets the shuffles)
  for (int64_t base = (int64_t)blockIdx.x * per_block; base < C;
       base += (int64_t)gridDim.x * per_block) {
    const int64_t c = base + (int64_t)wave * cpw + lane / L;
    const bool valid = c < C;
    int acc = 0;
    if (valid) {
      const unsigned long long* row = Q + c * W;
      for (int64_t w = sub; w < W; w += L)
        acc += __builtin_popcountll(live ? row[w] & live[w] : row[w]);
    }
    for (int m = L >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (valid && sub == 0) {
      out[c] = acc;
      if (ws) ws[c] = acc > 0 ? 1.0 / (double)acc : 0.0;
    }
  }
}

// abserr::two_sum without its guard for a sum that overflowed: the weights'
// sum is finite, so the guard never acts and the bits are the same
HD void hw_two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// The rows of one wave (see the head of this file).  A step's weight is
// masked to +0.0 by an integer AND with the row's bit spread over a word, and
// the case index stays in 32 bits (n_cases < 2^31, and a row's last step ends
// below n_cases + 64).
template <int G>
__device__ __forceinline__ void hw_rows(const uint32_t* __restrict__ planes, int64_t n, int64_t U,
                                        int64_t C, const double* wt, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kHwBlock / 64) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (kHwBlock / 64);
  const uint32_t tail = (C & 31) ? (1u << (C & 31)) - 1u : 0xffffffffu;
  const uint32_t last = (uint32_t)C - 1u;
  const int half = lane >> 5, sh = lane & 31;
  for (int64_t i = wave; i < n; i += n_waves) {
    const uint32_t* row = planes + i * U;
    double hi[G], lo[G];
#pragma unroll
    for (int g = 0; g < G; ++g) hi[g] = lo[g] = 0.0;
    for (int64_t w0 = 0; w0 < U; w0 += 64) {
      uint32_t mine = w0 + lane < U ? row[w0 + lane] : 0u;
      if (w0 + lane == U - 1) mine &= tail;
      const int steps = (int)(((U - w0 < 64 ? U - w0 : 64) + 1) / 2);
      const uint32_t c0 = (uint32_t)w0 * 32u + (uint32_t)lane;
#pragma unroll 4
      for (int t = 0; t < steps; ++t) {
        const uint32_t word = __shfl(mine, 2 * t + half, 64);
        const uint32_t keep = 0u - ((word >> sh) & 1u);         // all ones: a hit
        const uint32_t c = c0 + 64u * (uint32_t)t;
        const uint32_t cc = c < last ? c : last;                // (no hit past n_cases)
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const unsigned long long wb =
              (unsigned long long)__double_as_longlong(wt[(int64_t)g * C + cc]);
          const double w = __longlong_as_double(
              (long long)(wb & (((unsigned long long)keep << 32) | keep)));
          double s, r;
          hw_two_sum(hi[g], w, s, r);
          hi[g] = s;
          lo[g] = lo[g] + r;
        }
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int g = 0; g < G; ++g)
        abserr::dd_add(hi[g], lo[g], __shfl_xor(hi[g], m, 64), __shfl_xor(lo[g], m, 64));
    }
    if (lane == 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) out[i * G + g] = hi[g];
    }
  }
}

template <int G>
__global__ __launch_bounds__(kHwBlock) void hit_weighted_sums(
    const uint32_t* __restrict__ planes, int64_t n, int64_t U, int64_t C,
    const double* __restrict__ weights, int in_lds, double* __restrict__ out) {
  extern __shared__ double hw_lds[];
  // (one body, inlined twice: each copy knows its weights' address space)
  if (in_lds) {
    for (int64_t k = threadIdx.x; k < (int64_t)G * C; k += kHwBlock) hw_lds[k] = weights[k];
    __syncthreads();
    hw_rows<G>(planes, n, U, C, hw_lds, out);
  } else {
    hw_rows<G>(planes, n, U, C, weights, out);
  }
}

template <int G>
void hw_launch(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t units, int64_t n_cases,
               const double* weights, double* out) {
  const size_t bytes = (size_t)G * (size_t)n_cases * sizeof(double);
  const bool in_lds = bytes <= kHwLdsBytes;
  const int64_t per_block = kHwBlock / 64;
  const int64_t blocks = std::min<int64_t>((n + per_block - 1) / per_block,
                                           (int64_t)kHwBlocksPerCu * std::max(ctx->cu, 1));
  if (in_lds)
    (void)hipFuncSetAttribute((const void*)hit_weighted_sums<G>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHwLdsBytes);
  hipLaunchKernelGGL(hit_weighted_sums<G>, dim3((unsigned)blocks), dim3(kHwBlock),
                     in_lds ? bytes : 0, ctx->stream, planes, n, units, n_cases, weights,
                     in_lds ? 1 : 0, out);
}

void hw_launch_g(gpe_ctx* ctx, int G, const uint32_t* planes, int64_t n, int64_t units,
                 int64_t n_cases, const double* weights, double* out) {
  switch (G) {
    case 1: hw_launch<1>(ctx, planes, n, units, n_cases, weights, out); break;
    case 2: hw_launch<2>(ctx, planes, n, units, n_cases, weights, out); break;
    case 3: hw_launch<3>(ctx, planes, n, units, n_cases, weights, out); break;
    case 4: hw_launch<4>(ctx, planes, n, units, n_cases, weights, out); break;
    case 5: hw_launch<5>(ctx, planes, n, units, n_cases, weights, out); break;
    case 6: hw_launch<6>(ctx, planes, n, units, n_cases, weights, out); break;
    case 7: hw_launch<7>(ctx, planes, n, units, n_cases, weights, out); break;
    default: hw_launch<8>(ctx, planes, n, units, n_cases, weights, out); break;
  }
}

int hw_launch_counts(gpe_ctx* ctx, const unsigned long long* Q, int64_t n, int64_t n_cases,
                     const unsigned long long* live, int32_t* out, double* ws) {
  const int64_t W = (n + 63) / 64;
  int L = 64;
  if (W < 64) {
    L = 1;
    while (L < W) L <<= 1;
  }
  const int64_t per_block = (int64_t)(kHwCntBlock / 64) * (64 / L);
  const int64_t blocks = std::min<int64_t>((n_cases + per_block - 1) / per_block, kHwCntMaxBlocks);
  hipLaunchKernelGGL(case_solve_counts, dim3((unsigned)blocks), dim3(kHwCntBlock), 0, ctx->stream,
                     Q, n_cases, W, L, live, out, ws);
  HIPCHK(hipGetLastError());
  return 0;
}

// one row's sum under one weight row in the kernel's order: (hi, lo)
inline void hw_host_row(const uint32_t* row, int64_t n_cases, const double* w, double* out_hi,
                        double* out_lo) {
  double hi[64] = {}, lo[64] = {};
  for (int64_t c = 0; c < n_cases; ++c) {
    const bool bit = (row[c / 32] >> (c % 32)) & 1u;
    double s, r;
    hw_two_sum(hi[c & 63], bit ? w[c] : 0.0, s, r);
    hi[c & 63] = s;
    lo[c & 63] = lo[c & 63] + r;
  }
  // (lane p < m of the butterfly: its partner p ^ m is p + m)
  for (int m = 32; m >= 1; m >>= 1)
    for (int p = 0; p < m; ++p) abserr::dd_add(hi[p], lo[p], hi[p + m], lo[p + m]);
  *out_hi = hi[0];
  *out_lo = lo[0];
}

inline void hw_host_counts(const uint32_t* planes, int64_t n, int64_t n_cases,
                           const uint64_t* live, int32_t* out) {
  const int64_t units = (n_cases + 31) / 32;
  for (int64_t c = 0; c < n_cases; ++c) out[c] = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (live && !((live[i / 64] >> (i % 64)) & 1ull)) continue;
    for (int64_t c = 0; c < n_cases; ++c) out[c] += (planes[i * units + c / 32] >> (c % 32)) & 1u;
  }
}

// every weight finite and >= 0 (-0.0 counts as 0.0)
bool hw_weights_ok(const double* w, size_t count) {
  for (size_t k = 0; k < count; ++k)
    if (!(w[k] >= 0.0) || !__builtin_isfinite(w[k])) return false;
  return true;
}

// The sizes of a case-weight call, after hit_matrix_which (hit_matrix.h) has
// filled them in.  want_q: the call counts on the case-major planes, whose
// programs an int32 indexes.
int hw_check(gpe_ctx* ctx, const char* what, const HitMatrix& m, bool want_q) {
  char buf[160];
  if (m.n < 0) {
    snprintf(buf, sizeof(buf), "%s: n = %lld individuals (need >= 0)", what, (long long)m.n);
    return fail(ctx, GPE_E_ARG, buf);
  }
  if (m.n_cases < 1 || m.n_cases >= (1ll << 31)) {
    snprintf(buf, sizeof(buf), "%s: n_cases = %lld (need 1 .. 2^31 - 1)", what,
             (long long)m.n_cases);
    return fail(ctx, GPE_E_ARG, buf);
  }
  if (want_q && m.n > INT32_MAX) {
    snprintf(buf, sizeof(buf), "%s: n = %lld individuals (the counts need n <= 2^31 - 1)", what,
             (long long)m.n);
    return fail(ctx, GPE_E_ARG, buf);
  }
  return 0;
}

// The matrix of a counting call on the device, H and Q, its live mask
// uint64[ceil(n / 64)] travelling with the planes into d_hw_live (*d_live;
// nullptr: all live).
int hw_matrix_live(gpe_ctx* ctx, HitMatrix* m, const uint64_t* live,
                   const unsigned long long** d_live) {
  HostPiece pc[1];
  const size_t W = (size_t)((m->n + 63) / 64);
  if (live) {
    if (ensure(ctx, &ctx->d_hw_live, &ctx->hw_live_cap, W)) return GPE_E_HIP;
    pc[0] = {ctx->d_hw_live, live, W * sizeof(uint64_t)};
  }
  *d_live = live ? ctx->d_hw_live : nullptr;
  return hit_matrix_device(ctx, m, true, pc, live ? 1 : 0);
}

}  // namespace
}  // extern "C++"

int gpe_host_case_solve_counts(const uint32_t* planes, int64_t n, int64_t n_cases,
                               const uint64_t* live, int32_t* out_counts) {
  if (n < 0 || n > INT32_MAX || n_cases < 1 || n_cases >= (1ll << 31) || !out_counts ||
      (n > 0 && !planes))
    return GPE_E_ARG;
  hw_host_counts(planes, n, n_cases, live, out_counts);
  return 0;
}

int gpe_host_hit_weighted_sums(const uint32_t* planes, int64_t n, int64_t n_cases,
                               const double* weights, int G, double* out, double* out_lo) {
  if (G < 1 || G > kHwMaxRows || n < 0 || n_cases < 1 || n_cases >= (1ll << 31) || !weights ||
      (n > 0 && (!out || !planes)) || !hw_weights_ok(weights, (size_t)G * (size_t)n_cases))
    return GPE_E_ARG;
  const int64_t units = (n_cases + 31) / 32;
  for (int64_t i = 0; i < n; ++i)
    for (int g = 0; g < G; ++g) {
      double hi, lo;
      hw_host_row(planes + i * units, n_cases, weights + (int64_t)g * n_cases, &hi, &lo);
      out[i * G + g] = hi;
      if (out_lo) out_lo[i * G + g] = lo;
    }
  return 0;
}

int gpe_host_hit_shared_sums(const uint32_t* planes, int64_t n, int64_t n_cases,
                             const uint64_t* live, int32_t* out_counts, double* out,
                             double* out_lo) {
  if (n < 0 || n > INT32_MAX || n_cases < 1 || n_cases >= (1ll << 31) ||
      (n > 0 && (!out || !planes)))
    return GPE_E_ARG;
  std::vector<int32_t> s((size_t)n_cases);
  hw_host_counts(planes, n, n_cases, live, s.data());
  std::vector<double> ws((size_t)n_cases);
  for (int64_t c = 0; c < n_cases; ++c)
    ws[(size_t)c] = s[(size_t)c] > 0 ? 1.0 / (double)s[(size_t)c] : 0.0;
  if (out_counts) std::copy(s.begin(), s.end(), out_counts);
  const int64_t units = (n_cases + 31) / 32;
  for (int64_t i = 0; i < n; ++i) {
    double hi, lo;
    hw_host_row(planes + i * units, n_cases, ws.data(), &hi, &lo);
    out[i] = hi;
    if (out_lo) out_lo[i] = lo;
  }
  return 0;
}

int gpe_case_solve_counts(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                          double eps, const uint64_t* live, int32_t* out_counts) {
  if (!ctx) return GPE_E_INVALID;
  if (!out_counts) return fail(ctx, GPE_E_ARG, "case_solve_counts: out_counts is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  HitMatrix m;
  if (int rc = hit_matrix_which(ctx, "case_solve_counts", planes, n, n_cases, true, eps, &m))
    return rc;
  if (int rc = hw_check(ctx, "case_solve_counts", m, true)) return rc;
  if (m.n == 0) {                  // nobody solves anything
    if (planes) std::fill(out_counts, out_counts + m.n_cases, 0);
    return 0;
  }
  const unsigned long long* d_live = nullptr;
  if (int rc = hw_matrix_live(ctx, &m, live, &d_live)) return rc;
  if (ensure(ctx, &ctx->d_hw_cnt, &ctx->hw_cnt_cap, (size_t)m.n_cases)) return GPE_E_HIP;
  // (ev_redo: the context's timed pair; no run is in flight in this call)
  HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
  if (int rc = hw_launch_counts(ctx, m.Q, m.n, m.n_cases, d_live, ctx->d_hw_cnt, nullptr))
    return rc;
  HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
  if (int rc = values_to_host(ctx, out_counts, ctx->d_hw_cnt, (size_t)m.n_cases * sizeof(int32_t)))
    return rc;
  HIPCHK(hipEventElapsedTime(&ctx->hw_ms, ctx->ev_redo[0], ctx->ev_redo[1]));
  return 0;
}

int gpe_hit_weighted_sums(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                          double eps, const double* weights, int G, double* out) {
  if (!ctx) return GPE_E_INVALID;
  char buf[160];
  if (G < 1 || G > kHwMaxRows) {
    snprintf(buf, sizeof(buf), "hit_weighted_sums: G = %d weight rows (need 1 .. %d)", G,
             kHwMaxRows);
    return fail(ctx, GPE_E_ARG, buf);
  }
  if (!weights) return fail(ctx, GPE_E_ARG, "hit_weighted_sums: weights is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  // (a NULL out is refused before anything is copied: n is known by now
  // unless the matrix is the resident one, which has programs)
  if (!out && (!planes || n > 0)) return fail(ctx, GPE_E_ARG, "hit_weighted_sums: out is NULL");
  HitMatrix m;
  if (int rc = hit_matrix_which(ctx, "hit_weighted_sums", planes, n, n_cases, true, eps, &m))
    return rc;
  if (int rc = hw_check(ctx, "hit_weighted_sums", m, false)) return rc;
  if (m.n == 0) return 0;
  const size_t wn = (size_t)G * (size_t)m.n_cases;
  if (!hw_weights_ok(weights, wn))
    return fail(ctx, GPE_E_ARG, "hit_weighted_sums: every weight must be finite and >= 0");
  if (ensure(ctx, &ctx->d_hw_w, &ctx->hw_w_cap, wn) ||
      ensure(ctx, &ctx->d_hw_out, &ctx->hw_out_cap, (size_t)m.n * (size_t)G))
    return GPE_E_HIP;
  // (the weights travel with a caller's matrix; the sums read H alone)
  const HostPiece pc[1] = {{ctx->d_hw_w, weights, wn * sizeof(double)}};
  if (int rc = hit_matrix_device(ctx, &m, false, pc, 1)) return rc;
  HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
  hw_launch_g(ctx, G, m.H, m.n, m.units, m.n_cases, ctx->d_hw_w, ctx->d_hw_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
  if (int rc = values_to_host(ctx, out, ctx->d_hw_out, (size_t)m.n * (size_t)G * sizeof(double)))
    return rc;
  HIPCHK(hipEventElapsedTime(&ctx->hw_ms, ctx->ev_redo[0], ctx->ev_redo[1]));
  return 0;
}

int gpe_hit_shared_sums(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                        double eps, const uint64_t* live, int32_t* out_counts, double* out) {
  if (!ctx) return GPE_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (!out && (!planes || n > 0)) return fail(ctx, GPE_E_ARG, "hit_shared_sums: out is NULL");
  HitMatrix m;
  if (int rc = hit_matrix_which(ctx, "hit_shared_sums", planes, n, n_cases, true, eps, &m))
    return rc;
  if (int rc = hw_check(ctx, "hit_shared_sums", m, true)) return rc;
  if (m.n == 0) {
    if (planes && out_counts) std::fill(out_counts, out_counts + m.n_cases, 0);
    return 0;
  }
  const unsigned long long* d_live = nullptr;
  if (int rc = hw_matrix_live(ctx, &m, live, &d_live)) return rc;
  if (ensure(ctx, &ctx->d_hw_cnt, &ctx->hw_cnt_cap, (size_t)m.n_cases) ||
      ensure(ctx, &ctx->d_hw_w, &ctx->hw_w_cap, (size_t)m.n_cases) ||
      ensure(ctx, &ctx->d_hw_out, &ctx->hw_out_cap, (size_t)m.n))
    return GPE_E_HIP;
  // counts, weights and sums follow each other on the stream: neither the
  // counts nor the weights visit the host in between
  HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
  if (int rc = hw_launch_counts(ctx, m.Q, m.n, m.n_cases, d_live, ctx->d_hw_cnt, ctx->d_hw_w))
    return rc;
  hw_launch_g(ctx, 1, m.H, m.n, m.units, m.n_cases, ctx->d_hw_w, ctx->d_hw_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
  if (out_counts)
    if (int rc = values_to_host(ctx, out_counts, ctx->d_hw_cnt,
                                (size_t)m.n_cases * sizeof(int32_t)))
      return rc;
  if (int rc = values_to_host(ctx, out, ctx->d_hw_out, (size_t)m.n * sizeof(double))) return rc;
  HIPCHK(hipEventElapsedTime(&ctx->hw_ms, ctx->ev_redo[0], ctx->ev_redo[1]));
  return 0;
}

int gpe_last_case_weights_ms(const gpe_ctx* ctx, float* ms) {
  if (!ctx || !ms) return GPE_E_INVALID;
  *ms = ctx->hw_ms;
  return 0;
}
