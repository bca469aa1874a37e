// Part of gpeval.hip's single translation unit (included there once, after
// lexicase_par.h): selection by weighted error sums (DALex; Ni, Ding and
// Spector 2024) and weighted sums of the per-case errors themselves —
// gpe_dalex, gpe_dalex_bits, gpe_dalex_weights, gpe_dalex_sigma,
// gpe_weighted_errors, their host twins and gpe_last_dalex_ms.  The rule is in
// include/gpeval.h.
//
// Where lexicase filters case by case, DALex scores: every selection draws a
// weight per case and picks the smallest weighted sum of errors, so k
// selections are one product S = E W'^T, n x C x k fp64 FMAs, on
// v_mfma_f64_16x16x4_f64.
//
//   dalex_fit        fit[i] = every error of row i is finite (doubles only: a
//                    hit plane has no other rows).
//   dalex_sigma      sigma[c], the population standard deviation of case c
//                    over the fit rows: a block per case, two passes (mean,
//                    then squared deviations), each a double-double sum of
//                    256 strided partials (abserr::two_sum) merged by a fixed
//                    tree (abserr::dd_add).
//   dalex_weights    Wt[C][k], case-major: a block per 64 selections, lane =
//                    selection, so every access to Wt is 64 consecutive
//                    doubles.  Importance, max, exp, the ascending sum (one
//                    lane per selection walks its C terms in order), then
//                    w / sum and / sigma.
//   dalex_product    a wave owns a 64 x 64 tile of S (4 x 4 MFMA tiles, 16
//                    accumulators of 4 doubles) and walks ALL C cases in
//                    steps of 4, so a score's bits depend on its row, its
//                    column and C alone: no split-K, no atomics.  Both
//                    operands are read k-major straight from memory (L1 / L2):
//                    lane l takes case c0 + (l >> 4) and row / column l & 15,
//                    16 consecutive doubles per case, and an MFMA's 64 cycles
//                    pay for one such load.  E is the case-major copy
//                    double[C][n] (lexpar_transpose), or the case-major hit
//                    planes Q uint64[C..][W], a word's bit expanded to
//                    1.0 - bit on load.  Operand edges (rows >= n, columns
//                    >= k, cases >= C) are zero-filled: adding +0.0 to a
//                    non-negative sum changes nothing.  A block is 4 waves
//                    side by side in the columns (64 rows x 256 columns), which
//                    never meet: no LDS, no barrier.
//     C/D map of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg.
//     epilogue store:  S[i][g], nan for an unfit row (gpe_weighted_errors).
//     epilogue argmin: each column's best (S, tie key, i) over the tile's fit
//                      rows — in the lane over its 16 rows, then across the 4
//                      lane groups by xor shuffles 16 and 32 — into one partial
//                      (S, i) per 64-row tile and selection; the n x k scores
//                      never reach memory.  The tie key K2(s n + i) is computed
//                      only where two scores are equal.
//   dalex_fold       a thread per selection folds its partials in ascending
//                    tile order (the order is total, so any order gives the
//                    same pick) and writes out[s]; no pick: -1 and atomicMin
//                    of the failing s.
// Every loop is bounded by n, C, k; blocks never wait for each other.
// Cost grows as n C k: at very large n a popcount route over the bit planes
// would be cheaper for 0/1 data; there is none here.
#pragma once
extern "C++" {
namespace {

constexpr int kDlxBlock = 256;                        // 4 waves
constexpr int kDlxTile = 64;                          // a wave's tile: 64 x 64
constexpr int64_t kDlxMaxGrid = 1 << 20;
constexpr unsigned long long kDlxTieSalt = 0xD1B54A32D192ED03ull;

typedef double dlx_v4 __attribute__((ext_vector_type(4)));

// step 1 of the rule: I = pressure z, z a Box-Muller normal from K(2j), K(2j+1)
__host__ __device__ inline double dalex_importance(unsigned long long seed, unsigned long long j,
                                                   double pressure) {
  const double u1 = (double)((lexpar_key(seed, 2ull * j) >> 11) + 1ull) * 0x1p-53;
  const double u2 = (double)(lexpar_key(seed, 2ull * j + 1ull) >> 11) * 0x1p-53;
  const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
  return pressure * z;
}

// is candidate (sa, ia) ahead of (sb, ib) for selection s?  i < 0: none.  The
// order is (S, K2(s n + i), i); the key only where the scores are equal.
__host__ __device__ inline bool dalex_better(double sa, int32_t ia, double sb, int32_t ib,
                                             unsigned long long s, unsigned long long n,
                                             unsigned long long seed2) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  if (sa < sb) return true;
  if (!(sa == sb)) return false;
  const unsigned long long ka = lexpar_key(seed2, s * n + (unsigned long long)ia);
  const unsigned long long kb = lexpar_key(seed2, s * n + (unsigned long long)ib);
  return ka < kb || (ka == kb && ia < ib);
}

// one term into a strided partial (abserr::accumulate's step)
HD void dalex_dd_step(double& hi, double& lo, double e) {
  double s, r;
  abserr::two_sum(hi, e, s, r);
  hi = s;
  lo = lo + r;
}

// the two sources of E, read case-major
struct DlxDoubles {
  const double* VT;                                   // double[C][n]
  int64_t n;
  __device__ __forceinline__ double at(int64_t c, int64_t i) const { return VT[c * n + i]; }
};
struct DlxBits {
  const unsigned long long* Q;                        // uint64[C..][W]
  int64_t W;
  __device__ __forceinline__ double at(int64_t c, int64_t i) const {
    return 1.0 - (double)((Q[c * W + (i >> 6)] >> (i & 63)) & 1ull);
  }
};

__global__ __launch_bounds__(kDlxBlock) void dalex_fit(const double* __restrict__ VT, int64_t n,
                                                       int64_t C, uint8_t* __restrict__ fit) {
  for (int64_t i = (int64_t)blockIdx.x * kDlxBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kDlxBlock) {
    bool ok = true;
    for (int64_t c = 0; c < C; ++c) {
      const double e = VT[c * n + i];
      ok = ok && (e - e == 0.0);                      // (inf - inf and nan - nan are nan)
    }
    fit[i] = ok ? 1 : 0;
  }
}

// the block's double-double sum of its threads' partials, by the fixed tree
__device__ inline void dalex_block_dd(double& hi, double& lo, double* sh_hi, double* sh_lo) {
  const int tid = threadIdx.x;
  __syncthreads();                                    // (the slots may still be read)
  sh_hi[tid] = hi;
  sh_lo[tid] = lo;
  __syncthreads();
  for (int m = kDlxBlock / 2; m >= 1; m >>= 1) {
    if (tid < m) {
      double h = sh_hi[tid], l = sh_lo[tid];
      abserr::dd_add(h, l, sh_hi[tid + m], sh_lo[tid + m]);
      sh_hi[tid] = h;
      sh_lo[tid] = l;
    }
    __syncthreads();
  }
  hi = sh_hi[0];
  lo = sh_lo[0];
}

template <class Src>
__global__ __launch_bounds__(kDlxBlock) void dalex_sigma(Src src, int64_t n, int64_t C,
                                                         const uint8_t* __restrict__ fit,
                                                         double* __restrict__ sigma) {
  __shared__ double sh_hi[kDlxBlock], sh_lo[kDlxBlock];
  __shared__ LexparSh sh;
  const int tid = threadIdx.x;
  int mine = 0;
  for (int64_t i = tid; i < n; i += kDlxBlock) mine += fit[i];
  const int m = lexpar_block_sum(mine, &sh);
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    double hi = 0.0, lo = 0.0;
    for (int64_t i = tid; i < n; i += kDlxBlock)
      if (fit[i]) dalex_dd_step(hi, lo, src.at(c, i));
    dalex_block_dd(hi, lo, sh_hi, sh_lo);
    const double mean = hi / (double)m;
    hi = lo = 0.0;
    for (int64_t i = tid; i < n; i += kDlxBlock)
      if (fit[i]) {
        const double d = src.at(c, i) - mean;
        dalex_dd_step(hi, lo, d * d);
      }
    dalex_block_dd(hi, lo, sh_hi, sh_lo);
    if (tid == 0) sigma[c] = m > 0 ? sqrt(hi / (double)m) : 0.0;
  }
}

// Wt[C][k]: see the head of this file.  sigma: null without standardisation.
__global__ __launch_bounds__(kDlxBlock) void dalex_weights(unsigned long long seed,
                                                           double pressure, int64_t C, int64_t k,
                                                           const double* __restrict__ sigma,
                                                           double* Wt) {
  __shared__ double sh_m[kDlxBlock / 64][64];
  __shared__ double sh_sum[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t s0 = (int64_t)blockIdx.x * 64; s0 < k; s0 += (int64_t)gridDim.x * 64) {
    const int64_t s = s0 + lane;
    const bool live = s < k;
    double m = -__builtin_inf();
    if (live)
      for (int64_t c = wave; c < C; c += kDlxBlock / 64) {
        const double I = dalex_importance(
            seed, (unsigned long long)s * (unsigned long long)C + (unsigned long long)c, pressure);
        Wt[c * k + s] = I;
        if (I > m) m = I;
      }
    sh_m[wave][lane] = m;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kDlxBlock / 64; ++q)
      if (sh_m[q][lane] > m) m = sh_m[q][lane];
    // (a thread rereads only what it wrote itself)
    if (live)
      for (int64_t c = wave; c < C; c += kDlxBlock / 64) Wt[c * k + s] = exp(Wt[c * k + s] - m);
    __syncthreads();
    if (wave == 0 && live) {
      double t = 0.0;
      for (int64_t c = 0; c < C; ++c) t += Wt[c * k + s];     // ascending c
      sh_sum[lane] = t;
    }
    __syncthreads();
    if (live) {
      const double t = sh_sum[lane];
      for (int64_t c = wave; c < C; c += kDlxBlock / 64) {
        double w = Wt[c * k + s] / t;
        if (sigma) {
          const double sg = sigma[c];
          w = sg == 0.0 ? 0.0 : w / sg;
        }
        Wt[c * k + s] = w;
      }
    }
    __syncthreads();                                  // (sh_m / sh_sum are written again)
  }
}

// the tile's walk over the cases; FULL: no row or column of the tile is past
// the matrix, so only the last cases (C % 4) are checked
template <class Src, bool FULL>
__device__ __forceinline__ void dalex_kloop(const Src& src, const double* __restrict__ Wt,
                                            int64_t n, int64_t C, int64_t k, int64_t r0,
                                            int64_t s0, int l15, int lk, dlx_v4 (&acc)[4][4]) {
  const int64_t cmain = FULL ? (C & ~(int64_t)3) : 0;
#pragma unroll 2
  for (int64_t c0 = 0; c0 < cmain; c0 += 4) {
    const int64_t c = c0 + lk;
    double a[4], b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) a[m] = src.at(c, r0 + 16 * m + l15);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = Wt[c * k + s0 + 16 * j + l15];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[m][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[j], acc[m][j], 0, 0, 0);
  }
  for (int64_t c0 = cmain; c0 < C; c0 += 4) {
    const int64_t c = c0 + lk;
    const bool cok = c < C;
    double a[4], b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t row = r0 + 16 * m + l15;
      a[m] = cok && row < n ? src.at(c, row) : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t col = s0 + 16 * j + l15;
      b[j] = cok && col < k ? Wt[c * k + col] : 0.0;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[m][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[j], acc[m][j], 0, 0, 0);
  }
}

// S = E W'^T by 64 x 64 wave tiles; ARGMIN: part_s / part_i [row tiles][k],
// else out double[n][k] (k = G weight rows there)
template <class Src, bool ARGMIN>
__global__ __launch_bounds__(kDlxBlock) void dalex_product(
    Src src, const double* __restrict__ Wt, int64_t n, int64_t C, int64_t k,
    const uint8_t* __restrict__ fit, double* __restrict__ out, double* __restrict__ part_s,
    int32_t* __restrict__ part_i, unsigned long long seed2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lk = lane >> 4;
  const int64_t row_tiles = (n + kDlxTile - 1) / kDlxTile;
  const int64_t col_blocks = (k + 4 * kDlxTile - 1) / (4 * kDlxTile);
  const int64_t total = row_tiles * col_blocks;
  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int64_t cb = tile / row_tiles, rt = tile - cb * row_tiles;
    const int64_t r0 = rt * kDlxTile, s0 = (cb * 4 + wave) * kDlxTile;
    if (s0 >= k) continue;                            // (the waves never meet)
    dlx_v4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[m][j] = dlx_v4{0.0, 0.0, 0.0, 0.0};
    if (r0 + kDlxTile <= n && s0 + kDlxTile <= k)
      dalex_kloop<Src, true>(src, Wt, n, C, k, r0, s0, l15, lk, acc);
    else
      dalex_kloop<Src, false>(src, Wt, n, C, k, r0, s0, l15, lk, acc);
    // this lane's 16 rows: r0 + 16 m + lk + 4 reg, bit 4 m + reg of fits
    uint32_t fits = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = r0 + 16 * m + lk + 4 * reg;
        if (row < n && fit[row]) fits |= 1u << (4 * m + reg);
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t s = s0 + 16 * j + l15;
      if constexpr (ARGMIN) {
        double bs = 0.0;
        int32_t bi = -1;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int32_t row = (int32_t)(r0 + 16 * m + lk + 4 * reg);
            const double v = acc[m][j][reg];
            if (((fits >> (4 * m + reg)) & 1u) &&
                dalex_better(v, row, bs, bi, (unsigned long long)s, (unsigned long long)n,
                             seed2)) {
              bs = v;
              bi = row;
            }
          }
#pragma unroll
        for (int x = 16; x <= 32; x <<= 1) {
          const double os = __shfl_xor(bs, x, 64);
          const int32_t oi = __shfl_xor(bi, x, 64);
          if (dalex_better(os, oi, bs, bi, (unsigned long long)s, (unsigned long long)n,
                           seed2)) {
            bs = os;
            bi = oi;
          }
        }
        if (lk == 0 && s < k) {
          part_s[rt * k + s] = bs;
          part_i[rt * k + s] = bi;
        }
      } else {
        if (s < k) {
#pragma unroll
          for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int64_t row = r0 + 16 * m + lk + 4 * reg;
              if (row < n)
                out[row * k + s] =
                    ((fits >> (4 * m + reg)) & 1u) ? acc[m][j][reg] : __builtin_nan("");
            }
        }
      }
    }
  }
}

__global__ __launch_bounds__(kDlxBlock) void dalex_fold(const double* __restrict__ part_s,
                                                        const int32_t* __restrict__ part_i,
                                                        int64_t row_tiles, int64_t n, int64_t k,
                                                        unsigned long long seed2,
                                                        int32_t* __restrict__ out,
                                                        unsigned long long* failed) {
  for (int64_t s = (int64_t)blockIdx.x * kDlxBlock + threadIdx.x; s < k;
       s += (int64_t)gridDim.x * kDlxBlock) {
    double bs = 0.0;
    int32_t bi = -1;
    for (int64_t t = 0; t < row_tiles; ++t) {
      const double os = part_s[t * k + s];
      const int32_t oi = part_i[t * k + s];
      if (dalex_better(os, oi, bs, bi, (unsigned long long)s, (unsigned long long)n, seed2)) {
        bs = os;
        bi = oi;
      }
    }
    out[s] = bi;
    if (bi < 0) atomicMin(failed, (unsigned long long)s);
  }
}

unsigned dalex_grid(int64_t items, int64_t per_block) {
  return (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((items + per_block - 1) / per_block, kDlxMaxGrid));
}

// the sizes of a call; k (k_name in the message): the selections, or the
// weight rows of gpe_weighted_errors
int dalex_check(gpe_ctx* ctx, const char* what, int64_t n, int64_t n_cases, int64_t k,
                const char* k_name) {
  char buf[160];
  if (n < 1 || n > INT32_MAX) {
    snprintf(buf, sizeof(buf), "%s: n = %lld individuals (need 1 .. 2^31 - 1)", what,
             (long long)n);
    return fail(ctx, GPE_E_INVALID, buf);
  }
  if (n_cases < 1 || n_cases >= (1ll << 31)) {
    snprintf(buf, sizeof(buf), "%s: n_cases = %lld (need 1 .. 2^31 - 1)", what,
             (long long)n_cases);
    return fail(ctx, GPE_E_INVALID, buf);
  }
  if (k < 0 || k > INT32_MAX) {
    snprintf(buf, sizeof(buf), "%s: %s = %lld (need 0 .. 2^31 - 1)", what, k_name, (long long)k);
    return fail(ctx, GPE_E_INVALID, buf);
  }
  return 0;
}

int dalex_check_pressure(gpe_ctx* ctx, const char* what, double pressure) {
  if (pressure >= 0.0 && __builtin_isfinite(pressure)) return 0;
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: pressure must be finite and >= 0 (got %g)", what, pressure);
  return fail(ctx, GPE_E_ARG, buf);
}

// The error matrix of a doubles call, case-major on the device: the caller's
// host matrix (uploaded and transposed into d_lexp_vt) or, values == NULL, the
// resident per-case matrix through its cached transpose d_case_t — as
// gpe_lexicase_par reads it.  *n / *n_cases are filled in for the resident one.
int dalex_state(gpe_ctx* ctx, const double* values, int64_t* n, int64_t* n_cases) {
  if (values) return 0;
  if (!ctx->d_case_out || ctx->n_prog <= 0 || ctx->case_stale)
    return fail(ctx, GPE_E_STATE, "no per-case values on the device");
  if (ctx->case_n != ctx->n_prog)
    return fail(ctx, GPE_E_STATE,
                "no per-case values of the loaded programs on the device (another "
                "batch was loaded since the per-case run)");
  *n = ctx->n_prog;
  *n_cases = ctx->n_cases;
  return 0;
}
// extra: one further host input of the call, its device buffer ensured by the
// caller; it travels with the matrix in ONE staged copy (the staging buffer is
// not reused before the stream has read it).
int dalex_case_major(gpe_ctx* ctx, const double* values, int64_t n, int64_t C,
                     const double** VT, const HostPiece* extra = nullptr) {
  const size_t cells = (size_t)n * (size_t)C;
  const dim3 tgrid((unsigned)((C + 31) / 32), (unsigned)std::min<int64_t>((n + 31) / 32, 65535));
  if (values) {
    if (ensure(ctx, &ctx->d_lex_val, &ctx->lex_val_cap, cells) ||
        ensure(ctx, &ctx->d_lexp_vt, &ctx->lexp_vt_cap, cells))
      return GPE_E_HIP;
    HostPiece pc[2] = {{ctx->d_lex_val, values, cells * sizeof(double)}, {}};
    if (extra) pc[1] = *extra;
    if (int rc = h2d_staged(ctx, pc, extra ? 2 : 1)) return rc;
    hipLaunchKernelGGL(lexpar_transpose, tgrid, dim3(32, 8), 0, ctx->stream, ctx->d_lex_val, n, C,
                       ctx->d_lexp_vt);
    HIPCHK(hipGetLastError());
    *VT = ctx->d_lexp_vt;
    return 0;
  }
  if (extra)
    if (int rc = h2d_staged(ctx, extra, 1)) return rc;
  if (!ctx->case_t_valid || ctx->case_t_n != n || ctx->case_t_cases != C) {
    ctx->case_t_valid = false;
    if (ensure(ctx, &ctx->d_case_t, &ctx->case_t_cap, cells)) return GPE_E_HIP;
    hipLaunchKernelGGL(lexpar_transpose, tgrid, dim3(32, 8), 0, ctx->stream, ctx->d_case_out, n, C,
                       ctx->d_case_t);
    HIPCHK(hipGetLastError());
    ctx->case_t_n = n;
    ctx->case_t_cases = C;
    ctx->case_t_valid = true;
  }
  *VT = ctx->d_case_t;
  return 0;
}

// fit rows (and sigma when asked) of a matrix on the device
template <class Src>
int dalex_fit_sigma(gpe_ctx* ctx, Src src, const double* VT, int64_t n, int64_t C,
                    bool want_sigma) {
  if (ensure(ctx, &ctx->d_dlx_fit, &ctx->dlx_fit_cap, (size_t)n) ||
      ensure(ctx, &ctx->d_dlx_sigma, &ctx->dlx_sigma_cap, (size_t)C))
    return GPE_E_HIP;
  if (VT) {
    hipLaunchKernelGGL(dalex_fit, dim3(dalex_grid(n, kDlxBlock)), dim3(kDlxBlock), 0, ctx->stream,
                       VT, n, C, ctx->d_dlx_fit);
    HIPCHK(hipGetLastError());
  } else {                          // 0/1 errors: every row is fit
    HIPCHK(hipMemsetAsync(ctx->d_dlx_fit, 1, (size_t)n, ctx->stream));
  }
  if (want_sigma) {
    hipLaunchKernelGGL(dalex_sigma<Src>, dim3(dalex_grid(C, 1)), dim3(kDlxBlock), 0, ctx->stream,
                       src, n, C, ctx->d_dlx_fit, ctx->d_dlx_sigma);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int dalex_launch_weights(gpe_ctx* ctx, int64_t C, int64_t k, unsigned long long seed,
                         double pressure, const double* d_sigma) {
  if (ensure(ctx, &ctx->d_dlx_wt, &ctx->dlx_wt_cap, (size_t)C * (size_t)k)) return GPE_E_HIP;
  hipLaunchKernelGGL(dalex_weights, dim3(dalex_grid(k, 64)), dim3(kDlxBlock), 0, ctx->stream, seed,
                     pressure, C, k, d_sigma, ctx->d_dlx_wt);
  HIPCHK(hipGetLastError());
  return 0;
}

unsigned dalex_product_grid(int64_t n, int64_t k) {
  const int64_t row_tiles = (n + kDlxTile - 1) / kDlxTile;
  const int64_t col_blocks = (k + 4 * kDlxTile - 1) / (4 * kDlxTile);
  return (unsigned)std::min<int64_t>(row_tiles * col_blocks, kDlxMaxGrid);
}

// the selection, from a matrix on the device to out / failed on the host
template <class Src>
int dalex_select(gpe_ctx* ctx, Src src, const double* VT, int64_t n, int64_t C,
                 unsigned long long seed, double pressure, int standardize, int64_t k,
                 int32_t* out, int64_t* failed) {
  const int64_t row_tiles = (n + kDlxTile - 1) / kDlxTile;
  const size_t parts = (size_t)row_tiles * (size_t)k;
  if (ensure(ctx, &ctx->d_dlx_ps, &ctx->dlx_ps_cap, parts) ||
      ensure(ctx, &ctx->d_dlx_pi, &ctx->dlx_pi_cap, parts) ||
      ensure(ctx, &ctx->d_sel_out, &ctx->sel_out_cap, (size_t)k) ||
      ensure(ctx, &ctx->d_lexp_failed, &ctx->lexp_failed_cap, 1))
    return GPE_E_HIP;
  HIPCHK(hipMemsetAsync(ctx->d_lexp_failed, 0xff, sizeof(unsigned long long), ctx->stream));
  // (ev_redo: the context's timed pair; no run is in flight in this call)
  HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
  if (int rc = dalex_fit_sigma(ctx, src, VT, n, C, standardize != 0)) return rc;
  if (int rc = dalex_launch_weights(ctx, C, k, seed, pressure,
                                    standardize ? ctx->d_dlx_sigma : nullptr))
    return rc;
  const unsigned long long seed2 = seed ^ kDlxTieSalt;
  hipLaunchKernelGGL((dalex_product<Src, true>), dim3(dalex_product_grid(n, k)), dim3(kDlxBlock),
                     0, ctx->stream, src, ctx->d_dlx_wt, n, C, k, ctx->d_dlx_fit, nullptr,
                     ctx->d_dlx_ps, ctx->d_dlx_pi, seed2);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(dalex_fold, dim3(dalex_grid(k, kDlxBlock)), dim3(kDlxBlock), 0, ctx->stream,
                     ctx->d_dlx_ps, ctx->d_dlx_pi, row_tiles, n, k, seed2, ctx->d_sel_out,
                     ctx->d_lexp_failed);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
  if (int rc = lexpar_results(ctx, k, out, failed)) return rc;
  HIPCHK(hipEventElapsedTime(&ctx->dlx_ms, ctx->ev_redo[0], ctx->ev_redo[1]));
  return 0;
}

// the host's fit rows and sigma, in the kernels' order
void dalex_host_fit(const double* values, int64_t n, int64_t C, std::vector<uint8_t>& fit) {
  fit.assign((size_t)n, 1);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = 0; c < C; ++c) {
      const double e = values[i * C + c];
      if (!(e - e == 0.0)) fit[(size_t)i] = 0;
    }
}
// pass 0: the sum of e; pass 1: of (e - mean)^2
double dalex_host_dd(const double* values, int64_t n, int64_t C, int64_t c,
                     const std::vector<uint8_t>& fit, bool dev, double mean) {
  double hi[kDlxBlock] = {}, lo[kDlxBlock] = {};
  for (int64_t i = 0; i < n; ++i)
    if (fit[(size_t)i]) {
      const double e = values[i * C + c], d = e - mean;
      dalex_dd_step(hi[i % kDlxBlock], lo[i % kDlxBlock], dev ? d * d : e);
    }
  for (int m = kDlxBlock / 2; m >= 1; m >>= 1)
    for (int t = 0; t < m; ++t) abserr::dd_add(hi[t], lo[t], hi[t + m], lo[t + m]);
  return hi[0];
}
void dalex_host_sigma(const double* values, int64_t n, int64_t C, const std::vector<uint8_t>& fit,
                      double* sigma) {
  int64_t m = 0;
  for (int64_t i = 0; i < n; ++i) m += fit[(size_t)i];
  for (int64_t c = 0; c < C; ++c) {
    if (m == 0) {
      sigma[c] = 0.0;
      continue;
    }
    const double mean = dalex_host_dd(values, n, C, c, fit, false, 0.0) / (double)m;
    sigma[c] = sqrt(dalex_host_dd(values, n, C, c, fit, true, mean) / (double)m);
  }
}
// one selection's effective weights w[C]
void dalex_host_row(int64_t C, unsigned long long s, unsigned long long seed, double pressure,
                    const double* sigma, double* w) {
  double m = -__builtin_inf();
  for (int64_t c = 0; c < C; ++c) {
    w[c] = dalex_importance(seed, s * (unsigned long long)C + (unsigned long long)c, pressure);
    if (w[c] > m) m = w[c];
  }
  double t = 0.0;
  for (int64_t c = 0; c < C; ++c) {
    w[c] = exp(w[c] - m);
    t += w[c];
  }
  for (int64_t c = 0; c < C; ++c) {
    w[c] = w[c] / t;
    if (sigma) w[c] = sigma[c] == 0.0 ? 0.0 : w[c] / sigma[c];
  }
}

bool dalex_host_args_ok(int64_t n, int64_t C, int64_t k, double pressure) {
  return n >= 1 && n <= INT32_MAX && C >= 1 && C < (1ll << 31) && k >= 0 && k <= INT32_MAX &&
         pressure >= 0.0 && __builtin_isfinite(pressure);
}

}  // namespace
}  // extern "C++"

int gpe_host_dalex_weights(int64_t n_cases, int64_t k, uint64_t seed, double pressure,
                           const double* sigma, double* out_wt) {
  if (!dalex_host_args_ok(1, n_cases, k, pressure) || (k > 0 && !out_wt)) return GPE_E_INVALID;
  std::vector<double> w((size_t)n_cases);
  for (int64_t s = 0; s < k; ++s) {
    dalex_host_row(n_cases, (unsigned long long)s, seed, pressure, sigma, w.data());
    for (int64_t c = 0; c < n_cases; ++c) out_wt[c * k + s] = w[(size_t)c];
  }
  return 0;
}

int gpe_host_dalex_sigma(const double* values, int64_t n, int64_t n_cases, double* out_sigma) {
  if (!values || !out_sigma || !dalex_host_args_ok(n, n_cases, 0, 0.0)) return GPE_E_INVALID;
  std::vector<uint8_t> fit;
  dalex_host_fit(values, n, n_cases, fit);
  dalex_host_sigma(values, n, n_cases, fit, out_sigma);
  return 0;
}

int gpe_host_dalex(const double* values, int64_t n, int64_t n_cases, uint64_t seed,
                   double pressure, int standardize, int64_t k, int32_t* out, int64_t* failed) {
  if (!values || !dalex_host_args_ok(n, n_cases, k, pressure) || (k > 0 && !out))
    return GPE_E_INVALID;
  if (failed) *failed = -1;
  const int64_t C = n_cases;
  std::vector<uint8_t> fit;
  dalex_host_fit(values, n, C, fit);
  std::vector<double> sigma((size_t)C), w((size_t)C);
  if (standardize) dalex_host_sigma(values, n, C, fit, sigma.data());
  const unsigned long long seed2 = seed ^ kDlxTieSalt;
  for (int64_t s = 0; s < k; ++s) {
    dalex_host_row(C, (unsigned long long)s, seed, pressure, standardize ? sigma.data() : nullptr,
                   w.data());
    double bs = 0.0;
    int32_t bi = -1;
    for (int64_t i = 0; i < n; ++i) {
      if (!fit[(size_t)i]) continue;
      double S = 0.0;
      for (int64_t c = 0; c < C; ++c) S += w[(size_t)c] * values[i * C + c];   // ascending c
      if (dalex_better(S, (int32_t)i, bs, bi, (unsigned long long)s, (unsigned long long)n,
                       seed2)) {
        bs = S;
        bi = (int32_t)i;
      }
    }
    out[s] = bi;
    if (bi < 0 && failed && *failed < 0) *failed = s;
  }
  return 0;
}

int gpe_dalex_weights(gpe_ctx* ctx, int64_t n_cases, int64_t k, uint64_t seed, double pressure,
                      const double* sigma, double* out_wt) {
  if (!ctx) return GPE_E_INVALID;
  if (int rc = dalex_check(ctx, "dalex_weights", 1, n_cases, k, "k selections")) return rc;
  if (int rc = dalex_check_pressure(ctx, "dalex_weights", pressure)) return rc;
  if (k == 0) return 0;
  if (!out_wt) return fail(ctx, GPE_E_ARG, "dalex_weights: out_Wt is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  if (sigma) {
    if (ensure(ctx, &ctx->d_dlx_sigma, &ctx->dlx_sigma_cap, (size_t)n_cases)) return GPE_E_HIP;
    const HostPiece pc[1] = {{ctx->d_dlx_sigma, sigma, (size_t)n_cases * sizeof(double)}};
    if (int rc = h2d_staged(ctx, pc, 1)) return rc;
  }
  if (int rc = dalex_launch_weights(ctx, n_cases, k, seed, pressure,
                                    sigma ? ctx->d_dlx_sigma : nullptr))
    return rc;
  return values_to_host(ctx, out_wt, ctx->d_dlx_wt, (size_t)n_cases * (size_t)k * sizeof(double));
}

int gpe_dalex_sigma(gpe_ctx* ctx, const double* values, int64_t n, int64_t n_cases,
                    double* out_sigma) {
  if (!ctx) return GPE_E_INVALID;
  if (!out_sigma) return fail(ctx, GPE_E_ARG, "dalex_sigma: out_sigma is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = dalex_state(ctx, values, &n, &n_cases)) return rc;
  if (int rc = dalex_check(ctx, "dalex_sigma", n, n_cases, 0, "k")) return rc;
  const double* VT = nullptr;
  if (int rc = dalex_case_major(ctx, values, n, n_cases, &VT)) return rc;
  if (int rc = dalex_fit_sigma(ctx, DlxDoubles{VT, n}, VT, n, n_cases, true)) return rc;
  return values_to_host(ctx, out_sigma, ctx->d_dlx_sigma, (size_t)n_cases * sizeof(double));
}

int gpe_weighted_errors(gpe_ctx* ctx, const double* values, int64_t n, int64_t n_cases,
                        const double* weights, int64_t G, double* out) {
  if (!ctx) return GPE_E_INVALID;
  if (!weights) return fail(ctx, GPE_E_ARG, "weighted_errors: weights is NULL");
  if (!out) return fail(ctx, GPE_E_ARG, "weighted_errors: out is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = dalex_state(ctx, values, &n, &n_cases)) return rc;
  if (int rc = dalex_check(ctx, "weighted_errors", n, n_cases, G, "G weight rows")) return rc;
  if (G < 1) return fail(ctx, GPE_E_INVALID, "weighted_errors: G = 0 weight rows (need >= 1)");
  const int64_t C = n_cases;
  const size_t wn = (size_t)G * (size_t)C;
  bool w_ok = true;                 // (-0.0 counts as 0.0)
  for (size_t q = 0; q < wn && w_ok; ++q)
    w_ok = weights[q] >= 0.0 && __builtin_isfinite(weights[q]);
  if (!w_ok)
    return fail(ctx, GPE_E_ARG, "weighted_errors: every weight must be finite and >= 0");
  if (ensure(ctx, &ctx->d_dlx_win, &ctx->dlx_win_cap, wn) ||
      ensure(ctx, &ctx->d_dlx_wt, &ctx->dlx_wt_cap, wn) ||
      ensure(ctx, &ctx->d_dlx_out, &ctx->dlx_out_cap, (size_t)n * (size_t)G))
    return GPE_E_HIP;
  const HostPiece pc = {ctx->d_dlx_win, weights, wn * sizeof(double)};
  const double* VT = nullptr;
  if (int rc = dalex_case_major(ctx, values, n, C, &VT, &pc)) return rc;
  // W[G][C] into Wt[C][G], as a matrix of G rows
  const dim3 tgrid((unsigned)((C + 31) / 32), (unsigned)std::min<int64_t>((G + 31) / 32, 65535));
  hipLaunchKernelGGL(lexpar_transpose, tgrid, dim3(32, 8), 0, ctx->stream, ctx->d_dlx_win, G, C,
                     ctx->d_dlx_wt);
  HIPCHK(hipGetLastError());
  const DlxDoubles src{VT, n};
  HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
  if (int rc = dalex_fit_sigma(ctx, src, VT, n, C, false)) return rc;
  hipLaunchKernelGGL((dalex_product<DlxDoubles, false>), dim3(dalex_product_grid(n, G)),
                     dim3(kDlxBlock), 0, ctx->stream, src, ctx->d_dlx_wt, n, C, G, ctx->d_dlx_fit,
                     ctx->d_dlx_out, nullptr, nullptr, 0ull);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
  if (int rc = values_to_host(ctx, out, ctx->d_dlx_out, (size_t)n * (size_t)G * sizeof(double)))
    return rc;
  HIPCHK(hipEventElapsedTime(&ctx->dlx_ms, ctx->ev_redo[0], ctx->ev_redo[1]));
  return 0;
}

int gpe_dalex(gpe_ctx* ctx, const double* values, int64_t n, int64_t n_cases, uint64_t seed,
              double pressure, int standardize, int64_t k, int32_t* out, int64_t* failed) {
  if (!ctx || (k > 0 && !out)) return GPE_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (failed) *failed = -1;
  if (int rc = dalex_state(ctx, values, &n, &n_cases)) return rc;
  if (int rc = dalex_check(ctx, "dalex", n, n_cases, k, "k selections")) return rc;
  if (int rc = dalex_check_pressure(ctx, "dalex", pressure)) return rc;
  if (k == 0) return 0;
  const double* VT = nullptr;
  if (int rc = dalex_case_major(ctx, values, n, n_cases, &VT)) return rc;
  return dalex_select(ctx, DlxDoubles{VT, n}, VT, n, n_cases, seed, pressure, standardize, k, out,
                      failed);
}

int gpe_dalex_bits(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                   uint64_t seed, double pressure, int standardize, int64_t k, int32_t* out,
                   int64_t* failed) {
  if (!ctx || (k > 0 && !out)) return GPE_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (failed) *failed = -1;
  HitMatrix hm;
  if (int rc = hit_matrix_which(ctx, "dalex_bits", planes, n, n_cases, false, 0.0, &hm)) return rc;
  n = hm.n;
  n_cases = hm.n_cases;
  if (int rc = dalex_check(ctx, "dalex_bits", n, n_cases, k, "k selections")) return rc;
  if (int rc = dalex_check_pressure(ctx, "dalex_bits", pressure)) return rc;
  if (k == 0) return 0;
  if (int rc = hit_matrix_device(ctx, &hm, true)) return rc;
  return dalex_select(ctx, DlxBits{hm.Q, hm.W}, nullptr, n, n_cases, seed, pressure, standardize,
                      k, out, failed);
}

int gpe_last_dalex_ms(const gpe_ctx* ctx, float* ms) {
  if (!ctx || !ms) return GPE_E_INVALID;
  *ms = ctx->dlx_ms;
  return 0;
}
