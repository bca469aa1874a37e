// Part of gpeval.hip's single translation unit (included there once, after
// case_bits.h and lexicase_par.h): masked counts of the hit planes —
// gpe_hit_group_counts, gpe_host_hit_group_counts, gpe_last_hit_group_ms.
//
// out[i][g] = popcount(row_i & mask_g) for a program-major hit matrix
// uint32[n][U] (case_bits.h's layout, U = ceil(n_cases / 32)) and G <= 8 case
// groups given as planes of the same layout.  With the label plane as the one
// mask it is a classifier's true positives; with fold or stratum planes, the
// hits inside each fold.  A streaming read of the matrix and an integer
// reduction: no atomics, no LDS, nothing resident is written.
//
// Two kernels, chosen by the row length alone (kHitGrpShortUnits):
//   U <= 64  hitgrp_short: a row gets a power-of-two group of L >= U lanes
//            (64 / L rows a wave, 256 / L a block), lane j of the group reads
//            word j, and every lane keeps its G mask words in registers for
//            all the rows it visits.  The group sums by xor shuffles below L
//            and its lane 0 stores the row's G counts.  A wave's loads of
//            consecutive rows are consecutive words (the idle lanes of a
//            group aside), so parity-6's 2-word rows fill a 256-byte request.
//   U  > 64  hitgrp_long: a wave takes kHitGrpRows rows at once and strides
//            their words 64 at a time, so that a mask word fetched (through
//            L1 / L2: G * U words, the same for every wave) serves four rows;
//            the wave sums by xor shuffles and lane 0 stores.
// G is a template parameter: the mask registers and the accumulators are
// plain scalars after unrolling, and a one-mask call (the confusion matrix)
// pays for one popcount per word.
#pragma once
// (gpeval.hip includes this inside its extern "C" block: the templates need
// C++ linkage)
extern "C++" {
namespace {

constexpr int kHitGrpBlock = 256;                 // 4 waves
constexpr int kHitGrpBlocksPerCu = 8;
constexpr int64_t kHitGrpShortUnits = 64;         // rows up to a wave's width
constexpr int kHitGrpRows = 4;                    // rows a long-row wave takes
constexpr int kHitGrpMaxGroups = 8;

// lanes of a short row's group: the smallest power of two >= units (<= 64)
inline int hitgrp_lanes(int64_t units) {
  int L = 1;
  while (L < units) L <<= 1;
  return L;
}

template <int G>
__global__ __launch_bounds__(kHitGrpBlock) void hitgrp_short(
    const uint32_t* __restrict__ planes, int64_t n, int U, int L,
    const uint32_t* __restrict__ masks, int32_t* __restrict__ out) {
  const int tid = threadIdx.x;
  const int j = tid & (L - 1);                      // word of the row
  const int64_t rows_blk = kHitGrpBlock / L;
  const bool has = j < U;
  uint32_t m[G];
#pragma unroll
  for (int g = 0; g < G; ++g) m[g] = has ? masks[(int64_t)g * U + j] : 0u;
  // (the bound is the block's, so every lane of a wave makes the same trips
  // and meets the shuffles)
  for (int64_t r0 = (int64_t)blockIdx.x * rows_blk; r0 < n;
       r0 += (int64_t)gridDim.x * rows_blk) {
    const int64_t row = r0 + tid / L;
    const uint32_t w = (has && row < n) ? planes[row * (int64_t)U + j] : 0u;
    int c[G];
#pragma unroll
    for (int g = 0; g < G; ++g) c[g] = __popc(w & m[g]);
    for (int s = L >> 1; s >= 1; s >>= 1) {
#pragma unroll
      for (int g = 0; g < G; ++g) c[g] += __shfl_xor(c[g], s, 64);
    }
    if (j == 0 && row < n) {
#pragma unroll
      for (int g = 0; g < G; ++g) out[row * G + g] = c[g];
    }
  }
}

template <int G>
__global__ __launch_bounds__(kHitGrpBlock) void hitgrp_long(
    const uint32_t* __restrict__ planes, int64_t n, int64_t U,
    const uint32_t* __restrict__ masks, int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kHitGrpBlock / 64) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (kHitGrpBlock / 64);
  for (int64_t r0 = wave * kHitGrpRows; r0 < n; r0 += n_waves * kHitGrpRows) {
    // rows past the end read the last row again and are not stored
    const uint32_t* row[kHitGrpRows];
#pragma unroll
    for (int r = 0; r < kHitGrpRows; ++r)
      row[r] = planes + (r0 + r < n ? r0 + r : n - 1) * U;
    int c[kHitGrpRows][G];
#pragma unroll
    for (int r = 0; r < kHitGrpRows; ++r)
#pragma unroll
      for (int g = 0; g < G; ++g) c[r][g] = 0;
    for (int64_t w = lane; w < U; w += 64) {
      uint32_t x[kHitGrpRows], m[G];
#pragma unroll
      for (int r = 0; r < kHitGrpRows; ++r) x[r] = row[r][w];
#pragma unroll
      for (int g = 0; g < G; ++g) m[g] = masks[(int64_t)g * U + w];
#pragma unroll
      for (int r = 0; r < kHitGrpRows; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) c[r][g] += __popc(x[r] & m[g]);
    }
#pragma unroll
    for (int r = 0; r < kHitGrpRows; ++r)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        int v = c[r][g];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
        c[r][g] = v;
      }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < kHitGrpRows; ++r)
        if (r0 + r < n) {
#pragma unroll
          for (int g = 0; g < G; ++g) out[(r0 + r) * G + g] = c[r][g];
        }
    }
  }
}

template <int G>
void hitgrp_launch(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t units,
                   const uint32_t* masks, int32_t* out) {
  const int64_t cap = (int64_t)kHitGrpBlocksPerCu * std::max(ctx->cu, 1);
  if (units <= kHitGrpShortUnits) {
    const int L = hitgrp_lanes(units);
    const int64_t rows_blk = kHitGrpBlock / L;
    const int64_t blocks = std::min<int64_t>((n + rows_blk - 1) / rows_blk, cap);
    hipLaunchKernelGGL(hitgrp_short<G>, dim3((unsigned)blocks), dim3(kHitGrpBlock), 0,
                       ctx->stream, planes, n, (int)units, L, masks, out);
  } else {
    const int64_t rows_blk = (kHitGrpBlock / 64) * kHitGrpRows;
    const int64_t blocks = std::min<int64_t>((n + rows_blk - 1) / rows_blk, cap);
    hipLaunchKernelGGL(hitgrp_long<G>, dim3((unsigned)blocks), dim3(kHitGrpBlock), 0,
                       ctx->stream, planes, n, units, masks, out);
  }
}

void hitgrp_launch_g(gpe_ctx* ctx, int G, const uint32_t* planes, int64_t n, int64_t units,
                     const uint32_t* masks, int32_t* out) {
  switch (G) {
    case 1: hitgrp_launch<1>(ctx, planes, n, units, masks, out); break;
    case 2: hitgrp_launch<2>(ctx, planes, n, units, masks, out); break;
    case 3: hitgrp_launch<3>(ctx, planes, n, units, masks, out); break;
    case 4: hitgrp_launch<4>(ctx, planes, n, units, masks, out); break;
    case 5: hitgrp_launch<5>(ctx, planes, n, units, masks, out); break;
    case 6: hitgrp_launch<6>(ctx, planes, n, units, masks, out); break;
    case 7: hitgrp_launch<7>(ctx, planes, n, units, masks, out); break;
    default: hitgrp_launch<8>(ctx, planes, n, units, masks, out); break;
  }
}

// the masks with their pad bits cleared, uint32[G][units]
std::vector<uint32_t> hitgrp_clean_masks(const uint32_t* masks, int G, int64_t n_cases) {
  const int64_t units = (n_cases + 31) / 32;
  std::vector<uint32_t> m(masks, masks + (size_t)G * (size_t)units);
  const int tail = (int)(n_cases & 31);
  if (tail)
    for (int g = 0; g < G; ++g) m[(size_t)g * (size_t)units + (size_t)units - 1] &= (1u << tail) - 1u;
  return m;
}

}  // namespace
}  // extern "C++"

int gpe_host_hit_group_counts(const uint32_t* planes, int64_t n, int64_t n_cases,
                              const uint32_t* masks, int G, int32_t* out) {
  if (G < 1 || G > kHitGrpMaxGroups || n < 0 || n_cases < 1 || n_cases >= (1ll << 31) || !masks ||
      (n > 0 && (!out || !planes)))
    return GPE_E_ARG;
  const int64_t units = (n_cases + 31) / 32;
  const std::vector<uint32_t> m = hitgrp_clean_masks(masks, G, n_cases);
  for (int64_t i = 0; i < n; ++i)
    for (int g = 0; g < G; ++g) {
      int32_t c = 0;
      for (int64_t w = 0; w < units; ++w)
        c += __builtin_popcount(planes[i * units + w] & m[(size_t)g * (size_t)units + (size_t)w]);
      out[i * G + g] = c;
    }
  return 0;
}

int gpe_hit_group_counts(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                         const uint32_t* masks, int G, int32_t* out) {
  if (!ctx) return GPE_E_INVALID;
  char buf[160];
  if (G < 1 || G > kHitGrpMaxGroups) {
    snprintf(buf, sizeof(buf), "hit_group_counts: G = %d groups (need 1 .. %d)", G,
             kHitGrpMaxGroups);
    return fail(ctx, GPE_E_ARG, buf);
  }
  if (!masks) return fail(ctx, GPE_E_ARG, "hit_group_counts: masks is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  HitMatrix hm;
  if (int rc = hit_matrix_which(ctx, "hit_group_counts", planes, n, n_cases, false, 0.0, &hm))
    return rc;
  n = hm.n;
  n_cases = hm.n_cases;
  if (n < 0) {
    snprintf(buf, sizeof(buf), "hit_group_counts: n = %lld individuals (need >= 0)",
             (long long)n);
    return fail(ctx, GPE_E_ARG, buf);
  }
  if (n_cases < 1 || n_cases >= (1ll << 31)) {
    snprintf(buf, sizeof(buf), "hit_group_counts: n_cases = %lld (need 1 .. 2^31 - 1)",
             (long long)n_cases);
    return fail(ctx, GPE_E_ARG, buf);
  }
  if (n == 0) return 0;
  if (!out) return fail(ctx, GPE_E_ARG, "hit_group_counts: out is NULL");
  const std::vector<uint32_t> m = hitgrp_clean_masks(masks, G, n_cases);
  if (ensure(ctx, &ctx->d_hitgrp_masks, &ctx->hitgrp_masks_cap, m.size()) ||
      ensure(ctx, &ctx->d_hitgrp_out, &ctx->hitgrp_out_cap, (size_t)n * (size_t)G))
    return GPE_E_HIP;
  // (the masks travel with a caller's matrix; the counts read H alone)
  const HostPiece pc[1] = {{ctx->d_hitgrp_masks, m.data(), m.size() * sizeof(uint32_t)}};
  if (int rc = hit_matrix_device(ctx, &hm, false, pc, 1)) return rc;
  // (ev_redo: the context's timed pair; no run is in flight in this call)
  HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
  hitgrp_launch_g(ctx, G, hm.H, n, hm.units, ctx->d_hitgrp_masks, ctx->d_hitgrp_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
  if (int rc = values_to_host(ctx, out, ctx->d_hitgrp_out, (size_t)n * (size_t)G * sizeof(int32_t)))
    return rc;
  HIPCHK(hipEventElapsedTime(&ctx->hitgrp_ms, ctx->ev_redo[0], ctx->ev_redo[1]));
  return 0;
}

int gpe_last_hit_group_ms(const gpe_ctx* ctx, float* ms) {
  if (!ctx || !ms) return GPE_E_INVALID;
  *ms = ctx->hitgrp_ms;
  return 0;
}
