// Part of gpeval.hip's single translation unit (included there once, after
// hit_matrix.h): informed down-sampling — a farthest-first subset of the cases
// from the resident per-case matrix — gpe_informed_cases,
// gpe_host_informed_cases, gpe_host_hit_threshold.
//
// The distance between two cases is the Hamming distance of their pass/fail
// vectors over the programs, which is one row each of the case-major planes
// case_bits.h already builds: Q = uint64[32 n_units][W], W = ceil(n / 64),
// program i at bit i % 64 of word i / 64, pad programs 0.  A regression
// matrix (d_case_out, double[n][n_cases] of absolute errors) is first turned
// into program-major hit planes by hit_threshold and transposed like any other
// (hit_matrix.h, which resolves the matrix of a call; kInfBlock is there too).
//
// The traversal: key[c] = the (c + 1)-th output of SplitMix64(seed) orders the
// cases totally by (key, c).  The first pick is the smallest case in that
// order; every later pick is the unchosen case with the largest mind (its
// distance to the nearest chosen case), ties to the smallest (key, c).  One
// launch per pick (informed_step): it first settles the previous pick from the
// block partials of the previous launch (every block reduces them for itself:
// a few KiB from L2), folds the distance to that pick into mind, and writes
// this launch's block partials.  Launches on one stream are ordered, so a pick
// is final before anything reads it, with no barrier between blocks and
// nothing a lost block could leave waiting.  The total order makes the result
// independent of how the cases fall into blocks.
#pragma once
namespace {

constexpr int64_t kInfMaxBlocks = 1024;     // partials a block reduces per launch
constexpr size_t kInfPivotLds = 32 * 1024;  // the pivot row is staged in LDS up to here

__host__ __device__ inline unsigned long long informed_key(unsigned long long seed, int64_t c) {
  unsigned long long z = seed + (unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// candidate (md, key, c): a larger mind wins, then the smaller (key, c);
// md < 0 is no candidate
struct InfCand {
  int32_t md;
  int32_t c;
  unsigned long long key;
};
__host__ __device__ inline bool informed_better(const InfCand& a, const InfCand& b) {
  if (a.md != b.md) return a.md > b.md;
  if (a.md < 0) return false;
  if (a.key != b.key) return a.key < b.key;
  return a.c < b.c;
}

// the best of the block's candidates in every thread (all kInfBlock threads
// call; red: 4 slots of LDS)
__device__ inline InfCand informed_block_best(InfCand v, InfCand* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    InfCand o;
    o.md = __shfl_xor(v.md, m, 64);
    o.c = __shfl_xor(v.c, m, 64);
    o.key = __shfl_xor(v.key, m, 64);
    if (informed_better(o, v)) v = o;
  }
  __syncthreads();                                  // (red may still be read from before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  InfCand best = red[0];
#pragma unroll
  for (int q = 1; q < kInfBlock / 64; ++q)
    if (informed_better(red[q], best)) best = red[q];
  return best;
}

// the pick the nb partials of one launch hold
__device__ inline InfCand informed_reduce_partials(const ulonglong2* __restrict__ part, int nb,
                                                   InfCand* red) {
  InfCand v = {-1, 0, 0ull};
  for (int i = threadIdx.x; i < nb; i += kInfBlock) {
    const ulonglong2 p = part[i];
    InfCand o;
    o.key = p.x;
    o.md = (int32_t)(uint32_t)(p.y >> 32);
    o.c = (int32_t)(uint32_t)p.y;
    if (informed_better(o, v)) v = o;
  }
  return informed_block_best(v, red);
}

// Pick t of the traversal on Q[C..][W] (rows c >= C, the pad cases of the last
// word, are all-zero rows and are never looked at).  t = 0: every mind starts
// equal (INT32_MAX), so the partials name the smallest (key, c).  t >= 1:
// pick t - 1 is reduced from prev (nb_prev partials) and written to
// out_idx / out_dist by block 0; its row, staged in LDS when piv_lds, is the
// pivot; mind[c] = min(mind[c], hamming(Q[c], pivot)), -1 for chosen cases.
// G lanes share a case (a power of two, 64 when W >= 64: the wave's lanes read
// consecutive words of consecutive rows), 64 / G cases per wave.
__global__ __launch_bounds__(kInfBlock) void informed_step(
    const unsigned long long* __restrict__ Q, int64_t C, int64_t W, int G, int64_t t,
    unsigned long long seed, int32_t* __restrict__ mind, const ulonglong2* __restrict__ prev,
    int nb_prev, ulonglong2* __restrict__ part, int64_t* __restrict__ out_idx,
    int32_t* __restrict__ out_dist, int piv_lds) {
  extern __shared__ unsigned long long inf_pivot[];
  __shared__ InfCand red[kInfBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t last = -1;
  const unsigned long long* piv = nullptr;
  if (t > 0) {
    const InfCand pick = informed_reduce_partials(prev, nb_prev, red);
    last = pick.c;
    if (blockIdx.x == 0 && tid == 0) {
      out_idx[t - 1] = last;
      out_dist[t - 1] = t == 1 ? -1 : pick.md;
    }
    piv = Q + last * W;
    if (piv_lds) {
      for (int64_t w = tid; w < W; w += kInfBlock) inf_pivot[w] = piv[w];
      __syncthreads();
      piv = inf_pivot;
    }
  }
  const int sub = lane & (G - 1);
  const int cpw = 64 / G;
  const int64_t per_block = (int64_t)(kInfBlock / 64) * cpw;
  InfCand best = {-1, 0, 0ull};
  for (int64_t base = (int64_t)blockIdx.x * per_block; base < C;
       base += (int64_t)gridDim.x * per_block) {
    const int64_t c = base + (int64_t)wave * cpw + lane / G;
    const bool valid = c < C;
    int acc = 0;
    if (valid && t > 0) {
      const unsigned long long* row = Q + c * W;
      for (int64_t w = sub; w < W; w += G) acc += __builtin_popcountll(row[w] ^ piv[w]);
    }
    for (int m = G >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (valid) {
      int32_t md = INT32_MAX;
      if (t > 0) {
        md = mind[c];
        if (c == last) md = -1;
        else if (md >= 0) md = min(md, acc);
      }
      if (sub == 0) mind[c] = md;
      if (md >= 0 && sub == 0) {                    // (one lane speaks for the case)
        const InfCand mine = {md, (int32_t)c, informed_key(seed, c)};
        if (informed_better(mine, best)) best = mine;
      }
    }
  }
  best = informed_block_best(best, red);
  if (tid == 0)
    part[blockIdx.x] = make_ulonglong2(
        best.key, ((unsigned long long)(uint32_t)best.md << 32) | (uint32_t)best.c);
}

// the last pick (m - 1), from the last launch's partials
__global__ __launch_bounds__(kInfBlock) void informed_last(const ulonglong2* __restrict__ prev,
                                                           int nb_prev, int64_t m,
                                                           int64_t* __restrict__ out_idx,
                                                           int32_t* __restrict__ out_dist) {
  __shared__ InfCand red[kInfBlock / 64];
  const InfCand pick = informed_reduce_partials(prev, nb_prev, red);
  if (threadIdx.x == 0) {
    out_idx[m - 1] = pick.c;
    out_dist[m - 1] = m == 1 ? -1 : pick.md;
  }
}

// m picks on Q (device) into the context's d_inf_idx / d_inf_dist
int launch_informed(gpe_ctx* ctx, const unsigned long long* Q, int64_t n, int64_t C,
                    unsigned long long seed, int64_t m) {
  const int64_t W = (n + 63) / 64;
  int G = 64;
  if (W < 64) {
    G = 1;
    while (G < W) G <<= 1;
  }
  const int64_t per_block = (int64_t)(kInfBlock / 64) * (64 / G);
  const int nb = (int)std::min<int64_t>((C + per_block - 1) / per_block, kInfMaxBlocks);
  if (ensure(ctx, &ctx->d_inf_mind, &ctx->inf_mind_cap, (size_t)C) ||
      ensure(ctx, &ctx->d_inf_part, &ctx->inf_part_cap, (size_t)(4 * kInfMaxBlocks)) ||
      ensure(ctx, &ctx->d_inf_idx, &ctx->inf_idx_cap, (size_t)m) ||
      ensure(ctx, &ctx->d_inf_dist, &ctx->inf_dist_cap, (size_t)m))
    return GPE_E_HIP;
  const bool piv_lds = (size_t)W * 8 <= kInfPivotLds;
  const size_t lds = piv_lds ? (size_t)W * 8 : 0;
  ulonglong2* part[2] = {(ulonglong2*)ctx->d_inf_part,
                         (ulonglong2*)ctx->d_inf_part + kInfMaxBlocks};
  for (int64_t t = 0; t < m; ++t)
    hipLaunchKernelGGL(informed_step, dim3((unsigned)nb), dim3(kInfBlock), t > 0 ? lds : 0,
                       ctx->stream, Q, C, W, G, t, seed, ctx->d_inf_mind, part[(t + 1) & 1], nb,
                       part[t & 1], ctx->d_inf_idx, ctx->d_inf_dist, piv_lds ? 1 : 0);
  hipLaunchKernelGGL(informed_last, dim3(1), dim3(kInfBlock), 0, ctx->stream,
                     part[(m - 1) & 1], nb, m, ctx->d_inf_idx, ctx->d_inf_dist);
  HIPCHK(hipGetLastError());
  return 0;
}

int informed_check_m(gpe_ctx* ctx, int64_t n, int64_t n_cases, int64_t m) {
  char buf[160];
  if (n < 1 || n > INT32_MAX) {
    snprintf(buf, sizeof(buf), "informed_cases: n = %lld individuals (need 1 .. 2^31 - 1)",
             (long long)n);
    return fail(ctx, GPE_E_INVALID, buf);
  }
  if (n_cases < 1 || n_cases >= (1ll << 31)) {
    snprintf(buf, sizeof(buf), "informed_cases: n_cases = %lld (need 1 .. 2^31 - 1)",
             (long long)n_cases);
    return fail(ctx, GPE_E_INVALID, buf);
  }
  if (m < 1 || m > n_cases) {
    snprintf(buf, sizeof(buf), "informed_cases: m = %lld (need 1 .. n_cases = %lld)",
             (long long)m, (long long)n_cases);
    return fail(ctx, GPE_E_INVALID, buf);
  }
  return 0;
}

}  // namespace

int gpe_host_hit_threshold(const double* cases, int64_t n, int64_t n_cases, double eps,
                           uint32_t* out_planes) {
  if (n < 0 || n_cases <= 0 || (n > 0 && (!cases || !out_planes))) return GPE_E_INVALID;
  const int64_t units = (n_cases + 31) / 32;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t w = 0; w < units; ++w) {
      uint32_t bits = 0;
      for (int64_t c = w * 32; c < std::min(n_cases, w * 32 + 32); ++c) {
        const double e = cases[i * n_cases + c];
        if (e <= eps && e - e == 0.0) bits |= 1u << (c - w * 32);
      }
      out_planes[i * units + w] = bits;
    }
  return 0;
}

int gpe_host_informed_cases(const uint32_t* planes, int64_t n, int64_t n_cases, uint64_t seed,
                            int64_t m, int64_t* out_idx, int32_t* out_dist) {
  if (!planes || !out_idx || !out_dist || n < 1 || n > INT32_MAX || n_cases < 1 ||
      n_cases >= (1ll << 31) || m < 1 || m > n_cases)
    return GPE_E_INVALID;
  const int64_t units = (n_cases + 31) / 32, W = (n + 63) / 64;
  std::vector<unsigned long long> Q((size_t)n_cases * (size_t)W, 0ull);   // case-major
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = 0; c < n_cases; ++c)
      if ((planes[i * units + c / 32] >> (c % 32)) & 1u)
        Q[(size_t)c * W + i / 64] |= 1ull << (i % 64);
  std::vector<int32_t> mind((size_t)n_cases, INT32_MAX);
  int64_t last = -1;
  for (int64_t t = 0; t < m; ++t) {
    InfCand best = {-1, 0, 0ull};
    for (int64_t c = 0; c < n_cases; ++c) {
      int32_t md = mind[(size_t)c];
      if (t > 0) {
        if (c == last) {
          md = -1;
        } else if (md >= 0) {
          int acc = 0;
          for (int64_t w = 0; w < W; ++w)
            acc += __builtin_popcountll(Q[(size_t)c * W + w] ^ Q[(size_t)last * W + w]);
          md = std::min(md, acc);
        }
        mind[(size_t)c] = md;
      }
      const InfCand mine = {md, (int32_t)c, informed_key(seed, c)};
      if (informed_better(mine, best)) best = mine;
    }
    last = best.c;
    out_idx[t] = last;
    out_dist[t] = t == 0 ? -1 : best.md;
  }
  return 0;
}

int gpe_informed_cases(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                       double eps, uint64_t seed, int64_t m, int64_t* out_idx,
                       int32_t* out_dist) {
  if (!ctx || !out_idx || !out_dist) return GPE_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HitMatrix hm;
  if (int rc = hit_matrix_which(ctx, "informed_cases", planes, n, n_cases, true, eps, &hm))
    return rc;
  if (int rc = informed_check_m(ctx, hm.n, hm.n_cases, m)) return rc;
  if (int rc = hit_matrix_device(ctx, &hm, true)) return rc;
  if (int rc = launch_informed(ctx, hm.Q, hm.n, hm.n_cases, seed, m)) return rc;
  if (int rc = values_to_host(ctx, out_idx, ctx->d_inf_idx, (size_t)m * sizeof(int64_t)))
    return rc;
  return values_to_host(ctx, out_dist, ctx->d_inf_dist, (size_t)m * sizeof(int32_t));
}
