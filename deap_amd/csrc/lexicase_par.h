// Part of gpeval.hip's single translation unit (included there once, after
// case_informed.h): parallel lexicase selection, one workgroup per selection —
// gpe_lexicase_par, gpe_lexicase_bits_par, gpe_host_lexicase_par,
// gpe_lexicase_par_lds_values.
//
// The replaying kernels (lexicase_mt, lexicase_bits_mt) share one MT19937
// stream between their k selections: where selection s + 1 starts in it
// depends on randbelow(count_s), and count_s is the filter's result, so they
// cannot run side by side.  Here the call makes no draw at all: every
// selection's case order and final choice are SplitMix64 keys of one 64-bit
// seed (informed_key, case_informed.h; the rule is in include/gpeval.h), the
// selections are independent, and a grid of persistent blocks takes them
// s = blockIdx.x, blockIdx.x + gridDim.x, ...  Blocks never talk to each
// other; every loop is bounded by k, C, W or the 8 radix passes.
//
// Doubles: the matrix is read case-major, VT = double[C][n] (lexpar_transpose,
// once per per-case run), so a case's values are contiguous in the
// candidates.  The first case of a selection filters the whole population and
// its result depends on the case alone: lexpar_first_case names each
// selection's opening case, lexpar_case_stats filters the population once per
// distinct opening case (best, MAD, survivor mask uint64[W], count), and
// lexpar_select starts from that mask.  Medians are exact: a radix select
// (8 passes of 8 bits) on the order-preserving 64-bit image of the doubles,
// straight from where the values lie (a row of VT, or the compacted
// candidates), with no limit on their number.
//
// Bits: lexpar_select_bits on the case-major hit planes Q[C][W] hit_transpose
// makes; a case step is cand & Q[c], a popcount and a block sum.
#pragma once
namespace {

constexpr int kLexparBlock = 256;                 // 4 waves
constexpr int kLexparBlocksPerCu = 8;             // 32 waves per CU
// LDS of a lexpar_select block: candidate words and compacted values; with
// the reduction slots about 13.1 KiB, so 8 blocks share a CU's 160 KiB.
// Larger sets live in the block's slice of device scratch.
constexpr int64_t kLexparCandWords = 512;         // n <= 32768
constexpr int64_t kLexparLdsValues = 1024;        // compacted doubles
// lexpar_select_bits keeps only candidate words: 2048 (n <= 131072), 16 KiB
constexpr int64_t kLexparBitsCandWords = 2048;

__host__ __device__ inline unsigned long long lexpar_key(unsigned long long seed,
                                                         unsigned long long i) {
  return informed_key(seed, (int64_t)i);            // K(i), mod 2^64
}

// order-preserving image of a non-nan double and its inverse
__host__ __device__ inline unsigned long long lexpar_image(double v) {
  unsigned long long u;
  __builtin_memcpy(&u, &v, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double lexpar_unimage(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  __builtin_memcpy(&v, &u, 8);
  return v;
}

// reduction slots of a block (LDS)
struct LexparSh {
  unsigned long long k[kLexparBlock / 64];
  double d[kLexparBlock / 64];
  int c[kLexparBlock / 64];
  int v[kLexparBlock / 64];
  unsigned int hist[256];
  int bin, rem;
};

// block sum of an int (every thread gets it; all threads call)
__device__ inline int lexpar_block_sum(int v, LexparSh* sh) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();                                  // (slots may still be read from before)
  if ((threadIdx.x & 63) == 0) sh->v[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int q = 0; q < kLexparBlock / 64; ++q) t += sh->v[q];
  return t;
}

// exclusive block scan of an int in thread order, *total the block's sum
__device__ inline int lexpar_block_scan(int v, LexparSh* sh, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  __syncthreads();
  if (lane == 63) sh->v[wave] = x;
  __syncthreads();
  int off = 0, t = 0;
#pragma unroll
  for (int q = 0; q < kLexparBlock / 64; ++q) {
    if (q < wave) off += sh->v[q];
    t += sh->v[q];
  }
  *total = t;
  return off + x - v;
}

// the block's best value (max or min; no nan goes in) and smallest index
__device__ inline void lexpar_block_best(double* best, int* first, bool mx, LexparSh* sh) {
  double b = *best;
  int f = *first;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ob = __shfl_xor(b, m, 64);
    const int of = __shfl_xor(f, m, 64);
    b = mx ? fmax(b, ob) : fmin(b, ob);
    f = min(f, of);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    sh->d[threadIdx.x >> 6] = b;
    sh->c[threadIdx.x >> 6] = f;
  }
  __syncthreads();
  b = sh->d[0];
  f = sh->c[0];
#pragma unroll
  for (int q = 1; q < kLexparBlock / 64; ++q) {
    b = mx ? fmax(b, sh->d[q]) : fmin(b, sh->d[q]);
    f = min(f, sh->c[q]);
  }
  *best = b;
  *first = f;
}

// The next case of selection i0's order: the smallest (K(i0 + c), c) after
// (*pk, *pc), or the smallest of all when !have.  All threads call and get it
// (one exists while fewer than C cases were taken).
__device__ inline void lexpar_next_case(unsigned long long seed, unsigned long long i0, int64_t C,
                                        bool have, unsigned long long* pk, int* pc,
                                        LexparSh* sh) {
  const unsigned long long k0 = *pk;
  const int c0 = *pc;
  unsigned long long bk = ~0ull;
  int bc = INT32_MAX;                               // (every case is below it)
  for (int64_t c = threadIdx.x; c < C; c += kLexparBlock) {
    const unsigned long long key = lexpar_key(seed, i0 + (unsigned long long)c);
    const bool after = !have || key > k0 || (key == k0 && (int)c > c0);
    if (after && (key < bk || (key == bk && (int)c < bc))) {
      bk = key;
      bc = (int)c;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long ok = __shfl_xor(bk, m, 64);
    const int oc = __shfl_xor(bc, m, 64);
    if (ok < bk || (ok == bk && oc < bc)) {
      bk = ok;
      bc = oc;
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    sh->k[threadIdx.x >> 6] = bk;
    sh->c[threadIdx.x >> 6] = bc;
  }
  __syncthreads();
  bk = sh->k[0];
  bc = sh->c[0];
#pragma unroll
  for (int q = 1; q < kLexparBlock / 64; ++q) {
    const unsigned long long ok = sh->k[q];
    const int oc = sh->c[q];
    if (ok < bk || (ok == bk && oc < bc)) {
      bk = ok;
      bc = oc;
    }
  }
  *pk = bk;
  *pc = bc;
}

// the value a median ranks: v itself, or |v - med| (dev)
__device__ __forceinline__ double lexpar_term(double v, bool dev, double med) {
  return dev ? __builtin_fabs(v - med) : v;
}

// kth smallest (0-based) of the m terms of vals (none nan; LDS or device
// memory): radix select on their images, most significant byte first.  A pass
// counts the bytes of the terms that share the prefix found so far in 256
// bins, and the bin that holds rank kth extends the prefix.
__device__ double lexpar_kth(const double* vals, int m, int kth, bool dev, double med,
                             LexparSh* sh) {
  const int tid = threadIdx.x;
  unsigned long long prefix = 0, mask = 0;
  for (int pass = 7; pass >= 0; --pass) {
    const int shift = pass * 8;
    __syncthreads();                                // (bin / rem / hist read before)
    sh->hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += kLexparBlock) {
      const unsigned long long key = lexpar_image(lexpar_term(vals[i], dev, med));
      if ((key & mask) == prefix) atomicAdd(&sh->hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const int mine = (int)sh->hist[tid];
    int total;
    const int before = lexpar_block_scan(mine, sh, &total);
    if (before <= kth && kth < before + mine) {     // exactly one bin
      sh->bin = tid;
      sh->rem = kth - before;
    }
    __syncthreads();
    prefix |= (unsigned long long)sh->bin << shift;
    mask |= 0xffull << shift;
    kth = sh->rem;
  }
  __syncthreads();
  return lexpar_unimage(prefix);
}

// numpy.median of the m terms: nan if any is nan, else the middle one or
// (a + b) / 2 of the two middle ones
__device__ double lexpar_median(const double* vals, int m, bool dev, double med,
                                LexparSh* sh) {
  int nans = 0;
  for (int i = threadIdx.x; i < m; i += kLexparBlock) {
    const double t = lexpar_term(vals[i], dev, med);
    nans += t != t;
  }
  if (lexpar_block_sum(nans, sh)) return __builtin_nan("");
  if (m & 1) return lexpar_kth(vals, m, m / 2, dev, med, sh);
  const double a = lexpar_kth(vals, m, m / 2 - 1, dev, med, sh);
  const double b = lexpar_kth(vals, m, m / 2, dev, med, sh);
  return (a + b) / 2.0;
}

// the survivors' test of a case: plain v == lim, else within lim
__device__ __forceinline__ bool lexpar_keeps(double v, double lim, int mode, bool mx) {
  return mode == 0 ? (v == lim) : (mx ? v >= lim : v <= lim);
}

// V double[n][C] into VT double[C][n] through 32 x 32 LDS tiles (33 columns:
// no bank conflicts on the transposed read); blockDim (32, 8)
__global__ __launch_bounds__(256) void lexpar_transpose(const double* __restrict__ V, int64_t n,
                                                        int64_t C, double* __restrict__ VT) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int64_t c_base = (int64_t)blockIdx.x * 32;
  for (int64_t i_base = (int64_t)blockIdx.y * 32; i_base < n; i_base += (int64_t)gridDim.y * 32) {
    for (int r = ty; r < 32; r += 8) {
      const int64_t i = i_base + r, c = c_base + tx;
      if (i < n && c < C) tile[r][tx] = V[i * C + c];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int64_t c = c_base + r, i = i_base + tx;
      if (c < C && i < n) VT[c * n + i] = tile[tx][r];
    }
    __syncthreads();
  }
}

// first[s]: the case that opens selection s, the argmin of (K(i0 + c), c)
__global__ __launch_bounds__(kLexparBlock) void lexpar_first_case(unsigned long long seed,
                                                                  int64_t C, int64_t k,
                                                                  int32_t* __restrict__ first) {
  __shared__ LexparSh sh;
  for (int64_t s = blockIdx.x; s < k; s += gridDim.x) {
    unsigned long long pk = 0;
    int pc = 0;
    lexpar_next_case(seed, (unsigned long long)s * (unsigned long long)(C + 1), C, false, &pk,
                     &pc, &sh);
    if (threadIdx.x == 0) first[s] = pc;
  }
}

// One block per distinct opening case ucase[u]: the case filters the whole
// population.  masks[u][W]: the survivors, individual i at bit i % 64 of word
// i / 64; counts[u]: how many.
__global__ __launch_bounds__(kLexparBlock) void lexpar_case_stats(
    const double* __restrict__ VT, int64_t n, int64_t W, const int32_t* __restrict__ ucase,
    const uint8_t* __restrict__ maximise, int mode, double eps,
    unsigned long long* __restrict__ masks, int32_t* __restrict__ counts) {
  __shared__ LexparSh sh;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t u = blockIdx.x;
  const int64_t c = ucase[u];
  const double* row = VT + c * n;
  const bool mx = maximise[c] != 0;
  // Python's max / min in index order: nan never replaces, a leading nan stays
  double b = mx ? -__builtin_inf() : __builtin_inf();
  for (int64_t i = tid; i < n; i += kLexparBlock) {
    const double v = row[i];
    if (v == v) b = mx ? fmax(b, v) : fmin(b, v);
  }
  int first = 0;
  lexpar_block_best(&b, &first, mx, &sh);
  const double v0 = row[0];
  if (v0 != v0) b = v0;
  double lim = b;
  if (mode == 1) {
    lim = mx ? b - eps : b + eps;
  } else if (mode == 2) {
    const double med = lexpar_median(row, (int)n, false, 0.0, &sh);
    const double mad = lexpar_median(row, (int)n, true, med, &sh);
    lim = mx ? b - mad : b + mad;
  }
  int cnt = 0;
  for (int64_t base = (int64_t)(tid >> 6) * 64; base < W * 64; base += kLexparBlock) {
    const int64_t i = base + lane;
    const bool ok = i < n && lexpar_keeps(row[i], lim, mode, mx);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    if (lane == 0) {
      masks[u * W + base / 64] = m;
      cnt += __builtin_popcountll(m);
    }
  }
  cnt = lexpar_block_sum(cnt, &sh);
  if (tid == 0) counts[u] = cnt;
}

// The choice: the r-th of the count survivors in index order, r the high half
// of K(i0 + C) * count; no survivor: -1 and the smallest failing s.  Thread t
// owns the candidate words [w0, w1).
__device__ inline void lexpar_choose(const unsigned long long* cand, int64_t w0, int64_t w1,
                                     int count, unsigned long long key, int64_t s,
                                     int32_t* out, unsigned long long* failed, LexparSh* sh) {
  if (count == 0) {
    if (threadIdx.x == 0) {
      out[s] = -1;
      atomicMin(failed, (unsigned long long)s);
    }
    return;
  }
  const int r = (int)__umul64hi(key, (unsigned long long)count);
  int mine = 0;
  for (int64_t w = w0; w < w1; ++w) mine += __builtin_popcountll(cand[w]);
  int total;
  const int before = lexpar_block_scan(mine, sh, &total);
  if (before <= r && r < before + mine) {           // exactly one thread
    int left = r - before;
    for (int64_t w = w0; w < w1; ++w) {
      unsigned long long bits = cand[w];
      const int pc = __builtin_popcountll(bits);
      if (left < pc) {
        for (int q = 0; q < left; ++q) bits &= bits - 1;
        out[s] = (int32_t)(w * 64 + __builtin_ctzll(bits));
        break;
      }
      left -= pc;
    }
  }
}

// The selections on doubles.  first / slot / masks / counts: each selection's
// opening case and the stats slot that holds its survivors (unused for
// n == 1, where no case is looked at).  cand_g: per-block slices of W words
// when W > kLexparCandWords, else null; vals_g: per-block slices of
// vals_stride doubles for candidate sets above kLexparLdsValues (mode 2), or
// null when no set can be that large.
__global__ __launch_bounds__(kLexparBlock) void lexpar_select(
    const double* __restrict__ VT, int64_t n, int64_t C, int64_t W,
    const uint8_t* __restrict__ maximise, int mode, double eps, unsigned long long seed,
    int64_t k, const int32_t* __restrict__ first, const int32_t* __restrict__ slot,
    const unsigned long long* __restrict__ masks, const int32_t* __restrict__ counts,
    int32_t* __restrict__ out, unsigned long long* failed, unsigned long long* cand_g,
    double* vals_g, int64_t vals_stride) {
  __shared__ unsigned long long cand_l[kLexparCandWords];
  __shared__ double vals_l[kLexparLdsValues];
  __shared__ LexparSh sh;
  const int tid = threadIdx.x;
  unsigned long long* cand = cand_g ? cand_g + (int64_t)blockIdx.x * W : cand_l;
  double* vals_big = vals_g ? vals_g + (int64_t)blockIdx.x * vals_stride : nullptr;
  // this thread's candidate words: a contiguous run, so that thread order is
  // index order; nobody else reads or writes them
  const int64_t wpt = (W + kLexparBlock - 1) / kLexparBlock;
  const int64_t w0 = (int64_t)tid * wpt < W ? (int64_t)tid * wpt : W;
  const int64_t w1 = w0 + wpt < W ? w0 + wpt : W;
  for (int64_t s = blockIdx.x; s < k; s += gridDim.x) {
    const unsigned long long i0 = (unsigned long long)s * (unsigned long long)(C + 1);
    int count = 1;
    unsigned long long pk = 0;
    int pc = 0;
    if (n == 1) {
      if (w0 < w1) cand[w0] = 1ull;
    } else {
      const int64_t sl = slot[s];
      for (int64_t w = w0; w < w1; ++w) cand[w] = masks[sl * W + w];
      count = counts[sl];
      pc = first[s];
      pk = lexpar_key(seed, i0 + (unsigned long long)pc);
    }
    for (int64_t t = 1; t < C && count > 1; ++t) {
      lexpar_next_case(seed, i0, C, true, &pk, &pc, &sh);
      const int64_t c = pc;
      const double* row = VT + c * n;
      const bool mx = maximise[c] != 0;
      double b = mx ? -__builtin_inf() : __builtin_inf();
      int fi = INT32_MAX;
      for (int64_t w = w0; w < w1; ++w) {
        unsigned long long bits = cand[w];
        while (bits) {
          const int64_t i = w * 64 + __builtin_ctzll(bits);
          bits &= bits - 1;
          const double v = row[i];
          if ((int)i < fi) fi = (int)i;
          if (v == v) b = mx ? fmax(b, v) : fmin(b, v);
        }
      }
      lexpar_block_best(&b, &fi, mx, &sh);
      const double v0 = row[fi];                    // (count > 1: there is one)
      if (v0 != v0) b = v0;
      double lim = b;
      if (mode == 1) {
        lim = mx ? b - eps : b + eps;
      } else if (mode == 2) {
        // the candidates' values, compacted in index order
        int mine = 0;
        for (int64_t w = w0; w < w1; ++w) mine += __builtin_popcountll(cand[w]);
        int total;
        int pos = lexpar_block_scan(mine, &sh, &total);
        double* vals = count <= kLexparLdsValues ? vals_l : vals_big;
        for (int64_t w = w0; w < w1; ++w) {
          unsigned long long bits = cand[w];
          while (bits) {
            const int64_t i = w * 64 + __builtin_ctzll(bits);
            bits &= bits - 1;
            vals[pos++] = row[i];
          }
        }
        __syncthreads();
        const double med = lexpar_median(vals, count, false, 0.0, &sh);
        const double mad = lexpar_median(vals, count, true, med, &sh);
        lim = mx ? b - mad : b + mad;
      }
      int keep = 0;
      for (int64_t w = w0; w < w1; ++w) {
        unsigned long long bits = cand[w], left = bits;
        while (bits) {
          const int bb = __builtin_ctzll(bits);
          bits &= bits - 1;
          if (!lexpar_keeps(row[w * 64 + bb], lim, mode, mx)) left &= ~(1ull << bb);
        }
        cand[w] = left;
        keep += __builtin_popcountll(left);
      }
      count = lexpar_block_sum(keep, &sh);
    }
    lexpar_choose(cand, w0, w1, count, lexpar_key(seed, i0 + (unsigned long long)C), s, out,
                  failed, &sh);
  }
}

// The selections on case-major hit planes Q[C..][W], every case maximised:
// a case keeps the candidates that hit it when some do, else all of them.
// cand_g: per-block slices of W words when W > kLexparBitsCandWords.
__global__ __launch_bounds__(kLexparBlock) void lexpar_select_bits(
    const unsigned long long* __restrict__ Q, int64_t n, int64_t C, int64_t W,
    unsigned long long seed, int64_t k, int32_t* __restrict__ out, unsigned long long* failed,
    unsigned long long* cand_g) {
  __shared__ unsigned long long cand_l[kLexparBitsCandWords];
  __shared__ LexparSh sh;
  const int tid = threadIdx.x;
  unsigned long long* cand = cand_g ? cand_g + (int64_t)blockIdx.x * W : cand_l;
  const int64_t wpt = (W + kLexparBlock - 1) / kLexparBlock;
  const int64_t w0 = (int64_t)tid * wpt < W ? (int64_t)tid * wpt : W;
  const int64_t w1 = w0 + wpt < W ? w0 + wpt : W;
  for (int64_t s = blockIdx.x; s < k; s += gridDim.x) {
    const unsigned long long i0 = (unsigned long long)s * (unsigned long long)(C + 1);
    for (int64_t w = w0; w < w1; ++w) {
      const int64_t left = n - w * 64;
      cand[w] = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    }
    int count = (int)n;
    unsigned long long pk = 0;
    int pc = 0;
    for (int64_t t = 0; t < C && count > 1; ++t) {
      lexpar_next_case(seed, i0, C, t > 0, &pk, &pc, &sh);
      const unsigned long long* row = Q + (int64_t)pc * W;
      int c1 = 0;
      for (int64_t w = w0; w < w1; ++w) c1 += __builtin_popcountll(cand[w] & row[w]);
      const int tot = lexpar_block_sum(c1, &sh);
      if (tot > 0 && tot < count) {
        for (int64_t w = w0; w < w1; ++w) cand[w] &= row[w];
        count = tot;
      }
    }
    lexpar_choose(cand, w0, w1, count, lexpar_key(seed, i0 + (unsigned long long)C), s, out,
                  failed, &sh);
  }
}

int lexpar_grid(const gpe_ctx* ctx, int64_t k) {
  return (int)std::min<int64_t>(k, (int64_t)kLexparBlocksPerCu * std::max(ctx->cu, 1));
}

int lexpar_check(gpe_ctx* ctx, const char* what, int64_t n, int64_t n_cases, int64_t k) {
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
  if (k < 0) {
    snprintf(buf, sizeof(buf), "%s: k = %lld selections (need >= 0)", what, (long long)k);
    return fail(ctx, GPE_E_INVALID, buf);
  }
  return 0;
}

// out int32[k] and *failed from the device after a select launch
int lexpar_results(gpe_ctx* ctx, int64_t k, int32_t* out, int64_t* failed) {
  unsigned long long st = ~0ull;
  HIPCHK(hipMemcpyAsync(&st, ctx->d_lexp_failed, sizeof(st), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(hipMemcpyAsync(out, ctx->d_sel_out, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (failed) *failed = st == ~0ull ? -1 : (int64_t)st;
  return 0;
}

// the host's median of v (sorted in place): numpy.median
double lexpar_host_median(std::vector<double>& v) {
  for (double x : v)
    if (x != x) return __builtin_nan("");
  std::sort(v.begin(), v.end());
  const size_t m = v.size();
  return (m & 1) ? v[m / 2] : (v[m / 2 - 1] + v[m / 2]) / 2.0;
}

}  // namespace

int64_t gpe_lexicase_par_lds_values(void) { return kLexparLdsValues; }

int gpe_host_lexicase_par(const double* values, int64_t n, int64_t n_cases,
                          const uint8_t* maximise, int mode, double epsilon, uint64_t seed,
                          int64_t k, int32_t* out, int64_t* failed) {
  if (!values || !maximise || n < 1 || n > INT32_MAX || n_cases < 1 || n_cases >= (1ll << 31) ||
      k < 0 || (k > 0 && !out) || mode < 0 || mode > 2)
    return GPE_E_INVALID;
  if (failed) *failed = -1;
  const int64_t C = n_cases;
  std::vector<std::pair<unsigned long long, int64_t>> order((size_t)C);
  std::vector<int64_t> cand, next;
  std::vector<double> vals, dev;
  for (int64_t s = 0; s < k; ++s) {
    const unsigned long long i0 = (unsigned long long)s * (unsigned long long)(C + 1);
    for (int64_t c = 0; c < C; ++c)
      order[(size_t)c] = {lexpar_key(seed, i0 + (unsigned long long)c), c};
    std::sort(order.begin(), order.end());
    cand.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) cand[(size_t)i] = i;
    for (int64_t t = 0; t < C && cand.size() > 1; ++t) {
      const int64_t c = order[(size_t)t].second;
      const bool mx = maximise[c] != 0;
      vals.resize(cand.size());
      for (size_t j = 0; j < cand.size(); ++j) vals[j] = values[cand[j] * C + c];
      double b = vals[0];                           // Python's max / min
      for (size_t j = 1; j < vals.size(); ++j)
        if (mx ? vals[j] > b : vals[j] < b) b = vals[j];
      double lim = b;
      if (mode == 1) {
        lim = mx ? b - epsilon : b + epsilon;
      } else if (mode == 2) {
        dev = vals;
        const double med = lexpar_host_median(dev);
        for (size_t j = 0; j < vals.size(); ++j) dev[j] = __builtin_fabs(vals[j] - med);
        const double mad = lexpar_host_median(dev);
        lim = mx ? b - mad : b + mad;
      }
      next.clear();
      for (size_t j = 0; j < cand.size(); ++j) {
        const double v = vals[j];
        if (mode == 0 ? (v == lim) : (mx ? v >= lim : v <= lim)) next.push_back(cand[j]);
      }
      cand.swap(next);
    }
    if (cand.empty()) {
      out[s] = -1;
      if (failed && *failed < 0) *failed = s;
      continue;
    }
    const unsigned long long key = lexpar_key(seed, i0 + (unsigned long long)C);
    const unsigned long long r =
        (unsigned long long)(((unsigned __int128)key * (unsigned __int128)cand.size()) >> 64);
    out[s] = (int32_t)cand[(size_t)r];
  }
  return 0;
}

int gpe_lexicase_par(gpe_ctx* ctx, const double* values, int64_t n, int64_t n_cases,
                     const uint8_t* maximise, int mode, double epsilon, uint64_t seed,
                     int64_t k, int32_t* out, int64_t* failed) {
  if (!ctx || !maximise || (k > 0 && !out)) return GPE_E_INVALID;
  if (mode < 0 || mode > 2) return fail(ctx, GPE_E_INVALID, "lexicase_par: mode must be 0, 1 or 2");
  HIPCHK(hipSetDevice(ctx->device));
  if (failed) *failed = -1;
  if (!values) {                    // the matrix of the last per-case run
    if (!ctx->d_case_out || ctx->n_prog <= 0 || ctx->case_stale)
      return fail(ctx, GPE_E_STATE, "no per-case values on the device");
    n = ctx->n_prog;
    n_cases = ctx->n_cases;
  }
  if (int rc = lexpar_check(ctx, "lexicase_par", n, n_cases, k)) return rc;
  if (k == 0) return 0;
  const int64_t C = n_cases, W = (n + 63) / 64;
  const size_t cells = (size_t)n * (size_t)C;
  // the case-major matrix
  const double* VT = nullptr;
  const dim3 tgrid((unsigned)((C + 31) / 32), (unsigned)std::min<int64_t>((n + 31) / 32, 65535));
  if (values) {
    if (ensure(ctx, &ctx->d_lex_val, &ctx->lex_val_cap, cells) ||
        ensure(ctx, &ctx->d_lexp_vt, &ctx->lexp_vt_cap, cells))
      return GPE_E_HIP;
    HIPCHK(hipMemcpyAsync(ctx->d_lex_val, values, cells * sizeof(double), hipMemcpyHostToDevice,
                          ctx->stream));
    hipLaunchKernelGGL(lexpar_transpose, tgrid, dim3(32, 8), 0, ctx->stream, ctx->d_lex_val, n, C,
                       ctx->d_lexp_vt);
    HIPCHK(hipGetLastError());
    VT = ctx->d_lexp_vt;
  } else {
    if (!ctx->case_t_valid || ctx->case_t_n != n || ctx->case_t_cases != C) {
      ctx->case_t_valid = false;
      if (ensure(ctx, &ctx->d_case_t, &ctx->case_t_cap, cells)) return GPE_E_HIP;
      hipLaunchKernelGGL(lexpar_transpose, tgrid, dim3(32, 8), 0, ctx->stream, ctx->d_case_out, n,
                         C, ctx->d_case_t);
      HIPCHK(hipGetLastError());
      ctx->case_t_n = n;
      ctx->case_t_cases = C;
      ctx->case_t_valid = true;
    }
    VT = ctx->d_case_t;
  }
  if (ensure(ctx, &ctx->d_lex_max, &ctx->lex_max_cap, (size_t)C) ||
      ensure(ctx, &ctx->d_sel_out, &ctx->sel_out_cap, (size_t)k) ||
      ensure(ctx, &ctx->d_lexp_first, &ctx->lexp_first_cap, (size_t)k) ||
      ensure(ctx, &ctx->d_lexp_slot, &ctx->lexp_slot_cap, (size_t)k) ||
      ensure(ctx, &ctx->d_lexp_failed, &ctx->lexp_failed_cap, 1))
    return GPE_E_HIP;
  HIPCHK(hipMemcpyAsync(ctx->d_lex_max, maximise, (size_t)C, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_lexp_failed, 0xff, sizeof(unsigned long long), ctx->stream));
  const int grid = lexpar_grid(ctx, k);
  int max_count = 1;
  if (n > 1) {
    // each selection's opening case, and the distinct ones among them
    hipLaunchKernelGGL(lexpar_first_case, dim3((unsigned)grid), dim3(kLexparBlock), 0, ctx->stream,
                       seed, C, k, ctx->d_lexp_first);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> first((size_t)k);
    HIPCHK(hipMemcpyAsync(first.data(), ctx->d_lexp_first, (size_t)k * sizeof(int32_t),
                          hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> ucase(first);
    std::sort(ucase.begin(), ucase.end());
    ucase.erase(std::unique(ucase.begin(), ucase.end()), ucase.end());
    if (ucase.front() < 0 || ucase.back() >= C)
      return fail(ctx, GPE_E_HIP, "lexicase_par: an opening case out of range");
    const size_t U = ucase.size();
    std::vector<int32_t> slot((size_t)k);
    for (int64_t s = 0; s < k; ++s)
      slot[(size_t)s] = (int32_t)(std::lower_bound(ucase.begin(), ucase.end(), first[(size_t)s]) -
                                  ucase.begin());
    if (ensure(ctx, &ctx->d_lexp_ucase, &ctx->lexp_ucase_cap, U) ||
        ensure(ctx, &ctx->d_lexp_masks, &ctx->lexp_masks_cap, U * (size_t)W) ||
        ensure(ctx, &ctx->d_lexp_counts, &ctx->lexp_counts_cap, U))
      return GPE_E_HIP;
    HIPCHK(hipMemcpyAsync(ctx->d_lexp_ucase, ucase.data(), U * sizeof(int32_t),
                          hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_lexp_slot, slot.data(), (size_t)k * sizeof(int32_t),
                          hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(lexpar_case_stats, dim3((unsigned)U), dim3(kLexparBlock), 0, ctx->stream, VT,
                       n, W, ctx->d_lexp_ucase, ctx->d_lex_max, mode, epsilon, ctx->d_lexp_masks,
                       ctx->d_lexp_counts);
    HIPCHK(hipGetLastError());
    // (the sources of the two uploads must outlive them; the counts size the
    // scratch of the medians)
    std::vector<int32_t> counts(U);
    HIPCHK(hipMemcpyAsync(counts.data(), ctx->d_lexp_counts, U * sizeof(int32_t),
                          hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int32_t c : counts) max_count = std::max(max_count, (int)c);
    if (max_count > n) return fail(ctx, GPE_E_HIP, "lexicase_par: a survivor count out of range");
  }
  // per-block scratch where LDS does not hold the set
  unsigned long long* cand_g = nullptr;
  double* vals_g = nullptr;
  int64_t vals_stride = 0;
  if (W > kLexparCandWords) {
    if (ensure(ctx, &ctx->d_lexp_cand, &ctx->lexp_cand_cap, (size_t)grid * (size_t)W))
      return GPE_E_HIP;
    cand_g = ctx->d_lexp_cand;
  }
  if (mode == 2 && max_count > kLexparLdsValues) {
    vals_stride = max_count;
    if (ensure(ctx, &ctx->d_lexp_vals, &ctx->lexp_vals_cap, (size_t)grid * (size_t)vals_stride))
      return GPE_E_HIP;
    vals_g = ctx->d_lexp_vals;
  }
  hipLaunchKernelGGL(lexpar_select, dim3((unsigned)grid), dim3(kLexparBlock), 0, ctx->stream, VT, n,
                     C, W, ctx->d_lex_max, mode, epsilon, seed, k, ctx->d_lexp_first,
                     ctx->d_lexp_slot, ctx->d_lexp_masks, ctx->d_lexp_counts, ctx->d_sel_out,
                     ctx->d_lexp_failed, cand_g, vals_g, vals_stride);
  HIPCHK(hipGetLastError());
  return lexpar_results(ctx, k, out, failed);
}

int gpe_lexicase_bits_par(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                          uint64_t seed, int64_t k, int32_t* out, int64_t* failed) {
  if (!ctx || (k > 0 && !out)) return GPE_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (failed) *failed = -1;
  HitMatrix hm;
  if (int rc = hit_matrix_which(ctx, "lexicase_bits_par", planes, n, n_cases, false, 0.0, &hm))
    return rc;
  n = hm.n;
  n_cases = hm.n_cases;
  if (int rc = lexpar_check(ctx, "lexicase_bits_par", n, n_cases, k)) return rc;
  if (k == 0) return 0;
  if (int rc = hit_matrix_device(ctx, &hm, true)) return rc;
  const int64_t W = hm.W;
  const unsigned long long* Q = hm.Q;
  const int grid = lexpar_grid(ctx, k);
  if (ensure(ctx, &ctx->d_sel_out, &ctx->sel_out_cap, (size_t)k) ||
      ensure(ctx, &ctx->d_lexp_failed, &ctx->lexp_failed_cap, 1))
    return GPE_E_HIP;
  unsigned long long* cand_g = nullptr;
  if (W > kLexparBitsCandWords) {
    if (ensure(ctx, &ctx->d_lexp_cand, &ctx->lexp_cand_cap, (size_t)grid * (size_t)W))
      return GPE_E_HIP;
    cand_g = ctx->d_lexp_cand;
  }
  HIPCHK(hipMemsetAsync(ctx->d_lexp_failed, 0xff, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(lexpar_select_bits, dim3((unsigned)grid), dim3(kLexparBlock), 0, ctx->stream,
                     Q, n, n_cases, W, seed, k, ctx->d_sel_out, ctx->d_lexp_failed, cand_g);
  HIPCHK(hipGetLastError());
  return lexpar_results(ctx, k, out, failed);
}
