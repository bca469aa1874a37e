// Part of gpeval.hip's single translation unit (included there once, in
// order, after the values runs): per-case hit planes of the B machine and
// lexicase selection on them — gpe_run_hit_planes, gpe_lexicase_bits,
// gpe_host_hit_planes — and the F machine's run into the same matrix,
// gpe_run_typed_hit_planes (typed classifiers; its pieces are in typed_hits.h).
//
// A hit-planes run is a GPE_MODE_HITS_BITS run whose kernels (b_eval_hits,
// b_eval_lanes_hits: fb_kernels.h) also store each program's hit plane
// ~(T ^ out) & vmask, one bit per case, into ctx->d_hit:
// uint32[n_prog][n_units], case c at bit c % 32 of word c / 32, pad bits 0.
//
// Lexicase on 0/1 values with every case maximised: at a case the best value
// among the candidates is 1 if any candidate hits it, and then exactly the
// hitters survive; otherwise every candidate has 0 and all survive.  With an
// epsilon in [0, 1) the survivors are those with v >= best - eps, the same
// set; automatic epsilon takes the median absolute deviation of a 0/1 sample,
// which is 0 or 0.5, again in [0, 1).  So selLexicase, selEpsilonLexicase
// (0 <= eps < 1) and selAutomaticEpsilonLexicase make the same draws and pick
// the same individuals, and one kernel serves all three.
//
// The filter needs, per case, the set of programs that hit it: the matrix
// transposed, d_hit_t = uint64[32 n_units][W], W = ceil(n / 64), program i at
// bit i % 64 of word i / 64 (hit_transpose, once per run, at the first
// selection).  The candidates are W words; a case step is cand & Q[c] word by
// word, a popcount and one block sum — no per-candidate gather, no values.
#pragma once
namespace {

// One wave: 64 programs (group blockIdx.x) by one 32-case word; 32 ballots,
// lane b keeps case b's.  A block's 4 waves take 4 consecutive words.  Pad
// programs read as 0; the pad cases of the last word are 0 in H already, and
// their rows are written (as zeros) like any other.
__global__ __launch_bounds__(256) void hit_transpose(const uint32_t* __restrict__ H, int64_t n,
                                                     int64_t units, int64_t W,
                                                     unsigned long long* __restrict__ Q) {
  const int lane = threadIdx.x & 63;
  const int64_t g = blockIdx.x;
  const int64_t prog = g * 64 + lane;
  for (int64_t w = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6); w < units;
       w += (int64_t)gridDim.y * 4) {
    const uint32_t v = prog < n ? H[prog * units + w] : 0u;
    unsigned long long mine = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      const unsigned long long m = __builtin_amdgcn_ballot_w64((v >> b) & 1u);
      if (lane == b) mine = m;
    }
    if (lane < 32) Q[(w * 32 + lane) * W + g] = mine;
  }
}

// k lexicase selections on case-major hit planes Q[C][W] (see the head of this
// file), replaying random.shuffle(cases) and random.choice(candidates) on the
// MT19937 state as lexicase_mt does (select_dev.h: MtState, mt_randbelow,
// mt_twist_block, whose strides fix the block at kLexBlock threads).  gmem:
// the candidate words and the permutation in device memory (2 W + C uint32
// words) when they do not fit LDS, reached through the same generic pointers.
// Every thread owns the candidate words tid, tid + kLexBlock, ...: a case step
// reads and writes only its own, so one barrier (the count's) per case.
__global__ __launch_bounds__(kLexBlock) void lexicase_bits_mt(
    const unsigned long long* __restrict__ Q, int64_t n, int64_t C, int64_t W, uint32_t* state,
    int64_t k, int32_t* out, int64_t* status, uint32_t* gmem) {
  extern __shared__ unsigned long long lexb_lds[];
  unsigned long long* cand = gmem ? (unsigned long long*)gmem : lexb_lds;   // [W]
  uint32_t* perm = gmem ? gmem + 2 * W : (uint32_t*)(lexb_lds + W);         // [C]
  __shared__ MtState mt;
  __shared__ int64_t red[2][kLexBlock / 64];
  __shared__ int64_t sh_fail;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < kMtN; i += kLexBlock) mt.buf[0][i] = state[i];
  if (tid == 0) {
    mt.cur = 0;
    mt.idx = (int)state[kMtN];
    mt.next_ok = 0;
    sh_fail = -1;
  }
  __syncthreads();
  for (int64_t sel = 0; sel < k; ++sel) {
    // the next state block, in parallel, when this selection may reach it
    if (!mt.next_ok && mt.idx + 2 * C + 64 >= kMtN) {
      mt_twist_block(mt.buf[mt.cur], mt.buf[mt.cur ^ 1], tid);
      if (tid == 0) mt.next_ok = 1;
    }
    for (int64_t w = tid; w < W; w += kLexBlock) {
      const int64_t left = n - w * 64;
      cand[w] = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    }
    for (int64_t c = tid; c < C; c += kLexBlock) perm[c] = (uint32_t)c;
    __syncthreads();
    if (tid == 0)                                    // random.shuffle(cases)
      for (int64_t i = C - 1; i >= 1; --i) {
        const uint32_t j = mt_randbelow(mt, (uint32_t)(i + 1));
        const uint32_t a = perm[i];
        perm[i] = perm[j];
        perm[j] = a;
      }
    __syncthreads();
    int64_t count = n;
    // this thread's first word of the next case's plane, loaded a step ahead
    unsigned long long q0 = tid < W ? Q[(int64_t)perm[0] * W + tid] : 0ull;
    for (int64_t t = 0; t < C && count > 1; ++t) {
      const unsigned long long* row = Q + (int64_t)perm[t] * W;   // cases.pop(0) order
      const unsigned long long q = q0;
      if (t + 1 < C && tid < W) q0 = Q[(int64_t)perm[t + 1] * W + tid];
      int c1 = 0;                                   // (n <= INT32_MAX)
      if (tid < W) c1 = __builtin_popcountll(cand[tid] & q);
      for (int64_t w = tid + kLexBlock; w < W; w += kLexBlock)
        c1 += __builtin_popcountll(cand[w] & row[w]);
      for (int m = 32; m >= 1; m >>= 1) c1 += __shfl_xor(c1, m, 64);
      if (lane == 0) red[t & 1][wave] = c1;
      __syncthreads();
      int64_t tot = 0;
      for (int q4 = 0; q4 < kLexBlock / 64; ++q4) tot += red[t & 1][q4];
      // some candidate hits the case: the hitters stay; none: all stay
      if (tot > 0 && tot < count) {
        if (tid < W) cand[tid] &= q;
        for (int64_t w = tid + kLexBlock; w < W; w += kLexBlock) cand[w] &= row[w];
        count = tot;
      }
    }
    __syncthreads();
    if (tid == 0) {                                  // random.choice
      if (count == 0) {
        sh_fail = sel;                               // IndexError there
      } else {
        int64_t r = mt_randbelow(mt, (uint32_t)count);
        int64_t pick = -1;
        for (int64_t w = 0; w < W; ++w) {
          unsigned long long bits = cand[w];
          const int pc = __builtin_popcountll(bits);
          if (r < pc) {
            for (int64_t q = 0; q < r; ++q) bits &= bits - 1;
            pick = w * 64 + __builtin_ctzll(bits);
            break;
          }
          r -= pc;
        }
        out[sel] = (int32_t)pick;
      }
    }
    __syncthreads();
    if (sh_fail >= 0) break;
  }
  for (int i = tid; i < kMtN; i += kLexBlock) state[i] = mt.buf[mt.cur][i];
  if (tid == 0) {
    state[kMtN] = (uint32_t)mt.idx;
    *status = sh_fail;
  }
}

// H uint32[n][units] (device) into Q uint64[32 units][W]
int launch_hit_transpose(gpe_ctx* ctx, const uint32_t* H, int64_t n, int64_t units,
                         unsigned long long* Q) {
  const int64_t W = (n + 63) / 64;
  const unsigned gy = (unsigned)std::min<int64_t>((units + 3) / 4, 65535);
  hipLaunchKernelGGL(hit_transpose, dim3((unsigned)W, gy), dim3(256), 0, ctx->stream, H, n,
                     units, W, Q);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

int gpe_host_hit_planes(const uint32_t* result_planes, const uint32_t* out_plane, int64_t n,
                        int64_t n_cases, uint32_t* out) {
  if (n < 0 || n_cases <= 0 || !out_plane || (n > 0 && (!result_planes || !out)))
    return GPE_E_INVALID;
  const int64_t units = (n_cases + 31) / 32;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t w = 0; w < units; ++w) {
      const int64_t rem = n_cases - w * 32;
      const uint32_t vmask = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
      out[i * units + w] = ~(result_planes[i * units + w] ^ out_plane[w]) & vmask;
    }
  return 0;
}

int gpe_run_hit_planes(gpe_ctx* ctx, uint32_t* out_planes, double* out_hi, uint64_t* out_err,
                       uint32_t* out_flags) {
  if (!ctx) return GPE_E_INVALID;
  if (ctx->machine != GPE_MACHINE_B)
    return fail(ctx, GPE_E_ARG,
                "gpe_run_hit_planes needs the B machine (bit-sliced 0/1 cases); the F "
                "machine's per-case runs are gpe_run_cases and gpe_run_abserr_cases");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->hit_valid = ctx->hit_t_valid = false;
  if (ctx->n_prog <= 0) return 0;            // (as gpe_run: nothing to do)
  const size_t np = (size_t)ctx->n_prog;
  const size_t words = np * (size_t)ctx->n_units;
  if (ensure(ctx, &ctx->d_hit, &ctx->hit_cap, words)) return GPE_E_HIP;
  ctx->hits_on = 1;
  const int rc = run_mode(ctx, GPE_MODE_HITS_BITS, ctx->d_hi, ctx->d_lo, ctx->d_err, ctx->d_flags);
  ctx->hits_on = 0;
  if (rc) return rc;
  keep_resident(ctx, GPE_MODE_HITS_BITS, false);
  ctx->hit_n = ctx->n_prog;
  ctx->hit_cases = ctx->n_cases;
  ctx->hit_units = ctx->n_units;
  ctx->hit_valid = true;
  if (int rc_d = results_to_host(ctx, np, out_hi, nullptr, out_err, out_flags)) return rc_d;
  if (out_planes) return values_to_host(ctx, out_planes, ctx->d_hit, words * sizeof(uint32_t));
  return 0;
}

// The F machine's twin (typed_hits.h): a GPE_MODE_HITS_BOOL run of the typed
// classifiers whose routes also store the matches they count.
int gpe_run_typed_hit_planes(gpe_ctx* ctx, uint32_t* out_planes, double* out_hi,
                             uint64_t* out_err, uint32_t* out_flags) {
  if (!ctx) return GPE_E_INVALID;
  if (ctx->machine != GPE_MACHINE_F)
    return fail(ctx, GPE_E_ARG,
                "gpe_run_typed_hit_planes needs the F machine (typed classifiers, "
                "GPE_MODE_HITS_BOOL); the B machine's hit planes are gpe_run_hit_planes");
  if (ctx->prec != GPE_PREC_F64)
    return fail(ctx, GPE_E_ARG, "gpe_run_typed_hit_planes needs fp64 (GPE_PREC_F64): the "
                                "hit planes are the fp64 machine's");
  if (ctx->nt != 1)
    return fail(ctx, GPE_E_ARG, "gpe_run_typed_hit_planes needs exactly one target column "
                                "(the labels)");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->hit_valid = ctx->hit_t_valid = false;
  if (ctx->n_prog <= 0) return 0;            // (as gpe_run: nothing to do)
  const size_t np = (size_t)ctx->n_prog;
  const int64_t units = (ctx->n_cases + 31) / 32;
  const size_t words = np * (size_t)units;
  if (ensure(ctx, &ctx->d_hit, &ctx->hit_cap, words)) return GPE_E_HIP;
  // (every loaded program is in exactly one launch list, and each list's
  // kernel writes all words of its programs' rows: no clear)
  ctx->hits_on = 1;
  const int rc = run_mode(ctx, GPE_MODE_HITS_BOOL, ctx->d_hi, ctx->d_lo, ctx->d_err, ctx->d_flags);
  ctx->hits_on = 0;
  if (rc) return rc;
  keep_resident(ctx, GPE_MODE_HITS_BOOL, false);
  ctx->hit_n = ctx->n_prog;
  ctx->hit_cases = ctx->n_cases;
  ctx->hit_units = units;
  ctx->hit_valid = true;
  if (int rc_d = results_to_host(ctx, np, out_hi, nullptr, out_err, out_flags)) return rc_d;
  if (out_planes) return values_to_host(ctx, out_planes, ctx->d_hit, words * sizeof(uint32_t));
  return 0;
}

int gpe_host_typed_hit_planes(const double* values, const double* labels, int64_t n,
                              int64_t n_cases, uint32_t* out) {
  if (n < 0 || n_cases <= 0 || !labels || (n > 0 && (!values || !out))) return GPE_E_INVALID;
  const int64_t units = (n_cases + 31) / 32;
  for (int64_t i = 0; i < n; ++i) {
    uint32_t* row = out + i * units;
    for (int64_t w = 0; w < units; ++w) row[w] = 0u;
    for (int64_t c = 0; c < n_cases; ++c)       // (nan != 0: bool(nan) is True)
      if ((values[i * n_cases + c] != 0.0) == (labels[c] != 0.0))
        row[c >> 5] |= 1u << (c & 31);
  }
  return 0;
}

int gpe_read_hit_planes(gpe_ctx* ctx, uint32_t* out_planes) {
  if (!ctx || !out_planes) return GPE_E_INVALID;
  if (!ctx->hit_valid || ctx->hit_n <= 0)
    return fail(ctx, GPE_E_STATE, "no hit planes on the device (gpe_run_hit_planes first)");
  HIPCHK(hipSetDevice(ctx->device));
  return values_to_host(ctx, out_planes, ctx->d_hit,
                        (size_t)ctx->hit_n * (size_t)ctx->hit_units * sizeof(uint32_t));
}

int gpe_lexicase_bits(gpe_ctx* ctx, const uint32_t* planes, int64_t n, int64_t n_cases,
                      uint32_t* mt_state, int64_t k, int32_t* out, int64_t* failed) {
  if (!ctx || !mt_state || k < 0 || (k > 0 && !out)) return GPE_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (mt_state[kMtN] > (uint32_t)kMtN)
    return fail(ctx, GPE_E_INVALID, "lexicase_bits: MT19937 position beyond 624");
  if (failed) *failed = -1;
  HitMatrix hm;
  if (int rc = hit_matrix_which(ctx, "lexicase_bits", planes, n, n_cases, false, 0.0, &hm))
    return rc;
  n = hm.n;
  n_cases = hm.n_cases;
  if (n < 0 || n_cases <= 0 || n > INT32_MAX || n_cases >= (1ll << 31))
    return fail(ctx, GPE_E_INVALID, "lexicase_bits: bad or oversized input");
  if (n == 0) {                    // random.choice([]) at the first selection
    if (failed && k > 0) *failed = 0;
    return 0;
  }
  if (k == 0) return 0;
  if (int rc = hit_matrix_device(ctx, &hm, true)) return rc;
  const int64_t W = hm.W;
  const unsigned long long* Q = hm.Q;
  // candidates and permutation: LDS while ceil(n / 32) + n_cases words fit
  // 48 KiB (gpe_lexicase's rule), else device scratch
  const size_t need = (size_t)(2 * W + n_cases) * sizeof(uint32_t);
  const bool in_lds = ((size_t)((n + 31) / 32) + (size_t)n_cases) * 4 <= 48 * 1024;
  const size_t lds = in_lds ? need : 0;
  if (!in_lds && ensure(ctx, &ctx->d_lexb_scratch, &ctx->lexb_scratch_cap, (size_t)(2 * W + n_cases)))
    return GPE_E_HIP;
  if (ensure(ctx, &ctx->d_sel_out, &ctx->sel_out_cap, (size_t)k) ||
      ensure(ctx, &ctx->d_sel_state, &ctx->sel_state_cap, (size_t)kMtN + 2) ||
      ensure(ctx, &ctx->d_lex_status, &ctx->lex_status_cap, 1))
    return GPE_E_HIP;
  HIPCHK(hipMemcpyAsync(ctx->d_sel_state, mt_state, (kMtN + 1) * sizeof(uint32_t),
                        hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipFuncSetAttribute((const void*)lexicase_bits_mt,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)(48 * 1024 + 8)));
  hipLaunchKernelGGL(lexicase_bits_mt, dim3(1), dim3(kLexBlock), lds, ctx->stream, Q, n, n_cases,
                     W, ctx->d_sel_state, k, ctx->d_sel_out, ctx->d_lex_status,
                     in_lds ? (uint32_t*)nullptr : ctx->d_lexb_scratch);
  HIPCHK(hipGetLastError());
  int64_t st = -1;
  HIPCHK(hipMemcpyAsync(&st, ctx->d_lex_status, sizeof(int64_t), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int64_t done = st >= 0 ? st : k;
  if (done)
    HIPCHK(hipMemcpy(out, ctx->d_sel_out, (size_t)done * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(mt_state, ctx->d_sel_state, (kMtN + 1) * sizeof(uint32_t),
                   hipMemcpyDeviceToHost));
  if (failed) *failed = st;
  return 0;
}
