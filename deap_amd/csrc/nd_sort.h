// Part of gpeval.hip's single translation unit (included there once, after
// dalex.h): non-dominated sorting for NSGA-II selection.  The rule (dominance,
// the order inside a front, the stop) is in include/gpeval.h at gpe_nd_sort.
//
// The matrix lives objective-major on the device (WT[j][row]) so that a tile of
// candidate dominators loads coalesced.  nd_counts gives every row its number
// of dominators (a thread owns a row, tiles of the others stream through LDS;
// the candidate range is split over blockIdx.y and combined by integer
// atomicAdd, so the counts do not depend on scheduling).  nd_front0 appends the
// rows with count 0; nd_peel scans, for every unranked row, the ordered list of
// the current front through LDS, subtracts the dominators found, keeps the
// largest position and appends the rows that reach 0 with the key (P, row).
// The appends land in the order the atomics fire; a radix sort of the distinct
// keys makes the front's order the rule's, whatever that order was.  The host
// reads two counters back per front (rows ranked, individuals covered) and
// nothing else until the final order.  m == 1 is one sort of the values.
#pragma once
// (gpeval.hip includes this inside its extern "C" block: the templates need
// C++ linkage)
extern "C++" {
namespace {

constexpr int kNdMaxM = 32;

// The kernels' geometry: B threads (rows) per block, T candidates per LDS tile.
// M > 0: the row's M values in registers; M == 0: any m <= kNdMaxM, the rows'
// values in LDS (48 KiB a block with the tile).  (Enumerators: a static
// constexpr member here makes the host pass of this translation unit diagnose
// the asm cores' device-only constraints.)
template <int M>
struct NdGeom {
  enum : int { B = 256, T = 256, R = M, OWN = 1 };
};
template <>
struct NdGeom<0> {
  enum : int { B = 128, T = 64, R = kNdMaxM, OWN = kNdMaxM * 128 };
};

// A thread's own row d, and the test "tile column q dominates it":
// p >= d in every objective and p > d in one (Fitness.dominates; nan-free).
template <int M>
struct NdRow {
  double v[M];
  __device__ __forceinline__ void load(const double* __restrict__ WT, int64_t n, int64_t d,
                                       double*, int, int) {
#pragma unroll
    for (int j = 0; j < M; ++j) v[j] = WT[(size_t)j * (size_t)n + (size_t)d];
  }
  __device__ __forceinline__ bool dominated_by(const double* tile, int T, int q, int) const {
    bool ge = true, gt = false;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double p = tile[j * T + q];
      ge &= p >= v[j];
      gt |= p > v[j];
    }
    return ge && gt;
  }
};
template <>
struct NdRow<0> {
  const double* own;
  int B;
  __device__ __forceinline__ void load(const double* __restrict__ WT, int64_t n, int64_t d,
                                       double* own_lds, int B_, int m) {
    own = own_lds + threadIdx.x;
    B = B_;
    for (int j = 0; j < m; ++j) own_lds[j * B_ + threadIdx.x] = WT[(size_t)j * (size_t)n + (size_t)d];
  }
  __device__ __forceinline__ bool dominated_by(const double* tile, int T, int q, int m) const {
    bool gt = false;
    for (int j = 0; j < m; ++j) {
      const double p = tile[j * T + q], v = own[j * B];
      if (!(p >= v)) return false;
      gt |= p > v;
    }
    return gt;
  }
};

// cnt[d] += #{p in this block's slice of [0, n) : p dominates d}
template <int M>
__global__ __launch_bounds__(NdGeom<M>::B) void nd_counts(const double* __restrict__ WT,
                                                          int64_t n, int m, int64_t per,
                                                          int32_t* __restrict__ cnt) {
  constexpr int B = NdGeom<M>::B, T = NdGeom<M>::T;
  __shared__ double tile[NdGeom<M>::R * T];
  __shared__ double own[NdGeom<M>::OWN];
  const int t = threadIdx.x;
  const int64_t d = (int64_t)blockIdx.x * B + t;
  const bool live = d < n;
  NdRow<M> row;
  if (live) row.load(WT, n, d, own, B, m);
  const int64_t p0 = (int64_t)blockIdx.y * per, p1 = p0 + per < n ? p0 + per : n;
  int32_t c = 0;
  for (int64_t base = p0; base < p1; base += T) {
    const int nt = p1 - base < T ? (int)(p1 - base) : T;
    __syncthreads();
    if (t < nt)
      for (int j = 0; j < m; ++j) tile[j * T + t] = WT[(size_t)j * (size_t)n + (size_t)(base + t)];
    __syncthreads();
    if (live)
      for (int q = 0; q < nt; ++q) c += row.dominated_by(tile, T, q, m) ? 1 : 0;
  }
  if (live && c) atomicAdd(&cnt[d], c);
}

// Append `key` of the flagged lanes to keys[ctr[0]...] and add their `mu` to
// ctr[1]: one pair of atomics per wave.  Every lane of the wave calls this.
__device__ __forceinline__ void nd_append(bool flag, unsigned long long key, int32_t mu,
                                          unsigned long long* __restrict__ keys,
                                          unsigned long long* __restrict__ ctr) {
  const unsigned long long bal = __ballot(flag);
  if (!bal) return;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long musum = flag ? (unsigned long long)mu : 0ull;
  for (int off = 32; off >= 1; off >>= 1) musum += __shfl_xor(musum, off);
  const int leader = __ffsll((long long)bal) - 1;
  unsigned long long base = 0;
  if (lane == leader) {
    base = atomicAdd(&ctr[0], (unsigned long long)__popcll(bal));
    atomicAdd(&ctr[1], musum);
  }
  base = __shfl(base, leader);
  if (flag) keys[base + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull))] = key;
}

// front 0: the rows nobody dominates, key = row (P = 0); ranked rows get -1
__global__ __launch_bounds__(256) void nd_front0(int32_t* __restrict__ cnt,
                                                 const int32_t* __restrict__ mult, int64_t n,
                                                 unsigned long long* __restrict__ keys,
                                                 unsigned long long* __restrict__ ctr) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool flag = d < n && cnt[d] == 0;
  if (flag) cnt[d] = -1;
  nd_append(flag, (unsigned long long)(flag ? d : 0), flag && mult ? mult[d] : 1, keys, ctr);
}

// One peel: the current front is order[fs .. fs + fc).  Every unranked row
// loses its dominators there; a row that reaches 0 is appended with the key
// (P << db) | row, P the largest front position among its dominators.
template <int M>
__global__ __launch_bounds__(NdGeom<M>::B) void nd_peel(
    const double* __restrict__ WT, int64_t n, int m, const int32_t* __restrict__ order,
    int64_t fs, int64_t fc, int db, int32_t* __restrict__ cnt, const int32_t* __restrict__ mult,
    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ ctr) {
  constexpr int B = NdGeom<M>::B, T = NdGeom<M>::T;
  __shared__ double tile[NdGeom<M>::R * T];
  __shared__ double own[NdGeom<M>::OWN];
  const int t = threadIdx.x;
  const int64_t d = (int64_t)blockIdx.x * B + t;
  const bool live = d < n && cnt[d] > 0;
  if (!__syncthreads_or(live ? 1 : 0)) return;
  NdRow<M> row;
  if (live) row.load(WT, n, d, own, B, m);
  int32_t found = 0;
  int64_t P = 0;
  for (int64_t base = 0; base < fc; base += T) {
    const int nt = fc - base < T ? (int)(fc - base) : T;
    __syncthreads();
    if (t < nt) {
      const size_t p = (size_t)order[fs + base + t];
      for (int j = 0; j < m; ++j) tile[j * T + t] = WT[(size_t)j * (size_t)n + p];
    }
    __syncthreads();
    if (live)
      for (int q = 0; q < nt; ++q)
        if (row.dominated_by(tile, T, q, m)) {
          ++found;
          P = base + q;
        }
  }
  bool flag = false;
  if (live && found) {
    const int32_t c = cnt[d] - found;
    flag = c == 0;
    cnt[d] = flag ? -1 : c;
  }
  nd_append(flag, flag ? ((unsigned long long)P << db) | (unsigned long long)d : 0ull,
            flag && mult ? mult[d] : 1, keys, ctr);
}

// the sorted keys' rows into the order
__global__ __launch_bounds__(256) void nd_rows_of_keys(const unsigned long long* __restrict__ keys,
                                                       int64_t c, int db,
                                                       int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < c) out[i] = (int32_t)(keys[i] & ((1ull << db) - 1ull));
}

// m == 1: keys that sort ascending as the values sort descending (-0.0 as
// 0.0), and the rows 0 .. n - 1 as the sort's payload
__global__ __launch_bounds__(256) void nd_keys1(const double* __restrict__ w, int64_t n,
                                                unsigned long long* __restrict__ keys,
                                                int32_t* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = w[i] == 0.0 ? 0.0 : w[i];
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  b = (b >> 63) ? ~b : b | 0x8000000000000000ull;
  keys[i] = ~b;
  rows[i] = (int32_t)i;
}

template <int M>
void nd_launch_counts(gpe_ctx* ctx, int64_t n, int m) {
  constexpr int B = NdGeom<M>::B, T = NdGeom<M>::T;
  const int64_t bx = (n + B - 1) / B, tiles = (n + T - 1) / T;
  // enough blocks to fill the device when the rows alone give few
  int64_t split = std::min<int64_t>(std::max<int64_t>(2048 / bx, 1), std::min<int64_t>(tiles, 1024));
  const int64_t per = (tiles + split - 1) / split * T;
  split = (n + per - 1) / per;
  hipLaunchKernelGGL((nd_counts<M>), dim3((unsigned)bx, (unsigned)split), dim3(B), 0, ctx->stream,
                     (const double*)ctx->d_nd_wt, n, m, per, ctx->d_nd_cnt);
}
template <int M>
void nd_launch_peel(gpe_ctx* ctx, int64_t n, int m, int64_t fs, int64_t fc, int db,
                    const int32_t* d_mult) {
  constexpr int B = NdGeom<M>::B;
  hipLaunchKernelGGL((nd_peel<M>), dim3((unsigned)((n + B - 1) / B)), dim3(B), 0, ctx->stream,
                     (const double*)ctx->d_nd_wt, n, m, (const int32_t*)ctx->d_nd_order, fs, fc,
                     db, ctx->d_nd_cnt, d_mult, ctx->d_nd_keys, ctx->d_nd_ctr);
}

int nd_bits(int64_t x) {      // the bits that hold 0 .. x - 1 (at least 1)
  int b = 1;
  while (((int64_t)1 << b) < x) ++b;
  return b;
}

// What both sides check: the sizes, then the values.  0, or the code with msg.
int nd_check(const double* w, const int32_t* mult, int64_t n, int64_t m, int64_t k,
             std::string* msg) {
  char buf[160];
  if (n < 1 || n > INT32_MAX) {
    snprintf(buf, sizeof(buf), "nd_sort: n = %lld rows (need 1 .. 2^31 - 1)", (long long)n);
    *msg = buf;
    return GPE_E_INVALID;
  }
  if (m < 1 || m > kNdMaxM) {
    snprintf(buf, sizeof(buf), "nd_sort: m = %lld objectives (need 1 .. %d)", (long long)m,
             kNdMaxM);
    *msg = buf;
    return GPE_E_INVALID;
  }
  if (k < 0) {
    snprintf(buf, sizeof(buf), "nd_sort: k = %lld (need >= 0)", (long long)k);
    *msg = buf;
    return GPE_E_INVALID;
  }
  if (!w) {
    *msg = "nd_sort: w is NULL";
    return GPE_E_INVALID;
  }
  const size_t nm = (size_t)n * (size_t)m;
  for (size_t q = 0; q < nm; ++q)
    if (w[q] != w[q]) {
      snprintf(buf, sizeof(buf), "nd_sort: nan at row %lld, objective %lld",
               (long long)(q / (size_t)m), (long long)(q % (size_t)m));
      *msg = buf;
      return GPE_E_ARG;
    }
  if (mult)
    for (int64_t i = 0; i < n; ++i)
      if (mult[i] < 1) {
        snprintf(buf, sizeof(buf), "nd_sort: mult[%lld] = %d (need >= 1)", (long long)i,
                 (int)mult[i]);
        *msg = buf;
        return GPE_E_ARG;
      }
  return 0;
}

// min(total individuals, k)
int64_t nd_target(const int32_t* mult, int64_t n, int64_t k) {
  int64_t total = n;
  if (mult) {
    total = 0;
    for (int64_t i = 0; i < n; ++i) total += mult[i];
  }
  return std::min(total, k);
}

// m == 1: `order` holds the rows by (value descending, row ascending); the
// fronts are its runs of equal values, cut where the stop rule says
void nd_segment1(const double* w, const int32_t* mult, int64_t n, int64_t target,
                 int first_front_only, const int32_t* order, int64_t* front_end,
                 int64_t* n_fronts, int64_t* n_ranked) {
  int64_t covered = 0, nf = 0, i = 0;
  while (i < n) {
    const double v = w[order[i]];
    while (i < n && w[order[i]] == v) covered += mult ? mult[order[i]] : 1, ++i;
    front_end[nf++] = i;
    if (first_front_only || covered >= target) break;
  }
  *n_fronts = nf;
  *n_ranked = i;
}

bool nd_host_dominates(const double* p, const double* d, int64_t m) {
  bool gt = false;
  for (int64_t j = 0; j < m; ++j) {
    if (!(p[j] >= d[j])) return false;
    gt |= p[j] > d[j];
  }
  return gt;
}

}  // namespace
}  // extern "C++"

int gpe_host_nd_sort(const double* w, const int32_t* mult, int64_t n, int64_t m, int64_t k,
                     int first_front_only, int32_t* order, int64_t* front_end,
                     int64_t* n_fronts, int64_t* n_ranked) {
  std::string msg;
  if (int rc = nd_check(w, mult, n, m, k, &msg)) return rc;
  if (!order || !front_end || !n_fronts || !n_ranked) return GPE_E_INVALID;
  *n_fronts = *n_ranked = 0;
  if (k == 0) return 0;
  const int64_t target = nd_target(mult, n, k);
  if (m == 1) {
    std::vector<int32_t> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return w[a] > w[b]; });
    std::copy(idx.begin(), idx.end(), order);
    nd_segment1(w, mult, n, target, first_front_only, order, front_end, n_fronts, n_ranked);
    return 0;
  }
  std::vector<int32_t> cnt((size_t)n, 0);
  for (int64_t d = 0; d < n; ++d)
    for (int64_t p = 0; p < n; ++p)
      cnt[(size_t)d] += nd_host_dominates(w + p * m, w + d * m, m) ? 1 : 0;
  int64_t ranked = 0, covered = 0, nf = 0;
  for (int64_t d = 0; d < n; ++d)
    if (cnt[(size_t)d] == 0) {
      cnt[(size_t)d] = -1;
      order[ranked++] = (int32_t)d;
      covered += mult ? mult[d] : 1;
    }
  front_end[nf++] = ranked;
  int64_t fs = 0;
  std::vector<std::pair<int64_t, int32_t>> cand;
  while (!first_front_only && covered < target) {
    const int64_t fc = ranked - fs;
    cand.clear();
    for (int64_t d = 0; d < n; ++d) {
      if (cnt[(size_t)d] <= 0) continue;
      int32_t found = 0;
      int64_t P = 0;
      for (int64_t q = 0; q < fc; ++q)
        if (nd_host_dominates(w + (int64_t)order[fs + q] * m, w + d * m, m)) ++found, P = q;
      if (found && (cnt[(size_t)d] -= found) == 0) {
        cnt[(size_t)d] = -1;
        cand.emplace_back(P, (int32_t)d);
      }
    }
    if (cand.empty()) return GPE_E_STATE;   // (cannot happen: dominance is a strict order)
    std::sort(cand.begin(), cand.end());
    fs = ranked;
    for (const auto& c : cand) {
      order[ranked++] = c.second;
      covered += mult ? mult[c.second] : 1;
    }
    front_end[nf++] = ranked;
  }
  *n_fronts = nf;
  *n_ranked = ranked;
  return 0;
}

int gpe_nd_sort(gpe_ctx* ctx, const double* w, const int32_t* mult, int64_t n, int64_t m,
                int64_t k, int first_front_only, int32_t* order, int64_t* front_end,
                int64_t* n_fronts, int64_t* n_ranked) {
  if (!ctx) return GPE_E_INVALID;
  std::string msg;
  if (int rc = nd_check(w, mult, n, m, k, &msg)) return fail(ctx, rc, msg);
  if (!order || !front_end || !n_fronts || !n_ranked)
    return fail(ctx, GPE_E_INVALID, "nd_sort: an output is NULL");
  *n_fronts = *n_ranked = 0;
  ctx->nd_ms = 0;
  ctx->nd_fronts = 0;
  if (k == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t target = nd_target(mult, n, k);
  const size_t nm = (size_t)n * (size_t)m;
  if (ensure(ctx, &ctx->d_nd_wt, &ctx->nd_wt_cap, nm) ||
      ensure(ctx, &ctx->d_nd_keys, &ctx->nd_keys_cap, (size_t)n) ||
      ensure(ctx, &ctx->d_nd_sorted, &ctx->nd_sorted_cap, (size_t)n) ||
      ensure(ctx, &ctx->d_nd_order, &ctx->nd_order_cap, (size_t)n) ||
      ensure(ctx, &ctx->d_nd_cnt, &ctx->nd_cnt_cap, (size_t)n) ||
      ensure(ctx, &ctx->d_nd_mult, &ctx->nd_mult_cap, (size_t)n) ||
      ensure(ctx, &ctx->d_nd_ctr, &ctx->nd_ctr_cap, 2))
    return GPE_E_HIP;
  float ms = 0;
  size_t tmp_bytes = 0;
  if (m == 1) {
    const HostPiece pc[1] = {{ctx->d_nd_wt, w, nm * sizeof(double)}};
    if (int rc = h2d_staged(ctx, pc, 1)) return rc;
    // (the payload goes through d_nd_cnt: int32[n], unused on this path)
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, ctx->d_nd_keys, ctx->d_nd_sorted,
                                              ctx->d_nd_cnt, ctx->d_nd_order, (int)n, 0, 64,
                                              ctx->stream));
    if (ensure(ctx, &ctx->d_nd_tmp, &ctx->nd_tmp_cap, tmp_bytes)) return GPE_E_HIP;
    HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
    hipLaunchKernelGGL(nd_keys1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const double*)ctx->d_nd_wt, n, ctx->d_nd_keys, ctx->d_nd_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(ctx->d_nd_tmp, tmp_bytes, ctx->d_nd_keys,
                                              ctx->d_nd_sorted, ctx->d_nd_cnt, ctx->d_nd_order,
                                              (int)n, 0, 64, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
    if (int rc = values_to_host(ctx, order, ctx->d_nd_order, (size_t)n * sizeof(int32_t)))
      return rc;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_redo[0], ctx->ev_redo[1]));
    nd_segment1(w, mult, n, target, first_front_only, order, front_end, n_fronts, n_ranked);
    ctx->nd_ms = ms;
    ctx->nd_fronts = *n_fronts;
    return 0;
  }
  // objective-major on the way in
  {
    std::vector<double> wt(nm);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < m; ++j) wt[(size_t)j * (size_t)n + (size_t)i] = w[i * m + j];
    const HostPiece pc[2] = {{ctx->d_nd_wt, wt.data(), nm * sizeof(double)},
                             {ctx->d_nd_mult, mult, mult ? (size_t)n * sizeof(int32_t) : 0}};
    if (int rc = h2d_staged(ctx, pc, 2)) return rc;
  }
  const int32_t* d_mult = mult ? ctx->d_nd_mult : nullptr;
  unsigned long long* h_ctr = (unsigned long long*)pinned(ctx, 2 * sizeof(unsigned long long));
  if (!h_ctr) return fail(ctx, GPE_E_HIP, "hipHostMalloc (nd_sort)");
  const int im = (int)m, db = nd_bits(n);
  HIPCHK(hipMemsetAsync(ctx->d_nd_cnt, 0, (size_t)n * sizeof(int32_t), ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_nd_ctr, 0, 2 * sizeof(unsigned long long), ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
  switch (im) {
    case 2: nd_launch_counts<2>(ctx, n, im); break;
    case 3: nd_launch_counts<3>(ctx, n, im); break;
    case 4: nd_launch_counts<4>(ctx, n, im); break;
    default: nd_launch_counts<0>(ctx, n, im); break;
  }
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(nd_front0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                     ctx->d_nd_cnt, d_mult, n, ctx->d_nd_keys, ctx->d_nd_ctr);
  HIPCHK(hipGetLastError());
  int64_t ranked = 0, covered = 0, nf = 0, fs = 0, fc = 0;
  for (;;) {
    // the one readback per front: rows ranked and individuals covered so far
    HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(h_ctr, ctx->d_nd_ctr, 2 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float seg = 0;
    HIPCHK(hipEventElapsedTime(&seg, ctx->ev_redo[0], ctx->ev_redo[1]));
    ms += seg;
    const int64_t c = (int64_t)h_ctr[0] - ranked;
    covered = (int64_t)h_ctr[1];
    if (c <= 0 || (int64_t)h_ctr[0] > n)
      return fail(ctx, GPE_E_HIP, "nd_sort: a peel ranked no row");
    // the front's order: its keys sorted (the previous front's size bounds P)
    const int end_bit = db + (nf == 0 ? 0 : nd_bits(fc));
    HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, ctx->d_nd_keys + ranked,
                                             ctx->d_nd_sorted, (int)c, 0, end_bit, ctx->stream));
    if (ensure(ctx, &ctx->d_nd_tmp, &ctx->nd_tmp_cap, tmp_bytes)) return GPE_E_HIP;
    HIPCHK(hipEventRecord(ctx->ev_redo[0], ctx->stream));
    HIPCHK(hipcub::DeviceRadixSort::SortKeys(ctx->d_nd_tmp, tmp_bytes, ctx->d_nd_keys + ranked,
                                             ctx->d_nd_sorted, (int)c, 0, end_bit, ctx->stream));
    hipLaunchKernelGGL(nd_rows_of_keys, dim3((unsigned)((c + 255) / 256)), dim3(256), 0,
                       ctx->stream, (const unsigned long long*)ctx->d_nd_sorted, c, db,
                       ctx->d_nd_order + ranked);
    HIPCHK(hipGetLastError());
    fs = ranked;
    fc = c;
    ranked += c;
    front_end[nf++] = ranked;
    if (first_front_only || covered >= target) break;
    switch (im) {
      case 2: nd_launch_peel<2>(ctx, n, im, fs, fc, db, d_mult); break;
      case 3: nd_launch_peel<3>(ctx, n, im, fs, fc, db, d_mult); break;
      case 4: nd_launch_peel<4>(ctx, n, im, fs, fc, db, d_mult); break;
      default: nd_launch_peel<0>(ctx, n, im, fs, fc, db, d_mult); break;
    }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(ctx->ev_redo[1], ctx->stream));
  if (int rc = values_to_host(ctx, order, ctx->d_nd_order, (size_t)ranked * sizeof(int32_t)))
    return rc;
  float seg = 0;
  HIPCHK(hipEventElapsedTime(&seg, ctx->ev_redo[0], ctx->ev_redo[1]));
  ctx->nd_ms = ms + seg;
  ctx->nd_fronts = nf;
  *n_fronts = nf;
  *n_ranked = ranked;
  return 0;
}

int gpe_last_nd_sort_ms(const gpe_ctx* ctx, float* ms) {
  if (!ctx || !ms) return GPE_E_INVALID;
  *ms = ctx->nd_ms;
  return 0;
}

int gpe_last_nd_sort_fronts(const gpe_ctx* ctx, int64_t* fronts) {
  if (!ctx || !fronts) return GPE_E_INVALID;
  *fronts = ctx->nd_fronts;
  return 0;
}
