// The body of f_eval_asm, f_eval_asm_values, f_eval_asm_moments,
// f_eval_asm_abserr and f_eval_asm_abserr_cases (asm_kernels.h includes this
// file inside each of the five kernel templates, after
// `constexpr int EPILOGUE`): one text, five kernels.  The fitness kernel is compiled from exactly the
// text it always had (its VALUES branch is discarded), so its registers do not
// depend on the values epilogue; each kernel holds its own copy of its core
// and has its own jump table (init_asm).
// F32 = false: the fp64 core (gen_asm.py); true: the fp32 core
// (gen_asm32.py, fp32 mode).  DEEP: the cores with asmcore_deep::D stack
// slots.  Same geometry, staging, epilogue and redo.
  [[maybe_unused]] constexpr bool VALUES = EPILOGUE == kEpiValues;
  [[maybe_unused]] constexpr bool MOMENTS = EPILOGUE == kEpiMoments;
  [[maybe_unused]] constexpr bool ABSERR =
      EPILOGUE == kEpiAbsErr || EPILOGUE == kEpiAbsErrCases;
  // a cases run's abs-error kernels: each valid case's |d| to case_out too
  [[maybe_unused]] constexpr bool ABSCASES = EPILOGUE == kEpiAbsErrCases;
  // accumulator pairs per program and lane (moments: f, f f, f y; abs error:
  // the sum of |d|, then (max |d|, hits))
  constexpr int ACCW = MOMENTS ? 3 : ABSERR ? 2 : 1;
  using R = typename std::conditional<F32, float, double>::type;
  // cases per lane of this kernel's core (the D = 5 fast core may hold more
  // than the deep and exact cores)
  constexpr int K = F32 ? asmcore32::K
                        : EXACT ? asmcore_exact::K : DEEP ? asmcore_deep::K : asmcore::K;
  // fp64: the sin/cos table (EXACT: glibc's __sincostab and constants)
  constexpr uint32_t kTab = F32 ? 0u : EXACT ? (uint32_t)asmcore_exact::GLIBC_LDS_BYTES
                                             : kTrigLdsBytes;
  static_assert(!EXACT || !F32, "the exact cores are fp64");
  static_assert(asmcore_exact_deep::K == asmcore_exact::K && asmcore_exact::GLIBC_LDS_BYTES ==
                    asmcore_exact_deep::GLIBC_LDS_BYTES, "one exact tile layout");
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  double* trig = lds;                                 // [64][4] (fp64)
  // the case tile [nv][K][64] + [nt][K][64]; with dbuf two of them
  const int tile_elems = (a.nv + a.nt) * K * 64;
  const uint32_t tile_bytes = (uint32_t)tile_elems * (uint32_t)sizeof(R);
  // dma_tile moves one global_load_lds_dwordx4 (16 B) per lane per column:
  // exactly a K = 2 fp64 column (1 KiB); any other core stages by hand
  constexpr bool kDmaColumn = !F32 && K * 64 * sizeof(double) == 1024;
  const bool dbuf = kDmaColumn && a.dbuf;
  R* const xs0 = (R*)((char*)lds + kTab);
  R* xs = xs0;
  const R* ts = xs + a.nv * K * 64;
  double* acc = (double*)(xs0 + tile_elems * (dbuf ? 2 : 1)) + wave * a.P * (128 * ACCW);
  uint32_t xa = kTab + (uint32_t)lane * (uint32_t)sizeof(R);
  const int nthreads = (int)blockDim.x, nwaves = nthreads >> 6;
  // the D = 5 fp64 core with its own program loop (GP_CORE_LOOPED): the LDS
  // byte addresses of this lane's target (ts) and program 0's accumulator
  constexpr bool LOOP = !F32 && !DEEP && (EXACT ? GP_ASM_LOOP_EXACT : GP_ASM_LOOP);
  uint32_t vts = kTab + (uint32_t)((a.nv * K * 64 + lane) * (int)sizeof(R));
  const uint32_t vacc =
      kTab + tile_bytes * (dbuf ? 2u : 1u) +
      (uint32_t)((wave * a.P * (128 * ACCW) + lane) * (int)sizeof(double));
  if (!F32)
    for (int i = threadIdx.x; i < (int)(kTab / 8); i += nthreads)
      trig[i] = a.cst[kCstTable + i];

  // Workgroups go to the 8 XCDs round-robin by linear id.  With the tile
  // groups a multiple of 8, linear id L runs on XCD L % 8: that XCD takes
  // its groups (xcd, xcd + 8, ...) one after the other, every wave-block of
  // one group before the next, so one group's case range (not all of the
  // XCD's) is live in its L2 at a time.
  uint32_t grp = blockIdx.x, wb = blockIdx.y;
  if ((gridDim.x & 7u) == 0) {
    const uint32_t L = blockIdx.x + gridDim.x * blockIdx.y;
    const uint32_t r = L >> 3;
    grp = (L & 7u) + 8u * (r / gridDim.y);
    wb = r % gridDim.y;
  }
  const int64_t wave_id = (int64_t)wb * nwaves + wave;
  const int64_t slot0 = wave_id * a.P;
  // lane j < P holds program j of this wave and its first code word: read
  // with v_readlane in the loop (no memory round trip per program-tile)
  int my_prog = -1;
  uint32_t my_start = 0;
  if (lane < a.P && slot0 + lane < a.n_slots) my_prog = a.slot_prog[slot0 + lane];
  if (my_prog >= 0) my_start = a.start[my_prog];
  int n_mine = 0;
  for (int j = 0; j < a.P; ++j)
    if (__builtin_amdgcn_readlane(my_prog, j) >= 0) n_mine = j + 1;
  for (int j = 0; j < a.P * ACCW; ++j) {
    acc[(2 * j) * 64 + lane] = 0.0;
    acc[(2 * j + 1) * 64 + lane] = 0.0;
  }
  const int64_t t0 = (int64_t)grp * a.tiles_per_group;
  const int64_t t1 = min(a.n_tiles, t0 + a.tiles_per_group);
  uint32_t done_mask = 0;      // fp64: this wave's programs already flagged
  // fp64 MSE with one target column and no per-case output: the lean
  // epilogue (below) on full tiles
  // (a moments or abs-error run: the core returns at END for every program)
  const bool lean = !MOMENTS && !ABSERR && !F32 && a.nt == 1 && a.case_out == nullptr;
  Task st{};
  st.X = a.X;
  st.nv = a.nv;
  st.terms = a.terms;
  st.nt = a.nt;
  st.n_cases = a.n_cases;
  // Tile staging.  dbuf (fp64, full tiles): while tile t runs from one
  // buffer, the block's waves copy tile t + 1 into the other by LDS-DMA
  // (one global_load_lds_dwordx4 per 1 KiB column: K x 64 doubles, the same
  // contiguous run of cases in X and in the tile); a wave waits for its own
  // copies and the block meets once, after the tile.  Otherwise (and for a
  // partial tile) the tile is staged between two barriers.  (Measured on C4:
  // the staging loads, waited for between two barriers, were 5.5 % of the
  // kernel and the barriers 2 %; a register-held prefetch spilled.)
  const uint32_t ncol = (uint32_t)(a.nv + a.nt);
  auto dma_tile = [&](int64_t t, uint32_t b) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
    for (uint32_t col = w; col < ncol; col += (uint32_t)nwaves) {
      const double* src = (col < (uint32_t)a.nv)
                              ? a.X + (int64_t)col * a.n_cases
                              : a.terms + (int64_t)(col - a.nv) * a.n_cases;
      src += t * (K * 64) + 2 * lane;
      const uint32_t dst = kTab + b * tile_bytes + col * (uint32_t)(K * 64 * sizeof(double));
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                   "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    }
  };
  auto tile_full = [&](int64_t t) { return (t + 1) * (K * 64) <= a.n_cases; };
  bool staged = false;         // dbuf: tile t arrived by DMA (and was waited for)
  // The exact core's resident tile loop (gen_asm.py Gen.tile_next): entered
  // on a full tile of a lean, double-buffered launch, the core runs the
  // wave's programs on every tile up to the group's last full one — the
  // wait, the barrier, the buffer change and the next tile's DMA of this
  // loop's body are its own — and comes back only for a program this code
  // finishes (at the tile it returns in TIO) or at the end of the stretch.
  constexpr bool kResident = LOOP && EXACT && GP_ASM_TILE_LOOP_EXACT;
  const bool resident = kResident && dbuf && lean && a.tile_loop && a.n_tiles < (1ll << 31);
  const int64_t t_full = min(t1, a.n_cases / (K * 64));   // the first tile not full
  // lane i: this wave's i-th DMA column (as dma_tile: w, w + nwaves, ...)
  uint32_t dma_lo = 0, dma_hi = 0, dma_dst = 0;
  if (resident) {
    const uint32_t col = (uint32_t)wave + (uint32_t)lane * (uint32_t)nwaves;
    if (col < ncol) {
      const double* src = (col < (uint32_t)a.nv)
                              ? a.X + (int64_t)col * a.n_cases
                              : a.terms + (int64_t)(col - a.nv) * a.n_cases;
      dma_lo = (uint32_t)(uint64_t)src;
      dma_hi = (uint32_t)((uint64_t)src >> 32);
      dma_dst = kTab + col * (uint32_t)(K * 64 * sizeof(double));
    }
  }
  // fp64 main core: lane j's program's redo flag as the whole grid sees it,
  // loaded one tile ahead — a program another tile group flagged (it is
  // re-run whole with glibc's sin/cos) is skipped here too from then on
  uint32_t gflag = 0;
  for (int64_t t = t0; t < t1; ++t) {
    if (a.diag & 16) {
      // experiment (GPE_DIAG=16): 40 more v_readlane per wave-tile, the
      // order of the lane ops the compiler's SGPR spills add to each tile
      // here — the spills' price
      uint32_t sink;
      asm volatile(".rept 40\n\tv_readlane_b32 %0, %1, 5\n\t.endr" : "=s"(sink) : "v"(lane));
    }
    if constexpr (!F32 && !EXACT) {
      done_mask |= (uint32_t)__builtin_amdgcn_ballot_w64(gflag != 0);
      gflag = my_prog >= 0 ? __hip_atomic_load(&a.redo[my_prog], __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT)
                           : 0u;
    }
    if (dbuf) {
      const uint32_t b = (uint32_t)((t - t0) & 1);
      xs = xs0 + b * tile_elems;
      ts = xs + a.nv * K * 64;
      xa = kTab + b * tile_bytes + (uint32_t)lane * (uint32_t)sizeof(R);
      vts = xa + (uint32_t)(a.nv * K * 64 * (int)sizeof(R));
      if (!staged) {
        __syncthreads();
        f_stage<K>(st, xs, t, nthreads);
        __syncthreads();
      }
      staged = t + 1 < t1 && tile_full(t + 1);
      if (staged) dma_tile(t + 1, b ^ 1u);
    } else if (!(a.diag & 2) || t == t0) {
      // (experiments: diag 4 drops the barriers after the first tile — racy
      // values, the barrier's cost — and diag 8 the loads)
      if (!(a.diag & 4) || t == t0) __syncthreads();
      if (!(a.diag & 8) || t == t0) f_stage<K>(st, xs, t, nthreads);
      if (!(a.diag & 4) || t == t0) __syncthreads();
    }
    int64_t case0 = t * (K * 64) + lane;
    const bool full = (t + 1) * (K * 64) <= a.n_cases;
    // what follows a program's core run: the redo flag, the MSE epilogue
    // (lean or classifying), first errors and flags of program j
    auto finish = [&](int j, int prog, R (&T)[K], uint32_t (&vcase)[F32 ? K : 1],
                      uint32_t vbits, bool redo_lane) {
      if (a.diag & 1) {                          // experiment: no epilogue
        if (T[0] == R(12345) && T[1] == R(54321)) acc[lane] = vcase[0];
        return;
      }
      // this (program, tile) is left out here and re-evaluated by the C++
      // pass (f_eval_pairs)
      if (__builtin_amdgcn_ballot_w64(redo_lane)) {
        if (lane == 0) {
          const uint32_t i = atomicAdd(a.redo_count, 1u);
          if ((F32 || EXACT) && i < a.redo_list_cap)
            a.redo_list[i] = ((uint64_t)(uint32_t)prog << 32) | (uint64_t)(uint32_t)t;
          atomicOr(&a.redo[prog], 1u);
        }
        // fp64: re-run whole, skip its tiles; the exact core: only this
        // (program, tile) goes to the C++ pass (both are glibc to the bit)
        if (!F32 && !EXACT) done_mask |= 1u << j;
        return;
      }
      if constexpr (VALUES) {
        // a values run (f_eval_asm_values): case_out gets each case's value
        // itself, the default nan at a ValueError case (the cores' VINF bit,
        // the fp32 argument key); no term, no square, no accumulator, no flags
        unsigned long long verr_at = ~0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int64_t c = case0 + k * 64;
          if (c < a.n_cases) {
            const bool verr = F32 ? vcase[F32 ? k : 0] == asmcore32::RED_INF
                                  : ((vbits >> k) & 1u) != 0;
            if (verr) verr_at = min(verr_at, ((unsigned long long)c << 2) | GPE_ERR_VALUE);
            a.case_out[(size_t)prog * a.n_cases + c] =
                verr ? __builtin_nan("") : (double)T[k];
          }
        }
        if (verr_at != ~0ull) atomicMin(&a.first_err[prog], verr_at);
        return;
      }
      if constexpr (MOMENTS) {
        // a moments run (f_eval_asm_moments): per valid case f, f f and f y
        // into the lane's three double-double accumulators of program j, a
        // product with its exact low part (the build's one fused operation:
        // -ffp-contract=off); a case with a non-finite f or |f| >= 2^500 adds
        // nothing and raises GPE_FLAG_MOMENT_RANGE; pad lanes add nothing
        double* const ac = acc + (size_t)(6 * j) * 64 + lane;
        double m[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) m[q] = ac[q * 64];
        unsigned long long verr_at = ~0ull;
        uint32_t flag = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int64_t c = case0 + k * 64;
          if (c < a.n_cases) {
            const double f = (double)T[k];
            if ((vbits >> k) & 1u)
              verr_at = min(verr_at, ((unsigned long long)c << 2) | GPE_ERR_VALUE);
            if (!(__builtin_fabs(f) < 0x1p500)) {
              flag = GPE_FLAG_MOMENT_RANGE;
            } else {
              const double y = (double)ts[k * 64 + lane];
              const double ff = f * f, fy = f * y;
              dd_add(m[0], m[1], f, 0.0);
              dd_add(m[2], m[3], ff, __builtin_fma(f, f, -ff));
              dd_add(m[4], m[5], fy, __builtin_fma(f, y, -fy));
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) ac[q * 64] = m[q];
        if (verr_at != ~0ull) atomicMin(&a.first_err[prog], verr_at);
        if (__builtin_amdgcn_ballot_w64(flag != 0)) {
          if (lane == 0) atomicOr(&a.flags[prog], GPE_FLAG_MOMENT_RANGE);
        }
        return;
      }
      if constexpr (ABSERR) {
        // an abs-error run (f_eval_asm_abserr): per valid case d, formed as the
        // general path below forms it, into the lane's four words of program j
        // (abserr::accumulate: sum |d|, max |d|, hits); pad lanes add nothing
        double* const ac = acc + (size_t)(4 * j) * 64 + lane;
        abserr::Part p{ac[0], ac[64], ac[128], ac[192]};
        unsigned long long verr_at = ~0ull;
        uint32_t flag = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int64_t c = case0 + k * 64;
          if (c < a.n_cases) {
            double dlt = (double)T[k];
            for (int q = 0; q < a.nt; ++q) dlt = dlt - (double)ts[(q * K + k) * 64 + lane];
            if ((vbits >> k) & 1u)
              verr_at = min(verr_at, ((unsigned long long)c << 2) | GPE_ERR_VALUE);
            abserr::accumulate(p, flag, dlt, a.hit_eps);
            // (f_eval_asm_abserr_cases: nan at a ValueError case, as a values
            // run stores it; pad lanes store nothing)
            if constexpr (ABSCASES)
              a.case_out[(size_t)prog * a.n_cases + c] =
                  abserr::case_error(dlt, ((vbits >> k) & 1u) != 0);
          }
        }
        ac[0] = p.hi;
        ac[64] = p.lo;
        ac[128] = p.mx;
        ac[192] = p.hits;
        if (verr_at != ~0ull) atomicMin(&a.first_err[prog], verr_at);
        if (__builtin_amdgcn_ballot_w64(flag != 0)) {
          for (int m = 32; m >= 1; m >>= 1) flag |= __shfl_xor(flag, m, 64);
          if (lane == 0) atomicOr(&a.flags[prog], flag);
        }
        return;
      }
      double hi = acc[(2 * j) * 64 + lane], lo = acc[(2 * j + 1) * 64 + lane];
      if (lean && full) {
        // the common case: one target column, every case of the tile valid,
        // no per-case output.  The same operations as the general path below
        // (whose TwoSum guard only acts on a non-finite sum); a wave with a
        // non-finite sum falls through to it and is classified there.
        double s = hi, l = lo;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const double dlt = (double)T[k] - (double)ts[k * 64 + lane];
          const double sq = dlt * dlt;
          const double ns = s + sq;
          const double bb = ns - s;
          l = l + ((s - (ns - bb)) + (sq - bb));
          s = ns;
        }
        if (!__builtin_amdgcn_ballot_w64(!__builtin_isfinite(s) || vbits != 0)) {
          acc[(2 * j) * 64 + lane] = s;
          acc[(2 * j + 1) * 64 + lane] = l;
          return;
        }
      }
      unsigned long long err = ~0ull;
      uint32_t flag = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int64_t c = case0 + k * 64;
        if (c < a.n_cases) {
          R dlt = T[k];
          for (int q = 0; q < a.nt; ++q) dlt = dlt - ts[(q * K + k) * 64 + lane];
          const double sq = (double)(R)(dlt * dlt);
          // sin/cos(inf) in this case (the fp32 core's argument key, the
          // fp64 fast cores' VINF bit): ValueError, even where
          // protectedDiv(nan, 0) hid the nan from the value
          const bool verr = F32 ? vcase[F32 ? k : 0] == asmcore32::RED_INF
                                : ((vbits >> k) & 1u) != 0;
          if (verr) err = min(err, ((unsigned long long)c << 2) | GPE_ERR_VALUE);
          if (!__builtin_isfinite(sq)) {             // rare: classify
            const bool fin = __builtin_isfinite(dlt);
            if (!fin) flag |= GPE_FLAG_NONFINITE_TERM;
            flag |= (sq != sq) ? GPE_FLAG_NAN_TERM : GPE_FLAG_INF_TERM;
            if (fin && !verr)
              err = min(err, ((unsigned long long)c << 2) | GPE_ERR_OVERFLOW);
          }
          double s, e;
          two_sum(hi, sq, s, e);
          hi = s;
          lo = lo + e;
          if (a.case_out) a.case_out[(size_t)prog * a.n_cases + c] = sq;
        }
      }
      acc[(2 * j) * 64 + lane] = hi;
      acc[(2 * j + 1) * 64 + lane] = lo;
      if (err != ~0ull) atomicMin(&a.first_err[prog], err);
      if (__builtin_amdgcn_ballot_w64(flag != 0)) {
        for (int m = 32; m >= 1; m >>= 1) flag |= __shfl_xor(flag, m, 64);
        if (lane == 0) atomicOr(&a.flags[prog], flag);
      }
    };
    if constexpr (LOOP) {
      // the core runs the wave's programs and their lean epilogues itself and
      // returns at the end, or at a program this code finishes (jx)
      const uint32_t lean_full = (uint32_t)__builtin_amdgcn_readfirstlane(lean && full ? 1 : 0);
      const uint32_t probe =
          (uint32_t)__builtin_amdgcn_readfirstlane(a.base_probe != nullptr ? 1 : 0);
      uint32_t* probe_out = a.base_probe;
      const double* cst = a.cst;
      const uint64_t code = (uint64_t)a.code;
      uint32_t jn = 0;
      // resident: the stretch [t, t_full); the core leaves in tile tio
      [[maybe_unused]] uint32_t tio = (uint32_t)t;
      [[maybe_unused]] const uint32_t tend = !kResident ? 0u :
          (uint32_t)__builtin_amdgcn_readfirstlane(resident && full ? (uint32_t)t_full : 0u);
      [[maybe_unused]] uint32_t bflip = ((t - t0) & 1) ? 0u - tile_bytes : tile_bytes;
#pragma nounroll
      for (;;) {
        uint32_t jx = jn;
        const uint32_t done = (uint32_t)__builtin_amdgcn_readfirstlane(done_mask);
        R T[K];
        uint32_t vred, vinf = 0;
        if constexpr (EXACT) {
          GP_CORE_EXACT_LOOPED(code, probe, probe_out, jx, (uint32_t)n_mine, done,
                               a.redo_hi, lean_full, my_start, xa, vts, vacc, tio, tend,
                               bflip, dma_lo, dma_hi, dma_dst);
          if constexpr (kResident) {
            if (tio != (uint32_t)t) {        // (a full tile of the stretch)
              t = (int64_t)tio;
              xs = xs0 + ((t - t0) & 1) * tile_elems;
              ts = xs + a.nv * K * 64;
              case0 = t * (K * 64) + lane;
            }
          }
        } else {
          GP_CORE_LOOPED(code, probe, probe_out, jx, (uint32_t)n_mine, done, a.redo_hi,
                         lean_full, my_start, vts, vacc);
        }
        if (probe || jx >= (uint32_t)n_mine) break;
        const int prog = __builtin_amdgcn_readlane(my_prog, jx);
        uint32_t vcase[1] = {vred};
        finish((int)jx, prog, T, vcase, vinf, vred >= a.redo_hi);
        jn = jx + 1;
      }
      // (the stretch's last tile has no successor staged; the core met the
      // block after every tile before it)
      if constexpr (kResident) {
        if (tend) staged = false;
      }
    } else {
#pragma nounroll
      for (int j = 0; j < n_mine; ++j) {
        if (done_mask & (1u << j)) continue;
        const int prog = __builtin_amdgcn_readlane(my_prog, j);
        const uint32_t w0 = __builtin_amdgcn_readlane(my_start, j);
        const uint64_t pc = (uint64_t)(a.code + w0);
        // base_probe (init_asm, a dummy one-tile task): this call site writes
        // its handler table and .Lbase instead of running a program — the one
        // copy of the core in this kernel, whose addresses the jump words hold
        const uint32_t probe =
            (uint32_t)__builtin_amdgcn_readfirstlane(a.base_probe != nullptr ? 1 : 0);
        uint32_t* probe_out = a.base_probe;
        R T[K];
        // fp64 core: one running max of |x|'s high word over the lane's
        // sin/cos arguments; fp32 core: one max of |x|'s bits per case
        uint32_t vcase[F32 ? K : 1];
        uint32_t vbits = 0;        // fp64 fast cores: bit k = sin/cos(+-inf)
        bool redo_lane;
        if constexpr (F32) {
          const float* cst = a.cst32;
          uint32_t* vred = vcase;
          if constexpr (DEEP) {
            GP_CORE32_DEEP(pc, probe, probe_out);
          } else {
            GP_CORE32(pc, probe, probe_out);
          }
          // a finite argument at or past 2^30: re-run; an infinite one (and
          // none such): the ValueError below (gen_asm32.py's argument key)
          redo_lane = false;
          for (int k = 0; k < K; ++k) redo_lane |= vcase[k] < asmcore32::RED_INF;
        } else {
          const double* cst = a.cst;
          uint32_t vred, vinf = 0;
          if constexpr (DEEP && EXACT) {
            GP_CORE_EXACT_DEEP(pc, probe, probe_out);
          } else if constexpr (DEEP) {
            GP_CORE_DEEP(pc, probe, probe_out);
          } else if constexpr (EXACT) {
            GP_CORE_EXACT(pc, probe, probe_out);
          } else {
            GP_CORE(pc, probe, probe_out);
          }
          vcase[0] = vred;
          vbits = vinf;
          // fast cores: a finite argument at or past the threshold (2^40, deep
          // programs 2^20): re-run with glibc's algorithm; an infinite one is
          // the ValueError below, a nan one nan either way.  The exact core:
          // |x| >= 105414350, inf, nan go to the C++ pair pass.
          redo_lane = vred >= a.redo_hi;
        }
        finish(j, prog, T, vcase, vbits, redo_lane);
      }
    }
    if (staged) {
      // this wave's copies of tile t + 1 have landed; after the barrier every
      // wave's have, and nobody reads tile t's buffer any more
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
  // one cross-lane reduction per program per tile group (moments: of each
  // of the three pairs, six words per slot; abs error: the sum's pair, then
  // the (max, hits) pair by max and add, four words per slot)
#pragma nounroll
  for (int j = 0; j < n_mine * ACCW; ++j) {
    double hi = acc[(2 * j) * 64 + lane], lo = acc[(2 * j + 1) * 64 + lane];
    for (int m = 32; m >= 1; m >>= 1) {
      const double ohi = shfl_xor_d(hi, m);
      const double olo = shfl_xor_d(lo, m);
      if (ABSERR && (j & 1)) {
        if (ohi > hi) hi = ohi;
        lo += olo;
      } else {
        dd_add(hi, lo, ohi, olo);
      }
    }
    if (lane == 0) {
      double* p = a.part + ((size_t)grp * a.n_slots * ACCW + slot0 * ACCW + j) * 2;
      p[0] = hi;
      p[1] = lo;
    }
  }
