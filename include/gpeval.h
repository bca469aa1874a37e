/*
 * gpeval.h — C ABI of the MI355X GP population evaluator (libgpeval.so).
 *
 * Drop-in boundary.  The reference evaluates a population with
 *     fitnesses = toolbox.map(toolbox.evaluate, invalid_ind)
 * (deap/algorithms.py:150,172), where every evaluate call runs
 * gp.compile (deap/gp.py:462-487) and a Python per-case loop
 * (examples/gp/symbreg.py:55-61, multiplexer.py:73-75, parity.py:66-68,
 * spambase.py:80-87).  deap_amd.evaluator replaces that map call by ONE
 * batched call into this library; the ctypes binding is
 * deap_amd/_lib.py.  Nothing here uses torch types: plain pointers/sizes.
 *
 * Conventions: functions return 0 on success or a negative GPE_E* code;
 * gpe_last_error() describes the last failure.  Host buffers are only read
 * during the call.  A context is bound to one device and is not thread-safe.
 * All entry points block until their work is complete.
 */
#ifndef GPEVAL_H
#define GPEVAL_H

#include <stddef.h>
#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpe_ctx gpe_ctx;

/* machines (kernel families) */
#define GPE_MACHINE_F 0   /* fp64 accumulator machine: symreg, STGP */
#define GPE_MACHINE_B 1   /* bit-sliced boolean machine: mux, parity */

/* fitness modes */
#define GPE_MODE_MSE 0    /* sum over cases of (T - t0 - t1 - ...)^2, as a
                             double-double (hi, lo) pair; errors tracked   */
#define GPE_MODE_HITS_BOOL 1 /* F: count((T != 0) == (label != 0))        */
#define GPE_MODE_HITS_BITS 2 /* B: count(T == out) over bit-planes         */
#define GPE_MODE_SSE_NUMPY 3 /* F: sum over cases of (T - t0 - ...)^2 in
                                numpy.sum's exact order (pairwise over 8192-
                                element chunks); result in hi, lo = 0      */
#define GPE_MODE_SSE_SEQ 4   /* F: the same terms summed left to right from
                                0 (Python's builtin sum); hi, lo = 0       */

/* F-machine arithmetic (gpe_set_precision) */
#define GPE_PREC_F64 0    /* fp64 throughout: the reference's float        */
#define GPE_PREC_F32 1    /* fp32 cases/tree/d*d, fp64 double-double sum  */

/* error/flag encodings written by gpe_run */
#define GPE_NO_ERROR 0xFFFFFFFFFFFFFFFFull /* else (case << 2) | type       */
#define GPE_ERR_VALUE 1                    /* math.sin/cos(+-inf)          */
#define GPE_ERR_OVERFLOW 2                 /* (d)**2 overflow of finite d;
                                              exact pass: float(int) or
                                              int / int past 2**1024      */
#define GPE_ERR_XINT_RANGE 3               /* exact pass: an int past its
                                              1088-bit magnitude          */
#define GPE_XINT_WORDS 34                  /* uint32 words of an exact-pass
                                              int constant                */
#define GPE_FLAG_NONFINITE_TERM 1u         /* some d was inf or nan        */
#define GPE_FLAG_NAN_TERM 2u               /* some d*d was nan             */
#define GPE_FLAG_INF_TERM 4u               /* some d*d was +inf            */
#define GPE_FLAG_MOMENT_RANGE 8u           /* moments run: some value was
                                              inf, nan or >= 2^500 in size */

#define GPE_E_INVALID -1
#define GPE_E_HIP -2
#define GPE_E_STATE -3
#define GPE_E_DEPTH -4
#define GPE_E_COMM -5       /* a collective did not complete within GPE_COMM_TIMEOUT_S */
#define GPE_E_ARG -6        /* the context's cases / precision do not fit the call */

/* Replaces: the per-process setup of the reference's evaluation
 * (nothing to bind on CPU; the device context owns streams/buffers). */
int gpe_create(int device, gpe_ctx** out);
void gpe_destroy(gpe_ctx* ctx);
const char* gpe_last_error(const gpe_ctx* ctx);
int gpe_device_info(const gpe_ctx* ctx, int* n_cu, int* clock_khz,
                    char* name, size_t name_len);

/* Upload the fitness cases once; they stay resident in HBM.
 * Replaces the case lists the reference's evaluate closes over
 * (symbreg.py:63 points, multiplexer.py:37-54 / parity.py:31-47 tables,
 * spambase.py:33-35 rows).
 *   F: X = double[n_vars][n_cases] (variable-planar), terms =
 *      double[n_terms][n_cases] (targets subtracted in order, or labels)
 *   B: X = uint32[n_vars][ceil(n_cases/32)] bit-planes (case c is bit c%32
 *      of word c/32), terms = uint32[ceil(n_cases/32)] output plane. */
int gpe_set_cases(gpe_ctx* ctx, int machine, const void* X, int n_vars,
                  int64_t n_cases, const void* terms, int n_terms);

/* Case subsampling: run on rows idx[0..m) of the cases gpe_set_cases uploaded
 * (down-sampled lexicase, mini-batch fitness, bootstrap resampling) without a
 * new upload.  idx: values in [0, n_full), any order, duplicates allowed, m
 * >= 1 may exceed n_full; idx NULL: the full set again.  The rows are
 * gathered on the device into a second pair of case buffers (grown on need,
 * reused) and every following run, values run, gpe_lexicase(NULL) and
 * gpe_tournament(NULL) behaves as after a gpe_set_cases of those rows: case
 * numbers in first-error words are positions in idx, the MSE divisor is m.
 * The loaded programs, their exact pass and the lowering tables are kept;
 * the resident fitness and the per-case matrix are dropped until the next
 * run.  The column bounds the range pass reads stay the full set's (a hull of
 * a superset proves every class picked from it, so the handler picked for a
 * sin/cos may differ from a fresh context's, the bits may not).  idx is
 * checked on the host before any launch: an entry out of range returns
 * GPE_E_INVALID with a message naming the first one, and m <= 0 with idx !=
 * NULL returns GPE_E_INVALID; either leaves the active set as it was.
 * gpe_set_cases and gpe_set_trig_leaves drop an active subset. */
int gpe_select_cases(gpe_ctx* ctx, const int64_t* idx, int64_t m);
/* The active subset's size (m = -1: none active) and the full set's. */
int gpe_case_subset(const gpe_ctx* ctx, int64_t* m, int64_t* n_full);

/* Population-level evaluation of sin/cos leaves (F machine).  With
 * enable != 0 the context adds 2*n_vars columns, sin(x_v) then cos(x_v),
 * computed on the device at the start of every gpe_run with the same
 * near-correctly-rounded sin/cos as the interpreter; programs may then read
 * column n_vars + v for sin(ARGv) and 2*n_vars + v for cos(ARGv) (the
 * flattener's trig_leaves option).  Same values, one evaluation per case
 * instead of one per (program, case).  Must follow gpe_set_cases; discards
 * loaded programs. */
int gpe_set_trig_leaves(gpe_ctx* ctx, int enable);

/* Arithmetic of the F machine for the following runs (default GPE_PREC_F64).
 * GPE_PREC_F32 evaluates cases, constants, every node and (T - t)^2 in fp32
 * (device sinf/cosf), accumulating the squares in fp64 double-double: an
 * approximate throughput mode, not reference-exact (tolerance: DESIGN.md). */
int gpe_set_precision(gpe_ctx* ctx, int prec);

/* Upload one generation of flattened programs (deap_amd/flatten.py):
 * code = uint32 words, off[n_prog+1] word offsets, depth[n_prog] operand-
 * stack slots each program needs.  Replaces the n_prog gp.compile calls. */
int gpe_load_programs(gpe_ctx* ctx, const uint32_t* code, int64_t n_words,
                      const int64_t* off, int64_t n_prog,
                      const int32_t* depth);

/* Evaluate the loaded programs on the resident cases.  Outputs are HOST
 * arrays of n_prog entries (any may be NULL):
 *   out_hi/out_lo: MSE mode — double-double sum of squared errors;
 *                  hits modes — hit count in out_hi, 0 in out_lo
 *   out_err:       first erroring case per program (GPE_NO_ERROR if none)
 *   out_flags:     GPE_FLAG_* bits
 * Replaces: toolbox.map(toolbox.evaluate, invalid_ind) (algorithms.py:172)
 * minus the final division by len(points) and tuple packing. */
int gpe_run(gpe_ctx* ctx, int mode, double* out_hi, double* out_lo,
            uint64_t* out_err, uint32_t* out_flags);

/* Same, but writing DEVICE arrays (e.g. torch tensors) so that the caller
 * can all-reduce partial sums over RCCL before copying to the host. */
int gpe_run_device(gpe_ctx* ctx, int mode, void* d_hi, void* d_lo,
                   void* d_err, void* d_flags);

/* gpe_run plus the per-case terms behind the reduction, for selection
 * schemes that need them (lexicase: reference deap/tools/selection.py:
 * 214-320 reads one fitness value per case).  out_cases is a HOST array
 * double[n_prog][n_cases]: MSE mode — (T - t0 - ...)^2 per case, exactly the
 * values the SSE sums; HITS_BOOL — 1.0 for a hit, 0.0 otherwise.  F machine
 * only; the other outputs are those of gpe_run. */
int gpe_run_cases(gpe_ctx* ctx, int mode, double* out_cases, double* out_hi,
                  double* out_lo, uint64_t* out_err, uint32_t* out_flags);

/* A values run: what each loaded program COMPUTES on each resident case,
 * not a fitness.  out_values is a HOST array double[n_prog][n_cases]: the
 * program's result as numpy converts it to float64 (a bool 1.0 / 0.0, an int
 * float(int) correctly rounded; fp32 mode: the fp32 value widened).  No
 * target column is read (the cases may have n_terms = 0), nothing is squared
 * or summed, and GPE_ERR_OVERFLOW only means float(int) past the float
 * range.  out_err (may be NULL): the first erroring case per program as
 * gpe_run gives it (GPE_NO_ERROR if none); an erroring case of the fp64 /
 * fp32 cores holds the default nan (exact-int programs: at least the first
 * one).  F machine only.  The resident fitness that gpe_tournament(NULL) and
 * gpe_lexicase(NULL) read is not disturbed.
 * Replaces: [[gp.compile(t, pset)(*row) for row in rows] for t in pop], the
 * per-case Python loop behind held-out scoring, plots and residuals. */
int gpe_run_values(gpe_ctx* ctx, double* out_values, uint64_t* out_err);

/* Same, the kernels writing straight into the caller's DEVICE buffers (e.g.
 * torch tensors): d_values double[n_prog][n_cases], d_err uint64[n_prog] (may
 * be NULL).
 * Replaces: the same loop, without the host round trip. */
int gpe_run_values_device(gpe_ctx* ctx, void* d_values, void* d_err);

/* The B machine's values run: out_planes is a HOST array
 * uint32[n_prog][ceil(n_cases / 32)], bit c % 32 of word c / 32 the program's
 * output on case c; the bits past n_cases in the last word are 0.
 * Replaces: [[bool(func(*row)) for row in inputs] for func in compiled]
 * (multiplexer.py / parity.py evaluate, before the comparison with the
 * outputs). */
int gpe_run_values_bits(gpe_ctx* ctx, uint32_t* out_planes);

/* A moments run: each loaded program's Sf = sum f, Sff = sum f^2 and
 * Sfy = sum f y over the resident cases, f the program's value (as
 * gpe_run_values gives it) and y the cases' one target column.  out6 is a
 * HOST array double[n_prog][6] = (Sf hi, lo, Sff hi, lo, Sfy hi, lo), each sum
 * a double-double, summed in a fixed order (the same bits from run to run).
 * first_err / flags (may be NULL): the first erroring case per program as
 * gpe_run_values gives it, and GPE_FLAG_MOMENT_RANGE for a program with a
 * non-finite value or one of magnitude 2^500 or more (such cases are left out
 * of its sums).  Programs the exact cores hold (at most 12 stack slots and 32
 * variables, no exact-int pass) run on those cores' moments kernels, which
 * keep the three sums in LDS; a program with an inf / nan / huge sin/cos
 * argument in some tile, and every other program, takes the rows route: a
 * values run into a device scratch of bounded size (16 GiB at most;
 * GPE_MOMENTS_MB in the environment at gpe_create) reduced there
 * (moments_rows), in chunks of programs whose rows fit it, one program at
 * least, so any number of programs and cases is taken.  fp64 on the F machine with exactly one target column,
 * else GPE_E_ARG.  The resident fitness is not disturbed.
 * Replaces: three numpy sums over gpe_run_values' n_prog * n_cases matrix. */
int gpe_run_moments(gpe_ctx* ctx, double* out6, uint64_t* first_err, uint32_t* flags);

/* Linear-scaling fitness (Keijzer 2003) of the loaded programs: the mean
 * squared error of the best affine fit a + b f to the target, from one
 * moments run.  sy, syy: the target's sum y and sum y^2 as (hi, lo), computed
 * exactly by the caller.  With vf = Sff - Sf^2 / n, vy = Syy - Sy^2 / n,
 * cfy = Sfy - Sf Sy / n:  b = cfy / vf, a = (Sy - b Sf) / n,
 * mse = (vy - cfy^2 / vf) / n, evaluated in double-double.  Two rules: a
 * program under GPE_FLAG_MOMENT_RANGE has mse = inf, b = 0, a = Sy / n; one
 * with n vf <= 2^-40 Sff counts as constant: b = 0, a = Sy / n, mse = vy / n.
 * HOST arrays of n_prog entries (first_err, flags may be NULL).  Arguments as
 * gpe_run_moments.
 * Replaces: predict() and a per-individual numpy regression. */
int gpe_run_scaled(gpe_ctx* ctx, const double sy[2], const double syy[2], double* mse,
                   double* a, double* b, uint64_t* first_err, uint32_t* flags);

/* Same, writing DEVICE arrays (d_err, d_flags may be NULL). */
int gpe_run_scaled_device(gpe_ctx* ctx, const double sy[2], const double syy[2],
                          void* d_mse, void* d_a, void* d_b, void* d_err, void* d_flags);

/* Host twin of the formula gpe_run_scaled applies on the device (one
 * function compiled for both): m6 double[n][6], flags uint32[n] (may be
 * NULL: no flag), outputs double[n]. */
int gpe_host_scaled_from_moments(const double* m6, int64_t n, int64_t n_cases,
                                 const double sy[2], const double syy[2],
                                 const uint32_t* flags, double* mse, double* a, double* b);

/* An abs-error run: each loaded program's absolute-error figures over the
 * resident cases.  With e = |f - t0 - t1 - ...| per case (f the program's
 * value, the term columns subtracted left to right as the MSE modes do),
 * out4 is a HOST array double[n_prog][4] = (sum e hi, lo, max e, hits): the
 * sum a double-double summed in a fixed order (the same bits from run to run),
 * the max ignoring nan, and hits the number of cases with e <= hit_eps (a
 * whole number held as a double; a nan or inf e is never a hit, also with
 * hit_eps = inf).  flags (may be NULL): GPE_FLAG_NAN_TERM for a program with a
 * nan e (its max and mean are nan by definition; the caller applies that) and
 * GPE_FLAG_INF_TERM for one with an inf e, each with GPE_FLAG_NONFINITE_TERM.
 * A sum that is inf with no flag set overflowed from finite terms.  first_err
 * (may be NULL): the first erroring case per program as gpe_run_values gives
 * it.  Routes as gpe_run_moments: the exact cores' abs-error kernels keep the
 * four words in LDS; every other program, and one with a redo tile, takes the
 * rows route (chunked values runs reduced by abserr_rows; GPE_MOMENTS_MB).
 * fp64 on the F machine and hit_eps >= 0, else GPE_E_ARG.  The resident
 * fitness is not disturbed.
 * Replaces: numpy.abs over gpe_run_values' n_prog * n_cases matrix. */
int gpe_run_abserr(gpe_ctx* ctx, double hit_eps, double* out4, uint64_t* first_err,
                   uint32_t* flags);

/* Same, writing DEVICE arrays (d_err, d_flags may be NULL). */
int gpe_run_abserr_device(gpe_ctx* ctx, double hit_eps, void* d_out4, void* d_err,
                          void* d_flags);

/* A cases run: gpe_run_abserr that also writes every program's per-case
 * absolute error e_c = |f(*row_c) - t0_c - t1_c - ...| (the terms subtracted
 * left to right: the e the sums above are made of) into the context's
 * per-case matrix double[n_prog][n_cases], the one gpe_run_cases fills with
 * squared errors.  out4, first_err and flags are gpe_run_abserr's, from the
 * same pass, bit for bit.  out_cases: the HOST copy double[n_prog][n_cases]
 * (through pinned staging), or NULL to leave the matrix on the device only,
 * where gpe_lexicase(ctx, NULL, ...) selects on it.  An erroring case of the
 * exact cores holds nan; a program of the rows route holds nan at least at
 * its first erroring case.  Every row is written whole by one route (a
 * program the abs-error kernels leave for a redo is rewritten by the rows
 * route).  Refusals and codes as gpe_run_abserr.
 * Residency: a cases run replaces the per-case matrix, as gpe_run_cases does;
 * a plain gpe_run_abserr, a moments run and a values run leave it untouched;
 * the resident fitness (gpe_tournament(NULL)) is untouched by both abs-error
 * runs.  Launch plans, P and LDS are gpe_run_abserr's (GPE_LAUNCH_ABSERR,
 * GPE_LAUNCH_ABSERR_DEEP).
 * Replaces: predict, abs(... - y) on the host and a second pass for the
 * summaries, before epsilon-lexicase on absolute errors. */
int gpe_run_abserr_cases(gpe_ctx* ctx, double hit_eps, double* out_cases, double* out4,
                         uint64_t* first_err, uint32_t* flags);

/* Host twin of a cases run's per-case value (no GPU): out_cases[n_cases] of
 * one row f[n_cases] against terms[n_terms][n_cases], the same per-case
 * function in a plain loop. */
int gpe_host_abserr_cases(const double* f, const double* terms, int64_t n_terms,
                          int64_t n_cases, double* out_cases);

/* Host twin of the rows route's reduction (no GPU): the four words and the
 * flags of one row f[n_cases] of per-case values against
 * terms[n_terms][n_cases], in abserr_rows' order (256 strided partials, the
 * same fixed tree, the same per-case function). */
int gpe_host_abserr(const double* f, const double* terms, int64_t n_terms, int64_t n_cases,
                    double hit_eps, double* out4, uint32_t* flags);

/* Device lexicase selection that replays the reference's random stream:
 * selLexicase (mode 0), selEpsilonLexicase (mode 1, epsilon) and
 * selAutomaticEpsilonLexicase (mode 2; n <= 16384) of deap/tools/
 * selection.py:214-320.  values is a HOST double[n][n_cases]
 * (fitness.values per individual), or NULL to select on the per-case
 * matrix of the last gpe_run_cases or gpe_run_abserr_cases (n = programs)
 * without a host round trip.  maximise[n_cases]: 1 where the case's weight is positive.
 * mt_state[625] (in/out): CPython's MT19937 state as random.getstate()[1]
 * gives it (624 words, then the position); the kernel makes the
 * reference's draws — random.shuffle(cases), then random.choice(candidates),
 * per selection — and writes back the state after them (random.setstate).
 * Writes the k selected indices.  *failed = -1, or the index of the
 * selection that ended with no candidate (where the reference raises
 * IndexError from random.choice([])); out and mt_state then stop there. */
int gpe_lexicase(gpe_ctx* ctx, const double* values, int64_t n,
                 int64_t n_cases, const uint8_t* maximise, int mode,
                 double epsilon, uint32_t* mt_state, int64_t k, int32_t* out,
                 int64_t* failed);

/* A hit-planes run (B machine): gpe_run in GPE_MODE_HITS_BITS in every
 * respect — the same hit counts bit for bit in out_hi, the same resident
 * fitness for gpe_tournament(NULL), the same launch plans — whose kernels, in
 * the same pass, also store each program's hit plane ~(T ^ out) & vmask into a
 * context-owned device matrix uint32[n_prog][ceil(n_cases / 32)]: bit c % 32
 * of word c / 32 is 1 where the program's output equals the case's, the bits
 * past n_cases are 0.  out_planes: the HOST copy uint32[n_prog][n_units]
 * (through pinned staging), or NULL to leave the matrix on the device only,
 * where gpe_lexicase_bits(ctx, NULL, ...) selects on it.  out_hi, out_err,
 * out_flags (any may be NULL): gpe_run's.  The F machine gets GPE_E_ARG.
 * Residency: a hit-planes run replaces the bit matrix; gpe_select_cases and
 * gpe_set_cases drop it; gpe_run, gpe_run_values_bits and loading programs
 * leave it as it is (gpe_lexicase_bits(NULL) refuses while the loaded program
 * count differs from the matrix's).
 * Replaces: tuple(int(func(*in_) == out) for in_, out in zip(inputs,
 * outputs)) per individual (multiplexer.py:75 / parity.py:68 before the sum),
 * the per-case fitness lexicase selection reads. */
int gpe_run_hit_planes(gpe_ctx* ctx, uint32_t* out_planes, double* out_hi,
                       uint64_t* out_err, uint32_t* out_flags);

/* A typed hit-planes run (F machine, fp64, exactly one target column: the
 * labels): gpe_run in GPE_MODE_HITS_BOOL in every respect — the same counts in
 * out_hi, the same errors and flags, the same resident fitness for
 * gpe_tournament(NULL) — whose routes, in the same pass, also store the matches
 * they count into the context's hit-plane matrix
 * uint32[n_prog][ceil(n_cases / 32)] (gpe_run_hit_planes' layout: bit c % 32
 * of word c / 32 is 1 where bool(program(case c)) is bool(label c); bits past
 * n_cases are 0; popcount(row) == out_hi).  The routes: the typed asm core's
 * hit-planes variant (END's match masks, 128 cases a tile: lane l of chain k
 * is case 128 t + 64 k + l, words 4 t + 2 k + {0, 1}), the C++ interpreter
 * kernels for programs past the core's five stack slots (the count's
 * ballots), a fill for one-constant programs (the label plane or its
 * complement), and the exact-integer pass (its 0/1 terms).  out_planes: the
 * HOST copy, or NULL to leave the matrix on the device, where
 * gpe_lexicase_bits(NULL), gpe_lexicase_bits_par(NULL),
 * gpe_informed_cases(NULL) and gpe_read_hit_planes take it.  GPE_E_ARG with a
 * message on the B machine, in fp32, or with another number of target columns.
 * Residency: gpe_select_cases, gpe_set_cases, a precision change and a
 * per-case run (gpe_run_cases, gpe_run_abserr_cases) drop the planes; loading
 * programs leaves them (the NULL routes refuse while the program count
 * differs).  gpe_informed_cases(NULL) on the F machine reads whichever the
 * most recent per-case run of the loaded programs left: these planes (eps is
 * ignored, as on the B machine) or the double matrix (thresholded by eps).
 * Replaces: bool(func(*row)) is bool(label) per row before the sum
 * (spambase.py:70), the per-case fitness lexicase selection reads. */
int gpe_run_typed_hit_planes(gpe_ctx* ctx, uint32_t* out_planes, double* out_hi,
                             uint64_t* out_err, uint32_t* out_flags);

/* Host twin of a typed hit-planes run's word arithmetic (no GPU): out[n]
 * [ceil(n_cases / 32)] from program outputs values[n][n_cases] and
 * labels[n_cases]: bit c is (values[i][c] != 0) == (labels[c] != 0) (a nan
 * output is true, as bool(nan)); pad bits 0. */
int gpe_host_typed_hit_planes(const double* values, const double* labels, int64_t n,
                              int64_t n_cases, uint32_t* out);

/* The resident bit matrix of the last gpe_run_hit_planes /
 * gpe_run_typed_hit_planes into the HOST array
 * out_planes uint32[n_prog][n_units]; GPE_E_STATE when none is resident. */
int gpe_read_hit_planes(gpe_ctx* ctx, uint32_t* out_planes);

/* Host twin of the plane arithmetic (no GPU): out[n][n_units] =
 * ~(result_planes[n][n_units] ^ out_plane[n_units]) with the bits past
 * n_cases of the last word cleared. */
int gpe_host_hit_planes(const uint32_t* result_planes, const uint32_t* out_plane,
                        int64_t n, int64_t n_cases, uint32_t* out);

/* Device lexicase selection on 0/1 per-case values, every case maximised,
 * replaying the reference's random stream as gpe_lexicase does.  On such
 * values selLexicase, selEpsilonLexicase with 0 <= epsilon < 1 and
 * selAutomaticEpsilonLexicase (deap/tools/selection.py:214-320) make the same
 * draws and pick the same individuals (a 0/1 sample's median absolute
 * deviation is 0 or 0.5), so there is no mode.  planes is a HOST program-major
 * hit matrix uint32[n][ceil(n_cases / 32)] (pad bits 0), or NULL to select on
 * the matrix of the last gpe_run_hit_planes (n = programs) without a host
 * round trip.  The matrix is transposed on the device into case-major 64-bit
 * planes (once per hit-planes run); a case keeps cand & plane[c] when that is
 * not empty, else every candidate.  Candidate words and the case permutation
 * live in LDS while ceil(n / 32) + n_cases words fit 48 KiB, else in device
 * scratch: no population or case limit beyond memory.  mt_state, out and
 * failed are gpe_lexicase's; *failed can only be set for n = 0. */
int gpe_lexicase_bits(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                      int64_t n_cases, uint32_t* mt_state, int64_t k,
                      int32_t* out, int64_t* failed);

/* Informed down-sampling (Boldi et al. 2023): a farthest-first subset of m
 * cases from a 0/1 per-case matrix hit[n][n_cases].  The distance of two cases
 * is the Hamming distance of their columns.  key[c] is the (c + 1)-th output
 * of SplitMix64 seeded with `seed`:
 *   z = seed + (c + 1) * 0x9E3779B97F4A7C15;
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ z >> 27) * 0x94D049BB133111EB;   key = z ^ z >> 31   (mod 2^64)
 * and the cases are totally ordered by (key[c], c).  out_idx[0] is the
 * smallest case in that order and out_dist[0] = -1; mind[c] is the distance
 * of case c to out_idx[0].  Pick t = 1 .. m - 1 is the unchosen case with the
 * largest mind, ties to the smallest (key, c); out_dist[t] is its mind, and
 * mind[c] = min(mind[c], distance(c, out_idx[t])) afterwards.  out_idx
 * int64[m] has no duplicates; out_dist int32[m] is non-increasing from index
 * 1 on.  Once every remaining mind is 0 the rest arrive in key order.
 * planes is a HOST program-major hit matrix uint32[n][ceil(n_cases / 32)] (pad
 * bits 0), as gpe_lexicase_bits takes it (eps is ignored), or NULL for the
 * resident matrix of the loaded programs (n, n_cases are then the context's):
 * on the B machine the hit planes of the last gpe_run_hit_planes; on the F
 * machine the per-case matrix of the last gpe_run_abserr_cases /
 * gpe_run_cases, where case c is a hit of program i when its value e is finite
 * and e <= eps (a nan or inf is never a hit, also with eps = inf: the rule of
 * gpe_run_abserr's hit count; eps >= 0 and not nan, else GPE_E_ARG).
 * GPE_E_STATE when no such matrix of the active case set is resident (after
 * gpe_select_cases, before a per-case run, or while the loaded program count
 * differs from that run's).  GPE_E_INVALID with a message
 * naming the value for m < 1, m > n_cases, n < 1 or n > INT32_MAX.  One launch
 * per pick, no grid-wide barrier.  The call selects nothing: the resident
 * fitness, the per-case matrix, the hit planes (the thresholded planes have
 * buffers of their own) and the active case set are not disturbed. */
int gpe_informed_cases(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                       int64_t n_cases, double eps, uint64_t seed, int64_t m,
                       int64_t* out_idx, int32_t* out_dist);

/* Host twin of gpe_informed_cases on a host matrix (no GPU): the same
 * arithmetic in plain C++. */
int gpe_host_informed_cases(const uint32_t* planes, int64_t n, int64_t n_cases,
                            uint64_t seed, int64_t m, int64_t* out_idx,
                            int32_t* out_dist);

/* Host twin of the F machine's thresholding (no GPU): cases double[n][n_cases]
 * into hit planes out_planes uint32[n][ceil(n_cases / 32)], bit c % 32 of word
 * c / 32 set where the value is finite and <= eps, pad bits 0. */
int gpe_host_hit_threshold(const double* cases, int64_t n, int64_t n_cases,
                           double eps, uint32_t* out_planes);

/* Parallel lexicase selection: k selections that do not share a random
 * stream, one workgroup each.  gpe_lexicase / gpe_lexicase_bits replay
 * CPython's MT19937 stream, where selection s + 1 starts at a position that
 * depends on randbelow(count_s), the filter's result, so their selections run
 * one after another.  Here the caller makes one draw, a 64-bit seed, and every
 * selection's case order and final choice follow from it by this rule (the
 * picks are reproducible from the seed; they are not DEAP's picks for the
 * same random.seed).
 *
 * Keys.  K(i) is the (i + 1)-th output of SplitMix64 seeded with `seed`:
 *   z = seed + (i + 1) * 0x9E3779B97F4A7C15;
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ z >> 27) * 0x94D049BB133111EB;   K = z ^ z >> 31   (mod 2^64)
 * (gpe_informed_cases' key).  K(0) = 0xE220A8397B1DCDAF for seed = 0,
 * K(1) = 0x6E789E6AA1B965F4.
 *
 * For selection s in [0, k) over n individuals and C cases, with
 * i0 = s * (C + 1) as a uint64:
 * 1. Case order.  The cases are sorted ascending by (K(i0 + c), c).  The keys
 *    compare as unsigned integers.
 * 2. Filter.  This is the reference's loop (deap/tools/selection.py:214-320),
 *    with the arithmetic gpe_lexicase uses.  It starts with all n candidates.
 *    It continues while cases remain and more than one candidate is left.  A
 *    case's best value is Python's max / min over the candidates in index
 *    order, so a leading nan stays.  Mode 0 ("plain") keeps v == best.  Mode 1
 *    ("epsilon") keeps v <= best + eps (>= best - eps where the case is
 *    maximised).  Mode 2 ("automatic") uses numpy.median twice.  The median is
 *    nan if any value is nan.  For an even count it is (a + b) / 2 of the two
 *    middle values.  The MAD is the median of |v - med|, and takes eps' place.
 *    All of it is fp64.
 * 3. Choice.  With `count` survivors in ascending index order,
 *    r = (K(i0 + C) * count) >> 64.  This is the high half of the 64 x 64
 *    product.  The pick is the r-th survivor.  If count == 0, which happens
 *    when a nan is the best value, then out[s] = -1 and the selection fails.
 *    *failed is the smallest failing s, or -1 if none fails.
 *
 * values is a HOST double[n][n_cases], or NULL for the per-case matrix of the
 * last gpe_run_cases / gpe_run_abserr_cases (n, n_cases are then the
 * context's; GPE_E_STATE as gpe_lexicase).  maximise[n_cases] and mode /
 * epsilon are gpe_lexicase's.  out is int32[k], filled for every selection.
 * There is no limit on n or n_cases beyond memory: the matrix is read
 * case-major (a transposed copy double[n_cases][n], cached until the next
 * per-case run or gpe_select_cases), the first case of every selection is
 * filtered once per distinct opening case, medians are an exact radix select
 * on the doubles' order-preserving 64-bit image, and candidate words and
 * compacted values live in LDS while they fit (gpe_lexicase_par_lds_values
 * values) and in per-block device scratch otherwise.  The grid is
 * min(k, 8 x CUs) persistent blocks; blocks never wait for each other.
 * n <= 0, n > INT32_MAX, n_cases outside 1 .. 2^31 - 1, k < 0 or a mode
 * outside 0..2: GPE_E_INVALID with a message.  k == 0 does nothing.  The call
 * disturbs nothing else: the resident fitness, the per-case matrix, the hit
 * planes and the active case set stay as they were. */
int gpe_lexicase_par(gpe_ctx* ctx, const double* values, int64_t n,
                     int64_t n_cases, const uint8_t* maximise, int mode,
                     double epsilon, uint64_t seed, int64_t k, int32_t* out,
                     int64_t* failed);

/* The same rule on 0/1 hits with every case maximised, where the three modes
 * (epsilon in [0, 1)) keep the same survivors (see gpe_lexicase_bits), so
 * there is no mode: a case keeps cand & plane[c] when that is not empty, else
 * every candidate.  planes is gpe_lexicase_bits' HOST matrix
 * uint32[n][ceil(n_cases / 32)], or NULL for the matrix of the last
 * gpe_run_hit_planes (GPE_E_STATE as there).  seed, k, out, failed and the
 * argument errors are gpe_lexicase_par's. */
int gpe_lexicase_bits_par(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                          int64_t n_cases, uint64_t seed, int64_t k,
                          int32_t* out, int64_t* failed);

/* Host twin of gpe_lexicase_par on a host matrix (no GPU): the rule in plain
 * C++.  Hit planes are checked against it unpacked to 0/1 doubles with
 * maximise = 1 and mode 0.  GPE_E_INVALID for the arguments gpe_lexicase_par
 * refuses and for a NULL values or maximise. */
int gpe_host_lexicase_par(const double* values, int64_t n, int64_t n_cases,
                          const uint8_t* maximise, int mode, double epsilon,
                          uint64_t seed, int64_t k, int32_t* out,
                          int64_t* failed);

/* The number of compacted candidate values (doubles) a gpe_lexicase_par block
 * keeps in LDS; larger candidate sets go through device scratch. */
int64_t gpe_lexicase_par_lds_values(void);

/* DALex selection (Ni, Ding and Spector 2024): selection by weighted sums of
 * the per-case errors.  Every selection draws one normal importance score per
 * case, turns the scores into weights with a softmax and picks the individual
 * with the smallest weighted error sum.  A large `pressure` (the spread of the
 * scores, "particularity pressure") behaves like lexicase, a small one like
 * selection on the mean.  The k selections are one matrix product
 * S = E W'^T, n x n_cases x k fp64 FMAs on v_mfma_f64_16x16x4_f64; the cost
 * grows as n * n_cases * k.  As gpe_lexicase_par, the caller makes one draw, a
 * 64-bit seed, and everything follows from it by this rule.
 *
 * K(i) is gpe_lexicase_par's SplitMix64 key (K(0) = 0xE220A8397B1DCDAF,
 * K(1) = 0x6E789E6AA1B965F4 for seed = 0), and K2(i) the same function with
 * seed ^ 0xD1B54A32D192ED03 in seed's place.  For selection s in [0, k) and
 * case c in [0, C), with j = s * C + c as a uint64:
 * 1. Importance.  u1 = ((K(2j) >> 11) + 1) * 2^-53, u2 = (K(2j + 1) >> 11) *
 *    2^-53, z = sqrt(-2 ln u1) * cos(2 pi u2) (2 pi the double
 *    6.283185307179586, times u2 in fp64), I = pressure * z.  pressure is
 *    finite and >= 0 (pressure * 8.6 must not overflow: |z| <= 8.6).
 * 2. Softmax.  m = max_c I, x_c = exp(I_c - m), w_c = x_c / sum_c x_c, the
 *    sum taken in ascending c in fp64.
 * 3. Fit rows.  A row of the error matrix is fit when every one of its errors
 *    is finite.  Unfit rows take part in nothing below.
 * 4. Standardisation (standardize != 0).  sigma_c is the population standard
 *    deviation (ddof 0) of case c over the m fit rows: mean = hi(sum e) / m,
 *    sigma = sqrt(hi(sum (e - mean)^2) / m), each sum a double-double sum of
 *    256 strided partials (fit row i goes into partial i % 256 in ascending i,
 *    by gpe_run_abserr's two_sum step) merged by a fixed tree of its dd_add.
 *    The effective weight is w'_c = w_c / sigma_c, and 0 where sigma_c == 0;
 *    without standardisation w' = w.  The case mean is not subtracted: that
 *    adds a constant per selection and cannot change the argmin, so the product
 *    runs on the raw non-negative errors and every term is >= 0.
 * 5. Score and pick.  S(i, s) = sum_c w'_{s,c} * e_{i,c} in fp64.  The pick is
 *    the fit row with the smallest (S, K2(s * n + i), i), compared
 *    lexicographically; the tie key is computed only where two scores are
 *    equal, so duplicates are picked uniformly and not by position.  With no
 *    fit row out[s] = -1 and *failed is the smallest such s (-1 if none), as
 *    gpe_lexicase_par.
 * 6. Order independence.  The bits of S(i, s) depend only on row i's values,
 *    column s's weights and C — not on n, k, the row's position or the tile it
 *    lands in: a wave walks all C cases of its tile in steps of 4 (the MFMA's
 *    k), there is no split over the cases and no atomic combine.  Identical
 *    rows get identical scores.  (The host twin sums in ascending c; the two
 *    agree bit for bit where every partial sum is representable, and within
 *    (C + 1) * 2^-53 relative otherwise, every term being >= 0.)
 * On 0/1 hit planes the error of a case is 1 - hit.
 *
 * gpe_dalex: values is a HOST double[n][n_cases] of non-negative errors, or
 * NULL for the per-case matrix of the last gpe_run_cases /
 * gpe_run_abserr_cases (n, n_cases are then the context's; GPE_E_STATE as
 * gpe_lexicase_par, and when another batch was loaded since).  out is
 * int32[k].  n outside 1 .. 2^31 - 1, n_cases outside 1 .. 2^31 - 1 or k
 * outside 0 .. 2^31 - 1: GPE_E_INVALID with a message; a nan, negative or
 * infinite pressure: GPE_E_ARG.  k == 0 does nothing.  Ragged n, n_cases and k
 * are the kernel's business (operand edges are zero-filled, rows >= n masked);
 * there is no limit beyond memory.  The call disturbs nothing else: the
 * resident fitness, the per-case matrix, the hit planes and the active case
 * set stay as they were. */
int gpe_dalex(gpe_ctx* ctx, const double* values, int64_t n, int64_t n_cases,
              uint64_t seed, double pressure, int standardize, int64_t k,
              int32_t* out, int64_t* failed);

/* The same rule on 0/1 hits, e = 1 - hit (every row is fit).  planes is
 * gpe_lexicase_bits_par's HOST matrix uint32[n][ceil(n_cases / 32)], or NULL
 * for the resident hit planes (gpe_run_hit_planes /
 * gpe_run_typed_hit_planes; GPE_E_STATE as there).  The product reads the
 * case-major planes and expands a bit to 1.0 - bit in the operand load; sigma
 * comes from the same kernel as gpe_dalex's, so the picks are those of
 * gpe_dalex on the matrix unpacked to doubles. */
int gpe_dalex_bits(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                   int64_t n_cases, uint64_t seed, double pressure,
                   int standardize, int64_t k, int32_t* out, int64_t* failed);

/* The effective weights of k selections, read back: out_Wt is a HOST
 * double[n_cases][k] (case-major, as the product reads them).  sigma is a
 * HOST double[n_cases] (step 4; gpe_dalex_sigma gives the device's), or NULL
 * for w' = w.  Argument errors as gpe_dalex. */
int gpe_dalex_weights(gpe_ctx* ctx, int64_t n_cases, int64_t k, uint64_t seed,
                      double pressure, const double* sigma, double* out_Wt);

/* sigma of step 4 as the device computes it: out_sigma is a HOST
 * double[n_cases]; values as gpe_dalex. */
int gpe_dalex_sigma(gpe_ctx* ctx, const double* values, int64_t n,
                    int64_t n_cases, double* out_sigma);

/* Weighted sums of the errors themselves: out[i][g] = sum_c weights[g][c] *
 * e[i][c], the product kernel with a store epilogue.  values as gpe_dalex;
 * weights is a HOST double[G][n_cases], any G >= 1, every weight finite and
 * >= 0 (else GPE_E_ARG); out is a HOST double[n][G].  An unfit row (step 3)
 * gives nan.  The sum's order is step 6's: within (n_cases + 1) * 2^-53
 * relative of the exact sum, and exact where every partial sum is
 * representable.  Sizes out of range (G < 1 too): GPE_E_INVALID. */
int gpe_weighted_errors(gpe_ctx* ctx, const double* values, int64_t n,
                        int64_t n_cases, const double* weights, int64_t G,
                        double* out);

/* Device time of the last gpe_dalex / gpe_dalex_bits / gpe_weighted_errors'
 * kernels in ms (fit rows, sigma, weights, product and fold; the upload, the
 * transposition and the copies back are outside). */
int gpe_last_dalex_ms(const gpe_ctx* ctx, float* ms);

/* Host twins (no GPU) in plain C++ with libm: the weights of steps 1 - 4
 * (out_Wt double[n_cases][k]), sigma of step 4 and the selection of gpe_dalex
 * with every score summed in ascending c in fp64.  GPE_E_INVALID for the
 * arguments the device calls refuse and for a NULL matrix or output. */
int gpe_host_dalex_weights(int64_t n_cases, int64_t k, uint64_t seed,
                           double pressure, const double* sigma,
                           double* out_Wt);
int gpe_host_dalex_sigma(const double* values, int64_t n, int64_t n_cases,
                         double* out_sigma);
int gpe_host_dalex(const double* values, int64_t n, int64_t n_cases,
                   uint64_t seed, double pressure, int standardize, int64_t k,
                   int32_t* out, int64_t* failed);

/* Non-dominated sorting (the ranking of NSGA-II selection, Deb et al. 2002):
 * the fronts the reference's sortNondominated returns, in its order, from N^2
 * dominance tests on the GPU.  The rule:
 *
 * Input.  w is a HOST double[n][m] of weighted fitness values (wvalues), one
 * row per distinct fitness; mult int32[n] (or NULL for all 1) says how many
 * individuals share each row, every entry >= 1.
 * 1. Dominance.  Row p dominates row d iff w[p][j] >= w[d][j] for every j and
 *    w[p][j] > w[d][j] for some j (Fitness.dominates).  Equal rows do not
 *    dominate each other; infinities compare as in IEEE; -0.0 == 0.0.
 * 2. Front 0 is the rows nobody dominates, in ascending row index.
 * 3. Front r + 1.  Every unranked row loses one from its dominator count for
 *    each of its dominators in front r; the rows that reach 0 form front
 *    r + 1, ordered by the key (P, d) ascending: P the largest position
 *    within front r among d's dominators there, d the row index.  (The order
 *    in which the reference appends to its next front: a row is appended when
 *    the last of its dominators, in front order, is processed, and each
 *    dominator's list of dominated rows is in ascending index.)
 * 4. Stop after the front with which the individuals covered (the sum of
 *    mult over the ranked rows) reach min(total individuals, k); with
 *    first_front_only, after front 0.  k == 0 gives no fronts.
 * 5. m == 1 needs no peeling: the fronts are the distinct values in
 *    descending order, equal rows of one front in ascending index.  It is one
 *    sort, so a chain of a million fronts is not a million launches.
 * Counts and positions are integers and every combine is an integer atomic
 * add or a sort of distinct keys: the result does not depend on scheduling.
 *
 * order is int32[n]: the rows of front 0, then front 1, ...; front_end is
 * int64[n]: the cumulative ends of the fronts, *n_fronts of them; *n_ranked
 * (= front_end[*n_fronts - 1], or 0) rows of `order` are written.  n outside
 * 1 .. 2^31 - 1, m outside 1 .. 32 or k < 0: GPE_E_INVALID with a message.  A
 * nan in w (the reference's order there depends on its sort's internals) or a
 * mult < 1: GPE_E_ARG.  The matrix is uploaded (n * m doubles) into buffers
 * of the call's own: nothing resident is disturbed.  One small readback per
 * front (rows ranked, individuals covered); the cost grows as m * n^2. */
int gpe_nd_sort(gpe_ctx* ctx, const double* w, const int32_t* mult, int64_t n,
                int64_t m, int64_t k, int first_front_only, int32_t* order,
                int64_t* front_end, int64_t* n_fronts, int64_t* n_ranked);

/* Device time of the last gpe_nd_sort's kernels in ms (counts, peels, sorts;
 * the upload and the readbacks are outside), and its number of fronts. */
int gpe_last_nd_sort_ms(const gpe_ctx* ctx, float* ms);
int gpe_last_nd_sort_fronts(const gpe_ctx* ctx, int64_t* fronts);

/* Host twin (no GPU) of gpe_nd_sort: the same rule in plain C++, the same
 * argument errors (without a message). */
int gpe_host_nd_sort(const double* w, const int32_t* mult, int64_t n,
                     int64_t m, int64_t k, int first_front_only,
                     int32_t* order, int64_t* front_end, int64_t* n_fronts,
                     int64_t* n_ranked);

/* Masked counts of a hit matrix: out[i][g] = popcount(row_i & mask_g), an
 * individual's hits inside each of G case groups.  With the label plane as
 * the one mask the count is a classifier's true positives (and hits - tp its
 * true negatives); with fold, stratum or train / validation planes one
 * evaluation gives every group's count.  planes is a HOST program-major hit
 * matrix uint32[n][ceil(n_cases / 32)] (gpe_run_hit_planes' layout: case c at
 * bit c % 32 of word c / 32), or NULL for the resident matrix of the loaded
 * programs (the last gpe_run_hit_planes / gpe_run_typed_hit_planes; n and
 * n_cases are then the context's, GPE_E_STATE as gpe_lexicase_bits_par(NULL)
 * when none is valid or the program count differs).  masks is a HOST
 * uint32[G][ceil(n_cases / 32)] of the same layout, 1 <= G <= 8, copied to
 * the device per call (G * n_units words; not a case upload).  The library
 * clears the masks' pad bits itself, so a caller's planes may carry set pad
 * bits and a mask with pad bits set counts as the same mask without them.
 * out is a HOST int32[n][G].  GPE_E_ARG with a message for G outside 1 .. 8,
 * n < 0, n_cases outside 1 .. 2^31 - 1 with explicit planes, a NULL masks, or
 * a NULL out with n > 0; n == 0 succeeds and writes nothing.  Rows of up to
 * 64 words get a power-of-two group of lanes each (several rows a wave),
 * longer ones a whole wave per four rows; no atomics.  The call disturbs
 * nothing else: the counts, the resident fitness, the hit planes and their
 * transpose, and the active case set stay as they were. */
int gpe_hit_group_counts(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                         int64_t n_cases, const uint32_t* masks, int G,
                         int32_t* out);

/* Device time of the last gpe_hit_group_counts' kernel in ms (events around
 * the launch; the copies of the masks and the counts are outside). */
int gpe_last_hit_group_ms(const gpe_ctx* ctx, float* ms);

/* Host twin of gpe_hit_group_counts on a host matrix (no GPU): the same
 * arithmetic in plain C++; GPE_E_ARG for the arguments it refuses and for a
 * NULL planes with n > 0. */
int gpe_host_hit_group_counts(const uint32_t* planes, int64_t n,
                              int64_t n_cases, const uint32_t* masks, int G,
                              int32_t* out);

/* Case weights on a hit matrix H (bool[n][n_cases]): three entry points that
 * share their matrix argument.  planes is a HOST program-major hit matrix
 * uint32[n][ceil(n_cases / 32)] (eps is ignored; set pad bits are ignored
 * too), or NULL for the resident matrix of the loaded programs by
 * gpe_informed_cases' routes (n, n_cases are then the context's): the hit
 * planes of the last gpe_run_hit_planes / gpe_run_typed_hit_planes, or on the
 * F machine without them the per-case matrix of the last gpe_run_abserr_cases
 * / gpe_run_cases, where case c is a hit of program i when its value e is
 * finite and e <= eps (eps >= 0 and not nan, else GPE_E_ARG).  GPE_E_STATE
 * with gpe_informed_cases' messages when no such matrix of the loaded
 * programs is resident.  GPE_E_ARG with a message naming the value for n < 0,
 * n_cases outside 1 .. 2^31 - 1, and for n > INT32_MAX where counts are made;
 * n == 0 succeeds (explicit planes: the counts are written as zeros, no sum
 * is).  Nothing resident is written except the cached case-major transpose
 * of the hit planes (gpe_lexicase_bits' d_hit_t): the per-case matrix, the hit
 * planes, the resident fitness, the active case set and every launch plan
 * stay as they were.
 *
 * gpe_case_solve_counts: out_counts int32[n_cases] (HOST, not NULL),
 * s[c] = the programs i with H[i][c] and live bit i set.  live is a HOST
 * uint64[ceil(n / 64)], program i at bit i % 64 of word i / 64 (bits past n
 * are ignored), or NULL for all live.  A popcount of the case-major planes:
 * a power-of-two group of lanes per case (a whole wave from 4,033 programs
 * on), integer shuffles, no atomics. */
int gpe_case_solve_counts(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                          int64_t n_cases, double eps, const uint64_t* live,
                          int32_t* out_counts);

/* Weighted hits: out[i][g] = the sum of weights[g][c] over the cases c with
 * H[i][c]; weights is a HOST double[G][n_cases], 1 <= G <= 8, every weight
 * finite and >= 0 (-0.0 counts as 0.0) and every row's sum finite (the caller
 * checks the sum); out is a HOST double[n][G].  A row with no hits is +0.0.
 * The sum is a double-double sum in one fixed order, whatever G, the row
 * length and the grid are: partial p of 64 takes the hit cases c = p, p + 64,
 * ... in ascending order by (hi, r) = two_sum(hi, w); lo += r; the partials
 * merge by the xor butterfly m = 32 .. 1, partial p taking
 * dd_add(partial p, partial p ^ m) (gpe_run_abserr's dd_add); out is hi of
 * partial 0.  With non-negative terms nothing cancels: |hi + lo - S| <=
 * n_cases * 2^-100 * S for the exact sum S, so out is S rounded to fp64 or
 * its neighbour, and exactly S whenever every partial sum is representable.
 * A wave per row; the weights sit in LDS while G * n_cases * 8 bytes fit
 * 64 KiB and are read through L2 otherwise, with the same bits.  GPE_E_ARG
 * with a message for G outside 1 .. 8, a NULL weights, a NULL out with n > 0,
 * and a weight that is negative, nan or inf. */
int gpe_hit_weighted_sums(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                          int64_t n_cases, double eps, const double* weights,
                          int G, double* out);

/* Implicit fitness sharing: gpe_case_solve_counts (live, out_counts as there;
 * out_counts may be NULL), then gpe_hit_weighted_sums with G = 1 under
 * w[c] = s[c] > 0 ? 1.0 / (double)s[c] : 0.0 (one correctly rounded
 * division), out a HOST double[n].  The counts kernel writes the weights on
 * the device and the sums kernel follows it on the stream: neither the counts
 * nor the weights visit the host in between.  A program whose live bit is
 * clear is left out of the counts; its own sum is still written (the caller
 * overwrites it). */
int gpe_hit_shared_sums(gpe_ctx* ctx, const uint32_t* planes, int64_t n,
                        int64_t n_cases, double eps, const uint64_t* live,
                        int32_t* out_counts, double* out);

/* Device time of the last of these three calls' kernels in ms (events around
 * the counts and sums launches; the copies, the thresholding and the
 * transposition are outside). */
int gpe_last_case_weights_ms(const gpe_ctx* ctx, float* ms);

/* Host twins on a host matrix (no GPU): plain loops in the same order, so
 * the sums agree bit for bit.  out_lo (may be NULL) receives lo of the final
 * normalised pair, for accuracy tests.  GPE_E_ARG for the arguments the device
 * calls refuse and for a NULL planes with n > 0. */
int gpe_host_case_solve_counts(const uint32_t* planes, int64_t n,
                               int64_t n_cases, const uint64_t* live,
                               int32_t* out_counts);
int gpe_host_hit_weighted_sums(const uint32_t* planes, int64_t n,
                               int64_t n_cases, const double* weights, int G,
                               double* out, double* out_lo);
int gpe_host_hit_shared_sums(const uint32_t* planes, int64_t n,
                             int64_t n_cases, const uint64_t* live,
                             int32_t* out_counts, double* out, double* out_lo);

/* Device tournament selection that replays the reference's random stream:
 * selTournament (deap/tools/selection.py:51-69, aspirants drawn by selRandom
 * :15-28, i.e. random.choice) — k tournaments of tournsize aspirants, the
 * winner the first aspirant with the greatest fitness (Fitness.__gt__:
 * not (a.wvalues <= b.wvalues), Python tuple order).  wvalues is a HOST
 * double[n][nobj] (fitness.wvalues per individual), or NULL to select on the
 * last gpe_run's fitness still on the device (MSE: (hi + lo) / n_cases,
 * SSE and hit modes: hi), times `weight` (nobj = 1, n = programs) — no host
 * round trip.  mt_state[625] (in/out) as in gpe_lexicase: the draws are
 * CPython's getrandbits rejection sampling on MT19937, and the state after
 * them is written back.  Writes the k selected indices to out. */
int gpe_tournament(gpe_ctx* ctx, const double* wvalues, int64_t n, int nobj,
                   double weight, int64_t k, int tournsize, uint32_t* mt_state,
                   int32_t* out);

/* ---- Lowering on the device (the host flattener's job, deap_amd/flatten.py
 * Flattener._build/_emit/_encode, run one tree per GPU thread from the same
 * source, deap_amd/csrc/lower_core.h).  The host maps each node object of a
 * PrimitiveTree (reference deap/gp.py:44-184) to an entry of the primitive
 * set (deap/gp.py:260-456) and uploads one byte per node. */
typedef struct {          /* a Python number as the constant fold sees it */
  char t;                 /* 'f' float, 'i' int, 'b' bool, 'x' unsupported */
  double f;
  int64_t i;
  bool err_value;         /* the fold raised ValueError (sin/cos of inf) */
} gpe_value;
typedef struct {          /* one primitive / terminal of the pset */
  int32_t kind;           /* 0 primitive, 1 argument, 2 constant terminal */
  int32_t arity;
  int32_t sem;            /* deap_amd/flatten.py _NATIVE_SEM */
  int32_t var;            /* argument index */
  gpe_value c;            /* constant terminal's value */
} gpe_entry;

/* The pset tables of gpe_lower_programs: the machine (GPE_MACHINE_*), the
 * number of case variables, per argument whether sin/cos of it is read from
 * a trig-leaf column (gpe_set_trig_leaves), and the entries (< 255). */
int gpe_set_lowering(gpe_ctx* ctx, int machine, int nv, const uint8_t* leaf,
                     int n_leaf, const gpe_entry* entries, int n_entries);

/* Lower n trees on the device and load them as programs (as
 * gpe_load_programs does with host-flattened words).  codes[node_off[i] ..
 * node_off[i+1]) are tree i's node entries in prefix order, 255 for an
 * ephemeral constant whose value is the next of evals[eph_off[i] ..
 * eph_off[i+1]).  Per tree (host arrays): out_depth, out_err (0, 3 =
 * SyntaxError of a too-tall tree, 4 = a raising constant fold), out_status
 * (bit 0: declined — the host flattener must lower it, Python semantics the
 * device fold does not cover; bit 1: an int constant beyond 2^53 evaluated
 * in float64; bit 2: the raising fold is ValueError).  A declined tree is
 * loaded as END; the caller re-flattens the batch on the host.  On an error
 * return the context holds no programs.  Trees past 65,535 nodes are
 * declined (the device's lowering records hold 16-bit node indices). */
int gpe_lower_programs(gpe_ctx* ctx, const uint8_t* codes, const int64_t* node_off,
                       int64_t n, const gpe_value* evals, const int64_t* eph_off,
                       int32_t* out_depth, uint8_t* out_err, uint8_t* out_status);

/* gpe_lower_programs in chunks, for callers that read the trees in chunks:
 * the same result as one call on the concatenated trees, but each chunk's
 * upload and lowering run on the device (asynchronously, on the context's
 * stream) while the caller reads the next one.  gpe_lower_begin(n_total),
 * then gpe_lower_add for consecutive chunks of the trees (each chunk's
 * node_off / eph_off start at 0; its arrays may be freed when the call
 * returns), then gpe_lower_end with the per-tree outputs of all n_total
 * trees.  No other call may use the context in between; an error ends the
 * lowering (the context then holds no programs).  GPUEvaluator reads a
 * million trees in chunks (deap_amd/evaluator.py lower_on_device). */
int gpe_lower_begin(gpe_ctx* ctx, int64_t n_total);
/* gpe_lower_begin with the per-tree outputs given up front (all n_total
 * entries; they must stay valid until gpe_lower_end): each gpe_lower_add
 * then decodes the chunks whose metadata has reached the host, on the
 * caller's thread, so that gpe_lower_end is left with the last chunks only.
 * gpe_lower_end is then called with these pointers or with NULLs. */
int gpe_lower_begin_into(gpe_ctx* ctx, int64_t n_total, int32_t* out_depth, uint8_t* out_err,
                         uint8_t* out_status);
int gpe_lower_add(gpe_ctx* ctx, const uint8_t* codes, const int64_t* node_off, int64_t n,
                  const gpe_value* evals, const int64_t* eph_off);
int gpe_lower_end(gpe_ctx* ctx, int32_t* out_depth, uint8_t* out_err, uint8_t* out_status);
/* After gpe_lower_end (or gpe_lower_programs): how many of the trees got a
 * nonzero error code / status, so that a caller can skip scanning a million
 * zeros. */
int gpe_last_lower_flags(gpe_ctx* ctx, int64_t* n_err, int64_t* n_status);

/* gpe_load_programs + gpe_run. */
int gpe_eval(gpe_ctx* ctx, int mode, const uint32_t* code, int64_t n_words,
             const int64_t* off, int64_t n_prog, const int32_t* depth,
             double* out_hi, double* out_lo, uint64_t* out_err,
             uint32_t* out_flags);

/* Exact-integer pass.  The reference evaluates trees with Python numbers
 * (gp.compile, deap/gp.py:462-487): int constants (rand101,
 * examples/gp/symbreg.py:43) and protectedDiv's int 1 (:29-33) stay exact
 * ints through operator.add/sub/mul/neg, int / int rounds the exact ratio
 * once, and ints compare exactly with floats.  The kernels compute in
 * float64, which agrees while every int stays within 2^53.  The n programs
 * listed here (flatten.py Flattener.exact_programs: those whose ints can
 * pass 2^53) are re-evaluated after every run of the loaded population
 * with Python's semantics (glibc sin/cos), overwriting their outputs: hi/lo
 * and the per-case matrix of gpe_run_cases.  The device holds ints as sign
 * + 1088-bit magnitude; a program with a wider int constant, and a device
 * program whose case outgrew 1088 bits, is evaluated on the host with
 * unbounded ints instead (the same semantics, the same order of summation),
 * so every result is the reference's.  Modes MSE, SSE_SEQ (the exact pass
 * sums in its fixed order) and HITS_BOOL, fp64 only; SSE_NUMPY and fp32 runs
 * skip the pass.  A case's first exception goes to out_err as the reference
 * raises it: GPE_ERR_VALUE (sin/cos(inf)), GPE_ERR_OVERFLOW (float(int) or
 * int / int past the float range, or d**2).
 * progs[n]: indices into the loaded population; code/off/depth: their
 * programs in the usual words, except that an int constant has index field
 * 1 and its row of the int table in its two data words (low word first).
 * The table: n_ints rows of little-endian 32-bit words in two's complement,
 * row r = int_words[int_off[r] .. int_off[r + 1]) (int_off[0] = 0).
 * Cleared by gpe_load_programs, gpe_lower_programs and gpe_set_cases (call
 * it after those); n = 0 clears. */
int gpe_load_exact_v(gpe_ctx* ctx, const int32_t* progs, int64_t n,
                     const uint32_t* code, int64_t n_words, const int64_t* off,
                     const int32_t* depth, const uint32_t* int_words,
                     const int64_t* int_off, int64_t n_ints);

/* gpe_load_exact_v with rows of GPE_XINT_WORDS words: ints[n_ints][34],
 * and the round-4 encoding of an int constant (index field 1 + row, the
 * f64 bits in its data words), translated to gpe_load_exact_v's. */
int gpe_load_exact(gpe_ctx* ctx, const int32_t* progs, int64_t n,
                   const uint32_t* code, int64_t n_words, const int64_t* off,
                   const int32_t* depth, const uint32_t* ints, int64_t n_ints);

/* Exact-pass programs the last run evaluated on the host (ints past the
 * device's 1088 bits). */
int gpe_last_exact_host_runs(gpe_ctx* ctx, int64_t* n);

/* ... and the wall time of that host pass, ms (0 when none ran): a slow
 * host fallback shows up in the caller's stats. */
int gpe_last_exact_host_ms(gpe_ctx* ctx, double* ms);

/* ---- Multi-GPU over one node: one process per GPU,
 * each with its own context; the context owns an RCCL communicator.
 * Replaces the reference's only parallelism, a user-registered
 * multiprocessing.Pool.map over individuals (examples/ga/onemax_mp.py:58-59,
 * doc/tutorials/basic/part4.rst:19-56), which has no C-level interface.
 * RCCL is opened at first use (dlopen librccl.so.1); GPE_E_STATE if absent. */
#define GPE_UNIQUE_ID_BYTES 128

/* Rank 0 creates the communicator id (ncclGetUniqueId) and hands the
 * GPE_UNIQUE_ID_BYTES bytes to the other ranks by any means (a file, a
 * socket, torch.distributed's broadcast); no context needed. */
int gpe_comm_unique_id(void* id_out);

/* Join the communicator (ncclCommInitRank on the context's device).
 * Collective: every rank calls it with the same id and world. */
int gpe_comm_init(gpe_ctx* ctx, int rank, int world, const void* unique_id);

/* rank / world of the context's communicator (-1 / 0 if none). */
int gpe_comm_info(const gpe_ctx* ctx, int* rank, int* world);

/* Case sharding (config 4): this rank holds cases [case_offset,
 * case_offset + n_cases) (gpe_set_cases) and the same programs as every
 * rank.  gpe_run on the slice, then on the context's stream: the (hi, lo)
 * partials are all-gathered and summed in rank order as double-doubles, the
 * first-error codes (global case index) reduced with MIN and the flag bits
 * OR-ed.  Every rank receives the whole-population result.  MSE and hits
 * modes only (GPE_E_INVALID for the order-exact numpy / builtin-sum modes).
 * Collective.  _device: outputs are device arrays (NULL: the context's own),
 * no host synchronisation; otherwise host arrays of n_prog entries. */
int gpe_run_sharded_device(gpe_ctx* ctx, int mode, int64_t case_offset,
                           void* d_hi, void* d_lo, void* d_err, void* d_flags);
int gpe_run_sharded(gpe_ctx* ctx, int mode, int64_t case_offset,
                    double* out_hi, double* out_lo, uint64_t* out_err,
                    uint32_t* out_flags);

/* Population sharding (config 3): each rank loaded its own slice of the
 * programs (at most `width`); after gpe_run they are all-gathered, so every
 * rank receives host arrays of world * width entries, rank r's program i at
 * r * width + i (entries past a rank's n_prog: hi = lo = 0, err =
 * GPE_NO_ERROR, flags = 0).  tags (n_prog bytes, may be NULL) travel with
 * the results in bits 8..15 of out_flags (the Python layer sends the
 * flattener's per-tree verdicts this way).  Collective. */
int gpe_run_gathered(gpe_ctx* ctx, int mode, int64_t width,
                     const uint8_t* tags, double* out_hi, double* out_lo,
                     uint64_t* out_err, uint32_t* out_flags);

/* Device time of the last gpe_run* (HIP events on the context's stream):
 * ms[0] = interpreter kernels, ms[1] = reduction kernel, ms[2] = total. */
int gpe_last_timing(const gpe_ctx* ctx, float* ms);

/* Collective time of the last sharded run (HIP events on the context's
 * stream): ms[0] = the RCCL group of gpe_run_sharded* (all-gather of the
 * partials, first-error MIN, flag SUM) or the all-gather of
 * gpe_run_gathered, ms[1] = the case-sharded redo-flag all-reduce (0 when
 * none ran: the exact cores raise no flags).  Every wait on a stream that
 * holds collectives is bounded by GPE_COMM_TIMEOUT_S seconds (default 120):
 * past it the communicator is aborted and the call returns GPE_E_COMM with
 * the collective, rank and RCCL's asynchronous error in gpe_last_error().
 * Replaces nothing in the reference (its Pool.map, examples/ga/
 * onemax_mp.py:58-59, has no collectives to time or bound). */
int gpe_last_comm_timing(gpe_ctx* ctx, float* ms);

/* Test infrastructure (no HIP calls): the bounded wait above on a fake
 * stream that stays busy for `busy_polls` queries (< 0: forever); returns
 * 0 or GPE_E_COMM and the message a timed-out collective would report. */
int gpe_debug_bounded_wait(double timeout_s, int64_t busy_polls, char* msg, size_t n);

/* Launch geometry of the last gpe_run (for reports): programs on the asm
 * core, on the C++ fast and deep kernels, programs re-run because a sin/cos
 * argument left the asm core's range, programs per wave, tile groups,
 * (program, tile) pairs that raised the re-run flag, waves per block. */
int gpe_last_geometry(const gpe_ctx* ctx, int64_t* out8);

/* gpe_last_geometry's eight fields (there "programs on the asm core" counts
 * both asm cores), then for the deep asm core (programs needing 6..12 stack
 * slots): programs, programs per wave, tile groups, waves per block; then
 * the re-run programs that the exact asm core (glibc's sin/cos) left to the
 * C++ exact kernels (a sin/cos argument at or past 105414350, inf or nan);
 * then for the typed asm core (GPE_MODE_HITS_BOOL: PrimitiveSetTyped
 * programs, spambase.py): programs, programs per wave, tile groups; then
 * the HITS_BOOL programs that are one folded constant, whose hit count
 * (the cases whose label has the constant's truth) needs no core run.
 * Writes the first min(n, GPE_GEOMETRY_FIELDS) fields. */
#define GPE_GEOMETRY_FIELDS 17
int gpe_last_geometry_ex(const gpe_ctx* ctx, int64_t* out, int n);

/* One launch of the last gpe_run as the planner shaped it (read-only, for
 * tests and reports).  `which`: the D = 5 asm core and the deep asm core as
 * they ran (the exact cores' launches when the run put its asm programs on
 * them, as gpe_last_geometry reports them, else the table or fp32 cores'),
 * the typed core, the C++ fast and deep kernels, and the table / fp32 asm
 * cores' own plans (from which an exact run takes its programs).  Fields:
 * programs, programs per wave, waves per block, waves, slots (waves x
 * programs per wave, -1 padded), cases per lane of an asm core (0: a C++
 * kernel), stack slots, case tiles, tiles per group, tile groups, two tile
 * buffers (0 / 1), the dynamic LDS bytes the launch passed to its kernel
 * (0: planned but not launched, or no programs), and whether the launch ran
 * with the exact core's resident tile loop (0 / 1: the exact D = 5 core on a
 * lean launch — one target column, no per-case output — with two tile
 * buffers, unless GPE_TILE_LOOP=0, read once by gpe_create).  Writes the first
 * min(n, GPE_LAUNCH_SHAPE_FIELDS) fields; GPE_E_INVALID for another `which`. */
#define GPE_LAUNCH_ASM_FAST 0
#define GPE_LAUNCH_ASM_DEEP 1
#define GPE_LAUNCH_TYPED 2
#define GPE_LAUNCH_CPP_FAST 3
#define GPE_LAUNCH_CPP_DEEP 4
#define GPE_LAUNCH_FASM 5
#define GPE_LAUNCH_DASM 6
#define GPE_LAUNCH_MOMENTS 7      /* the last moments run's launch of the exact
                                     D = 5 core's moments kernel ... */
#define GPE_LAUNCH_MOMENTS_DEEP 8 /* ... and of the exact deep core's */
#define GPE_LAUNCH_ABSERR 9       /* the last abs-error run's launch of the exact
                                     D = 5 core's abs-error kernel ... */
#define GPE_LAUNCH_ABSERR_DEEP 10 /* ... and of the exact deep core's */
#define GPE_LAUNCH_SHAPE_FIELDS 13
int gpe_last_launch_shape(const gpe_ctx* ctx, int which, int64_t* out, int n);

/* Diagnostic (host only): the program -> threaded-code translation the asm
 * core executes, with a caller-given handler table; starts[i] = -1 for
 * programs the asm core does not run.  Lets CPU tests check translation and
 * jump targets without a GPU. */
int gpe_debug_translate(const uint32_t* code, int64_t n_words,
                        const int64_t* off, int64_t n_prog,
                        const int32_t* depth, int nv, const uint32_t* table,
                        int n_table, uint32_t* out, int64_t out_cap,
                        int64_t* starts, int64_t* n_out);

/* gpe_debug_translate as the exact cores' translation runs it: with the case
 * columns' bounds lo[v], hi[v] (v < nv), every sin/cos word is the handler
 * of its argument's proven range (the table's SIN_MID, COS_MID, SIN_SMALL,
 * COS_SMALL entries after COS); lo == hi == NULL: gpe_debug_translate.  The
 * word count never depends on the bounds. */
int gpe_debug_translate_ranges(const uint32_t* code, int64_t n_words,
                               const int64_t* off, int64_t n_prog,
                               const int32_t* depth, int nv, const uint32_t* table,
                               int n_table, uint32_t* out, int64_t out_cap,
                               int64_t* starts, int64_t* n_out, const double* lo,
                               const double* hi);

/* Diagnostic (host only, no context): the range pass over one F-machine
 * program (n_words flattener words ending in END) with column bounds lo[v],
 * hi[v] (v < nv; an infinite bound: unbounded).  Writes the class of each
 * sin/cos node in word order — 0 general, 1 mid (|x| < 2.42 proven in every
 * lane), 2 small (|x| < 0.855) — into out[0 .. cap) and returns their number,
 * or -1 for a malformed program. */
int gpe_debug_trig_classes(const uint32_t* code, int64_t n_words, const double* lo,
                           const double* hi, int nv, int32_t* out, int64_t cap);

/* The sin/cos words of the last exact-core translation per base class:
 * out[0] general, out[1] mid, out[2] small, as gpe_debug_trig_classes
 * classes them (GPE_TRIG_RANGES=0, read once by gpe_create: all general).
 * The column bounds the classes are proven from are those of the last
 * gpe_set_cases.  The handlers picked: gpe_last_trig_picked. */
int gpe_last_trig_classes(const gpe_ctx* ctx, int64_t* out);

/* gpe_debug_translate_ranges and gpe_debug_trig_classes with the pass's mode
 * (GPE_TRIG_RANGES, read once by gpe_create): 1, what those two do — the
 * base classes general,
 * mid, small; 2, the library's default — also 3 midlo (a cos node with
 * |x| < 1.44 proven: COS_MIDLO, the table's entry after COS_SMALL) and 4 wide
 * (every lane finite and |x| < 1e8: SIN_WIDE, COS_WIDE, the last two
 * entries), and a sin/cos over a possibly non-finite value is bounded by
 * [-1, 1] "or NaN", which mid, small and midlo accept (csrc/trig_ranges.h).
 * gpe_debug_translate_mode also takes 3, the library's default: mode 2 with
 * midlo for a sin node too, and for mid and midlo the handlers with static
 * lane roles (SIN_MID3, COS_MID3, SIN_MIDLO3, COS_MIDLO3, the table's last
 * four entries), and 4: mode 2's classes with mode 3's handlers (a sin node
 * below 1.44 stays mid: SIN_MID3), the A/B control of SIN_MIDLO3.  The classes
 * of those modes: gpe_debug_trig_picks, which takes 1 to 4.  Any other mode:
 * an error. */
int gpe_debug_translate_mode(const uint32_t* code, int64_t n_words,
                                const int64_t* off, int64_t n_prog,
                                const int32_t* depth, int nv, const uint32_t* table,
                                int n_table, uint32_t* out, int64_t out_cap,
                                int64_t* starts, int64_t* n_out, const double* lo,
                                const double* hi, int mode);
int gpe_debug_trig_classes_mode(const uint32_t* code, int64_t n_words, const double* lo,
                            const double* hi, int nv, int mode, int32_t* out, int64_t cap);
int gpe_debug_trig_picks(const uint32_t* code, int64_t n_words, const double* lo,
                         const double* hi, int nv, int mode, int32_t* out, int64_t cap);

/* The sin/cos words of the last exact-core translation by the class whose
 * handler was picked: out[0] general, out[1] mid, out[2] small, out[3] midlo,
 * out[4] wide; their sum is that of gpe_last_trig_classes, which keeps
 * counting the base classes (GPE_TRIG_RANGES=1's choice) in every mode.
 * GPE_TRIG_RANGES=1: out[3] = out[4] = 0 and the rest is
 * gpe_last_trig_classes'.  GPE_TRIG_RANGES=3, the default: out[3] counts the
 * sin nodes picked midlo too (mode 2 counts them mid). */
int gpe_last_trig_picked(const gpe_ctx* ctx, int64_t* out);

/* Diagnostic: evaluate the device's sin (fn 0), cos (fn 1), square (fn 2),
 * the platform libm's sin (3) / cos (4), or sin (5) / cos (6) through the
 * hand-scheduled asm interpreter core; fp32 mode: sin (7) / cos (8) through
 * the fp32 asm core, sin (9) / cos (10) of the C++ kernels; glibc_sin (11) /
 * glibc_cos (12), the restatement of the reference's libm; sin (13) /
 * cos (14) through the exact asm core (glibc's algorithm in the handler;
 * arguments it leaves to the C++ pass through glibc_sin/cos); the C++
 * kernels' square root, fp64 (15) and fp32 of (float)x (16): IEEE, correctly
 * rounded, nan for a negative argument; the same through the exact asm core's
 * SQRT handler (17) and the fp32 asm core's (18), the handler's own value in
 * every lane; on n host
 * inputs — the elementary operations whose rounding can differ from glibc.
 * Used by the parity tests to quantify ulp differences. */
int gpe_math_probe(gpe_ctx* ctx, int fn, const double* x, double* y,
                   int64_t n);

/* The same sin (0) / cos (1) / square (2) code compiled for the host CPU
 * (no GPU needed): lets the CPU test suite check the kernels' elementary
 * functions bit for bit against correctly rounded values.  3 / 4: the fp32
 * mode's sin / cos of (float)x, returned as double.  5 / 6: glibc_sin /
 * glibc_cos (the restatement of glibc 2.35's sin/cos the redo pass uses;
 * checked against the host libm bit for bit).  7 / 8: the same through the
 * exact interpreter's two-cases-at-once form (glibc_trig_k). */
int gpe_host_math(int fn, const double* x, double* y, int64_t n);

/* Host twin of the GPE_MODE_SSE_NUMPY reduction (test infrastructure): the
 * numpy.sum of each of n_rows contiguous rows of n_cols doubles, in
 * numpy's order (replaces numpy.sum at examples/gp/symbreg_numpy.py:66). */
int gpe_host_np_sum(const double* x, int64_t n_rows, int64_t n_cols,
                    double* out);

/* Test infrastructure for the multi-rank collectives on one device.
 * gpe_debug_shard_combine: gpe_run_sharded_device's combine for `world`
 * ranks whose outputs the caller gives (parts[world][2][n]: each rank's
 * (hi, lo) partials, the buffer its RCCL all-gather fills; errs[world][n],
 * flags[world][n]: each rank's first-error words and flag bits as its run
 * left them; case_offsets[world]): the same shard_prep and shard_finish
 * kernels, with the two all-reduces (MIN of the errors, SUM of the packed
 * flag counters) computed on the device from the given arrays.  Replaces
 * the reference's Pool.map over individuals
 * (examples/ga/onemax_mp.py:58-59), which has no combine of its own.
 * gpe_debug_redo_union: redo flags (one per loaded program, n = 0 clears)
 * that "other ranks" raised; every later run ORs them into this context's
 * own before its redo pass, as the case-sharded all-reduce (MAX) does. */
int gpe_debug_shard_combine(gpe_ctx* ctx, int world, int64_t n,
                            const double* parts, const uint64_t* errs,
                            const uint32_t* flags, const int64_t* case_offsets,
                            double* out_hi, double* out_lo, uint64_t* out_err,
                            uint32_t* out_flags);
int gpe_debug_redo_union(gpe_ctx* ctx, const uint32_t* flags, int64_t n);

/* Host twin of the exact pass's device interpreter (test infrastructure):
 * one program (gpe_load_exact_v's encoding and int table) on one case
 * x[nv].  Returns 0, the case's GPE_ERR_* (1 ValueError, 2 OverflowError,
 * 3 past the device's 1088 bits), or a negative error.  *out_isint: whether
 * the result is a Python int; *out_f: float(result) (inf where that would
 * overflow); out_words[GPE_XINT_WORDS]: the int as 1088-bit two's
 * complement. */
int gpe_host_exact_eval(const uint32_t* code, const uint32_t* int_words,
                        const int64_t* int_off, int64_t n_ints, const double* x,
                        int nv, double* out_f, uint32_t* out_words, int* out_isint);

/* The host evaluator of the exact pass's wide programs (no int size limit;
 * csrc/bigint_host.h) on one case.  Returns as gpe_host_exact_eval, never
 * 3.  The int result goes to out_words as two's complement in
 * *inout_nwords words (the capacity in, the count out; a capacity too small
 * returns GPE_E_INVALID with the count needed; out_words NULL: the count
 * only). */
int gpe_host_bigint_eval(const uint32_t* code, const uint32_t* int_words,
                         const int64_t* int_off, int64_t n_ints, const double* x,
                         int nv, double* out_f, uint32_t* out_words,
                         int64_t* inout_nwords, int* out_isint);

#ifdef __cplusplus
}
#endif

#endif /* GPEVAL_H */
