/* bioen_hip.h -- C ABI of the MI355X (gfx950) BioEn optimizer hot path.
 *
 * This is the boundary a BioEn maintainer binds instead of the Cython module
 * bioen/optimize/ext/c_bioen.pyx (ctypes stub: bioen_amd/optimize/ext/c_bioen.py,
 * walk-through: INTEGRATION.md).  Plain C: pointers, sizes, PODs.  No torch
 * types, no C++ types.  All arithmetic is IEEE double.
 *
 * Ownership: every `const double*` / `double*` argument is a HOST buffer owned
 * by the caller and only read (inputs) or written (outputs) during the call;
 * nothing is retained after return (the batch optimizers register large result arrays with the
 * HIP runtime -- hipHostRegister -- while the call runs, so that finished problems leave by DMA,
 * and unregister them before they return).  Device memory belongs to the context and
 * is released by bioen_hip_ctx_destroy().  A context is not re-entrant (one
 * HIP stream, one scratch set); distinct contexts are independent.
 *
 * Return value: 0 on success, a negative BIOEN_HIP_E* code otherwise
 * (bioen_hip_strerror() gives the text; bioen_hip_last_error() the detail).
 * The L-BFGS drivers additionally report the liblbfgs status code through
 * `lbfgs_code` (0,1,2 = success; negative = liblbfgs error numbering,
 * third-party/liblbfgs-1.10/include/lbfgs.h:76-147), which the Python shim
 * turns into the reference's RuntimeError("... return code ...").
 */
#ifndef BIOEN_HIP_H
#define BIOEN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIOEN_HIP_OK 0
#define BIOEN_HIP_EINVAL (-1)    /* bad argument (NULL, non-positive size, ...) */
#define BIOEN_HIP_ENODEV (-2)    /* no usable HIP device */
#define BIOEN_HIP_EHIP (-3)      /* a HIP runtime call failed */
#define BIOEN_HIP_ENOMEM (-4)    /* device or host allocation failed */
#define BIOEN_HIP_ERCCL (-5)     /* RCCL unavailable or an RCCL call failed */
#define BIOEN_HIP_ESTATE (-6)    /* call not valid in the context's state */

typedef struct bioen_hip_ctx bioen_hip_ctx;

/* Same fields, same order as the reference's lbfgs_config_params
 * (bioen/optimize/ext/c_bioen_common.h:69-79) so the shim mirrors its packing. */
typedef struct bioen_lbfgs_config {
    int linesearch;      /* 0 More-Thuente, 1 Armijo, 2 Wolfe (yaml default), 3 strong Wolfe */
    int max_iterations;
    double delta;
    double epsilon;
    double ftol;
    double gtol;
    double wolfe;
    int past;
    int max_linesearch;
} bioen_lbfgs_config;

/* Same fields, same order as the reference's gsl_config_params (c_bioen_common.h:62-67);
 * algorithm ids of c_bioen_common.h:28-34: 0 conjugate_fr, 1 conjugate_pr, 2 vector_bfgs2,
 * 3 vector_bfgs, 4 steepest_descent. */
typedef struct bioen_gsl_config {
    double step_size;
    double tol;
    int max_iterations;
    int algorithm;
} bioen_gsl_config;

/* reference visual_params, c_bioen_common.h:89-92 */
typedef struct bioen_visual_params {
    size_t debug;
    size_t verbose;
} bioen_visual_params;

/* What the reference only prints (c_bioen_kernels_logw.c:646-653) is returned. */
typedef struct bioen_opt_result {
    double fmin;          /* final negative log-posterior                        */
    double chi2;          /* 0.5 * |yTilde w - YTilde|^2 at the optimum          */
    double kl;            /* KL(w || w0) = -S at the optimum (S: utils.py:83-106) */
    double seconds;       /* wall time inside the minimiser (device-synchronised) */
    int lbfgs_code;       /* liblbfgs status (GSL status for the opt_gsl_* entry points) */
    int iterations;       /* progress-callback count (accepted line searches)     */
    int evaluations;      /* objective+gradient evaluations                       */
    int reserved;
} bioen_opt_result;

/* ---- library / device ------------------------------------------------------ */
const char* bioen_hip_version(void);
int bioen_hip_device_count(int* count);
const char* bioen_hip_strerror(int code);
const char* bioen_hip_last_error(void);
/* replaces lbfgs_strerror(), bioen/optimize/ext/c_bioen_error.c:23-115 */
const char* bioen_hip_lbfgs_strerror(int lbfgs_code);
/* replace _set_fast_openmp_flag/_get_fast_openmp_flag (c_bioen_common.c:46-55): accepted and stored.  What the
 * reference's flag = 0 buys -- the same bits whatever the thread count (serial sums, c_bioen_kernels_logw.c:58-93;
 * test/optimize/test_logw_reproducibility.py:14-46) -- holds here for BOTH values, and across GPU counts: every sum over
 * structures is formed per canonical column segment and the segments' totals are added in segment order (see the
 * sharded contexts below), so 1, 2, 4 and 8 GPUs return identical bits. */
void bioen_hip_set_fast_openmp_flag(int flag);
int bioen_hip_get_fast_openmp_flag(void);

/* ---- context: yTilde (m x n, row-major, host) is uploaded once and stays
 *      resident in HBM across evaluations, thetas and minimiser runs.
 *      Replaces the per-call pointer bag params_t (c_bioen_common.h:44-60) and
 *      the host-side transposed copy of c_bioen.pyx:471-473 (not needed). ---- */
int bioen_hip_ctx_create(int m, int n, const double* yTilde, const double* YTilde,
                         int device, bioen_hip_ctx** ctx);
/* Synthetic ensemble generated directly in HBM (bench / scale tests):
 *   yTilde[i][j] = (YTrue[i] + sig_sim[i] * z_ij) / sig_exp[i],  z_ij ~ N(0,1)
 * with z_ij a counter-based Box-Muller stream of (seed, i, j); recipe after
 * forces.gen_sythetic_ensemble (bioen/optimize/forces.py:44-68). */
int bioen_hip_ctx_create_synthetic(int m, int n, const double* YTrue, const double* sig_sim,
                                   const double* sig_exp, const double* YTilde,
                                   unsigned long long seed, int device, bioen_hip_ctx** ctx);
/* Structure-sharded contexts (multi-GPU, one process per GPU).  The n columns are cut into CANONICAL SEGMENTS: 8 of
 * them whenever `world` divides 8 (1, 2, 4, 8 GPUs), else `world`; S = ceil(n / segments) rounded up to 128 columns each.
 * Rank r keeps the (segments / world) consecutive segments from r * (segments / world) on, i.e. the column block
 * [r*P, min(n, (r+1)*P)), P = S * segments / world -- `yTilde` is the caller's FULL row-major matrix, only the block is
 * uploaded (resp. generated).  All N-vector arguments of the calls below stay GLOBAL (n long) on every
 * rank; the library slices inputs and gathers outputs.  Every reduction over structures is formed per segment and the
 * segments' totals are added in segment order -- the SAME shape on every GPU count, a single GPU included: contexts of
 * 1, 2, 4 and 8 ranks return bit-identical results.  Across ranks a reduction is completed by one in-place all-gather
 * per stage through the peer-to-peer mailboxes (bioen_hip_p2p_attach), RCCL (bioen_hip_comm_init) or, for
 * processes that can share neither, a host callback.  Every rank must
 * issue the same calls in the same order.  Supported on sharded contexts: logw_weights, logw_fdf, chi_squared,
 * opt_lbfgs_logw(_batch), opt_gsl_logw, and the forces method (forces_weights, forces_fdf(_batch),
 * opt_lbfgs_forces(_batch), opt_gsl_forces) for every M served by strip copies (M <= 1024: two passes; beyond: four
 * passes over row panels).
 * The strip kernels serve M <= 16 x 1024 = 16384: at most 16 row panels.  Beyond that the streaming kernels on the
 * row-major matrix serve the context (the log-weights method, and the forces method on unsharded contexts only:
 * BIOEN_HIP_ESTATE on a sharded one), and the Hessian-vector products of the forces objective (bioen_hip_forces_hessp;
 * bioen_hip_forces_gram serves M <= 1024) are refused with BIOEN_HIP_ESTATE.
 * Minimum size: the LAST rank must still own a column, (world - 1) * P < n -- n > 512 for two ranks, > 768 for four,
 * > 896 for eight (S is at least 128); BIOEN_HIP_EINVAL ("too few structures to shard") on EVERY rank otherwise, so that
 * none waits in a collective for one that failed.  The leading dimension of the local data is segments-per-rank * S. */
int bioen_hip_ctx_create_sharded(int m, long long n, const double* yTilde, const double* YTilde,
                                 int device, int rank, int world, bioen_hip_ctx** ctx);
int bioen_hip_ctx_create_synthetic_sharded(int m, long long n, const double* YTrue,
                                           const double* sig_sim, const double* sig_exp,
                                           const double* YTilde, unsigned long long seed, int device,
                                           int rank, int world, bioen_hip_ctx** ctx);
/* host_buf = [world][count_per_rank] doubles; on entry this rank's segment is filled, on
 * return (0 = ok) all segments must be.  Called from the thread that called into the library. */
typedef int (*bioen_hip_exchange_fn)(void* user, double* host_buf, size_t count_per_rank);
int bioen_hip_ctx_set_exchange_callback(bioen_hip_ctx* ctx, bioen_hip_exchange_fn fn, void* user);
int bioen_hip_ctx_shard(const bioen_hip_ctx* ctx, int* rank, int* world, long long* n_global,
                        long long* col0, int* n_local);
/* Test hook for the stage exchanges: on an UNSHARDED context (world = 1) that has a communicator
 * (bioen_hip_comm_init(ctx, id, 0, 1)) or an exchange callback, every stage all-gather of the sharded
 * code path -- ybar + softmax totals, gradient dot products, Gram products; the forces method's two --
 * is executed although there is nobody to exchange with: a one-rank ncclAllGather on the context's stream,
 * between the same kernels as on 8 GPUs, leaving every bit of the result unchanged.  Also switched on by
 * BIOEN_HIP_FORCE_EXCHANGE=1 in the environment at context creation.  bioen_hip_exchange_counts tells how
 * many stage all-gathers went through RCCL / through the host callback so far. */
int bioen_hip_ctx_set_force_exchange(bioen_hip_ctx* ctx, int on);
/* Measurement aid: a MIRROR exchange.  A context created as rank r of `world` whose stage all-gathers copy ITS OWN part
 * into every other rank's part of the stage buffer -- one small kernel per exchange, no peer, no host.  The run is that of
 * a problem whose `world` column blocks are all equal to this rank's: numerically a valid problem, and kernel for kernel
 * the work ONE rank of a `world`-GPU run does per round, measured on a single GPU (bench.py, tools/engine_ab.py: the
 * per-rank share behind the multi-GPU projection).  Results are returned as for any sharded context (every block of
 * the gathered vectors equals this rank's). */
int bioen_hip_ctx_set_mirror_exchange(bioen_hip_ctx* ctx, int on);
int bioen_hip_exchange_counts(const bioen_hip_ctx* ctx, long long* rccl, long long* host_staged);
int bioen_hip_ctx_destroy(bioen_hip_ctx* ctx);
int bioen_hip_ctx_shape(const bioen_hip_ctx* ctx, int* m, int* n);
/* copy rows [row0,row0+rows) x cols [col0,col0+cols) of the resident matrix to host (row-major): the caller's
 * numbers bit for bit, whichever form of the matrix is resident */
int bioen_hip_ctx_read_ytilde(bioen_hip_ctx* ctx, int row0, int rows, int col0, int cols, double* out);
/* Which forms of the matrix are resident and what they occupy.  forms: bit 0 the row-major matrix (the form data
 * arrive in; the operand of the streaming kernels for M > 1024), bit 1 the strip-major copy in row-sum operand order,
 * bit 2 the one in column-sum operand order.  For M <= 1024 the strip copies hold the raw numbers and REPLACE the
 * row-major matrix once built: log-weights 2 x the matrix (bits 1 + 2; r06: 1 x, bit 1 alone, once a copy exceeds 1 GiB), forces method 1 x (bit 1; beyond 1024 rows,
 * where the copies are kept as row panels of <= 1024 rows, 2 x: both orders).  ONE copy (r05: bit 1 alone; log-weights at every M, and the forces method's row panels beyond 1024 rows): environment BIOEN_HIP_ONE_COPY=1 at context creation, or taken by itself when the second copy cannot
 * be allocated -- the adjoint then runs on the row-sum order copy (1-3 % slower per launch, same minima, last bits differ
 * from the two-copy default: the sums over rows are formed in another order). */
/* (bit 3: copies of the reduced-storage experiment, bioen_hip_ctx_set_storage, beside the FP64 row-major matrix) */
/* (bit 5: the device buffer of bioen_hip_forces_gram, from its first call on) */
/* (bit 6: the device buffer of bioen_hip_forces_colquad, from its first call on) */
int bioen_hip_ctx_footprint(const bioen_hip_ctx* ctx, int* forms, long long* bytes);
/* r06: HOW the strip copies are held.  one_copy: 1 = the log-weights adjoint runs on the row-sum order copy (asked for, or
 * taken by THIS rank because the second copy could not be allocated -- its last bits then differ from a two-copy rank's:
 * sharded drivers compare this value across ranks, bioen_amd/sweep.py).  interleave: the local segments' strips are stored
 * interleaved by this many in the row-sum order copy (1: strip order) -- the log-weights passes want the context's local
 * segment count (one contiguous window of the copy is read at any moment), the forces passes 1; the copy is moved when the
 * other method starts on the context (relayouts counts the moves; results never depend on the layout).
 * BIOEN_HIP_STRIP_INTERLEAVE=0: strip order always (A/B). */
int bioen_hip_ctx_layout(const bioen_hip_ctx* ctx, int* one_copy, int* interleave, int* relayouts);
/* Which regime of the strip passes' launch plan this context is in (read-only: what the launchers compute, no device
 * call).  pass 0: the log-weights forward pass, pass 1: the forces passes (gs = 0: they do not apply to this context).
 * Per column segment: its sps strips of 16 columns are dealt to gs groups (group g: strips g, g + gs, ...), so the
 * first sps - gs * (ceil(sps / gs) - 1) groups hold ceil(sps / gs) strips and the others one fewer.  tc: strips per chunk (forces passes: per
 * group and segment, the larger count), nch: chunks per group, fold: 1 = a slot runs a whole group and adds its chunks up
 * in registers, local_segments: the segments this context holds.
 * pass 2: the streaming pair on the row-major matrix (k_fwd_partial / k_adj: what serves a context without strip copies),
 * whether or not the context is on it at the moment -- sps: 128-column steps per segment, gs: column tiles per segment, tc:
 * steps per tile (a segment's last tile is cut at the segment's end), nch: rows a wave of the adjoint kernel walks, fold:
 * 1 = the passes use non-temporal loads, local_segments as above.
 * pass 3: the forces method's dense Gram passes (bioen_hip_forces_gram, _gram_bf16; M <= 1024) -- sps as above, gs: sets
 * per segment (set g chains the strips g, g + gs, ...), tc: the longest chain, ceil(sps / gs), nch: sets in all, fold: tile
 * pairs of 128 rows.  pass 4: the quadratic-form pass (bioen_hip_forces_colquad) -- sps: panels of 32 columns, gs: blocks
 * of the launch (block b runs the panels b, b + gs, ...), tc: the most panels a block runs, nch: the 64-row slices of a
 * strip (the kernel's NB), fold: the strips' padded rows.
 * Any result pointer may be NULL; another pass is BIOEN_HIP_EINVAL.  For tests that must prove a slot ran several strips
 * of a segment, or a tile several steps. */
int bioen_hip_ctx_strip_plan(const bioen_hip_ctx* ctx, int pass, int* sps, int* gs, int* tc, int* nch, int* fold,
                             int* local_segments);
/* r05: ask for (1) / give up (0) the ONE-copy form described above; to be called before the context's first gradient
 * evaluation (BIOEN_HIP_ESTATE once the column-sum order copy exists).  Beyond 1024 rows it serves both methods: one set
 * of row panels instead of two.
 * r06: without this call (and without BIOEN_HIP_ONE_COPY=0 / 1 in the environment) the form follows the matrix's size:
 * a strip copy of the WHOLE matrix (all ranks' columns) above 1 GiB is kept once -- the one-copy adjoint then runs at the
 * two-copy kernel's time (the headline: 8.2 GB resident instead of 16.4, the sweep within its run-to-run spread) --
 * smaller matrices keep the dedicated second copy, whose kernel is the faster one where launches are short. */
int bioen_hip_ctx_set_one_copy(bioen_hip_ctx* ctx, int on);
int bioen_hip_ctx_set_ytilde_target(bioen_hip_ctx* ctx, const double* YTilde);
/* Affine observable model: the optimizer sees yTilde_eff[i][j] = row_offset[i] + row_scale[i] * yTilde[i][j]
 * without the resident matrix being touched.  This is how DEER (modulation depth m:
 * yTilde = 1/sigma + m (F-1)/sigma, bioen/analyze/observables/observables.py:133-134) and SAXS
 * (scaling c: yTilde = c I/sigma, :141) nuisance parameters enter, so the refit loop of
 * bioen/analyze/procedure.py:79-83 needs no rebuild / re-upload of yTilde (the reference rebuilds it
 * on the host, observables.py:110-143).  row_offset = NULL means 0, row_scale = NULL means 1 (both m
 * long; one value per DEER trace / data set, repeated over its rows).  Both methods: the log-weights
 * evaluations and Hessian-vector products, and every forces entry (weights, fdf, fdf_batch, the L-BFGS and
 * GSL optimizers, sharded contexts included) -- there the forces enter the first pass as f_i row_scale_i
 * and the gradient leaves the device multiplied by row_scale_i; (0, 1) gives the plain model's bits.  Not
 * served: the forces method on the reduced-storage experiment's copies (BIOEN_HIP_ESTATE).
 * chi_squared() returns the raw yTilde . w and the chi^2 of the affine model. */
int bioen_hip_ctx_set_affine(bioen_hip_ctx* ctx, const double* row_offset, const double* row_scale);
/* EXPERIMENT, opt-in, never the default and never part of a headline number ("keep FP64 as the graded path;
 * treat FP32/BF16-split as an experiment"; 8 f4): the two matrix passes of the LOG-WEIGHTS evaluation stream copies
 * of the centred operand yTilde_ij - YTilde_i held in fewer bytes and reassembled to FP64 in registers in front of the
 * FP64 matrix-core products (all sums stay FP64):
 *   format 1: fp32 high part + bf16 residual, 6 bytes per element, |error| <= 2^-33 of the centred element;
 *   format 2: fp32, 4 bytes, 2^-25;       format 0: back to FP64 (8 bytes, exact).
 * The FP64 row-major matrix stays resident beside them (read-back, chi_squared).  M <= 1024.  The forces method's fused
 * strip passes (M <= 1024: forces_fdf(_batch), the forces optimizers) stream the same reduced copy; everything else of
 * the forces method (forces_weights, M > 1024) returns BIOEN_HIP_ESTATE while a reduced format is selected.  No reference counterpart: the reference computes in double
 * throughout (bioen/optimize/ext/c_bioen_common.c:70-108). */
int bioen_hip_ctx_set_storage(bioen_hip_ctx* ctx, int format);
/* How the L-BFGS direction d = -H g is formed on the device.
 *   1  two-loop recursion on the vectors, liblbfgs' order of operations (lbfgs.c:571-598):
 *      13 fused vector sweeps and 13 dependent reductions per direction;
 *   2  the same recursion carried out on coefficients over {S_0..5, Y_0..5, g} from their
 *      inner products: one sweep commits (s, y) and yields all 39 new products, one sweep forms
 *      d -- half the vector traffic and ONE reduction stage instead of 14 (what matters when
 *      every stage is an all-gather between GPUs).  Mathematically identical; rounding differs;
 *   0  auto (default): 2.  Measured on one MI355X, same process: N = 1e6 x M = 1024 8-theta series
 *      1.54 s vs 1.62-1.68 s; N = 1e5 x M = 256 single theta 176 vs 200 us per iteration. */
int bioen_hip_ctx_set_direction_mode(bioen_hip_ctx* ctx, int mode);
int bioen_hip_synchronize(bioen_hip_ctx* ctx);

/* ---- log-weights method ---------------------------------------------------- */
/* _get_weights, c_bioen_kernels_logw.c:55-94: w = softmax(g); *log_s = log sum exp(g) */
int bioen_hip_logw_weights(bioen_hip_ctx* ctx, const double* g, double* w, double* log_s);
/* interface_lbfgs_logw, c_bioen_kernels_logw.c:525-561 (= _get_weights +
 * _bioen_log_posterior_logw :131-147 + _grad_bioen_log_posterior_logw :151-268).
 * `f` and/or `grad` may be NULL (f-only skips the adjoint pass). */
int bioen_hip_logw_fdf(bioen_hip_ctx* ctx, const double* g, const double* G, double theta,
                       double* f, double* grad);
/* H(g) v for k <= 8 directions (v, hv: k x n, row-major).  g != NULL: evaluates the point first (as
   bioen_hip_logw_fdf with a gradient; f, grad optional outputs) and keeps it; g == NULL: the point kept by the
   last such call (G, theta ignored), BIOEN_HIP_ESTATE when it is gone.  k == 0 with g != NULL only sets the point. */
int bioen_hip_logw_hessp(bioen_hip_ctx* ctx, const double* g, const double* G, double theta, int k,
                         const double* v, double* hv, double* f, double* grad);
/* _opt_lbfgs_logw, c_bioen_kernels_logw.c:581-669, with the liblbfgs loop
 * (lbfgs.c:245-641) device-resident.  result[n] = optimal log-weights;
 * w_opt[n] (optional, may be NULL) = softmax(result).
 * Inputs are not validated (the reference validates nothing, c_bioen.pyx:274-290).  Non-finite ones end the run the way the
 * reference's binary -- liblbfgs built with -ffast-math -- ends it: NaN / inf in the start point, prior, matrix, targets
 * or theta: lbfgs_code 2, the start point, a non-finite fmin, after one evaluation; a direction whose slope is not a
 * number (a degenerate pair beyond the rounding floor) or positive: lbfgs_code -994 and the last accepted point with ITS
 * objective.  The same holds for the forces method and for every member of a batch on its own. */
int bioen_hip_opt_lbfgs_logw(bioen_hip_ctx* ctx, const double* g0, const double* G, double theta,
                             const bioen_lbfgs_config* config, const bioen_visual_params* visual,
                             double* result, double* w_opt, bioen_opt_result* info);

/* A whole theta series in one call.  Up to `max_batch` (<= 8) thetas advance in lock step --
 * one evaluation each per round -- and SHARE every pass over yTilde, so the matrix bytes per
 * theta drop by the batch width; finished thetas hand their slot to the next one.  Each theta
 * does exactly the arithmetic of a single run (results are bitwise identical to
 * bioen_hip_opt_lbfgs_logw called per theta).  This replaces the serial loop of
 * bioen/analyze/procedure.py:62-83 for cold-started series.
 *   thetas[ntheta]; g0: start log-weights, shared (g0_stride = 0) or per theta (stride >= n);
 *   results[ntheta][n]; w_opt[ntheta][n] or NULL; infos[ntheta].
 *   max_batch bounds the THETAS in flight.  Columns of the matrix passes that no theta occupies may carry speculative
 *   line-search trials of the thetas that are in flight (the steps a backtracking search asks for after a rejected trial;
 *   results are identical with and without them): up to 8 - max_batch on an unsharded context at the headline size, up to
 *   two on a structure-sharded context -- their N-vectors (seven per column) are allocated only where they can be used. */
int bioen_hip_opt_lbfgs_logw_batch(bioen_hip_ctx* ctx, int ntheta, const double* thetas,
                                   const double* g0, size_t g0_stride, const double* G,
                                   const bioen_lbfgs_config* config, const bioen_visual_params* visual,
                                   int max_batch, double* results, double* w_opt,
                                   bioen_opt_result* infos);

/* ---- forces method --------------------------------------------------------- */
/* _get_weights_from_forces, c_bioen_kernels_forces.c:111-224 */
int bioen_hip_forces_weights(bioen_hip_ctx* ctx, const double* forces, const double* w0, double* w);
/* interface_lbfgs_forces, c_bioen_kernels_forces.c:43-76 (= F1 + :227-277 + :280-340) */
int bioen_hip_forces_fdf(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta,
                         double* f, double* grad);
/* The same evaluation for K <= 8 force vectors at once (forces[K][m], thetas[K]; f[K], grad[K][m] or NULL):
 * the K problems share every pass over yTilde, each result equal to the last bit to the single call. */
int bioen_hip_forces_fdf_batch(bioen_hip_ctx* ctx, int k, const double* forces, const double* w0,
                               const double* thetas, double* f, double* grad);
/* _opt_lbfgs_forces, c_bioen_kernels_forces.c:574-662.  result[m] = optimal forces. */
int bioen_hip_opt_lbfgs_forces(bioen_hip_ctx* ctx, const double* forces0, const double* w0,
                               double theta, const bioen_lbfgs_config* config,
                               const bioen_visual_params* visual, double* result, double* w_opt,
                               bioen_opt_result* info);

/* theta series of the forces method in one call (cf. bioen_hip_opt_lbfgs_logw_batch): the M
 * variables of every problem stay on the host, the up to `max_batch` problems of a round share
 * all matrix passes of the evaluation (two for M <= 1024, else four).  forces0: shared (f0_stride = 0) or per theta
 * (stride >= m); results[ntheta][m]; w_opt[ntheta][n] or NULL. */
int bioen_hip_opt_lbfgs_forces_batch(bioen_hip_ctx* ctx, int ntheta, const double* thetas,
                                     const double* forces0, size_t f0_stride, const double* w0,
                                     const bioen_lbfgs_config* config, const bioen_visual_params* visual,
                                     int max_batch, double* results, double* w_opt,
                                     bioen_opt_result* infos);

/* ---- shared pieces --------------------------------------------------------- */
/* _bioen_chi_squared (c_bioen_common.c:70-108) / _getAve (c_bioen_kernels_forces.c:93-109):
 * yave[m] = yTilde . w ; *chi2 = 0.5 |yave - YTilde|^2.  Either output may be NULL.
 * With an affine row model set (bioen_hip_ctx_set_affine) chi2 is that of the EFFECTIVE observables
 * off_i + sc_i (yTilde . w)_i (sum w = 1 assumed, as everywhere in BioEn), while yave stays the RAW product
 * of the resident matrix -- the quantity a nuisance refit needs; bioen_hip_last_average hands out both. */
int bioen_hip_chi_squared(bioen_hip_ctx* ctx, const double* w, double* yave, double* chi2);
/* Averages left on the device by the most recent SINGLE-problem call (bioen_hip_chi_squared, bioen_hip_logw_fdf,
 * bioen_hip_forces_fdf, bioen_hip_opt_lbfgs_logw, bioen_hip_opt_lbfgs_forces, bioen_hip_opt_gsl_logw):
 * yraw[m] = yTilde . w of the resident matrix at the point that call ended on, yeff[m] = off + sc * yraw.  Either
 * may be NULL.  2 m doubles cross PCIe -- a refit between two optimizations (analyze/procedure.py:82-83) never moves
 * the N weights.  After a multi-problem call (*_batch with more than one problem) there is no single point to report:
 * BIOEN_HIP_ESTATE until the next single-problem call. */
int bioen_hip_last_average(bioen_hip_ctx* ctx, double* yraw, double* yeff);

/* ---- measurement hooks (bench.py) -------------------------------------------- */
/* Average device time (HIP events on the context's stream) and launch count of the
 * two matrix-streaming kernels since the last reset. which: 0 = forward, 1 = adjoint; 2 .. 5 = the four kernels
 * of bioen_hip_logw_hessp (dots, tangent, combine, epilogue). */
int bioen_hip_kernel_stats(bioen_hip_ctx* ctx, int which, double* total_ms, long long* launches);
/* as above, plus the sum over launches of the batch width (problems served per matrix pass) */
int bioen_hip_kernel_stats_ex(bioen_hip_ctx* ctx, int which, double* total_ms, long long* launches,
                              long long* problem_passes);
int bioen_hip_kernel_stats_reset(bioen_hip_ctx* ctx);
int bioen_hip_kernel_stats_enable(bioen_hip_ctx* ctx, int enable);

/* Line-search evaluations the log-weights batch engine issued speculatively in idle batch slots (the steps a
 * backtracking search asks for after a rejected trial, evaluated in the same matrix passes as the trial) and how
 * many of them it adopted, summed over the context's life.  BIOEN_HIP_SPECULATE=0 switches the mechanism off;
 * results are the same to the last bit either way. */
int bioen_hip_speculation_stats(bioen_hip_ctx* ctx, long long* issued, long long* adopted);

/* Diagnostic builds only (-DSTRIP_DIAG=4, tools/strip_probe.py): per-phase cycle sums of the last forces strip
 * launch, out[nblocks][16 waves][8 phases]; a normal build leaves the buffer untouched. */
int bioen_hip_debug_strip_stamps(bioen_hip_ctx* ctx, int enable, long long* out, int nblocks);

/* Measurement aid (tools/pass_probe.py): the two matrix passes of a log-weights evaluation alone --
 * `reps` launches each at batch width k (1..8) over whatever the problem slots hold -- mean milliseconds per launch,
 * HIP events on the context's stream.  Produces and changes no result. */
int bioen_hip_debug_pass_probe(bioen_hip_ctx* ctx, int k, int reps, double* fwd_ms, double* adj_ms);

/* ---- dense inverse-Hessian BFGS session (log-weights): the vector backend of bioen_amd/bfgs.py -------------------
 * scipy's fmin_bfgs (the reference's default minimizer) keeps H, the N x N inverse Hessian, as a host array and
 * updates it with two dense N x N products per iteration.  Here H lives in HBM (ld x ld FP64, ld = N rounded up to
 * 16) and is updated lazily in ONE streaming pass per iteration; the host driver keeps scipy's scalar decisions
 * (its own line searches) and only scalars cross PCIe per trial.  UNSHARDED contexts only (world > 1: ESTATE).
 *   begin   x = g0, objective and gradient at x, p = -g.  norm_inf: *gnorm = max |g| (else |g|_2); *gnorm2 = |g|_2;
 *           *dphi0 = g.p.  Memory check first: when ld^2 * 8 bytes plus the work vectors exceed hipMemGetInfo's free
 *           bytes it returns BIOEN_HIP_ENOMEM (message naming the N x N matrix) and allocates nothing.  A live session
 *           on the context is ended first.
 *   trial   *f = f(x + alpha p) (forward pass only); need_grad: also the adjoint at the same point, *dphi = g(alpha).p.
 *           The same alpha again reuses what is in place.
 *   accept  alpha must be the last trial, with its gradient: s = alpha p, x += s, y = g(alpha) - g, g = g(alpha);
 *           -> the driver's norm of the new g, |p|_2, |x|_2 (scipy's stopping tests).
 *   update  one pass over H (the previous step's rank-2 update + the row sums H [y, g]), the next direction
 *           p = -H' g and *dphi0 = g.p; *rho_fallback = 1 when y.s == 0 (rho = 1000, as scipy).
 *   end     optimum -> g_out, weights -> w_out (either may be NULL); info: fmin = f(x), chi2, kl, iterations = H passes.
 *           Frees H.
 * H is freed at _end, on every error of a bfgs call, and by bioen_hip_ctx_destroy; bioen_hip_ctx_footprint counts it
 * (forms bit 16) while the session is live.  Any other evaluation or optimiser call on the context (logw_*, forces_*,
 * opt_*, chi_squared) ends a live session: the session's next call returns BIOEN_HIP_ESTATE. */
int bioen_hip_bfgs_logw_begin(bioen_hip_ctx* ctx, const double* g0, const double* G, double theta, int norm_inf,
                              double* f0, double* gnorm, double* gnorm2, double* dphi0);
int bioen_hip_bfgs_logw_trial(bioen_hip_ctx* ctx, double alpha, int need_grad, double* f, double* dphi);
int bioen_hip_bfgs_logw_accept(bioen_hip_ctx* ctx, double alpha, int norm_inf, double* gnorm, double* pnorm,
                               double* xnorm);
int bioen_hip_bfgs_logw_update(bioen_hip_ctx* ctx, double* dphi0, int* rho_fallback);
int bioen_hip_bfgs_logw_end(bioen_hip_ctx* ctx, double* g_out, double* w_out, bioen_opt_result* info);
/* Debug / tests: rows [row0, row0 + rows) of the session's current H (the one whose product with g gave the current
 * direction; scipy's Bopt at the end) -> out (rows x N); padded = 1: the stored form, rows < ld and ld columns, pads
 * included (rows x ld); and a session vector -> out (N): which 0 = x, 1 = g, 2 = p,
 * 3 = the newest step s, 4 = the newest y, 5 = u = H y of the pending update. */
int bioen_hip_bfgs_logw_read_hinv(bioen_hip_ctx* ctx, int row0, int rows, int padded, double* out);
int bioen_hip_bfgs_logw_read_vec(bioen_hip_ctx* ctx, int which, double* out);

/* ---- host self-test of the L-BFGS driver (no GPU needed) ------------------------------
 * Runs the SAME driver + line-search code as the optimizers above on a built-in analytic
 * objective evaluated on the host: kind 0 = extended Rosenbrock, kind 1 = ill-conditioned
 * convex quadratic + quartic.  Lets the CPU test-suite pin the control flow
 * (lbfgs.c:245-641, 645-734, 812-1296) without a device. */
int bioen_hip_selftest_lbfgs(int kind, int n, const double* x0, const bioen_lbfgs_config* config,
                             double* x_out, bioen_opt_result* info);

/* Forces method on structure-sharded contexts: bioen_hip_forces_weights (one all-gather), bioen_hip_forces_fdf and the
 * forces optimizers (two all-gathers per evaluation) -- the two strip passes for M <= 1024, the four
 * passes over row panels beyond (r05: both in canonical segments, the bits of the single-GPU run).  Only the r01
 * streaming kernels (no strip copies: BIOEN_HIP_PANELS=0, BIOEN_HIP_STRIP_TALL=0, or a device without the memory for
 * them) remain unsharded-only: BIOEN_HIP_ESTATE there. */

/* ---- yTilde assembled on the device from raw observables ---------------------------------
 * Replaces the host loops of bioen/analyze/observables/observables.py:110-143 (sim / sigma built
 * element by element, structure by structure) and the host division: yTilde_ij = sim_ij / err_i,
 * YTilde_i = exp_i / err_i, divided on the device (true division: bitwise what numpy gives).
 *   structure_major = 0: sim is [m][n] (observables-major, like yTilde);
 *   structure_major = 1: sim is [n][m] -- each structure's (model's) M observables contiguous, the
 *     order in which simulated data arrive; uploaded in chunks and transposed on the device. */
int bioen_hip_ctx_create_raw(int m, long long n, int structure_major, const double* sim,
                             const double* exp_values, const double* exp_err, int device,
                             bioen_hip_ctx** ctx);

/* ---- GSL-style minimizers on the device objective -----------------------------------------
 * Replace _opt_bfgs_logw (c_bioen_kernels_logw.c:366-509) and _opt_bfgs_forces
 * (c_bioen_kernels_forces.c), i.e. gsl_multimin_fdfminimizer_{conjugate_fr, conjugate_pr,
 * vector_bfgs2, vector_bfgs, steepest_descent} (GSL 2.5) driven by the reference's loop with its
 * max-norm gradient test (c_bioen_common.c:112-138).  GSL is not linked: the five algorithms are
 * restated in bioen_amd/csrc/multimin.hpp.  Log-weights: variables, gradient and all work vectors
 * stay in HBM; forces: the M variables stay on the host.
 * info->lbfgs_code carries the GSL status: 0 success, -2 GSL_CONTINUE (iteration budget used),
 * 27 GSL_ENOPROG, 13 GSL_EBADTOL -- the reference treats {0, -2, 27} as success
 * (c_bioen.pyx:109-116).  info->iterations = driver iterations, info->evaluations = f + gradient
 * evaluations.  Sharded contexts (r05): served -- the minimizers' inner products and norms are sums over structures
 * like every other one (per canonical segment, one stage all-gather each), so every rank takes the same steps. */
const char* bioen_hip_gsl_strerror(int gsl_code);   /* replaces bioen_gsl_error(), c_bioen_error.c:14-20 */
int bioen_hip_opt_gsl_logw(bioen_hip_ctx* ctx, const double* g0, const double* G, double theta,
                           const bioen_gsl_config* config, const bioen_visual_params* visual,
                           double* result, double* w_opt, bioen_opt_result* info);
int bioen_hip_opt_gsl_forces(bioen_hip_ctx* ctx, const double* forces0, const double* w0, double theta,
                             const bioen_gsl_config* config, const bioen_visual_params* visual,
                             double* result, double* w_opt, bioen_opt_result* info);
/* GSL's own multimin test programme (multimin/test.c:106-160, test_funcs.c) on the SAME minimizer
 * code with host vectors, no GPU needed: kind 0 Roth, 1 Wood, 2 Rosenbrock, 3 SimpleAbs.
 * info->lbfgs_code = last status, info->reserved = gradient evaluations. */
int bioen_hip_selftest_multimin(int algorithm, int kind, const double* x0, double* x_out,
                                bioen_opt_result* info);

/* The same minimizer code on a host objective the CALLER supplies (host vectors, no GPU): run under the
 * reference's driver loop (c_bioen_kernels_logw.c:434-464) exactly as bioen_hip_opt_gsl_* are.
 * objective(user, x, &f, grad): grad == NULL asks for f alone (GSL's `f` callback), otherwise f and
 * the gradient (`df` / `fdf`); a non-zero return aborts the run.  The tests drive this with the
 * reference's own C objective to pin the minimizers against real GSL runs bit for bit. */
typedef int (*bioen_host_objective)(void* user, const double* x, double* f, double* grad);
int bioen_hip_multimin_host(int n, bioen_host_objective objective, void* user, const double* x0,
                            const bioen_gsl_config* config, double* x_out, bioen_opt_result* info);

/* ---- theta-sweep gather over RCCL (multi-GPU; one process per GPU) ----------------- */
/* rank 0 obtains the 128-byte ncclUniqueId; the host side ships it to the other ranks */
int bioen_hip_comm_unique_id(unsigned char id[128]);
int bioen_hip_comm_init(bioen_hip_ctx* ctx, const unsigned char id[128], int rank, int nranks);
/* all-gather of `count` doubles per rank, host in / host out (staged through HBM, RCCL over xGMI) */
int bioen_hip_comm_allgather(bioen_hip_ctx* ctx, const double* send, size_t count, double* recv);
/* != 0: a bioen_hip_comm_init was given up at its time bound (a rank never called it) and its helper thread is still
 * blocked inside ncclCommInitRank.  The process goes on without RCCL; it should leave through _exit (after flushing its
 * output) rather than through normal teardown, where the collective library's static destructors would run under that
 * thread.  Reset if the late peer shows up (the orphaned communicator is then aborted). */
int bioen_hip_comm_init_abandoned(void);
/* average wall time (microseconds) of one stage exchange of `count` doubles per rank on a sharded
 * context, back to back on the context's stream: lets the host decide whether splitting the
 * structures beats dealing thetas for a given problem size */
int bioen_hip_exchange_probe(bioen_hip_ctx* ctx, size_t count, int reps, double* usec_per_exchange);

/* Measurement aid (bench.py: roofline.read_ceiling): streams the resident form of the matrix `reps` times with a plain
 * read-only kernel (wide nontemporal loads, no LDS, no matrix cores) and reports the rate -- what this box's memory
 * system delivers to a read stream of exactly the bytes the matrix passes read.  form: 0 = whichever form is resident
 * (strip copy first), 1 / 2 / 4 = the form of that bioen_hip_ctx_footprint bit.  No reference counterpart. */
int bioen_hip_read_probe(bioen_hip_ctx* ctx, int form, int reps, double* gbytes_per_s, long long* bytes);
int bioen_hip_comm_destroy(bioen_hip_ctx* ctx);

/* ---- peer-to-peer stage exchange (r04): a third transport for the stage all-gathers of structure-sharded contexts,
 *      beside RCCL (bioen_hip_comm_init) and the host callback.  Every rank owns a mailbox in its HBM; the peers map
 *      it through hipIpc (xGMI between GPUs; between processes sharing ONE GPU too, which is how the single-GPU test
 *      box runs it) and an exchange is one small kernel on the context's stream: stores of this rank's segment into
 *      every peer's mailbox, a system-scope flag per peer, a bounded wait for the peers' flags -- no collective launch
 *      and no host.  No reference counterpart (bioen/analyze/procedure.py:62-63 is a serial loop in one process).
 *        1. every rank: bioen_hip_p2p_export(ctx, handle)           -- allocates the mailbox, returns its 64-byte hipIpc handle
 *        2. the host side all-gathers the handles (bioen_amd.sweep: SocketComm)
 *        3. every rank: bioen_hip_p2p_attach(ctx, handles[world][64]) -- maps the peers; from now on the exchanges of this
 *           context use this transport (it takes precedence over a communicator / callback that is also set)
 *      bioen_hip_p2p_detach unmaps and frees (also done by bioen_hip_ctx_destroy).  world = 1 with
 *      bioen_hip_ctx_set_force_exchange: attach(ctx, NULL) runs the (empty) exchange kernels all the same. */
int bioen_hip_p2p_export(bioen_hip_ctx* ctx, unsigned char handle[64]);
int bioen_hip_p2p_attach(bioen_hip_ctx* ctx, const unsigned char* handles);
int bioen_hip_p2p_detach(bioen_hip_ctx* ctx);
/* which transport the next stage exchange would use: 0 none (unsharded), 1 RCCL, 2 host callback, 3 peer-to-peer */
int bioen_hip_exchange_transport(const bioen_hip_ctx* ctx);
/* Self-test of whichever transport is active (sharded context, or world = 1 with forced exchanges): `reps` stage
 * exchanges of varying size queued back to back, each rank's segment a pattern of (rank, exchange, index), every segment
 * checked on the device after each exchange.  *mismatches = wrong doubles seen (0 = the transport delivers). */
int bioen_hip_exchange_selftest(bioen_hip_ctx* ctx, int reps, long long* mismatches);
int bioen_hip_exchange_counts3(const bioen_hip_ctx* ctx, long long* rccl, long long* host_staged, long long* p2p);
/* Every wait of the library on a round's results or on a peer is bounded: after `seconds` (default 60, environment
 * BIOEN_HIP_WAIT_TIMEOUT) without the awaited word the call returns BIOEN_HIP_ERCCL (a context that exchanges: a peer
 * is gone; an RCCL communicator is aborted with ncclCommAbort so that its kernel returns) or BIOEN_HIP_EHIP, with
 * bioen_hip_last_error() naming what was awaited.  The context is unusable afterwards (BIOEN_HIP_ESTATE): destroy it. */
int bioen_hip_ctx_set_wait_timeout(bioen_hip_ctx* ctx, double seconds);

/* ---- forces method: Hessian-vector products ------------------------------------------------------------------------ */
/* H(forces) v for k <= 8 directions of the forces objective L(f) = theta KL(w || w0) + 0.5 |ybar - YTilde|^2 (of the
 * affine model if bioen_hip_ctx_set_affine has set one); v, hv: k x m, row-major.  H is the exact Hessian: symmetric,
 * not positive definite away from the optimum.  No reference counterpart (the reference has first-order drivers only).
 *
 * forces != NULL (with w0): evaluates the point first -- bioen_hip_forces_fdf with a gradient, launch for launch: f and
 * grad (optional outputs) are its bits -- and keeps it on the context, at the cost of one column-sum pass more;
 * k == 0 then only sets the point.  forces == NULL: a product at the point kept by the last such call (w0, theta
 * ignored): two fused matrix passes, what a gradient costs, whatever k.
 *
 * A context keeps ONE point, of either method: this entry and bioen_hip_logw_hessp replace each other's, every call that
 * evaluates, optimises or changes the matrix state drops it (BIOEN_HIP_ESTATE from the next product, naming the call),
 * and a product on a point of the other method is BIOEN_HIP_ESTATE.  A call rejected for its arguments (BIOEN_HIP_EINVAL)
 * or refused for the context's state leaves point, BFGS session and device alone.
 *
 * Served: the FP64 strip copies, on any number of ranks (k directions in one call give the bits of k calls, one GPU the
 * bits of 2, 4 or 8) -- M <= 1024: two fused passes per product; M > 1024: two column-sum and two row-sum passes per row
 * panel, as the evaluation there, and setting the point costs no pass more.  Refused with BIOEN_HIP_ESTATE: contexts
 * without the strip copies (the streaming fallback), the reduced-storage experiment's copies.
 * bioen_hip_kernel_stats: which = 6 / 7 are the two fused passes of a product (M <= 1024). */
int bioen_hip_forces_hessp(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta, int k,
                           const double* v, double* hv, double* f, double* grad);

/* ---- forces method: the dense Hessian and the covariance of the observables in one pass over the matrix ------------ */
/* cov = C, the covariance of the observables under the weights of the point (= d ybar / d forces), and hess = H, the
 * exact Hessian of L(f) = theta KL(w || w0) + 0.5 |ybar - YTilde|^2 at it (of the affine model if
 * bioen_hip_ctx_set_affine has set one); both m x m, row-major, bitwise symmetric; either may be NULL.  With
 * a_j = A_:j - ybar and q_j = theta x_j + b_j:  C = sum_j w_j a_j a_j^T,  H = theta C + C C + sum_j w_j (q_j - qbar) a_j a_j^T
 * -- ONE compute-bound pass over the matrix on the FP64 matrix cores for both, where bioen_hip_forces_hessp needs
 * 2 ceil(m / 8) bandwidth-bound ones for H.  No reference counterpart.
 *
 * The point is bioen_hip_forces_hessp's.  forces != NULL (with w0): evaluates the point first -- bioen_hip_forces_fdf
 * with a gradient, launch for launch: f and grad (optional outputs) are its bits --, keeps it on the context and ends
 * a BFGS session.  forces == NULL: serves the kept forces point (w0, theta ignored), keeps point and session; refused
 * with BIOEN_HIP_ESTATE on a log-weights point or without a point.  A call rejected for its arguments
 * (BIOEN_HIP_EINVAL: forces without w0; nothing asked for) or refused for the context's state leaves point, session
 * and device alone.
 *
 * Two calls at one point give the same bits (fixed summation order, no atomics); a call that sets the point gives the
 * bits of a call that serves it.  Refused with BIOEN_HIP_ESTATE: m > 1024 (row panels), contexts without the strip
 * copies, the reduced-storage experiment's copies, structure-sharded contexts.  The device buffer of the partial
 * sums is allocated at the first call and freed with the context (bioen_hip_ctx_footprint: bit 5).  Its size is
 * O(sets x m^2) whatever n is -- sets = 8 segments x ceil(512 / (8 tiles)) groups, each holding the lower triangle's 64 x 64
 * sub-tiles of both matrices: 117 MB at m = 256, 139 MB at m = 512, 168 MB at m = 1024, 4 MB at m = 7 -- so a small
 * matrix does not make it small: callers that keep many small contexts should use bioen_hip_forces_hessp there. */
int bioen_hip_forces_gram(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta,
                          double* cov, double* hess, double* f, double* grad);

/* ---- forces method: one quadratic form per structure at a kept forces point, in one pass over the matrix ----------- */
/* out_j = a_j^T P a_j, j = 0 .. n - 1, with a_j = A_:j - ybar the j-th structure's observables (of the affine model if
 * bioen_hip_ctx_set_affine has set one: a_j = S (Y_:j - ybar), S = diag(scale)) centred on the averages under the
 * weights of the point, and P a symmetric m x m matrix, row-major.  Because d ln w_j / d forces = a_j:
 *   P = H^-1 (bioen_hip_forces_gram's H)  the Laplace variance of ln w_j around an optimum,
 *   P = C^-1                              the structure's Mahalanobis distance from the refined ensemble,
 *   P = I                                 its spread |a_j|^2.
 * ONE compute-bound pass over the matrix on the FP64 matrix cores (2 m^2 n flops), where the column sums of
 * bioen_hip_forces_hessp's passes would need ceil(m / 8) bandwidth-bound ones.  No reference counterpart.
 *
 * The point is bioen_hip_forces_hessp's, with bioen_hip_forces_gram's semantics.  forces != NULL (with w0): evaluates
 * the point first -- bioen_hip_forces_fdf with a gradient, launch for launch: f and grad (optional outputs) are its
 * bits --, keeps it on the context and ends a BFGS session; P == NULL then only sets the point (out is not written).
 * forces == NULL: serves the kept forces point (w0, theta ignored), keeps point and session; refused with
 * BIOEN_HIP_ESTATE on a log-weights point or without a point.  A call rejected for its arguments (BIOEN_HIP_EINVAL:
 * forces without w0; neither forces nor P; P without out; "P is not symmetric": |P_ij - P_ji| > 1e-12 max |P|) or
 * refused for the context's state leaves point, session and device alone.  Non-finite entries of P are the caller's
 * business.  What is computed is the form of the symmetric part (P + P^T) / 2.
 *
 * Two calls at one point give the same bits (every out_j has one writer, fixed summation order, no atomics).  Refused
 * with BIOEN_HIP_ESTATE: m > 1024 (row panels), contexts without the strip copies, the reduced-storage experiment's
 * copies, structure-sharded contexts.  The device buffer -- P padded to a multiple of 16 rows, and the n results -- is
 * allocated at the first call that computes and freed with the context (bioen_hip_ctx_footprint: bit 6). */
int bioen_hip_forces_colquad(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta,
                             const double* P, double* out, double* f, double* grad);

/* ---- forces method: the dense Hessian for a Newton minimizer, from split-BF16 operands on the BF16 matrix cores ---- */
/* cov = C~ and hess = H~: bioen_hip_forces_gram's C and H (above: the same formulas, arguments, layout
 * and point semantics) with the two M x M x N products formed from split-BF16 operands -- every operand is hi + lo, two
 * bfloat16 numbers, the products hi hi + hi lo + lo hi are accumulated in f32 -- at 32 x the matrix rate of FP64.
 * Everything else (the point, its weights, the row sums, the rank corrections, theta C + G2 + C C) stays FP64.  The
 * result is a MINIMIZER's Hessian, good to about 1e-5 .. 1e-4 of max|H|: it shapes a Newton step, whose gradient (f and
 * grad of this entry are bioen_hip_forces_fdf's bits) decides the optimum.  Error bars and anything else that needs C
 * or H themselves take them from bioen_hip_forces_gram, which this entry leaves bitwise alone.
 *
 * Both matrices are m x m, row-major, bitwise symmetric; either may be NULL.  forces != NULL (with w0): evaluates the
 * point first, keeps it on the context and ends a BFGS session.  forces == NULL: serves the kept forces point (w0,
 * theta ignored), keeps point and session; refused with BIOEN_HIP_ESTATE on a log-weights point or without a point.  A
 * call rejected for its arguments (BIOEN_HIP_EINVAL: forces without w0; nothing asked for) or refused for the
 * context's state leaves point, session and device alone.
 *
 * Two calls at one point give the same bits (fixed summation order, no atomics; the sets' f32 sums are added in FP64).
 * Refused with BIOEN_HIP_ESTATE: m > 1024 (row panels), contexts without the strip copies, the reduced-storage
 * experiment's copies, structure-sharded contexts.  The device buffer of the partial sums is this entry's own, of
 * bioen_hip_forces_gram's size, allocated at the first computing call and freed with the context
 * (bioen_hip_ctx_footprint: bit 7). */
int bioen_hip_forces_gram_bf16(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta,
                               double* cov, double* hess, double* f, double* grad);

/* ---- forces method: device-resident Newton minimizer -- the dense Hessian stays in device memory, is factorised
 *      (FP64 Cholesky) and solved there, and the loop runs behind one call.
 *
 * All three entries are refused with BIOEN_HIP_ESTATE, each case with a message of its own, where
 * bioen_hip_forces_gram_bf16 is: m > 1024 (row panels), contexts without the strip copies, the reduced-storage
 * experiment's copies, structure-sharded contexts. ---- */

/* A + lambda I = L L^T, L lower triangular, on the device (blocked, right-looking, panels of 64; the trailing update on
 * the FP64 matrix cores).  Only the lower triangle of the matrix is read.
 *   A != NULL: an m x m row-major host matrix (source is ignored).
 *   A == NULL: the Hessian of the kept forces point, computed now on the device and not downloaded -- source 0:
 *              bioen_hip_forces_gram's H, source 1: bioen_hip_forces_gram_bf16's.  Refused with BIOEN_HIP_ESTATE without
 *              a forces point.
 * *info (required) is LAPACK dpotrf's: 0 and L is complete, or k + 1 where pivot k was <= 0 or not finite -- an ordinary
 * result (the call returns 0), after which no kernel of the factorisation has touched the rest of the matrix.  L (may be
 * NULL): m x m row-major, zeros above the diagonal; written only when *info == 0.  The order of every sum is a function
 * of m alone: the same bits in give the same bits out.  Keeps point and session.  The device buffer of L is this
 * section's own, allocated at the first call and freed with the context (bioen_hip_ctx_footprint: bit 8). */
int bioen_hip_forces_newton_factor(bioen_hip_ctx* ctx, const double* A, int source, double lambda, double* L, int* info);

/* X = (L L^T)^-1 B with the factor of the last bioen_hip_forces_newton_factor call; B, X: [k][m], 1 <= k <= 8 (they may
 * be the same buffer).  A right-hand side's result does not depend on k.  BIOEN_HIP_ESTATE if there is no factor, or if
 * the last factorisation ended with info != 0.  Keeps point and session. */
int bioen_hip_forces_newton_solve(bioen_hip_ctx* ctx, int k, const double* B, double* X);

typedef struct {
    double gtol;            /* ends with status 0 when max |g_i| <= gtol */
    double armijo;          /* a step is accepted when f+ - f <= -armijo * pred                          (1e-4) */
    double rho_good;        /* lambda shrinks after a step with (f - f+) / pred above this               (0.75) */
    double lambda_factor;   /* lambda grows and shrinks by this factor                                   (4)    */
    double lambda_first;    /* the first lambda > 0, in units of d = max |diag H|                        (1e-10) */
    double lambda_max;      /* status 3 when lambda exceeds this many d                                  (1e10) */
    double lambda_zero;     /* a lambda below this many d becomes 0                                      (1e-12) */
    double floor_ulps;      /* pred <= floor_ulps * epsilon * |f|: f cannot judge the step, max |g| does  (8)    */
    int max_iterations;     /* accepted steps; status 1 when reached */
    int hessian;            /* 0: bioen_hip_forces_gram's H, 1: bioen_hip_forces_gram_bf16's */
} bioen_newton_config;

typedef struct {
    double fmin;            /* objective at the returned forces */
    double gmax;            /* max |g_i| there */
    double lambda;          /* the final damping */
    int status;             /* 0: max|g| <= gtol; 1: max_iterations; 2: at the minimum to the rounding of f (a step at the
                               rounding floor did not lower max|g|); 3: lambda grew beyond lambda_max * d */
    int iterations;         /* accepted steps */
    int evaluations;        /* evaluations of f and g (each two matrix passes and the point's one) */
    int hessians;           /* Hessian passes */
    int factorisations;
    int switched;           /* 1: the run began with hessian = 1 and went over to 0 at the rounding floor */
} bioen_newton_result;

/* Regularised Newton on the forces objective from forces0 [m] (DESIGN 6h has the loop; forces.py's
 * newton_bioen_log_posterior_base restates it in numpy, decision for decision): H at the kept point from `hessian`,
 * H + lambda I factorised and solved on the device -- only m doubles go down and m come up per step --, the trial
 * evaluated as bioen_hip_forces_hessp evaluates a point, so that an accepted trial is the kept point of the next Hessian.
 * forces_out [m] (required), weights_out [n] (may be NULL), result (required).  Returns 0 with every status; the
 * returned point is then the context's kept point (bioen_hip_forces_gram and bioen_hip_forces_colquad serve it at once).
 * Ends a BFGS session. */
int bioen_hip_opt_newton_forces(bioen_hip_ctx* ctx, const double* forces0, const double* w0, double theta,
                                const bioen_newton_config* config, double* forces_out, double* weights_out,
                                bioen_newton_result* result);

/* ---- forces method: Laplace error bars without leaving the device -- the dense Hessian
 * of bioen_hip_forces_gram is factorised where it stands (the kernels of bioen_hip_forces_newton_factor), inverted from
 * the factor, and the inverse is handed to the quadratic-form pass of bioen_hip_forces_colquad in device memory.  Only
 * what the caller asks for is downloaded: O(M + N) doubles per point for the error bars themselves.
 *
 * With H = L L^T and W = L^-1:
 *   cov_forces   = H^-1     = W^T W
 *   cov_averages = C H^-1 C = B^T B,  B = W C
 *   var_logw_j   = a_j^T H^-1 a_j
 *   logdet       = 2 sum_i ln L_ii
 * Both covariances are bitwise symmetric, and the same bits in give the same bits out.
 *
 * Both entries are refused with BIOEN_HIP_ESTATE, each case with a message of its own, where bioen_hip_forces_gram is:
 * m > 1024 (row panels), contexts without the strip copies, the reduced-storage experiment's copies, structure-sharded
 * contexts.  A rejected call leaves point, session and device alone.  The device buffers (W, H^-1, B, C H^-1 C) are this
 * section's own, allocated at the first call and freed with the context (bioen_hip_ctx_footprint: bit 9, value 512). ---- */

/* H^-1 of a caller's symmetric positive definite m x m row-major matrix A (only the lower triangle is read), or with
 * A == NULL of the Hessian (bioen_hip_forces_gram's, FP64) of the kept forces point (BIOEN_HIP_ESTATE without one).  The
 * factor becomes the context's factor: bioen_hip_forces_newton_solve afterwards solves with it.  Ainv (m x m) and logdet
 * may be NULL: the inverse stays resident.  *info (required) as LAPACK's dpotrf: 0, or k + 1 where pivot k was <= 0 or
 * not finite -- an ordinary result (the call returns 0) after which nothing is written, neither Ainv nor logdet nor the
 * resident inverse.  Keeps point and session. */
int bioen_laplace_forces_inverse(bioen_hip_ctx* ctx, const double* A, double* Ainv, double* logdet, int* info);

/* The error bars at a forces point.  With forces [m] (and w0 [n], theta) the point is evaluated and kept, as by
 * bioen_hip_forces_gram with forces: *f and grad [m] (either may be NULL) are bioen_hip_forces_fdf's bits, and a BFGS
 * session ends.  With forces == NULL the kept forces point is served (BIOEN_HIP_ESTATE without one; point and session
 * stay).  Every output may be NULL, and only what is asked for is computed and downloaded:
 *   std_forces [m], std_averages [m]      the roots of the covariances' diagonals (averages in the units of yTilde)
 *   var_logw [n]                          the Laplace variance of every ln w_j
 *   cov_forces, cov_averages [m x m]      row-major
 *   *logdet                               ln det H
 *   *min_pivot                            min_i L_ii^2: the caller judges definiteness against the scale of H
 * *info (required) as LAPACK's dpotrf; with *info != 0 the call returns 0 and writes nothing else (f and grad apart). */
int bioen_laplace_forces(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta, double* std_forces,
                         double* std_averages, double* var_logw, double* cov_forces, double* cov_averages, double* logdet,
                         double* min_pivot, int* info, double* f, double* grad);

/* ---- log-weights method: dual Newton minimizer -- the N log-weights through an M x M system that
 * is formed, factorised (FP64 Cholesky) and solved in device memory, and the covariance of the observables under the
 * refined weights it is built on.  DESIGN section 6j.
 *
 * Both entries are refused with BIOEN_HIP_ESTATE, each case with a message of its own, on m > 1024 (row panels; up to 4096
 * rows are served after bioen_hip_ctx_set_dense_panels, at the end of this header), on contexts
 * without the strip copies, on the reduced-storage experiment's copies and on structure-sharded contexts. ---- */

/* C = sum_j w_j (y_j - ybar)(y_j - ybar)^T, w = softmax(g): the covariance of the (affine model: effective) observables
 * under the weights of a log-weights point, m x m row-major, bitwise symmetric; the same bits call after call.
 *   g != NULL: an evaluation (bioen_hip_logw_hessp's with k = 0: the same f and grad, both optional) that leaves g as the
 *              context's kept log-weights point; G [n] is required then.  C may be NULL: the call only sets the point.
 *   g == NULL: serves the kept log-weights point (set by this entry, by bioen_hip_logw_hessp or by bioen_logwn_opt);
 *              BIOEN_HIP_ESTATE without one, naming what dropped it.  G, theta, f and grad are ignored.
 * The device buffer of the pass is this section's own, allocated at the first call that computes C and freed with the
 * context (bioen_hip_ctx_footprint: bit 10). */
int bioen_logwn_cov(bioen_hip_ctx* ctx, const double* g, const double* G, double theta, double* C, double* f, double* grad);

typedef struct {
    double gtol;            /* ends with status 0 when max |grad_k| <= gtol * max w_k (and max |gamma_k| <= theta) */
    double armijo;          /* a step alpha u is accepted when f+ - f <= armijo * alpha * grad . u                (1e-4) */
    double floor_ulps;      /* |alpha grad . u| <= floor_ulps * epsilon * |f|: f cannot judge the step, max |grad| does (8) */
    int max_iterations;     /* accepted steps; status 1 when reached */
    int max_halvings;       /* trials of one step, alpha = 1, 1/2, ...; status 3 when exhausted                   (60) */
} bioen_logwn_config;

typedef struct {
    double fmin;            /* objective at the returned log-weights */
    double gmax;            /* max |grad_k| there */
    double wmax;            /* max w_k there */
    int status;             /* 0: the gradient test; 1: max_iterations; 2: a step at the rounding floor of f did not lower
                               max |grad|; 3: the step was exhausted elsewhere (or C + theta I did not factorise) */
    int iterations;         /* accepted steps */
    int evaluations;        /* evaluations of f and grad (status 2, 3: one more than the trials, to restore the point) */
    int factorisations;
} bioen_logwn_result;

/* The dual Newton minimizer of the log-weights objective from g0 [n] with the prior G [n] (DESIGN 6j has the loop;
 * log_weights.py's dual_newton_bioen_log_posterior_base restates it in numpy, decision for decision): per iteration one
 * covariance pass, one factorisation of C + theta I and one solve on the device, one centred adjoint pass, and one
 * evaluation per trial; every N-vector stays in device memory.  theta > 0 is required (BIOEN_HIP_EINVAL otherwise: the step
 * divides by theta).  gopt [n] (required) is in the gauge the steps leave it in: compare weights, not g.  Returns 0 with
 * every status; the returned point is then the context's kept log-weights point (bioen_logwn_cov and bioen_hip_logw_hessp
 * without g serve it at once).  Ends a BFGS session. */
int bioen_logwn_opt(bioen_hip_ctx* ctx, const double* g0, const double* G, double theta, const bioen_logwn_config* config,
                    double* gopt, bioen_logwn_result* result);

/* ---- the theta series by dual Newton, and the covariance from split-BF16 operands.  DESIGN section 6k.  The refusals
 * (BIOEN_HIP_ESTATE) are the two entries' above. ---- */

/* bioen_logwn_cov's contract (arguments, point, buffer), C from the split-BF16 pass: the M x M x N product of operands split
 * hi + lo into bfloat16, hi hi + hi lo + lo hi on the BF16 matrix cores with float accumulators, the sets added in double.
 * |C_bf16 - C|_ik stays below 3 * 2^-16 sqrt(G'_ii G'_kk), G' the uncentred second moment: good for a Newton step, which
 * is what it is for.  f and grad are bioen_logwn_cov's bits; bitwise symmetric; the same bits call after call. */
int bioen_logwn_cov_bf16(bioen_hip_ctx* ctx, const double* g, const double* G, double theta, double* C, double* f, double* grad);

typedef struct {
    double fmin, gmax, wmax;        /* as in bioen_logwn_result */
    int status, iterations, evaluations, factorisations;
    int bf16_passes;                /* covariances formed by the split-BF16 pass (factorisations - bf16_passes: by the FP64 one) */
    int switched;                   /* 1: a step from a split-BF16 covariance was rejected at the rounding floor of f and the
                                       run went over to the FP64 pass for the rest of this theta (one more evaluation) */
} bioen_logwn_series_result;

/* The dual Newton minimizer for ntheta values of theta, in the order given, in one call: G goes up once, every N-vector
 * stays in device memory between the thetas, n doubles come down per theta (gopt: [ntheta][n], results: [ntheta]).
 *   source  0: the covariance of every step from the FP64 pass; 1: from the split-BF16 pass (bioen_logwn_cov_bf16's), with
 *           the switch above.  Gradient, stop test and Armijo test are FP64 either way: the optimum is the same.
 *   warm    1: theta k starts at the point theta k - 1 returned (theta 0 at g0); 0: every theta starts at g0.
 * With source 0 a warm series is, bit for bit and count for count, ntheta chained bioen_logwn_opt calls each starting at
 * the previous gopt; a cold one the ntheta single calls from g0.  A theta that ends with status != 0 does not stop the
 * series: every status is reported, and with warm = 1 the next theta starts from that theta's kept point.
 * BIOEN_HIP_EINVAL, before the device, the point or a session are touched, on NULL arguments, ntheta < 1, any theta <= 0 or
 * not finite, source or warm out of range, and a config bioen_logwn_opt refuses.  Returns 0 with every status; the last
 * theta's returned point is then the context's kept log-weights point.  Ends a BFGS session. */
int bioen_logwn_series(bioen_hip_ctx* ctx, const double* g0, const double* G, const double* thetas, int ntheta,
                       const bioen_logwn_config* config, int source, int warm, double* gopt,
                       bioen_logwn_series_result* results);

/* ---- log-weights method: Laplace error bars at a log-weights point, formed on the device.  DESIGN section 6l.  With
 * w = softmax(g), a_j = y_j - ybar, C = sum_j w_j a_j a_j^T (bioen_logwn_cov's) and P = (C + theta I)^-1, the
 * gauge-invariant quantities of the posterior's Gaussian approximation -- the Hessian theta (W - w w^T) + W Yc^T Yc W of
 * DESIGN 6j, which is the exact one at an optimum -- through the M x M system the dual Newton solves:
 *   leverage_j = w_j a_j^T P a_j, in [0, 1 - w_j)      var(ln w_j) = (1 - w_j - leverage_j) / (theta w_j)
 *   cov_averages = C P = I - theta P                   var(obar)   = (Var_w(o) - c^T P c) / theta, c = sum_j w_j (o_j - obar) a_j
 * The refusals (BIOEN_HIP_ESTATE) are bioen_logwn_cov's. ---- */

/* The error bars at a log-weights point.  The point is bioen_logwn_cov's: with g [n] (and G [n]) it is evaluated and kept
 * (*f and grad [n], either may be NULL, are bioen_hip_logw_fdf's bits; a BFGS session ends); with g == NULL the kept
 * log-weights point is served -- right after bioen_logwn_opt without a further evaluation -- (BIOEN_HIP_ESTATE without
 * one; point and session stay; G, f and grad are ignored).  theta is used as given in both cases.  Every output may be
 * NULL, and only what is asked for is computed and downloaded:
 *   std_averages [m], cov_averages [m x m]   the posterior covariance of the refined averages (units of yTilde; affine
 *                                            model: of the effective observables), bitwise symmetric, and the roots of
 *                                            its diagonal
 *   w [n], leverage [n]                      the weights; the share of structure j's prior log-weight variance the data removed
 *   var_logw [n], std_w [n]                  the variance of ln w_j and the standard deviation of w_j.
 *                                            An individual weight is poorly determined whenever theta w_j << 1 (std_w_j /
 *                                            w_j ~ 1 / sqrt(theta w_j)): the information is in the averages, above and below.
 *                                            Without any of these four the quadratic-form pass over the matrix does not run.
 *   observables [nobs][n], nobs <= 8         per-structure quantities that were NOT fitted (both or neither):
 *   obs_averages [nobs], var_observables [nobs]   their refined averages sum_j w_j o_j and the variances of those
 *   *logdet, *min_pivot                      ln det (C + theta I); min_i L_ii^2 of its Cholesky factor
 * *info (required) as LAPACK's dpotrf: 0, or k + 1 where pivot k was <= 0 or not finite (a point that is not finite);
 * with *info != 0 the call returns 0 and writes nothing else (f and grad apart).  BIOEN_HIP_EINVAL, before the device, the
 * point or a session are touched: theta <= 0 or not finite, nobs outside 0 .. 8, observables without nobs or the reverse,
 * g without G.  The factor becomes the context's factor.  The same bits in give the same bits out; k observables in one
 * call give the bits of k calls.  The device buffers are those of bioen_logwn_cov, the Newton entries,
 * bioen_laplace_forces and bioen_hip_forces_colquad (bioen_hip_ctx_footprint: bits 10, 8, 9, 6). */
int bioen_logwn_laplace(bioen_hip_ctx* ctx, const double* g, const double* G, double theta, const double* observables, int nobs,
                        double* std_averages, double* cov_averages, double* w, double* leverage, double* var_logw,
                        double* std_w, double* obs_averages, double* var_observables, double* logdet, double* min_pivot,
                        int* info, double* f, double* grad);

/* ---- log-weights method: the dual Newton theta series with nuisance scales profiled out (DEER modulation depths, the
 * scattering scale factor).  DESIGN section 6m.  The model is the affine one, off_i + sigma_i (Y w)_i, with ONE scale per
 * group of rows, sigma_i = s_group[i] (group -1: the row's scale stays 1), and the scales are a function of the point:
 *   s_k = sum_{i in k} ybar_i (YTilde_i - off_i) / sum_{i in k} ybar_i^2,  ybar = Y w the raw averages,
 * the least-squares refit of bioen_amd.nuisance.refit_scales, formed inside every evaluation.  The minimizer is
 * bioen_logwn_series's loop on the profile objective theta KL + 1/2 |off + sigma o ybar - YTilde|^2: its gradient is the
 * affine model's at row_scale = sigma, its step solves (Pi C_A Pi + theta I) z = -Pi b_A with Pi the projector that removes
 * the groups' normalised ybar.  One run replaces the alternation optimise / refit of the reference's protocol. ---- */

/* source, warm, config, gopt [ntheta][n], results [ntheta], the statuses and the refusals (BIOEN_HIP_ESTATE) are
 * bioen_logwn_series's.  row_offset [m] (NULL: zeros), group [m] with values in -1 .. ngroups - 1, 1 <= ngroups <= 64, every
 * group with at least one row.  scales [ntheta][ngroups] (required): the scales at each theta's returned point; chi2,
 * kl [ntheta] (either may be NULL): 1/2 sum r^2 (bioen_opt_result's chi2) and KL(w || w0) there.  There are no start values for the scales.  A group
 * whose sum ybar^2 is 0 or not finite makes f not finite: such a trial is rejected, at the start point the run ends with
 * status 3.  BIOEN_HIP_EINVAL, before the device, the point, the model or a session are touched: NULL arguments, ntheta <
 * 1, any theta <= 0 or not finite, ngroups outside 1 .. 64, a group id outside -1 .. ngroups - 1, an empty group, source or
 * warm out of range, a config bioen_logwn_opt refuses.  Returns 0 with every status; then the context's affine model
 * (bioen_hip_ctx_set_affine's) is (row_offset, sigma of the last theta's returned point), and that point is the kept
 * log-weights point: bioen_hip_logw_hessp, bioen_logwn_cov and bioen_logwn_laplace without g serve it at those FIXED
 * scales.  Ends a BFGS session.  The device buffer of the scales and the projection is this section's own, allocated at
 * the first call and freed with the context (bioen_hip_ctx_footprint: bit 11, value 2048). */
int bioen_logwn_profile_series(bioen_hip_ctx* ctx, const double* g0, const double* G, const double* thetas, int ntheta,
                               const bioen_logwn_config* config, int source, int warm, const double* row_offset,
                               const int* group, int ngroups, double* gopt, double* scales, double* chi2, double* kl,
                               bioen_logwn_series_result* results);

/* ---- log-weights method: the dual Newton beyond 1024 observables, over the row panels of the matrix.  DESIGN section 6n.
 * A setting of the context, off by default: with it, bioen_logwn_cov, bioen_logwn_cov_bf16, bioen_logwn_opt and
 * bioen_logwn_series serve 1024 < m <= 4096 on contexts whose row panels' strip copies are resident (not BIOEN_HIP_PANELS=0,
 * not the streaming fallback); beyond 4096 rows they answer BIOEN_HIP_ESTATE, naming 4096.  Every other dense entry
 * (bioen_logwn_laplace, bioen_logwn_profile_series, the forces method's), structure-sharded contexts and the
 * reduced-storage copies are refused in their present words, setting or not.  m <= 1024 is served as before either way.
 * The pass's buffer grows with m^2: (sets + 1) x (m / 64)(m / 64 + 1) / 2 sub-tiles of 32 KiB (sets: the context's
 * canonical segments, 8 unless BIOEN_HIP_SEGMENTS says otherwise, x their groups) -- 68 MB a set at 4096 rows, 0.6 GB in
 * all -- plus C; the factor's buffer holds 2 m^2 doubles (bioen_hip_ctx_footprint: bits 10 and 8).
 * on: 0 or 1 (BIOEN_HIP_EINVAL otherwise).  Keeps the point and a session; no device work. ---- */
int bioen_hip_ctx_set_dense_panels(bioen_hip_ctx* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif /* BIOEN_HIP_H */
