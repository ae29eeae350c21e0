/*
 * gpmpc.h -- C-ABI of libgpmpc_hip.so, the MI355X (gfx950) GP + QP hot path.
 *
 * The reference (shiivashaakeri/gp-mpc-rocket-landing) is pure Python: its
 * "boundary" for this path is a set of duck-typed classes whose heavy lifting
 * is numpy/LAPACK and the third-party OSQP C solver.  Each entry point below
 * replaces one of those native calls; the Python mirror in
 * gp_mpc_rocket_landing_amd/ binds them with ctypes.
 *
 * Conventions
 *   - every function returns int: 0 = ok, >0 = LAPACK-style info (e.g. the
 *     1-based column of the first non-positive pivot), <0 = argument / HIP
 *     error (gpmpc_last_error() has the message).  Nothing throws.
 *   - all arithmetic is fp64; host buffers are caller-owned, row-major, with
 *     explicit leading dimensions.  Functions suffixed _dev take device
 *     pointers that must stay resident for the call.
 *   - one gpmpc_ctx per process/rank owns one HIP stream; a ctx is not
 *     thread-safe.
 */
#ifndef GPMPC_H
#define GPMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: gpmpc_fleet_config gained sqp_iters / sqp_tol (round 2) and
 * gpmpc_rollout6_config the GPMPC problem data (round 3);
 * 3: gpmpc_rollout6_config gained the rocket parameters and horizon 20 or 30,
 * gpmpc_rollout6_solve_ref (X_ref / U_ref), gpmpc_comm_count (round 4); round 4 also
 * gave gpmpc_fleet_config.sqp_qp the max_iter = 0 "same as qp" meaning.  Round 5 adds
 * entry points only (gpmpc_fleet_get_posterior, gpmpc_gather_prepare / _collective) and
 * refuses a fleet config whose sqp_qp was edited with max_iter left 0.
 * 4 (round 6): gpmpc_rollout6_config gained rocket_J (the full inertia tensor); new
 * entry points gpmpc_fleet_create_shard, gpmpc_fleet_create_fitc. */
#define GPMPC_ABI_VERSION 4

typedef struct gpmpc_ctx gpmpc_ctx;
typedef struct gpmpc_gp gpmpc_gp;
typedef struct gpmpc_knn gpmpc_knn;
typedef struct gpmpc_fitc gpmpc_fitc;
typedef struct gpmpc_fleet gpmpc_fleet;

/* kernel kinds: kernels.py:130 (SE-ARD), :392 (isotropic SE), :482 (Matern32), :579 (Matern52) */
enum { GPMPC_SE_ARD = 0, GPMPC_SE_ISO = 1, GPMPC_MATERN32 = 2, GPMPC_MATERN52 = 3 };

/* Composite kernels (kernels.py:676-844: SumKernel, ProductKernel, WhiteNoise) as a
 * postfix program: nops pairs (code, offset into par).  Leaves: the four kinds above
 * (par[off] = sigma2, then the d lengthscales; SE_ISO: sigma2, l) and GPMPC_KP_WHITE
 * (par[off] = its noise variance: on the diagonal of a Gram of one row set, zero
 * between two sets, kernels.py:805-815).  GPMPC_KP_SUM / _PROD combine the two values
 * on top of the stack.  E.g. SumKernel(SE_ARD(d), WhiteNoise(s)): ops = {0,0, 4,d+1, 10,0},
 * par = {sigma2, l_0..l_{d-1}, s}.  At most GPMPC_KP_MAXOPS pairs, stack depth 8. */
enum { GPMPC_KP_WHITE = 4, GPMPC_KP_SUM = 10, GPMPC_KP_PROD = 11 };
#define GPMPC_KP_MAXOPS 64
#define GPMPC_KP_MAXSTACK 8

/* OSQP-style status values (OSQP 0.6 constants.h), reported by the ADMM. */
enum {
  GPMPC_QP_SOLVED = 1, GPMPC_QP_SOLVED_INACCURATE = 2, GPMPC_QP_MAX_ITER_REACHED = -2,
  GPMPC_QP_PRIMAL_INFEASIBLE = -3, GPMPC_QP_PRIMAL_INFEASIBLE_INACCURATE = 3,
  GPMPC_QP_DUAL_INFEASIBLE = -4, GPMPC_QP_DUAL_INFEASIBLE_INACCURATE = 4,
  GPMPC_QP_NON_CVX = -7, GPMPC_QP_UNSOLVED = -10
};

int gpmpc_abi_version(void);
const char *gpmpc_last_error(void);

/* ---- context ---------------------------------------------------------- */
int gpmpc_ctx_create(int device, gpmpc_ctx **out);
int gpmpc_ctx_destroy(gpmpc_ctx *ctx);
int gpmpc_ctx_sync(gpmpc_ctx *ctx);
/* the HIP stream the context launches on (hipStream_t as void*) */
void *gpmpc_ctx_stream(gpmpc_ctx *ctx);

/* ---- a2/a3: kernel Gram matrix -----------------------------------------
 * Replaces SquaredExponentialARD.__call__ / Matern32/52.__call__ /
 * SquaredExponential.__call__ (kernels.py:238-262, :532-545, :625-637,
 * :417-432): K[i,j] = k(X1[i], X2[j]).  X2 == NULL means X2 = X1.
 * ls: d lengthscales (SE_ISO reads ls[0]). */
int gpmpc_gram(gpmpc_ctx *ctx, int kind, const double *X1, int n1, const double *X2, int n2,
               int d, const double *ls, double sigma2, double *K, int ldk);
/* Hyperparameter gradients of the Gram, d K / d(log theta)
 * (SquaredExponentialARD.gradients kernels.py:279-318: K (x1_i - x2_i)^2 / l_i^2
 * for every input dimension i; SquaredExponential.gradients :438-456:
 * K r^2 / l^2).  kind SE_ARD writes d matrices, SE_ISO one, each n1 x n2
 * row-major, stacked in G; K (n1 x n2) is written too unless NULL.  The
 * log-signal-variance gradient is K itself (and the only one the reference's
 * Matern kernels define). */
int gpmpc_gram_grad(gpmpc_ctx *ctx, int kind, const double *X1, int n1, const double *X2, int n2,
                    int d, const double *ls, double sigma2, double *K, double *G);
/* diagnostic (tests only), no device: the kernel the Gram launcher takes for n1 rows of d
 * features under this process's GPMPC_GRAM_ROWS (the launcher itself branches on this
 * value).  Returns D, the width k_gram is instantiated for (11, 12, 13, or 0: the
 * instantiation that reads the width at run time), or GPMPC_GRAM_PATH_ROWS | D for the
 * row-tiled k_gram_rows<D>; transpose_out != 0 always takes k_gram.  -2 for d outside
 * 1..32 or n1 < 0. */
enum { GPMPC_GRAM_PATH_ROWS = 64 };
int gpmpc_gram_path(int n1, int d, int transpose_out);

/* ---- Cholesky factor / solve -------------------------------------------
 * Replaces np.linalg.cholesky (exact_gp.py:164,170; sparse_gp.py:187,205).
 * In place on the lower triangle; info = 1-based first non-positive pivot
 * (returned as well).  info = -1: the factor kernel's bounded internal wait
 * expired (a broken invariant, factor unreliable); the call then returns -1
 * with gpmpc_last_error naming it. */
int gpmpc_potrf(gpmpc_ctx *ctx, int n, double *A, int lda, int *info);
/* batch x (n x n) SPD matrices, device-resident, stride elements apart;
 * dinfo: device int[batch], with gpmpc_potrf's meaning per matrix (the caller
 * reads it; -1 marks an unreliable factor). */
int gpmpc_potrf_batched_dev(gpmpc_ctx *ctx, int n, int batch, double *dA, int lda, int64_t stride,
                            int *dinfo);
/* C = alpha A A^T + beta C on the lower triangle (dsyrk 'L','N') for batch
 * device matrices: A (n x k, lda), C (n x n, ldc); the trailing update of the
 * blocked potrf (FP64 MFMA). */
int gpmpc_syrk_batched_dev(gpmpc_ctx *ctx, int n, int k, int batch, const double *dA, int lda,
                           int64_t strideA, double *dC, int ldc, int64_t strideC, double alpha,
                           double beta);
/* Replaces scipy.linalg.solve_triangular(L, B, lower=True) (exact_gp.py:251,260;
 * sparse_gp.py:190,293,296): B (n x nrhs) overwritten by L^-1 B. */
int gpmpc_trsm_lower(gpmpc_ctx *ctx, int n, int nrhs, const double *L, int ldl, double *B, int ldb);
/* Replaces scipy.linalg.cho_solve((L, True), B) (exact_gp.py:179; sparse_gp.py:210,214). */
int gpmpc_potrs(gpmpc_ctx *ctx, int n, int nrhs, const double *L, int ldl, double *B, int ldb);
/* diagnostic (tests only; no product path calls it): one launcher of the internal FP64
 * MFMA GEMM family (csrc/gemm.h) on device pointers, so that every kernel of the family
 * can be compared with an exact reference.  All matrices row-major, batch members
 * sA / sB / sC elements apart.  Per op (unused arguments are ignored):
 *   NT          C = alpha A (M x K) B (N x K)^T + beta C; flags TRI_A (A lower triangular,
 *               K <= M, beta != 1), LOWER_C (only C[i][j], j <= i, is written)
 *   NN / NN_BATCHED  B is K x N;   TN  A is K x M, B is K x N  (NN, TN: batch 1)
 *   ROWBLOCK    the NT product with N <= 128 (C may alias A); LOWER_C, p0 = K split
 *               (> 1 only with beta = 1)
 *   LAT0        the NT product with N <= 128, K <= 128 (C may alias A); TRI_B
 *   LAT1        lower C = alpha A A^T + beta C, M = N, K <= 128 (B unused)
 *   SYRK_DIAG   lower C (M x M, M <= 128, ld lda, stride sA) -= A (M x K) A^T, p0 = K split
 *   UPDSOLVE    C (M x 128, ld lda) <- (C - A (M x K) B (128 x K)^T) Linv^T, Linv = D
 *               (128 x 128 lower, stride ldd), batch a multiple of 8, B at stride sA;
 *               p0 = wn (<= 128, <= M; > 0 needs C = A + K): also the lower wn x wn block
 *               at C + 128 -= A[0:wn, 0:K+128] A[0:wn, 0:K+128]^T
 *   SUMSQ       A (n x n lower, ld n; n = M = K), Ks = B (P x n, ld n; P = N): part = C
 *               (ld ldc), row t = the column sums of squares of (A Ks^T) over row tile t;
 *               p0 = forced kind (-1 the launcher's choice, 0 64-row tiles, 1 128-row
 *               tiles, 2 the K split, which keeps 64-row tiles)
 *   SUMSQ_MEAN  the same with A = [W; alpha^T] ((n + p1) x n): rows n.. of the product go
 *               to D (p1 x P, ld ldd)
 * A combination outside the launcher's contract returns -2 and launches nothing; the
 * caller answers for the extents of its buffers.  path[0] = the kernel path taken
 * (GPMPC_GEMM_PATH_*, -1 when the product is empty), path[1] = its K split (chunks of the
 * split forms, workgroups of stream-K; 1 otherwise), path[2] = the grid mapping. */
enum { GPMPC_GEMM_OP_NT = 0, GPMPC_GEMM_OP_NN = 1, GPMPC_GEMM_OP_NN_BATCHED = 2, GPMPC_GEMM_OP_TN = 3,
       GPMPC_GEMM_OP_ROWBLOCK = 4, GPMPC_GEMM_OP_LAT0 = 5, GPMPC_GEMM_OP_LAT1 = 6, GPMPC_GEMM_OP_SYRK_DIAG = 7,
       GPMPC_GEMM_OP_UPDSOLVE = 8, GPMPC_GEMM_OP_SUMSQ = 9, GPMPC_GEMM_OP_SUMSQ_MEAN = 10 };
enum { GPMPC_GEMM_TRI_A = 1, GPMPC_GEMM_LOWER_C = 2, GPMPC_GEMM_TRI_B = 4 };
enum { GPMPC_GEMM_PATH_64 = 0, GPMPC_GEMM_PATH_128 = 1, GPMPC_GEMM_PATH_128_KSPLIT = 2,
       GPMPC_GEMM_PATH_STREAMK = 3, GPMPC_GEMM_PATH_SPLITK = 4, GPMPC_GEMM_PATH_LAT = 5,
       GPMPC_GEMM_PATH_SYRK_DIAG = 6, GPMPC_GEMM_PATH_UPDSOLVE = 7 };
enum { GPMPC_GEMM_GRID_2D = 0, GPMPC_GEMM_GRID_TRI = 1, GPMPC_GEMM_GRID_XCD_BATCH = 2,
       GPMPC_GEMM_GRID_ROWBLOCK_XCD = 3 };
int gpmpc_gemm_diag(gpmpc_ctx *ctx, int op, int M, int N, int K, int batch, const double *A, int64_t lda,
                    int64_t sA, const double *B, int64_t ldb, int64_t sB, double *C, int64_t ldc, int64_t sC,
                    double *D, int64_t ldd, double alpha, double beta, int flags, int p0, int p1, int *path);
/* diagnostic (tests only), no device: the rows of the SUMSQ partial buffer that the
 * posterior's consumers sum for an M x N x K product, and in *kind (may be NULL) the kernel
 * the launcher picks for it (0 64-row tiles, 1 128-row tiles, 2 the K split, 64-row tiles),
 * both under this process's GPMPC_GEMM128 / GPMPC_GEMM128_KMIN / GPMPC_SPLITK. */
int gpmpc_gemm_row_tiles(int M, int N, int K, int *kind);
/* diagnostic (tests only): what the launcher of op would do for the product, without
 * touching a device (no context) -- the plan the launchers execute (csrc/gemm_plan.h).  op,
 * flags, p0, p1 as for gpmpc_gemm_diag; only the ops with a decision: NT, NN, NN_BATCHED,
 * TN, ROWBLOCK, SUMSQ, SUMSQ_MEAN (any other, or arguments gpmpc_gemm_diag refuses: -2).
 * flags may add GPMPC_GEMM_NO_SCRATCH: the plan a launcher falls back to when the split-K
 * partial buffer is not to be had.
 * policy: NULL = this process's switches; else GPMPC_GEMM_POLICY_N ints in the order big,
 * kmin, splitk, syrk128, streamk, ksplit, remap, xcd_batch, rowblock_xcd, post_xcd
 * (GemmPolicy: the GPMPC_* switch of each and its default).  plan receives
 * GPMPC_GEMM_PLAN_INTS ints: the path, split and grid gpmpc_gemm_diag reports (path -1: an
 * empty product), the launch grid gx, gy, gz (of the split forms: of the partial products),
 * the tile height (64 or 128) and the chunk length of the skinny K splits (else 0). */
enum { GPMPC_GEMM_NO_SCRATCH = 8 };
#define GPMPC_GEMM_POLICY_N 10
#define GPMPC_GEMM_PLAN_INTS 8
int gpmpc_gemm_plan(int op, int M, int N, int K, int batch, double beta, int flags, int p0, int p1,
                    const int *policy, int *plan);
/* diagnostic (tests only): the launches gpmpc_potrf_batched_dev would make for (n, batch),
 * without touching a device (no context).
 * policy: NULL = this process's switches; else GPMPC_POTRF_POLICY_N ints in the order p128,
 * persist, lat, sweep, trsm, pk, ob, ksplit, fuse, la, syrk_diag, fuse_min, stamps
 * (csrc/potrf_plan.h PotrfPolicy: the GPMPC_* switch of each and its "auto" value), so a
 * test sets a switch without mutating the environment of a process that has already cached
 * it.  form: 0 = 32-column, 1 = persistent, 2 =
 * 128-column (steps filled only for 2).  Each step is GPMPC_POTRF_STEP_INTS ints: kind
 * (GPMPC_POTRF_*), c (its first column; of a TRAIL_*, the first trailing column), K0 (the
 * outer panel's first column) and four operands:
 *   DIAG            w, packed layout, mode = sweep | (TRSM-form blocks ? 2 : 0), Linv written
 *   UPD_SYRK_DIAG   w, K, ks            UPD_ROWBLOCK   rows, w, K, ks
 *   UPDSOLVE        below, K, wn        PSOLVE_*       rows
 *   TRAIL_*         M, K
 * Returns the number of steps (may exceed cap; only cap are written), or -2 for a refused
 * argument. */
#define GPMPC_POTRF_POLICY_N 13
#define GPMPC_POTRF_STEP_INTS 7
enum { GPMPC_POTRF_DIAG = 0, GPMPC_POTRF_UPD_SYRK_DIAG = 1, GPMPC_POTRF_UPD_ROWBLOCK = 2, GPMPC_POTRF_UPDSOLVE = 3,
       GPMPC_POTRF_PSOLVE_TRSM = 4, GPMPC_POTRF_PSOLVE_LAT = 5, GPMPC_POTRF_PSOLVE_ROWBLOCK = 6,
       GPMPC_POTRF_TRAIL_LAT = 7, GPMPC_POTRF_TRAIL_SYRK = 8 };
int gpmpc_potrf_plan(int n, int batch, const int *policy, int *form, int *steps, int cap);
/* diagnostic (tests only): gpmpc_potrf_batched_dev under an explicit policy (as for
 * gpmpc_potrf_plan: NULL = this process's switches), so that every form and switch runs in
 * one process.  A policy gpmpc_potrf_plan refuses, or batch > 1 members that overlap
 * (stride < (n - 1) lda + n), returns -2 and launches nothing. */
int gpmpc_potrf_diag(gpmpc_ctx *ctx, int n, int batch, double *dA, int lda, int64_t stride, int *dinfo,
                     const int *policy);
/* diagnostic (tests only): one triangular launcher or solve helper on device pointers (row-
 * major, L n x n lower at ld ldl, X n x nrhs at ld ldx, overwritten):
 *   TRSM           X <- L^-1 X, or L^-T X under GPMPC_TRI_TRANS; GPMPC_TRI_RHS_LOWER (forward
 *                  only): X is lower triangular (zero above its diagonal), which the walk uses
 *   TRI_INVERSE    X <- L^-1 by the doubling inverse; X preset to the identity, nrhs = n
 *   CHO_SOLVE_INV  X <- (L L^T)^-1 X through W = L^-1 (dW, ld n) with one refinement step;
 *                  nrhs <= 16, ldl = n, ldx = nrhs
 *   POTRS_COLS     X <- (L L^T)^-1 X by the per-column substitution kernel; ldx = nrhs
 * Arguments outside a launcher's contract return -2 and launch nothing. */
enum { GPMPC_TRI_OP_TRSM = 0, GPMPC_TRI_OP_TRI_INVERSE = 1, GPMPC_TRI_OP_CHO_SOLVE_INV = 2,
       GPMPC_TRI_OP_POTRS_COLS = 3 };
enum { GPMPC_TRI_TRANS = 1, GPMPC_TRI_RHS_LOWER = 2 };
int gpmpc_tri_diag(gpmpc_ctx *ctx, int op, int n, int nrhs, const double *dL, int64_t ldl, double *dX, int64_t ldx,
                   const double *dW, int flags);

/* ---- a4-a6: exact GP ------------------------------------------------------
 * MultiOutputExactGP.fit (exact_gp.py:476-499 -> ExactGP.fit :118-184) for
 * n_out outputs sharing one kernel (one Gram + one Cholesky).
 * Y is (n x n_out) row-major.  Reproduces the jitter ladder of
 * exact_gp.py:163-175; jitter_steps = 0 (none) .. 6, and the function returns
 * GPMPC_ERR_NOT_PD (-100) when the ladder is exhausted (the reference raises
 * ValueError).  Outputs per output: y_mean, y_std, lml. */
#define GPMPC_ERR_NOT_PD (-100)
int gpmpc_gp_fit_exact(gpmpc_ctx *ctx, int kind, const double *X, int n, int d, const double *Y,
                       int n_out, const double *ls, double sigma2, double noise, gpmpc_gp **out,
                       double *y_mean, double *y_std, double *lml, int *jitter_steps);
/* gpmpc_gp_fit_exact with any kernel (ExactGP(kernel=...) fits whatever Kernel it is
 * given, exact_gp.py:157): the Gram from a composite-kernel program over the raw rows
 * (GPMPC_KP_*); predict / predict_cov then form K* and K** from the same program, and
 * the prior variance k(x, x) is the program's diagonal (a constant: the sum / product
 * of its leaves' sigma2).  -2 for a malformed program.  gpmpc_gp_append refits such a
 * GP (returns GPMPC_ERR_NOT_PD). */
int gpmpc_gp_fit_exact_prog(gpmpc_ctx *ctx, const int *ops, int nops, const double *par, int npar,
                            const double *X, int n, int d, const double *Y, int n_out, double noise,
                            gpmpc_gp **out, double *y_mean, double *y_std, double *lml, int *jitter_steps);
/* ExactGP.predict (exact_gp.py:213-268) for all outputs: mean/var (p x n_out). */
int gpmpc_gp_predict(gpmpc_ctx *ctx, gpmpc_gp *gp, const double *Xq, int p, double *mean,
                     double *var);
/* ExactGP.predict(return_cov=True) (exact_gp.py:247-254): cov (p x p) of the
 * latent posterior in normalised units (caller multiplies by y_std^2). */
int gpmpc_gp_predict_cov(gpmpc_ctx *ctx, gpmpc_gp *gp, const double *Xq, int p, double *mean,
                         double *cov);
/* append k training rows Xnew (k x d) to a fitted GP in O(n^2 k)
 * -- the result of gpmpc_gp_fit_exact on the concatenated data without the
 * O(n^3) refit (SparseGP.update's refit-with-concatenation semantics,
 * sparse_gp.py:328-353; online_update.py:361-408).  Yall holds the targets of
 * all n + k rows ((n + k) x n_out, old rows first): normalisation, alpha and
 * lml are recomputed over all of them.  Returns GPMPC_ERR_NOT_PD, with the
 * handle unchanged, when the GP was fitted with jitter or the new rows' Schur
 * complement is not positive definite: the caller refits the whole set (which
 * reruns the exact_gp.py:163-175 ladder).  A fleet built on the GP must be
 * recreated after an append (its scratch is sized for the old row count). */
int gpmpc_gp_append(gpmpc_ctx *ctx, gpmpc_gp *gp, const double *Xnew, int k, const double *Yall,
                    double *y_mean, double *y_std, double *lml);
/* Copies of the device state (L lower, n x n; alpha n x n_out). Either may be NULL. */
int gpmpc_gp_get_state(gpmpc_ctx *ctx, gpmpc_gp *gp, double *L, double *alpha);
int gpmpc_gp_destroy(gpmpc_gp *gp);

/* ---- 8f-3: batched log marginal likelihood (hyperparameter search) --------
 * Replaces the objective of ExactGP.optimize_hyperparameters
 * (exact_gp.py:357-421), each call of which is a full ExactGP.fit
 * (exact_gp.py:118-204), for B parameter sets at once: per set b the Gram of
 * X (n x d) with lengthscales ls[b*d .. b*d+d) (SE_ISO: ls[b*d]) and signal
 * variance sigma2[b], + noise[b] I, Cholesky (one batched launch; the
 * exact_gp.py:163-175 jitter ladder for sets that fail), and
 * lml[b] = -1/2 y^T alpha - sum log L_ii - n/2 log 2 pi on the normalised y.
 * jitter_steps[b] = 0..6, or -1 (and lml[b] = -inf) when the ladder is
 * exhausted -- the reference objective's ValueError -> inf. */
int gpmpc_gp_lml_batched(gpmpc_ctx *ctx, int kind, const double *X, int n, int d,
                         const double *y, int B, const double *ls, const double *sigma2,
                         const double *noise, double *lml, int *jitter_steps);

/* ---- a8-a10: FITC sparse GP ----------------------------------------------
 * MultiOutputSparseGP.fit (sparse_gp.py:430-456 -> SparseGP.fit FITC :150-219)
 * with caller-supplied inducing points Z (m x d) shared by all outputs.
 * Outputs per output: y_mean, y_std, lml.  Lambda (n) optional. */
int gpmpc_fitc_fit(gpmpc_ctx *ctx, const double *Z, int m, const double *X, int n, int d,
                   const double *Y, int n_out, const double *ls, double sigma2, double noise,
                   double jitter, gpmpc_fitc **out, double *y_mean, double *y_std, double *lml,
                   double *lambda_diag);
/* SparseGP(method="vfe").fit (sparse_gp.py:221-249 after the shared :181-188):
 * B = K_uu + K_uf K_fu / noise + jitter I, alpha = B^-1 K_uf y / noise, the VFE
 * lower bound as lml.  Same handle type as gpmpc_fitc_fit: gpmpc_fitc_predict
 * evaluates it with the reference's one predict body (sparse_gp.py:255-305). */
int gpmpc_vfe_fit(gpmpc_ctx *ctx, const double *Z, int m, const double *X, int n, int d,
                  const double *Y, int n_out, const double *ls, double sigma2, double noise,
                  double jitter, gpmpc_fitc **out, double *y_mean, double *y_std, double *lml);
/* SparseGP(kernel=any).fit (sparse_gp.py:182-183: K_uu = kernel(Z), K_uf = kernel(Z, X),
 * the diagonal kernel.diagonal(X)) with a composite-kernel program (above); method 0 =
 * FITC (lambda_diag optional), 1 = VFE. */
int gpmpc_sparse_fit_prog(gpmpc_ctx *ctx, int method, const int *ops, int nops, const double *par, int npar,
                          const double *Z, int m, const double *X, int n, int d, const double *Y, int n_out,
                          double noise, double jitter, gpmpc_fitc **out, double *y_mean, double *y_std,
                          double *lml, double *lambda_diag);
/* SparseGP.predict (sparse_gp.py:255-305), mean as written. */
int gpmpc_fitc_predict(gpmpc_ctx *ctx, gpmpc_fitc *gp, const double *Xq, int p, double *mean,
                       double *var);
/* copy of the fitted alpha (m x n_out: L_B^-T L_B^-1 A Lambda^-1 y per output,
 * sparse_gp.py:208-210) */
int gpmpc_fitc_get_state(gpmpc_ctx *ctx, gpmpc_fitc *gp, double *alpha);
int gpmpc_fitc_destroy(gpmpc_fitc *gp);

/* ---- a15: batched OSQP-style ADMM ------------------------------------------
 * Replaces osqp.OSQP().setup / update / warm_start / solve
 * (osqp_rti.py:464-478, 496, 517, 524, 527) for a batch of QPs
 *     min 1/2 x'Px + q'x  s.t.  l <= Ax <= u
 * sharing one sparsity pattern of A (CSR: rowptr m+1, colidx nnz) and a
 * diagonal P.  Per problem: Aval (nnz), Pdiag (n), q (n), l/u (m).  The
 * reduced KKT matrix M = P + sigma I + A' diag(rho) A is factored either
 * block-tridiagonally (the MPC stage structure: blocks of 10 variables
 * coupled through their first 7, n <= 216) or, for any other pattern, as a
 * banded LDL^T with half-bandwidth <= 16.  Caps: n <= 216, m <= 360,
 * nnz <= 896, <= 8 entries per row and <= 12 per column of A
 * (GPMPC_QP_NMAX / _MMAX / _NNZMAX / _WMAX / _ROWMAX / _COLMAX below); a
 * pattern outside them is refused with -2 and nothing is written.
 * State carried between solves (OSQP keeps it in its workspace):
 *   rho (batch), y_scaled (batch x m).  x_ws: warm-start primal (unscaled),
 *   NULL for zeros.
 * Outputs: x (batch x n), y (batch x m) unscaled, iters, status, obj.  A
 * status without a solution (not 1, 2 or -2) has x, y and obj NaN.  Status
 * -100, a reduced KKT matrix that is not positive definite (a negative
 * Pdiag entry), is one of them: iters 0, x, y and obj NaN, and that
 * problem's rho and y_scaled are left as they were passed in. */
#define GPMPC_QP_NMAX 216
#define GPMPC_QP_MMAX 360
#define GPMPC_QP_NNZMAX 896
#define GPMPC_QP_WMAX 16
#define GPMPC_QP_ROWMAX 8
#define GPMPC_QP_COLMAX 12
typedef struct {
  double rho, sigma, alpha;
  double eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  int max_iter, check_termination, adaptive_rho, adaptive_rho_interval;
  double adaptive_rho_tolerance;
  int scaling, warm_start;
} gpmpc_qp_settings;
void gpmpc_qp_default_settings(gpmpc_qp_settings *s); /* osqp_rti.py:54-60 + OSQP 0.6 defaults */
int gpmpc_qp_solve_batched(gpmpc_ctx *ctx, int batch, int n, int m, int nnz, const int *rowptr,
                           const int *colidx, const double *Aval, const double *Pdiag,
                           const double *q, const double *l, const double *u,
                           const gpmpc_qp_settings *s, const double *x_ws, double *rho,
                           double *y_scaled, double *x, double *y, int *iters, int *status,
                           double *obj);
/* Which KKT factor path gpmpc_qp_solve_batched takes for a pattern; needs no context and
 * no device.  info (GPMPC_QP_PATTERN_INFO_INTS ints): mode (0 banded LDL^T, 1 block
 * tridiagonal), half-bandwidth w, nblk (blocks of 10 variables), fac_len (factor slots),
 * maxrow, maxcol (most entries in a row / column of A), n_offd (mode 1: the slots of the
 * fleet's coalesced assembly list, -1 when the pattern has none), fits (1: within the caps,
 * 0: the solve refuses it with -2), is_fleet_pattern (1: the 3-DoF MPC at N = 20, which the
 * fleet's solver takes).  Returns 0, or -2 for a malformed pattern (n or m <= 0, rowptr not
 * non-decreasing from 0, a column outside [0, n)). */
#define GPMPC_QP_PATTERN_INFO_INTS 9
int gpmpc_qp_pattern_info(int n, int m, const int *rowptr, const int *colidx, int *info);

/* ---- the control step: a fleet of closed-loop 3-DoF GP-MPC landings -------
 * One "step" = for every landing: GP posterior (mean + variance) at the N
 * horizon points of its linearisation trajectory, RTI QP assembly with the GP
 * mean on the velocity rows (gp_mpc.py:303-320, correct sign), batched ADMM
 * (osqp_rti.py:501-567 protocol), plant step and Monte-Carlo termination
 * (monte_carlo.py:455-537).  Everything stays device-resident. */
typedef struct {
  int horizon;           /* N (osqp_rti.py OSQPRTIConfig.N / MPCConfig.N) */
  double dt;             /* control period */
  int target_mode;       /* must be 1: the solve protocol of monte_carlo.py:495-512 with its
                            incremental target (:497-500); the step protocol of
                            FastRTI3DoF is the host mirror (mpc/osqp_rti.py) */
  int use_gp;            /* add GP mean to c_k */
  int residual_model;    /* 1: plant gets the aero-drag residual (dispersion.py:349-360) */
  int max_steps;         /* max_time / dt */
  gpmpc_qp_settings qp;
  int sqp_iters;         /* 1: RTI, one QP per control step (the bench metric).
                            > 1: GPMPC.solve's loop (gp_mpc.py:296-345): up to sqp_iters
                            re-linearise -> GP posterior -> QP passes around the last QP
                            solution, stop when max|dX|, max|dU| < sqp_tol; not converged
                            -> MPCSolution.success False -> DIVERGENCE (monte_carlo.py
                            :506-508).  The warm start is the unshifted plan (gp_mpc.py
                            :358-359). */
  double sqp_tol;        /* 1e-4 (gp_mpc.py:343) */
  gpmpc_qp_settings sqp_qp;  /* QP settings of the SQP passes (sqp_iters > 1).  sqp_qp.max_iter
                                = 0 (the default) means "the same as qp", resolved when the fleet
                                launches, so a caller that edits only qp changes the passes too.
                                With sqp_iters > 1 and max_iter 0, an sqp_qp that equals neither
                                the defaults nor qp (a field edited alongside max_iter 0, which
                                would be ignored) makes gpmpc_fleet_create fail (-2): set
                                sqp_qp.max_iter to give the passes their own settings.
                                The reference solves this subproblem with IPOPT (gp_mpc.py:462-470) */
} gpmpc_fleet_config;
void gpmpc_fleet_default_config(gpmpc_fleet_config *c);
int gpmpc_fleet_create(gpmpc_ctx *ctx, gpmpc_gp *gp, const gpmpc_fleet_config *cfg, int batch,
                       gpmpc_fleet **out);
/* A shard of batch landings of a Monte-Carlo fleet of fleet_batch landings (>= batch;
 * gpmpc_fleet_create = fleet_batch equal to batch).  Every size-dependent path choice
 * (the posterior GEMM's kernel, the few-query posterior launch, the control kernel's
 * build) is made once, here, for fleet_batch landings -- never from the running count --
 * so each landing's results are bit-identical whatever the shard size and however many
 * landings still fly beside it. */
int gpmpc_fleet_create_shard(gpmpc_ctx *ctx, gpmpc_gp *gp, const gpmpc_fleet_config *cfg, int batch,
                             int fleet_batch, gpmpc_fleet **out);
/* The same fleet over a sparse GP (gpmpc_fitc_fit / gpmpc_vfe_fit, 11 features, 3
 * outputs): the reference-default Simple3DoFGP() is MultiOutputSparseGP FITC with 50
 * inducing points (structured_gp.py:423-428, sparse_gp.py:400-456).  Every step's
 * posterior is the reference's SparseGP.predict (sparse_gp.py:255-305) at every horizon
 * point: the mean K*u alpha as written (what GPMPC consumes through
 * gp.predict), the variance sigma2 - |L_uu^-1 k*|^2 + |L_B^-1 L_uu^-1 k*|^2.  The
 * sparse GP must outlive the fleet. */
int gpmpc_fleet_create_fitc(gpmpc_ctx *ctx, gpmpc_fitc *gp, const gpmpc_fleet_config *cfg, int batch,
                            int fleet_batch, gpmpc_fleet **out);
/* (re)initialise landings [first, first+count) from x0 (count x 7) */
int gpmpc_fleet_reset(gpmpc_fleet *f, int first, int count, const double *x0);
/* advance every active landing by nsteps control steps (async on the ctx stream) */
int gpmpc_fleet_step(gpmpc_fleet *f, int nsteps);
/* one step split in its phases, launched in the order 0, 2, 3, 1:
 * bit 0: horizon features + K* = k(Z*, X) Gram; bit 2: one FP64-MFMA pass
 * over K* with [L^-1; alpha^T]: variance partial sums |L^-1 K*^T|^2 and the
 * means alpha^T K*^T; bit 3: posterior finish;
 * bit 1: QP assembly + ADMM + plant step.  A full step = phases(15). */
int gpmpc_fleet_step_phases(gpmpc_fleet *f, int phase_mask);
/* records (batch x GPMPC_REC_LEN doubles): 0 outcome (0 running, 1..6 =
 * LandingOutcome of monte_carlo.py:25-33), 1 steps, 2 fuel used, 3 flight time,
 * 4..10 state, 11 total ADMM iterations, 12 solves with status "solved",
 * 13 initial mass, 14 last QP status, 15 last rho */
#define GPMPC_REC_LEN 16
int gpmpc_fleet_read(gpmpc_fleet *f, double *records, double *x /* batch x 7, may be NULL */);
/* the rest of every landing's controller state, any pointer may be NULL:
 * linearisation / warm-start trajectory Xw (batch x (N+1) x 7) and Uw
 * (batch x N x 3), the ADMM's persistent scaled duals (batch x m) and rho
 * (batch) -- what OSQP keeps between solves (osqp_rti.py:517-527) */
int gpmpc_fleet_get_state(gpmpc_fleet *f, double *Xw, double *Uw, double *y_scaled, double *rho);
/* the last control step's GP posterior at every landing's N horizon points
 * (ExactGP.predict, exact_gp.py:256-266, over the step's linearisation
 * trajectory): mean and variance, batch x N x 3 each, in landing order (either
 * may be NULL).  The step covers the running prefix of its dispatch order (every
 * landing running at its start, plus terminated ones the host had not yet read):
 * those read the posterior at their own trajectory, landings past it read NaN.
 * -2 when use_gp = 0. */
int gpmpc_fleet_get_posterior(gpmpc_fleet *f, double *mean, double *var);
/* diagnostic: launches of the query-feature kernel (k_fleet_queries) since the fleet was
 * created; a step whose Gram kernel forms the query rows itself adds none.  -1: f NULL */
int gpmpc_fleet_query_launches(gpmpc_fleet *f);
/* diagnostic: accumulate s_memtime cycles of landing 0's control kernel per
 * phase into dev_u64x16 (16 x uint64 device buffer; NULL disables):
 * 0 assembly, 1 scaling, 2 factor, 3 A' rhs, 4 KKT solve (band path, or the
 * block path's barrier tail), 5 fused z/y update, 6 checks + adaptive rho,
 * 7 tail (plant step, records), 8/9/10 block KKT solve forward / diagonal /
 * backward; 14 s_memrealtime ticks (100 MHz) and 15 shader-clock ticks over
 * the same solves */
int gpmpc_fleet_set_stamps(gpmpc_fleet *f, void *dev_u64x16);
/* diagnostic: per-landing control-kernel trace into dev_u64xbx4 (batch x 4
 * uint64 device buffer; NULL disables): start and end s_memrealtime (100 MHz),
 * HW_ID and XCC_ID of the landing's first wave */
int gpmpc_fleet_set_trace(gpmpc_fleet *f, void *dev_u64xbx4);
/* ---- Monte-Carlo protocol attachment (optional; entry points only, ABI 4 unchanged) --
 * What MonteCarloSimulator.run_single does around the control step besides the
 * termination rules: the plant dispersions (monte_carlo.py:530-537) and the trajectory
 * lists of SimulationResult (:539-544).  With nothing attached the fleet launches exactly
 * what it launches without these entry points; attached, one more small kernel follows
 * the control kernel of every control step (in SQP mode: of the last pass), and for each
 * landing whose step count advanced in that step
 *   v_next += (n0 thrust_dispersion) u0[0] / m_prev dt   (thrust_dispersion > 0; m_prev the
 *                                                          pre-step mass, u0[0] the first
 *                                                          control component only, :533)
 *   v_next += (n[1:4] aero_dispersion) dt                 (aero_dispersion > 0)
 * in that order and with the reference's roundings, written to the plant state and the
 * record's state slots, then (x_{t+1}, u0_t) is appended to the landing's log.  A landing
 * that terminates or diverges in a step appends nothing (the break before the append).
 * Landing outcomes 1 and 4 are both "landed" with the compiled run_experiments.py
 * tolerances; a caller with its own LandingConstraints re-decides between them on the host
 * from the record's final state. */
typedef struct {
  double thrust_dispersion; /* SimulationConfig.thrust_dispersion (>= 0) */
  double aero_dispersion;   /* SimulationConfig.aero_dispersion (>= 0) */
  int log_steps;            /* 0: no trajectory log; else the fleet's max_steps */
} gpmpc_fleet_mc_config;
/* noise: host, batch x max_steps x 4 standard normals, row [landing][step]: column 0 the
 * thrust draw, 1..3 the aero draws (copied; NULL allowed when both dispersions are 0).
 * Buffers come from the context's pool.  Attaching to landings in flight starts each log
 * at the landing's current step and state.  Replaces an earlier attachment.  -2: bad
 * arguments (a dispersion > 0 without noise, a negative dispersion, log_steps neither 0
 * nor max_steps). */
int gpmpc_fleet_mc_attach(gpmpc_fleet *f, const gpmpc_fleet_mc_config *mc, const double *noise);
/* the logs of landings [first, first+count): states (count x (max_steps+1) x 7, row 0 the
 * state at the reset), controls (count x max_steps x 3: the applied u0 of every step),
 * nsteps (count: appends so far = the landing's control steps); any may be NULL.  Rows
 * past a landing's count are NaN.  -2 without an attached log. */
int gpmpc_fleet_mc_read_log(gpmpc_fleet *f, int first, int count, double *states, double *controls, int *nsteps);
/* drop the attachment (gpmpc_fleet_destroy does too); gpmpc_fleet_reset restarts the
 * reset landings' logs (count 0, states[0] = x0) and leaves the others' alone */
int gpmpc_fleet_mc_detach(gpmpc_fleet *f);
/* ---- uncertainty propagation (uncertainty_prop.py:117-177) ------------------
 * Replaces the covariance recursion of UncertaintyPropagator._propagate_linear
 * (Sigma_next = A_d @ Sigma_k @ A_d.T + Q_gp, uncertainty_prop.py:163-167) for
 * batch trajectories at once: A (batch x N x nx x nx), q (batch x N x nx, the
 * diagonal of Q_gp), S0 (batch x nx x nx, or NULL for s0_diag * I, the
 * reference's default 1e-6 I), out (batch x (N+1) x nx x nx), all row-major;
 * nx <= 16.  The host version copies in and out; _dev takes device pointers and
 * is asynchronous on the context stream. */
int gpmpc_cov_propagate(gpmpc_ctx *ctx, int batch, int N, int nx, const double *A, const double *q,
                        const double *S0, double s0_diag, double *out);
int gpmpc_cov_propagate_dev(gpmpc_ctx *ctx, int batch, int N, int nx, const double *dA,
                            const double *dq, const double *dS0, double s0_diag, double *dout);
/* UncertaintyPropagator._propagate_linear (uncertainty_prop.py:117-177) of the 3-DoF model
 * on the device, for batch trajectories in one call (what GPMPC.solve runs on every call,
 * gp_mpc.py:284-290, with N sequential GP predictions on the host): the explicit-Euler
 * dynamics of rocket_3dof.py (x+ = x + dt f, f = [-alpha |u|, v, u / m + g3]) plus dt times
 * the exact GP's mean on the velocity rows, A_k = I + dt J(x_k, u_k), q_k = dt^2 times the
 * GP variance on the velocity rows, Sigma_0 = S0 (batch x 7 x 7) or s0_diag I.  gp: the
 * 3-DoF exact GP (11 features, 3 outputs, a leaf kernel; else -2).  Host buffers: x0
 * (batch x 7), U (batch x N x 3) in; means (batch x (N+1) x 7), covs (batch x (N+1) x 7 x 7)
 * out.  (Round 6, ABI 4: an added entry point.) */
int gpmpc_uprop3_linear(gpmpc_ctx *ctx, gpmpc_gp *gp, int batch, int N, double dt, double alpha,
                        const double *g3, const double *x0, const double *U, const double *S0,
                        double s0_diag, double *means, double *covs);
/* The same for the 14-state model (uncertainty_prop.py:117-177 as GPMPC.solve runs it for
 * Rocket6DoFDynamics, gp_mpc.py:284-290): RK4 with quaternion normalisation
 * (rocket_6dof.py step) plus dt times the StructuredRocketGP means on the velocity
 * (rows 4-6, d_v) and rate rows (11-13, d_omega), A_k = I + dt J(x_k, u_k), q_k = dt^2 times
 * the GP variances on those rows.  gp_v / gp_w: the pair's device GPs, gpmpc_gp * (exact = 1)
 * or gpmpc_fitc * (exact = 0), 13 / 12 features and 3 outputs each, leaf kernels (else -2).
 * rocket: J_B (9, row-major; invertible), r_T_B (3), g_I (3), alpha = 1 / (I_sp g0), g0.
 * Host buffers: x0 (batch x 14), U (batch x N x 3), S0 (batch x 14 x 14) or NULL (s0_diag I)
 * in; means (batch x (N+1) x 14), covs (batch x (N+1) x 14 x 14) out.  (Round 6, ABI 4: an
 * added entry point.) */
int gpmpc_uprop6_linear(gpmpc_ctx *ctx, void *gp_v, void *gp_w, int exact, const double *rocket,
                        int batch, int N, double dt, const double *x0, const double *U,
                        const double *S0, double s0_diag, double *means, double *covs);
/* UncertaintyPropagator._propagate_unscented (uncertainty_prop.py:179-264) of the 3-DoF
 * model on the device, for batch trajectories in one call: per step the Cholesky factor of
 * (n + lambda) Sigma_k + 1e-10 I, the 15 sigma points through the explicit-Euler step plus
 * dt times the GP mean on the velocity rows, x_k+1 = sum w_m,i of their images, Sigma_k+1 =
 * sum w_c,i d_i d_i^T + dt^2 times the GP variance at x_k on the velocity rows.  One
 * workgroup per trajectory runs the whole recursion (csrc/uprop_ut.hip).  gp: gpmpc_gp *
 * (exact = 1) or gpmpc_fitc * (exact = 0; FITC and VFE), 11 features, 3 outputs, a leaf
 * kernel, at most 4096 training / inducing rows (else -2).  ut: the transform's alpha, beta,
 * kappa (the reference: 1e-3, 2, 0).  dt, alpha, g3, x0, U, S0, s0_diag, means, covs as
 * gpmpc_uprop3_linear.  info (batch, host): 0, or k + 1 when the factor of step k met a
 * non-positive pivot -- that trajectory stops there, its rows k+1 .. N of means and covs
 * are NaN, the others are unaffected and the call still returns 0.  (ABI 4: an added
 * entry point.) */
int gpmpc_uprop3_unscented(gpmpc_ctx *ctx, void *gp, int exact, int batch, int N, double dt, double alpha,
                           const double *g3, const double *ut, const double *x0, const double *U,
                           const double *S0, double s0_diag, double *means, double *covs, int *info);
/* The same for the 14-state model: 29 sigma points through RK4 with quaternion
 * normalisation (rocket_6dof.py step) plus dt times the StructuredRocketGP means on rows
 * 4-6 (d_v) and 11-13 (d_omega), the variances of both GPs at x_k on those rows.  gp_v /
 * gp_w, exact, rocket and the host buffers as gpmpc_uprop6_linear; ut and info as
 * gpmpc_uprop3_unscented.  (ABI 4: an added entry point.) */
int gpmpc_uprop6_unscented(gpmpc_ctx *ctx, void *gp_v, void *gp_w, int exact, const double *rocket,
                           const double *ut, int batch, int N, double dt, const double *x0, const double *U,
                           const double *S0, double s0_diag, double *means, double *covs, int *info);
/* UncertaintyPropagator._propagate_monte_carlo (uncertainty_prop.py:266-315) of the 3-DoF
 * model on the device, for batch trajectories of n_samples (>= 2) particles in one call.  The
 * draws are the caller's (numpy's global RNG in the reference's order): particles0 (batch x
 * n_samples x 7), the particles at step 0, and normals (batch x N x n_samples x 1 x 3), the
 * standard normals of every step.  Per step: one posterior at all batch * n_samples particles,
 * then per particle the explicit-Euler step plus (d + sqrt(var) z) dt on the velocity rows
 * (csrc/uprop_mc.hip).  means[b, k] (k >= 1) is the sample mean, summed in particle order and
 * divided by n_samples; covs[b, k] the sample covariance over n_samples - 1, exactly
 * symmetric; row 0 of both is x0 and S0 (NULL: s0_diag I).  particles (batch x (N+1) x
 * n_samples x 7; row 0 = particles0) or NULL: the paths are not read back.  gp, exact, dt,
 * alpha, g3, x0, U as gpmpc_uprop3_unscented, without its cap on the row count.  Nothing
 * can fail per trajectory: no info.  (ABI 4: an added entry point.) */
int gpmpc_uprop3_mc(gpmpc_ctx *ctx, void *gp, int exact, int batch, int N, int n_samples,
                    double dt, double alpha, const double *g3,
                    const double *x0, const double *U, const double *S0, double s0_diag,
                    const double *particles0, const double *normals,
                    double *means, double *covs, double *particles /* nullable */);
/* The same for the 14-state model: RK4 with quaternion normalisation (rocket_6dof.py step)
 * plus (d + sqrt(var) z) dt on rows 4-6 (d_v) and 11-13 (d_omega), one posterior per GP and
 * step.  normals (batch x N x n_samples x 2 x 3): per particle the d_v normals, then the
 * d_omega ones; particles0 and particles 14 wide.  gp_v / gp_w, exact and rocket as
 * gpmpc_uprop6_linear.  (ABI 4: an added entry point.) */
int gpmpc_uprop6_mc(gpmpc_ctx *ctx, void *gp_v, void *gp_w, int exact, const double *rocket,
                    int batch, int N, int n_samples, double dt,
                    const double *x0, const double *U, const double *S0, double s0_diag,
                    const double *particles0, const double *normals,
                    double *means, double *covs, double *particles /* nullable */);

/* ---- BASELINE configs[4]: batched 6-DoF GP-MPC rollouts --------------------
 * gpmpc_rollout_batched of SURVEY 8b.  One step = for every running rollout:
 * the Monte-Carlo termination rules (monte_carlo.py:455-488 on [m, r, v]),
 * GPMPC.solve's forward simulation with the StructuredRocketGP FITC means
 * (gp_mpc.py:258-281; RK4 of nominal_mpc.py:163-203), the QP subproblem of
 * gp_mpc.py:394-460 in deviation variables with its QCQP rows made linear
 * (DESIGN.md section 9), the OSQP-0.6 ADMM on the block-tridiagonal reduced
 * KKT matrix, the truth plant step (RK4 + the dispersion.py:349-360 drag) and
 * the plan kept unshifted as the next warm start.  State 14 = [m, r_I, v_I,
 * q_BI (w, x, y, z), omega_B]; horizon 20 (GPMPCConfig's N, gp_mpc.py:110 /
 * nominal_mpc.py:47) or 30 (BASELINE configs[4]), each a compiled instance. */
typedef struct gpmpc_rollout6 gpmpc_rollout6;
typedef struct {
  int horizon;           /* 20 or 30 (the compiled instances); default 30 */
  double dt;
  int max_steps;
  gpmpc_qp_settings qp;  /* osqp_rti.py:54-60 defaults */
  int fitc_mean_as_written;  /* 1 (default since round 6): the reference's K*u alpha
                                (sparse_gp.py:280-283, SURVEY D1 kept); 0: the FITC
                                posterior mean K*u L_uu^-T alpha (D1 fixed) */
  /* GPMPC's problem data (ABI 2).  Defaults: CostWeights (cost_functions.py:39-98),
   * ConstraintParams (constraints.py:35-50), gp_mpc.py:432-435. */
  double q_diag[14];     /* stage cost Q (diagonal) */
  double p_diag[14];     /* terminal cost P (diagonal; 10 Q) */
  double r_diag[3];      /* control cost R (diagonal) */
  double t_min, t_max;   /* thrust magnitude bounds */
  double tan_gamma_gs;   /* tan of the glide-slope angle, np.tan(np.deg2rad(30)) */
  double trust_x2, trust_u2;  /* squared trust radii 10, 5 */
  int use_gp_mean;       /* GPMPCConfig.use_gp_mean: 0 drops the GP from the simulation and c_k */
  int upright_target;    /* rollouts: 0 = monte_carlo.py:497-500 as written (x copied, v = 0,
                            altitude - 2); 1 = also q = (1, 0, 0, 0), omega = 0 */
  /* the rocket (ABI 3): Rocket6DoFConfig (rocket_6dof.py:36-84) as the dynamics of
   * nominal_mpc.py:163-203 use it.  Defaults J_B = diag(0.02, 1, 1) 0.168 (a full
   * tensor: rocket_J below), r_T_B = (-0.25, 0, 0), g_I = (-1, 0, 0), I_sp 30, g0 1:
   * alpha = 1 / (I_sp g0); g0 also sets the hover guess [0, 0, m g0] (gp_mpc.py:271-275) */
  double rocket_j[3];    /* diagonal of J_B */
  double rocket_r_t[3];  /* thrust application point r_T_B */
  double rocket_g_i[3];  /* gravity g_I */
  double rocket_alpha;   /* 1 / (I_sp g0) */
  double rocket_g0;
  /* ABI 4: the full inertia tensor J_B (row-major 3 x 3, rocket_6dof.py:44, 77-78, 147:
   * any invertible matrix; nominal_mpc.py:196-199 solves with it).  All zeros (the
   * default) = diag(rocket_j).  A diagonal tensor runs exactly as its diagonal would. */
  double rocket_J[9];
} gpmpc_rollout6_config;
void gpmpc_rollout6_default_config(gpmpc_rollout6_config *c);
/* gp_v: FITC on the 13 translational features, gp_w: on the 12 rotational
 * ones (features.py:149-365), 3 outputs each; both must outlive the batch */
int gpmpc_rollout6_create(gpmpc_ctx *ctx, gpmpc_fitc *gp_v, gpmpc_fitc *gp_w,
                          const gpmpc_rollout6_config *cfg, int batch, gpmpc_rollout6 **out);
/* the same over a pair of exact GPs (StructuredRocketGP(use_sparse=False),
 * exact_gp.py:213-268: mean K* alpha over the training rows) */
int gpmpc_rollout6_create_exact(gpmpc_ctx *ctx, gpmpc_gp *gp_v, gpmpc_gp *gp_w,
                                const gpmpc_rollout6_config *cfg, int batch, gpmpc_rollout6 **out);
/* GPMPC.solve (gp_mpc.py:229-369) for every rollout b of the batch at x0[b]
 * (batch x 14) with target x_target[b] (batch x 14), X_ref = x_target, U_ref = 0:
 *   pass 1: forward simulation of the warm-start controls with the GP mean
 *           (gp_mpc.py:258-281), the QP around it (:394-460, made linear as the
 *           rollouts), plan <- X_pred + dX, U_pred + dU;
 *   pass p > 1: GP means and Jacobians at the last plan (:299-320), QP, plan;
 *   stop after max_sqp_iter passes or when max|X_new - X_pred| and
 *   max|U_new - U_pred| are both < sqp_tol (:336-345).
 * A QP without a solution returns the nominal trajectory (:478-482: X_new =
 * X_pred, so the loop stops as converged) with qp_status < 0 (not -2).
 * cold = 1: the hover guess [0, 0, m0 g0] at every stage and fresh ADMM duals /
 * rho (first call, GPMPC.reset_warm_start); cold = 2: fresh duals / rho, the
 * controls already set (gpmpc_rollout6_set_state: U_ref, :268-269); cold = 0:
 * the previous call's plan U, unshifted (:266-267, :358-359).  The batch's Monte-Carlo records are not
 * touched except rec[11] (ADMM iterations of this call), rec[12] (solves with
 * status solved), rec[14] (last QP status), rec[15] (rho).
 * Outputs (any may be NULL): X (batch x (N+1) x 14), U (batch x N x 3), passes,
 * converged (0 / 1), qp_status of the last pass, qp_iters summed over passes. */
int gpmpc_rollout6_solve(gpmpc_rollout6 *r, const double *x0, const double *x_target, int cold,
                         int max_sqp_iter, double sqp_tol, double *X, double *U, int *passes,
                         int *converged, int *qp_status, int *qp_iters);
/* the same with the QP cost's reference trajectory (gp_mpc.py:442-453): X_ref
 * (batch x (N+1) x 14; NULL = x_target on every stage) and U_ref (batch x N x 3;
 * NULL = 0) in sum_k |x_k - X_ref[k]|_Q^2 + |u_k - U_ref[k]|_R^2 + |x_N - X_ref[N]|_P^2.
 * (U_ref's other use, the first guess of :268-269, is cold = 2 after
 * gpmpc_rollout6_set_state.) */
int gpmpc_rollout6_solve_ref(gpmpc_rollout6 *r, const double *x0, const double *x_target, const double *X_ref,
                             const double *U_ref, int cold, int max_sqp_iter, double sqp_tol, double *X,
                             double *U, int *passes, int *converged, int *qp_status, int *qp_iters);
/* (re)start rollouts [first, first+count) at x0 (count x 14) */
int gpmpc_rollout6_reset(gpmpc_rollout6 *r, int first, int count, const double *x0);
/* nsteps control steps of every running rollout (async on the ctx stream) */
int gpmpc_rollout6_step(gpmpc_rollout6 *r, int nsteps);
/* one step split in its kernels, launched in order: bit 0 termination rules +
 * forward simulation + GP means + Jacobians (k_r6_predict), bit 1 QP + ADMM +
 * plan (k_r6_control), bit 2 truth plant step (k_r6_plant); a full step = 7 */
int gpmpc_rollout6_step_phases(gpmpc_rollout6 *r, int mask);
/* records (batch x GPMPC_REC_LEN, the fleet layout; state slots hold [m, r, v])
 * and the full states (batch x 14, may be NULL) */
int gpmpc_rollout6_read(gpmpc_rollout6 *r, double *records, double *x);
/* controller state, any pointer may be NULL: warm-start controls U (batch x N
 * x 3), last QP plan X (batch x (N+1) x 14), forward-simulated X_pred (batch x
 * (N+1) x 14), its GP means (batch x N x 6: d_v, d_omega), the ADMM's persistent
 * scaled duals (batch x M, M = 36 N + 24: 1104 at N = 30, 744 at N = 20) and rho (batch) */
int gpmpc_rollout6_get_state(gpmpc_rollout6 *r, double *U, double *X_plan, double *X_pred,
                             double *gp_mean, double *y_scaled, double *rho);
/* set controller state (any pointer may be NULL): U (batch x N x 3), scaled
 * duals (batch x M), rho (batch) -- e.g. to carry a warm start across a GP
 * refit, or to start GPMPC.solve from caller-given controls */
int gpmpc_rollout6_set_state(gpmpc_rollout6 *r, const double *U, const double *y_scaled, const double *rho);
int gpmpc_rollout6_destroy(gpmpc_rollout6 *r);

/* device pointer of the record array (for collectives) */
double *gpmpc_fleet_records_dev(gpmpc_fleet *f);
double *gpmpc_rollout6_records_dev(gpmpc_rollout6 *r);

/* ---- (e) the one collective: shard records to the root over RCCL -----------
 * SURVEY 8b gpmpc_gather_results.  Landings are sharded in contiguous blocks,
 * one process per GPU, with no data-path collective (monte_carlo.py:401-583 is
 * per landing); at the end one ncclGather over xGMI brings every rank's record
 * block to the root.  The communicator is bootstrapped from a ncclUniqueId
 * that rank 0 creates (gpmpc_comm_unique_id) and the caller distributes (a
 * file on local disk, or the process group it already has).  RCCL is loaded at
 * run time (librccl.so.1; the copy torch loaded when there is one). */
typedef struct gpmpc_comm gpmpc_comm;
#define GPMPC_COMM_ID_BYTES 128
int gpmpc_comm_unique_id(unsigned char *id /* GPMPC_COMM_ID_BYTES */);
int gpmpc_comm_init(gpmpc_ctx *ctx, const unsigned char *id, int nranks, int rank, gpmpc_comm **out);
int gpmpc_comm_destroy(gpmpc_comm *c);
/* ranks the RCCL communicator spans (ncclCommCount) */
int gpmpc_comm_count(gpmpc_comm *c, int *nranks);
/* d_records: this rank's counts[rank] x GPMPC_REC_LEN records (device, e.g.
 * gpmpc_fleet_records_dev); counts: every rank's shard size (host, nranks).
 * On the root, out (host) receives sum(counts) x GPMPC_REC_LEN doubles in
 * rank order; elsewhere out may be NULL.  Collective: every rank calls it.
 * = gpmpc_gather_prepare + gpmpc_gather_collective. */
int gpmpc_gather_results(gpmpc_ctx *ctx, gpmpc_comm *c, const double *d_records, const int *counts, int root,
                         double *out);
/* The same gather in two steps, so that the ranks can agree in between: prepare is
 * local (argument checks, send/receive buffers, the device padding of the ragged
 * block; the stream is drained before it returns), so every failure a rank can
 * meet alone is reported by it; collective issues only the ncclGather and the
 * root's compaction, and fails with -2 unless prepare succeeded since the last
 * collective with the same counts and root (the buffers were sized and padded for
 * them; a call with other arguments leaves the prepared block for the right one).  Agree on every rank's prepare status before any rank calls
 * collective (sharding.gather_shard_records does, with one all-reduce). */
int gpmpc_gather_prepare(gpmpc_ctx *ctx, gpmpc_comm *c, const double *d_records, const int *counts, int root);
int gpmpc_gather_collective(gpmpc_ctx *ctx, gpmpc_comm *c, const int *counts, int root, double *out);
int gpmpc_fleet_destroy(gpmpc_fleet *f);

/* ---- novelty / diverse-subset selection of GP training data ---------------
 * Replaces the distance part of NoveltySelector._compute_distance_novelty
 * (novelty_selector.py:154-170) and the greedy loop of NoveltySelector.select_diverse
 * (:264-296).  Every squared distance is summed in numpy's order for
 * np.linalg.norm(A - x, axis=1), so the results are numpy's bits.
 *
 * dist[i] = min_j |X[i] - R[j]|_2: X n x d, R r x d (host, row-major), dist n (host).
 * 1 <= d <= 32, n >= 0, r >= 1. */
int gpmpc_nn_dist(gpmpc_ctx *ctx, const double *X, int n, const double *R, int r, int d, double *dist);
/* Greedy farthest-point picking: pick 0 = argmax(scores); pick t = argmax over the
 * unselected i of scores[i] + diversity_weight * mind[i], mind[i] the distance of X[i] to
 * the nearest pick so far (the reference's weight is 0.5); the lowest index wins equal
 * values.  X n x d, scores n (host; finite); idx_out n_select picks in order,
 * combined_out (n_select, may be NULL) each pick's winning value (pick 0: its score).
 * 1 <= d <= 32, 1 <= n_select <= n.  path: 0 automatic, 1 one workgroup in one launch
 * (n <= 8192, else -2), 2 a grid of workgroups with one launch per pick. */
int gpmpc_select_diverse(gpmpc_ctx *ctx, const double *X, int n, int d, const double *scores, int n_select,
                         double diversity_weight, int path, int *idx_out, double *combined_out);

/* ---- k-means for the sparse GP's inducing points ---------------------------
 * Lloyd's iteration of scipy.cluster.vq.kmeans2 (SparseGP._initialize_inducing_points,
 * sparse_gp.py:122-148) from the code book C0 (k x d): `iters` times label = index of the
 * nearest centre (lowest index on equal distances), then every centre = the mean of its
 * observations, summed in ascending observation order and divided once by the count; a
 * centre without observations keeps its row.  X n x d, C0 k x d (host,
 * row-major); C_out k x d the last code book, labels_out n the labels of the last
 * assignment (from before the last update, as kmeans2 returns them), empty_per_iter
 * `iters` counts of centres without observations.
 * min_margin: the smallest (second nearest - nearest squared distance) / (|x|^2 + max_j
 * |c_j|^2) over every decision of the call; unsafe: the decisions with a margin <=
 * gpmpc_kmeans_tau(d) = 16 (d + 2) 2^-53, within which the rounding of scipy's distance
 * formula and of this one may order two centres differently.  With unsafe = 0 the labels
 * and the code book are kmeans2's bits.  1 <= d <= 32, n, k, iters >= 1 (k > n allowed). */
int gpmpc_kmeans_lloyd(gpmpc_ctx *ctx, const double *X, int n, int d, const double *C0, int k, int iters,
                       double *C_out, int *labels_out, int *empty_per_iter, double *min_margin, int *unsafe);
double gpmpc_kmeans_tau(int d);

/* ---- k-nearest-neighbour search over a resident set -----------
 * The neighbour search of the learning-MPC safe sets: LocalSafeSet.query / interpolate_q
 * (local_safe_set.py:158-300) and the K neighbours of the Q-function approximators
 * (q_function.py:97-190), batched over B queries against a set that stays on the device.
 *
 * gpmpc_knn_create: S n x d (host, row-major; stored as given, the caller applies any
 * weighting), q (n, may be NULL) the rows' cost-to-go, fuel_req (n, may be NULL) the fuel a
 * row needs.  1 <= d <= 32, n >= 1, else -2.
 *
 * gpmpc_knn_query, per query b (Xq B x d host): the k smallest distances in ascending order
 * (dist, B x k) with their row indices (idx, B x k; positions in the full set), equal
 * distances by lower row index; where fewer than k rows qualify the tail is inf / n.
 * n_ball[b] = qualifying rows with s^2 <= radius * radius (the product rounded once, rows at
 * the radius counted).  avail_fuel (B, may be NULL): row i qualifies iff fuel_req[i] <=
 * avail_fuel[b] (without it every row does); n_feasible[b] = qualifying rows.  1 <= k <= 64,
 * else -2.  Every s^2 is a sum of squared direct differences in the order `order` names:
 * 0 scipy's KD-tree (four accumulators over full blocks of four, ((a0+a1)+a2)+a3, the tail
 * one by one: KDTree.query's and query_ball_point's bits), 1 numpy's
 * np.linalg.norm(A - x, axis=1) (as gpmpc_nn_dist); selection is on s^2, the square root is
 * the correctly rounded one.
 *
 * gpmpc_knn_interp: LocalSafeSet.interpolate_q(method="inverse_distance") per query: K =
 * k_base, with adaptive != 0 K = (int)(k_base * (1 + 2 * n_ball / n_feasible)) clipped to
 * [k_min, k_max]; then min with n_feasible, max with k_min, min with k_max (k_max <= 64);
 * q_out[b] = q of the nearest when its distance < 1e-10, else the mean of the K nearest q
 * weighted by 1 / (dist + 1e-10); k_used[b] = K.  No qualifying row: q_out = inf, k_used = 0;
 * fewer than K qualifying rows (the reference raises IndexError): q_out = NaN, k_used = -1.
 *
 * gpmpc_knn_plan (no device): how a call of B queries over n rows is launched: parts = the
 * row ranges the scan's grid splits n into (> 1: a second launch merges them), q_per_wave =
 * the queries a wave serves at once. */
int gpmpc_knn_create(gpmpc_ctx *ctx, const double *S, int n, int d, const double *q, const double *fuel_req,
                     gpmpc_knn **out);
int gpmpc_knn_destroy(gpmpc_knn *set);
int gpmpc_knn_query(gpmpc_knn *set, int order, const double *Xq, int B, int k, double radius,
                    const double *avail_fuel, int *idx, double *dist, int *n_ball, int *n_feasible);
int gpmpc_knn_interp(gpmpc_knn *set, int order, const double *Xq, int B, int k_base, int k_min, int k_max,
                     int adaptive, double radius, const double *avail_fuel, double *q_out, int *k_used);
int gpmpc_knn_plan(int n, int d, int B, int k, int *parts, int *q_per_wave);

/* ---- projection onto a convex hull ------------------------------
 * The terminal constraint x_N in Conv{v_1 .. v_K} of learning MPC: ConvexHullConstraint.
 * project_onto_hull / check_feasibility / get_interpolated_q (convex_hull.py:125-237), batched
 * over B queries.  Per query x and its nv <= 64 vertices in d <= 32 dimensions: lambda >= 0,
 * sum lambda = 1, minimising |sum lambda_i w_i|, w_i = v_i - x, by Wolfe's minimum-norm-point
 * method.  A major cycle takes the vertex that minimises p . w_i (p = sum lambda_i w_i; equal
 * values: the lower index) into the active set unless |p|^2 - min_i p . w_i <= tol max_i |w_i|^2;
 * a minor cycle moves to the minimum-norm point of the active set's affine hull, or towards it
 * up to the boundary and drops the vertex that reaches zero.  The run starts at the vertex
 * nearest x (the lowest such index) and takes at most max_iter cycles, major and minor counted
 * alike.
 *
 * gpmpc_hull_project: shared = 1: one vertex set V (kmax x d, host, row-major) and q (kmax, may
 * be NULL) for all B queries; shared = 0: V B x kmax x d and q B x kmax.  nv (B, may be NULL:
 * kmax for every query): query b uses the first nv[b] rows of its set, rows past them are never
 * read by the device.  X B x d.  Per query: lambda (B x kmax, zero past nv[b]), proj (B x d) =
 * x + sum lambda_i w_i, dist = |proj - x|, gap = (|p|^2 - min_i p . w_i) / max_i |w_i|^2 (0
 * where that maximum is 0), qhull = sum lambda_i q_i (written only when q is given), iters the
 * cycles taken, status:
 *   0 certified: the stop test holds in fp64;
 *   1 not certified: max_iter reached, or the active set numerically dependent; lambda is
 *     still a convex combination and gap says how far it is from certified;
 *   2 nv[b] = 0: proj = x, dist = +inf, lambda 0, gap 0, qhull +inf;
 *   3 a non-finite entry among x or the used vertices (or a difference whose square
 *     overflows), tested before the first cycle: the outputs are NaN (lambda past nv[b] zero).
 * The result of a query depends on its own x, nv[b] and used rows alone, bit for bit.
 * 1 <= d <= 32, 1 <= kmax <= 64, 0 <= nv[b] <= kmax, tol > 0 (finite), 1 <= max_iter <= 4096,
 * else -2; B = 0 returns 0.
 *
 * gpmpc_knn_set_points: attaches n x dp payload rows P (host, row-major, 1 <= dp <= 32) to a
 * k-NN set: the raw states of the rows the set searches by (the set itself holds the weighted
 * ones).  A second call replaces them; the other calls of the set do not read them.
 *
 * gpmpc_knn_hull: gpmpc_knn_query's search for Xq (B x d), the K rule of gpmpc_knn_interp, then
 * the projection of Xp (B x dp) onto the hull of the K nearest payload rows, nearest first, in
 * one call that does not leave the device in between.  k_used[b] = K (0 with status 2 when no
 * row qualifies; -1, also status 2, where the reference raises IndexError), idx (B x k_max)
 * the K row indices (n past K), lambda B x k_max, qhull from the set's q (may be NULL; written
 * only when the set has q); the other outputs as gpmpc_hull_project, whose result on the same
 * rows it equals bit for bit.  -2 without payload rows.
 *
 * gpmpc_hull_plan (no device): q_per_group = the queries one workgroup serves (one a wave). */
int gpmpc_hull_project(gpmpc_ctx *ctx, const double *V, const double *q, const int *nv, int shared,
                       const double *X, int B, int kmax, int d, double tol, int max_iter, double *lambda,
                       double *proj, double *dist, double *gap, double *qhull, int *iters, int *status);
int gpmpc_knn_set_points(gpmpc_knn *set, const double *P, int dp);
int gpmpc_knn_hull(gpmpc_knn *set, int order, const double *Xq, const double *Xp, int B, int k_base, int k_min,
                   int k_max, int adaptive, double radius, const double *avail_fuel, double tol, int max_iter,
                   int *k_used, int *idx, double *lambda, double *proj, double *dist, double *gap, double *qhull,
                   int *iters, int *status);
int gpmpc_hull_plan(int d, int kmax, int B, int *q_per_group);

/* ---- predictive safety filter ----------------------------------
 * PredictiveSafetyFilter.filter of the reference's src/safety/safety_filter.py on its
 * gradient path (_solve_gradient_qp), for the 14-state rocket under the linear backup law
 * u = clip(u_eq - K (x - x_eq), u_min, u_max) and the ellipsoid V(x) = (x - x_eq)' P (x - x_eq)
 * <= alpha.  A control is safe when (x, u) meets the constraints, the trajectory "u for one
 * step, then the backup law" (horizon RK4 steps of dt) meets them at every step, and alpha -
 * V(x_N) > 0.  An unsafe control takes at most n_iters steps u <- u - lr (grad V + 2 (u -
 * u_nom)) with forward differences of fd_eps, each projected onto T_min <= |u| <= T_max (the
 * lower side divides by max(|u|, 1e-6)), until V(x_N(u)) <= backup_margin * alpha.
 *
 * K 3 x 14 and P 14 x 14 row-major, any values (P is read as given, both triangles).
 * u_min / u_max: -inf / +inf for no bound.  have_constraints = 0: no constraint test (the
 * projection still uses T_min, T_max); else |u| in [T_min, T_max], 1 - 2 (qx^2 + qy^2) >=
 * cos_theta_max and, above 0.1 of altitude, r_x^2 tan2_gamma >= r_y^2 + r_z^2.
 * rocket: 17 doubles, J_B (9, row-major), r_T_B (3), g_I (3), alpha, g0 (gpmpc_uprop6_linear).
 *
 * gpmpc_safety_filter: batch queries x (batch x 14), u_nom (batch x 3), host buffers, one
 * upload, one device call, one read-back.  Per query: u_safe (3), margin = alpha - V and
 * backup_value = V of the returned control's trajectory, flags (bit 0: modified, bit 1: the
 * returned control is safe), viol_mask (bit 0: the immediate test failed, bit 1 + k: step k of
 * the path), iters (gradient steps taken; 0 when unmodified).
 * gpmpc_safety_simulate: the closed loop x_(t+1) = step(x_t, filter(x_t, U_nom[t])) for T
 * steps from batch starts x0 in one device call: X (batch x (T+1) x 14), U (batch x T x 3),
 * margin / flags / iters (batch x T).
 * Both return -2 with gpmpc_last_error set for a null pointer, batch < 1, horizon outside
 * 1..31, dt <= 0 or a singular rocket J_B. */
typedef struct {
  int horizon;            /* 10 */
  double dt;              /* 0.1 */
  double K[42];
  double P[196];
  double x_eq[14];
  double u_eq[3];
  double u_min[3];        /* -inf */
  double u_max[3];        /* +inf */
  double alpha;           /* 1.0 */
  double backup_margin;   /* 0.9 */
  int have_constraints;   /* 0 */
  double T_min;           /* 0.5 */
  double T_max;           /* 5.0 */
  double cos_theta_max;   /* cos 60 deg */
  double tan2_gamma;      /* tan^2 30 deg */
  int n_iters;            /* 50 */
  double lr;              /* 0.1 */
  double fd_eps;          /* 1e-4 */
} gpmpc_safety_config;
void gpmpc_safety_default_config(gpmpc_safety_config *cfg);
int gpmpc_safety_filter(gpmpc_ctx *ctx, const double *rocket, const gpmpc_safety_config *cfg, int batch,
                        const double *x, const double *u_nom, double *u_safe, double *margin,
                        double *backup_value, int *flags, int *viol_mask, int *iters);
int gpmpc_safety_simulate(gpmpc_ctx *ctx, const double *rocket, const gpmpc_safety_config *cfg, int batch, int T,
                          const double *x0, const double *U_nom, double *X, double *U, double *margin, int *flags,
                          int *iters);

/* ---- tube MPC: uncertainty tubes ---------------------------------
 * TubePropagator of the reference's src/safety/tube_mpc.py for the 14-state rocket (rocket: the
 * 17 doubles of gpmpc_uprop6_linear), batch trajectories per call, host buffers, one upload,
 * one device call, one read-back.  X_nom (batch x (N+1) x 14), U_nom (batch x N x 3), tubes
 * (batch x (N+1) x 14) with tubes[b, 0] = 0.
 * gpmpc_tube_linear: per (b, k) the forward-difference linearisation of the plant step at
 * (X_nom[b,k], U_nom[b,k]) (the nominal step, x[i] += eps for the 14 states, u[i] += eps for
 * the 3 controls, the differences divided by eps), A_cl = A + B K (A when K is NULL) and
 * e_(k+1) = |A_cl| e_k + w_k.  w_mode 0: w_k = w_max on every row (w unused); 1: w holds 14
 * bounds; 2: w is (batch x N x 14).  A_out (batch x N x 14 x 14) and B_out (batch x N x 14 x 3)
 * receive the linearisation when not NULL.
 * gpmpc_tube_mc: n_samples particles per trajectory from X_nom[b, 0]; per step the plant step
 * plus noise[b, k, i, :] (batch x N x n_samples x 14, the caller's draws already times w_max);
 * tubes[b, k+1, d] = numpy's linear-method quantile of |x - X_nom[b, k+1]| over the particles
 * (virtual index (n - 1) q, _lerp with its t >= 0.5 form); NaN where a deviation is NaN.
 * gpmpc_tube_plan (no device): k_tile = the horizon steps one pass of the linear kernel takes,
 * mc_cap = the largest n_samples gpmpc_tube_mc accepts.
 * -2 with gpmpc_last_error set for a null pointer, batch < 1, N < 1, dt not positive and
 * finite, eps zero or not finite, a w_mode outside 0..2, a singular J_B, n_samples outside
 * 1..mc_cap and a quantile outside [0, 1]; the context stays usable. */
int gpmpc_tube_linear(gpmpc_ctx *ctx, const double *rocket, int batch, int N, double dt, double eps,
                      const double *X_nom, const double *U_nom, const double *w, int w_mode, double w_max,
                      const double *K, double *tubes, double *A_out, double *B_out);
int gpmpc_tube_mc(gpmpc_ctx *ctx, const double *rocket, int batch, int N, int n_samples, double dt, double quantile,
                  const double *X_nom, const double *U_nom, const double *noise, double *tubes);
int gpmpc_tube_plan(int N, int n_samples, int *k_tile, int *mc_cap);

/* ---- baseline controllers and dispersed plants --------------------
 * The landings of MonteCarloSimulator.run_single (reference src/experiments/monte_carlo.py)
 * for a controller with `solve` and no `step`, under the reference's baseline controllers
 * (src/experiments/baselines.py) and, optionally, its DispersedDynamics (src/experiments/
 * dispersion.py) around the 3-DoF Euler plant m+ = m - dt alpha |u|, r+ = r + dt v,
 * v+ = v + dt (u / m + g).  One call flies batch landings from x0 (batch x 7) to termination
 * in one launch: host buffers, one upload, one read-back of the records and step counts and
 * one of the log's used rows.
 *
 * Per control step and landing: the termination tests of the fleet (records' outcomes 1..6:
 * step == max_steps, altitude < 0, m <= 1.01, |x| > 1e6 or NaN, the landing window), the
 * target x with zero velocity and altitude max(0.5, altitude - 2), the control law, the plant
 * step, the append of (x_next, commanded u).
 *   kind LQR: u = u_hover - K (x - target), u[0] clipped to [T_lo, T_hi], u[1:] to
 *     +-gimbal_max; K (batch x 3 x 7) and u_hover (batch x 3) per landing.
 *   kind PID: integral += position error x pid_dt, clipped to +-max_integral; vertical
 *     m (pid_g + Kp_z e + Ki_z I + Kd_z de) clipped to [thrust_min, thrust_max], lateral
 *     (Kp_xy e + Ki_xy I + Kd_xy de) m clipped to +-0.3 thrust_max; de = the velocity error.
 *   kind OPEN_LOOP: row min(step, n_ref - 1) of U_ref (n_ref x 3).
 * Plant: with thrust_rows != 0 the control becomes u[0] *= t[0], u[1] += t[1], u[2] += t[2],
 * u[0] *= t[3] with t = thrust_table[i + s] (landing i, plant step s = 1..max_steps;
 * thrust_rows >= batch + max_steps rows of 4); the Euler step; wind_kind 1: v += w dt with
 * w = wind_table[i + wind_step_rows[s - 1]] (wind_rows x 3), wind_kind 2: the same with w
 * times min(1, max(x[3], 10) / 100); drag != 0: when |v| > 1 on the pre-step state,
 * v -= (drag_cda[i] |v|^2 / m) (v / |v|) dt.  sim_thrust / sim_aero > 0: the fleet's
 * Monte-Carlo draws from noise (batch x max_steps x 4, gpmpc_fleet_mc_attach).
 *
 * records (batch x GPMPC_REC_LEN, the fleet layout; the solver slots 11, 12, 14, 15 are 0),
 * nsteps (batch), log (max_steps x batch x 10, step-major: x_next (7), u (3); rows past the
 * longest landing are not written; may be NULL with log = 0), kernel_ms (the launch between
 * two events, or NULL).
 * -2 with gpmpc_last_error set, before any launch, for a null pointer, batch < 1,
 * max_steps < 1, dt <= 0, an unknown kind, an empty open-loop table, a non-finite K, u_hover
 * or x0, a table shorter than its indices reach. */
#define GPMPC_BASELINE_LQR 0
#define GPMPC_BASELINE_PID 1
#define GPMPC_BASELINE_OPEN_LOOP 2
typedef struct {
  int kind;               /* GPMPC_BASELINE_* */
  int batch;
  int max_steps;          /* 300 */
  double dt;              /* 0.1 */
  double alpha;           /* 1/30 */
  double g[3];            /* -1, 0, 0 */
  double T_lo, T_hi, gimbal_max;                          /* LQR clips: 0, 6.5, 0.5 */
  double Kp_z, Ki_z, Kd_z, Kp_xy, Ki_xy, Kd_xy;           /* PIDConfig defaults */
  double max_integral, thrust_min, thrust_max, pid_dt, pid_g;
  int n_ref;              /* rows of U_ref */
  int thrust_rows;        /* 0: no thrust dispersion */
  int wind_kind;          /* 0 none, 1 table, 2 table x altitude factor */
  int wind_rows;
  int drag;               /* 0 */
  double sim_thrust, sim_aero;                            /* SimulationConfig's dispersions, 0 */
  int log;                /* 1 */
} gpmpc_baseline_config;
void gpmpc_baseline_default_config(gpmpc_baseline_config *cfg);
int gpmpc_baseline_fly(gpmpc_ctx *ctx, const gpmpc_baseline_config *cfg, const double *x0, const double *K,
                       const double *u_hover, const double *U_ref, const double *thrust_table,
                       const double *wind_table, const int *wind_step_rows, const double *drag_cda,
                       const double *noise, double *records, int *nsteps, double *log, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GPMPC_H */
