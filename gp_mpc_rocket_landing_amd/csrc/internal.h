// internal.h -- shared helpers for libgpmpc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include "../../include/gpmpc.h"
#include "stage.h"

struct gpmpc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
};

void gpmpc_set_error(const char *fmt, ...);
// The one reader of the GPMPC_* switches: atoi of the variable (empty or non-numeric: 0), dflt when
// unset.  Read once per process: `static const int v = gpmpc_env_int(...)`; per call: a plain call.
int gpmpc_env_int(const char *name, int dflt);
// persistent scratch per stream (= per context; slots: 0 trsm block inverses,
// 1 potrf 32x32 inverses, 2 potrf 128x128 inverses, 3 batched-LML Gram/factor
// matrices, 4 gp_append temporaries, 5 split-K partials, 7 the Stage device arena; slots 0..7).  Valid until the next call
// on the same stream that asks the slot for more bytes.
#define GPMPC_SCRATCH_SLOTS 8
void *gpmpc_scratch(hipStream_t s, int slot, size_t bytes);

#define GPMPC_HIP(call)                                                               \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                           \
      gpmpc_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return -1;                                                                      \
    }                                                                                 \
  } while (0)

#define GPMPC_CHECK_ARG(cond)                                    \
  do {                                                           \
    if (!(cond)) {                                               \
      gpmpc_set_error("%s:%d bad argument: %s", __FILE__, __LINE__, #cond); \
      return -2;                                                 \
    }                                                            \
  } while (0)

// Per-stream caching pool for the temporaries of host-boundary calls (fits, predicts,
// solves): a released block goes back to its stream's free list instead of hipFree
// (an implicit device-wide synchronisation, ~41 us a call: ~15 per exact fit, DESIGN
// §11).  A block is handed out again only on the stream it was last used on, so that
// stream's order keeps its earlier readers ahead of the next writer.  Blocks are sized
// in classes (<= 12.5% rounding), cached up to a per-stream cap (GPMPC_POOL_CAP_MB, 8 GB),
// and released with the context (gpmpc_ctx_destroy); a failed hipMalloc first gives the
// stream's cached blocks back and retries.  gen: the pool generation the block came from
// (a block returned after its context's destruction is freed, not cached).
void *gpmpc_pool_get(hipStream_t s, size_t bytes, size_t *cls, uint64_t *gen);
void gpmpc_pool_put(hipStream_t s, void *p, size_t cls, uint64_t gen);

// RAII device buffer (host-side bookkeeping only).  alloc(bytes): its own hipMalloc
// (handle-owned state that outlives the call); alloc(stream, bytes): a pooled
// temporary of that stream.
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  hipStream_t pool = nullptr;  // non-null: pooled on this stream
  size_t cls = 0;
  uint64_t gen = 0;            // the pool generation it came from
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) {
      if (pool) gpmpc_pool_put(pool, p, cls, gen);
      else (void)hipFree(p);
    }
    p = nullptr;
    pool = nullptr;
  }
  hipError_t alloc(size_t b) {
    release();
    bytes = b;
    return b ? hipMalloc(&p, b) : hipSuccess;
  }
  hipError_t alloc(hipStream_t s, size_t b) {
    release();
    bytes = b;
    if (!b) return hipSuccess;
    p = gpmpc_pool_get(s, b, &cls, &gen);
    if (!p) return hipErrorOutOfMemory;
    pool = s;
    return hipSuccess;
  }
  void swap(DevBuf &o) {
    std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(pool, o.pool); std::swap(cls, o.cls);
    std::swap(gen, o.gen);
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

// Staging for the host-buffer entry points: a call packs its inputs into one pinned
// arena and uploads them with ONE copy, and places its outputs in one device range
// read back with ONE copy (a pageable hipMemcpyAsync costs 10-30 us of host time; a
// single-landing QP solve made 14 of them).  The arenas are per stream (= per
// context; device side = gpmpc_scratch slot 7), grown after the stream drains, and
// valid until the next Stage on the stream.  Order of use: declare every buffer once
// (stage.h: in(&dev, host, count), then inout(), then out()); commit(what) sizes both
// arenas from the declarations, packs the inputs, writes every declared device pointer
// and uploads; download() after the last kernel (it synchronises the stream).
char *gpmpc_stage_host(hipStream_t s, size_t bytes);
void gpmpc_qp_cache_release(hipStream_t s);  // qp.hip: the stream's kept QP pattern
struct Stage : StageLayout {
  hipStream_t s;
  char *h = nullptr, *d = nullptr;
  explicit Stage(hipStream_t st) : s(st) {}
  // 0, or -1 with the error set and no declared pointer written
  int commit(const char *what) {
    if (refused) {
      gpmpc_set_error("%s: staging buffers: %s", what, refused);
      return -1;
    }
    h = gpmpc_stage_host(s, total);
    d = (char *)gpmpc_scratch(s, 7, total);
    if (!h || !d) {
      gpmpc_set_error("%s: staging buffers: out of memory", what);
      return -1;
    }
    pack(h);
    bind(d);
    // the whole arena goes up, outputs included (trimming it to the inputs is a speed change of its own)
    if (total) GPMPC_HIP(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, s));
    return 0;
  }
  hipError_t download() {
    if (back_lo != kNone) {
      hipError_t e = hipMemcpyAsync(h + back_lo, d + back_lo, total - back_lo, hipMemcpyDeviceToHost, s);
      if (e != hipSuccess) return e;
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    fetch(h);
    return hipSuccess;
  }
};

// kernel value from r^2 of the length-scaled rows (the k_gram epilogue; shared
// so that every kernel that forms K*(x, x') produces the same bits)
__device__ __forceinline__ double kernel_epilogue(int kind, double d2, double sigma2,
                                                  double iso_scale) {
  d2 = d2 > 0.0 ? d2 : 0.0;  // np.maximum(dist_sq, 0.0)
  switch (kind) {
    case GPMPC_SE_ARD: return sigma2 * exp(-0.5 * d2);
    case GPMPC_SE_ISO: return sigma2 * exp(-d2 * iso_scale);
    case GPMPC_MATERN32: {
      double r = sqrt(d2);
      double s3 = 1.7320508075688772 * r;
      return sigma2 * (1.0 + s3) * exp(-s3);
    }
    default: {
      double r = sqrt(d2);
      double s5 = 2.23606797749979 * r;
      return sigma2 * (1.0 + s5 + 5.0 * (r * r) / 3.0) * exp(-s5);
    }
  }
}

// Simple3DoFFeatureExtractor.extract (features.py:403-444)
__device__ __forceinline__ void features3(const double *x, const double *u, double *z) {
  const double vx = x[4], vy = x[5], vz = x[6], alt = x[1];
  const double speed = sqrt(vx * vx + vy * vy + vz * vz);
  const double rho = 1.225 * exp(-alt / 8500.0);
  const double qd = 0.5 * rho * speed * speed;
  const double tm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  z[0] = vx / 10.0; z[1] = vy / 10.0; z[2] = vz / 10.0; z[3] = speed / 10.0;
  z[4] = qd / (0.5 * 1.225 * 100.0);
  z[5] = u[0] / 10.0; z[6] = u[1] / 10.0; z[7] = u[2] / 10.0; z[8] = tm / 10.0;
  z[9] = alt / 100.0; z[10] = rho / 1.225;
}

// The linearisation plans of a 3-DoF fleet (fleet.hip), for kernels that form the GP
// query rows themselves: row g = slot * N + k is horizon point k of landing order[slot]
// (or of landing slot without a dispatch order).  Xw null: no plans.
struct FleetPlans {
  const double *Xw, *Uw, *ls;
  const int *order;
  int N, iso;
};

// Query row g of the plans: its 11 features over the lengthscales into v, the squared
// norm returned.  The one place this arithmetic lives, so every kernel that forms the
// rows (k_fleet_queries, k_fleet_queries_gram, k_gram_rows) produces the same bits.
__device__ __forceinline__ double fleet_query_row(const FleetPlans &p, int g, double *v) {
  const int sl = g / p.N, k = g - sl * p.N;
  const int b = p.order ? p.order[sl] : sl;
  double z[11];
  features3(p.Xw + ((int64_t)b * (p.N + 1) + k) * 7, p.Uw + ((int64_t)b * p.N + k) * 3, z);
  double s = 0.0;
#pragma unroll
  for (int f = 0; f < 11; ++f) {
    v[f] = p.iso ? z[f] : z[f] / p.ls[f];
    s += v[f] * v[f];
  }
  return s;
}

// ---- internal device entry points shared across translation units ----------
// Gram: K (n1 x n2, ldk) from pre-scaled rows (a = X1/ls, b = X2/ls) and their
// squared norms; kind selects the epilogue.  With plans (row-tiled kernel only, see
// gram_rows_tiled) the a-rows are the fleet's query rows, formed in the kernel: a and na
// are not read.
hipError_t launch_gram(hipStream_t s, int kind, const double *a, const double *na, int n1,
                       const double *b, const double *nb, int n2, int d, double sigma2,
                       double iso_scale, double *K, int64_t ldk, int transpose_out,
                       const FleetPlans *plans = nullptr);
// launch_gram takes the row-tiled kernel (k_gram_rows) for this shape, row-major output
bool gram_rows_tiled(int n1, int d);
#define GPMPC_KPROG 16  // GpCore kind of a composite-kernel program
// composite kernel programs (gram.hip; codes GPMPC_KP_* in gpmpc.h): Gram of raw rows,
// same = 1: one row set (X2 ignored; WhiteNoise on the diagonal)
hipError_t launch_gram_prog(hipStream_t s, const int *ops, int nops, const double *par, const double *X1, int n1,
                            const double *X2, int n2, int d, int same, double *K, int64_t ldk);
int kprog_check(const int *ops, int nops, int npar, int d, const double *par, double *diag);
// rows / lengthscales -> scaled rows + squared norms
hipError_t launch_scale_rows(hipStream_t s, const double *X, int n, int d, const double *ls,
                             int iso, double *out, double *norms);
// blocked Cholesky of batch matrices; info (device int[batch]), 1-based pivot
hipError_t launch_potrf_batched(hipStream_t s, int n, int batch, double *A, int64_t lda,
                                int64_t stride, int *info);
// info < 0 from the blocked Cholesky: the 128-column diagonal kernel's bounded wait
// for an LDS step flag expired (a broken invariant, not a non-PD matrix); the factor of
// that matrix is unreliable and is never reported as success or as a pivot column
#define GPMPC_POTRF_SWEEP_TIMEOUT (-1)
int gpmpc_potrf_info_error(int info, const char *what);  // sets the message, returns the code
// X <- L^-1 X (L lower n x n, X n x nrhs row-major ld ldx), batch via strides
hipError_t launch_trsm_lower(hipStream_t s, int n, int nrhs, const double *L, int64_t ldl,
                             double *X, int64_t ldx, int transpose_L);
// add value to the diagonal of A
hipError_t launch_add_diag(hipStream_t s, int n, double *A, int64_t lda, double v, int batch,
                           int64_t stride);
// copy lower triangle of src into dst and zero the strict upper part of dst
hipError_t launch_copy_lower(hipStream_t s, int n, const double *src, int64_t lds, double *dst,
                             int64_t ldd);

// read-only view of a fitted exact GP (gp.hip) for the fleet
struct GpView {
  int kind, n, d, n_out;
  double sigma2, iso_scale;
  const double *ls, *Xs, *Xn, *W, *alphaT, *ymean, *ystd;
  const double *Wf, *Xp;  // column-stationary posterior operands (post.hip), or null
};
GpView gp_view(const gpmpc_gp *gp);
// the exact GP's posterior of p device-resident raw query rows (gp.hip): mean / var (p x n_out)
int gp_posterior_dev(gpmpc_ctx *ctx, gpmpc_gp *gp, const double *dq, int p, double *dmean, double *dvar);
// the same for a FITC GP (gp.hip, the gpmpc_fitc_predict arithmetic)
int fitc_posterior_dev(gpmpc_ctx *ctx, gpmpc_fitc *gp, const double *dq, int p, double *dmean, double *dvar);
// the same view of a FITC GP: n = inducing points, Xs / Xn their scaled rows, alphaT
GpView fitc_view(const gpmpc_fitc *gp);
// its W2 = L_B^-1 L_uu^-1 (n x n lower): the predict's w = W2 k* (sparse_gp.py:293-296)
const double *fitc_W2(const gpmpc_fitc *gp);
// the sparse posterior finish (k_fitc_finish): var = sigma2 - sum pv + sum pw, mean
hipError_t launch_fitc_finish(hipStream_t s, int P, int n_out, int nrv, int nrw, const double *pv,
                              const double *pw, int64_t ldp, const double *meanT, int64_t ldm,
                              const double *ymean, const double *ystd, double sigma2, double *mean,
                              double *var);
// posterior finish: var/mean (P x n_out) from SUMSQ partials and K* alpha (gp.hip)
hipError_t launch_post_finish(hipStream_t s, int P, int n_out, int nrt, const double *part,
                              int64_t ldp, const double *meanT, int64_t ldm, const double *ymean,
                              const double *ystd, double sigma2, double *mean, double *var);
