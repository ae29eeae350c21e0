// qp.hip -- batched OSQP-style ADMM: one workgroup (256 threads) per QP.
//
// Replaces the osqp.OSQP() setup / update(q) / update(l, u, Ax) / warm_start(x)
// / solve() sequence of OSQPRTIMPC (osqp_rti.py:454-567) for a whole batch of
// QPs that share one sparsity pattern.  The pattern is pre-processed once on
// the host (CSR -> CSC map, banded-KKT product terms) and shared by every
// workgroup; the numeric data of each problem is staged into LDS.
#include "internal.h"
#include "qp.h"
#include "qp_pattern.h"
#include <algorithm>
#include <cstdlib>
#include <vector>

extern "C" void gpmpc_qp_default_settings(gpmpc_qp_settings *s) {
  // osqp_rti.py:54-60 (max_iter 50, eps 1e-4, polish off, warm start, scaling 3)
  // + OSQP 0.6 defaults pinned, adaptive-rho interval fixed at 25.
  s->rho = 0.1;
  s->sigma = 1e-6;
  s->alpha = 1.6;
  s->eps_abs = 1e-4;
  s->eps_rel = 1e-4;
  s->eps_prim_inf = 1e-4;
  s->eps_dual_inf = 1e-4;
  s->max_iter = 50;
  s->check_termination = 25;
  s->adaptive_rho = 1;
  s->adaptive_rho_interval = 25;
  s->adaptive_rho_tolerance = 5.0;
  s->scaling = 3;
  s->warm_start = 1;
}

QPSettingsDev to_dev(const gpmpc_qp_settings &s) {
  QPSettingsDev d;
  d.rho = s.rho; d.sigma = s.sigma; d.alpha = s.alpha; d.eps_abs = s.eps_abs;
  d.eps_rel = s.eps_rel; d.eps_prim_inf = s.eps_prim_inf; d.eps_dual_inf = s.eps_dual_inf;
  d.max_iter = s.max_iter; d.check_termination = s.check_termination;
  d.adaptive_rho = s.adaptive_rho; d.adaptive_rho_interval = s.adaptive_rho_interval;
  d.adaptive_rho_tolerance = s.adaptive_rho_tolerance; d.scaling = s.scaling;
  d.warm_start = s.warm_start;
  return d;
}

int QPPatternHost::build(int n_, int m_, const int *rowptr, const int *colidx, hipStream_t s) {
  const QPPatternPlan pl = qp_pattern_analyze(n_, m_, rowptr, colidx);  // host only (qp_pattern.h)
  n = pl.n; m = pl.m; nnz = pl.nnz; w = pl.w; maxrow = pl.maxrow; maxcol = pl.maxcol;
  mode = pl.mode; fac_len = pl.fac_len; nblk = pl.nblk;
  if (buf.alloc(sizeof(int) * pl.all.size()) != hipSuccess) return -1;
  if (hipMemcpyAsync(buf.p, pl.all.data(), sizeof(int) * pl.all.size(), hipMemcpyHostToDevice, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return -1;
  const int *d = buf.as<int>();
  dev.n = n; dev.m = m; dev.nnz = nnz; dev.w = w;
  dev.rowptr = d + pl.o_rp; dev.colidx = d + pl.o_ci; dev.colptr = d + pl.o_cp; dev.csc2csr = d + pl.o_cm;
  dev.cscrow = d + pl.o_cr; dev.facptr = d + pl.o_bp; dev.facdiag = d + pl.o_fd; dev.terms = d + pl.o_tv;
  dev.mode = mode; dev.fac_len = fac_len; dev.nblk = nblk; dev.bsz = QP_BLK_SZ; dev.bcm = QP_BLK_CM;
  dev.offd = reinterpret_cast<const int4 *>(d + pl.o_od);
  dev.n_offd = pl.n_offd;
  return 0;
}

// the refusals of a malformed pattern: what qp_pattern_analyze may index with
static bool qp_pattern_well_formed(int n, int m, const int *rowptr, const int *colidx) {
  if (n <= 0 || m <= 0 || !rowptr || !colidx || rowptr[0] != 0) return false;
  for (int r = 0; r < m; ++r)
    if (rowptr[r + 1] < rowptr[r]) return false;
  for (int k = 0; k < rowptr[m]; ++k)
    if (colidx[k] < 0 || colidx[k] >= n) return false;
  return true;
}

// which factor path a pattern takes, without a context or a device (include/gpmpc.h)
extern "C" int gpmpc_qp_pattern_info(int n, int m, const int *rowptr, const int *colidx, int *info) {
  GPMPC_CHECK_ARG(info && qp_pattern_well_formed(n, m, rowptr, colidx));
  const QPPatternPlan pl = qp_pattern_analyze(n, m, rowptr, colidx);
  QPPatternHost h;
  h.n = pl.n; h.m = pl.m; h.nnz = pl.nnz; h.w = pl.w; h.maxrow = pl.maxrow; h.maxcol = pl.maxcol;
  h.mode = pl.mode; h.fac_len = pl.fac_len; h.nblk = pl.nblk;
  const int out[GPMPC_QP_PATTERN_INFO_INTS] = {pl.mode, pl.w, pl.nblk, pl.fac_len, pl.maxrow, pl.maxcol,
                                               pl.n_offd, h.fits() ? 1 : 0,
                                               qp_is_fleet_pattern(n, m, rowptr, colidx) ? 1 : 0};
  std::copy(out, out + GPMPC_QP_PATTERN_INFO_INTS, info);
  return 0;
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_qp_batched(QPPattern pt, QPSettingsDev st,
                                                    const double *__restrict__ Aval,
                                                    const double *__restrict__ Pd,
                                                    const double *__restrict__ q,
                                                    const double *__restrict__ l,
                                                    const double *__restrict__ u,
                                                    const double *__restrict__ xws, double *rho,
                                                    double *yst, double *xo, double *yo,
                                                    int *iters, int *status, double *obj,
                                                    unsigned long long *stamps) {
  __shared__ QPSmemStd s;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = pt.n, m = pt.m, nnz = pt.nnz;
  for (int k = tid; k < nnz; k += nt) s.A[k] = Aval[(int64_t)b * nnz + k];
  for (int j = tid; j < n; j += nt) {
    s.P[j] = Pd[(int64_t)b * n + j];
    s.q[j] = q[(int64_t)b * n + j];
    s.x[j] = xws ? xws[(int64_t)b * n + j] : 0.0;
  }
  for (int r = tid; r < m; r += nt) {
    s.l[r] = l[(int64_t)b * m + r];
    s.u[r] = u[(int64_t)b * m + r];
    s.y[r] = yst[(int64_t)b * m + r];
  }
  if (tid == 0) s.rho_s = rho[b];
  __syncthreads();
  QPStamps T;
  if (b == 0) T.out = stamps;  // (GPMPC_QP_STAMPS: problem 0's phase cycles)
  T.start();
  QPResult res = qp_solve(pt, s, st, &T);
  T.mark(7);
  T.flush();
  if (res.factor_fail) {
    if (tid == 0) { status[b] = -100; iters[b] = 0; obj[b] = nan(""); }
    return;
  }
  const bool has = (res.status == 1 || res.status == 2 || res.status == -2);
  for (int j = tid; j < n; j += nt) xo[(int64_t)b * n + j] = has ? s.D[j] * s.x[j] : nan("");
  for (int r = tid; r < m; r += nt) {
    yo[(int64_t)b * m + r] = has ? s.E[r] * s.y[r] / s.c : nan("");
    yst[(int64_t)b * m + r] = s.y[r];
  }
  if (tid == 0) {
    rho[b] = s.rho_s;
    iters[b] = res.iter;
    status[b] = res.status;
    obj[b] = has ? res.obj : nan("");
  }
}

hipError_t launch_qp_batched(hipStream_t s, const QPPattern &pt, const QPSettingsDev &st,
                             int batch, const double *Aval, const double *Pd, const double *q,
                             const double *l, const double *u, const double *xws, double *rho,
                             double *yst, double *xo, double *yo, int *iters, int *status,
                             double *obj, unsigned long long *stamps = nullptr) {
  hipLaunchKernelGGL(k_qp_batched, dim3(batch), dim3(256), 0, s, pt, st, Aval, Pd, q, l, u, xws,
                     rho, yst, xo, yo, iters, status, obj, stamps);
  return hipGetLastError();
}

// The last pattern of each stream, kept: a caller that re-solves one pattern (the OSQP
// workspace, QPWorkspace.solve, once per control step) pays its host pre-processing,
// upload and the upload's synchronisation once instead of per solve.
#include <map>
#include <memory>
#include <mutex>
struct QPPatCache {
  std::vector<int> rowptr, colidx;
  int n = 0;
  std::unique_ptr<QPPatternHost> pat;
};
static std::mutex g_qpcache_mu;
static std::map<hipStream_t, QPPatCache> g_qpcache;

void gpmpc_qp_cache_release(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_qpcache_mu);
  g_qpcache.erase(s);
}

static QPPatternHost *qp_pattern(hipStream_t s, int n, int m, const int *rowptr, const int *colidx) {
  std::lock_guard<std::mutex> lk(g_qpcache_mu);
  QPPatCache &c = g_qpcache[s];
  const int nnz = rowptr[m];
  if (c.pat && c.n == n && (int)c.rowptr.size() == m + 1 && (int)c.colidx.size() == nnz &&
      !memcmp(c.rowptr.data(), rowptr, sizeof(int) * (m + 1)) &&
      !memcmp(c.colidx.data(), colidx, sizeof(int) * nnz))
    return c.pat.get();
  c.pat.reset();
  auto pat = std::make_unique<QPPatternHost>();
  if (pat->build(n, m, rowptr, colidx, s)) return nullptr;
  c.rowptr.assign(rowptr, rowptr + m + 1);
  c.colidx.assign(colidx, colidx + nnz);
  c.n = n;
  c.pat = std::move(pat);
  return c.pat.get();
}

static int qp_cu_count(int dev) {
  static int cus[64] = {0};
  if (dev < 0 || dev >= 64) return 0;
  if (!cus[dev]) (void)hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev);
  return cus[dev];
}

extern "C" int gpmpc_qp_solve_batched(gpmpc_ctx *ctx, int batch, int n, int m, int nnz,
                                      const int *rowptr, const int *colidx, const double *Aval,
                                      const double *Pdiag, const double *q, const double *l,
                                      const double *u, const gpmpc_qp_settings *st,
                                      const double *x_ws, double *rho, double *y_scaled,
                                      double *x, double *y, int *iters, int *status,
                                      double *obj) {
  GPMPC_CHECK_ARG(ctx && rowptr && colidx && Aval && Pdiag && q && l && u && st && rho &&
                  y_scaled && x && y && iters && status && obj);
  GPMPC_CHECK_ARG(batch >= 0 && n > 0 && m > 0 && nnz == rowptr[m]);
  GPMPC_CHECK_ARG(n <= QP_NMAX && m <= QP_MMAX && nnz <= QP_NNZMAX);
  if (batch == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const QPPatternHost *pat = qp_pattern(s, n, m, rowptr, colidx);
  if (!pat) {
    gpmpc_set_error("qp: pattern upload failed");
    return -1;
  }
  if (!pat->fits()) {
    gpmpc_set_error("qp: pattern outside the compiled caps (n %d<=%d, m %d<=%d, half-bandwidth "
                    "%d<=%d, row nnz %d<=%d, col nnz %d<=%d)", pat->n, QP_NMAX, pat->m, QP_MMAX, pat->w,
                    QP_W, pat->maxrow, QP_RMAX, pat->maxcol, QP_CMAX);
    return -2;
  }
  // The fleet's solver (fleet_qp.h, registers + twisted KKT solve) for its own pattern -- the
  // 3-DoF MPC at N = 20 -- when the dynamics rows are equalities, as that solver assumes
  // (GPMPC_QP_FLEET=0: always the generic kernel).  The same OSQP iteration; the block-wide
  // sums and the KKT solve round differently from the generic kernel's.
  const bool fleet_env = gpmpc_env_int("GPMPC_QP_FLEET", 1) != 0;  // (read per call: tests switch it)
  bool fleet = fleet_env && qp_is_fleet_pattern(n, m, rowptr, colidx);
  for (int64_t r = 0; fleet && r < (int64_t)batch * m; ++r)
    if (r % m < QP_FLEET_MD && l[r] != u[r]) fleet = false;
  // every input in one pinned upload, every output in one read-back
  const size_t B = batch;
  Stage sg(s);
  const double *dA, *dP, *dq, *dl, *du, *dx0;  // dx0 null without a warm start
  double *drho, *dy0, *dxo, *dyo, *dob;
  int *dit, *dst;
  sg.in(&dA, Aval, B * nnz); sg.in(&dP, Pdiag, B * n); sg.in(&dq, q, B * n);
  sg.in(&dl, l, B * m); sg.in(&du, u, B * m);
  sg.in(&dx0, x_ws, B * n);
  sg.inout(&drho, rho, B); sg.inout(&dy0, y_scaled, B * m);
  sg.out(&dxo, x, B * n); sg.out(&dyo, y, B * m);
  sg.out(&dit, iters, B); sg.out(&dst, status, B);
  sg.out(&dob, obj, B);
  if (int rc = sg.commit("qp")) return rc;
  // GPMPC_QP_STAMPS=1: problem 0's phase cycles (s_memtime) to stderr, a diagnostic
  static const int stamp = gpmpc_env_int("GPMPC_QP_STAMPS", 0);
  DevBuf dts;
  if (stamp) {
    GPMPC_HIP(dts.alloc(s, 16 * sizeof(unsigned long long)));
    GPMPC_HIP(hipMemsetAsync(dts.p, 0, 16 * sizeof(unsigned long long), s));
  }
  if (fleet) {
    GPMPC_HIP((batch <= qp_cu_count(ctx->device) ? fq_wide::launch_qp : fq_narrow::launch_qp)(
        s, batch, pat->dev, to_dev(*st), dA, dP, dq, dl, du, dx0, drho, dy0, dxo, dyo, dit, dst, dob));
  } else {
    GPMPC_HIP(launch_qp_batched(s, pat->dev, to_dev(*st), batch, dA, dP, dq, dl, du, dx0, drho, dy0, dxo, dyo,
                                dit, dst, dob, dts.as<unsigned long long>()));
  }
  GPMPC_HIP(sg.download());
  // a failed factorisation (-100) returns before the kernels write x and y: without this the
  // caller would read whatever the staging buffer held, e.g. an earlier solve's solution
  for (int b = 0; b < batch; ++b)
    if (status[b] == -100) {
      std::fill(x + (size_t)b * n, x + (size_t)(b + 1) * n, nan(""));
      std::fill(y + (size_t)b * m, y + (size_t)(b + 1) * m, nan(""));
    }
  if (stamp) {
    unsigned long long h[16];
    GPMPC_HIP(hipMemcpy(h, dts.p, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "qp_stamps iter %d:", iters[0]);
    for (int k = 0; k < 16; ++k) fprintf(stderr, " %llu", h[k]);
    fprintf(stderr, "\n");
  }
  return 0;
}
