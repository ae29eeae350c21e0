// uprop.h -- what the linear (uprop.hip), unscented (uprop_ut.hip) and Monte-Carlo
// (uprop_mc.hip) uncertainty propagators share: the GP mean a workgroup forms inside a
// kernel, the 3-DoF model's step and query row, where a step's controls are read from, and
// the host set-up of the entry points (GP views, the posterior, the staged buffers).
#pragma once
#include "internal.h"
#include <algorithm>

#define UP_NCAP 256  // horizon steps whose controls a propagation kernel stages in LDS
#define UP_R3 4      // 3-DoF: training rows per thread held in registers (n <= 1024); larger n reads them per step

// ---- device: the GP mean over a workgroup of 256 threads ---------------------------------
// this thread's rows j = tid + 256 r of a GP: scaled features, squared norm, alpha.  Loaded
// once (reg: the GP has at most 256 R rows), the sequential steps then read no global
// memory on their critical path; a larger GP reads its rows per step
template <int D, int R>
struct GpRows {
  double x[R][D], xn[R], a[R][3];
};

template <int D, int R>
__device__ __forceinline__ void gp_rows_load(const GpView &g, bool reg, GpRows<D, R> &w) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = tid + 256 * r;
    const bool ok = reg && j < g.n;
#pragma unroll
    for (int f = 0; f < D; ++f) w.x[r][f] = ok ? g.Xs[(int64_t)j * D + f] : 0.0;
    w.xn[r] = ok ? g.Xn[j] : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) w.a[r][c] = ok ? g.alphaT[(int64_t)c * g.n + j] : 0.0;
  }
}

// the GP's latent means (alpha^T k*) at the P scaled query rows sz (P x D, squared norms
// szn): per-wave partials into red[wave * ldr + p * G + c0 + c], C points a pass.  The
// caller adds the four waves' partials in the order ((r0 + r1) + r2) + r3
template <int D, int R, int P, int C, int G>
__device__ __forceinline__ void gp_rows_means(const GpView &g, bool reg, const GpRows<D, R> &w,
                                              const double *sz, const double *szn, double *red, int ldr,
                                              int c0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll 1
  for (int p0 = 0; p0 < P; p0 += C) {
    double acc[C][3];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c][0] = acc[c][1] = acc[c][2] = 0.0;
    if (reg) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (p0 + c >= P) continue;
        double z[D];
#pragma unroll
        for (int f = 0; f < D; ++f) z[f] = sz[(p0 + c) * D + f];
        const double zn = szn[p0 + c];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (tid + 256 * r < g.n) {
            double dot = 0.0;
#pragma unroll
            for (int f = 0; f < D; ++f) dot = fma(z[f], w.x[r][f], dot);
            const double kv = kernel_epilogue(g.kind, (zn + w.xn[r]) - 2.0 * dot, g.sigma2, g.iso_scale);
#pragma unroll
            for (int o = 0; o < 3; ++o) acc[c][o] = fma(kv, w.a[r][o], acc[c][o]);
          }
        }
      }
    } else {
      for (int j = tid; j < g.n; j += 256) {
        double xr[D], ar[3];
#pragma unroll
        for (int f = 0; f < D; ++f) xr[f] = g.Xs[(int64_t)j * D + f];
        const double xn = g.Xn[j];
#pragma unroll
        for (int o = 0; o < 3; ++o) ar[o] = g.alphaT[(int64_t)o * g.n + j];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if (p0 + c >= P) continue;
          double dot = 0.0;
#pragma unroll
          for (int f = 0; f < D; ++f) dot = fma(sz[(p0 + c) * D + f], xr[f], dot);
          const double kv = kernel_epilogue(g.kind, (szn[p0 + c] + xn) - 2.0 * dot, g.sigma2, g.iso_scale);
#pragma unroll
          for (int o = 0; o < 3; ++o) acc[c][o] = fma(kv, ar[o], acc[c][o]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (p0 + c >= P) continue;
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        double v = acc[c][o];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
        if (lane == 0) red[wave * ldr + (p0 + c) * G + c0 + o] = v;
      }
    }
  }
}

// ---- device: the 3-DoF model ---------------------------------------------------------------
// rocket_3dof.py's explicit-Euler step xn = x + dt f(x, u), f = [-alpha |u|, v, u / m + g]:
// products and sums unfused, as numpy forms them
__device__ __forceinline__ void up3_euler(const double *x, const double *u, double alpha, const double *g3,
                                          double dt, double *xn) {
#pragma clang fp contract(off)
  const double um = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(u[0], u[0]), __dmul_rn(u[1], u[1])), __dmul_rn(u[2], u[2])));
  double f[7];
  f[0] = __dmul_rn(-alpha, um);
  f[1] = x[4]; f[2] = x[5]; f[3] = x[6];
  f[4] = __dadd_rn(u[0] / x[0], g3[0]); f[5] = __dadd_rn(u[1] / x[0], g3[1]); f[6] = __dadd_rn(u[2] / x[0], g3[2]);
#pragma unroll
  for (int i = 0; i < 7; ++i) xn[i] = __dadd_rn(x[i], __dmul_rn(dt, f[i]));
}

// the 3-DoF GP's query row of (x, u): the raw features into z, over the GP's length-scales
// into v, the squared norm of v returned
__device__ __forceinline__ double up3_query_row(const GpView &g, const double *x, const double *u, double *z,
                                                double *v) {
  features3(x, u, z);
  double sn = 0.0;
#pragma unroll
  for (int f = 0; f < 11; ++f) {
    const double s = g.kind == GPMPC_SE_ISO ? z[f] : z[f] / g.ls[f];
    v[f] = s;
    sn += s * s;
  }
  return sn;
}

// ---- device: where a step's controls come from -------------------------------------------
// Trajectory b's N x 3 controls: staged into sU (UP_NCAP x 3, LDS) by the whole workgroup
// when N <= UP_NCAP -- no global round trip on the step chain -- else read where they are.
// Step k's controls are the returned pointer + 3 k, after the caller's next barrier.
__device__ __forceinline__ const double *up_controls(const double *__restrict__ U, int b, int N, double *sU) {
  const bool uc = N <= UP_NCAP;
  for (int e = threadIdx.x; uc && e < N * 3; e += 256) sU[e] = U[(int64_t)b * N * 3 + e];
  return uc ? sU : U + (int64_t)b * N * 3;
}

// ---- host: the entry points' set-up -------------------------------------------------------
// the view of a GP given as (handle, exact): an exact GP's, or a FITC GP's inducing rows
static inline GpView up_view(void *gp, int exact) {
  return exact ? gp_view((gpmpc_gp *)gp) : fitc_view((gpmpc_fitc *)gp);
}

// the 3-DoF GP's view, checked (gp_word: how the message names what the call takes, "GP" or
// "exact GP"); W2: a sparse GP's fitc_W2, null for an exact one.  0, or -2 with the error set
static inline int up_view3(void *gp, int exact, const char *what, const char *gp_word, GpView &g,
                           const double **W2 = nullptr) {
  g = up_view(gp, exact);
  if (g.d != 11 || g.n_out != 3 || g.kind == GPMPC_KPROG) {
    gpmpc_set_error("%s: needs the 3-DoF %s (11 features, 3 outputs, a leaf kernel)", what, gp_word);
    return -2;
  }
  if (W2) *W2 = exact ? nullptr : fitc_W2((gpmpc_fitc *)gp);
  return 0;
}

// the same for the 14-state model's StructuredRocketGP pair (d_v, d_omega)
static inline int up_view6(void *gp_v, void *gp_w, int exact, const char *what, GpView &gv, GpView &gw,
                           const double **W2v = nullptr, const double **W2w = nullptr) {
  gv = up_view(gp_v, exact);
  gw = up_view(gp_w, exact);
  if (gv.d != 13 || gw.d != 12 || gv.n_out != 3 || gw.n_out != 3 || gv.kind == GPMPC_KPROG ||
      gw.kind == GPMPC_KPROG) {
    gpmpc_set_error("%s: needs the StructuredRocketGP pair (13 / 12 features, 3 outputs, leaf kernels)", what);
    return -2;
  }
  if (W2v) *W2v = exact ? nullptr : fitc_W2((gpmpc_fitc *)gp_v);
  if (W2w) *W2w = exact ? nullptr : fitc_W2((gpmpc_fitc *)gp_w);
  return 0;
}

// the posterior of P device-resident raw query rows (P x d) of a GP given as (handle,
// exact): mean / var (P x 3), chunk rows a call (bounds K* at 8 n chunk bytes)
static inline int up_posterior(gpmpc_ctx *ctx, void *gp, int exact, int d, const double *dq, size_t P, double *dmean,
                               double *dvar, size_t chunk) {
  for (size_t c0 = 0; c0 < P; c0 += chunk) {
    const int pc = (int)std::min(chunk, P - c0);
    const int rc = exact ? gp_posterior_dev(ctx, (gpmpc_gp *)gp, dq + c0 * d, pc, dmean + c0 * 3, dvar + c0 * 3)
                         : fitc_posterior_dev(ctx, (gpmpc_fitc *)gp, dq + c0 * d, pc, dmean + c0 * 3, dvar + c0 * 3);
    if (rc) return rc;
  }
  return 0;
}

// what every propagation call stages: x0 (B x n), U (B x N x 3) and S0 (B x n x n, or null)
// up, means (B x (N+1) x n) and covs (B x (N+1) x n x n) back.  The constructor declares them
// and the Stage's commit fills in the device pointers (so an UpIo stays where it was made).  A
// caller with inputs of its own declares them first, with outputs of its own after (Stage's
// order of use).
struct UpIo {
  const double *x0, *U, *S0;
  double *means, *covs;
  UpIo(Stage &sg, size_t B, size_t N, size_t n, const double *hx0, const double *hU, const double *hS0,
       double *hmeans, double *hcovs) {
    sg.in(&x0, hx0, B * n);
    sg.in(&U, hU, B * N * 3);
    sg.in(&S0, hS0, B * n * n);
    sg.out(&means, hmeans, B * (N + 1) * n);
    sg.out(&covs, hcovs, B * (N + 1) * n * n);
  }
  UpIo(const UpIo &) = delete;
};
