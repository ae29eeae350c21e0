// uprop_mc.hip -- Monte-Carlo uncertainty propagation along MPC horizons on the device
// (reference src/mpc/uncertainty_prop.py:266-315, UncertaintyPropagator._propagate_monte_carlo),
// batch trajectories of n_samples particles in one call, for the 3-DoF model
// (gpmpc_uprop3_mc) and the 14-state model (gpmpc_uprop6_mc).
//
// The particles never meet again after Sigma_0 and a step's statistics feed nothing back, so
// every particle of every trajectory is an independent query of the same GP at step k: one
// horizon step of the whole batch is one posterior at P = batch * n_samples points, the shape
// gp_posterior_dev / fitc_posterior_dev serve on the MFMA loop (W read once per step for all
// particles, no cap on its row count).  The call is step-synchronous on ctx->stream:
//   k_mc_step(-1): particles0 into row 0 of the paths, the raw features of (x_0, u_0);
//   per step k:    the posterior of the P feature rows (one GP, or the d_v / d_omega pair);
//                  k_mc_step(k): a lane per particle p = b S + i: the nominal step (explicit
//                  Euler with the unfused expressions of k_uprop3_means / r6_step), then
//                  + (d + sqrt(var) z) dt on rows 4:7 (and 11:14) rounded as numpy rounds it,
//                  the new state into paths[b, k+1, i, :], the raw features of
//                  (x_k+1, u_k+1) for the next posterior;
//   k_mc_stats:    once after the loop, a workgroup per (b, k): the sample mean with the sum
//                  sequential in particle order (the bits of np.mean(axis=0)) and the sample
//                  covariance over S - 1, its lower triangle mirrored; row 0 is x0 / Sigma_0.
// The draws (particles0, the standard normals) are the caller's: numpy's global RNG in the
// reference's order, so a seed means what it means there.  The only synchronisation is the
// final read-back.
#include "uprop.h"
#include "fleet6.h"
#include <algorithm>
#include <climits>

#define MC_T 128          // k_mc_step: lanes (particles) per workgroup
#define MC_ST 128         // k_mc_stats: threads per workgroup (>= 14 * 15 / 2 entries)
#define MC_CH 32          // k_mc_stats: particles staged in LDS at a time
#define MC_PCHUNK 65536   // query rows per posterior call (bounds K* at 8 n MC_PCHUNK bytes)

struct McArgs {
  R6Rocket rk;          // 14-state model
  double alpha, g3[3];  // 3-DoF model
  int B, N, S;
  double dt;
  const double *U, *particles0, *normals;
  const double *mv, *vv, *mw, *vw;  // the posterior at step k's particles (P x 3; mw / vw: d_omega)
  double *paths;                    // B x (N + 1) x S x n
  double *Qv, *Qw;                  // raw feature rows of the next posterior (P x 11 | P x 13, P x 12)
};

// x + (d + sqrt(var) z) dt: sqrt(var) z rounded, then the sum, then the product with dt, then
// the sum into the nominal row (numpy: nxt[:, rows] += (d + np.sqrt(var) * z) * dt)
__device__ __forceinline__ double mc_residual(double x, double d, double var, double z, double dt) {
#pragma clang fp contract(off)
  return __dadd_rn(x, __dmul_rn(__dadd_rn(d, __dmul_rn(sqrt(var), z)), dt));
}

// MODEL 3: the 7-state explicit-Euler model over one GP (11 features); MODEL 6: the 14-state
// RK4 model over the StructuredRocketGP pair (13 / 12 features).  k = -1: no step, the
// features of the initial particles only.
template <int MODEL>
__global__ __launch_bounds__(MC_T) void k_mc_step(McArgs a, int k) {
  constexpr int n = MODEL == 3 ? 7 : 14, G = MODEL == 3 ? 1 : 2;
  const int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x;
  if (p >= (int64_t)a.B * a.S) return;
  const int b = (int)(p / a.S), i = (int)(p - (int64_t)b * a.S);
  const int N = a.N;
  const double dt = a.dt;
  double x[n];
  if (k < 0) {
#pragma unroll
    for (int r = 0; r < n; ++r) x[r] = a.particles0[p * n + r];
  } else {
    const double *xp = a.paths + (((int64_t)b * (N + 1) + k) * a.S + i) * n;
    const double *u = a.U + ((int64_t)b * N + k) * 3;
    const double *z = a.normals + (((int64_t)b * N + k) * a.S + i) * (G * 3);
    double xc[n];
#pragma unroll
    for (int r = 0; r < n; ++r) xc[r] = xp[r];
    if (MODEL == 3) {
      up3_euler(xc, u, a.alpha, a.g3, dt, x);
    } else {
      r6_step(a.rk, xc, u, dt, x);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x[4 + c] = mc_residual(x[4 + c], a.mv[p * 3 + c], a.vv[p * 3 + c], z[c], dt);
      if (MODEL == 6) x[11 + c] = mc_residual(x[11 + c], a.mw[p * 3 + c], a.vw[p * 3 + c], z[3 + c], dt);
    }
  }
  double *xo = a.paths + (((int64_t)b * (N + 1) + k + 1) * a.S + i) * n;
#pragma unroll
  for (int r = 0; r < n; ++r) xo[r] = x[r];
  if (k + 1 >= N) return;
  // the raw feature rows of (x_k+1, u_k+1): the posterior scales them by its own length-scales
  const double *un = a.U + ((int64_t)b * N + k + 1) * 3;
  if (MODEL == 3) {
    double q[11];
    features3(x, un, q);
#pragma unroll
    for (int f = 0; f < 11; ++f) a.Qv[p * 11 + f] = q[f];
  } else {
    const double one[13] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    double qv[13], qw[12];
#pragma unroll
    for (int role = 0; role < R6_FEAT_ROLES; ++role) r6_features_role(role, x, un, one, one, qv, qw);
#pragma unroll
    for (int f = 0; f < 13; ++f) a.Qv[p * 13 + f] = qv[f];
#pragma unroll
    for (int f = 0; f < 12; ++f) a.Qw[p * 12 + f] = qw[f];
  }
}

// The sample statistics of step k of trajectory b, a workgroup per (b, k), the particles going
// by through LDS in chunks of MC_CH (coalesced reads; every thread then walks the chunk in
// particle order).  Thread r < n: means[b, k, r] = (((p_0 + p_1) + p_2) + ...) / S.  Thread
// e < n (n + 1) / 2: entry (i, j <= i) of sum_p d_p d_p^T / (S - 1), d_p = x_p - mean, written
// to (i, j) and (j, i).  k = 0: x0 and Sigma_0 (or s0_diag I), not a sample statistic.
template <int n>
__global__ __launch_bounds__(MC_ST) void k_mc_stats(int N, int S, const double *__restrict__ x0,
                                                    const double *__restrict__ S0, double s0_diag,
                                                    const double *__restrict__ paths, double *__restrict__ means,
                                                    double *__restrict__ covs) {
  constexpr int T = n * (n + 1) / 2;
  static_assert(T <= MC_ST, "an entry of the triangle per thread");
  const int b = blockIdx.x / (N + 1), k = blockIdx.x - b * (N + 1), tid = threadIdx.x;
  double *mb = means + ((int64_t)b * (N + 1) + k) * n, *cb = covs + ((int64_t)b * (N + 1) + k) * n * n;
  if (k == 0) {
    if (tid < n) mb[tid] = x0[(int64_t)b * n + tid];
    for (int e = tid; e < n * n; e += MC_ST) {
      const int i = e / n, j = e - i * n;
      cb[e] = S0 ? S0[(int64_t)b * n * n + e] : (i == j ? s0_diag : 0.0);
    }
    return;
  }
  __shared__ double sp[MC_CH * n], sm[n];
  const double *pk = paths + ((int64_t)b * (N + 1) + k) * S * n;
  double s = 0.0;
  for (int p0 = 0; p0 < S; p0 += MC_CH) {
    const int pc = min(MC_CH, S - p0);
    __syncthreads();
    for (int e = tid; e < pc * n; e += MC_ST) sp[e] = pk[(int64_t)p0 * n + e];
    __syncthreads();
    if (tid < n)
      for (int q = 0; q < pc; ++q) s = __dadd_rn(s, sp[q * n + tid]);
  }
  if (tid < n) {
    s = s / (double)S;
    sm[tid] = s;
    mb[tid] = s;
  }
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= tid) ++i;
  const int j = tid - i * (i + 1) / 2;
  const bool act = tid < T;
  double c = 0.0;
  for (int p0 = 0; p0 < S; p0 += MC_CH) {
    const int pc = min(MC_CH, S - p0);
    __syncthreads();  // (the first trip: sm is written; later trips: the chunk has been read)
    for (int e = tid; e < pc * n; e += MC_ST) sp[e] = pk[(int64_t)p0 * n + e];
    __syncthreads();
    if (act)
      for (int q = 0; q < pc; ++q) c = fma(__dsub_rn(sp[q * n + i], sm[i]), __dsub_rn(sp[q * n + j], sm[j]), c);
  }
  if (act) {
    c = c / (double)(S - 1);
    cb[i * n + j] = c;
    cb[j * n + i] = c;
  }
}

template <int MODEL>
static int mc_run(gpmpc_ctx *ctx, McArgs &a, const char *what, void *gp_v, void *gp_w, int exact, int batch, int N,
                  int n_samples, const double *x0, const double *U, const double *S0, double s0_diag,
                  const double *particles0, const double *normals, double *means, double *covs,
                  double *particles) {
  constexpr size_t n = MODEL == 3 ? 7 : 14, G = MODEL == 3 ? 1 : 2, DV = MODEL == 3 ? 11 : 13, DW = 12;
  if (batch == 0) return 0;
  const size_t B = batch, S = n_samples, P = B * S, NP = (size_t)N + 1;
  if (P > (size_t)INT_MAX / MC_T || B * NP > (size_t)INT_MAX) {
    gpmpc_set_error("%s: batch * n_samples = %zu particles is more than one call takes", what, P);
    return -2;
  }
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // inputs in one pinned upload; means, covariances (and the paths, when asked for) in one read-back
  const size_t npath = B * NP * S * n;
  DevBuf paths, dQv, dQw, mv, vv, mw, vw;
  GPMPC_HIP(dQv.alloc(s, sizeof(double) * (P * DV + 1)));
  for (DevBuf *d : {&mv, &vv}) GPMPC_HIP(d->alloc(s, sizeof(double) * P * 3));
  if (MODEL == 6) {
    GPMPC_HIP(dQw.alloc(s, sizeof(double) * (P * DW + 1)));
    for (DevBuf *d : {&mw, &vw}) GPMPC_HIP(d->alloc(s, sizeof(double) * P * 3));
  }
  if (!particles) GPMPC_HIP(paths.alloc(s, sizeof(double) * npath));
  Stage sg(s);
  sg.in(&a.particles0, particles0, P * n);
  sg.in(&a.normals, normals, B * N * S * G * 3);
  UpIo io(sg, B, N, n, x0, U, S0, means, covs);
  // the paths: read back when the caller asks for them, else a pooled temporary
  if (particles) sg.out(&a.paths, particles, npath);
  else a.paths = paths.as<double>();
  a.B = batch; a.N = N; a.S = n_samples;
  a.Qv = dQv.as<double>(); a.Qw = dQw.as<double>();
  a.mv = mv.as<double>(); a.vv = vv.as<double>(); a.mw = mw.as<double>(); a.vw = vw.as<double>();
  if (int rc = sg.commit(what)) return rc;
  a.U = io.U;
  const dim3 grid((unsigned)((P + MC_T - 1) / MC_T));
  for (int k = -1; k < N; ++k) {
    if (k >= 0) {
      int rc = up_posterior(ctx, gp_v, exact, DV, dQv.as<double>(), P, mv.as<double>(), vv.as<double>(), MC_PCHUNK);
      if (rc) return rc;
      if (MODEL == 6)
        rc = up_posterior(ctx, gp_w, exact, DW, dQw.as<double>(), P, mw.as<double>(), vw.as<double>(), MC_PCHUNK);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(k_mc_step<MODEL>, grid, dim3(MC_T), 0, s, a, k);
    GPMPC_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_mc_stats<(int)n>, dim3((unsigned)(B * NP)), dim3(MC_ST), 0, s, N, n_samples, io.x0, io.S0,
                     s0_diag, a.paths, io.means, io.covs);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}

extern "C" int gpmpc_uprop3_mc(gpmpc_ctx *ctx, void *gp, int exact, int batch, int N, int n_samples, double dt,
                               double alpha, const double *g3, const double *x0, const double *U, const double *S0,
                               double s0_diag, const double *particles0, const double *normals, double *means,
                               double *covs, double *particles) {
  GPMPC_CHECK_ARG(ctx && gp && g3 && x0 && U && particles0 && normals && means && covs && batch >= 0 && N >= 0 &&
                  n_samples >= 2);
  GpView g;
  if (up_view3(gp, exact, "uprop3_mc", "GP", g)) return -2;
  McArgs a{};
  a.alpha = alpha;
  for (int i = 0; i < 3; ++i) a.g3[i] = g3[i];
  a.dt = dt;
  return mc_run<3>(ctx, a, "uprop3_mc", gp, nullptr, exact, batch, N, n_samples, x0, U, S0, s0_diag, particles0,
                   normals, means, covs, particles);
}

extern "C" int gpmpc_uprop6_mc(gpmpc_ctx *ctx, void *gp_v, void *gp_w, int exact, const double *rocket, int batch,
                               int N, int n_samples, double dt, const double *x0, const double *U, const double *S0,
                               double s0_diag, const double *particles0, const double *normals, double *means,
                               double *covs, double *particles) {
  GPMPC_CHECK_ARG(ctx && gp_v && gp_w && rocket && x0 && U && particles0 && normals && means && covs && batch >= 0 &&
                  N >= 0 && n_samples >= 2);
  GpView gv, gw;
  if (up_view6(gp_v, gp_w, exact, "uprop6_mc", gv, gw)) return -2;
  McArgs a{};
  if (r6_rocket(rocket, a.rk, "uprop6_mc")) return -2;
  a.dt = dt;
  return mc_run<6>(ctx, a, "uprop6_mc", gp_v, gp_w, exact, batch, N, n_samples, x0, U, S0, s0_diag, particles0,
                   normals, means, covs, particles);
}
