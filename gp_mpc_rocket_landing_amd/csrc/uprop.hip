// uprop.hip -- batched linear covariance propagation along MPC horizons
// (reference src/mpc/uncertainty_prop.py:117-177, UncertaintyPropagator._propagate_linear):
//
//   Sigma_{k+1} = (A_k Sigma_k) A_k^T + diag(q_k),   k = 0 .. N-1
//
// q_k is the GP variance as process noise (var * dt^2 on the velocity block,
// and on the angular-rate block for 6-DoF), A_k the discrete Jacobian of the
// nominal step.  The mean recursion does not depend on Sigma, so the host
// (or the fleet) produces every A_k and q_k first and one launch runs all
// trajectories.  One workgroup per trajectory with one thread per entry of Sigma (n_x <=
// 16: 64 threads at n_x = 7, 256 at 14), so a step is two n_x-term dot products per
// thread and two barriers; the A_k and q_k of UP_CHUNK steps are staged into LDS in one
// cooperative load, off the step chain (one global round trip per chunk, not per step).
// HBM traffic per trajectory-step: read A_k (8 n_x^2 B) and q_k (8 n_x B), write
// Sigma_{k+1} (8 n_x^2 B).
//
// For the 3-DoF model the whole recursion runs on the device (gpmpc_uprop3_linear, below):
// k_uprop3_means walks each trajectory's means with the exact GP mean at every step and
// writes the A_k, the GP's batched posterior gives the variances, k_uprop3_q turns them
// into the q_k, and k_cov_propagate does the rest.  The 14-state model over a
// StructuredRocketGP pair does the same with k_uprop6_means / k_uprop6_q
// (gpmpc_uprop6_linear, at the end).  What these kernels share with the unscented and
// Monte-Carlo propagators is in uprop.h.
#include "uprop.h"
#include "fleet6.h"

#define UP_NXMAX 16

#define UP_CHUNK 16

// NXC > 0: n_x known at compile time (7, 14): the dot products unrolled, their LDS reads in
// flight together (same terms, same order: the same bits as the runtime-n_x form)
template <int NXC>
__global__ __launch_bounds__(256) void k_cov_propagate(int N, int nx_rt, const double *__restrict__ A,
                                                       const double *__restrict__ q,
                                                       const double *__restrict__ S0, double s0_diag,
                                                       double *__restrict__ out) {
  __shared__ double sA[UP_CHUNK][UP_NXMAX][UP_NXMAX + 1];
  __shared__ double sq[UP_CHUNK][UP_NXMAX];
  __shared__ double sS[UP_NXMAX][UP_NXMAX + 1];
  __shared__ double sT[UP_NXMAX][UP_NXMAX + 1];
  const int nx = NXC > 0 ? NXC : nx_rt;
  const int b = blockIdx.x, e = threadIdx.x, nt = blockDim.x, nn = nx * nx;
  const int64_t mat = (int64_t)nn;
  const bool act = e < nn;
  const int i = act ? e / nx : 0, j = act ? e - (e / nx) * nx : 0;
  double *ob = out + (int64_t)b * (N + 1) * mat;
  if (act) {
    const double v = S0 ? S0[(int64_t)b * mat + e] : (i == j ? s0_diag : 0.0);
    sS[i][j] = v;
    ob[e] = v;
  }
  for (int k0 = 0; k0 < N; k0 += UP_CHUNK) {
    const int kc = min(UP_CHUNK, N - k0);
    const double *Ac = A + ((int64_t)b * N + k0) * mat;
    const double *qc = q + ((int64_t)b * N + k0) * nx;
    for (int t = e; t < kc * nn; t += nt) {
      const int kk = t / nn, r = t - kk * nn, ri = r / nx;
      sA[kk][ri][r - ri * nx] = Ac[t];
    }
    for (int t = e; t < kc * nx; t += nt) {
      const int kk = t / nx;
      sq[kk][t - kk * nx] = qc[t];
    }
    __syncthreads();
    for (int kk = 0; kk < kc; ++kk) {
      if (act) {  // T = A Sigma
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < (NXC > 0 ? NXC : UP_NXMAX); ++c)
          if (NXC > 0 || c < nx) t = fma(sA[kk][i][c], sS[c][j], t);
        sT[i][j] = t;
      }
      __syncthreads();
      if (act) {  // Sigma' = T A^T + diag(q)
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < (NXC > 0 ? NXC : UP_NXMAX); ++c)
          if (NXC > 0 || c < nx) t = fma(sT[i][c], sA[kk][j][c], t);
        if (i == j) t += sq[kk][i];
        ob[(int64_t)(k0 + kk + 1) * mat + e] = t;
        sS[i][j] = t;
      }
      __syncthreads();
    }
  }
}

static hipError_t launch_cov_propagate(hipStream_t s, int batch, int N, int nx, const double *A,
                                       const double *q, const double *S0, double s0_diag,
                                       double *out) {
  const dim3 g(batch), t((nx * nx + 63) / 64 * 64);
  if (nx == 7) hipLaunchKernelGGL(k_cov_propagate<7>, g, t, 0, s, N, nx, A, q, S0, s0_diag, out);
  else if (nx == 14) hipLaunchKernelGGL(k_cov_propagate<14>, g, t, 0, s, N, nx, A, q, S0, s0_diag, out);
  else hipLaunchKernelGGL(k_cov_propagate<0>, g, t, 0, s, N, nx, A, q, S0, s0_diag, out);
  return hipGetLastError();
}

extern "C" int gpmpc_cov_propagate_dev(gpmpc_ctx *ctx, int batch, int N, int nx, const double *dA,
                                       const double *dq, const double *dS0, double s0_diag,
                                       double *dout) {
  GPMPC_CHECK_ARG(ctx && dA && dq && dout && batch >= 0 && N >= 0 && nx >= 1 && nx <= UP_NXMAX);
  if (batch == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  GPMPC_HIP(launch_cov_propagate(ctx->stream, batch, N, nx, dA, dq, dS0, s0_diag, dout));
  return 0;
}

extern "C" int gpmpc_cov_propagate(gpmpc_ctx *ctx, int batch, int N, int nx, const double *A,
                                   const double *q, const double *S0, double s0_diag,
                                   double *out) {
  GPMPC_CHECK_ARG(ctx && A && q && out && batch >= 0 && N >= 0 && nx >= 1 && nx <= UP_NXMAX);
  if (batch == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t mat = (size_t)nx * nx;
  DevBuf dA, dq, dS, dout;
  GPMPC_HIP(dA.alloc(s, sizeof(double) * (size_t)batch * N * mat + 8));
  GPMPC_HIP(dq.alloc(s, sizeof(double) * (size_t)batch * N * nx + 8));
  GPMPC_HIP(dout.alloc(s, sizeof(double) * (size_t)batch * (N + 1) * mat));
  if (N > 0) {
    GPMPC_HIP(hipMemcpyAsync(dA.p, A, sizeof(double) * (size_t)batch * N * mat,
                             hipMemcpyHostToDevice, s));
    GPMPC_HIP(hipMemcpyAsync(dq.p, q, sizeof(double) * (size_t)batch * N * nx,
                             hipMemcpyHostToDevice, s));
  }
  if (S0) {
    GPMPC_HIP(dS.alloc(s, sizeof(double) * (size_t)batch * mat));
    GPMPC_HIP(hipMemcpyAsync(dS.p, S0, sizeof(double) * (size_t)batch * mat,
                             hipMemcpyHostToDevice, s));
  }
  GPMPC_HIP(launch_cov_propagate(s, batch, N, nx, dA.as<double>(), dq.as<double>(),
                                 S0 ? dS.as<double>() : nullptr, s0_diag, dout.as<double>()));
  GPMPC_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * (size_t)batch * (N + 1) * mat,
                           hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---------------------------------------------------------------------------
// UncertaintyPropagator._propagate_linear (uncertainty_prop.py:117-177) for the 3-DoF model
// on the device, batch trajectories at once (gpmpc_uprop3_linear).  The mean recursion is
// sequential -- x_k+1 needs the GP mean at x_k -- so one workgroup per trajectory walks the
// N steps: the query's features (features3, the fleet's), the exact GP mean over the n
// training rows (256 threads, a fixed-order block reduction), the explicit-Euler step of
// rocket_3dof.py (x + dt f, f = [-alpha |u|, v, u / m + g], products and sums unfused as
// numpy forms them) plus dt d_v on the velocity rows, and A_k = I + dt J(x_k, u_k).  The
// variances of all B N queries then come from the GP's own batched posterior, and one
// launch propagates every covariance (k_cov_propagate).
#define NX 7      // the 3-DoF model's sizes (features3, internal.h): state, control,
#define NU 3      // GP features
#define NFEAT 11
__global__ __launch_bounds__(256) void k_uprop3_means(GpView g, int N, double dt, double alpha, double g0,
                                                      double g1, double g2, const double *__restrict__ x0,
                                                      const double *__restrict__ U, double *__restrict__ Q,
                                                      double *__restrict__ A, double *__restrict__ means) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double sx[NX], sz[NFEAT], szn, red[4][3];
  __shared__ double sU[UP_NCAP * NU];
  const bool reg = g.n <= 256 * UP_R3;
  GpRows<NFEAT, UP_R3> rows;
  gp_rows_load(g, reg, rows);
  const double *Ub = up_controls(U, b, N, sU);
  if (tid < NX) {
    sx[tid] = x0[(int64_t)b * NX + tid];
    means[(int64_t)b * (N + 1) * NX + tid] = sx[tid];
  }
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    const double *u = Ub + k * NU;
    if (tid == 0) {
      double z[NFEAT];
      szn = up3_query_row(g, sx, u, z, sz);
      for (int f = 0; f < NFEAT; ++f) Q[((int64_t)b * N + k) * NFEAT + f] = z[f];
    } else if (tid >= 64 && tid < 64 + NX * NX) {
      // A_k = I + dt J: J[1:4, 4:7] = I, J[4:7, 0] = -u / m^2 (rocket_3dof.py jacobian_x), one entry a thread
      const int e = tid - 64, r = e / NX, c = e - r * NX;
      double v = (r == c) ? 1.0 : 0.0;
      if (r >= 1 && r <= 3 && c == r + 3) v = __dmul_rn(1.0, dt);
      if (r >= 4 && c == 0) v = __dmul_rn(-u[r - 4] / __dmul_rn(sx[0], sx[0]), dt);
      A[((int64_t)b * N + k) * NX * NX + e] = v;
    }
    __syncthreads();
    gp_rows_means<NFEAT, UP_R3, 1, 1, 3>(g, reg, rows, sz, &szn, &red[0][0], 3, 0);
    __syncthreads();
    if (tid == 0) {
      double dv[3];
      for (int c = 0; c < 3; ++c) {
        const double m = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        dv[c] = __dadd_rn(__dmul_rn(m, g.ystd[c]), g.ymean[c]);
      }
      // x + dt f(x, u), then + d_v dt on the velocity rows
      const double g3[3] = {g0, g1, g2};
      double xn[NX];
      up3_euler(sx, u, alpha, g3, dt, xn);
      for (int c = 0; c < 3; ++c) xn[4 + c] = __dadd_rn(xn[4 + c], __dmul_rn(dv[c], dt));
      for (int i = 0; i < NX; ++i) {
        sx[i] = xn[i];
        means[((int64_t)b * (N + 1) + k + 1) * NX + i] = xn[i];
      }
    }
    __syncthreads();
  }
}

// q_k = var dt^2 on the velocity rows (uncertainty_prop.py:160-161)
__global__ void k_uprop3_q(int P, double dt2, const double *__restrict__ var, double *__restrict__ q) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  for (int i = 0; i < NX; ++i) q[(int64_t)j * NX + i] = (i >= 4) ? __dmul_rn(var[(int64_t)j * 3 + i - 4], dt2) : 0.0;
}

extern "C" int gpmpc_uprop3_linear(gpmpc_ctx *ctx, gpmpc_gp *gp, int batch, int N, double dt, double alpha,
                                   const double *g3, const double *x0, const double *U, const double *S0,
                                   double s0_diag, double *means, double *covs) {
  GPMPC_CHECK_ARG(ctx && gp && g3 && x0 && U && means && covs && batch >= 0 && N >= 0);
  GpView g;
  if (up_view3(gp, 1, "uprop3_linear", "exact GP", g)) return -2;
  if (batch == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch, P = B * N;
  DevBuf dQ, dA, dq, dvar, dmu;
  GPMPC_HIP(dQ.alloc(s, sizeof(double) * (P * NFEAT + 1)));
  GPMPC_HIP(dA.alloc(s, sizeof(double) * (P * NX * NX + 1)));
  GPMPC_HIP(dq.alloc(s, sizeof(double) * (P * NX + 1)));
  // inputs in one pinned upload, means and covariances in one read-back
  Stage sg(s);
  UpIo io(sg, B, N, NX, x0, U, S0, means, covs);
  if (int rc = sg.commit("uprop3_linear")) return rc;
  hipLaunchKernelGGL(k_uprop3_means, dim3(batch), dim3(256), 0, s, g, N, dt, alpha, g3[0], g3[1], g3[2], io.x0, io.U,
                     dQ.as<double>(), dA.as<double>(), io.means);
  GPMPC_HIP(hipGetLastError());
  if (P) {
    GPMPC_HIP(dmu.alloc(s, sizeof(double) * P * 3));
    GPMPC_HIP(dvar.alloc(s, sizeof(double) * P * 3));
    const int rc = up_posterior(ctx, gp, 1, NFEAT, dQ.as<double>(), P, dmu.as<double>(), dvar.as<double>(), P);
    if (rc) return rc;
    hipLaunchKernelGGL(k_uprop3_q, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (int)P, dt * dt,
                       dvar.as<double>(), dq.as<double>());
    GPMPC_HIP(hipGetLastError());
  }
  const int rc = gpmpc_cov_propagate_dev(ctx, batch, N, NX, dA.as<double>(), dq.as<double>(), io.S0, s0_diag, io.covs);
  if (rc) return rc;
  GPMPC_HIP(sg.download());
  return 0;
}

// ---------------------------------------------------------------------------
// UncertaintyPropagator._propagate_linear (uncertainty_prop.py:117-177) for the 14-state
// model over a StructuredRocketGP pair, batch trajectories at once (gpmpc_uprop6_linear).
// One workgroup per trajectory walks the N steps: the raw features of (x_k, u_k) (six
// roles on six lanes, r6_features_role with unit length-scales) and -[A_d | B_d] at
// (x_k, u_k) (r6_neg_lin, one lane of wave 1) side by side; then the features scaled by
// each GP's length-scales (the k_scale_rows arithmetic), both GPs' means over their rows
// (all threads, a fixed-order reduction), and on thread 0 the RK4 step with quaternion
// normalisation (rocket_6dof.py step) plus dt d_v / dt d_w on the velocity / rate rows.
// The variances of all B N queries then come from each GP's batched posterior, and one
// launch propagates every covariance (k_cov_propagate).
__global__ __launch_bounds__(256) void k_uprop6_means(GpView gv, GpView gw, R6Rocket rk, int N, double dt,
                                                      const double *__restrict__ x0, const double *__restrict__ U,
                                                      double *__restrict__ Qv, double *__restrict__ Qw,
                                                      double *__restrict__ A, double *__restrict__ means) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double sx[R6_NX], sxn[R6_NX], qv[13], qw[12], zv[13], zw[12], red[4][6];
  __shared__ double blk[R6_NX * R6_SZ];
  __shared__ double sU[UP_NCAP * R6_NU];
  // this thread's row of each GP (row tid), held in registers for the N steps when both
  // GPs have at most 256 rows (FITC inducing sets); else read per step
  const bool reg = gv.n <= 256 && gw.n <= 256;
  GpRows<13, 1> rv;
  GpRows<12, 1> rw;
  gp_rows_load(gv, reg, rv);
  gp_rows_load(gw, reg, rw);
  const double *Ub = up_controls(U, b, N, sU);
  if (tid < R6_NX) {
    sx[tid] = x0[(int64_t)b * R6_NX + tid];
    means[(int64_t)b * (N + 1) * R6_NX + tid] = sx[tid];
  }
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    const int64_t pk = (int64_t)b * N + k;
    const double *su = Ub + k * R6_NU;
    // the raw features (six roles, six lanes), -[A_d | B_d] and the nominal RK4 step, side by side
    if (tid < R6_FEAT_ROLES) {
      const double one[13] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
      r6_features_role(tid, sx, su, one, one, qv, qw);
    } else if (tid == 64) {
      for (int e = 0; e < R6_NX * R6_SZ; ++e) blk[e] = 0.0;
      r6_neg_lin(rk, sx, su, dt, blk);
    } else if (tid == 255) {
      r6_step(rk, sx, su, dt, sxn);
    }
    __syncthreads();
    if (tid < 13) {
      zv[tid] = gv.kind == GPMPC_SE_ISO ? qv[tid] : qv[tid] / gv.ls[tid];
      Qv[pk * 13 + tid] = qv[tid];
    } else if (tid >= 64 && tid < 76) {
      const int f = tid - 64;
      zw[f] = gw.kind == GPMPC_SE_ISO ? qw[f] : qw[f] / gw.ls[f];
      Qw[pk * 12 + f] = qw[f];
    } else if (tid >= 128 && tid < 128 + 98) {  // A_k = I + A_c dt = -(the block's first 14 columns)
      for (int e = tid - 128; e < R6_NX * R6_NX; e += 98) {
        const int r = e / R6_NX, c = e - r * R6_NX;
        A[pk * R6_NX * R6_NX + e] = -blk[r * R6_SZ + c];
      }
    }
    __syncthreads();
    double znv = 0.0, znw = 0.0;  // every thread forms the two squared norms itself
#pragma unroll
    for (int f = 0; f < 13; ++f) znv += zv[f] * zv[f];
#pragma unroll
    for (int f = 0; f < 12; ++f) znw += zw[f] * zw[f];
    gp_rows_means<13, 1, 1, 1, 6>(gv, reg, rv, zv, &znv, &red[0][0], 6, 0);
    gp_rows_means<12, 1, 1, 1, 6>(gw, reg, rw, zw, &znw, &red[0][0], 6, 3);
    __syncthreads();
    if (tid == 0) {
      double d[6];
      for (int c = 0; c < 6; ++c) {
        const double m = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        const GpView &g = c < 3 ? gv : gw;
        d[c] = m * g.ystd[c % 3] + g.ymean[c % 3];
      }
      double xn[R6_NX];
      for (int i = 0; i < R6_NX; ++i) xn[i] = sxn[i];
      for (int c = 0; c < 3; ++c) {
        xn[4 + c] = xn[4 + c] + d[c] * dt;
        xn[11 + c] = xn[11 + c] + d[3 + c] * dt;
      }
      for (int i = 0; i < R6_NX; ++i) {
        sx[i] = xn[i];
        means[((int64_t)b * (N + 1) + k + 1) * R6_NX + i] = xn[i];
      }
    }
    __syncthreads();
  }
}

// q_k = var dt^2 on the velocity rows 4-6 (d_v) and the rate rows 11-13 (d_omega)
__global__ void k_uprop6_q(int P, double dt2, const double *__restrict__ vv, const double *__restrict__ vw,
                           double *__restrict__ q) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  for (int i = 0; i < R6_NX; ++i) {
    double v = 0.0;
    if (i >= 4 && i < 7) v = vv[(int64_t)j * 3 + i - 4] * dt2;
    if (i >= 11) v = vw[(int64_t)j * 3 + i - 11] * dt2;
    q[(int64_t)j * R6_NX + i] = v;
  }
}

extern "C" int gpmpc_uprop6_linear(gpmpc_ctx *ctx, void *gp_v, void *gp_w, int exact, const double *rocket,
                                   int batch, int N, double dt, const double *x0, const double *U,
                                   const double *S0, double s0_diag, double *means, double *covs) {
  GPMPC_CHECK_ARG(ctx && gp_v && gp_w && rocket && x0 && U && means && covs && batch >= 0 && N >= 0);
  GpView gv, gw;
  if (up_view6(gp_v, gp_w, exact, "uprop6_linear", gv, gw)) return -2;
  R6Rocket rk{};
  if (r6_rocket(rocket, rk, "uprop6_linear")) return -2;
  if (batch == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch, P = B * N;
  DevBuf dQv, dQw, dA, dq, mv, vv, mw, vw;
  GPMPC_HIP(dQv.alloc(s, sizeof(double) * (P * 13 + 1)));
  GPMPC_HIP(dQw.alloc(s, sizeof(double) * (P * 12 + 1)));
  GPMPC_HIP(dA.alloc(s, sizeof(double) * (P * R6_NX * R6_NX + 1)));
  GPMPC_HIP(dq.alloc(s, sizeof(double) * (P * R6_NX + 1)));
  // inputs in one pinned upload, means and covariances in one read-back
  Stage sg(s);
  UpIo io(sg, B, N, R6_NX, x0, U, S0, means, covs);
  if (int rc = sg.commit("uprop6_linear")) return rc;
  hipLaunchKernelGGL(k_uprop6_means, dim3(batch), dim3(256), 0, s, gv, gw, rk, N, dt, io.x0, io.U, dQv.as<double>(),
                     dQw.as<double>(), dA.as<double>(), io.means);
  GPMPC_HIP(hipGetLastError());
  if (P) {
    for (DevBuf *d : {&mv, &vv, &mw, &vw}) GPMPC_HIP(d->alloc(s, sizeof(double) * P * 3));
    int rc = up_posterior(ctx, gp_v, exact, 13, dQv.as<double>(), P, mv.as<double>(), vv.as<double>(), P);
    if (rc) return rc;
    rc = up_posterior(ctx, gp_w, exact, 12, dQw.as<double>(), P, mw.as<double>(), vw.as<double>(), P);
    if (rc) return rc;
    hipLaunchKernelGGL(k_uprop6_q, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (int)P, dt * dt,
                       vv.as<double>(), vw.as<double>(), dq.as<double>());
    GPMPC_HIP(hipGetLastError());
  }
  const int rc = gpmpc_cov_propagate_dev(ctx, batch, N, R6_NX, dA.as<double>(), dq.as<double>(), io.S0, s0_diag,
                                         io.covs);
  if (rc) return rc;
  GPMPC_HIP(sg.download());
  return 0;
}
