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
// into the q_k, and k_cov_propagate does the rest.
#include "internal.h"

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
#define UP3_R 4  // training rows per thread held in registers (n <= 1024); larger n reads them per step
#define UP_NCAP 256  // horizon steps whose controls the propagation kernels stage in LDS
__global__ __launch_bounds__(256) void k_uprop3_means(GpView g, int N, double dt, double alpha, double g0,
                                                      double g1, double g2, const double *__restrict__ x0,
                                                      const double *__restrict__ U, double *__restrict__ Q,
                                                      double *__restrict__ A, double *__restrict__ means) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double sx[NX], sz[NFEAT], szn, red[4][3];
  // this thread's training rows j = tid + 256 r (scaled features, |x_j|^2, alpha), loaded once:
  // the N sequential steps then read no global memory on their critical path
  const bool reg = g.n <= 256 * UP3_R;
  double xr[UP3_R][NFEAT], xnr[UP3_R], ar[UP3_R][3];
#pragma unroll
  for (int r = 0; r < UP3_R; ++r) {
    const int j = tid + 256 * r;
    const bool ok = reg && j < g.n;
#pragma unroll
    for (int f = 0; f < NFEAT; ++f) xr[r][f] = ok ? g.Xs[(int64_t)j * NFEAT + f] : 0.0;
    xnr[r] = ok ? g.Xn[j] : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) ar[r][c] = ok ? g.alphaT[(int64_t)c * g.n + j] : 0.0;
  }
  // the trajectory's controls staged in LDS once (up to UP_NCAP steps): no global
  // round trip on the step chain
  __shared__ double sU[UP_NCAP * NU];
  const bool uc = N <= UP_NCAP;
  for (int e = tid; uc && e < N * NU; e += 256) sU[e] = U[(int64_t)b * N * NU + e];
  const double *Ub = uc ? sU : U + (int64_t)b * N * NU;
  if (tid < NX) {
    sx[tid] = x0[(int64_t)b * NX + tid];
    means[(int64_t)b * (N + 1) * NX + tid] = sx[tid];
  }
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    const double *u = Ub + k * NU;
    if (tid == 0) {
      double z[NFEAT];
      features3(sx, u, z);
      double sn = 0.0;
      for (int f = 0; f < NFEAT; ++f) {
        Q[((int64_t)b * N + k) * NFEAT + f] = z[f];
        const double v = g.kind == GPMPC_SE_ISO ? z[f] : z[f] / g.ls[f];
        sz[f] = v;
        sn += v * v;
      }
      szn = sn;
    } else if (tid >= 64 && tid < 64 + NX * NX) {
      // A_k = I + dt J: J[1:4, 4:7] = I, J[4:7, 0] = -u / m^2 (rocket_3dof.py jacobian_x), one entry a thread
      const int e = tid - 64, r = e / NX, c = e - r * NX;
      double v = (r == c) ? 1.0 : 0.0;
      if (r >= 1 && r <= 3 && c == r + 3) v = __dmul_rn(1.0, dt);
      if (r >= 4 && c == 0) v = __dmul_rn(-u[r - 4] / __dmul_rn(sx[0], sx[0]), dt);
      A[((int64_t)b * N + k) * NX * NX + e] = v;
    }
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};
    const double zn = szn;
    if (reg) {
      double zv[NFEAT];
#pragma unroll
      for (int f = 0; f < NFEAT; ++f) zv[f] = sz[f];
#pragma unroll
      for (int r = 0; r < UP3_R; ++r) {
        if (tid + 256 * r >= g.n) break;
        double dot = 0.0;
#pragma unroll
        for (int f = 0; f < NFEAT; ++f) dot = fma(zv[f], xr[r][f], dot);
        const double kv = kernel_epilogue(g.kind, (zn + xnr[r]) - 2.0 * dot, g.sigma2, g.iso_scale);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fma(kv, ar[r][c], acc[c]);
      }
    } else {
      for (int j = tid; j < g.n; j += 256) {
        double dot = 0.0;
#pragma unroll
        for (int f = 0; f < NFEAT; ++f) dot = fma(sz[f], g.Xs[(int64_t)j * NFEAT + f], dot);
        const double kv = kernel_epilogue(g.kind, (zn + g.Xn[j]) - 2.0 * dot, g.sigma2, g.iso_scale);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fma(kv, g.alphaT[(int64_t)c * g.n + j], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
    if (lane == 0)
      for (int c = 0; c < 3; ++c) red[wave][c] = acc[c];
    __syncthreads();
    if (tid == 0) {
      double dv[3];
      for (int c = 0; c < 3; ++c) {
        const double m = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        dv[c] = __dadd_rn(__dmul_rn(m, g.ystd[c]), g.ymean[c]);
      }
      // x + dt f(x, u), then + d_v dt on the velocity rows
      const double um = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(u[0], u[0]), __dmul_rn(u[1], u[1])), __dmul_rn(u[2], u[2])));
      double f[NX];
      f[0] = __dmul_rn(-alpha, um);
      f[1] = sx[4]; f[2] = sx[5]; f[3] = sx[6];
      f[4] = __dadd_rn(u[0] / sx[0], g0); f[5] = __dadd_rn(u[1] / sx[0], g1); f[6] = __dadd_rn(u[2] / sx[0], g2);
      double xn[NX];
      for (int i = 0; i < NX; ++i) xn[i] = __dadd_rn(sx[i], __dmul_rn(dt, f[i]));
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
  const GpView g = gp_view(gp);
  if (g.d != NFEAT || g.n_out != 3 || g.kind == GPMPC_KPROG) {
    gpmpc_set_error("uprop3_linear: needs the 3-DoF exact GP (11 features, 3 outputs, a leaf kernel)");
    return -2;
  }
  if (batch == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch, P = B * N;
  DevBuf dQ, dA, dq, dvar, dmu;
  GPMPC_HIP(dQ.alloc(s, sizeof(double) * (P * NFEAT + 1)));
  GPMPC_HIP(dA.alloc(s, sizeof(double) * (P * NX * NX + 1)));
  GPMPC_HIP(dq.alloc(s, sizeof(double) * (P * NX + 1)));
  // inputs in one pinned upload, means and covariances in one read-back
  const size_t bytes = Stage::pad(8 * B * NX) + Stage::pad(8 * P * NU) + (S0 ? Stage::pad(8 * B * NX * NX) : 0) +
                       Stage::pad(8 * B * (N + 1) * NX) + Stage::pad(8 * B * (N + 1) * NX * NX);
  Stage sg(s, bytes);
  if (!sg.ok()) {
    gpmpc_set_error("uprop3_linear: staging buffers: out of memory");
    return -1;
  }
  const double *dx0 = sg.in(x0, B * NX), *dU = sg.in(U, P * NU);
  const double *dS0 = S0 ? sg.in(S0, B * NX * NX) : nullptr;
  double *dmeans = sg.out(means, B * (N + 1) * NX), *dcov = sg.out(covs, B * (N + 1) * NX * NX);
  GPMPC_HIP(sg.upload());
  hipLaunchKernelGGL(k_uprop3_means, dim3(batch), dim3(256), 0, s, g, N, dt, alpha, g3[0], g3[1], g3[2], dx0, dU,
                     dQ.as<double>(), dA.as<double>(), dmeans);
  GPMPC_HIP(hipGetLastError());
  if (P) {
    GPMPC_HIP(dmu.alloc(s, sizeof(double) * P * 3));
    GPMPC_HIP(dvar.alloc(s, sizeof(double) * P * 3));
    const int rc = gp_posterior_dev(ctx, gp, dQ.as<double>(), (int)P, dmu.as<double>(), dvar.as<double>());
    if (rc) return rc;
    hipLaunchKernelGGL(k_uprop3_q, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (int)P, dt * dt,
                       dvar.as<double>(), dq.as<double>());
    GPMPC_HIP(hipGetLastError());
  }
  const int rc = gpmpc_cov_propagate_dev(ctx, batch, N, NX, dA.as<double>(), dq.as<double>(), dS0, s0_diag, dcov);
  if (rc) return rc;
  GPMPC_HIP(sg.download());
  return 0;
}
