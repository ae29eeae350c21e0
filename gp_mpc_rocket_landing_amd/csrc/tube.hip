// tube.hip -- tube MPC's uncertainty tubes on the device (reference src/safety/tube_mpc.py:
// TubePropagator.propagate_linear / propagate_with_gp / _linearize and propagate_monte_carlo),
// batch trajectories in one call (gpmpc_tube_linear, gpmpc_tube_mc; gpmpc_tube_plan on the CPU).
//
// The nominal trajectory is given, so the 18 plant steps of every finite-difference
// linearisation (the nominal step, 14 state and 3 control perturbations) of every horizon step
// of every trajectory are independent; only e_(k+1) = |A_cl| e_k + w_k is serial.  Mapping
// (DESIGN §20):
//   k_tube_linear: one workgroup of 256 lanes per trajectory, the horizon in passes of
//     TB_KTILE = 14 steps.  A pass: lane t < 18 * steps runs plant step (t / 18, t % 18) with
//     r6_step and leaves its 14 numbers in LDS; after a barrier all lanes form the 196 entries
//     per step of |A_cl| = |A + B K| (A, B: the differences divided by eps, a true division) in
//     LDS (and write A / B out when asked); after a second barrier the first wave runs the
//     row recursion, lane r < 14 holding e[r] and reading e[j] of the others by __shfl.
//     The rocket and the scalars are kernel arguments, K is copied to LDS once.
//   k_tube_mc: one workgroup per trajectory, one lane per particle, the particle's state in
//     registers over the whole horizon.  Per step and dimension the lanes publish their
//     deviation |x - x_nom| to LDS (double-buffered: one barrier per dimension), every lane
//     counts its rank (ties broken by lane index), and the two lanes whose ranks are numpy's
//     lower and upper neighbour publish the order statistics; 14 lanes then interpolate with
//     numpy's _lerp.  A NaN among a dimension's deviations gives NaN for that dimension.
// Every loop bound is known at launch; no atomics, no cross-workgroup traffic, no spin-waits.
#include "fleet6.h"
#include <climits>
#include <cmath>

#define TB_T 256          // k_tube_linear: lanes per workgroup
#define TB_KTILE 14       // horizon steps per pass: 14 * 18 = 252 plant steps on 256 lanes
#define TB_COLS 18        // nominal, 14 state columns, 3 control columns
#define TB_MC_CAP 1024    // k_tube_mc: the most particles (one lane each)
static_assert(TB_KTILE * TB_COLS <= TB_T, "a pass's plant steps fit the workgroup");

struct TbArgs {
  R6Rocket rk;
  int B, N, w_mode, have_K;
  double dt, eps, w_max;
  const double *X, *U, *w, *K;
  double *tubes, *A_out, *B_out;
};

__global__ __launch_bounds__(TB_T) void k_tube_linear(const TbArgs a) {
  __shared__ double sx[TB_KTILE * TB_COLS * R6_NX];   // the plant steps of a pass
  __shared__ double sA[TB_KTILE * R6_NX * R6_NX];     // |A_cl| of a pass
  __shared__ double sK[R6_NU * R6_NX];
  const int tid = threadIdx.x, b = blockIdx.x, N = a.N;
  if (a.have_K && tid < R6_NU * R6_NX) sK[tid] = a.K[tid];
  const int r = tid < R6_NX ? tid : R6_NX - 1;       // the recursion's row (first wave)
  double e = 0.0;
  if (tid < R6_NX) a.tubes[(int64_t)b * (N + 1) * R6_NX + tid] = 0.0;
  for (int k0 = 0; k0 < N; k0 += TB_KTILE) {
    const int nt = min(TB_KTILE, N - k0);
    __syncthreads();   // the previous pass has read sA (and sK is written)
    if (tid < nt * TB_COLS) {
      const int kk = tid / TB_COLS, c = tid - kk * TB_COLS, k = k0 + kk;
      const double *xp = a.X + ((int64_t)b * (N + 1) + k) * R6_NX, *up = a.U + ((int64_t)b * N + k) * R6_NU;
      double x[R6_NX], u[R6_NU], xn[R6_NX];
#pragma unroll
      for (int i = 0; i < R6_NX; ++i) x[i] = (c == 1 + i) ? xp[i] + a.eps : xp[i];
#pragma unroll
      for (int i = 0; i < R6_NU; ++i) u[i] = (c == 1 + R6_NX + i) ? up[i] + a.eps : up[i];
      r6_step(a.rk, x, u, a.dt, xn);
#pragma unroll
      for (int i = 0; i < R6_NX; ++i) sx[tid * R6_NX + i] = xn[i];
    }
    __syncthreads();
    for (int en = tid; en < nt * R6_NX * R6_NX; en += TB_T) {
      const int kk = en / (R6_NX * R6_NX), rc = en - kk * (R6_NX * R6_NX), row = rc / R6_NX, col = rc - row * R6_NX;
      const double *s0 = sx + kk * TB_COLS * R6_NX;
      const double nom = s0[row];
      const double av = (s0[(1 + col) * R6_NX + row] - nom) / a.eps;
      if (a.A_out) a.A_out[((int64_t)b * N + k0 + kk) * (R6_NX * R6_NX) + rc] = av;
      double acl = av;
      if (a.have_K) {
        double bk = 0.0;
#pragma unroll
        for (int m = 0; m < R6_NU; ++m) bk += (s0[(1 + R6_NX + m) * R6_NX + row] - nom) / a.eps * sK[m * R6_NX + col];
        acl = av + bk;
      }
      sA[en] = fabs(acl);
    }
    if (a.B_out)
      for (int en = tid; en < nt * R6_NX * R6_NU; en += TB_T) {
        const int kk = en / (R6_NX * R6_NU), rc = en - kk * (R6_NX * R6_NU), row = rc / R6_NU, m = rc - row * R6_NU;
        const double *s0 = sx + kk * TB_COLS * R6_NX;
        a.B_out[((int64_t)b * N + k0 + kk) * (R6_NX * R6_NU) + rc] = (s0[(1 + R6_NX + m) * R6_NX + row] - s0[row]) / a.eps;
      }
    __syncthreads();
    if (tid < 64) {   // the first wave, whole (the exchange is wave-wide); lanes past 13 repeat row 13
      for (int kk = 0; kk < nt; ++kk) {
        const int k = k0 + kk;
        const double *Ar = sA + kk * (R6_NX * R6_NX) + r * R6_NX;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < R6_NX; ++j) s += Ar[j] * __shfl(e, j);
        const double wk = a.w_mode == 0 ? a.w_max : a.w_mode == 1 ? a.w[r] : a.w[((int64_t)b * N + k) * R6_NX + r];
        e = s + wk;
        if (tid < R6_NX) a.tubes[((int64_t)b * (N + 1) + k + 1) * R6_NX + tid] = e;
      }
    }
  }
}

struct TmArgs {
  R6Rocket rk;
  int B, N, S, lo, hi;       // lo / hi: numpy's previous and next index of the quantile
  double dt, gamma;          // gamma: numpy's interpolation weight
  const double *X, *U, *noise;
  double *tubes;
};

// numpy's _lerp(a, b, t): a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5, unfused
__device__ __forceinline__ double tm_lerp(double lo, double hi, double t) {
  const double d = __dsub_rn(hi, lo);
  return t >= 0.5 ? __dsub_rn(hi, __dmul_rn(d, __dsub_rn(1.0, t))) : __dadd_rn(lo, __dmul_rn(d, t));
}

template <int T>
__global__ __launch_bounds__(T) void k_tube_mc(const TmArgs a) {
  __shared__ double sd[2][T];             // a dimension's deviations, double-buffered
  __shared__ double sp[R6_NX][2];         // the two order statistics per dimension
  __shared__ int snan[R6_NX];
  const int tid = threadIdx.x, b = blockIdx.x, N = a.N, S = a.S;
  const bool live = tid < S;
  const int i = live ? tid : S - 1;       // a lane past the particles reruns the last one and publishes nothing
  double x[R6_NX];
#pragma unroll
  for (int d = 0; d < R6_NX; ++d) x[d] = a.X[(int64_t)b * (N + 1) * R6_NX + d];
  if (tid < R6_NX) a.tubes[(int64_t)b * (N + 1) * R6_NX + tid] = 0.0;
  for (int k = 0; k < N; ++k) {
    const double *u = a.U + ((int64_t)b * N + k) * R6_NU;
    const double *z = a.noise + (((int64_t)b * N + k) * S + i) * R6_NX;
    const double *xn = a.X + ((int64_t)b * (N + 1) + k + 1) * R6_NX;
    double y[R6_NX], dev[R6_NX];
    r6_step(a.rk, x, u, a.dt, y);
#pragma unroll
    for (int d = 0; d < R6_NX; ++d) {
      x[d] = __dadd_rn(y[d], z[d]);
      dev[d] = fabs(__dsub_rn(x[d], xn[d]));
    }
#pragma unroll 1
    for (int d = 0; d < R6_NX; ++d) {
      double mine = dev[0];
#pragma unroll
      for (int q = 1; q < R6_NX; ++q) mine = d == q ? dev[q] : mine;
      double *buf = sd[d & 1];
      if (live) buf[tid] = mine;
      __syncthreads();
      int rank = 0;
      bool nan = false;
      for (int j = 0; j < S; ++j) {
        const double v = buf[j];
        nan = nan || v != v;
        rank += (v < mine || (v == mine && j < tid)) ? 1 : 0;
      }
      if (live && !nan) {
        if (rank == a.lo) sp[d][0] = mine;
        if (rank == a.hi) sp[d][1] = mine;
      }
      if (tid == 0) snan[d] = nan ? 1 : 0;
    }
    __syncthreads();
    if (tid < R6_NX)
      a.tubes[((int64_t)b * (N + 1) + k + 1) * R6_NX + tid] = snan[tid] ? NAN : tm_lerp(sp[tid][0], sp[tid][1], a.gamma);
    __syncthreads();   // sp / snan are read before the next step writes them
  }
}

extern "C" int gpmpc_tube_plan(int N, int n_samples, int *k_tile, int *mc_cap) {
  GPMPC_CHECK_ARG(k_tile && mc_cap);
  GPMPC_CHECK_ARG(N >= 0 && n_samples >= 0);
  *k_tile = TB_KTILE;
  *mc_cap = TB_MC_CAP;
  return 0;
}

static int tb_shape(const char *what, int batch, int N, double dt) {
  if (batch < 1) {
    gpmpc_set_error("%s: batch = %d, needs at least one trajectory", what, batch);
    return -2;
  }
  if (N < 1) {
    gpmpc_set_error("%s: N = %d, needs at least one horizon step", what, N);
    return -2;
  }
  if (!(dt > 0.0) || !std::isfinite(dt)) {
    gpmpc_set_error("%s: dt must be positive and finite", what);
    return -2;
  }
  if ((int64_t)batch * ((int64_t)N + 1) > (int64_t)INT_MAX / (R6_NX * R6_NX)) {
    gpmpc_set_error("%s: batch * N = %lld steps is more than one call takes", what, (long long)batch * N);
    return -2;
  }
  return 0;
}

extern "C" int gpmpc_tube_linear(gpmpc_ctx *ctx, const double *rocket, int batch, int N, double dt, double eps,
                                 const double *X_nom, const double *U_nom, const double *w, int w_mode, double w_max,
                                 const double *K, double *tubes, double *A_out, double *B_out) {
  GPMPC_CHECK_ARG(ctx && rocket && X_nom && U_nom && tubes);
  if (tb_shape("tube_linear", batch, N, dt)) return -2;
  if (!(eps != 0.0) || !std::isfinite(eps)) {
    gpmpc_set_error("tube_linear: eps must be finite and not zero");
    return -2;
  }
  if (w_mode < 0 || w_mode > 2 || (w_mode != 0 && !w)) {
    gpmpc_set_error("tube_linear: w_mode = %d needs 0 (w_max), 1 (14 bounds) or 2 (batch x N x 14 bounds) and its array",
                    w_mode);
    return -2;
  }
  TbArgs a{};
  if (r6_rocket(rocket, a.rk, "tube_linear")) return -2;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch, BN = B * (size_t)N, nw = w_mode == 0 ? 0 : w_mode == 1 ? R6_NX : BN * R6_NX;
  Stage sg(s);
  a.B = batch; a.N = N; a.w_mode = w_mode; a.have_K = K ? 1 : 0;
  a.dt = dt; a.eps = eps; a.w_max = w_max;
  sg.in(&a.X, X_nom, B * (N + 1) * R6_NX);
  sg.in(&a.U, U_nom, BN * R6_NU);
  sg.in(&a.w, nw ? w : nullptr, nw);  // null where no bound is read (w_mode 0, or no steps)
  sg.in(&a.K, K, (size_t)R6_NU * R6_NX);  // K, A_out, B_out: null where the caller gives none
  sg.out(&a.tubes, tubes, B * (N + 1) * R6_NX);
  sg.out(&a.A_out, A_out, BN * R6_NX * R6_NX);
  sg.out(&a.B_out, B_out, BN * R6_NX * R6_NU);
  if (int rc = sg.commit("tube_linear")) return rc;
  hipLaunchKernelGGL(k_tube_linear, dim3(batch), dim3(TB_T), 0, s, a);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}

extern "C" int gpmpc_tube_mc(gpmpc_ctx *ctx, const double *rocket, int batch, int N, int n_samples, double dt,
                             double quantile, const double *X_nom, const double *U_nom, const double *noise,
                             double *tubes) {
  GPMPC_CHECK_ARG(ctx && rocket && X_nom && U_nom && noise && tubes);
  if (tb_shape("tube_mc", batch, N, dt)) return -2;
  if (n_samples < 1 || n_samples > TB_MC_CAP) {
    gpmpc_set_error("tube_mc: n_samples = %d is outside 1..%d (one lane per particle)", n_samples, TB_MC_CAP);
    return -2;
  }
  if (!(quantile >= 0.0 && quantile <= 1.0)) {
    gpmpc_set_error("tube_mc: quantile = %g is outside [0, 1]", quantile);
    return -2;
  }
  if ((int64_t)batch * N * (int64_t)n_samples > (int64_t)INT_MAX / R6_NX) {
    gpmpc_set_error("tube_mc: batch * N * n_samples = %lld draws is more than one call takes",
                    (long long)batch * N * n_samples);
    return -2;
  }
  TmArgs a{};
  if (r6_rocket(rocket, a.rk, "tube_mc")) return -2;
  // numpy's linear method: the virtual index (n - 1) q, its floor and the next index, both the
  // last index at or past n - 1 (where numpy's previous index is -1, so gamma = v + 1)
  const double v = (double)(n_samples - 1) * quantile;
  double prev = std::floor(v);
  a.lo = (int)prev;
  a.hi = a.lo + 1;
  if (v >= (double)(n_samples - 1)) {
    a.lo = a.hi = n_samples - 1;
    prev = -1.0;
  }
  a.gamma = v - prev;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch, BN = B * (size_t)N, S = n_samples;
  Stage sg(s);
  a.B = batch; a.N = N; a.S = n_samples; a.dt = dt;
  sg.in(&a.X, X_nom, B * (N + 1) * R6_NX);
  sg.in(&a.U, U_nom, BN * R6_NU);
  sg.in(&a.noise, noise, BN * S * R6_NX);
  sg.out(&a.tubes, tubes, B * (N + 1) * R6_NX);
  if (int rc = sg.commit("tube_mc")) return rc;
  if (n_samples <= 128)
    hipLaunchKernelGGL(k_tube_mc<128>, dim3(batch), dim3(128), 0, s, a);
  else if (n_samples <= 256)
    hipLaunchKernelGGL(k_tube_mc<256>, dim3(batch), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_tube_mc<TB_MC_CAP>, dim3(batch), dim3(TB_MC_CAP), 0, s, a);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}
