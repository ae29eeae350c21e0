// uprop_ut.hip -- unscented uncertainty propagation along MPC horizons on the device
// (reference src/mpc/uncertainty_prop.py:179-264, UncertaintyPropagator._propagate_unscented),
// batch trajectories in one call, for the 3-DoF model (gpmpc_uprop3_unscented) and the
// 14-state model (gpmpc_uprop6_unscented).
//
// Unlike the linear method (uprop.hip) the variance cannot leave the step chain: Sigma_{k+1}
// contains var(x_k), and the sigma points of step k+1 come from chol(Sigma_{k+1}).  So one
// workgroup of 256 threads per trajectory runs the whole recursion, persistent over the N
// steps, with x_k, Sigma_k, the factor, the P = 2n+1 sigma points and their images in LDS.
// Step k (uncertainty_prop.py:222-262):
//   1. L = chol((n + lambda) Sigma_k + 1e-10 I), lower, by columns in LDS;
//   2. sp_0 = x_k, sp_{i+1} = x_k + L[:, i], sp_{n+i+1} = x_k - L[:, i];
//   3. per sigma point, one lane each: the nominal step (explicit Euler / r6_step) and the
//      GP features (features3 / the six roles of r6_features_role), scaled rows and squared
//      norms with the expressions of k_uprop3_means / k_uprop6_means;
//   4. the GP means at all P points: every thread owns training (inducing) rows, the points
//      go by in chunks so the accumulators stay in registers, a fixed-order reduction;
//      mean ystd + ymean, then + dt d on rows 4:7 (and 11:14);
//   5. the GP variance at the centre x_k only: k* into LDS (dynamic, 8 B a row), then
//      sigma2 - |W k*|^2 (+ |W2 k*|^2 for a sparse GP) with the finish of k_post_finish /
//      k_fitc_finish.  W is streamed once per step (its lower triangle, 4 n^2 B), consecutive
//      lanes on consecutive doubles (ut_sumsq).  This is the step's main cost;
//   6. x_{k+1} = sum w_m,i spn_i in index order (products rounded before the adds, as
//      numpy's axis-0 sum), Sigma_{k+1} = sum w_c,i d_i d_i^T + diag(var dt^2), a thread
//      per entry.
// A non-positive pivot in step k's factor ends that trajectory: info[b] = k + 1 and its
// remaining rows are NaN; the other trajectories do not notice.
#include "uprop.h"
#include "fleet6.h"
#include <algorithm>
#include <cmath>

#define UT_MAXROWS 4096  // k* in dynamic LDS: 8 B a row next to ~30 KB of static LDS

struct UtArgs {
  GpView gv, gw;            // gw: the 14-state model's d_omega GP only
  const double *W2v, *W2w;  // sparse GPs: L_B^-1 L_uu^-1 (fitc_W2); null for exact GPs
  R6Rocket rk;              // 14-state model
  double alpha, g3[3];      // 3-DoF model
  double scale, wm0, wc0, wi;  // n + lambda, the centre weights, 1 / (2 (n + lambda))
  int N;
  double dt;
  const double *x0, *U, *S0;
  double s0_diag;
  double *means, *covs;
  int *info;
};

// k* of the scaled query row z (LDS) against every row of the GP, into sk[0 .. g.n)
template <int D, int R>
__device__ __forceinline__ void ut_kstar(const GpView &g, bool reg, const GpRows<D, R> &w, const double *zq,
                                         double zn, double *sk) {
  const int tid = threadIdx.x;
  double z[D];
#pragma unroll
  for (int f = 0; f < D; ++f) z[f] = zq[f];
  if (reg) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = tid + 256 * r;
      if (j < g.n) {
        double dot = 0.0;
#pragma unroll
        for (int f = 0; f < D; ++f) dot = fma(z[f], w.x[r][f], dot);
        sk[j] = kernel_epilogue(g.kind, (zn + w.xn[r]) - 2.0 * dot, g.sigma2, g.iso_scale);
      }
    }
  } else {
    for (int j = tid; j < g.n; j += 256) {
      double dot = 0.0;
#pragma unroll
      for (int f = 0; f < D; ++f) dot = fma(z[f], g.Xs[(int64_t)j * D + f], dot);
      sk[j] = kernel_epilogue(g.kind, (zn + g.Xn[j]) - 2.0 * dot, g.sigma2, g.iso_scale);
    }
  }
}

// this wave's share of |W k*|^2, W n x n lower triangular, row-major; the same value on
// every lane of the wave, lane 0 leaves it in *out.  The pass over W is the step's main cost
// and one workgroup has to keep enough of it in flight:
//   n even: 16 rows a wave pass, a row per 16-lane group (four rows each), the lanes of a
//   group on consecutive 16-byte pairs, 128 columns a batch: 16 independent 16-byte loads a
//   lane before the first use (64 KB a workgroup).  A pair (c, c + 1) with c <= i lies inside
//   the n x n array because c is even and n is; its second half is dropped above the diagonal.
//   n odd (rows not 16-byte aligned): a wave per row, four rows in flight, 8-byte loads.
template <int T>  // T: 32-column chunks a batch (4 T loads a lane in flight)
__device__ __forceinline__ void ut_sumsq(const double *__restrict__ W, int n, const double *sk, double *out) {
  // the thread index made opaque here: what derives from it (lane group, column offsets, row
  // addresses) is formed in place, not hoisted out of the step loop into registers that are
  // short where the 14-state kernel runs its RK4 lanes (60 B of scratch a lane otherwise)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, wave = tid >> 6;
  double ss = 0.0;
  if ((n & 1) == 0) {
    const int g = lane >> 4, l2 = 2 * (lane & 15);
    for (int r0 = 16 * wave; r0 < n; r0 += 64) {
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      const int imax = min(r0 + 15, n - 1);
      for (int cb = 0; cb <= imax; cb += 32 * T) {
        double2 w[4][T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const int c = cb + 32 * t + l2;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int i = r0 + 4 * q + g;
            const bool ok = i < n && c <= i;
            w[q][t] = *reinterpret_cast<const double2 *>(W + (ok ? (int64_t)i * n + c : 0));
          }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const int c = cb + 32 * t + l2;
          const double k0 = c < n ? sk[c] : 0.0, k1 = c < n ? sk[c + 1] : 0.0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int i = r0 + 4 * q + g;
            const bool ok = i < n && c <= i;
            const double wx = ok ? w[q][t].x : 0.0, wy = ok && c + 1 <= i ? w[q][t].y : 0.0;
            v[q] = fma(wy, k1, fma(wx, k0, v[q]));
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double t = v[q];
#pragma unroll
        for (int s = 8; s > 0; s >>= 1) t += __shfl_xor(t, s);
        ss = fma(t, t, ss);  // (this group's row r0 + 4 q + g; rows past n: t = 0)
      }
    }
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
  } else {
    for (int i0 = wave; i0 < n; i0 += 16) {
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      const int imax = min(i0 + 12, n - 1);
#pragma unroll 4
      for (int c = lane; c <= imax; c += 64) {
        const double kc = sk[c];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + 4 * q;
          if (i < n && c <= i) v[q] = fma(W[(int64_t)i * n + c], kc, v[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double t = v[q];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) t += __shfl_xor(t, s);
        ss = fma(t, t, ss);  // (rows past n: t = 0)
      }
    }
  }
  if (lane == 0) *out = ss;
}

// MODEL 3: the 7-state explicit-Euler model over one GP (11 features); MODEL 6: the 14-state
// RK4 model over the StructuredRocketGP pair (13 / 12 features)
template <int MODEL>
__global__ __launch_bounds__(256) void k_uprop_ut(UtArgs a) {
  constexpr int n = MODEL == 3 ? 7 : 14, P = 2 * n + 1, G = MODEL == 3 ? 3 : 6;
  constexpr int DV = MODEL == 3 ? 11 : 13, DW = 12, R = MODEL == 3 ? UP_R3 : 1;
  constexpr int CV = 5;  // points per pass of the means
  constexpr int UT_T = 4;  // 32-column chunks a batch of the W pass
  const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
  const double dt = a.dt;
  extern __shared__ double sk[];  // k* of the centre point
  __shared__ double sx[n], sxn[n], sS[n][n + 1], sL[n][n + 1], sp[P][n], spn[P][n];
  __shared__ double zv[P][DV], zw[P][DW], znv[P], znw[P];
  __shared__ double red[4][P * G], redw[4][4], svar[G];
  __shared__ double sU[UP_NCAP * 3];
  __shared__ int sfail;
  const GpView &gv = a.gv, &gw = a.gw;
  const bool reg = MODEL == 3 ? gv.n <= 256 * UP_R3 : (gv.n <= 256 && gw.n <= 256);
  GpRows<DV, R> rv;
  GpRows<DW, 1> rw;  // (the 14-state model only)
  gp_rows_load(gv, reg, rv);
  if (MODEL == 6) gp_rows_load(gw, reg, rw);
  const double *Ub = up_controls(a.U, b, N, sU);
  double *mb = a.means + (int64_t)b * (N + 1) * n, *cb = a.covs + (int64_t)b * (N + 1) * n * n;
  if (tid < n) {
    sx[tid] = a.x0[(int64_t)b * n + tid];
    mb[tid] = sx[tid];
  }
  if (tid < n * n) {
    const int i = tid / n, j = tid - i * n;
    const double v = a.S0 ? a.S0[(int64_t)b * n * n + tid] : (i == j ? a.s0_diag : 0.0);
    sS[i][j] = v;
    sL[i][j] = 0.0;
    cb[tid] = v;
  }
  if (tid == 0) {
    sfail = 0;
    a.info[b] = 0;
  }
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    const double *u = Ub + k * 3;
    // 1. L = chol((n + lambda) Sigma_k + 1e-10 I), in place in sL's lower triangle
    if (tid < n * n) {
#pragma clang fp contract(off)  // numpy rounds the product before it adds
      const int i = tid / n, j = tid - i * n;
      if (j <= i) sL[i][j] = __dadd_rn(__dmul_rn(a.scale, sS[i][j]), i == j ? 1e-10 : 0.0);
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      if (tid == j) {
        double d = sL[j][j];
        for (int c = 0; c < j; ++c) d -= sL[j][c] * sL[j][c];
        if (d > 0.0) sL[j][j] = sqrt(d);
        else sfail = 1;  // (a NaN pivot too)
      }
      __syncthreads();
      if (sfail) break;
      if (tid > j && tid < n) {
        double s = sL[tid][j];
        for (int c = 0; c < j; ++c) s -= sL[tid][c] * sL[j][c];
        sL[tid][j] = s / sL[j][j];
      }
      __syncthreads();
    }
    if (sfail) {  // (read after a barrier: the same on every thread)
      if (tid == 0) a.info[b] = k + 1;
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      for (int e = tid; e < (N - k) * n; e += 256) mb[(int64_t)(k + 1) * n + e] = nan;
      for (int e = tid; e < (N - k) * n * n; e += 256) cb[(int64_t)(k + 1) * n * n + e] = nan;
      return;
    }
    // 2. the sigma points: columns of L
    for (int e = tid; e < P * n; e += 256) {
      const int p = e / n, r = e - p * n;
      double v = sx[r];
      if (p >= 1 && p <= n) v = __dadd_rn(v, sL[r][p - 1]);
      else if (p > n) v = __dsub_rn(v, sL[r][p - n - 1]);
      sp[p][r] = v;
    }
    __syncthreads();
    // 3. the nominal step and the features of every point, side by side
    if (MODEL == 3) {
      if (tid < P) {
        up3_euler(sp[tid], u, a.alpha, a.g3, dt, spn[tid]);
      } else if (tid >= 64 && tid < 64 + P) {
        const int p = tid - 64;
        double z[11];
        znv[p] = up3_query_row(gv, sp[p], u, z, zv[p]);
      }
      __syncthreads();
    } else {
      if (tid < R6_FEAT_ROLES * P) {  // role-major: a wave runs at most three roles
        const int role = tid / P, p = tid - role * P;
        const double one[13] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
        r6_features_role(role, sp[p], u, one, one, zv[p], zw[p]);
      } else if (tid >= 192 && tid < 192 + P) {
        r6_step(a.rk, sp[tid - 192], u, dt, spn[tid - 192]);
      }
      __syncthreads();
      for (int e = tid; e < P * (DV + DW); e += 256) {
        const int p = e / (DV + DW), f = e - p * (DV + DW);
        if (f < DV) zv[p][f] = gv.kind == GPMPC_SE_ISO ? zv[p][f] : zv[p][f] / gv.ls[f];
        else zw[p][f - DV] = gw.kind == GPMPC_SE_ISO ? zw[p][f - DV] : zw[p][f - DV] / gw.ls[f - DV];
      }
      __syncthreads();
      if (tid < P) {
        double zn = 0.0;
#pragma unroll
        for (int f = 0; f < DV; ++f) zn += zv[tid][f] * zv[tid][f];
        znv[tid] = zn;
      } else if (tid >= 64 && tid < 64 + P) {
        double zn = 0.0;
#pragma unroll
        for (int f = 0; f < DW; ++f) zn += zw[tid - 64][f] * zw[tid - 64][f];
        znw[tid - 64] = zn;
      }
      __syncthreads();
    }
    // 4. the GP means at the P points; 5. k* of the centre, |W k*|^2 (and |W2 k*|^2)
    gp_rows_means<DV, R, P, CV, G>(gv, reg, rv, &zv[0][0], znv, &red[0][0], P * G, 0);
    if (MODEL == 6) gp_rows_means<DW, 1, P, CV, G>(gw, reg, rw, &zw[0][0], znw, &red[0][0], P * G, 3);
    ut_kstar<DV, R>(gv, reg, rv, zv[0], znv[0], sk);
    __syncthreads();
    const int wave = tid >> 6;
    ut_sumsq<UT_T>(gv.W, gv.n, sk, &redw[0][wave]);
    if (a.W2v) ut_sumsq<UT_T>(a.W2v, gv.n, sk, &redw[1][wave]);
    if (MODEL == 6) {
      __syncthreads();
      ut_kstar<DW, 1>(gw, reg, rw, zw[0], znw[0], sk);
      __syncthreads();
      ut_sumsq<UT_T>(gw.W, gw.n, sk, &redw[2][wave]);
      if (a.W2w) ut_sumsq<UT_T>(a.W2w, gw.n, sk, &redw[3][wave]);
    }
    __syncthreads();
    if (tid < P * G) {
      // mean ystd + ymean, then + dt d on the velocity (rate) rows of the point's image
      const int p = tid / G, c = tid - p * G;
      const GpView &g = c < 3 ? gv : gw;
      const double m = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
      const double d = m * g.ystd[c % 3] + g.ymean[c % 3];
      const int row = c < 3 ? 4 + c : 8 + c;
      {
#pragma clang fp contract(off)  // spn[:, rows] += d * dt: the product rounded, then the sum
        spn[p][row] = __dadd_rn(spn[p][row], __dmul_rn(d, dt));
      }
    } else if (tid >= 192 && tid < 192 + G) {
      // the posterior finish (k_post_finish / k_fitc_finish): lat = sigma2 - |v|^2 (+ |w|^2), floor 1e-10
      const int c = tid - 192, q = c < 3 ? 0 : 2;
      const GpView &g = c < 3 ? gv : gw;
      const double *W2 = c < 3 ? a.W2v : a.W2w;
      const double sv = ((redw[q][0] + redw[q][1]) + redw[q][2]) + redw[q][3];
      double lat = g.sigma2 - sv;
      if (W2) lat = lat + (((redw[q + 1][0] + redw[q + 1][1]) + redw[q + 1][2]) + redw[q + 1][3]);
      lat = lat > 1e-10 ? lat : 1e-10;
      svar[c] = lat * g.ystd[c % 3] * g.ystd[c % 3];
    }
    __syncthreads();
    // 6. x_{k+1}, then Sigma_{k+1}
    if (tid < n) {
#pragma clang fp contract(off)
      double s = __dmul_rn(a.wm0, spn[0][tid]);
      for (int p = 1; p < P; ++p) s = __dadd_rn(s, __dmul_rn(a.wi, spn[p][tid]));
      sxn[tid] = s;
      mb[(int64_t)(k + 1) * n + tid] = s;
    }
    __syncthreads();
    if (tid < n * n) {
#pragma clang fp contract(off)
      const int i = tid / n, j = tid - i * n;
      double s = 0.0;
      for (int p = 0; p < P; ++p) {
        const double di = __dsub_rn(spn[p][i], sxn[i]), dj = __dsub_rn(spn[p][j], sxn[j]);
        s = __dadd_rn(s, __dmul_rn(p == 0 ? a.wc0 : a.wi, __dmul_rn(di, dj)));
      }
      if (i == j) {
        const double dt2 = __dmul_rn(dt, dt);
        if (i >= 4 && i < 7) s = __dadd_rn(s, __dmul_rn(svar[i - 4], dt2));
        if (MODEL == 6 && i >= 11) s = __dadd_rn(s, __dmul_rn(svar[i - 8], dt2));
      }
      sS[i][j] = s;
      cb[(int64_t)(k + 1) * n * n + tid] = s;
      if (j == 0) sx[i] = sxn[i];
    }
    __syncthreads();
  }
}

// the unscented transform's constants from (alpha, beta, kappa), uncertainty_prop.py:196-210
static void ut_weights(const double *ut, int n, UtArgs &a) {
  const double lam = std::pow(ut[0], 2.0) * (n + ut[2]) - n;
  a.scale = n + lam;
  a.wi = 1 / (2 * (n + lam));
  a.wm0 = lam / (n + lam);
  a.wc0 = lam / (n + lam) + (1 - std::pow(ut[0], 2.0) + ut[1]);
}

template <int MODEL>
static int ut_run(gpmpc_ctx *ctx, UtArgs &a, const char *what, int batch, int N, const double *x0, const double *U,
                  const double *S0, double *means, double *covs, int *info) {
  constexpr size_t n = MODEL == 3 ? 7 : 14;
  const int rows = std::max(a.gv.n, MODEL == 6 ? a.gw.n : 0);
  if (rows > UT_MAXROWS) {
    gpmpc_set_error("%s: at most %d training / inducing rows (k* is held in LDS)", what, UT_MAXROWS);
    return -2;
  }
  if (batch == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch;
  // inputs in one pinned upload; means, covariances and info in one read-back
  Stage sg(s);
  UpIo io(sg, B, N, n, x0, U, S0, means, covs);
  sg.out(&a.info, info, B);
  if (int rc = sg.commit(what)) return rc;
  a.x0 = io.x0; a.U = io.U; a.S0 = io.S0; a.means = io.means; a.covs = io.covs;
  hipLaunchKernelGGL(k_uprop_ut<MODEL>, dim3(batch), dim3(256), sizeof(double) * (size_t)rows, s, a);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}

extern "C" int gpmpc_uprop3_unscented(gpmpc_ctx *ctx, void *gp, int exact, int batch, int N, double dt, double alpha,
                                      const double *g3, const double *ut, const double *x0, const double *U,
                                      const double *S0, double s0_diag, double *means, double *covs, int *info) {
  GPMPC_CHECK_ARG(ctx && gp && g3 && ut && x0 && U && means && covs && info && batch >= 0 && N >= 0);
  UtArgs a{};
  if (up_view3(gp, exact, "uprop3_unscented", "GP", a.gv, &a.W2v)) return -2;
  a.gw = a.gv;
  a.alpha = alpha;
  for (int i = 0; i < 3; ++i) a.g3[i] = g3[i];
  ut_weights(ut, 7, a);
  a.N = N;
  a.dt = dt;
  a.s0_diag = s0_diag;
  return ut_run<3>(ctx, a, "uprop3_unscented", batch, N, x0, U, S0, means, covs, info);
}

extern "C" int gpmpc_uprop6_unscented(gpmpc_ctx *ctx, void *gp_v, void *gp_w, int exact, const double *rocket,
                                      const double *ut, int batch, int N, double dt, const double *x0,
                                      const double *U, const double *S0, double s0_diag, double *means,
                                      double *covs, int *info) {
  GPMPC_CHECK_ARG(ctx && gp_v && gp_w && rocket && ut && x0 && U && means && covs && info && batch >= 0 && N >= 0);
  UtArgs a{};
  if (up_view6(gp_v, gp_w, exact, "uprop6_unscented", a.gv, a.gw, &a.W2v, &a.W2w)) return -2;
  if (r6_rocket(rocket, a.rk, "uprop6_unscented")) return -2;
  ut_weights(ut, 14, a);
  a.N = N;
  a.dt = dt;
  a.s0_diag = s0_diag;
  return ut_run<6>(ctx, a, "uprop6_unscented", batch, N, x0, U, S0, means, covs, info);
}
