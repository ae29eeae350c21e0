// qp_rules.h -- the OSQP-0.6 iteration rules, stated once for the three ADMM solvers
// (qp_device.h: generic, everything in LDS; fleet_qp.h: 3-DoF fleet, items in registers;
// fleet6_n.h: 6-DoF).  Functions of scalars, by value in and small structs out: no LDS, no
// thread index, no barrier, no storage layout -- each solver keeps its own storage, KKT
// solve, Ruiz scaling and loop skeleton and calls these per item.  The workgroup
// reductions at the end are the one exception: they take the caller's `red` rows.
// oracle/admm_oracle.py and oracle/admm_ref.c restate the same rules on the CPU.
#pragma once
#include <hip/hip_runtime.h>

#define QP_OSQP_INFTY 1e30
#define QP_MIN_SCALING 1e-4
#define QP_MAX_SCALING 1e4
#define QP_RHO_MIN 1e-6
#define QP_RHO_MAX 1e6
#define QP_RHO_TOL 1e-4
#define QP_RHO_EQ 1e3
#define QP_DIV_TOL 1e-30

struct QPSettingsDev {
  double rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  int max_iter, check_termination, adaptive_rho, adaptive_rho_interval;
  double adaptive_rho_tolerance;
  int scaling, warm_start;
};

// scaling.c limit_scaling
__device__ __forceinline__ double qp_limit(double v) {
  v = v < QP_MIN_SCALING ? 1.0 : v;
  return v > QP_MAX_SCALING ? QP_MAX_SCALING : v;
}

// rho of a row from its (scaled) bounds: free rows, equalities, inequalities
__device__ __forceinline__ double qp_row_rho(double l, double u, double rs) {
  if (l < -QP_OSQP_INFTY * QP_MIN_SCALING && u > QP_OSQP_INFTY * QP_MIN_SCALING) return QP_RHO_MIN;
  if (u - l < QP_RHO_TOL) return QP_RHO_EQ * rs;
  return rs;
}

// x = a x~ + (1 - a) x
struct QPXStep { double xn, dx; };
__device__ __forceinline__ QPXStep qp_x_step(double al, double xt, double xo) {
  const double xn = al * xt + (1.0 - al) * xo;
  return {xn, xn - xo};
}

// z = Pi(a z~ + (1 - a) z + y / rho),  y += rho (a z~ + (1 - a) z - z)
struct QPRowStep { double zn, yn, dy; };
__device__ __forceinline__ QPRowStep qp_row_step(double al, double zt, double rho, double l, double u,
                                                 double zo, double yo) {
  const double zr = al * zt + (1.0 - al) * zo;
  double zn = zr + yo / rho;
  zn = fmin(fmax(zn, l), u);
  const double d = rho * (zr - zn);
  return {zn, yo + d, d};
}

// residual norms (auxil.c update_info) and the rho-estimate quantities, max-accumulated:
// v: 0 pri (unscaled)  1 |z/E|  2 |Ax/E|  3 dua*c  4 |q/D|  5 |A'y/D|  6 |Px/D|
//    8 |Ax - z|  9 max(|z|,|Ax|)  10 |q + Px + A'y|  11 max(|q|,|A'y|,|Px|)   (scaled)
__device__ __forceinline__ void qp_acc_row(double (&v)[12], double ax, double z, double e) {
  v[0] = fmax(v[0], fabs((ax - z) / e));
  v[1] = fmax(v[1], fabs(z / e));
  v[2] = fmax(v[2], fabs(ax / e));
  v[8] = fmax(v[8], fabs(ax - z));
  v[9] = fmax(v[9], fmax(fabs(z), fabs(ax)));
}
__device__ __forceinline__ void qp_acc_var(double (&v)[12], double q, double px, double aty, double d) {
  v[3] = fmax(v[3], fabs((q + px + aty) / d));
  v[4] = fmax(v[4], fabs(q / d));
  v[5] = fmax(v[5], fabs(aty / d));
  v[6] = fmax(v[6], fabs(px / d));
  v[10] = fmax(v[10], fabs(q + px + aty));
  v[11] = fmax(v[11], fmax(fmax(fabs(q), fabs(aty)), fabs(px)));
}

// the infeasibility certificates' per-row arithmetic (auxil.c is_primal_infeasible /
// is_dual_infeasible): delta y projected onto the polar of the recession cone of [l, u],
// its support-function term, and "A delta x leaves the recession cone by more than thr"
__device__ __forceinline__ double qp_polar(double dy, double l, double u) {
  const bool bu = u > QP_OSQP_INFTY * QP_MIN_SCALING, bl = l < -QP_OSQP_INFTY * QP_MIN_SCALING;
  if (bu && bl) return 0.0;
  if (bu) return fmin(dy, 0.0);
  if (bl) return fmax(dy, 0.0);
  return dy;
}
__device__ __forceinline__ double qp_support(double dy, double l, double u) {
  return u * fmax(dy, 0.0) + l * fmin(dy, 0.0);
}
__device__ __forceinline__ bool qp_recedes_bad(double v, double l, double u, double thr) {
  return (u < QP_OSQP_INFTY * QP_MIN_SCALING && v > thr) || (l > -QP_OSQP_INFTY * QP_MIN_SCALING && v < -thr);
}

// auxil.c check_termination over the norms o[] (qp_acc_*) and the cost scaling c; status
// values as OSQP 0.6.  prim_inf(eps) / dual_inf(eps) are the caller's certificate walks,
// evaluated only when their residual test fails.
template <class PI, class DI>
__device__ __forceinline__ bool qp_terminated(const double (&o)[8], double c, const QPSettingsDev &st, bool approx,
                                              int &status, PI prim_inf, DI dual_inf) {
  const double pri = o[0], dua = o[3] / c;
  double ea = st.eps_abs, er = st.eps_rel, epi = st.eps_prim_inf, edi = st.eps_dual_inf;
  if (pri > QP_OSQP_INFTY || dua > QP_OSQP_INFTY) {
    status = -7;
    return true;
  }
  if (approx) { ea *= 10; er *= 10; epi *= 10; edi *= 10; }
  bool prim_ok = false, pinf = false, dual_ok = false, dinf = false;
  if (pri < ea + er * fmax(o[1], o[2])) prim_ok = true;
  else pinf = prim_inf(epi);
  if (dua < ea + er * fmax(fmax(o[4], o[5]), o[6]) / c) dual_ok = true;
  else dinf = dual_inf(edi);
  if (prim_ok && dual_ok) { status = approx ? 2 : 1; return true; }
  if (pinf) { status = approx ? 3 : -3; return true; }
  if (dinf) { status = approx ? 4 : -4; return true; }
  return false;
}

// compute_rho_estimate from re = v[8..11] of the accumulators, and "changed enough to refactor"
__device__ __forceinline__ double qp_rho_estimate(const double (&re)[4], double rho_s) {
  const double pr = re[0] / (re[1] + 1e-10);
  const double du = re[2] / (re[3] + 1e-10);
  const double est = rho_s * sqrt(pr / (du + 1e-10));
  return fmin(fmax(est, QP_RHO_MIN), QP_RHO_MAX);
}
__device__ __forceinline__ bool qp_rho_moved(double est, double rho_s, double tol) {
  return est > rho_s * tol || est < rho_s / tol;
}

// is a termination check / a rho adaptation due at iteration it (1-based)
__device__ __forceinline__ void qp_due(const QPSettingsDev &st, int it, bool &can_check, bool &adapt) {
  can_check = st.check_termination && (it % st.check_termination == 0);
  adapt = st.adaptive_rho && st.adaptive_rho_interval && (it % st.adaptive_rho_interval == 0);
}

// ---------------------------------------------------------------------------
// Workgroup reduction of K values over NW waves; every thread gets the result.  The wave
// partials go through red[wave][k] (any row width >= K).  Their combine order is part of
// the sums' bits: PAIR = (r0 + r1) + (r2 + r3), the generic kernel's, else in sequence.
template <int K, int NW, bool PAIR, int RW, class Op>
__device__ __forceinline__ void wg_reduce(double (&v)[K], double (*red)[RW], Op op) {
  static_assert(K <= RW && (!PAIR || NW == 4), "wg_reduce: row width / pairwise combine of four waves");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] = op(v[k], __shfl_xor(v[k], o));
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[wv][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if constexpr (PAIR) {
      v[k] = op(op(red[0][k], red[1][k]), op(red[2][k], red[3][k]));
    } else {
      double t = red[0][k];
#pragma unroll
      for (int w = 1; w < NW; ++w) t = op(t, red[w][k]);
      v[k] = t;
    }
  }
  __syncthreads();
}
template <int K, int NW, bool PAIR = false, int RW>
__device__ __forceinline__ void wg_max(double (&v)[K], double (*red)[RW]) {  // of non-negative values
  wg_reduce<K, NW, PAIR>(v, red, [](double a, double b) { return fmax(a, b); });
}
template <int K, int NW, bool PAIR = false, int RW>
__device__ __forceinline__ void wg_sum(double (&v)[K], double (*red)[RW]) {
  wg_reduce<K, NW, PAIR>(v, red, [](double a, double b) { return a + b; });
}
// sum of a and max of b in one exchange (3 barriers instead of 6); each tree is wg_sum's / wg_max's
template <int NW, int RW>
__device__ __forceinline__ void wg_sum_max(double &a, double &b, double (*red)[RW]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    b = fmax(b, __shfl_xor(b, o));
  }
  __syncthreads();
  if (lane == 0) { red[wv][0] = a; red[wv][1] = b; }
  __syncthreads();
  a = red[0][0];
  b = red[0][1];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    a += red[w][0];
    b = fmax(b, red[w][1]);
  }
  __syncthreads();
}
