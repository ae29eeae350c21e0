// fleet_control.h -- the 3-DoF fleet's control step on the fleet-specialised solver
// (fleet_qp.h), and what it shares with the generic control kernel of fleet.hip: the model
// sizes, the plant, the landing check and the kernels' argument block.
//
// Two units compile this header, and they differ only by three defines set before it:
//   fleet.hip       FQ_T 128, FQ_WPE FQ_NW (2), FQ_KNS fq_narrow   (the defaults)
//   fleet_wide.hip  FQ_T 256, FQ_WPE 1,         FQ_KNS fq_wide
// Each gets, in namespace FQ_KNS, k_fleet_control2<STAMPS>, k_qp_fleet and their two
// launchers launch_control / launch_qp.
#pragma once
#include "internal.h"
#include "qp.h"
#include "fleet_qp.h"

#ifndef FQ_KNS
#define FQ_KNS fq_narrow
#endif
#ifndef FQ_WPE
#define FQ_WPE FQ_NW  // waves per SIMD the register budget is sized for
#endif
#define NX 7
#define NU 3
#define NFEAT 11
#define DYN_NNZ 26

// ---------------------------------------------------------------------------
__device__ __forceinline__ void plant_euler(const double *x, const double *u, double dt,
                                            double *o) {
  // nominal_mpc.py:585-605 (alpha = 1/(I_sp g0) = 1/30, g = [-1, 0, 0])
  const double tm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  o[0] = x[0] - dt * (1.0 / 30.0) * tm;
  o[1] = x[1] + dt * x[4];
  o[2] = x[2] + dt * x[5];
  o[3] = x[3] + dt * x[6];
  o[4] = x[4] + dt * (u[0] / x[0] + -1.0);
  o[5] = x[5] + dt * (u[1] / x[0] + 0.0);
  o[6] = x[6] + dt * (u[2] / x[0] + 0.0);
}

__device__ __forceinline__ void drag_residual(const double *x, double *d) {
  // experiments/dispersion.py:349-360: rho 0.02, Cd = A = 1, |v| > 1
  const double vx = x[4], vy = x[5], vz = x[6];
  const double sp = sqrt(vx * vx + vy * vy + vz * vz);
  if (sp > 1.0) {
    const double a = (0.5 * 0.02 * 1.0 * 1.0 * sp * sp) / x[0];
    d[0] = -a * (vx / sp); d[1] = -a * (vy / sp); d[2] = -a * (vz / sp);
  } else {
    d[0] = d[1] = d[2] = 0.0;
  }
}

__device__ __forceinline__ bool landing_ok(const double *x, double m0) {
  // LandingConstraints.check_landing (monte_carlo.py:54-104), run_experiments.py tolerances.
  // Outcomes 1 and 4 both mean "landed" (the landing stops either way, monte_carlo.py
  // :482-488); a caller with other LandingConstraints re-decides between them on the host
  // from the record's final state (MonteCarloSimulator.run does, experiments/monte_carlo.py),
  // so custom tolerances need no device change.
  if (fabs(x[1]) > 1.0) return false;
  if (fabs(x[2]) > 5.0 || fabs(x[3]) > 5.0) return false;
  if (fabs(x[4]) > 3.0) return false;
  if (fabs(x[5]) > 1.0 || fabs(x[6]) > 1.0) return false;
  if (1.0 - x[0] / m0 > 1.0 - 0.05) return false;
  return true;
}

struct FleetArgs {
  QPPattern pt;
  QPSettingsDev st;
  int N, target_mode, use_gp, residual_model, max_steps;
  double dt;
  double *x, *Xw, *Uw, *ysc, *rho, *rec, *xt;
  const double *gmean;  // (B*N) x 3, row (slot or landing)*N + k
  int gp_by_slot;       // gmean rows follow the dispatch slot (order[]) instead of the landing
  const int *order;     // workgroup -> landing (longest predicted first), or null
  int alt_wave;         // fleet solver: odd workgroups run the KKT chain on wave 1
  // fused posterior finish (k_fleet_control2 only; null part: k_post_finish ran)
  const double *part, *meanT, *ymean, *ystd;
  double *mean_out, *var_out;
  double sigma2;
  int nrt;
  int64_t pld;          // leading dimension of part / meanT (P)
  const double *part2;  // a sparse GP's second partials |W2 k*|^2 (or null: exact GP)
  int nrt2;
  unsigned *claims;     // per-CU claimed chain SIMDs, (epoch << 8) | 4-bit mask (or null)
  unsigned epoch;       // this launch's claim generation (never 0)
  int *lastit;          // ADMM iterations of each landing's last solve
  unsigned long long *stamps;  // diagnostic phase cycles of block 0 (or null)
  unsigned long long *trace;   // diagnostic per-landing placement/timing (or null)
  // SQP pass of GPMPC.solve's loop (gp_mpc.py:296-345; sqp = 0: RTI)
  int sqp, sqp_first, sqp_last;
  double sqp_tol;
  int *sqp_done;               // landing converged in an earlier pass of this control step
  double *u0_out;              // batch x 3 applied controls of the plant step (or null: nothing attached)
};

// The latent variance of query row q from the SUMSQ partials (k_post_finish / k_fitc_finish
// arithmetic): exact GP sigma2 - |L^-1 k*|^2 (exact_gp.py:256-266); a sparse GP (FITC / VFE,
// one predict body, sparse_gp.py:285-301) sigma2 - |L_uu^-1 k*|^2 + |L_B^-1 L_uu^-1 k*|^2
__device__ __forceinline__ double fleet_latent_var(const FleetArgs &a, int64_t q) {
  double ss = 0.0;
  for (int t = 0; t < a.nrt; ++t) ss += a.part[(int64_t)t * a.pld + q];
  double lat;
  if (a.part2) {
    double sw = 0.0;
    for (int t = 0; t < a.nrt2; ++t) sw += a.part2[(int64_t)t * a.pld + q];
    lat = a.sigma2 - ss + sw;
  } else {
    lat = a.sigma2 - ss;
  }
  return lat > 1e-10 ? lat : 1e-10;
}

// ---------------------------------------------------------------------------
// The parts of the landing-step protocol that k_fleet_control (fleet.hip, the generic solver)
// and k_fleet_control2 (below) both call: the record writes, the boxes and the plant step.
// The solver bookkeeping of the record (rho, rec[11..15], lastit) differs between the RTI
// and SQP sites and stays there.
//
// Four parts stay written out in each of the two kernels, every copy with a comment naming
// its twin: the termination checks, the target, the cost weights and the stage
// linearisation.  As helpers they gave the same bits and the same VGPR, scratch and LDS
// sizes, but a call changes the order in which the compiler meets the expressions, the
// register allocation of the whole kernel follows, and the 128-thread k_fleet_control2
// measured 0.3-0.9% slower per helper at 1024 landings (docs/PERF_HISTORY.md, "fleet.hip
// split").  The calls below leave the kernels' instructions as they were but for the order
// of a few moves and stores.

// The record of a landing that stops at state sx: outcome, fuel used, final state
__device__ __forceinline__ void fleet_record_stop(double *rec, const double *sx, int outcome) {
  rec[0] = outcome;
  rec[2] = rec[13] - sx[0];
  for (int i = 0; i < NX; ++i) rec[4 + i] = sx[i];
}

// State and thrust boxes of entry i of a stage block
__device__ __forceinline__ void fleet_box(int i, double &lo, double &hi) {
  if (i < NX) {
    const double xmin[NX] = {-INFINITY, -100, -100, -100, -50, -50, -50};
    const double xmax[NX] = {INFINITY, 500, 100, 100, 50, 50, 50};
    lo = xmin[i]; hi = xmax[i];
  } else {
    const double umin[NU] = {0.3, -5, -5}, umax[NU] = {5, 5, 5};
    lo = umin[i - NX]; hi = umax[i - NX];
  }
}

// The plant step of landing b under control u0 (nominal Euler + the aero residual the GP
// learns): the new state into xn and the plant state x, u0 to the Monte-Carlo attachment
__device__ __forceinline__ void fleet_plant_step(const FleetArgs &a, int b, const double *sx, const double *u0,
                                                 double *x, double *xn) {
  double dr[3];
  plant_euler(sx, u0, a.dt, xn);
  if (a.u0_out) for (int i = 0; i < NU; ++i) a.u0_out[(int64_t)b * NU + i] = u0[i];
  if (a.residual_model) {
    drag_residual(sx, dr);
    xn[4] += dr[0] * a.dt; xn[5] += dr[1] * a.dt; xn[6] += dr[2] * a.dt;
  }
  for (int i = 0; i < NX; ++i) x[i] = xn[i];
}

// The record of a landing that took a step to xn: step count, time, fuel used, state
__device__ __forceinline__ void fleet_record_step(double *rec, const double *xn, double dt) {
  rec[1] += 1.0;
  rec[3] = rec[1] * dt;
  rec[2] = rec[13] - xn[0];
  for (int i = 0; i < NX; ++i) rec[4 + i] = xn[i];
}

// the control launch of each build (the batched-QP launchers launch_qp are declared in qp.h)
namespace fq_narrow { hipError_t launch_control(hipStream_t s, int nb, const FleetArgs &a, bool stamps); }
namespace fq_wide { hipError_t launch_control(hipStream_t s, int nb, const FleetArgs &a, bool stamps); }

// the control kernel lives in a namespace of its build: fleet.hip (128 threads, four
// landings per CU) and fleet_wide.hip (256 threads, one wave per SIMD) each have one
namespace FQ_KNS {
// The same control step as k_fleet_control (fleet.hip) on the fleet-specialised solver
// (fleet_qp.h): 128 threads and ~37 KB of LDS per landing, four landings per CU.  Assembly
// goes straight into the owners' registers; results and the plant step as there.
// STAMPS: the diagnostic phase-cycle instance (gpmpc_fleet_set_stamps); the
// production instance has no stamp code or state at all.
template <bool STAMPS>
__global__ __launch_bounds__(FQ_T) __attribute__((amdgpu_waves_per_eu(FQ_WPE, FQ_WPE))) void k_fleet_control2(FleetArgs a) {
  __shared__ FleetSmem s;
  __shared__ double sx[NX], st_tgt[NX];
  __shared__ int s_out;
  const int b = a.order ? a.order[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
  const int N = a.N, n = a.pt.n, m = a.pt.m;
  const double dt = a.dt;
  double *rec = a.rec + (int64_t)b * GPMPC_REC_LEN;
  // The posterior finish of this slot's queries (k_post_finish's arithmetic) for a landing
  // that returns before its QP assembly: every launched slot is finished, so a slot never
  // keeps the values another landing left in it at an earlier step; the
  // posterior is the one at this landing's linearisation trajectory, as on the unfused path
  auto finish_only = [&]() {
    if (!(a.part && a.use_gp)) return;
    for (int k = tid; k < N; k += FQ_T) {
      const int64_t q = (int64_t)(a.gp_by_slot ? (int)blockIdx.x : b) * N + k;
      const double lat = fleet_latent_var(a, q);
      for (int c = 0; c < 3; ++c) {
        a.mean_out[q * 3 + c] = a.meanT[(int64_t)c * a.pld + q] * a.ystd[c] + a.ymean[c];
        a.var_out[q * 3 + c] = lat * a.ystd[c] * a.ystd[c];
      }
    }
  };
  if (rec[0] != 0.0) {  // terminated landing
    finish_only();
    return;
  }
  if (a.sqp && !a.sqp_first && a.sqp_done[b]) {  // converged in an earlier SQP pass
    finish_only();
    return;
  }
  QPStamps T;
  T.out = (STAMPS && b == 0) ? a.stamps : nullptr;
  T.start();
  if (a.trace && (tid & 63) == 0 && tid < 128) {
    // [0] start, [1] end (realtime), [2] wave 0 HW_ID | XCC_ID << 32, [3] wave 1 the same
    unsigned long long *tr = a.trace + (int64_t)b * 4;
    if (tid == 0) tr[0] = __builtin_amdgcn_s_memrealtime();
    tr[2 + (tid >> 6)] = (unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
                         ((unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
  }
  double *x = a.x + (int64_t)b * NX;
  double *Xw = a.Xw + (int64_t)b * (N + 1) * NX;
  double *Uw = a.Uw + (int64_t)b * N * NU;
  // Chain wave: the two waves of a workgroup sit on two SIMDs, and the four
  // workgroups of a CU fill each SIMD with two waves.  Two KKT chains on one
  // SIMD slow both (the slowest landings, which set the kernel time, are the
  // ones sharing), so each workgroup claims a SIMD of its CU for its chain:
  // wave 0's if no earlier workgroup of this launch took it, else wave 1's.
  __shared__ int s_simd[FQ_NW], s_cw;
  if (a.claims && (tid & 63) == 0) s_simd[tid >> 6] = (__builtin_amdgcn_s_getreg(4 | (31 << 11)) >> 4) & 3;
  if (tid < NX) sx[tid] = x[tid];
  __syncthreads();
  if (tid == 0) {
    int cw0 = a.alt_wave ? (int)(blockIdx.x & 1) : 0;
    if (a.claims) {
      const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));
      const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11)) & 15;
      const unsigned key = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
      unsigned *cl = a.claims + key;
      unsigned old = __hip_atomic_load(cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int tries = 0; tries < 16; ++tries) {  // bounded: contention is at most 4 workgroups
        const unsigned mask = (old >> 8) == a.epoch ? (old & 15u) : 0u;
        int w = 0;  // the first wave whose SIMD no earlier workgroup claimed (else wave 0)
        while (w < FQ_NW && (mask & (1u << s_simd[w]))) ++w;
        if (w == FQ_NW) w = 0;
        const unsigned nv = (a.epoch << 8) | mask | (1u << s_simd[w]);
        const unsigned prev = atomicCAS(cl, old, nv);
        if (prev == old) { cw0 = w; break; }
        old = prev;
      }
    }
    s_cw = cw0;
  }
  if (tid == 0) {
    // termination checks (monte_carlo.py:458-488) and target (:497-500 or fixed).  Twin:
    // k_fleet_control (fleet.hip); a change goes into both
    int out = 0;
    const double m0 = rec[13];
    bool div = false;
    for (int i = 0; i < NX; ++i) div = div || !(fabs(sx[i]) <= 1e6);
    if (a.sqp && !a.sqp_first) out = 0;  // later SQP passes: same state, checks done
    else if ((int)rec[1] >= a.max_steps) out = 5;
    else if (sx[1] < 0.0) out = 2;
    else if (sx[0] <= 1.0 + 0.01) out = 3;
    else if (div) out = 6;
    else if (sx[1] < 1.0 && fabs(sx[4]) < 5.0) out = landing_ok(sx, m0) ? 1 : 4;
    if (a.sqp && a.sqp_first) a.sqp_done[b] = 0;  // a new control step: no pass has converged
    s_out = out;
    for (int i = 0; i < NX; ++i) st_tgt[i] = a.target_mode ? sx[i] : a.xt[(int64_t)b * NX + i];
    if (a.target_mode) {
      st_tgt[4] = st_tgt[5] = st_tgt[6] = 0.0;
      st_tgt[1] = fmax(0.5, sx[1] - 2.0);
    }
  }
  __syncthreads();
  if (s_out) {
    if (tid == 0) fleet_record_stop(rec, sx, s_out);
    finish_only();
    return;
  }
  FleetRegs R;
  fq_init_pattern(a.pt, R, n);
  const int Nv = N * (NX + NU);
  const int MD = NX * (N + 1);
  // ---- QP data (osqp_rti.py:203-372 with the GPMPC sign): variables + bound rows
#pragma unroll
  for (int h = 0; h < FQ_H; ++h) {
    if (!R.vok[h]) continue;
    const int j = R.vj[h];
    double p, qq, lo, hi, xw;
    const int i = (j >= Nv) ? j - Nv : j % (NX + NU);
    // cost weights Q, Q_f = 10 Q, R.  Twin: k_fleet_control (fleet.hip); a change goes into both
    if (j >= Nv) {
      const double qd = (i == 0) ? 0.0 : (i < 4 ? 100.0 : 10.0);
      p = qd; qq = -qd * st_tgt[i];
      xw = Xw[N * NX + i];
    } else {
      const int k = j / (NX + NU);
      if (i < NX) {
        const double qd = (i == 0) ? 0.0 : (i < 4 ? 10.0 : 1.0);
        p = qd; qq = -qd * st_tgt[i];
        xw = Xw[k * NX + i];
      } else {
        p = 0.01; qq = 0.0;
        xw = Uw[k * NU + (i - NX)];
      }
    }
    fleet_box(i, lo, hi);
    R.P[h] = p; R.q[h] = qq; R.x[h] = xw;
    R.Ab[h] = 1.0; R.lb[h] = lo; R.ub[h] = hi;
    R.yb_(h) = a.ysc[(int64_t)b * m + MD + j];
  }
  // dynamics rows: A values (one thread per stage) and c_k, staged in zt for the row owners
  for (int r = tid; r < NX; r += FQ_T) {
    s.A[r] = 1.0;
    s.zt[r] = sx[r];
  }
  for (int k = tid; k < N; k += FQ_T) {
    const double *xk = Xw + k * NX;
    const double *uk = Uw + k * NU;
    // FastRTI3DoF._linearize (osqp_rti.py:656-710) and c_k = (f - A x) - B u (:340-341).  Twin:
    // k_fleet_control (fleet.hip); a change goes into both
    const double mk = xk[0], tx = uk[0], ty = uk[1], tz = uk[2];
    const double tm = sqrt(tx * tx + ty * ty + tz * tz) + 1e-10;
    const double al = 1.0 / 30.0;
    const double a40 = -tx / (mk * mk) * dt, a50 = -ty / (mk * mk) * dt, a60 = -tz / (mk * mk) * dt;
    const double b00 = -al * tx / tm * dt, b01 = -al * ty / tm * dt, b02 = -al * tz / tm * dt;
    const double bv = dt / mk;
    double *Ak = s.A + NX + k * DYN_NNZ;
    Ak[0] = 1.0; Ak[1] = b00; Ak[2] = b01; Ak[3] = b02; Ak[4] = -1.0;
    Ak[5] = 1.0; Ak[6] = dt; Ak[7] = -1.0;
    Ak[8] = 1.0; Ak[9] = dt; Ak[10] = -1.0;
    Ak[11] = 1.0; Ak[12] = dt; Ak[13] = -1.0;
    Ak[14] = a40; Ak[15] = 1.0; Ak[16] = bv; Ak[17] = -1.0;
    Ak[18] = a50; Ak[19] = 1.0; Ak[20] = bv; Ak[21] = -1.0;
    Ak[22] = a60; Ak[23] = 1.0; Ak[24] = bv; Ak[25] = -1.0;
    double f[NX];
    plant_euler(xk, uk, dt, f);
    double ax[NX], bu[NX];
    ax[0] = xk[0];
    ax[1] = xk[1] + dt * xk[4];
    ax[2] = xk[2] + dt * xk[5];
    ax[3] = xk[3] + dt * xk[6];
    ax[4] = a40 * xk[0] + xk[4];
    ax[5] = a50 * xk[0] + xk[5];
    ax[6] = a60 * xk[0] + xk[6];
    bu[0] = b00 * tx + b01 * ty + b02 * tz;
    bu[1] = bu[2] = bu[3] = 0.0;
    bu[4] = bv * tx; bu[5] = bv * ty; bu[6] = bv * tz;
    const int64_t q = (int64_t)(a.gp_by_slot ? (int)blockIdx.x : b) * N + k;  // query row
    double gm[3];
    if (a.part && a.use_gp) {
      // the posterior finish of this landing's query (k_post_finish / k_fitc_finish arithmetic)
      const double lat = fleet_latent_var(a, q);
      for (int c = 0; c < 3; ++c) {
        gm[c] = a.meanT[(int64_t)c * a.pld + q] * a.ystd[c] + a.ymean[c];
        a.mean_out[q * 3 + c] = gm[c];
        a.var_out[q * 3 + c] = lat * a.ystd[c] * a.ystd[c];
      }
    } else {
      for (int c = 0; c < 3; ++c) gm[c] = a.gmean[q * 3 + c];
    }
    for (int i = 0; i < NX; ++i) {
      double c = (f[i] - ax[i]) - bu[i];
      if (a.use_gp && i >= 4) c += gm[i - 4] * dt;  // the GP mean on the velocity rows of c_k
      s.zt[NX * (k + 1) + i] = -c;
    }
  }
  if (tid == 0) s.rho_s = a.rho[b];
  __syncthreads();
#pragma unroll
  for (int h = 0; h < FQ_H; ++h)
    if (R.rok[h]) {
      R.ur(h) = s.zt[R.rr[h]];  // l = u
      R.yr(h) = a.ysc[(int64_t)b * m + R.rr[h]];
    }
  __syncthreads();
  T.mark(0);
  QPResult res = fq_solve(a.pt, s, R, a.st, &T, s_cw);
  T.mark(7);
  const bool has = !res.factor_fail && (res.status == 1 || res.status == 2 || res.status == -2);
  if (has) {
#pragma unroll
    for (int h = 0; h < FQ_H; ++h)
      if (R.vok[h]) s.rhs[R.vj[h]] = R.D[h] * R.x[h];  // unscaled solution
  }
  __syncthreads();
  if (!has && a.target_mode == 1) {  // solve protocol: failed solve -> DIVERGENCE
    if (tid == 0) {
      fleet_record_stop(rec, sx, 6);
      rec[14] = res.factor_fail ? -100 : res.status;
    }
    return;
  }
  if (a.sqp) {
    // GPMPC.solve's loop (gp_mpc.py:336-353): the change of the trajectory,
    // X_pred <- X_new (no shift), stop below sqp_tol
    double dm[1] = {0.0};
#pragma unroll
    for (int h = 0; h < FQ_H; ++h)
      if (R.vok[h]) {
        const int j = R.vj[h], i = (j >= Nv) ? j - Nv : j % (NX + NU), k = j / (NX + NU);
        const double old = (j >= Nv) ? Xw[N * NX + i] : (i < NX ? Xw[k * NX + i] : Uw[k * NU + i - NX]);
        dm[0] = fmax(dm[0], fabs(s.rhs[j] - old));
      }
    wg_max<1, FQ_NW>(dm, s.red);  // (its barriers order the reads of Xw / Uw before the writes)
    for (int e = tid; e < (N + 1) * NX; e += FQ_T) {
      const int k = e / NX, i = e - k * NX;
      Xw[e] = s.rhs[(k == N) ? Nv + i : k * (NX + NU) + i];
    }
    for (int e = tid; e < N * NU; e += FQ_T) {
      const int k = e / NU, i = e - k * NU;
      Uw[e] = s.rhs[k * (NX + NU) + NX + i];
    }
#pragma unroll
    for (int h = 0; h < FQ_H; ++h) {
      if (R.rok[h]) a.ysc[(int64_t)b * m + R.rr[h]] = R.yr(h);
      if (R.vok[h]) a.ysc[(int64_t)b * m + MD + R.vj[h]] = R.yb_(h);
    }
    if (tid == 0) {
      const bool conv = dm[0] < a.sqp_tol;
      a.rho[b] = s.rho_s;
      rec[11] += res.iter;
      a.lastit[b] = res.iter;
      rec[12] += (res.status == 1) ? 1.0 : 0.0;
      rec[14] = res.status;
      rec[15] = s.rho_s;
      if (conv) {
        const double u0[NU] = {s.rhs[NX], s.rhs[NX + 1], s.rhs[NX + 2]};
        double xn[NX];
        fleet_plant_step(a, b, sx, u0, x, xn);
        fleet_record_step(rec, xn, dt);
        a.sqp_done[b] = 1;
      } else if (a.sqp_last) {  // MPCSolution.success False -> DIVERGENCE (monte_carlo.py:506-508)
        fleet_record_stop(rec, sx, 6);
      }
    }
    T.mark(7);
    T.flush();
    if (a.trace && tid == 0) a.trace[(int64_t)b * 4 + 1] = __builtin_amdgcn_s_memrealtime();
    return;
  }
  if (has) {
    for (int e = tid; e < (N + 1) * NX; e += FQ_T) {
      const int k = e / NX, i = e - k * NX;
      const int ks = (k + 1 <= N) ? k + 1 : N;
      const int src = (ks == N) ? Nv + i : ks * (NX + NU) + i;
      Xw[e] = s.rhs[src];
    }
    for (int e = tid; e < N * NU; e += FQ_T) {
      const int k = e / NU, i = e - k * NU;
      const int ks = (k + 1 < N) ? k + 1 : N - 1;
      Uw[e] = s.rhs[ks * (NX + NU) + NX + i];
    }
#pragma unroll
    for (int h = 0; h < FQ_H; ++h) {
      if (R.rok[h]) a.ysc[(int64_t)b * m + R.rr[h]] = R.yr(h);
      if (R.vok[h]) a.ysc[(int64_t)b * m + MD + R.vj[h]] = R.yb_(h);
    }
  }
  if (tid == 0) {
    double u0[NU];
    if (has) {
      u0[0] = s.rhs[NX]; u0[1] = s.rhs[NX + 1]; u0[2] = s.rhs[NX + 2];
    } else {
      u0[0] = Uw[0]; u0[1] = Uw[1]; u0[2] = Uw[2];
    }
    double xn[NX];
    fleet_plant_step(a, b, sx, u0, x, xn);
    a.rho[b] = s.rho_s;
    fleet_record_step(rec, xn, dt);
    rec[11] += res.iter;
    a.lastit[b] = res.iter;
    rec[12] += (res.status == 1) ? 1.0 : 0.0;
    rec[14] = res.factor_fail ? -100 : res.status;
    rec[15] = s.rho_s;
  }
  T.mark(7);
  T.flush();
  if (a.trace && tid == 0) a.trace[(int64_t)b * 4 + 1] = __builtin_amdgcn_s_memrealtime();
}


// gpmpc_qp_solve_batched on this solver (qp.hip picks it): problems whose pattern is the
// fleet's MPC pattern at N = 20 (fleet_qp.h's fixed row layout: dynamics rows 0..MD-1 as
// equalities, then the identity bound rows) -- the host surface's QPWorkspace.solve.  The
// QP data come from global memory instead of the fleet's assembly; rho, the scaled y and
// the outputs are the generic kernel's (k_qp_batched), one problem per workgroup.
__global__ __launch_bounds__(FQ_T) __attribute__((amdgpu_waves_per_eu(FQ_WPE, FQ_WPE))) void k_qp_fleet(
    QPPattern pt, QPSettingsDev st, const double *__restrict__ Aval, const double *__restrict__ Pd,
    const double *__restrict__ q, const double *__restrict__ l, const double *__restrict__ u,
    const double *__restrict__ xws, double *rho, double *yst, double *xo, double *yo, int *iters, int *status,
    double *obj) {
  __shared__ FleetSmem s;
  const int b = blockIdx.x, tid = threadIdx.x, n = pt.n, m = pt.m;
  const double *Ab = Aval + (int64_t)b * pt.nnz;
  FleetRegs R;
  fq_init_pattern(pt, R, n);
  for (int e = tid; e < FQ_NNZD; e += FQ_T) s.A[e] = Ab[e];
#pragma unroll
  for (int h = 0; h < FQ_H; ++h) {
    if (!R.vok[h]) continue;
    const int j = R.vj[h];
    R.P[h] = Pd[(int64_t)b * n + j];
    R.q[h] = q[(int64_t)b * n + j];
    R.x[h] = xws ? xws[(int64_t)b * n + j] : 0.0;
    R.Ab[h] = Ab[FQ_NNZD + j];  // bound row MD + j: its one entry
    R.lb[h] = l[(int64_t)b * m + FQ_MD + j];
    R.ub[h] = u[(int64_t)b * m + FQ_MD + j];
    R.yb_(h) = yst[(int64_t)b * m + FQ_MD + j];
  }
#pragma unroll
  for (int h = 0; h < FQ_H; ++h)
    if (R.rok[h]) {
      R.ur(h) = l[(int64_t)b * m + R.rr[h]];  // l = u (checked by the host)
      R.yr(h) = yst[(int64_t)b * m + R.rr[h]];
    }
  if (tid == 0) s.rho_s = rho[b];
  __syncthreads();
  QPStamps T;
  const QPResult res = fq_solve(pt, s, R, st, &T, 0);
  if (res.factor_fail) {
    if (tid == 0) { status[b] = -100; iters[b] = 0; obj[b] = nan(""); }
    return;
  }
  const bool has = (res.status == 1 || res.status == 2 || res.status == -2);
  const double c = s.c;
#pragma unroll
  for (int h = 0; h < FQ_H; ++h) {
    if (R.vok[h]) {
      const int j = R.vj[h];
      xo[(int64_t)b * n + j] = has ? R.D[h] * R.x[h] : nan("");
      yo[(int64_t)b * m + FQ_MD + j] = has ? s.E[FQ_MD + j] * R.yb_(h) / c : nan("");
      yst[(int64_t)b * m + FQ_MD + j] = R.yb_(h);
    }
    if (R.rok[h]) {
      yo[(int64_t)b * m + R.rr[h]] = has ? s.E[R.rr[h]] * R.yr(h) / c : nan("");
      yst[(int64_t)b * m + R.rr[h]] = R.yr(h);
    }
  }
  if (tid == 0) {
    rho[b] = s.rho_s;
    iters[b] = res.iter;
    status[b] = res.status;
    obj[b] = has ? res.obj : nan("");
  }
}

// this build's launchers (one definition per namespace: each unit that includes this header
// sets its own FQ_KNS)
hipError_t launch_control(hipStream_t s, int nb, const FleetArgs &a, bool stamps) {
  if (stamps)
    hipLaunchKernelGGL(k_fleet_control2<true>, dim3(nb), dim3(FQ_T), 0, s, a);
  else
    hipLaunchKernelGGL(k_fleet_control2<false>, dim3(nb), dim3(FQ_T), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_qp(hipStream_t s, int batch, const QPPattern &pt, const QPSettingsDev &st, const double *Aval,
                     const double *Pd, const double *q, const double *l, const double *u, const double *xws,
                     double *rho, double *yst, double *xo, double *yo, int *iters, int *status, double *obj) {
  hipLaunchKernelGGL(k_qp_fleet, dim3(batch), dim3(FQ_T), 0, s, pt, st, Aval, Pd, q, l, u, xws, rho, yst, xo, yo,
                     iters, status, obj);
  return hipGetLastError();
}
}  // namespace FQ_KNS
