// baseline.hip -- the baseline controllers' landings on the device (reference
// src/experiments/baselines.py: LQRController, PIDController, OpenLoopController, flown by
// MonteCarloSimulator.run_single's "solve" protocol over the Euler plant, bare or inside
// src/experiments/dispersion.py's DispersedDynamics).  One launch flies a whole batch from
// start to termination (gpmpc_baseline_fly).
//
// One landing is a serial chain of a few hundred flops per control step: termination tests,
// the incremental target, the control law, the dispersed plant step, one append to the log.
// Mapping (after safety.hip / §18):
//   - one lane per landing, one wave64 per workgroup; the chain is latency bound and
//     independent across landings;
//   - no divergence inside a wave: a landing that has terminated keeps computing and stops
//     committing (selects); the step loop runs while any lane of the wave is active (__any) and
//     is bounded by max_steps + 1.  No spin-wait, no cross-workgroup traffic, no atomics;
//   - a lane past the batch reruns the last landing and stores nothing, so loads stay in bounds;
//   - gains, clips and scalars are kernel-argument scalars (no by-value arrays: §18's SGPR
//     lesson); K (3 x 7) and u_hover are per landing (they depend on m0) and live in the lane;
//   - the log is step-major [t][landing][10] like k_fleet_mc's: every lane stages its step's
//     ten values in LDS and the wave stores 640 consecutive doubles;
//   - the noise of DispersedDynamics comes from key tables: landing i at plant step s reads
//     thrust row i + s and wind row i + wind_rows[s - 1] (the host's reseed keys), so the tables
//     hold batch + O(max_steps) rows and stay cache resident.
// The plant, the drag term and the landing window restate fleet_control.h's plant_euler,
// drag_residual and landing_ok with alpha, g, Cd and A as runtime values.
#include "internal.h"
#include <cmath>

#define BL_NX 7
#define BL_NU 3
#define BL_WAVE 64
#define BL_ROW 10   // doubles per append: x (7), u (3)

struct BlArgs {
  int B, max_steps, n_ref, thrust_on, wind_kind, drag, log;
  double dt, alpha, g0, g1, g2;
  double T_lo, T_hi, gmax;                                             // LQR clips
  double Kp_z, Ki_z, Kd_z, Kp_xy, Ki_xy, Kd_xy, imax, t_min, t_max, t_lat, pid_dt, pid_g;
  double sim_thrust, sim_aero;                                         // the simulator's own dispersions
  const double *x0, *K, *uh, *Uref, *ttab, *wtab, *cda, *noise;
  const int *wrow;
  double *rec, *logbuf;
  int *nsteps;
};

// LandingConstraints.check_landing with run_experiments.py's tolerances (fleet_control.h's
// landing_ok): 1 and 4 both stop the landing, the host re-decides between them
__device__ __forceinline__ bool bl_landing_ok(const double *x, double m0) {
  if (fabs(x[1]) > 1.0) return false;
  if (fabs(x[2]) > 5.0 || fabs(x[3]) > 5.0) return false;
  if (fabs(x[4]) > 3.0) return false;
  if (fabs(x[5]) > 1.0 || fabs(x[6]) > 1.0) return false;
  if (1.0 - x[0] / m0 > 1.0 - 0.05) return false;
  return true;
}

__device__ __forceinline__ double bl_clip(double v, double lo, double hi) {  // np.clip: a NaN stays
  v = v < lo ? lo : v;
  return v > hi ? hi : v;
}

template <int KIND>
__global__ __launch_bounds__(BL_WAVE) void k_baseline(const BlArgs a) {
  __shared__ double sv[BL_WAVE * BL_ROW];
  __shared__ int sact[BL_WAVE];
  const int lane = threadIdx.x, b0 = blockIdx.x * BL_WAVE;
  const bool live = b0 + lane < a.B;
  const int b = live ? b0 + lane : a.B - 1;
  double x[BL_NX];
#pragma unroll
  for (int i = 0; i < BL_NX; ++i) x[i] = a.x0[(int64_t)b * BL_NX + i];
  const double m0 = x[0];
  double K[BL_NU * BL_NX], uh[BL_NU];
  if (KIND == GPMPC_BASELINE_LQR) {
#pragma unroll
    for (int i = 0; i < BL_NU * BL_NX; ++i) K[i] = a.K[(int64_t)b * (BL_NU * BL_NX) + i];
#pragma unroll
    for (int i = 0; i < BL_NU; ++i) uh[i] = a.uh[(int64_t)b * BL_NU + i];
  }
  double integ[3] = {0.0, 0.0, 0.0};   // the PID's integral state
  const double cda = a.drag ? a.cda[b] : 0.0;
  const double dt = a.dt;
  int out = 0, steps = 0;
  for (int s = 0; s <= a.max_steps; ++s) {
    // termination tests, fleet_control.h's order and constants (monte_carlo.py:458-488)
    bool div = false;
#pragma unroll
    for (int i = 0; i < BL_NX; ++i) div = div || !(fabs(x[i]) <= 1e6);
    int o = 0;
    if (s >= a.max_steps) o = 5;
    else if (x[1] < 0.0) o = 2;
    else if (x[0] <= 1.0 + 0.01) o = 3;
    else if (div) o = 6;
    else if (x[1] < 1.0 && fabs(x[4]) < 5.0) o = bl_landing_ok(x, m0) ? 1 : 4;
    if (out == 0 && o != 0) {
      out = o;
      steps = s;
    }
    const bool act = out == 0;
    if (!__any(act)) break;   // s == max_steps ends every lane: below s < max_steps
    // the incremental target (:497-500): x with zero velocity, 2 below, not under 0.5
    double tgt[BL_NX];
#pragma unroll
    for (int i = 0; i < BL_NX; ++i) tgt[i] = x[i];
    tgt[4] = tgt[5] = tgt[6] = 0.0;
    tgt[1] = fmax(0.5, x[1] - 2.0);
    double u[BL_NU];
    if (KIND == GPMPC_BASELINE_LQR) {   // u = u_hover - K (x - target), clipped
      double dx[BL_NX];
#pragma unroll
      for (int i = 0; i < BL_NX; ++i) dx[i] = x[i] - tgt[i];
#pragma unroll
      for (int r = 0; r < BL_NU; ++r) {
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < BL_NX; ++i) sum += K[r * BL_NX + i] * dx[i];
        u[r] = uh[r] + -sum;
      }
      u[0] = bl_clip(u[0], a.T_lo, a.T_hi);
      u[1] = bl_clip(u[1], -a.gmax, a.gmax);
      u[2] = bl_clip(u[2], -a.gmax, a.gmax);
    } else if (KIND == GPMPC_BASELINE_PID) {
      double pe[3], ve[3], in[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        pe[j] = tgt[1 + j] - x[1 + j];
        ve[j] = tgt[4 + j] - x[4 + j];
        in[j] = bl_clip(integ[j] + pe[j] * a.pid_dt, -a.imax, a.imax);
        if (act) integ[j] = in[j];
      }
      const double tv = a.Kp_z * pe[0] + a.Ki_z * in[0] + a.Kd_z * ve[0];
      u[0] = bl_clip(x[0] * (a.pid_g + tv), a.t_min, a.t_max);
      u[1] = bl_clip((a.Kp_xy * pe[1] + a.Ki_xy * in[1] + a.Kd_xy * ve[1]) * x[0], -a.t_lat, a.t_lat);
      u[2] = bl_clip((a.Kp_xy * pe[2] + a.Ki_xy * in[2] + a.Kd_xy * ve[2]) * x[0], -a.t_lat, a.t_lat);
    } else {   // open loop: row min(step, n_ref - 1) of the shared table
      const int idx = s < a.n_ref - 1 ? s : a.n_ref - 1;
#pragma unroll
      for (int j = 0; j < BL_NU; ++j) u[j] = a.Uref[(int64_t)idx * BL_NU + j];
    }
    // thrust dispersion on the commanded control (dispersion.py:177-190): scale, the two
    // misalignments, the fluctuation; key seed_i + step_count = row b + s + 1 <= B - 1 + max_steps
    double ua[BL_NU] = {u[0], u[1], u[2]};
    if (a.thrust_on) {
      const double *tr = a.ttab + (int64_t)(b + s + 1) * 4;
      ua[0] = ua[0] * tr[0];
      ua[1] = ua[1] + tr[1];
      ua[2] = ua[2] + tr[2];
      ua[0] = ua[0] * tr[3];
    }
    // the Euler step (plant_euler with runtime alpha and g)
    double xn[BL_NX];
    const double tm = sqrt(ua[0] * ua[0] + ua[1] * ua[1] + ua[2] * ua[2]);
    xn[0] = x[0] + dt * -(a.alpha * tm);
    xn[1] = x[1] + dt * x[4];
    xn[2] = x[2] + dt * x[5];
    xn[3] = x[3] + dt * x[6];
    xn[4] = x[4] + dt * (ua[0] / x[0] + a.g0);
    xn[5] = x[5] + dt * (ua[1] / x[0] + a.g1);
    xn[6] = x[6] + dt * (ua[2] / x[0] + a.g2);
    if (a.wind_kind) {   // v += wind dt; row b + wrow[s] < wind rows (checked on the host)
      const double *wr = a.wtab + (int64_t)(b + a.wrow[s]) * 3;
      double f = 1.0;
      if (a.wind_kind == 2) f = fmin(1.0, fmax(x[3], 10.0) / 100.0);   // DRYDEN's altitude factor
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double w = a.wind_kind == 2 ? wr[j] * f : wr[j];
        xn[4 + j] += w * dt;
      }
    }
    if (a.drag) {   // extra drag from the pre-step velocity and mass, |v| > 1 (dispersion.py:349-360)
      const double sp = sqrt(x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
      const double da = cda * (sp * sp) / x[0];
      const bool on = sp > 1.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double d = (da * (x[4 + j] / sp)) * dt;
        xn[4 + j] = on ? xn[4 + j] - d : xn[4 + j];
      }
    }
    if (a.sim_thrust > 0.0 || a.sim_aero > 0.0) {   // k_fleet_mc's draws (monte_carlo.py:531-537)
      const double *nz = a.noise + ((int64_t)b * a.max_steps + s) * 4;
      if (a.sim_thrust > 0.0) {
        const double d = __dmul_rn(__dmul_rn(__dmul_rn(nz[0], a.sim_thrust), u[0]) / x[0], dt);
#pragma unroll
        for (int i = 4; i < BL_NX; ++i) xn[i] = __dadd_rn(xn[i], d);
      }
      if (a.sim_aero > 0.0) {
#pragma unroll
        for (int i = 4; i < BL_NX; ++i) xn[i] = __dadd_rn(xn[i], __dmul_rn(__dmul_rn(nz[i - 3], a.sim_aero), dt));
      }
    }
    // append (x_next, commanded u): staged per lane, stored with consecutive lanes on
    // consecutive doubles; s < max_steps and b0 + l < B for every committed row
#pragma unroll
    for (int i = 0; i < BL_NX; ++i) sv[lane * BL_ROW + i] = xn[i];
#pragma unroll
    for (int i = 0; i < BL_NU; ++i) sv[lane * BL_ROW + BL_NX + i] = u[i];
    sact[lane] = act && live;
    __syncthreads();
    if (a.log) {
      double *dst = a.logbuf + ((int64_t)s * a.B + b0) * BL_ROW;
#pragma unroll
      for (int k = 0; k < BL_ROW; ++k) {
        const int e = lane + BL_WAVE * k, l = e / BL_ROW;
        if (sact[l]) dst[e] = sv[e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < BL_NX; ++i) x[i] = act ? xn[i] : x[i];
  }
  if (live) {   // the fleet's 16-double record; the solver slots stay 0
    double *rec = a.rec + (int64_t)b * GPMPC_REC_LEN;
    rec[0] = out;
    rec[1] = steps;
    rec[2] = m0 - x[0];
    rec[3] = steps * dt;
#pragma unroll
    for (int i = 0; i < BL_NX; ++i) rec[4 + i] = x[i];
    rec[11] = 0.0;
    rec[12] = 0.0;
    rec[13] = m0;
    rec[14] = 0.0;
    rec[15] = 0.0;
    a.nsteps[b] = steps;
  }
}

extern "C" void gpmpc_baseline_default_config(gpmpc_baseline_config *c) {
  if (!c) return;
  *c = gpmpc_baseline_config{};
  c->kind = GPMPC_BASELINE_LQR;
  c->batch = 1;
  c->max_steps = 300;
  c->dt = 0.1;
  c->alpha = 1.0 / 30.0;
  c->g[0] = -1.0;
  c->T_lo = 0.0;
  c->T_hi = 6.5;
  c->gimbal_max = 0.5;
  c->Kp_z = 2.0; c->Ki_z = 0.1; c->Kd_z = 1.5;
  c->Kp_xy = 0.5; c->Ki_xy = 0.01; c->Kd_xy = 0.3;
  c->max_integral = 10.0;
  c->thrust_min = 0.3;
  c->thrust_max = 5.0;
  c->pid_dt = 0.1;
  c->pid_g = 1.0;
  c->log = 1;
}

static bool bl_finite(const double *p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

#define BL_REFUSE(...)                \
  do {                                \
    gpmpc_set_error(__VA_ARGS__);     \
    return -2;                        \
  } while (0)

extern "C" int gpmpc_baseline_fly(gpmpc_ctx *ctx, const gpmpc_baseline_config *cfg, const double *x0, const double *K,
                                  const double *u_hover, const double *U_ref, const double *thrust_table,
                                  const double *wind_table, const int *wind_step_rows, const double *drag_cda,
                                  const double *noise, double *records, int *nsteps, double *log,
                                  double *kernel_ms) {
  if (!ctx || !cfg || !x0 || !records || !nsteps) BL_REFUSE("baseline_fly: ctx, cfg, x0, records and nsteps must not be null");
  const int kind = cfg->kind;
  if (kind != GPMPC_BASELINE_LQR && kind != GPMPC_BASELINE_PID && kind != GPMPC_BASELINE_OPEN_LOOP)
    BL_REFUSE("baseline_fly: unknown controller kind %d", kind);
  if (cfg->batch < 1) BL_REFUSE("baseline_fly: batch = %d, needs at least one landing", cfg->batch);
  if (cfg->max_steps < 1) BL_REFUSE("baseline_fly: max_steps = %d, needs at least one step", cfg->max_steps);
  if (!(cfg->dt > 0.0)) BL_REFUSE("baseline_fly: dt must be positive");
  const size_t B = cfg->batch, T = cfg->max_steps;
  if (B * T > ((size_t)1 << 31) / BL_ROW) BL_REFUSE("baseline_fly: batch x max_steps = %zu is past the log's index range", B * T);
  if (!bl_finite(x0, B * BL_NX)) BL_REFUSE("baseline_fly: x0 is not finite");
  if (kind == GPMPC_BASELINE_LQR) {
    if (!K || !u_hover) BL_REFUSE("baseline_fly: the LQR needs K (batch x 3 x 7) and u_hover (batch x 3)");
    if (!bl_finite(K, B * BL_NU * BL_NX) || !bl_finite(u_hover, B * BL_NU)) BL_REFUSE("baseline_fly: K or u_hover is not finite");
  }
  if (kind == GPMPC_BASELINE_OPEN_LOOP && (cfg->n_ref < 1 || !U_ref)) BL_REFUSE("baseline_fly: the open-loop table is empty");
  if (cfg->thrust_rows != 0 && (!thrust_table || (size_t)cfg->thrust_rows < B + T))
    BL_REFUSE("baseline_fly: the thrust table needs batch + max_steps = %zu rows, has %d", B + T, cfg->thrust_rows);
  if (cfg->wind_kind < 0 || cfg->wind_kind > 2) BL_REFUSE("baseline_fly: unknown wind kind %d", cfg->wind_kind);
  if (cfg->wind_kind) {
    if (!wind_table || !wind_step_rows) BL_REFUSE("baseline_fly: wind needs its table and the per-step rows");
    for (size_t s = 0; s < T; ++s)
      if (wind_step_rows[s] < 0 || (size_t)wind_step_rows[s] + B > (size_t)(cfg->wind_rows < 0 ? 0 : cfg->wind_rows))
        BL_REFUSE("baseline_fly: wind row %d of step %zu plus the batch is outside the table's %d rows", wind_step_rows[s], s + 1,
                  cfg->wind_rows);
  }
  if (cfg->drag && !drag_cda) BL_REFUSE("baseline_fly: drag needs the per-landing coefficients");
  const bool sim = cfg->sim_thrust > 0.0 || cfg->sim_aero > 0.0;
  if (sim && !noise) BL_REFUSE("baseline_fly: a dispersion > 0 needs the noise table (batch x max_steps x 4)");
  if (cfg->log && !log) BL_REFUSE("baseline_fly: log = 1 needs the log buffer (max_steps x batch x 10)");

  BlArgs a{};
  a.B = cfg->batch; a.max_steps = cfg->max_steps; a.n_ref = cfg->n_ref;
  a.thrust_on = cfg->thrust_rows != 0; a.wind_kind = cfg->wind_kind; a.drag = cfg->drag != 0; a.log = cfg->log != 0;
  a.dt = cfg->dt; a.alpha = cfg->alpha; a.g0 = cfg->g[0]; a.g1 = cfg->g[1]; a.g2 = cfg->g[2];
  a.T_lo = cfg->T_lo; a.T_hi = cfg->T_hi; a.gmax = cfg->gimbal_max;
  a.Kp_z = cfg->Kp_z; a.Ki_z = cfg->Ki_z; a.Kd_z = cfg->Kd_z;
  a.Kp_xy = cfg->Kp_xy; a.Ki_xy = cfg->Ki_xy; a.Kd_xy = cfg->Kd_xy;
  a.imax = cfg->max_integral; a.t_min = cfg->thrust_min; a.t_max = cfg->thrust_max;
  a.t_lat = cfg->thrust_max * 0.3;
  a.pid_dt = cfg->pid_dt; a.pid_g = cfg->pid_g;
  a.sim_thrust = cfg->sim_thrust; a.sim_aero = cfg->sim_aero;

  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t nref = kind == GPMPC_BASELINE_OPEN_LOOP ? (size_t)cfg->n_ref : 0;
  const size_t nK = kind == GPMPC_BASELINE_LQR ? B : 0;
  const size_t ntr = a.thrust_on ? (size_t)cfg->thrust_rows : 0, nwr = a.wind_kind ? (size_t)cfg->wind_rows : 0;
  DevBuf logbuf;
  if (a.log && logbuf.alloc(s, sizeof(double) * B * T * BL_ROW) != hipSuccess) {
    gpmpc_set_error("baseline_fly: staging and log buffers: out of memory");
    return -1;
  }
  a.logbuf = logbuf.as<double>();
  // a table the kind or the switches leave unread takes no room (count 0, or a null pointer)
  Stage sg(s);
  sg.in(&a.x0, x0, B * BL_NX);
  sg.in(&a.K, K, nK * BL_NU * BL_NX);
  sg.in(&a.uh, u_hover, nK * BL_NU);
  sg.in(&a.Uref, U_ref, nref * BL_NU);
  sg.in(&a.ttab, thrust_table, ntr * 4);
  sg.in(&a.wtab, wind_table, nwr * 3);
  sg.in(&a.wrow, wind_step_rows, a.wind_kind ? T : 0);
  sg.in(&a.cda, drag_cda, a.drag ? B : 0);
  sg.in(&a.noise, noise, sim ? B * T * 4 : 0);
  sg.out(&a.rec, records, B * GPMPC_REC_LEN);
  sg.out(&a.nsteps, nsteps, B);
  if (int rc = sg.commit("baseline_fly")) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    GPMPC_HIP(hipEventCreate(&e0));
    GPMPC_HIP(hipEventCreate(&e1));
    GPMPC_HIP(hipEventRecord(e0, s));
  }
  const dim3 grid((cfg->batch + BL_WAVE - 1) / BL_WAVE), block(BL_WAVE);
  if (kind == GPMPC_BASELINE_LQR) hipLaunchKernelGGL(k_baseline<GPMPC_BASELINE_LQR>, grid, block, 0, s, a);
  else if (kind == GPMPC_BASELINE_PID) hipLaunchKernelGGL(k_baseline<GPMPC_BASELINE_PID>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_baseline<GPMPC_BASELINE_OPEN_LOOP>, grid, block, 0, s, a);
  hipError_t le = hipGetLastError();
  if (kernel_ms && le == hipSuccess) le = hipEventRecord(e1, s);
  hipError_t de = le == hipSuccess ? sg.download() : le;
  if (kernel_ms) {
    float ms = 0.0f;
    if (de == hipSuccess) de = hipEventElapsedTime(&ms, e0, e1);
    *kernel_ms = ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  GPMPC_HIP(de);
  if (a.log) {   // the steps any landing reached: the log's leading rows
    int tmax = 0;
    for (size_t i = 0; i < B; ++i) tmax = nsteps[i] > tmax ? nsteps[i] : tmax;
    if (tmax > cfg->max_steps) tmax = cfg->max_steps;
    if (tmax > 0) {
      GPMPC_HIP(hipMemcpyAsync(log, logbuf.p, sizeof(double) * (size_t)tmax * B * BL_ROW, hipMemcpyDeviceToHost, s));
      GPMPC_HIP(hipStreamSynchronize(s));
    }
  }
  return 0;
}
