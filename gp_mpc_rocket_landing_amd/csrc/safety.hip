// safety.hip -- the predictive safety filter on the device (reference src/safety/
// safety_filter.py: PredictiveSafetyFilter.filter with _solve_gradient_qp, the path it takes
// without CasADi), batch queries in one call (gpmpc_safety_filter), and the closed loop
// filter -> plant step over T steps in one call (gpmpc_safety_simulate).
//
// One query is a bounded serial chain: a check rollout of the nominal control (N RK4 steps,
// the first with u, the rest under the backup law u_eq - K (x - x_eq)), then, when that is
// unsafe, at most n_iters gradient steps of four rollouts each (the control and its three
// forward differences), then the check rollout of the result.  Mapping:
//   - a quad of lanes per query, sixteen queries per wave64, one wave per workgroup (the chain
//     is latency bound: B = 1024 is 64 workgroups on 64 CUs);
//   - in the gradient phase lane r of the quad rolls out u + fd_eps e_(r-1) (lane 0: u); each
//     forms its own V = dx' P dx, the quad exchanges the four values (__shfl, width 4) and all
//     four lanes apply the same update and projection, so u stays replicated without a
//     broadcast;
//   - the check rollouts run on all four lanes redundantly (straight-line code; the quad's
//     lanes hold the same numbers);
//   - the rocket and the scalars are kernel arguments (scalar registers); K, P, x_eq, u_eq and
//     the bounds are copied to LDS once and read with compile-time offsets (broadcast reads of
//     one address): no per-lane copy of P;
//   - no divergence inside a wave: a quad that is safe, or finished, keeps computing and stops
//     committing (selects); the iteration loop runs while any quad of the wave is active
//     (__any).  Every loop bound is known at launch (n_iters, horizon, T); no spin-wait, no
//     cross-workgroup traffic, no atomics.  A NaN follows the IEEE comparisons as in numpy.
#include "fleet6.h"
#include <cmath>
#include <cstddef>

#define SF_QUADS 16   // queries per wave64
#define SF_WAVE 64

// the uniform tables: K, P, x_eq, u_eq, u_min, u_max, as they lie in gpmpc_safety_config
#define SF_K 0
#define SF_P 42
#define SF_XEQ 238
#define SF_UEQ 252
#define SF_UMIN 255
#define SF_UMAX 258
#define SF_NTAB 261
static_assert(offsetof(gpmpc_safety_config, u_max) + 3 * sizeof(double) - offsetof(gpmpc_safety_config, K) ==
                  SF_NTAB * sizeof(double), "K .. u_max are contiguous doubles");

// the rocket and the scalars are kernel arguments (scalar registers); the tables are staged
// with the inputs and copied to LDS once (a by-value copy of all 261 doubles is hoisted into
// scalar registers and spilled from there into vector lanes: 10 lane reads per FMA)
struct SfArgs {
  R6Rocket rk;
  int horizon, n_iters, have_constraints;
  double dt, alpha, backup_margin, T_min, T_max, cos_theta_max, tan2_gamma, lr, fd_eps;
  int B, T;
  const double *tab;                             // SF_NTAB doubles
  const double *x, *u_nom;                       // filter: (B, 14), (B, 3); simulate: x0, (B, T, 3)
  double *u_safe, *margin, *value, *X;           // simulate: u_safe = U (B, T, 3), X (B, T+1, 14)
  int *flags, *mask, *iters;
};

__shared__ double sf_tab[SF_NTAB];

// an index the compiler cannot see through: the table reads behind it stay where they are used
// (LDS broadcast reads at compile-time offsets) instead of being hoisted out of every loop
__device__ __forceinline__ int sf_base() {
  int o = 0;
  asm volatile("" : "+v"(o));
  return o;
}

// u = u_eq - K (x - x_eq), saturated (np.maximum / np.minimum: a NaN stays a NaN)
__device__ __forceinline__ void sf_backup(const double *x, double *u) {
  const int o = sf_base();
  double dx[R6_NX];
#pragma unroll
  for (int i = 0; i < R6_NX; ++i) dx[i] = x[i] - sf_tab[o + SF_XEQ + i];
#pragma unroll
  for (int r = 0; r < R6_NU; ++r) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < R6_NX; ++i) s += sf_tab[o + SF_K + r * R6_NX + i] * dx[i];
    double v = sf_tab[o + SF_UEQ + r] - s;
    const double lo = sf_tab[o + SF_UMIN + r], hi = sf_tab[o + SF_UMAX + r];
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    u[r] = v;
  }
}

// V = dx' P dx as (dx' P) dx
__device__ __forceinline__ double sf_value(const double *x) {
  const int o = sf_base();
  double dx[R6_NX];
#pragma unroll
  for (int i = 0; i < R6_NX; ++i) dx[i] = x[i] - sf_tab[o + SF_XEQ + i];
  double v = 0.0;
#pragma unroll
  for (int j = 0; j < R6_NX; ++j) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < R6_NX; ++i) t += dx[i] * sf_tab[o + SF_P + i * R6_NX + j];
    v += t * dx[j];
  }
  return v;
}

__device__ __forceinline__ double sf_norm3(const double *u) { return sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]); }

// _check_constraints: thrust shell, tilt, and the glideslope above 0.1 of altitude
__device__ __forceinline__ bool sf_constraints(const SfArgs &a, const double *x, const double *u) {
  if (!a.have_constraints) return true;
  const double tm = sf_norm3(u);
  bool ok = !(tm < a.T_min || tm > a.T_max);
  const double ct = 1 - 2 * (x[8] * x[8] + x[9] * x[9]);
  ok = ok && !(ct < a.cos_theta_max);
  const bool gs = x[1] > 0.1 && (x[1] * x[1]) * a.tan2_gamma < x[2] * x[2] + x[3] * x[3];
  return ok && !gs;
}

// the trajectory "u for one step, then the backup law": its terminal V and, with CHECK, the
// violation mask (bit 0 immediate, bit 1 + k path_k; path_0 is the immediate test again)
template <bool CHECK>
__device__ __forceinline__ double sf_rollout(const SfArgs &a, const double *x0, const double *u0, unsigned &mask) {
  double x[R6_NX], xn[R6_NX], u[R6_NU];
#pragma unroll
  for (int i = 0; i < R6_NX; ++i) x[i] = x0[i];
#pragma unroll
  for (int i = 0; i < R6_NU; ++i) u[i] = u0[i];
  if (CHECK) mask = 0u;
  for (int k = 0; k < a.horizon; ++k) {
    if (k > 0) sf_backup(x, u);
    if (CHECK && !sf_constraints(a, x, u)) mask |= (k == 0 ? 3u : (1u << (1 + k)));
    r6_step(a.rk, x, u, a.dt, xn);
#pragma unroll
    for (int i = 0; i < R6_NX; ++i) x[i] = xn[i];
  }
  return sf_value(x);
}

struct SfOut {
  double u[R6_NU], margin, value;
  unsigned mask;
  int flags, iters;   // flags: bit 0 is_modified, bit 1 is_safe
};

// the whole filter for the quad's query; every lane of the wave calls it (the exchange and the
// vote are wave-wide), the four lanes of a quad with the same x and u_nom
__device__ __forceinline__ void sf_filter(const SfArgs &a, int r, const double *x, const double *un, SfOut &o) {
  unsigned mask;
  double V = sf_rollout<true>(a, x, un, mask);
  double margin = a.alpha - V;
  const bool safe0 = mask == 0u && margin > 0;
  double u[R6_NU] = {un[0], un[1], un[2]};
  int iters = 0;
  bool active = !safe0;
  const double thr = a.alpha * a.backup_margin;
  for (int it = 0; it < a.n_iters; ++it) {
    if (!__any(active)) break;
    double up[R6_NU];
#pragma unroll
    for (int i = 0; i < R6_NU; ++i) up[i] = (r == i + 1) ? u[i] + a.fd_eps : u[i];
    unsigned unused;
    const double Vr = sf_rollout<false>(a, x, up, unused);
    const double V0 = __shfl(Vr, 0, 4);
    double g[R6_NU];
#pragma unroll
    for (int i = 0; i < R6_NU; ++i) g[i] = (__shfl(Vr, i + 1, 4) - V0) / a.fd_eps;
    if (V0 <= thr) active = false;
    double w[R6_NU];
#pragma unroll
    for (int i = 0; i < R6_NU; ++i) w[i] = u[i] - a.lr * (g[i] + 2 * (u[i] - un[i]));
    const double tm = sf_norm3(w);
    if (tm < a.T_min) {
      const double d = fmax(tm, 1e-6);
#pragma unroll
      for (int i = 0; i < R6_NU; ++i) w[i] = w[i] / d * a.T_min;
    } else if (tm > a.T_max) {
#pragma unroll
      for (int i = 0; i < R6_NU; ++i) w[i] = w[i] / tm * a.T_max;
    }
    if (active) {
#pragma unroll
      for (int i = 0; i < R6_NU; ++i) u[i] = w[i];
      ++iters;
    }
  }
  // the check of the filtered control; an unmodified quad keeps the nominal check's numbers
  unsigned mask2 = 0u;
  double V2 = V;
  if (__any(!safe0)) V2 = sf_rollout<true>(a, x, u, mask2);
  if (!safe0) {
    V = V2;
    mask = mask2;
    margin = a.alpha - V2;
  }
#pragma unroll
  for (int i = 0; i < R6_NU; ++i) o.u[i] = u[i];
  o.margin = margin;
  o.value = V;
  o.mask = mask;
  o.iters = iters;
  o.flags = (safe0 ? 0 : 1) | ((mask == 0u && margin > 0) ? 2 : 0);
}

// SIM = false: one filter per query.  SIM = true: the T-step closed loop of every start
template <bool SIM>
__global__ __launch_bounds__(SF_WAVE) void k_safety(const SfArgs a) {
  const int lane = threadIdx.x, r = lane & 3;
  const int q = blockIdx.x * SF_QUADS + (lane >> 2);
  const bool live = q < a.B;
  for (int i = lane; i < SF_NTAB; i += SF_WAVE) sf_tab[i] = a.tab[i];
  __syncthreads();
  const int b = live ? q : a.B - 1;   // a lane past the batch reruns the last query and stores nothing
  double x[R6_NX], un[R6_NU];
#pragma unroll
  for (int i = 0; i < R6_NX; ++i) x[i] = a.x[(int64_t)b * R6_NX + i];
  if (!SIM) {
#pragma unroll
    for (int i = 0; i < R6_NU; ++i) un[i] = a.u_nom[(int64_t)b * R6_NU + i];
    SfOut o;
    sf_filter(a, r, x, un, o);
    if (live && r == 0) {
#pragma unroll
      for (int i = 0; i < R6_NU; ++i) a.u_safe[(int64_t)b * R6_NU + i] = o.u[i];
      a.margin[b] = o.margin;
      a.value[b] = o.value;
      a.flags[b] = o.flags;
      a.mask[b] = (int)o.mask;
      a.iters[b] = o.iters;
    }
    return;
  }
  const bool store = live && r == 0;
  if (store) {
#pragma unroll
    for (int i = 0; i < R6_NX; ++i) a.X[(int64_t)b * (a.T + 1) * R6_NX + i] = x[i];
  }
  for (int t = 0; t < a.T; ++t) {
    const int64_t row = (int64_t)b * a.T + t;
#pragma unroll
    for (int i = 0; i < R6_NU; ++i) un[i] = a.u_nom[row * R6_NU + i];
    SfOut o;
    sf_filter(a, r, x, un, o);
    double xn[R6_NX];
    r6_step(a.rk, x, o.u, a.dt, xn);
#pragma unroll
    for (int i = 0; i < R6_NX; ++i) x[i] = xn[i];
    if (store) {
#pragma unroll
      for (int i = 0; i < R6_NU; ++i) a.u_safe[row * R6_NU + i] = o.u[i];
      a.margin[row] = o.margin;
      a.flags[row] = o.flags;
      a.iters[row] = o.iters;
#pragma unroll
      for (int i = 0; i < R6_NX; ++i) a.X[((int64_t)b * (a.T + 1) + t + 1) * R6_NX + i] = x[i];
    }
  }
}

extern "C" void gpmpc_safety_default_config(gpmpc_safety_config *c) {
  if (!c) return;
  *c = gpmpc_safety_config{};
  c->horizon = 10;
  c->dt = 0.1;
  for (int i = 0; i < 3; ++i) {
    c->u_min[i] = -INFINITY;
    c->u_max[i] = INFINITY;
  }
  c->alpha = 1.0;
  c->backup_margin = 0.9;
  c->have_constraints = 0;
  c->T_min = 0.5;
  c->T_max = 5.0;
  c->cos_theta_max = 0.5000000000000001;    // np.cos(np.deg2rad(60.0))
  c->tan2_gamma = 0.3333333333333333;       // np.tan(np.deg2rad(30.0)) ** 2
  c->n_iters = 50;
  c->lr = 0.1;
  c->fd_eps = 1e-4;
}

static int sf_check(const char *what, const double *rocket, const gpmpc_safety_config *cfg, int batch, SfArgs &a) {
  if (batch < 1) {
    gpmpc_set_error("%s: batch = %d, needs at least one query", what, batch);
    return -2;
  }
  if (cfg->horizon < 1 || cfg->horizon > 31) {
    gpmpc_set_error("%s: horizon = %d is outside 1..31 (the violation mask's width)", what, cfg->horizon);
    return -2;
  }
  if (!(cfg->dt > 0.0)) {
    gpmpc_set_error("%s: dt must be positive", what);
    return -2;
  }
  if (cfg->n_iters < 0) {
    gpmpc_set_error("%s: n_iters must not be negative", what);
    return -2;
  }
  if (r6_rocket(rocket, a.rk, what)) return -2;
  a.horizon = cfg->horizon;
  a.n_iters = cfg->n_iters;
  a.have_constraints = cfg->have_constraints;
  a.dt = cfg->dt;
  a.alpha = cfg->alpha;
  a.backup_margin = cfg->backup_margin;
  a.T_min = cfg->T_min;
  a.T_max = cfg->T_max;
  a.cos_theta_max = cfg->cos_theta_max;
  a.tan2_gamma = cfg->tan2_gamma;
  a.lr = cfg->lr;
  a.fd_eps = cfg->fd_eps;
  a.B = batch;
  return 0;
}

extern "C" int gpmpc_safety_filter(gpmpc_ctx *ctx, const double *rocket, const gpmpc_safety_config *cfg, int batch,
                                   const double *x, const double *u_nom, double *u_safe, double *margin,
                                   double *backup_value, int *flags, int *viol_mask, int *iters) {
  GPMPC_CHECK_ARG(ctx && rocket && cfg && x && u_nom && u_safe && margin && backup_value && flags && viol_mask &&
                  iters);
  SfArgs a{};
  if (sf_check("safety_filter", rocket, cfg, batch, a)) return -2;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch;
  Stage sg(s);
  a.T = 0;
  sg.in(&a.tab, cfg->K, SF_NTAB);
  sg.in(&a.x, x, B * R6_NX);
  sg.in(&a.u_nom, u_nom, B * R6_NU);
  sg.out(&a.u_safe, u_safe, B * R6_NU);
  sg.out(&a.margin, margin, B);
  sg.out(&a.value, backup_value, B);
  sg.out(&a.flags, flags, B);
  sg.out(&a.mask, viol_mask, B);
  sg.out(&a.iters, iters, B);
  if (int rc = sg.commit("safety_filter")) return rc;
  hipLaunchKernelGGL(k_safety<false>, dim3((batch + SF_QUADS - 1) / SF_QUADS), dim3(SF_WAVE), 0, s, a);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}

extern "C" int gpmpc_safety_simulate(gpmpc_ctx *ctx, const double *rocket, const gpmpc_safety_config *cfg, int batch,
                                     int T, const double *x0, const double *U_nom, double *X, double *U,
                                     double *margin, int *flags, int *iters) {
  GPMPC_CHECK_ARG(ctx && rocket && cfg && x0 && U_nom && X && U && margin && flags && iters && T >= 0);
  SfArgs a{};
  if (sf_check("safety_simulate", rocket, cfg, batch, a)) return -2;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t B = batch, BT = B * (size_t)T;
  Stage sg(s);
  a.T = T;
  sg.in(&a.tab, cfg->K, SF_NTAB);
  sg.in(&a.x, x0, B * R6_NX);
  sg.in(&a.u_nom, U_nom, BT * R6_NU);
  sg.out(&a.X, X, B * (T + 1) * R6_NX);
  sg.out(&a.u_safe, U, BT * R6_NU);
  sg.out(&a.margin, margin, BT);
  sg.out(&a.flags, flags, BT);
  sg.out(&a.iters, iters, BT);
  if (int rc = sg.commit("safety_simulate")) return rc;
  hipLaunchKernelGGL(k_safety<true>, dim3((batch + SF_QUADS - 1) / SF_QUADS), dim3(SF_WAVE), 0, s, a);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}
