// fleet.hip -- a batch of closed-loop 3-DoF GP-MPC landings, device-resident.
//
// One control step for every landing b:
//   1. k_fleet_queries   Simple3DoF features (features.py:403-444) of the N
//                        horizon points of b's linearisation trajectory
//                        (X_lin, U_lin = shifted previous solution: RTI), scaled
//                        by the kernel lengthscales (fleet_query_row; at fleet sizes the
//                        row-tiled gram kernel forms them itself and this launch is skipped);
//   2. GP posterior      K* = k(Z*, X) (gram kernel), mean = K* alpha and
//                        var = sigma2 - |L^-1 K*^T|^2 on the FP64-MFMA GEMM with
//                        fused sum-of-squares epilogue (gemm.hip) -- all B*N
//                        queries in one batched pass over one shared factor;
//   3. k_fleet_control   one workgroup per landing: Monte-Carlo termination
//                        checks (monte_carlo.py:455-488), target (monte_carlo.py
//                        :497-500 or fixed), RTI QP assembly with analytic
//                        Jacobians (osqp_rti.py:656-710) and the GP mean on the
//                        velocity rows of c_k with the correct sign (gp_mpc.py
//                        :309-314, 410-411), the OSQP-style ADMM of
//                        qp_device.h, the plant step (nominal Euler + the aero
//                        residual the GP learns) and the warm-start shift;
//   4. k_fleet_mc        only with the Monte-Carlo attachment (gpmpc_fleet_mc_attach):
//                        the plant dispersions of monte_carlo.py:530-537 from a host
//                        noise table and the step-major trajectory log (:539-544).
//
// This unit holds the host side and the kernels that exist once, k_fleet_control (the
// generic solver of qp_device.h, any horizon) among them.  The control step on the
// fleet-specialised solver, k_fleet_control2, is fleet_control.h: compiled here as its
// 128-thread build (fq_narrow) and in fleet_wide.hip as its 256-thread build (fq_wide).
#include "internal.h"
#include "gemm.h"
#include "fleet_control.h"
#include <climits>
#include <mutex>
#include <vector>
#include <algorithm>

struct gpmpc_fleet {
  gpmpc_ctx *ctx = nullptr;
  gpmpc_gp *gp = nullptr;
  gpmpc_fleet_config cfg{};
  int B = 0, N = 0, n = 0, m = 0;
  int gp_n = 0;  // training rows of the GP when the GP scratch was sized
  // upper bound on the running landings, refreshed whenever the host reads the
  // records (landings only terminate between resets): with the dispatch order
  // putting running landings first, the GP posterior and the control launch
  // cover only the first n_active slots
  int n_active = 0;
  QPPatternHost pat;
  DevBuf x, Xw, Uw, ysc, rho, rec, xt;      // landing state
  DevBuf Q, Qn, Ks, part, meanT, mean, var;  // GP scratch
  DevBuf order, lastit;                      // dispatch order: longest predicted solve first
  unsigned long long *stamps = nullptr;      // diagnostic (gpmpc_fleet_set_stamps)
  unsigned long long *trace = nullptr;       // diagnostic (gpmpc_fleet_set_trace)
  bool use_order = true;                     // GPMPC_FLEET_ORDER=0 launches in landing order
  bool use_fq = true;                        // fleet-specialised solver (GPMPC_FLEET_SOLVER=0: generic)
  bool wide = false;                         // its 256-thread build (fleet_wide.hip): fleets of <= 1 landing per CU
  int alt_wave = 0;                          // GPMPC_FLEET_ALTWAVE=1: alternate the chain wave
  DevBuf claims;                             // per-CU chain-SIMD claims (k_fleet_control2)
  DevBuf sqp_done;                           // SQP mode: landing converged this control step
  int sqp_it = 0;                            // SQP mode: pass of the current control step
  unsigned epoch = 0;                        // control launches so far (claim generation)
  bool simd_pick = true;                     // GPMPC_FLEET_SIMD=0: chain on wave 0 always
  bool fuse_post = true;                     // GPMPC_FLEET_FUSE_POST=0: separate k_post_finish
  int64_t post_P = 0;                        // query rows / partial row tiles of the last
  int post_nrt = 0;                          //   posterior GEMM (fused finish reads them)
  int query_launches = 0;                    // k_fleet_queries launches so far (diagnostic)
  // Every size-dependent path choice is made once, at creation, for plan_B landings (the
  // fleet's own size, or the whole Monte-Carlo fleet this one is a shard of): the kernels
  // differ in summation order, so choosing them from the running count or the shard size
  // would make a landing's bits depend on how many others fly beside it
  int plan_B = 0;
  int post_kind = 0;                         // posterior GEMM kernel (gemm_sumsq_kind at plan_B N)
  bool post_few = false;                     // queries + K* in one launch (<= 64 planned query rows)
  // a sparse GP (FITC or VFE, gpmpc_fleet_create_fitc) instead of the exact one: the
  // posterior is K*u against the inducing rows, mean K*u alpha as the reference writes it
  // (sparse_gp.py:280-283), variance sigma2 - |L_uu^-1 k*|^2 + |W2 k*|^2
  gpmpc_fitc *fitc = nullptr;
  DevBuf part2;                              // |W2 k*|^2 partials
  int post_kind2 = 0, post_nrt2 = 0;
  // Monte-Carlo protocol attachment (gpmpc_fleet_mc_attach; pooled on the context's
  // stream): plant dispersions from a host-drawn noise table and the trajectory log
  bool mc = false;
  double mc_thrust = 0.0, mc_aero = 0.0;
  int mc_log_steps = 0;                      // 0: no log, else cfg.max_steps
  DevBuf mc_noise;                           // batch x max_steps x 4 standard normals (or empty)
  DevBuf mc_u0;                              // batch x 3: the control kernel's applied control
  DevBuf mc_cnt;                             // batch: appends so far (= the landing's steps)
  DevBuf mc_mprev;                           // batch: mass at the last append (pre-step mass)
  DevBuf mc_x0;                              // batch x 7: states[0] of every landing's log
  DevBuf mc_logbuf;                          // step-major [t][landing][10]: x_{t+1}, u_t
};

// the GP the fleet reads: its exact GP, or the sparse one's inducing-point view
static GpView fleet_view(const gpmpc_fleet *f) { return f->fitc ? fitc_view(f->fitc) : gp_view(f->gp); }

extern "C" int gpmpc_fleet_set_stamps(gpmpc_fleet *f, void *dev_u64x16) {
  GPMPC_CHECK_ARG(f);
  f->stamps = (unsigned long long *)dev_u64x16;
  return 0;
}

extern "C" int gpmpc_fleet_set_trace(gpmpc_fleet *f, void *dev_u64xbx4) {
  GPMPC_CHECK_ARG(f);
  f->trace = (unsigned long long *)dev_u64xbx4;
  return 0;
}

extern "C" void gpmpc_fleet_default_config(gpmpc_fleet_config *c) {
  c->horizon = 20;           // BASELINE config: N = 20
  c->dt = 0.1;               // MPCConfig.dt / SimulationConfig.dt
  c->target_mode = 1;        // solve protocol of MonteCarloSimulator (GPMPC surface)
  c->use_gp = 1;
  c->residual_model = 1;
  c->max_steps = 300;        // run_experiments.py SimulationConfig max_time 30 s / dt
  gpmpc_qp_default_settings(&c->qp);
  c->sqp_iters = 1;          // RTI; > 1: GPMPC.solve's loop (gp_mpc.py:296-345)
  c->sqp_tol = 1e-4;         // gp_mpc.py:343
  c->sqp_qp = c->qp;         // the SQP passes' QP settings: max_iter 0 = "the same as qp",
  c->sqp_qp.max_iter = 0;    // resolved at launch, so later edits of qp reach the passes too
}

// ---------------------------------------------------------------------------
// structural CSR of the 3-DoF MPC QP (unfiltered: SURVEY D3 zeros kept)
static void mpc_pattern(int N, std::vector<int> &rp, std::vector<int> &ci) {
  const int n = (N + 1) * NX + N * NU, m = NX * (N + 1) + n;
  rp.assign(1, 0);
  ci.clear();
  auto row = [&](std::initializer_list<int> cols) {
    for (int c : cols) ci.push_back(c);
    rp.push_back((int)ci.size());
  };
  for (int i = 0; i < NX; ++i) row({i});
  for (int k = 0; k < N; ++k) {
    const int o = k * (NX + NU), on = (k + 1) * (NX + NU);
    row({o + 0, o + 7, o + 8, o + 9, on + 0});  // mass: A00, B0j, -1
    row({o + 1, o + 4, on + 1});                // r: A_ii, dt, -1
    row({o + 2, o + 5, on + 2});
    row({o + 3, o + 6, on + 3});
    row({o + 0, o + 4, o + 7, on + 4});         // v: A_i0, A_ii, B, -1
    row({o + 0, o + 5, o + 8, on + 5});
    row({o + 0, o + 6, o + 9, on + 6});
  }
  for (int j = 0; j < n; ++j) row({j});
  (void)m;
}

// GPMPC.solve's loop: X_pred[0] = x0 (gp_mpc.py:263) -- before the first pass of
// a control step the unshifted plan's first point becomes the current state
__global__ void k_fleet_x0_to_plan(int B, int N, const double *__restrict__ x, const double *__restrict__ rec,
                                   double *__restrict__ Xw) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= B * NX) return;
  const int b = g / NX, i = g - b * NX;
  if (rec[(int64_t)b * GPMPC_REC_LEN] != 0.0) return;
  Xw[(int64_t)b * (N + 1) * NX + i] = x[g];
}

__global__ void k_fleet_queries(int B, int N, const double *__restrict__ Xw,
                                const double *__restrict__ Uw, const double *__restrict__ ls,
                                int iso, const int *__restrict__ order, double *__restrict__ Q,
                                double *__restrict__ Qn) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;  // = slot*N + k
  if (g >= B * N) return;
  double v[NFEAT];
  Qn[g] = fleet_query_row(FleetPlans{Xw, Uw, ls, order, N, iso}, g, v);
#pragma unroll
  for (int f = 0; f < NFEAT; ++f) Q[(int64_t)g * NFEAT + f] = v[f];
}

// The queries and K* in one launch for a fleet of at most 64 query rows (one to three
// landings: the single-landing step): every workgroup forms all the rows' features in LDS
// (k_fleet_queries' arithmetic) and its 64 training columns of K* as k_gram does (same
// fma order, same kernel_epilogue: the same bits as the two-launch path).
__global__ __launch_bounds__(256) void k_fleet_queries_gram(int B, int N, const double *__restrict__ Xw,
                                                            const double *__restrict__ Uw,
                                                            const double *__restrict__ ls, int iso,
                                                            const int *__restrict__ order, int kind,
                                                            const double *__restrict__ Xs,
                                                            const double *__restrict__ Xn, int n, double sigma2,
                                                            double iso_scale, double *__restrict__ Ks) {
  __shared__ double sq[64][NFEAT + 1];
  __shared__ double sqn[64];
  const int P = B * N, tid = threadIdx.x;
  if (tid < P) {
    double v[NFEAT];
    sqn[tid] = fleet_query_row(FleetPlans{Xw, Uw, ls, order, N, iso}, tid, v);
#pragma unroll
    for (int f = 0; f < NFEAT; ++f) sq[tid][f] = v[f];
  }
  __syncthreads();
  const int col = blockIdx.x * 64 + (tid & 63), rg = tid >> 6;
  if (col >= n) return;
  double bj[NFEAT];
#pragma unroll
  for (int k = 0; k < NFEAT; ++k) bj[k] = Xs[(int64_t)col * NFEAT + k];
  const double nbj = Xn[col];
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rg * 16 + rr;
    if (row >= P) break;
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < NFEAT; ++k) dot = fma(sq[row][k], bj[k], dot);
    const double d2 = (sqn[row] + nbj) - 2.0 * dot;
    Ks[(int64_t)row * n + col] = kernel_epilogue(kind, d2, sigma2, iso_scale);
  }
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fleet_control(FleetArgs a) {
  __shared__ QPSmemStd s;
  __shared__ double sx[NX], st_tgt[NX];
  __shared__ int s_out;
  const int b = a.order ? a.order[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int N = a.N, n = a.pt.n, m = a.pt.m;
  const double dt = a.dt;
  double *rec = a.rec + (int64_t)b * GPMPC_REC_LEN;
  if (rec[0] != 0.0) return;  // terminated landing
  if (a.sqp && !a.sqp_first && a.sqp_done[b]) return;  // converged in an earlier SQP pass
  QPStamps T;
  T.out = (b == 0) ? a.stamps : nullptr;
  T.start();
  if (a.trace && tid == 0) {
    unsigned long long *tr = a.trace + (int64_t)b * 4;
    tr[0] = __builtin_amdgcn_s_memrealtime();
    tr[2] = (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11));   // HW_ID: wave, simd, cu, sh, se
    tr[3] = (unsigned)__builtin_amdgcn_s_getreg(20 | (31 << 11));  // XCC_ID
  }
  double *x = a.x + (int64_t)b * NX;
  double *Xw = a.Xw + (int64_t)b * (N + 1) * NX;
  double *Uw = a.Uw + (int64_t)b * N * NU;
  if (tid < NX) sx[tid] = x[tid];
  __syncthreads();
  // ---- termination checks at the top of the step (monte_carlo.py:458-488)
  if (tid == 0) {  // (twin: k_fleet_control2, fleet_control.h; a change goes into both)
    int out = 0;
    const double m0 = rec[13];
    bool div = false;
    for (int i = 0; i < NX; ++i) div = div || !(fabs(sx[i]) <= 1e6);
    if (a.sqp && !a.sqp_first) out = 0;                         // later SQP passes: checks done
    else if ((int)rec[1] >= a.max_steps) out = 5;               // TIMEOUT
    else if (sx[1] < 0.0) out = 2;                              // CRASH
    else if (sx[0] <= 1.0 + 0.01) out = 3;                      // FUEL_EXHAUSTED
    else if (div) out = 6;                                      // DIVERGENCE
    else if (sx[1] < 1.0 && fabs(sx[4]) < 5.0) out = landing_ok(sx, m0) ? 1 : 4;
    if (a.sqp && a.sqp_first) a.sqp_done[b] = 0;  // a new control step: no pass has converged
    s_out = out;
    // target: incremental (monte_carlo.py:497-500) or fixed
    for (int i = 0; i < NX; ++i) st_tgt[i] = a.target_mode ? sx[i] : a.xt[(int64_t)b * NX + i];
    if (a.target_mode) {
      st_tgt[4] = st_tgt[5] = st_tgt[6] = 0.0;
      st_tgt[1] = fmax(0.5, sx[1] - 2.0);
    }
  }
  __syncthreads();
  if (s_out) {
    if (tid == 0) fleet_record_stop(rec, sx, s_out);
    return;
  }
  // ---- QP data (osqp_rti.py:203-372 with the GPMPC sign), straight into LDS
  const int Nv = N * (NX + NU);
  for (int j = tid; j < n; j += nt) {
    double p, qq;
    // (twin: k_fleet_control2, fleet_control.h; a change goes into both)
    if (j >= Nv) {               // x_N block: Q_f = 10 Q
      const int i = j - Nv;
      const double qd = (i == 0) ? 0.0 : (i < 4 ? 100.0 : 10.0);
      p = qd; qq = -qd * st_tgt[i];
    } else {
      const int k = j / (NX + NU), i = j - k * (NX + NU);
      if (i < NX) {
        const double qd = (i == 0) ? 0.0 : (i < 4 ? 10.0 : 1.0);
        p = qd; qq = -qd * st_tgt[i];
      } else {
        p = 0.01; qq = 0.0;
      }
      (void)k;
    }
    s.P[j] = p;
    s.q[j] = qq;
    // warm start / linearisation point vector
    if (j >= Nv) s.x[j] = Xw[N * NX + (j - Nv)];
    else {
      const int k = j / (NX + NU), i = j - k * (NX + NU);
      s.x[j] = (i < NX) ? Xw[k * NX + i] : Uw[k * NU + (i - NX)];
    }
  }
  // x0 rows and bound rows
  for (int r = tid; r < m; r += nt) {
    if (r < NX) {
      s.A[r] = 1.0;
      s.l[r] = sx[r];
      s.u[r] = sx[r];
    } else if (r >= NX * (N + 1)) {
      const int j = r - NX * (N + 1);
      s.A[NX + N * DYN_NNZ + j] = 1.0;
      double lo, hi;
      const int i = (j >= Nv) ? j - Nv : j % (NX + NU);
      fleet_box(i, lo, hi);
      s.l[r] = lo;
      s.u[r] = hi;
    }
  }
  // dynamics blocks: one thread per stage k
  for (int k = tid; k < N; k += nt) {
    const double *xk = Xw + k * NX;
    const double *uk = Uw + k * NU;
    // (twin: k_fleet_control2, fleet_control.h; a change goes into both)
    const double mk = xk[0], tx = uk[0], ty = uk[1], tz = uk[2];
    const double tm = sqrt(tx * tx + ty * ty + tz * tz) + 1e-10;
    const double al = 1.0 / 30.0;
    // FastRTI3DoF._linearize (osqp_rti.py:656-710)
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
    // c_k = f(x,u) - A x - B u (+ dt * GP mean on the velocity rows)
    double f[NX];
    plant_euler(xk, uk, dt, f);
    // (f - A x) - B u, as osqp_rti.py:340-341 evaluates it
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
    const double *gm = a.gmean + ((int64_t)(a.gp_by_slot ? (int)blockIdx.x : b) * N + k) * 3;
    for (int i = 0; i < NX; ++i) {
      double c = (f[i] - ax[i]) - bu[i];
      if (a.use_gp && i >= 4) c += gm[i - 4] * dt;
      const int r = NX * (k + 1) + i;
      s.l[r] = -c;   // A x + B u - x+ = -c   <=>   x+ = A x + B u + c
      s.u[r] = -c;
    }
  }
  for (int r = tid; r < m; r += nt) s.y[r] = a.ysc[(int64_t)b * m + r];
  if (tid == 0) s.rho_s = a.rho[b];
  __syncthreads();
  T.mark(0);
  // ---- ADMM (qp_device.h)
  QPResult res = qp_solve(a.pt, s, a.st, &T);
  T.mark(7);
  const bool has = !res.factor_fail && (res.status == 1 || res.status == 2 || res.status == -2);
  // ---- solution, plant step, warm-start shift
  if (has) {
    for (int j = tid; j < n; j += nt) s.x[j] = s.D[j] * s.x[j];  // unscale
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
    // GPMPC.solve's loop (gp_mpc.py:336-353), as k_fleet_control2: the change of the
    // trajectory, X_pred <- X_new (no shift), stop below sqp_tol
    __shared__ double s_dm[4];
    double dm = 0.0;
    for (int j = tid; j < n; j += nt) {
      const int i = (j >= Nv) ? j - Nv : j % (NX + NU), k = j / (NX + NU);
      const double old = (j >= Nv) ? Xw[N * NX + i] : (i < NX ? Xw[k * NX + i] : Uw[k * NU + i - NX]);
      dm = fmax(dm, fabs(s.x[j] - old));
    }
    for (int o = 32; o > 0; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o));
    if ((tid & 63) == 0) s_dm[tid >> 6] = dm;
    __syncthreads();  // (also orders every read of Xw / Uw before the writes)
    dm = s_dm[0];
    for (int w = 1; w < nt / 64; ++w) dm = fmax(dm, s_dm[w]);
    for (int e = tid; e < (N + 1) * NX; e += nt) {
      const int k = e / NX, i = e - k * NX;
      Xw[e] = s.x[(k == N) ? Nv + i : k * (NX + NU) + i];
    }
    for (int e = tid; e < N * NU; e += nt) {
      const int k = e / NU, i = e - k * NU;
      Uw[e] = s.x[k * (NX + NU) + NX + i];
    }
    for (int r = tid; r < m; r += nt) a.ysc[(int64_t)b * m + r] = s.y[r];
    if (tid == 0) {
      const bool conv = dm < a.sqp_tol;
      a.rho[b] = s.rho_s;
      rec[11] += res.iter;
      a.lastit[b] = res.iter;
      rec[12] += (res.status == 1) ? 1.0 : 0.0;
      rec[14] = res.status;
      rec[15] = s.rho_s;
      if (conv) {
        const double u0[NU] = {s.x[NX], s.x[NX + 1], s.x[NX + 2]};
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
    // shifted solution -> next linearisation point (X[1:], X[-1]), (U[1:], U[-1])
    for (int e = tid; e < (N + 1) * NX; e += nt) {
      const int k = e / NX, i = e - k * NX;
      const int ks = (k + 1 <= N) ? k + 1 : N;
      const int src = (ks == N) ? Nv + i : ks * (NX + NU) + i;
      Xw[e] = s.x[src];
    }
    for (int e = tid; e < N * NU; e += nt) {
      const int k = e / NU, i = e - k * NU;
      const int ks = (k + 1 < N) ? k + 1 : N - 1;
      Uw[e] = s.x[ks * (NX + NU) + NX + i];
    }
    for (int r = tid; r < m; r += nt) a.ysc[(int64_t)b * m + r] = s.y[r];
  }
  if (tid == 0) {
    double u0[NU];
    if (has) {
      u0[0] = s.x[NX]; u0[1] = s.x[NX + 1]; u0[2] = s.x[NX + 2];
    } else {  // step protocol fallback: shifted previous plan (osqp_rti.py:546-552)
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

// the fleet solver's pattern: the MPC pattern at N = 20 (fleet_qp.h's compiled sizes)
static_assert(FQ_MD == QP_FLEET_MD, "qp.h's copy of the dynamics row count");
bool qp_is_fleet_pattern(int n, int m, const int *rowptr, const int *colidx) {
  static std::vector<int> rp, ci;
  static std::once_flag once;
  std::call_once(once, [] { mpc_pattern(20, rp, ci); });
  const int nv = (20 + 1) * NX + 20 * NU;
  if (n != nv || m + 1 != (int)rp.size() || rowptr[m] != (int)ci.size()) return false;
  return !memcmp(rowptr, rp.data(), sizeof(int) * rp.size()) && !memcmp(colidx, ci.data(), sizeof(int) * ci.size());
}

// initial linearisation point: X linear to the target, U hover (osqp_rti.py:425-446)
__global__ void k_fleet_reset(int first, int count, int N, int target_mode,
                              const double *__restrict__ x0, double *x, double *Xw, double *Uw,
                              double *ysc, int m, double *rho, double rho0, double *rec,
                              double *xt) {
  const int i = blockIdx.x;
  if (i >= count) return;
  const int b = first + i;
  const double *xi = x0 + (int64_t)i * NX;
  double tg[NX];
  for (int c = 0; c < NX; ++c) tg[c] = 0.0;
  tg[0] = xi[0];                       // x_target = [m0, 0, ...] (monte_carlo.py:428-430)
  if (target_mode) {
    for (int c = 0; c < NX; ++c) tg[c] = xi[c];
    tg[4] = tg[5] = tg[6] = 0.0;
    tg[1] = fmax(0.5, xi[1] - 2.0);
  }
  for (int e = threadIdx.x; e < (N + 1) * NX; e += blockDim.x) {
    const int k = e / NX, c = e - k * NX;
    const double al = (double)k / N;
    Xw[(int64_t)b * (N + 1) * NX + e] = (1.0 - al) * xi[c] + al * tg[c];
  }
  for (int e = threadIdx.x; e < N * NU; e += blockDim.x)
    Uw[(int64_t)b * N * NU + e] = (e % NU == 0) ? xi[0] * 1.0 : 0.0;
  for (int r = threadIdx.x; r < m; r += blockDim.x) ysc[(int64_t)b * m + r] = 0.0;
  if (threadIdx.x < GPMPC_REC_LEN) rec[(int64_t)b * GPMPC_REC_LEN + threadIdx.x] = 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int c = 0; c < NX; ++c) {
      x[(int64_t)b * NX + c] = xi[c];
      xt[(int64_t)b * NX + c] = tg[c];
      rec[(int64_t)b * GPMPC_REC_LEN + 4 + c] = xi[c];
    }
    rec[(int64_t)b * GPMPC_REC_LEN + 13] = xi[0];
    rho[b] = rho0;
  }
}

// ---------------------------------------------------------------------------
// Monte-Carlo protocol attachment (gpmpc_fleet_mc_attach): MonteCarloSimulator.run_single's
// plant dispersions (monte_carlo.py:530-537) and its trajectory lists (:539-544), after the
// control kernel of every control step (in SQP mode after the last pass).
//
// A landing whose step count advanced in this step (rec[1] = its append count + 1; one that
// terminated or diverged appends nothing: the break before the append, :455-544) gets
//   v_next += (n0 thrust_dispersion) u0[0] / m_prev dt,  v_next += (n[1:4] aero_dispersion) dt
// in the reference's order and roundings (no contraction), written to the plant state and
// the record's state slots, and appends (x_{t+1}, u0_t) to the log at its own count t.
//
// One thread per landing does the arithmetic (a few flops) and stages its ten values in
// LDS; the workgroup's 64 landings then append with consecutive threads on consecutive
// doubles: the log is step-major, [t][landing][10], and landings reset together share t, so
// one step's appends are one contiguous range of the fleet (640 doubles per workgroup)
// instead of 80-byte pieces 2.4 KB x max_steps apart.  One small launch per control step.
struct FleetMcArgs {
  int B, max_steps, log;
  double dt, thrust, aero;
  const double *noise, *u0;
  double *x, *rec, *mprev, *logbuf;
  int *cnt;
};
#define MC_LPB 64   // landings per workgroup
#define MC_ROW 10   // doubles per append: x (7), u0 (3)

__global__ __launch_bounds__(256) void k_fleet_mc(FleetMcArgs a) {
  __shared__ double sv[MC_LPB][MC_ROW];
  __shared__ int st[MC_LPB];
  const int tid = threadIdx.x, b0 = blockIdx.x * MC_LPB;
  if (tid < MC_LPB) {
    const int b = b0 + tid;
    int t = -1;
    if (b < a.B) {
      double *rec = a.rec + (int64_t)b * GPMPC_REC_LEN;
      const int c = a.cnt[b];
      if ((int)rec[1] == c + 1 && c >= 0 && c < a.max_steps) {
        t = c;
        double xn[NX], u[NU];
        for (int i = 0; i < NX; ++i) xn[i] = a.x[(int64_t)b * NX + i];
        for (int i = 0; i < NU; ++i) u[i] = a.u0[(int64_t)b * NU + i];
        if (a.thrust > 0.0 || a.aero > 0.0) {
          const double *nz = a.noise + ((int64_t)b * a.max_steps + t) * 4;
          if (a.thrust > 0.0) {  // thrust_noise * u[0] / x[0] * dt (monte_carlo.py:532-533)
            const double d = __dmul_rn(__dmul_rn(__dmul_rn(nz[0], a.thrust), u[0]) / a.mprev[b], a.dt);
            for (int i = 4; i < NX; ++i) xn[i] = __dadd_rn(xn[i], d);
          }
          if (a.aero > 0.0)      // aero_noise * dt (:536-537)
            for (int i = 4; i < NX; ++i)
              xn[i] = __dadd_rn(xn[i], __dmul_rn(__dmul_rn(nz[i - 3], a.aero), a.dt));
          for (int i = 4; i < NX; ++i) {
            a.x[(int64_t)b * NX + i] = xn[i];
            rec[4 + i] = xn[i];
          }
        }
        a.mprev[b] = xn[0];
        a.cnt[b] = c + 1;
        for (int i = 0; i < NX; ++i) sv[tid][i] = xn[i];
        for (int i = 0; i < NU; ++i) sv[tid][NX + i] = u[i];
      }
    }
    st[tid] = t;
  }
  __syncthreads();
  if (!a.log) return;
  for (int e = tid; e < MC_LPB * MC_ROW; e += blockDim.x) {
    const int l = e / MC_ROW, j = e - l * MC_ROW, t = st[l];
    if (t >= 0) a.logbuf[((int64_t)t * a.B + b0 + l) * MC_ROW + j] = sv[l][j];  // t < max_steps, b0 + l < B
  }
}

// (re)start the logs of landings [first, first + count): no appends, states[0] = x0
__global__ void k_fleet_mc_reset(int first, int count, const double *__restrict__ x0, int *cnt, double *mprev,
                                 double *x0log) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int b = first + i;
  cnt[b] = 0;
  mprev[b] = x0[(int64_t)i * NX];
  for (int c = 0; c < NX; ++c) x0log[(int64_t)b * NX + c] = x0[(int64_t)i * NX + c];
}

// attach to a fleet in flight: every landing's log starts at its current step and state
__global__ void k_fleet_mc_init(int B, const double *__restrict__ rec, const double *__restrict__ x, int *cnt,
                                double *mprev, double *x0log) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  cnt[b] = (int)rec[(int64_t)b * GPMPC_REC_LEN + 1];
  mprev[b] = x[(int64_t)b * NX];
  for (int c = 0; c < NX; ++c) x0log[(int64_t)b * NX + c] = x[(int64_t)b * NX + c];
}

static void fleet_mc_release(gpmpc_fleet *f) {
  f->mc = false;
  f->mc_thrust = f->mc_aero = 0.0;
  f->mc_log_steps = 0;
  f->mc_noise.release(); f->mc_u0.release(); f->mc_cnt.release(); f->mc_mprev.release();
  f->mc_x0.release(); f->mc_logbuf.release();
}

extern "C" int gpmpc_fleet_mc_detach(gpmpc_fleet *f) {
  GPMPC_CHECK_ARG(f);
  if (!f->mc) return 0;
  GPMPC_HIP(hipStreamSynchronize(f->ctx->stream));
  fleet_mc_release(f);
  return 0;
}

extern "C" int gpmpc_fleet_mc_attach(gpmpc_fleet *f, const gpmpc_fleet_mc_config *mc, const double *noise) {
  GPMPC_CHECK_ARG(f && mc);
  const int ms = f->cfg.max_steps;
  if (!(mc->thrust_dispersion >= 0.0) || !(mc->aero_dispersion >= 0.0) || !std::isfinite(mc->thrust_dispersion) ||
      !std::isfinite(mc->aero_dispersion)) {
    gpmpc_set_error("fleet_mc_attach: the dispersions must be finite and >= 0");
    return -2;
  }
  if (mc->log_steps != 0 && mc->log_steps != ms) {
    gpmpc_set_error("fleet_mc_attach: log_steps must be 0 or the fleet's max_steps (%d), got %d", ms, mc->log_steps);
    return -2;
  }
  const bool disp = mc->thrust_dispersion > 0.0 || mc->aero_dispersion > 0.0;
  if (disp && !noise) {
    gpmpc_set_error("fleet_mc_attach: a dispersion > 0 needs the noise table (batch x max_steps x 4)");
    return -2;
  }
  if (ms < 1) {
    gpmpc_set_error("fleet_mc_attach: the fleet's max_steps must be >= 1");
    return -2;
  }
  GPMPC_HIP(hipSetDevice(f->ctx->device));
  hipStream_t s = f->ctx->stream;
  GPMPC_HIP(hipStreamSynchronize(s));
  fleet_mc_release(f);
  const size_t B = (size_t)f->B;
  const size_t nlog = mc->log_steps ? (size_t)ms * B * MC_ROW : 0, nnoise = disp ? B * (size_t)ms * 4 : 0;
  if (f->mc_u0.alloc(s, sizeof(double) * B * NU) || f->mc_cnt.alloc(s, sizeof(int) * B) ||
      f->mc_mprev.alloc(s, sizeof(double) * B) || f->mc_x0.alloc(s, sizeof(double) * B * NX) ||
      f->mc_logbuf.alloc(s, sizeof(double) * nlog) || f->mc_noise.alloc(s, sizeof(double) * nnoise)) {
    fleet_mc_release(f);
    gpmpc_set_error("fleet_mc_attach: out of device memory");
    return -1;
  }
  GPMPC_HIP(hipMemsetAsync(f->mc_u0.p, 0, sizeof(double) * B * NU, s));
  if (nlog) GPMPC_HIP(hipMemsetAsync(f->mc_logbuf.p, 0xff, sizeof(double) * nlog, s));  // all ones: NaN
  if (nnoise) GPMPC_HIP(hipMemcpyAsync(f->mc_noise.p, noise, sizeof(double) * nnoise, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_fleet_mc_init, dim3((f->B + 255) / 256), dim3(256), 0, s, f->B, f->rec.as<double>(),
                     f->x.as<double>(), f->mc_cnt.as<int>(), f->mc_mprev.as<double>(), f->mc_x0.as<double>());
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(hipStreamSynchronize(s));  // the pageable noise table is the caller's again
  f->mc_thrust = mc->thrust_dispersion;
  f->mc_aero = mc->aero_dispersion;
  f->mc_log_steps = mc->log_steps;
  f->mc = true;
  return 0;
}

extern "C" int gpmpc_fleet_mc_read_log(gpmpc_fleet *f, int first, int count, double *states, double *controls,
                                       int *nsteps) {
  GPMPC_CHECK_ARG(f && first >= 0 && count >= 0 && first + count <= f->B);
  if (!f->mc || !f->mc_log_steps) {
    gpmpc_set_error("fleet_mc_read_log: no trajectory log is attached (gpmpc_fleet_mc_attach with log_steps)");
    return -2;
  }
  if (count == 0) return 0;
  GPMPC_HIP(hipSetDevice(f->ctx->device));
  hipStream_t s = f->ctx->stream;
  const size_t C = (size_t)count, ms = (size_t)f->cfg.max_steps;
  std::vector<int> cnt(C);
  std::vector<double> x0(C * NX);
  GPMPC_HIP(hipMemcpyAsync(cnt.data(), f->mc_cnt.as<int>() + first, sizeof(int) * C, hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipMemcpyAsync(x0.data(), f->mc_x0.as<double>() + (size_t)first * NX, sizeof(double) * C * NX,
                           hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  size_t tmax = 0;
  for (size_t i = 0; i < C; ++i) {
    cnt[i] = std::min(std::max(cnt[i], 0), (int)ms);
    tmax = std::max(tmax, (size_t)cnt[i]);
  }
  std::vector<double> rows(tmax * C * MC_ROW);  // [t][i][10]: the landings' columns of the first tmax steps
  if (tmax) {
    GPMPC_HIP(hipMemcpy2DAsync(rows.data(), sizeof(double) * C * MC_ROW,
                               f->mc_logbuf.as<double>() + (size_t)first * MC_ROW, sizeof(double) * f->B * MC_ROW,
                               sizeof(double) * C * MC_ROW, tmax, hipMemcpyDeviceToHost, s));
    GPMPC_HIP(hipStreamSynchronize(s));
  }
  for (size_t i = 0; i < C; ++i) {
    if (nsteps) nsteps[i] = cnt[i];
    if (states) {
      double *S = states + i * (ms + 1) * NX;
      for (int c = 0; c < NX; ++c) S[c] = x0[i * NX + c];
      for (size_t t = 0; t < ms; ++t)
        for (int c = 0; c < NX; ++c)
          S[(t + 1) * NX + c] = t < (size_t)cnt[i] ? rows[(t * C + i) * MC_ROW + c] : NAN;
    }
    if (controls) {
      double *U = controls + i * ms * NU;
      for (size_t t = 0; t < ms; ++t)
        for (int c = 0; c < NU; ++c) U[t * NU + c] = t < (size_t)cnt[i] ? rows[(t * C + i) * MC_ROW + NX + c] : NAN;
    }
  }
  return 0;
}

static int fleet_create(gpmpc_ctx *ctx, gpmpc_gp *gp, gpmpc_fitc *fitc, const gpmpc_fleet_config *cfg,
                        int batch, int fleet_batch, gpmpc_fleet **out) {
  GPMPC_CHECK_ARG(ctx && (gp || fitc) && cfg && out && batch > 0 && fleet_batch >= batch);
  const GpView g = fitc ? fitc_view(fitc) : gp_view(gp);
  GPMPC_CHECK_ARG(g.d == NFEAT && g.n_out == 3);
  if (g.kind < GPMPC_SE_ARD || g.kind > GPMPC_MATERN52) {
    gpmpc_set_error("fleet: the GP must use one of the four stationary kernels (not a composite program)");
    return -2;
  }
  // the fleet runs MonteCarloSimulator's solve protocol (monte_carlo.py:495-512)
  // with the GPMPC adapter; FastRTI3DoF's step protocol (unshifted linearisation,
  // D2 sign, fallback to the shifted plan) is the host mirror mpc/osqp_rti.py
  if (cfg->target_mode != 1) {
    gpmpc_set_error("fleet: target_mode must be 1 (solve protocol); the step protocol of "
                    "FastRTI3DoF runs on the host mirror");
    return -2;
  }
  {
    // sqp_qp.max_iter = 0 means "use qp".  sqp_qp left at the defaults (a caller that
    // edits only qp) or equal to qp is that; any other field edited alongside max_iter 0
    // would be silently ignored, so such a config is refused
    auto same = [](const gpmpc_qp_settings &a, const gpmpc_qp_settings &b) {
      return a.rho == b.rho && a.sigma == b.sigma && a.alpha == b.alpha && a.eps_abs == b.eps_abs &&
             a.eps_rel == b.eps_rel && a.eps_prim_inf == b.eps_prim_inf && a.eps_dual_inf == b.eps_dual_inf &&
             a.check_termination == b.check_termination && a.adaptive_rho == b.adaptive_rho &&
             a.adaptive_rho_interval == b.adaptive_rho_interval &&
             a.adaptive_rho_tolerance == b.adaptive_rho_tolerance && a.scaling == b.scaling &&
             a.warm_start == b.warm_start;
    };
    gpmpc_qp_settings def;
    gpmpc_qp_default_settings(&def);
    if (cfg->sqp_iters > 1 && cfg->sqp_qp.max_iter == 0 && !same(cfg->sqp_qp, cfg->qp) &&
        !same(cfg->sqp_qp, def)) {
      gpmpc_set_error("fleet: sqp_qp was edited but sqp_qp.max_iter is 0 (= use qp); set "
                      "sqp_qp.max_iter to use the SQP passes' own settings");
      return -2;
    }
  }
  const int N = cfg->horizon;
  const int n = (N + 1) * NX + N * NU, m = NX * (N + 1) + n;
  GPMPC_CHECK_ARG(N >= 1 && n <= QP_NMAX && m <= QP_MMAX && NX + N * DYN_NNZ + n <= QP_NNZMAX);
  GPMPC_HIP(hipSetDevice(ctx->device));
  auto *f = new gpmpc_fleet();
  f->ctx = ctx; f->gp = gp; f->fitc = fitc; f->cfg = *cfg; f->B = batch; f->N = N; f->n = n; f->m = m;
  f->gp_n = g.n;
  f->n_active = batch;
  std::vector<int> rp, ci;
  mpc_pattern(N, rp, ci);
  if (f->pat.build(n, m, rp.data(), ci.data(), ctx->stream) || !f->pat.fits()) {
    delete f;
    gpmpc_set_error("fleet: QP pattern setup failed");
    return -1;
  }
  const size_t B = batch, P = (size_t)batch * N;
  f->plan_B = fleet_batch;
  f->post_kind = gemm_sumsq_kind(g.n + 3, (int)std::min<int64_t>((int64_t)fleet_batch * N, 1 << 30), g.n);
  f->post_few = (int64_t)fleet_batch * N <= 64 && g.d == NFEAT;
  // partial rows of any posterior path: W rows + the 3 alpha^T rows in 64-row tiles (the
  // most rows any kernel writes), at least the column-stationary posterior's two halves
  const int nrt = std::max(gemm_sumsq_rows(GEMM_SUMSQ_64, g.n + 3), POST_CS_PARTS);
  if (fitc) {
    f->post_kind2 = gemm_sumsq_kind(g.n, (int)std::min<int64_t>((int64_t)fleet_batch * N, 1 << 30), g.n);
    f->post_nrt2 = gemm_sumsq_rows(f->post_kind2, g.n);
    if (f->part2.alloc(sizeof(double) * gemm_sumsq_rows(GEMM_SUMSQ_64, g.n) * P)) {
      delete f;
      gpmpc_set_error("fleet: out of device memory");
      return -1;
    }
  }
  if (f->x.alloc(sizeof(double) * B * NX) || f->Xw.alloc(sizeof(double) * B * (N + 1) * NX) ||
      f->Uw.alloc(sizeof(double) * B * N * NU) || f->ysc.alloc(sizeof(double) * B * m) ||
      f->rho.alloc(sizeof(double) * B) || f->rec.alloc(sizeof(double) * B * GPMPC_REC_LEN) ||
      f->xt.alloc(sizeof(double) * B * NX) || f->Q.alloc(sizeof(double) * P * NFEAT) ||
      f->Qn.alloc(sizeof(double) * P) || f->Ks.alloc(sizeof(double) * P * g.n) ||
      f->part.alloc(sizeof(double) * nrt * P) || f->meanT.alloc(sizeof(double) * 3 * P) ||
      f->mean.alloc(sizeof(double) * P * 3) || f->var.alloc(sizeof(double) * P * 3) ||
      f->order.alloc(sizeof(int) * B) || f->lastit.alloc(sizeof(int) * B) ||
      f->claims.alloc(sizeof(unsigned) * 4096) || f->sqp_done.alloc(sizeof(int) * B)) {
    delete f;
    gpmpc_set_error("fleet: out of device memory");
    return -1;
  }
  // every landing starts terminated until reset
  std::vector<double> r(B * GPMPC_REC_LEN, 0.0);
  for (size_t b = 0; b < B; ++b) r[b * GPMPC_REC_LEN] = -1.0;
  hipMemcpyAsync(f->rec.p, r.data(), sizeof(double) * r.size(), hipMemcpyHostToDevice, ctx->stream);
  hipMemsetAsync(f->lastit.p, 0, sizeof(int) * B, ctx->stream);
  hipMemsetAsync(f->claims.p, 0, sizeof(unsigned) * 4096, ctx->stream);
  hipMemsetAsync(f->sqp_done.p, 0, sizeof(int) * B, ctx->stream);
  {  // identity dispatch order until the first order kernel (every slot maps in range)
    std::vector<int> id(B);
    for (size_t b = 0; b < B; ++b) id[b] = (int)b;
    hipMemcpyAsync(f->order.p, id.data(), sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream);
    GPMPC_HIP(hipStreamSynchronize(ctx->stream));
  }
  // the fleet's switches, read at creation
  f->use_order = gpmpc_env_int("GPMPC_FLEET_ORDER", 1) != 0;
  f->alt_wave = gpmpc_env_int("GPMPC_FLEET_ALTWAVE", 0) != 0;
  f->simd_pick = gpmpc_env_int("GPMPC_FLEET_SIMD", 1) != 0;
  f->fuse_post = gpmpc_env_int("GPMPC_FLEET_FUSE_POST", 1) != 0;
  // the specialised solver assumes the N = 20 stage layout of its LDS caps
  f->use_fq = gpmpc_env_int("GPMPC_FLEET_SOLVER", 1) != 0 && N == 20 && f->pat.mode == 1 && f->pat.nblk == FQ_NBLK &&
              m - n == FQ_MD && f->pat.nnz - n == FQ_NNZD;
  // small fleets (at most one landing per CU) take the 256-thread, one-wave-per-SIMD build of
  // the control kernel: twice the threads for the parallel ADMM phases and no register
  // spills (single landing 216 -> 192 us per step); decided by the fleet size, not by the
  // running count, so a fleet's landings always see the same arithmetic (GPMPC_FLEET_WIDE
  // = 0 / 1 forces it)
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
  const int we = gpmpc_env_int("GPMPC_FLEET_WIDE", INT_MIN);  // (unset: by the fleet size)
  f->wide = f->use_fq && (we != INT_MIN ? we != 0 : fleet_batch <= cus);
  GPMPC_HIP(hipStreamSynchronize(ctx->stream));
  *out = f;
  return 0;
}

extern "C" int gpmpc_fleet_create_shard(gpmpc_ctx *ctx, gpmpc_gp *gp, const gpmpc_fleet_config *cfg,
                                        int batch, int fleet_batch, gpmpc_fleet **out) {
  GPMPC_CHECK_ARG(gp);
  return fleet_create(ctx, gp, nullptr, cfg, batch, fleet_batch, out);
}

extern "C" int gpmpc_fleet_create(gpmpc_ctx *ctx, gpmpc_gp *gp, const gpmpc_fleet_config *cfg, int batch,
                                  gpmpc_fleet **out) {
  return gpmpc_fleet_create_shard(ctx, gp, cfg, batch, batch, out);
}

extern "C" int gpmpc_fleet_create_fitc(gpmpc_ctx *ctx, gpmpc_fitc *gp, const gpmpc_fleet_config *cfg, int batch,
                                       int fleet_batch, gpmpc_fleet **out) {
  GPMPC_CHECK_ARG(gp);
  return fleet_create(ctx, nullptr, gp, cfg, batch, fleet_batch, out);
}

extern "C" int gpmpc_fleet_reset(gpmpc_fleet *f, int first, int count, const double *x0) {
  GPMPC_CHECK_ARG(f && x0 && first >= 0 && count >= 0 && first + count <= f->B);
  if (count == 0) return 0;
  hipStream_t s = f->ctx->stream;
  DevBuf d;
  GPMPC_HIP(d.alloc(sizeof(double) * count * NX));
  GPMPC_HIP(hipMemcpyAsync(d.p, x0, sizeof(double) * count * NX, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_fleet_reset, dim3(count), dim3(256), 0, s, first, count, f->N,
                     f->cfg.target_mode, d.as<double>(), f->x.as<double>(), f->Xw.as<double>(),
                     f->Uw.as<double>(), f->ysc.as<double>(), f->m, f->rho.as<double>(),
                     f->cfg.qp.rho, f->rec.as<double>(), f->xt.as<double>());
  GPMPC_HIP(hipGetLastError());
  if (f->mc) {  // restart those landings' logs: count 0, states[0] = x0
    hipLaunchKernelGGL(k_fleet_mc_reset, dim3((count + 255) / 256), dim3(256), 0, s, first, count, d.as<double>(),
                       f->mc_cnt.as<int>(), f->mc_mprev.as<double>(), f->mc_x0.as<double>());
    GPMPC_HIP(hipGetLastError());
  }
  GPMPC_HIP(hipStreamSynchronize(s));
  f->n_active = f->B;  // conservative until the host reads the records
  return 0;
}

// GP posterior of every landing's horizon, in three timed sub-phases:
//   bit 0: features + K* gram;  bit 2: one MFMA pass over K* with [W; alpha^T]:
//   variance partial sums (SUMSQ epilogue) and the means;  bit 3: finish
static hipError_t fleet_gp_posterior(gpmpc_fleet *f, int mask) {
  hipStream_t s = f->ctx->stream;
  const GpView g = fleet_view(f);
  const int nb = f->use_order ? f->n_active : f->B;  // slots 0 .. nb-1 (running first)
  const int P = nb * f->N;
  if (P == 0) return hipSuccess;
  // GPMPC_POST_FUSED=1: K* formed inside the posterior GEMM (no K* in HBM).
  // Measured slower (0.60 ms vs 0.062 ms gram + 0.415 ms GEMM at 1024 x 20):
  // each of the 8 row tiles regenerates its K* columns (4.6x the exps of the
  // gram kernel) and the exp/scalar-load stream does not hide under the FP64
  // MFMAs at 2 waves per SIMD.  Off by default.
  static const int fused_env = gpmpc_env_int("GPMPC_POST_FUSED", 0);
  // GPMPC_POST_CS=1: the column-stationary posterior (post.hip), K* formed once per
  // workgroup inside the MFMA pass, never in HBM; two partial rows
  const bool cs = !f->fitc && g.Wf && post_cs_env();
  const bool fused = !f->fitc && !cs && fused_env && g.d >= 11 && g.d <= 13;
  const int nrt = cs ? POST_CS_PARTS : fused ? (g.n + 3 + 127) / 128 : gemm_sumsq_rows(f->post_kind, g.n + 3);
  hipError_t e = hipSuccess;
  if ((mask & 1) && !fused && !cs && f->post_few) {
    hipLaunchKernelGGL(k_fleet_queries_gram, dim3((g.n + 63) / 64), dim3(256), 0, s, nb, f->N, f->Xw.as<double>(),
                       f->Uw.as<double>(), g.ls, g.kind == GPMPC_SE_ISO, f->use_order ? f->order.as<int>() : nullptr,
                       g.kind, g.Xs, g.Xn, g.n, g.sigma2, g.iso_scale, f->Ks.as<double>());
    if ((e = hipGetLastError()) != hipSuccess) return e;
  } else if (mask & 1) {
    // GPMPC_GRAM_FEAT=0: the query rows from a launch of their own (k_fleet_queries -> Q).
    // Default: the row-tiled Gram kernel forms its 128 rows itself (same function, same
    // bits), one launch and the Q round trip less; Q is then not written.
    static const int feat_env = gpmpc_env_int("GPMPC_GRAM_FEAT", 1);
    const FleetPlans pl{f->Xw.as<double>(), f->Uw.as<double>(), g.ls, f->use_order ? f->order.as<int>() : nullptr,
                        f->N, g.kind == GPMPC_SE_ISO};
    const bool in_gram = feat_env && !fused && !cs && g.d == NFEAT && gram_rows_tiled(P, g.d);
    if (!in_gram) {
      hipLaunchKernelGGL(k_fleet_queries, dim3((P + 255) / 256), dim3(256), 0, s, nb, f->N, pl.Xw, pl.Uw, pl.ls,
                         pl.iso, pl.order, f->Q.as<double>(), f->Qn.as<double>());
      ++f->query_launches;
    }
    if (!fused && !cs) {
      e = launch_gram(s, g.kind, f->Q.as<double>(), f->Qn.as<double>(), P, g.Xs, g.Xn, g.n, g.d,
                      g.sigma2, g.iso_scale, f->Ks.as<double>(), g.n, 0, in_gram ? &pl : nullptr);
      if (e != hipSuccess) return e;
    }
  }
  if (mask & 4) {
    if (cs)
      e = launch_post_cs(s, g.n, 3, P, g.Wf, g.Xp, f->Q.as<double>(), f->Qn.as<double>(), g.d, g.kind, g.sigma2,
                         g.iso_scale, f->part.as<double>(), P, f->meanT.as<double>(), P);
    else if (fused)
      e = launch_gemm_post_fused(s, g.n, 3, P, g.W, f->Q.as<double>(), f->Qn.as<double>(), g.Xs,
                                 g.Xn, g.d, g.kind, g.sigma2, g.iso_scale, f->part.as<double>(), P,
                                 f->meanT.as<double>(), P);
    else
      e = launch_gemm_sumsq_mean(s, g.n, 3, P, g.W, f->Ks.as<double>(), f->part.as<double>(), P,
                                 f->meanT.as<double>(), P, f->post_kind);
    if (e != hipSuccess) return e;
    if (f->fitc) {  // |w|^2 = |L_B^-1 L_uu^-1 k*|^2 (sparse_gp.py:293-299)
      e = launch_gemm_sumsq(s, g.n, P, fitc_W2(f->fitc), f->Ks.as<double>(), f->part2.as<double>(), P,
                            f->post_kind2);
      if (e != hipSuccess) return e;
    }
  }
  if (mask & 4) {
    f->post_P = P;
    f->post_nrt = nrt;
  }
  // fused: k_fleet_control2 finishes each landing's own queries as it assembles
  if ((mask & 8) && !(f->use_fq && f->fuse_post)) {
    if (f->fitc)
      e = launch_fitc_finish(s, P, 3, nrt, f->post_nrt2, f->part.as<double>(), f->part2.as<double>(), P,
                             f->meanT.as<double>(), P, g.ymean, g.ystd, g.sigma2, f->mean.as<double>(),
                             f->var.as<double>());
    else
      e = launch_post_finish(s, P, 3, nrt, f->part.as<double>(), P, f->meanT.as<double>(), P,
                             g.ymean, g.ystd, g.sigma2, f->mean.as<double>(), f->var.as<double>());
  }
  return e;
}

// Dispatch order for the control kernel.  Workgroups start in blockIdx order
// and a landing's solve costs ~proportional to its ADMM iterations (25 or 50
// here: 237 vs 490 us), so launching the landings whose last solve was
// longest first is the LPT schedule over the 512 resident slots (measured
// span 916 us vs 826 us LPT-ideal).  Terminated landings (they return at once)
// go last.  Counting sort in one workgroup; the order inside a bucket is
// arbitrary, which cannot change results: landings are independent.
#define ORDER_BUCKETS 256
__global__ __launch_bounds__(1024) void k_fleet_order(int B, const double *__restrict__ rec,
                                                      const int *__restrict__ lastit,
                                                      int *__restrict__ order) {
  __shared__ int cnt[ORDER_BUCKETS];
  for (int i = threadIdx.x; i < ORDER_BUCKETS; i += blockDim.x) cnt[i] = 0;
  __syncthreads();
  auto key = [&](int b) {  // larger = earlier; 0 = terminated
    if (rec[(int64_t)b * GPMPC_REC_LEN] != 0.0) return 0;
    return min(lastit[b], ORDER_BUCKETS - 2) + 1;
  };
  // Wave-aggregated LDS atomics: nearly every landing sits in one of two or
  // three buckets (25 / 50 iterations, terminated), and per-lane atomics on one
  // LDS word serialise.  Each wave adds once per distinct key it holds; lanes
  // take base + their rank among the wave's lanes with that key.
  const int lane = threadIdx.x & 63;
  auto wave_add = [&](int k, bool active) {
    int slot = 0;
    unsigned long long todo = __ballot(active);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int lk = __shfl(k, leader);
      const unsigned long long same = __ballot(active && k == lk);
      int base = 0;
      if (lane == leader) base = atomicAdd(&cnt[lk], __popcll(same));
      base = __shfl(base, leader);
      if (active && k == lk) slot = base + __popcll(same & ((1ull << lane) - 1));
      todo &= ~same;
    }
    return slot;
  };
  for (int b0 = 0; b0 < B; b0 += blockDim.x) {
    const int b = b0 + threadIdx.x;
    wave_add(b < B ? key(b) : 0, b < B);
  }
  __syncthreads();
  // descending exclusive scan over the buckets, 256 threads (4 waves, shuffles)
  static_assert(ORDER_BUCKETS == 256, "scan is laid out for 256 buckets");
  __shared__ int wsum[4];
  int c = 0, inc = 0;
  if (threadIdx.x < ORDER_BUCKETS) {
    c = cnt[ORDER_BUCKETS - 1 - threadIdx.x];
    inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[threadIdx.x >> 6] = inc;
  }
  __syncthreads();
  if (threadIdx.x < ORDER_BUCKETS) {
    int pre = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += wsum[w];
    cnt[ORDER_BUCKETS - 1 - threadIdx.x] = pre + inc - c;
  }
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += blockDim.x) {
    const int b = b0 + threadIdx.x;
    const int slot = wave_add(b < B ? key(b) : 0, b < B);
    if (b < B) order[slot] = b;
  }
}

static FleetArgs fleet_args(gpmpc_fleet *f) {
  FleetArgs a;
  a.pt = f->pat.dev;
  a.st = to_dev(f->cfg.sqp_iters > 1 && f->cfg.sqp_qp.max_iter > 0 ? f->cfg.sqp_qp : f->cfg.qp);
  a.N = f->N;
  a.target_mode = f->cfg.target_mode;
  a.use_gp = f->cfg.use_gp;
  a.residual_model = f->cfg.residual_model;
  a.max_steps = f->cfg.max_steps;
  a.dt = f->cfg.dt;
  a.x = f->x.as<double>(); a.Xw = f->Xw.as<double>(); a.Uw = f->Uw.as<double>();
  a.ysc = f->ysc.as<double>(); a.rho = f->rho.as<double>(); a.rec = f->rec.as<double>();
  a.xt = f->xt.as<double>();
  a.gmean = f->mean.as<double>();
  a.gp_by_slot = f->use_order && f->cfg.use_gp;
  a.order = f->use_order ? f->order.as<int>() : nullptr;
  a.alt_wave = f->alt_wave;
  a.claims = f->simd_pick ? f->claims.as<unsigned>() : nullptr;
  a.part = nullptr;
  a.part2 = nullptr;
  a.nrt2 = 0;
  if (f->use_fq && f->fuse_post && f->cfg.use_gp && f->post_P > 0) {
    const GpView g = fleet_view(f);
    if (f->fitc) {
      a.part2 = f->part2.as<double>();
      a.nrt2 = f->post_nrt2;
    }
    a.part = f->part.as<double>();
    a.meanT = f->meanT.as<double>();
    a.ymean = g.ymean;
    a.ystd = g.ystd;
    a.mean_out = f->mean.as<double>();
    a.var_out = f->var.as<double>();
    a.sigma2 = g.sigma2;
    a.nrt = f->post_nrt;
    a.pld = f->post_P;
  }
  f->epoch = (f->epoch + 1) & 0xffffff;
  if (f->epoch == 0) f->epoch = 1;
  a.epoch = f->epoch;
  a.lastit = f->lastit.as<int>();
  a.stamps = f->stamps;
  a.trace = f->trace;
  a.sqp = f->cfg.sqp_iters > 1;
  a.sqp_first = f->sqp_it == 0;
  a.sqp_last = f->sqp_it >= f->cfg.sqp_iters - 1;
  a.sqp_tol = f->cfg.sqp_tol;
  a.sqp_done = f->sqp_done.as<int>();
  a.u0_out = f->mc ? f->mc_u0.as<double>() : nullptr;
  return a;
}

extern "C" int gpmpc_fleet_step_phases(gpmpc_fleet *f, int phase_mask) {
  GPMPC_CHECK_ARG(f);
  if (fleet_view(f).n != f->gp_n) {  // gpmpc_gp_append grew the GP under the fleet
    gpmpc_set_error("fleet: the GP has %d training rows, the fleet was built for %d; recreate it",
                    fleet_view(f).n, f->gp_n);
    return -2;
  }
  GPMPC_HIP(hipSetDevice(f->ctx->device));
  if (f->cfg.sqp_iters > 1 && f->sqp_it == 0 && (phase_mask & 3))
    hipLaunchKernelGGL(k_fleet_x0_to_plan, dim3((f->B * NX + 255) / 256), dim3(256), 0, f->ctx->stream, f->B,
                       f->cfg.horizon, f->x.as<double>(), f->rec.as<double>(), f->Xw.as<double>());
  // the dispatch order of this step, before the GP phase when there is one:
  // the posterior rows then follow the same slots as the control workgroups
  // (one landing: the identity order set at creation is the only one)
  const bool order_now = f->use_order && f->sqp_it == 0 && f->B > 1 &&
                         ((f->cfg.use_gp && (phase_mask & 1)) || (!f->cfg.use_gp && (phase_mask & 2)));
  if (order_now)
    hipLaunchKernelGGL(k_fleet_order, dim3(1), dim3(1024), 0, f->ctx->stream, f->B,
                       f->rec.as<double>(), f->lastit.as<int>(), f->order.as<int>());
  if ((phase_mask & 13) && f->cfg.use_gp) GPMPC_HIP(fleet_gp_posterior(f, phase_mask));
  if (phase_mask & 2) {
    const int nb = f->use_order ? f->n_active : f->B;
    if (nb > 0) {
      if (f->use_fq) {
        GPMPC_HIP((f->wide ? fq_wide::launch_control : fq_narrow::launch_control)(f->ctx->stream, nb, fleet_args(f),
                                                                                  f->stamps != nullptr));
      } else {
        hipLaunchKernelGGL(k_fleet_control, dim3(nb), dim3(256), 0, f->ctx->stream, fleet_args(f));
      }
    }
    GPMPC_HIP(hipGetLastError());
    // the attached Monte-Carlo protocol, once per control step: after the last SQP pass
    if (f->mc && f->sqp_it >= (f->cfg.sqp_iters > 1 ? f->cfg.sqp_iters : 1) - 1) {
      FleetMcArgs m;
      m.B = f->B; m.max_steps = f->cfg.max_steps; m.log = f->mc_log_steps != 0;
      m.dt = f->cfg.dt; m.thrust = f->mc_thrust; m.aero = f->mc_aero;
      m.noise = f->mc_noise.as<double>(); m.u0 = f->mc_u0.as<double>();
      m.x = f->x.as<double>(); m.rec = f->rec.as<double>(); m.mprev = f->mc_mprev.as<double>();
      m.logbuf = f->mc_logbuf.as<double>(); m.cnt = f->mc_cnt.as<int>();
      hipLaunchKernelGGL(k_fleet_mc, dim3((f->B + MC_LPB - 1) / MC_LPB), dim3(256), 0, f->ctx->stream, m);
      GPMPC_HIP(hipGetLastError());
    }
  }
  return 0;
}

extern "C" int gpmpc_fleet_step(gpmpc_fleet *f, int nsteps) {
  GPMPC_CHECK_ARG(f && nsteps >= 0);
  const int passes = f->cfg.sqp_iters > 1 ? f->cfg.sqp_iters : 1;
  for (int it = 0; it < nsteps; ++it) {
    // SQP mode: every pass re-linearises around the last QP solution (GP
    // posterior at the new horizon points, QP); landings that converged skip
    // the later passes' control launches
    for (int p = 0; p < passes; ++p) {
      f->sqp_it = p;
      const int rc = gpmpc_fleet_step_phases(f, 15);
      if (rc) { f->sqp_it = 0; return rc; }
    }
    f->sqp_it = 0;
  }
  return 0;
}

extern "C" int gpmpc_fleet_read(gpmpc_fleet *f, double *records, double *x) {
  GPMPC_CHECK_ARG(f);
  hipStream_t s = f->ctx->stream;
  if (records)
    GPMPC_HIP(hipMemcpyAsync(records, f->rec.p, sizeof(double) * f->B * GPMPC_REC_LEN,
                             hipMemcpyDeviceToHost, s));
  if (x) GPMPC_HIP(hipMemcpyAsync(x, f->x.p, sizeof(double) * f->B * NX, hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  if (records) {
    int run = 0;
    for (int b = 0; b < f->B; ++b) run += records[(size_t)b * GPMPC_REC_LEN] == 0.0;
    f->n_active = run;
  }
  return 0;
}

extern "C" int gpmpc_fleet_get_state(gpmpc_fleet *f, double *Xw, double *Uw, double *y_scaled,
                                     double *rho) {
  GPMPC_CHECK_ARG(f);
  hipStream_t s = f->ctx->stream;
  const size_t B = (size_t)f->B, N = (size_t)f->N;
  if (Xw) GPMPC_HIP(hipMemcpyAsync(Xw, f->Xw.p, sizeof(double) * B * (N + 1) * NX, hipMemcpyDeviceToHost, s));
  if (Uw) GPMPC_HIP(hipMemcpyAsync(Uw, f->Uw.p, sizeof(double) * B * N * NU, hipMemcpyDeviceToHost, s));
  if (y_scaled)
    GPMPC_HIP(hipMemcpyAsync(y_scaled, f->ysc.p, sizeof(double) * B * f->m, hipMemcpyDeviceToHost, s));
  if (rho) GPMPC_HIP(hipMemcpyAsync(rho, f->rho.p, sizeof(double) * B, hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  return 0;
}

// The GP posterior of the last control step at every landing's N horizon points, per
// landing (B x N x 3 each, row-major): the mean and variance the step's QP assembly
// consumed (the variance is computed beside it, exact_gp.py:256-266, and not read by
// the QP).  The device rows follow the dispatch slots of that step; they are put back
// in landing order here.  Every slot of the step's launched prefix is finished (the
// control kernel finishes the slots of landings that return before their QP too), so a
// landing in it reads the posterior at its own trajectory; landings past it read NaN.
extern "C" int gpmpc_fleet_get_posterior(gpmpc_fleet *f, double *mean, double *var) {
  GPMPC_CHECK_ARG(f && (mean || var));
  if (!f->cfg.use_gp) {
    gpmpc_set_error("fleet: use_gp = 0, the fleet runs no GP posterior");
    return -2;
  }
  hipStream_t s = f->ctx->stream;
  GPMPC_HIP(hipSetDevice(f->ctx->device));
  const size_t B = (size_t)f->B, N = (size_t)f->N, P = B * N;
  std::vector<double> dm(P * 3), dv(P * 3), rec(B * GPMPC_REC_LEN);
  std::vector<int> ord(B);
  GPMPC_HIP(hipMemcpyAsync(dm.data(), f->mean.p, sizeof(double) * P * 3, hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipMemcpyAsync(dv.data(), f->var.p, sizeof(double) * P * 3, hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipMemcpyAsync(ord.data(), f->order.p, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  const bool by_slot = f->use_order;  // gp_by_slot of fleet_args (use_gp holds here)
  const size_t nslots = by_slot ? (size_t)f->post_P / N : B;
  std::vector<char> ran(B, 0);
  for (size_t sl = 0; sl < nslots && sl < B; ++sl) {
    const int b = by_slot ? ord[sl] : (int)sl;
    if (b < 0 || (size_t)b >= B) continue;
    ran[b] = 1;
    for (size_t e = 0; e < N * 3; ++e) {
      if (mean) mean[(size_t)b * N * 3 + e] = dm[sl * N * 3 + e];
      if (var) var[(size_t)b * N * 3 + e] = dv[sl * N * 3 + e];
    }
  }
  for (size_t b = 0; b < B; ++b)
    if (!ran[b])
      for (size_t e = 0; e < N * 3; ++e) {
        if (mean) mean[b * N * 3 + e] = NAN;
        if (var) var[b * N * 3 + e] = NAN;
      }
  return 0;
}

extern "C" int gpmpc_fleet_query_launches(gpmpc_fleet *f) { return f ? f->query_launches : -1; }

extern "C" double *gpmpc_fleet_records_dev(gpmpc_fleet *f) { return f ? f->rec.as<double>() : nullptr; }

extern "C" int gpmpc_fleet_destroy(gpmpc_fleet *f) {
  if (f && f->ctx) (void)hipStreamSynchronize(f->ctx->stream);
  if (f) fleet_mc_release(f);  // the attachment's pooled buffers go back to the context's pool
  delete f;
  return 0;
}
