// hull.hip -- batched projection of a query onto the convex hull of K <= 64 vertices in d <= 32
// dimensions in fp64: the terminal constraint x_N in Conv{v_1 .. v_K} of learning MPC
// (terminal/convex_hull.py), DESIGN §19.
//
// Reference: ConvexHullConstraint.project_onto_hull / check_feasibility / get_interpolated_q
// (convex_hull.py:125-237): the reference solves min |x - V' l|^2, sum l = 1, l >= 0 with IPOPT.
// Here it is Wolfe's minimum-norm-point method on w_i = v_i - x: an active set (the corral) of
// affinely independent vertices; a major cycle takes the vertex that minimises p . w_i (p = sum
// l_i w_i) into the corral unless |p|^2 - min_i p . w_i <= tol max_i |w_i|^2; a minor cycle
// moves to the minimum-norm point of the corral's affine hull, or up to the boundary towards it
// and drops the vertex that reaches zero.
//
// Kernel shape.  One wave a query, lane i owns vertex i with w_i in registers (d padded with
// zeros to 4, 8, 16 or 32).  p is kept by every lane (summed over the corral by v_readlane
// broadcasts), so p . w_i is lane-local and the argmin one wave reduction, ties to the lower
// lane: a duplicate of a corral vertex never enters.  The corral's system (s e e' + Q Q') u = e
// (s = max |w_i|^2: the scale does not change u / sum u and keeps the two terms comparable)
// lies in LDS by corral slot, (D + 1)^2 doubles a wave, one row and one column written when a
// vertex enters, the last slot moved into a dropped one.  A minor cycle solves it afresh by
// Gauss-Jordan elimination without pivoting (the matrix is positive definite): lane a holds
// row a in registers, the loops are unrolled so every register index is static, and the pivot
// row goes round by v_readlane.  Every branch is on a reduced, broadcast value; the loop is
// `for (cycle = 0; cycle < max_iter; ++cycle)`, a cycle one major or one minor step.
#include "hull.h"
#include <cmath>

#define HULL_THREADS (HULL_WAVES * 64)

namespace {

// lane j's value for every lane, j wave-uniform
__device__ __forceinline__ int lane_get(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ double lane_get(double v, int j) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, j);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), j);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// the smallest / largest value of the wave, the same bits in every lane (a NaN loses to a number)
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return lane_get(v, 0);
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return lane_get(v, 0);
}
// the lowest lane of a ballot, -1 for an empty one
__device__ __forceinline__ int first_lane(unsigned long long m) { return __ffsll((long long)m) - 1; }
// LDS written by some lanes of the wave is read by others: keep the accesses in program order
__device__ __forceinline__ void wave_lds_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

}  // namespace

template <int D>
__global__ __launch_bounds__(HULL_THREADS) void k_hull(const HullArgs a) {
  constexpr int HM = D + 1;  // the most vertices of a corral: affinely independent in D dimensions
  __shared__ double Gs[HULL_WAVES][HM * HM];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * HULL_WAVES + wv;
  if (b >= a.B) return;  // wave-uniform; the kernel has no workgroup barrier
  double *G = Gs[wv];
  const int d = a.d, kmax = a.kmax;
  int nv = a.nv ? a.nv[b] : kmax;
  nv = nv < 0 ? 0 : (nv > kmax ? kmax : nv);
  const bool live = lane < nv;
  const double *xq = a.X + b * d;

  // w_i = v_i - x, zero in the padding and in the lanes without a vertex
  int64_t r = 0;
  if (live) r = a.gidx ? (int64_t)a.gidx[b * kmax + lane] : (a.shared ? (int64_t)lane : b * kmax + lane);
  const double *row = a.V + r * d;
  double w[D], nrm2 = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double xk = k < d ? xq[k] : 0.0;
    const double vk = live && k < d ? row[k] : xk;
    w[k] = vk - xk;
    nrm2 += w[k] * w[k];
  }
  const double qi = a.q && live ? a.q[r] : 0.0;

  double *lam_out = a.lambda + b * kmax;
  if (nv == 0) {  // the reference's K == 0 branch
    if (lane < kmax) lam_out[lane] = 0.0;
    if (lane == 0) {
      for (int k = 0; k < d; ++k) a.proj[b * d + k] = xq[k];
      a.dist[b] = INFINITY;
      a.gap[b] = 0.0;
      if (a.q) a.qhull[b] = INFINITY;
      a.iters[b] = 0;
      a.status[b] = 2;
    }
    return;
  }
  if (__ballot(live && !isfinite(nrm2))) {  // a non-finite x or vertex (or a difference that overflows)
    if (lane < kmax) lam_out[lane] = live ? NAN : 0.0;
    if (lane == 0) {
      for (int k = 0; k < d; ++k) a.proj[b * d + k] = NAN;
      a.dist[b] = NAN;
      a.gap[b] = NAN;
      if (a.q) a.qhull[b] = NAN;
      a.iters[b] = 0;
      a.status[b] = 3;
    }
    return;
  }

  const double maxn = wave_max(live ? nrm2 : 0.0);
  const double s = maxn;
  // p = sum l_i w_i over the corral, the same in every lane; -> |p|^2, p . w_i of this lane
  double lam = 0.0;
  int slot = -1, m = 0;
  double p[D], pp, pw;
  auto evaluate = [&]() {
#pragma unroll
    for (int k = 0; k < D; ++k) p[k] = 0.0;
    for (int c = 0; c < m; ++c) {
      const int j = first_lane(__ballot(slot == c));
      const double lj = lane_get(lam, j);
#pragma unroll
      for (int k = 0; k < D; ++k) p[k] += lj * lane_get(w[k], j);
    }
    pp = 0.0;
    pw = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      pp += p[k] * p[k];
      pw += p[k] * w[k];
    }
  };

  // start: the vertex nearest the query
  {
    const double mn = wave_min(live ? nrm2 : INFINITY);
    const int j0 = first_lane(__ballot(live && nrm2 == mn));
    if (lane == j0) {
      lam = 1.0;
      slot = 0;
      G[0] = s + nrm2;
    }
    m = 1;
  }
  int status = 1, cycle = 0;
  bool minor = false;
  for (cycle = 0; cycle < a.max_iter; ++cycle) {
    if (!minor) {
      evaluate();
      const double mn = wave_min(live ? pw : INFINITY);
      if (pp - mn <= a.tol * maxn) {
        status = 0;
        break;
      }
      const int j = first_lane(__ballot(live && pw == mn));
      if (j < 0 || lane_get(slot, j) >= 0 || m == HM) break;  // no vertex to make progress with
      // the product summed at its own magnitude, s added once: summed from s every addition
      // would round at s, and the minimum-norm point inherits the matrix's rounding
      double g = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) g += w[k] * lane_get(w[k], j);
      g += s;
      if (lane == j) slot = m;
      if (slot >= 0) {
        G[slot * HM + m] = g;
        G[m * HM + slot] = g;
      }
      ++m;
      minor = true;
      continue;
    }
    // minor cycle: (s e e' + Q Q') u = e by Gauss-Jordan, lane c < m holds row c and its right side
    wave_lds_order();
    double A[HM], t = lane < m ? 1.0 : 0.0, diag = 1.0;
#pragma unroll
    for (int c = 0; c < HM; ++c) A[c] = lane < m && c < m ? G[lane * HM + c] : (lane == c ? 1.0 : 0.0);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < HM; ++k) {
      if (k < m && ok) {
        const double piv = lane_get(A[k], k);
        if (!(piv > 0.0)) {
          ok = false;
        } else {
          const double f = lane == k ? 0.0 : A[k] / piv;
          t -= f * lane_get(t, k);
#pragma unroll
          for (int c = k + 1; c < HM; ++c) A[c] -= f * lane_get(A[c], k);
          if (lane == k) diag = piv;
        }
      }
    }
    const double u = t / diag;
    const double su = wave_sum(lane < m ? u : 0.0);
    const double us = __shfl(u, slot >= 0 ? slot : 0, 64);  // by every lane: the source lanes stay active
    const double al = slot >= 0 ? us / su : 0.0;            // of this lane's vertex
    if (!ok || !(su > 0.0) || __ballot(slot >= 0 && !isfinite(al))) break;  // numerically dependent
    const unsigned long long out = __ballot(slot >= 0 && !(al > 0.0));
    if (!out) {
      lam = al;
      minor = false;
      continue;
    }
    // towards al up to the boundary; the vertex that reaches zero leaves
    const bool cand = slot >= 0 && !(al > 0.0);
    const double th = cand ? (lam - al > 0.0 ? lam / (lam - al) : 0.0) : INFINITY;
    double theta = wave_min(th);
    const int r = first_lane(__ballot(cand && th == theta));
    if (r < 0) break;
    theta = theta < 1.0 ? theta : 1.0;
    lam = slot >= 0 ? fmax(lam + theta * (al - lam), 0.0) : 0.0;
    const int rs = lane_get(slot, r), last = m - 1;
    if (lane == r) {
      lam = 0.0;
      slot = -1;
    }
    wave_lds_order();
    if (rs != last) {  // the last slot's row and column move into the freed one
      if (slot == last) {
        G[rs * HM + rs] = G[last * HM + last];
        slot = rs;
      } else if (slot >= 0) {
        const double v = G[last * HM + slot];
        G[rs * HM + slot] = v;
        G[slot * HM + rs] = v;
      }
    }
    --m;
  }

  evaluate();
  const double mn = wave_min(live ? pw : INFINITY);
  const double qh = a.q ? wave_sum(lam * qi) : 0.0;
  if (lane < kmax) lam_out[lane] = live ? lam : 0.0;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (k < d) a.proj[b * d + k] = xq[k] + p[k];
    a.dist[b] = sqrt(pp);
    a.gap[b] = maxn > 0.0 ? (pp - mn) / maxn : 0.0;
    if (a.q) a.qhull[b] = qh;
    a.iters[b] = cycle < a.max_iter ? cycle + 1 : a.max_iter;
    a.status[b] = status;
  }
}

hipError_t launch_hull(hipStream_t s, const HullArgs &a) {
  if (a.B <= 0) return hipSuccess;
  const dim3 grid((unsigned)(((int64_t)a.B + HULL_WAVES - 1) / HULL_WAVES)), block(HULL_THREADS);
  if (a.d <= 4) hipLaunchKernelGGL(k_hull<4>, grid, block, 0, s, a);
  else if (a.d <= 8) hipLaunchKernelGGL(k_hull<8>, grid, block, 0, s, a);
  else if (a.d <= 16) hipLaunchKernelGGL(k_hull<16>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_hull<32>, grid, block, 0, s, a);
  return hipGetLastError();
}

extern "C" int gpmpc_hull_plan(int d, int kmax, int B, int *q_per_group) {
  GPMPC_CHECK_ARG(q_per_group);
  GPMPC_CHECK_ARG(d >= 1 && d <= HULL_MAXD);
  GPMPC_CHECK_ARG(kmax >= 1 && kmax <= HULL_MAXK);
  GPMPC_CHECK_ARG(B >= 0);
  *q_per_group = HULL_WAVES;
  return 0;
}

extern "C" int gpmpc_hull_project(gpmpc_ctx *ctx, const double *V, const double *q, const int *nv, int shared,
                                  const double *X, int B, int kmax, int d, double tol, int max_iter, double *lambda,
                                  double *proj, double *dist, double *gap, double *qhull, int *iters, int *status) {
  // the shapes first: they are refused without a context (and so without a device) too
  GPMPC_CHECK_ARG(d >= 1 && d <= HULL_MAXD);
  GPMPC_CHECK_ARG(kmax >= 1 && kmax <= HULL_MAXK);
  GPMPC_CHECK_ARG(shared == 0 || shared == 1);
  GPMPC_CHECK_ARG(tol > 0.0 && tol < INFINITY);
  GPMPC_CHECK_ARG(max_iter >= 1 && max_iter <= HULL_MAX_ITER);
  GPMPC_CHECK_ARG(B >= 0);
  if (B > 0) {
    GPMPC_CHECK_ARG(V && X && lambda && proj && dist && gap && iters && status);
    GPMPC_CHECK_ARG(!q || qhull);
    if (nv)
      for (int b = 0; b < B; ++b) GPMPC_CHECK_ARG(nv[b] >= 0 && nv[b] <= kmax);
  }
  GPMPC_CHECK_ARG(ctx);
  if (B == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t nb = (size_t)B, sets = shared ? 1 : nb, kd = (size_t)kmax * d;
  Stage sg(s);
  HullArgs a{};
  sg.in(&a.V, V, sets * kd);
  sg.in(&a.q, q, sets * kmax);  // null without q
  sg.in(&a.nv, nv, nb);         // null without nv
  sg.in(&a.X, X, nb * d);
  a.gidx = nullptr;
  a.B = B;
  a.kmax = kmax;
  a.d = d;
  a.shared = shared;
  a.tol = tol;
  a.max_iter = max_iter;
  sg.out(&a.lambda, lambda, nb * kmax);
  sg.out(&a.proj, proj, nb * d);
  sg.out(&a.dist, dist, nb);
  sg.out(&a.gap, gap, nb);
  sg.out(&a.qhull, q ? qhull : nullptr, nb);  // (written when a.q is given)
  sg.out(&a.iters, iters, nb);
  sg.out(&a.status, status, nb);
  if (int rc = sg.commit("hull_project")) return rc;
  GPMPC_HIP(launch_hull(s, a));
  GPMPC_HIP(sg.download());
  return 0;
}
