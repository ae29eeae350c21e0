// kmeans.hip -- Lloyd's iteration for the sparse GP's inducing points in fp64.
//
// Reference: SparseGP._initialize_inducing_points (sparse_gp.py:122-148) calls
// scipy.cluster.vq.kmeans2(X, k, minit="points"): from a code book C0 = X[idx] it repeats
// `iter` times  label = vq(X, C)  (for every observation the first index of the strict
// minimum of the squared distance) and  C = update_cluster_means(X, label)  (every
// observation added into its cluster's row in ascending observation order, starting from
// zero; one division by the member count; a cluster without members keeps its previous row),
// and returns the last code book with the labels of the last vq.
//
// What is pinned and what is free.  The update is pinned: given equal labels, the plain
// rounded adds in ascending observation order and the one division are scipy's bits.  The
// distance is free: scipy forms |x|^2 + |c|^2 - 2 x.c through BLAS for d >= 5, whose bits
// cannot be had by construction; k_km_assign sums (x - c)^2 directly.  The labels agree
// whenever nearest and second nearest are further apart than both formulas' rounding, and
// the guard below says when that is not certain; the caller then hands the draw to scipy.
//
// The guard.  margin = (second smallest - smallest squared distance) / (|x|^2 + max_j |c_j|^2),
// a decision is unsafe when margin <= tau = 16 (d + 2) 2^-53 (also when the scale is 0 or the
// margin is not a number).  To first order in u = 2^-53, with S = |x|^2 + |c|^2:
//   expanded form: the two squared norms err by d u (|x|^2 + |c|^2), the doubled dot product by
//     2 d u |x|.|c| <= d u S, the two final additions (of terms <= 2 S) by 4 u S:
//     (2d + 4) u S per distance;
//   direct form: each (x_f - c_f)^2 carries 2 u, the d-term sum d - 1 more: at most
//     (d + 2) u dist^2 <= 2 (d + 2) u S per distance, as dist^2 <= 2 S.
// Either formula orders two centres like the exact distances when their exact gap exceeds the
// sum of its two errors, 4 (d + 2) u S_max.  The kernel sees the computed direct gap, itself
// within 4 (d + 2) u S_max of the exact one, so a computed gap above 8 (d + 2) u S_max is
// enough; tau is twice that, which also covers the rounding of the scale and the quotient.
// Centres further than the second nearest have a larger computed gap still.
//
// Launches: one k_km_assign and one k_km_update per iteration on the context's stream; the
// kernel boundary is the only ordering between workgroups.  No kernel waits on another
// workgroup.
//
// The file is compiled with contraction off, like select.hip: the update's adds must round.
#include "internal.h"
#include <climits>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

#define KM_MAXD 32           // = SEL_MAXD
#define KM_TILE 128          // centres per LDS tile of k_km_assign
#define KM_OBS 64            // k_km_assign: observations per workgroup (n = 4000: 63 CUs busy; 256: 16)
#define KM_WAVES 8           // ... and its waves: each scans every KM_WAVES-th centre for the same 64
#define KM_THREADS (KM_OBS * KM_WAVES)
#define KM_UPD_THREADS 256   // k_km_update: four waves, one cluster each
#define KM_TAU_FACTOR 16.0   // tau = KM_TAU_FACTOR (d + 2) 2^-53

// bit pattern of a non-negative double: ordered like the value as an unsigned integer
__device__ __forceinline__ unsigned long long km_bits(double v) {
  return (unsigned long long)__double_as_longlong(v);
}

// ---------------------------------------------------------------------------
// label[i] = the lowest index of the smallest |X[i] - C[j]|^2.  A workgroup owns KM_OBS
// observations, lane l of every wave observation l (its row in registers); the code book is
// staged through LDS KM_TILE rows at a time and read as wave-uniform broadcasts (as
// k_nn_dist), wave w taking rows w, w + KM_WAVES, ... of each tile.  Within a wave j runs
// upward with a strict <, and the waves' (smallest, its index, second smallest) are merged
// through LDS with the lower index winning equal values: the lowest index over all centres.
// The call's two scalars: the minimum margin (an integer atomic minimum on the bit pattern) and
// the count of unsafe decisions.
template <int D>
__global__ __launch_bounds__(KM_THREADS) void k_km_assign(const double *__restrict__ X, int n,
                                                        const double *__restrict__ C, int k,
                                                        const double *__restrict__ cmax, double tau,
                                                        int *__restrict__ label,
                                                        unsigned long long *__restrict__ min_margin,
                                                        int *__restrict__ unsafe) {
  __shared__ double sc[KM_TILE * D];
  __shared__ double sbest[KM_WAVES][KM_OBS], ssecond[KM_WAVES][KM_OBS];
  __shared__ int sidx[KM_WAVES][KM_OBS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * KM_OBS + lane;
  const bool live = i < n;
  double x[D];
  double xx = 0.0;
#pragma unroll
  for (int f = 0; f < D; ++f) {
    x[f] = live ? X[i * D + f] : 0.0;
    xx += x[f] * x[f];
  }
  double best = INFINITY, second = INFINITY;
  int bi = INT_MAX;  // no centre compared below inf yet
  for (int t0 = 0; t0 < k; t0 += KM_TILE) {
    const int rows = min(KM_TILE, k - t0);
    __syncthreads();  // the previous tile's readers are done
    for (int e = tid; e < rows * D; e += KM_THREADS) sc[e] = C[(int64_t)t0 * D + e];
    __syncthreads();
#pragma unroll 2
    for (int j = wv; j < rows; j += KM_WAVES) {
      const double *row = sc + j * D;
      double d2 = 0.0;
#pragma unroll
      for (int f = 0; f < D; ++f) {
        const double df = x[f] - row[f];
        d2 += df * df;
      }
      if (d2 < best) {
        second = best;
        best = d2;
        bi = t0 + j;
      } else if (d2 < second) {
        second = d2;
      }
    }
  }
  sbest[wv][lane] = best;
  ssecond[wv][lane] = second;
  sidx[wv][lane] = bi;
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int w = 1; w < KM_WAVES; ++w) {
    const double ob = sbest[w][lane], os = ssecond[w][lane];
    const int oi = sidx[w][lane];
    if (ob < best || (ob == best && oi < bi)) {
      second = best < os ? best : os;
      best = ob;
      bi = oi;
    } else {
      second = ob < second ? ob : second;
    }
  }
  if (live) label[i] = (unsigned)bi < (unsigned)k ? bi : 0;  // every distance inf or not a number: 0
  // one centre: second = inf, the margin inf (safe).  Scale 0, or a margin that is not a number
  // (overflowed distances): unsafe, reported as margin 0.
  const double scale = xx + cmax[0];
  double m = scale > 0.0 ? (second - best) / scale : 0.0;
  const bool bad = live && !(m > tau);
  m = live ? (m >= 0.0 ? m : 0.0) : INFINITY;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(m, off, 64);
    m = o < m ? o : m;
  }
  const int nbad = __popcll(__ballot(bad));
  if (lane == 0) {
    atomicMin(min_margin, km_bits(m));
    if (nbad) atomicAdd(unsafe, nbad);
  }
}

// ---------------------------------------------------------------------------
// Cout[c] = the mean of the observations labelled c, in scipy's order: one wave per cluster,
// lane f < d owns feature f.  The wave walks the labels 64 at a time: a ballot of label == c,
// then its set bits in ascending order, each a plain rounded add of X[i * d + f]; one
// division by the count at the end.  (The loads run ahead of the adds, four label words and
// four members at a time; the adds keep their order.)  Without members the previous row is
// kept and the iteration's empty counter goes up by one.  The largest |c|^2 of the new code
// book goes to cmax_next for the next assign's scale (an integer atomic maximum on the bit
// pattern).
__global__ __launch_bounds__(KM_UPD_THREADS) void k_km_update(const double *__restrict__ X, int n, int d,
                                                             const int *__restrict__ label,
                                                             const double *__restrict__ Cin, int k,
                                                             double *__restrict__ Cout,
                                                             int *__restrict__ empty,
                                                             unsigned long long *__restrict__ cmax_next) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (KM_UPD_THREADS / 64) + (threadIdx.x >> 6);
  if (c >= k) return;  // the whole wave
  const bool own = lane < d;
  double acc = 0.0;
  int cnt = 0;
  for (int64_t base0 = 0; base0 < n; base0 += 256) {
    bool hit[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t i = base0 + 64 * q + lane;
      hit[q] = i < n && label[i] == c;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t base = base0 + 64 * q;
      unsigned long long m = __ballot(hit[q]);
      cnt += __popcll(m);
      while (m) {
        int b[4];
        double v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          b[r] = m ? __ffsll((long long)m) - 1 : -1;
          m &= m - 1;  // (0 stays 0)
          v[r] = own && b[r] >= 0 ? X[(base + b[r]) * d + lane] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (b[r] >= 0) acc += v[r];  // (the wave as one: b is the same in every lane)
      }
    }
  }
  double v = 0.0;
  if (own) {
    v = cnt > 0 ? acc / (double)cnt : Cin[(int64_t)c * d + lane];
    Cout[(int64_t)c * d + lane] = v;
  }
  double sq = v * v;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
  if (lane == 0) {
    atomicMax(cmax_next, km_bits(sq));
    if (cnt == 0) atomicAdd(empty, 1);
  }
}

// the assign kernel is instantiated for every width 1 .. KM_MAXD
#define KM_DISPATCH(d, CALL)                                                                  \
  switch (d) {                                                                                \
    case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;               \
    case 4: CALL(4); break;   case 5: CALL(5); break;   case 6: CALL(6); break;               \
    case 7: CALL(7); break;   case 8: CALL(8); break;   case 9: CALL(9); break;               \
    case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;             \
    case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break;             \
    case 16: CALL(16); break; case 17: CALL(17); break; case 18: CALL(18); break;             \
    case 19: CALL(19); break; case 20: CALL(20); break; case 21: CALL(21); break;             \
    case 22: CALL(22); break; case 23: CALL(23); break; case 24: CALL(24); break;             \
    case 25: CALL(25); break; case 26: CALL(26); break; case 27: CALL(27); break;             \
    case 28: CALL(28); break; case 29: CALL(29); break; case 30: CALL(30); break;             \
    case 31: CALL(31); break; default: CALL(32);                                              \
  }

// ---------------------------------------------------------------------------
// C-ABI
extern "C" double gpmpc_kmeans_tau(int d) { return KM_TAU_FACTOR * (double)(d + 2) * 0x1p-53; }

extern "C" int gpmpc_kmeans_lloyd(gpmpc_ctx *ctx, const double *X, int n, int d, const double *C0, int k,
                                  int iters, double *C_out, int *labels_out, int *empty_per_iter,
                                  double *min_margin, int *unsafe) {
  GPMPC_CHECK_ARG(ctx && X && C0 && C_out && labels_out && empty_per_iter && min_margin && unsafe);
  GPMPC_CHECK_ARG(d >= 1 && d <= KM_MAXD);
  GPMPC_CHECK_ARG(n >= 1 && k >= 1 && iters >= 1);
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t nd = (size_t)n * d, kd = (size_t)k * d, ni = (size_t)iters;
  // the scalars start on the host and travel with the one upload: margin inf, counters 0, and
  // the scale's max |c|^2 per assign (C0's from here, the later ones from the update kernel)
  std::vector<double> cmax(ni + 1, 0.0);
  for (size_t j = 0; j < (size_t)k; ++j) {
    double sq = 0.0;
    for (int f = 0; f < d; ++f) sq += C0[j * d + f] * C0[j * d + f];
    if (!(sq <= cmax[0])) cmax[0] = sq;
  }
  *min_margin = INFINITY;
  *unsafe = 0;
  for (size_t t = 0; t < ni; ++t) empty_per_iter[t] = 0;
  DevBuf dA, dB;  // the code books between the first and the last
  if (iters > 1) GPMPC_HIP(dA.alloc(s, sizeof(double) * kd));
  if (iters > 2) GPMPC_HIP(dB.alloc(s, sizeof(double) * kd));
  Stage sg(s);
  const double *dX, *dC0;
  double *dcmax, *dmargin, *dC;
  int *dunsafe, *dempty, *dlabel;
  sg.in(&dX, X, nd); sg.in(&dC0, C0, kd);
  sg.in(&dcmax, cmax.data(), ni + 1);  // (cmax lives until the commit packs it)
  sg.inout(&dmargin, min_margin, 1);
  sg.inout(&dunsafe, unsafe, 1); sg.inout(&dempty, empty_per_iter, ni);
  sg.out(&dC, C_out, kd);
  sg.out(&dlabel, labels_out, (size_t)n);
  if (int rc = sg.commit("kmeans_lloyd")) return rc;
  const double tau = gpmpc_kmeans_tau(d);
  const dim3 ga((unsigned)(((int64_t)n + KM_OBS - 1) / KM_OBS));
  const dim3 gu((unsigned)(((int64_t)k + KM_UPD_THREADS / 64 - 1) / (KM_UPD_THREADS / 64)));
  const double *src = dC0;
  for (int t = 0; t < iters; ++t) {
    double *dst = t == iters - 1 ? dC : ((t & 1) ? dB.as<double>() : dA.as<double>());
#define KM_CALL(DD)                                                                             \
  hipLaunchKernelGGL(k_km_assign<DD>, ga, dim3(KM_THREADS), 0, s, dX, n, src, k, dcmax + t, tau, \
                     dlabel, (unsigned long long *)dmargin, dunsafe)
    KM_DISPATCH(d, KM_CALL)
#undef KM_CALL
    GPMPC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_km_update, gu, dim3(KM_UPD_THREADS), 0, s, dX, n, d, (const int *)dlabel, src, k, dst,
                       dempty + t, (unsigned long long *)(dcmax + t + 1));
    GPMPC_HIP(hipGetLastError());
    src = dst;
  }
  GPMPC_HIP(sg.download());
  return 0;
}
