// select.hip -- novelty / diverse-subset selection of GP training data in fp64.
//
// Reference: NoveltySelector._compute_distance_novelty (novelty_selector.py:154-170, the
// brute-force branch) and the greedy loop of NoveltySelector.select_diverse
// (novelty_selector.py:264-296), restated with a running minimum: pick 0 = argmax(scores),
// pick t = argmax over the unselected i of scores[i] + w * mind[i], mind[i] the distance to
// the nearest pick so far, lowest index on equal values (the reference scans in ascending
// index order with a strict >).
//
// Summation order: every squared distance is formed the way numpy forms
// np.linalg.norm(A - x, axis=1) on a C-contiguous array -- rounded difference, rounded
// square, no FMA, and add.reduce's order along a contiguous axis: d < 8 left to right;
// d >= 8 eight accumulators over elements 0..7, every further full block of eight added
// lane-wise, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the d % 8 tail one by one.  The
// square root is the correctly rounded one.  With that order the combined scores are the
// reference's bits and the picks its indices, ties included.
//
// The whole file is compiled with contraction off: hipcc's default fuses a product into a
// following sum, also through the header's __dmul_rn / __dadd_rn (plain operators there),
// so the rounded operations are sqdist.h's mul_rn / add_rn / sub_rn.
#include "internal.h"
#include "sqdist.h"
#include <climits>
#include <cmath>

#pragma clang fp contract(off)

#define SEL_MAXD 32          // = GRAM_MAXD
#define NN_TILE 128          // reference rows per LDS tile (k_nn_dist)
#define NN_THREADS 256
#define SEL1_THREADS 512     // path 1: the one workgroup (2 waves a SIMD: 256 VGPRs a thread)
#define SEL1_CPT 16          // candidates a path-1 thread keeps in registers
#define SEL1_MAXN (SEL1_THREADS * SEL1_CPT)
#define SEL2_THREADS 256     // path 2: a workgroup ...
#define SEL2_CPT 4           // ... and the candidates per thread
#define SEL2_SLICE (SEL2_THREADS * SEL2_CPT)
// automatic path: one workgroup up to this n, the grid above it (docs/PERF_HISTORY.md)
#define SEL_CROSSOVER 6144

// mul_rn / add_rn / sub_rn and sqdist (|x - y|^2 in numpy's order) are sqdist.h's, shared with knn.hip

// ---------------------------------------------------------------------------
// dist[i] = min_j |X[i] - R[j]|: one candidate per thread (its row in registers), the
// reference rows staged through LDS NN_TILE at a time and read as wave-uniform
// broadcasts.  The minimum is taken over the squared sums; one sqrt at the end.
template <int D>
__global__ __launch_bounds__(NN_THREADS) void k_nn_dist(const double *__restrict__ X, int n,
                                                        const double *__restrict__ R, int r,
                                                        double *__restrict__ dist) {
  __shared__ double sr[NN_TILE * D];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * NN_THREADS + tid;
  const bool live = i < n;
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = live ? X[i * D + k] : 0.0;
  double best = INFINITY;
  for (int t0 = 0; t0 < r; t0 += NN_TILE) {
    const int rows = min(NN_TILE, r - t0);
    __syncthreads();  // the previous tile's readers are done
    for (int e = tid; e < rows * D; e += NN_THREADS) sr[e] = R[(int64_t)t0 * D + e];
    __syncthreads();
    for (int j = 0; j < rows; ++j) {
      const double *row = sr + j * D;
      const double d2 = sqdist<D>(x, [&](int k) { return row[k]; });
      best = d2 < best ? d2 : best;
    }
  }
  if (live) dist[i] = sqrt(best);
}

// X (n x d row-major) -> Xt (d x n): the selection kernels read one feature of
// consecutive candidates per load
__global__ void k_sel_transpose(const double *__restrict__ X, int n, int d,
                                double *__restrict__ Xt) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n * d) return;
  const int64_t i = e / d;
  const int k = (int)(e - i * d);
  Xt[(int64_t)k * n + i] = X[e];
}

// argmax with the lowest index on equal values
__device__ __forceinline__ void best_of(double &bv, int &bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

__device__ __forceinline__ void wave_best(double &bv, int &bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    best_of(bv, bi, ov, oi);
  }
}

// ---------------------------------------------------------------------------
// Path 1: one workgroup, one launch for all picks.  Thread tid owns candidates
// tid + j * SEL1_THREADS (j < SEL1_CPT): their running minimum distance and selected
// flags stay in registers.  A pick: update against the last pick's row -> per-thread
// argmax -> wave reduction by shuffles -> the waves' results through LDS (two buffers by
// pick parity: one barrier a pick).
template <int D>
__global__ __launch_bounds__(SEL1_THREADS) void k_select_one(const double *__restrict__ Xt, int n,
                                                             const double *__restrict__ scores,
                                                             int n_select, double w,
                                                             int *__restrict__ idx_out,
                                                             double *__restrict__ comb_out) {
  constexpr int NW = SEL1_THREADS / 64;
  __shared__ double sv[2][NW];
  __shared__ int si[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cpt = (n + SEL1_THREADS - 1) / SEL1_THREADS;  // <= SEL1_CPT (host check)
  double mind[SEL1_CPT];
#pragma unroll
  for (int j = 0; j < SEL1_CPT; ++j) mind[j] = INFINITY;
  unsigned taken = 0;  // bit j: candidate j of this thread is selected
  int win = -1;
  for (int t = 0; t < n_select; ++t) {
    double p[D];
    if (t > 0) {
#pragma unroll
      for (int k = 0; k < D; ++k) p[k] = Xt[(int64_t)k * n + win];
    }
    double bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int j = 0; j < SEL1_CPT; ++j) {
      if (j < cpt) {
        int i = tid + j * SEL1_THREADS;
        // the index is re-formed every pick: hoisted out of the pick loop, the D * SEL1_CPT
        // load addresses it feeds would take every register and spill
        asm volatile("" : "+v"(i));
        if (i < n && !((taken >> j) & 1u)) {
          double v = scores[i];
          if (t > 0) {
            const double d2 = sqdist<D>(p, [&](int k) { return Xt[(int64_t)k * n + i]; });
            const double ds = sqrt(d2);
            mind[j] = ds < mind[j] ? ds : mind[j];
            v = add_rn(v, mul_rn(w, mind[j]));
          }
          best_of(bv, bi, v, i);
        }
      }
    }
    wave_best(bv, bi);
    const int pb = t & 1;
    if (lane == 0) {
      sv[pb][wv] = bv;
      si[pb][wv] = bi;
    }
    __syncthreads();
    bv = sv[pb][0];
    bi = si[pb][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) best_of(bv, bi, sv[pb][q], si[pb][q]);
    win = __builtin_amdgcn_readfirstlane(bi);
    // no candidate compared greater than -inf (NaN scores past the binding's check): the
    // remaining picks stay -1 and the entry point refuses
    if ((unsigned)win >= (unsigned)n) return;
    if (tid == 0) {
      idx_out[t] = win;
      if (comb_out) comb_out[t] = bv;
    }
    if ((win & (SEL1_THREADS - 1)) == tid) taken |= 1u << (win / SEL1_THREADS);
  }
}

// ---------------------------------------------------------------------------
// Path 2: a grid of workgroups, one launch per pick (launches 0 .. n_select).  Launch
// t > 0 first reduces launch t-1's per-workgroup partials (value, index; lowest index on
// equal value) -- every workgroup reads them all, so each knows pick t-1 without any
// in-launch hand-off; workgroup 0 records it.  Each workgroup then updates its slice of
// SEL2_SLICE candidates against the picked row and writes its own partial for pick t.
// The partials are two buffers by pick parity; ordering is the kernel boundary alone.
// Launch n_select only reduces and records.
template <int D>
__global__ __launch_bounds__(SEL2_THREADS) void k_select_grid(
    const double *__restrict__ Xt, int n, const double *__restrict__ scores, int t, int n_select,
    int nparts, double w, double *__restrict__ mind, unsigned char *__restrict__ taken,
    const double *__restrict__ pv_in, const int *__restrict__ pi_in, double *__restrict__ pv_out,
    int *__restrict__ pi_out, int *__restrict__ idx_out, double *__restrict__ comb_out) {
  constexpr int NW = SEL2_THREADS / 64;
  __shared__ double sv[2][NW];
  __shared__ int si[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int win = -1;
  bool valid = true;
  if (t > 0) {
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int q = tid; q < nparts; q += SEL2_THREADS) best_of(bv, bi, pv_in[q], pi_in[q]);
    wave_best(bv, bi);
    if (lane == 0) {
      sv[0][wv] = bv;
      si[0][wv] = bi;
    }
    __syncthreads();
    bv = sv[0][0];
    bi = si[0][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) best_of(bv, bi, sv[0][q], si[0][q]);
    win = __builtin_amdgcn_readfirstlane(bi);
    valid = (unsigned)win < (unsigned)n;  // else: no pick (k_select_one), idx_out stays -1
    if (valid && blockIdx.x == 0 && tid == 0) {
      idx_out[t - 1] = win;
      if (comb_out) comb_out[t - 1] = bv;
    }
    if (t == n_select) return;
  }
  double p[D];
  if (t > 0 && valid) {
#pragma unroll
    for (int k = 0; k < D; ++k) p[k] = Xt[(int64_t)k * n + win];
  }
  double bv = -INFINITY;
  int bi = INT_MAX;
  const int64_t base = (int64_t)blockIdx.x * SEL2_SLICE;
#pragma unroll
  for (int j = 0; j < SEL2_CPT; ++j) {
    const int64_t i64 = base + tid + j * SEL2_THREADS;
    if (i64 < n && valid) {  // without a pick every partial is (-inf, none) from here on
      const int i = (int)i64;
      if (t == 0) {
        mind[i] = INFINITY;
        taken[i] = 0;
        best_of(bv, bi, scores[i], i);
      } else if (i == win) {
        taken[i] = 1;
      } else if (!taken[i]) {
        const double d2 = sqdist<D>(p, [&](int k) { return Xt[(int64_t)k * n + i]; });
        const double ds = sqrt(d2);
        const double m0 = mind[i];
        const double m = ds < m0 ? ds : m0;
        mind[i] = m;
        best_of(bv, bi, add_rn(scores[i], mul_rn(w, m)), i);
      }
    }
  }
  wave_best(bv, bi);
  if (lane == 0) {
    sv[1][wv] = bv;
    si[1][wv] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    bv = sv[1][0];
    bi = si[1][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) best_of(bv, bi, sv[1][q], si[1][q]);
    pv_out[blockIdx.x] = bv;
    pi_out[blockIdx.x] = bi;
  }
}

// the kernels are instantiated for every width 1 .. SEL_MAXD
#define SEL_DISPATCH(d, CALL)                                                                 \
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
// C-ABI: host buffers in, host buffers out.
extern "C" int gpmpc_nn_dist(gpmpc_ctx *ctx, const double *X, int n, const double *R, int r, int d,
                             double *dist) {
  GPMPC_CHECK_ARG(ctx && X && R && dist);
  GPMPC_CHECK_ARG(d >= 1 && d <= SEL_MAXD);
  GPMPC_CHECK_ARG(n >= 0 && r >= 1);
  if (n == 0) return 0;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf dX, dR, dd;
  GPMPC_HIP(dX.alloc(s, sizeof(double) * (size_t)n * d));
  GPMPC_HIP(dR.alloc(s, sizeof(double) * (size_t)r * d));
  GPMPC_HIP(dd.alloc(s, sizeof(double) * (size_t)n));
  GPMPC_HIP(hipMemcpyAsync(dX.p, X, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, s));
  GPMPC_HIP(hipMemcpyAsync(dR.p, R, sizeof(double) * (size_t)r * d, hipMemcpyHostToDevice, s));
  const dim3 g((unsigned)(((int64_t)n + NN_THREADS - 1) / NN_THREADS));
#define NN_CALL(DD)                                                                            \
  hipLaunchKernelGGL(k_nn_dist<DD>, g, dim3(NN_THREADS), 0, s, dX.as<double>(), n, dR.as<double>(), \
                     r, dd.as<double>())
  SEL_DISPATCH(d, NN_CALL)
#undef NN_CALL
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(hipMemcpyAsync(dist, dd.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gpmpc_select_diverse(gpmpc_ctx *ctx, const double *X, int n, int d,
                                    const double *scores, int n_select, double diversity_weight,
                                    int path, int *idx_out, double *combined_out) {
  GPMPC_CHECK_ARG(ctx && X && scores && idx_out);
  GPMPC_CHECK_ARG(d >= 1 && d <= SEL_MAXD);
  GPMPC_CHECK_ARG(n >= 1 && n_select >= 1 && n_select <= n);
  GPMPC_CHECK_ARG(path >= 0 && path <= 2);
  GPMPC_CHECK_ARG(path != 1 || n <= SEL1_MAXN);  // past the one workgroup's registers
  if (path == 0) path = n <= SEL_CROSSOVER && n <= SEL1_MAXN ? 1 : 2;
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int nwg = (int)(((int64_t)n + SEL2_SLICE - 1) / SEL2_SLICE);
  const size_t nd = (size_t)n * d;
  DevBuf dX, dXt, dsc, didx, dcomb, dmind, dtaken, dpv, dpi;
  GPMPC_HIP(dX.alloc(s, sizeof(double) * nd));
  GPMPC_HIP(dXt.alloc(s, sizeof(double) * nd));
  GPMPC_HIP(dsc.alloc(s, sizeof(double) * (size_t)n));
  GPMPC_HIP(didx.alloc(s, sizeof(int) * (size_t)n_select));
  GPMPC_HIP(dcomb.alloc(s, sizeof(double) * (size_t)n_select));
  GPMPC_HIP(hipMemcpyAsync(dX.p, X, sizeof(double) * nd, hipMemcpyHostToDevice, s));
  GPMPC_HIP(hipMemcpyAsync(dsc.p, scores, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_sel_transpose, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s,
                     dX.as<double>(), n, d, dXt.as<double>());
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(hipMemsetAsync(didx.p, 0xFF, sizeof(int) * (size_t)n_select, s));  // -1: no pick
  double *comb = combined_out ? dcomb.as<double>() : nullptr;
  if (path == 1) {
#define ONE_CALL(DD)                                                                          \
  hipLaunchKernelGGL(k_select_one<DD>, dim3(1), dim3(SEL1_THREADS), 0, s, dXt.as<double>(), n, \
                     dsc.as<double>(), n_select, diversity_weight, didx.as<int>(), comb)
    SEL_DISPATCH(d, ONE_CALL)
#undef ONE_CALL
    GPMPC_HIP(hipGetLastError());
  } else {
    GPMPC_HIP(dmind.alloc(s, sizeof(double) * (size_t)n));
    GPMPC_HIP(dtaken.alloc(s, (size_t)n));
    GPMPC_HIP(dpv.alloc(s, sizeof(double) * 2 * (size_t)nwg));
    GPMPC_HIP(dpi.alloc(s, sizeof(int) * 2 * (size_t)nwg));
    for (int t = 0; t <= n_select; ++t) {
      const int in = (t + 1) & 1, out = t & 1;  // launch t reads pick t-1's partials
      // the last launch only reduces (all nwg partials) and records: one workgroup
      const dim3 g(t == n_select ? 1u : (unsigned)nwg);
#define GRID_CALL(DD)                                                                          \
  hipLaunchKernelGGL(k_select_grid<DD>, g, dim3(SEL2_THREADS), 0, s, dXt.as<double>(), n,      \
                     dsc.as<double>(), t, n_select, nwg, diversity_weight, dmind.as<double>(), \
                     dtaken.as<unsigned char>(), dpv.as<double>() + (size_t)in * nwg,          \
                     dpi.as<int>() + (size_t)in * nwg, dpv.as<double>() + (size_t)out * nwg,   \
                     dpi.as<int>() + (size_t)out * nwg, didx.as<int>(), comb)
      SEL_DISPATCH(d, GRID_CALL)
#undef GRID_CALL
      GPMPC_HIP(hipGetLastError());
    }
  }
  GPMPC_HIP(hipMemcpyAsync(idx_out, didx.p, sizeof(int) * (size_t)n_select, hipMemcpyDeviceToHost, s));
  if (combined_out)
    GPMPC_HIP(hipMemcpyAsync(combined_out, dcomb.p, sizeof(double) * (size_t)n_select,
                             hipMemcpyDeviceToHost, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  GPMPC_CHECK_ARG(idx_out[n_select - 1] >= 0);  // a pick without a comparable value: NaN scores
  return 0;
}
