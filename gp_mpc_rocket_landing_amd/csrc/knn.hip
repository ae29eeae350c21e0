// knn.hip -- batched brute-force k-nearest-neighbour search over a resident set in fp64:
// the neighbours, ball counts and interpolated cost-to-go that the learning-MPC safe sets
// ask for (terminal/local_safe_set.py, terminal/q_function.py), DESIGN §17.
//
// Reference: LocalSafeSet.query / _compute_adaptive_K / interpolate_q (local_safe_set.py:
// 158-300: one scipy KDTree.query and one query_ball_point per state) and the brute-force
// neighbour search of InverseDistanceQFunction / LocalLinearQFunction (q_function.py:97-190).
//
// Contract per query: the k <= 64 smallest squared distances in ascending order with their
// row indices, equal distances by lower index (a total order); (inf, n) where fewer than k
// rows qualify; n_ball = qualifying rows with s^2 <= radius * radius (rounded once, rows at
// the radius counted); with avail_fuel, row i qualifies iff fuel_req[i] <= avail_fuel[b], and
// n_feasible counts them.  Distances are direct differences summed in a stated order
// (sqdist.h): order 0 the KD-tree's, order 1 numpy's; selection is on s^2 and the one
// correctly rounded square root goes on the survivors.
//
// Kernel shape.  Stored rows live in lanes (d features in registers, read from the
// feature-major copy made at create time, so consecutive lanes read consecutive doubles).  A
// wave serves Q queries at once (their vectors are wave-uniform), and each query's running
// list of 64 (s^2, index) pairs lies across the 64 lanes of one register pair: lane j holds
// the j-th smallest so far, lane 63 the admission threshold.  A row is inserted only when it
// beats the threshold: its position is a ballot + popcount of "precedes", the lanes above
// shift up by one.  The four waves of a workgroup scan disjoint 64-row chunks of the
// workgroup's part and merge their four lists through LDS by rank counting.  For small B and
// large n the rows are split over P parts (grid.y) and a second launch merges the P lists of
// a query; the order between the launches is the kernel boundary alone.
#include "internal.h"
#include "hull.h"
#include "sqdist.h"
#include <climits>
#include <cmath>

#pragma clang fp contract(off)

#define KNN_MAXD 32          // = GRAM_MAXD
#define KNN_MAXK 64          // the list: one entry a lane
#define KNN_THREADS 256
#define KNN_WAVES 4
#ifndef KNN_Q
#define KNN_Q 2              // queries a wave serves at once (docs/PERF_HISTORY.md); 1 when B = 1
#endif
#define KNN_PART_ROWS 1024   // at most one part per this many rows: no split up to it
#define KNN_MAX_PARTS 64     // the merge kernel's LDS: 64 lists of 64
#ifndef KNN_TARGET_WG
#define KNN_TARGET_WG 512    // split until the grid has two workgroups a CU
#endif
#define KNN_EMPTY INT_MAX    // index of an unused list entry (its s^2 is inf)

struct gpmpc_knn {
  gpmpc_ctx *ctx = nullptr;
  int n = 0, d = 0;
  DevBuf St, q, fuel;  // St: d x n feature-major; q, fuel: n or unallocated
  int dp = 0;
  DevBuf P;            // n x dp payload rows (gpmpc_knn_set_points), or unallocated
};

// (sa, ia) before (sb, ib) in the total order: by s^2, then by row index
__device__ __forceinline__ bool precedes(double sa, int ia, double sb, int ib) {
  return sa < sb || (sa == sb && ia < ib);
}

// how many entries of a sorted list of 64 precede (cs, ci)
__device__ __forceinline__ int count_preceding(const double *ls, const int *li, double cs, int ci) {
  int lo = 0, hi = KNN_MAXK;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (precedes(ls[mid], li[mid], cs, ci)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// lane j's value for every lane, j wave-uniform: v_readlane, no LDS crossbar
__device__ __forceinline__ int lane_get(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ double lane_get(double v, int j) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, j);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), j);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// lane i takes lane i - 1's value (lane 0 keeps its own): the DPP wave shift right by one
__device__ __forceinline__ int lane_up1(int v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ double lane_up1(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)lane_up1((int)(unsigned)b);
  const unsigned hi = (unsigned)lane_up1((int)(unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = add_rn(v, __shfl_xor(v, off, 64));
  return v;
}

// S (n x d row-major) -> St (d x n)
__global__ void k_knn_transpose(const double *__restrict__ S, int n, int d, double *__restrict__ St) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n * d) return;
  const int64_t i = e / d;
  const int k = (int)(e - i * d);
  St[(int64_t)k * n + i] = S[e];
}

// ---------------------------------------------------------------------------
// Workgroup (g, p): queries g*Q .. g*Q+Q-1 against rows [p*part_len, min(n, (p+1)*part_len)).
// out_s / out_i: [B][P][64] the part's sorted list; out_cnt: [B][P][2] ball and feasible counts.
template <int D, int ORDER, int Q>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_scan(
    const double *__restrict__ St, int n, const double *__restrict__ fuel, const double *__restrict__ Xq, int B,
    const double *__restrict__ avail, double r2, int part_len, double *__restrict__ out_s, int *__restrict__ out_i,
    int *__restrict__ out_cnt) {
  __shared__ double ls[Q][KNN_WAVES][KNN_MAXK];
  __shared__ int li[Q][KNN_WAVES][KNN_MAXK];
  __shared__ int lc[Q][KNN_WAVES][2];
  __shared__ double ms[Q][KNN_MAXK];
  __shared__ int mi[Q][KNN_MAXK];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b0 = blockIdx.x * Q, part = blockIdx.y, P = gridDim.y;
  const int64_t row0 = (int64_t)part * part_len;
  const int64_t row1 = row0 + part_len < n ? row0 + part_len : n;
  const bool filter = avail != nullptr;

  // the queries: wave-uniform (a query past B repeats the last one; nothing of it is written)
  double xq[Q][D], av[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int b = b0 + q < B ? b0 + q : B - 1;
#pragma unroll
    for (int k = 0; k < D; ++k) xq[q][k] = Xq[(int64_t)b * D + k];
    av[q] = filter ? avail[b] : 0.0;
  }
  double list_s[Q];
  int list_i[Q], cball[Q], cfeas[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    list_s[q] = INFINITY;
    list_i[q] = KNN_EMPTY;
    cball[q] = cfeas[q] = 0;
  }

  // wave wv takes chunks wv, wv + 4, ... of the part: ascending row indices, so a row never
  // precedes a list entry of equal s^2 and the admission test is the strict s^2 < threshold
  // the next chunk's rows are in flight while this one is scanned
  double rn[D], fn;
  auto load = [&](int64_t c, double (&row)[D], double &f) {
    const int64_t i = c + lane;
    const bool live = i < row1;
#pragma unroll
    for (int k = 0; k < D; ++k) row[k] = live ? St[(int64_t)k * n + i] : 0.0;
    f = filter && live ? fuel[i] : 0.0;
  };
  int64_t c0 = row0 + wv * 64;
  if (c0 < row1) load(c0, rn, fn);
  for (; c0 < row1; c0 += KNN_THREADS) {
    const bool live = c0 + lane < row1;
    double r[D];
#pragma unroll
    for (int k = 0; k < D; ++k) r[k] = rn[k];
    const double f = fn;
    if (c0 + KNN_THREADS < row1) load(c0 + KNN_THREADS, rn, fn);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      double s2;
      if constexpr (ORDER == 0) s2 = sqdist_kd<D>(xq[q], [&](int k) { return r[k]; });
      else s2 = sqdist<D>(xq[q], [&](int k) { return r[k]; });
      const bool ok = live && (!filter || f <= av[q]);
      cfeas[q] += ok ? 1 : 0;
      cball[q] += ok && s2 <= r2 ? 1 : 0;
      double thr = lane_get(list_s[q], 63);  // read by every lane: not behind ok's short circuit
      unsigned long long m = __ballot(ok && s2 < thr);
      while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        const double cs = lane_get(s2, j);
        const int ci = (int)(c0 + j);
        if (!(cs < thr)) continue;  // an earlier insert of this chunk raised the bar
        const int pos = __popcll(__ballot(precedes(list_s[q], list_i[q], cs, ci)));
        const double us = lane_up1(list_s[q]);
        const int ui = lane_up1(list_i[q]);
        if (lane > pos) {
          list_s[q] = us;
          list_i[q] = ui;
        } else if (lane == pos) {
          list_s[q] = cs;
          list_i[q] = ci;
        }
        thr = lane_get(list_s[q], 63);
      }
    }
  }

  // the four waves' lists and counts -> LDS; the merged list starts empty
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    ls[q][wv][lane] = list_s[q];
    li[q][wv][lane] = list_i[q];
    const int nb = wave_sum(cball[q]), nf = wave_sum(cfeas[q]);
    if (lane == 0) {
      lc[q][wv][0] = nb;
      lc[q][wv][1] = nf;
    }
    if (wv == 0) {
      ms[q][lane] = INFINITY;
      mi[q][lane] = KNN_EMPTY;
    }
  }
  __syncthreads();
  // rank counting: each of the 256 candidates counts its predecessors in the four sorted
  // lists (its own included: its position); distinct rows have distinct ranks
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const double cs = ls[q][wv][lane];
    const int ci = li[q][wv][lane];
    if (ci != KNN_EMPTY) {
      int rank = 0;
#pragma unroll
      for (int w = 0; w < KNN_WAVES; ++w) rank += count_preceding(ls[q][w], li[q][w], cs, ci);
      if (rank < KNN_MAXK) {
        ms[q][rank] = cs;
        mi[q][rank] = ci;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < Q * KNN_MAXK; e += KNN_THREADS) {
    const int q = e >> 6, j = e & 63;
    if (b0 + q < B) {
      const int64_t o = ((int64_t)(b0 + q) * P + part) * KNN_MAXK + j;
      out_s[o] = ms[q][j];
      out_i[o] = mi[q][j];
    }
  }
  if (tid < Q * 2) {
    const int q = tid >> 1, c = tid & 1;
    if (b0 + q < B) {
      int v = 0;
#pragma unroll
      for (int w = 0; w < KNN_WAVES; ++w) v += lc[q][w][c];
      out_cnt[((int64_t)(b0 + q) * P + part) * 2 + c] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// The P part lists of query blockIdx.x -> its one list (fin_s, fin_i: [B][64]) and counts
// (fin_cnt: [B][2]).  P <= KNN_MAX_PARTS.  A full list bounds the answer: its 64 entries precede
// every entry with a larger s^2, so only entries up to a bound `cut` on the answer's 64th
// entry can rank.  Those survivors (a few times 64 of the P * 64; all of them when the lists
// tie) are gathered in LDS, and each counts the survivors that precede it: its rank.
__global__ __launch_bounds__(KNN_THREADS) void k_knn_merge(const double *__restrict__ part_s,
                                                           const int *__restrict__ part_i,
                                                           const int *__restrict__ part_cnt, int P,
                                                           double *__restrict__ fin_s, int *__restrict__ fin_i,
                                                           int *__restrict__ fin_cnt) {
  __shared__ double ss[KNN_MAX_PARTS * KNN_MAXK];
  __shared__ int si[KNN_MAX_PARTS * KNN_MAXK];
  __shared__ double ms[KNN_MAXK];
  __shared__ int mi[KNN_MAXK];
  __shared__ double bound[KNN_MAXK];
  __shared__ int count;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int nc = P * KNN_MAXK;
  // Bounds on the 64th entry of the answer.  The lists ascend, so when `need` lists have an
  // entry at position j up to v, (j + 1) * need entries are up to v: with need = ceil(64 / (j + 1))
  // the need-th smallest of the lists' entries at position j bounds the answer, for every j
  // (j = 63: the smallest last entry; j = ceil(64 / P) - 1: the largest entry at that position).
  // `cut` is the smallest of the 64 bounds; thread (j, quarter) ranks a quarter of column j.
  for (int e = tid; e < nc; e += KNN_THREADS) ss[e] = part_s[b * nc + e];
  if (tid < KNN_MAXK) {
    bound[tid] = INFINITY;
    ms[tid] = INFINITY;
    mi[tid] = KNN_EMPTY;
  }
  if (tid == 0) count = 0;
  __syncthreads();
  {
    const int j = tid & 63, quarter = tid >> 6;
    const int need = (KNN_MAXK + j) / (j + 1);
    if (need <= P) {
      for (int p = quarter; p < P; p += KNN_WAVES) {
        const double v = ss[p * KNN_MAXK + j];
        int below = 0;
        for (int o = 0; o < P; ++o) {
          const double w = ss[o * KNN_MAXK + j];
          below += w < v || (w == v && o < p) ? 1 : 0;
        }
        if (below == need - 1) bound[j] = v;  // one p of the column has this rank
      }
    }
  }
  __syncthreads();
  double cut = INFINITY;
  for (int j = 0; j < KNN_MAXK; ++j) cut = bound[j] < cut ? bound[j] : cut;
  __syncthreads();  // ss and bound are read: the survivors may overwrite ss
  for (int e = tid; e < nc; e += KNN_THREADS) {
    const double cs = part_s[b * nc + e];
    const int ci = part_i[b * nc + e];
    if (ci != KNN_EMPTY && !(cs > cut)) {
      const int slot = atomicAdd(&count, 1);  // < nc: one slot an entry
      ss[slot] = cs;
      si[slot] = ci;
    }
  }
  __syncthreads();
  const int ns = count;
  for (int e = tid; e < ns; e += KNN_THREADS) {
    const double cs = ss[e];
    const int ci = si[e];
    int rank = 0;
    for (int o = 0; o < ns; ++o) rank += precedes(ss[o], si[o], cs, ci) ? 1 : 0;
    if (rank < KNN_MAXK) {
      ms[rank] = cs;
      mi[rank] = ci;
    }
  }
  __syncthreads();
  if (tid < KNN_MAXK) {
    fin_s[b * KNN_MAXK + tid] = ms[tid];
    fin_i[b * KNN_MAXK + tid] = mi[tid];
  }
  if (tid < 2) {
    int v = 0;
    for (int p = 0; p < P; ++p) v += part_cnt[(b * P + p) * 2 + tid];
    fin_cnt[b * 2 + tid] = v;
  }
}

// the query's outputs from the final lists: one wave a query
__global__ __launch_bounds__(64) void k_knn_emit(const double *__restrict__ fin_s, const int *__restrict__ fin_i,
                                                 const int *__restrict__ fin_cnt, int n, int k,
                                                 int *__restrict__ idx, double *__restrict__ dist,
                                                 int *__restrict__ n_ball, int *__restrict__ n_feas) {
  const int64_t b = blockIdx.x;
  const int j = threadIdx.x;
  if (j < k) {
    const int ci = fin_i[b * KNN_MAXK + j];
    idx[b * k + j] = ci == KNN_EMPTY ? n : ci;
    dist[b * k + j] = ci == KNN_EMPTY ? INFINITY : sqrt(fin_s[b * KNN_MAXK + j]);
  }
  if (j == 0) {
    n_ball[b] = fin_cnt[b * 2];
    n_feas[b] = fin_cnt[b * 2 + 1];
  }
}

// The K rule of LocalSafeSet.query (local_safe_set.py:182-213, 236-249) from a query's ball and
// available counts: K; 0 without a safe state; -1 where the reference raises (fewer available
// rows than K).  The one place it lives on the device (k_knn_interp, k_knn_hull_prep).
__device__ __forceinline__ int knn_k_rule(int nball, int navail, int k_base, int k_min, int k_max, int adaptive) {
  int K = k_base;
  if (navail > 0 && adaptive) {
    const double dens = (double)nball / (double)navail;
    K = (int)mul_rn((double)k_base, add_rn(1.0, mul_rn(dens, 2.0)));
    K = K < k_min ? k_min : K;
    K = K > k_max ? k_max : K;
  }
  K = K < navail ? K : navail;
  K = K > k_min ? K : k_min;
  K = K < k_max ? K : k_max;
  if (navail == 0 || K == 0) return 0;
  return K > navail ? -1 : K;
}

// LocalSafeSet.interpolate_q(method="inverse_distance") from the final lists: the K rule of
// LocalSafeSet.query (local_safe_set.py:182-213, 236-249) and the weighting (:279-287), one wave
// a query.  k_used = -1 (q_out NaN) where the reference raises (fewer available rows than K).
__global__ __launch_bounds__(64) void k_knn_interp(const double *__restrict__ fin_s, const int *__restrict__ fin_i,
                                                   const int *__restrict__ fin_cnt, const double *__restrict__ qv,
                                                   int k_base, int k_min, int k_max, int adaptive,
                                                   double *__restrict__ q_out, int *__restrict__ k_used) {
  const int64_t b = blockIdx.x;
  const int j = threadIdx.x;
  const int K = knn_k_rule(fin_cnt[b * 2], fin_cnt[b * 2 + 1], k_base, k_min, k_max, adaptive);
  if (K == 0) {  // no safe state: the reference returns inf
    if (j == 0) {
      q_out[b] = INFINITY;
      k_used[b] = 0;
    }
    return;
  }
  if (K < 0) {
    if (j == 0) {
      q_out[b] = NAN;
      k_used[b] = -1;
    }
    return;
  }
  const int ci = fin_i[b * KNN_MAXK + j];
  const bool in = j < K && ci != KNN_EMPTY;
  const double dj = in ? sqrt(fin_s[b * KNN_MAXK + j]) : INFINITY;
  const double qj = in ? qv[ci] : 0.0;
  const double d0 = __shfl(dj, 0, 64);
  double res;
  if (d0 < 1e-10) {
    res = __shfl(qj, 0, 64);
  } else {
    double w = in ? 1.0 / add_rn(dj, 1e-10) : 0.0;
    const double sum = wave_sum(w);
    w = w / sum;
    res = wave_sum(mul_rn(w, qj));
  }
  if (j == 0) {
    q_out[b] = res;
    k_used[b] = K;
  }
}

#define KNN_DISPATCH(d, CALL)                                                                 \
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
// The plan (no device): Q = KNN_Q queries a wave (1 for a single query).  The rows are split
// until the grid has KNN_TARGET_WG workgroups: at most one part per KNN_PART_ROWS rows (so no
// split up to that many) and at most KNN_MAX_PARTS; a part's length is a multiple of the
// workgroup's 256-row stride, the last part takes what is left.
static void knn_plan(int n, int B, int *parts, int *q_per_wave, int *part_len) {
  const int Q = B >= 2 ? KNN_Q : 1;
  const int64_t groups = ((int64_t)B + Q - 1) / Q;
  int64_t want = (KNN_TARGET_WG + groups - 1) / groups;
  const int64_t most = ((int64_t)n + KNN_PART_ROWS - 1) / KNN_PART_ROWS;
  if (want > most) want = most;
  if (want > KNN_MAX_PARTS) want = KNN_MAX_PARTS;
  if (want < 1) want = 1;
  const int64_t per = ((int64_t)n + want - 1) / want;
  const int64_t len = (per + KNN_THREADS - 1) / KNN_THREADS * KNN_THREADS;
  *parts = (int)(((int64_t)n + len - 1) / len);
  *q_per_wave = Q;
  *part_len = (int)(len < INT_MAX ? len : INT_MAX);
}

extern "C" int gpmpc_knn_plan(int n, int d, int B, int k, int *parts, int *q_per_wave) {
  GPMPC_CHECK_ARG(parts && q_per_wave);
  GPMPC_CHECK_ARG(n >= 1 && B >= 1);
  GPMPC_CHECK_ARG(d >= 1 && d <= KNN_MAXD);
  GPMPC_CHECK_ARG(k >= 1 && k <= KNN_MAXK);
  int len;
  knn_plan(n, B, parts, q_per_wave, &len);
  return 0;
}

// ---------------------------------------------------------------------------
extern "C" int gpmpc_knn_create(gpmpc_ctx *ctx, const double *S, int n, int d, const double *q,
                                const double *fuel_req, gpmpc_knn **out) {
  GPMPC_CHECK_ARG(ctx && S && out);
  GPMPC_CHECK_ARG(n >= 1);
  GPMPC_CHECK_ARG(d >= 1 && d <= KNN_MAXD);
  GPMPC_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  gpmpc_knn *h = new gpmpc_knn;
  h->ctx = ctx;
  h->n = n;
  h->d = d;
  const size_t nd = (size_t)n * d;
  DevBuf dS;
  hipError_t e = dS.alloc(s, sizeof(double) * nd);
  if (e == hipSuccess) e = h->St.alloc(sizeof(double) * nd);
  if (e == hipSuccess && q) e = h->q.alloc(sizeof(double) * (size_t)n);
  if (e == hipSuccess && fuel_req) e = h->fuel.alloc(sizeof(double) * (size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(dS.p, S, sizeof(double) * nd, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && q) e = hipMemcpyAsync(h->q.p, q, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && fuel_req)
    e = hipMemcpyAsync(h->fuel.p, fuel_req, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_knn_transpose, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s, dS.as<double>(), n, d,
                       h->St.as<double>());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    delete h;
    gpmpc_set_error("knn_create: %s", hipGetErrorString(e));
    return -1;
  }
  *out = h;
  return 0;
}

extern "C" int gpmpc_knn_destroy(gpmpc_knn *set) {
  if (!set) return 0;
  delete set;  // its buffers are its own hipMalloc: hipFree waits for the device (every call also ends drained)
  return 0;
}

// the scan (and, for P > 1, the merge) of B staged queries: final lists and counts
struct KnnFinal {
  DevBuf ps, pi, pc, fs, fi, fc;  // part buffers (P > 1) and final buffers
  const double *s = nullptr;
  const int *i = nullptr, *cnt = nullptr;
};

static int knn_search(gpmpc_knn *set, int order, const double *dXq, int B, const double *davail, double radius,
                      KnnFinal &f) {
  hipStream_t s = set->ctx->stream;
  const int n = set->n, d = set->d;
  int P = 1, Q = 1, part_len = 0;
  knn_plan(n, B, &P, &Q, &part_len);
  const size_t lists = (size_t)B * P * KNN_MAXK;
  DevBuf &os = P > 1 ? f.ps : f.fs, &oi = P > 1 ? f.pi : f.fi, &oc = P > 1 ? f.pc : f.fc;
  GPMPC_HIP(os.alloc(s, sizeof(double) * lists));
  GPMPC_HIP(oi.alloc(s, sizeof(int) * lists));
  GPMPC_HIP(oc.alloc(s, sizeof(int) * (size_t)B * P * 2));
  const double r2 = radius * radius;  // rounded once
  const dim3 grid((unsigned)(((int64_t)B + Q - 1) / Q), (unsigned)P);
#define SCAN_CALL_OQ(DD, OO, QQ)                                                                         \
  hipLaunchKernelGGL((k_knn_scan<DD, OO, QQ>), grid, dim3(KNN_THREADS), 0, s, set->St.as<double>(), n,   \
                     set->fuel.as<double>(), dXq, B, davail, r2, part_len, os.as<double>(), oi.as<int>(), \
                     oc.as<int>())
#define SCAN_CALL(DD)                                  \
  do {                                                 \
    if (order == 0 && Q == 1) SCAN_CALL_OQ(DD, 0, 1);  \
    else if (order == 0) SCAN_CALL_OQ(DD, 0, KNN_Q);   \
    else if (Q == 1) SCAN_CALL_OQ(DD, 1, 1);           \
    else SCAN_CALL_OQ(DD, 1, KNN_Q);                   \
  } while (0)
  KNN_DISPATCH(d, SCAN_CALL)
#undef SCAN_CALL
#undef SCAN_CALL_OQ
  GPMPC_HIP(hipGetLastError());
  if (P > 1) {
    GPMPC_HIP(f.fs.alloc(s, sizeof(double) * (size_t)B * KNN_MAXK));
    GPMPC_HIP(f.fi.alloc(s, sizeof(int) * (size_t)B * KNN_MAXK));
    GPMPC_HIP(f.fc.alloc(s, sizeof(int) * (size_t)B * 2));
    hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)B), dim3(KNN_THREADS), 0, s, f.ps.as<double>(), f.pi.as<int>(),
                       f.pc.as<int>(), P, f.fs.as<double>(), f.fi.as<int>(), f.fc.as<int>());
    GPMPC_HIP(hipGetLastError());
  }
  f.s = f.fs.as<double>();
  f.i = f.fi.as<int>();
  f.cnt = f.fc.as<int>();
  return 0;
}

static int knn_check_call(const gpmpc_knn *set, int order, const double *Xq, int B, double radius,
                          const double *avail_fuel) {
  GPMPC_CHECK_ARG(set && set->ctx);
  GPMPC_CHECK_ARG(order == 0 || order == 1);
  GPMPC_CHECK_ARG(B >= 0 && (Xq || B == 0));
  GPMPC_CHECK_ARG(radius >= 0.0);
  if (avail_fuel && !set->fuel.p) {
    gpmpc_set_error("knn: avail_fuel given, but the set was created without fuel_req");
    return -2;
  }
  return 0;
}

extern "C" int gpmpc_knn_query(gpmpc_knn *set, int order, const double *Xq, int B, int k, double radius,
                               const double *avail_fuel, int *idx, double *dist, int *n_ball, int *n_feasible) {
  if (int rc = knn_check_call(set, order, Xq, B, radius, avail_fuel)) return rc;
  GPMPC_CHECK_ARG(k >= 1 && k <= KNN_MAXK);
  GPMPC_CHECK_ARG(B == 0 || (idx && dist && n_ball && n_feasible));
  if (B == 0) return 0;
  GPMPC_HIP(hipSetDevice(set->ctx->device));
  hipStream_t s = set->ctx->stream;
  const size_t nb = (size_t)B, d = (size_t)set->d;
  Stage sg(s);
  const double *dXq, *dav;  // dav null without avail_fuel
  int *didx, *dball, *dfeas;
  double *ddist;
  sg.in(&dXq, Xq, nb * d);
  sg.in(&dav, avail_fuel, nb);
  sg.out(&didx, idx, nb * k);
  sg.out(&ddist, dist, nb * k);
  sg.out(&dball, n_ball, nb); sg.out(&dfeas, n_feasible, nb);
  if (int rc = sg.commit("knn_query")) return rc;
  KnnFinal f;
  if (int rc = knn_search(set, order, dXq, B, dav, radius, f)) return rc;
  hipLaunchKernelGGL(k_knn_emit, dim3((unsigned)B), dim3(64), 0, s, f.s, f.i, f.cnt, set->n, k, didx, ddist, dball,
                     dfeas);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}

extern "C" int gpmpc_knn_interp(gpmpc_knn *set, int order, const double *Xq, int B, int k_base, int k_min,
                                int k_max, int adaptive, double radius, const double *avail_fuel, double *q_out,
                                int *k_used) {
  if (int rc = knn_check_call(set, order, Xq, B, radius, avail_fuel)) return rc;
  GPMPC_CHECK_ARG(k_base >= 1 && k_min >= 0 && k_min <= k_max && k_max >= 1 && k_max <= KNN_MAXK);
  GPMPC_CHECK_ARG(B == 0 || (q_out && k_used));
  if (!set->q.p) {
    gpmpc_set_error("knn_interp: the set was created without q");
    return -2;
  }
  if (B == 0) return 0;
  GPMPC_HIP(hipSetDevice(set->ctx->device));
  hipStream_t s = set->ctx->stream;
  const size_t nb = (size_t)B, d = (size_t)set->d;
  Stage sg(s);
  const double *dXq, *dav;  // dav null without avail_fuel
  double *dq;
  int *dk;
  sg.in(&dXq, Xq, nb * d);
  sg.in(&dav, avail_fuel, nb);
  sg.out(&dq, q_out, nb);
  sg.out(&dk, k_used, nb);
  if (int rc = sg.commit("knn_interp")) return rc;
  KnnFinal f;
  if (int rc = knn_search(set, order, dXq, B, dav, radius, f)) return rc;
  hipLaunchKernelGGL(k_knn_interp, dim3((unsigned)B), dim3(64), 0, s, f.s, f.i, f.cnt, set->q.as<double>(), k_base,
                     k_min, k_max, adaptive, dq, dk);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(sg.download());
  return 0;
}

// ---------------------------------------------------------------------------
// The vertex sets of the fused hull call from the final lists: the K rule, then the K nearest
// row indices, nearest first (idx: [B][k_max], n past K), nv = K (0 where k_used is 0 or -1).
__global__ __launch_bounds__(64) void k_knn_hull_prep(const int *__restrict__ fin_i, const int *__restrict__ fin_cnt,
                                                      int n, int k_base, int k_min, int k_max, int adaptive,
                                                      int *__restrict__ idx, int *__restrict__ nv,
                                                      int *__restrict__ k_used) {
  const int64_t b = blockIdx.x;
  const int j = threadIdx.x;
  const int K = knn_k_rule(fin_cnt[b * 2], fin_cnt[b * 2 + 1], k_base, k_min, k_max, adaptive);
  const int used = K > 0 ? K : 0;
  if (j < k_max) idx[b * k_max + j] = j < used ? fin_i[b * KNN_MAXK + j] : n;
  if (j == 0) {
    nv[b] = used;
    k_used[b] = K;
  }
}

extern "C" int gpmpc_knn_set_points(gpmpc_knn *set, const double *P, int dp) {
  GPMPC_CHECK_ARG(set && set->ctx && P);
  GPMPC_CHECK_ARG(dp >= 1 && dp <= HULL_MAXD);
  GPMPC_HIP(hipSetDevice(set->ctx->device));
  hipStream_t s = set->ctx->stream;
  const size_t bytes = sizeof(double) * (size_t)set->n * dp;
  set->dp = 0;
  GPMPC_HIP(set->P.alloc(bytes));
  GPMPC_HIP(hipMemcpyAsync(set->P.p, P, bytes, hipMemcpyHostToDevice, s));
  GPMPC_HIP(hipStreamSynchronize(s));
  set->dp = dp;
  return 0;
}

extern "C" int gpmpc_knn_hull(gpmpc_knn *set, int order, const double *Xq, const double *Xp, int B, int k_base,
                              int k_min, int k_max, int adaptive, double radius, const double *avail_fuel,
                              double tol, int max_iter, int *k_used, int *idx, double *lambda, double *proj,
                              double *dist, double *gap, double *qhull, int *iters, int *status) {
  if (int rc = knn_check_call(set, order, Xq, B, radius, avail_fuel)) return rc;
  GPMPC_CHECK_ARG(k_base >= 1 && k_min >= 0 && k_min <= k_max && k_max >= 1 && k_max <= KNN_MAXK);
  GPMPC_CHECK_ARG(tol > 0.0 && tol < INFINITY);
  GPMPC_CHECK_ARG(max_iter >= 1 && max_iter <= HULL_MAX_ITER);
  GPMPC_CHECK_ARG(B == 0 || (Xp && k_used && idx && lambda && proj && dist && gap && iters && status));
  if (!set->dp) {
    gpmpc_set_error("knn_hull: the set has no payload rows (gpmpc_knn_set_points)");
    return -2;
  }
  if (B == 0) return 0;
  GPMPC_HIP(hipSetDevice(set->ctx->device));
  hipStream_t s = set->ctx->stream;
  const size_t nb = (size_t)B, d = (size_t)set->d, dp = (size_t)set->dp, km = (size_t)k_max;
  const bool with_q = set->q.p && qhull;
  DevBuf nvbuf;  // the vertex counts stay on the device
  GPMPC_HIP(nvbuf.alloc(s, sizeof(int) * nb));
  int *dnv = nvbuf.as<int>();
  HullArgs a{};
  a.V = set->P.as<double>();
  a.q = with_q ? set->q.as<double>() : nullptr;
  a.nv = dnv;
  a.B = B;
  a.kmax = k_max;
  a.d = set->dp;
  a.shared = 0;
  a.tol = tol;
  a.max_iter = max_iter;
  Stage sg(s);
  const double *dXq, *dav;  // dav null without avail_fuel
  int *dused, *didx;
  sg.in(&dXq, Xq, nb * d);
  sg.in(&a.X, Xp, nb * dp);
  sg.in(&dav, avail_fuel, nb);
  sg.out(&dused, k_used, nb);
  sg.out(&didx, idx, nb * km);
  sg.out(&a.lambda, lambda, nb * km);
  sg.out(&a.proj, proj, nb * dp);
  sg.out(&a.dist, dist, nb);
  sg.out(&a.gap, gap, nb);
  sg.out(&a.qhull, with_q ? qhull : nullptr, nb);  // (written when a.q is given)
  sg.out(&a.iters, iters, nb);
  sg.out(&a.status, status, nb);
  if (int rc = sg.commit("knn_hull")) return rc;
  a.gidx = didx;
  KnnFinal f;
  if (int rc = knn_search(set, order, dXq, B, dav, radius, f)) return rc;
  hipLaunchKernelGGL(k_knn_hull_prep, dim3((unsigned)B), dim3(64), 0, s, f.i, f.cnt, set->n, k_base, k_min, k_max,
                     adaptive, didx, dnv, dused);
  GPMPC_HIP(hipGetLastError());
  GPMPC_HIP(launch_hull(s, a));
  GPMPC_HIP(sg.download());
  return 0;
}
