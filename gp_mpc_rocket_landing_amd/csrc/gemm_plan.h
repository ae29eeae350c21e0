// gemm_plan.h -- the dispatch of the GEMM launchers (gemm.hip) without a launch in it: the
// resolved switches (GemmPolicy) and, for one product, the kernel path, K split, grid and
// kernel mapping arguments it gets (gemm_plan).  The launchers execute the plan; the paths
// sum in different orders, so the plan decides a product's bits, and its tile height is what
// the SUMSQ consumers size their partial buffer by (gemm_sumsq_kind, gemm_row_tiles).  The
// GEMM thresholds live here and nowhere else.  Host-only and free of HIP types, so a plain
// C++17 compiler accepts it and gpmpc_gemm_plan reports the plan without a device.
#pragma once
#include <cstdint>
#include "../../include/gpmpc.h"

int gpmpc_env_int(const char *name, int dflt);  // internal.h
constexpr int GEMM_GT = 64, GEMM_GK = 16, GEMM_BT = 128;  // GT, GK of gemm.hip, BT of mma128.h

// The switches, in the order of gpmpc_gemm_plan's policy argument (GPMPC_GEMM_POLICY_N ints).
// Three-state switches keep their "auto" value (-1, or 0 for ksplit).
struct GemmPolicy {
  int big = 1;           // GPMPC_GEMM128: 0 = never the 128-tile kernels (but a forced SUMSQ kind)
  int kmin = 256;        // GPMPC_GEMM128_KMIN: the shortest K that takes 128-tiles
  int splitk = 1;        // GPMPC_SPLITK: 0 = skinny products on the one-pass 64-tile kernel
  int syrk128 = -1;      // GPMPC_SYRK128: 128-tiles for a lower-triangular square C (auto: by fill or K)
  int streamk = -1;      // GPMPC_STREAMK: stream-K for accumulations on big tiles (auto: by size)
  int ksplit = 0;        // GPMPC_KSPLIT: > 0 = that K split of the 128-tile kernel (0: the cost model)
  int remap = 0;         // GPMPC_GEMM_REMAP: the 64-tile kernel's 1-D XCD-aware order
  int xcd_batch = 1;     // GPMPC_XCD_BATCH: 0 = a lower-triangular batch on the plain triangular grid
  int rowblock_xcd = 1;  // GPMPC_ROWBLOCK_XCD: 0 = the row-block form's plain grid
  int post_xcd = 0;      // GPMPC_POST_XCD: the 128-tile SUMSQ kernel's column-grouped XCD mapping
};

// This process's switches, read once.
inline const GemmPolicy &gemm_policy_env() {
  static const GemmPolicy once = [] {
    GemmPolicy p;
    p.big = gpmpc_env_int("GPMPC_GEMM128", 1);
    p.kmin = gpmpc_env_int("GPMPC_GEMM128_KMIN", 2 * GEMM_BT);
    p.splitk = gpmpc_env_int("GPMPC_SPLITK", 1);
    p.syrk128 = gpmpc_env_int("GPMPC_SYRK128", -1);
    p.streamk = gpmpc_env_int("GPMPC_STREAMK", -1);
    p.ksplit = gpmpc_env_int("GPMPC_KSPLIT", 0);
    p.remap = gpmpc_env_int("GPMPC_GEMM_REMAP", 0);
    p.xcd_batch = gpmpc_env_int("GPMPC_XCD_BATCH", 1);
    p.rowblock_xcd = gpmpc_env_int("GPMPC_ROWBLOCK_XCD", 1);
    p.post_xcd = gpmpc_env_int("GPMPC_POST_XCD", 0);
    return p;
  }();
  return once;
}

// One product as a launcher sees it.  op: the launcher, a GPMPC_GEMM_OP_* that has a
// decision (NT, NN, NN_BATCHED, TN, ROWBLOCK, SUMSQ; SUMSQ_MEAN is SUMSQ with the mean rows
// counted in M).  M x N is C (the SUMSQ product's rows x columns), K the summed extent.
struct GemmRequest {
  int op, M, N, K, batch;
  bool beta1;               // beta == 1.0: the product accumulates into C
  int tri_a, lower_c;       // NT / SUMSQ
  int kind = -1;            // SUMSQ, batch 1: the forced GEMM_SUMSQ_* kind (-1: by size)
  int ksplit = 1;           // ROWBLOCK: the caller's K split
  bool no_scratch = false;  // the split-K partial buffer is not to be had: plan without it
};

// What the launcher does.  The first GPMPC_GEMM_PLAN_INTS ints are what gpmpc_gemm_plan
// reports: path, split, grid are the triple gpmpc_gemm_diag reports (split: the chunks S of
// the skinny splits, the workgroups of stream-K); gx, gy, gz the launch grid (of the split
// forms: of the partial products' launch); tile the tile height; kc the skinny splits' chunk.
constexpr int GEMM_PATH_NONE = -1;  // an empty product: nothing is launched
struct GemmPlan {
  int path = GEMM_PATH_NONE, split = 0, grid = GPMPC_GEMM_GRID_2D, gx = 0, gy = 0, gz = 0, tile = GEMM_GT, kc = 0;
  // the kernels' mapping arguments: k_gemm_nt's remap_ty and xcd_batch, k_gemm128's tri_grid
  // (0 the 2-D grid, 1 triangular, 2 column-grouped XCDs, 3 a matrix's row blocks on one XCD)
  int rt = 0, xb = 0, tg = 0;
  int tx = 0, T = 0;  // stream-K: tile columns, tiles per matrix, K steps over all tiles
  int64_t total = 0;
};

// The chunk count S (and length kc, a multiple of GK) of a skinny product's K split over
// `tiles` 64-tiles: chunks of >= 64 of K that fill 512 workgroups; 0 = one pass.
inline int gemm_skinny_split(int K, int tiles, int &kc) {
  if (K < 256) return 0;
  const int S = 512 / tiles < K / 64 ? 512 / tiles : K / 64;
  if (S < 2) return 0;
  kc = ((K + S - 1) / S + GEMM_GK - 1) / GEMM_GK * GEMM_GK;
  return (K + kc - 1) / kc;
}

inline GemmPlan gemm_plan(const GemmPolicy &p, const GemmRequest &r) {
  constexpr int GT = GEMM_GT, GK = GEMM_GK, BT = GEMM_BT;
  const int M = r.M, N = r.N, K = r.K, batch = r.batch;
  GemmPlan q;
  if (M <= 0 || N <= 0 || (r.op == GPMPC_GEMM_OP_NN_BATCHED && batch <= 0)) return q;
  const bool store = r.op != GPMPC_GEMM_OP_SUMSQ && r.op != GPMPC_GEMM_OP_SUMSQ_MEAN;
  auto set = [&](int path, int split, int grid, int gx, int gy, int gz, int tile) {
    q.path = path, q.split = split, q.grid = grid, q.gx = gx, q.gy = gy, q.gz = gz, q.tile = tile;
  };
  const int tx64 = (N + GT - 1) / GT, ty64 = (M + GT - 1) / GT;

  if (r.op == GPMPC_GEMM_OP_ROWBLOCK) {
    // split K (partial products added atomically): only with beta = 1 and C apart from A, B
    const int ks = (r.ksplit < 1 || !r.beta1) ? 1 : r.ksplit;
    // a batch of >= 8 matrices (a multiple of 8): each matrix's row tiles on one XCD
    q.tg = (p.rowblock_xcd && batch >= 8 && batch % 8 == 0) ? 3 : 0;
    set(ks > 1 ? GPMPC_GEMM_PATH_128_KSPLIT : GPMPC_GEMM_PATH_128, ks,
        q.tg ? GPMPC_GEMM_GRID_ROWBLOCK_XCD : GPMPC_GEMM_GRID_2D, 1, (M + BT - 1) / BT, batch * ks, BT);
    return q;
  }
  // Skinny products (M or N <= 32) with a long K -- the GEMVs of alpha = W^T (W y), the
  // append's B^T = K21 W^T, S -= B^T B: on the 64-tile kernel they were a few workgroups
  // each walking K / 16 dependent steps (70-90 us at K = 1000).  K is cut into S chunks
  // whose partial products go to scratch as a batch of the 64-tile kernel, then summed in
  // chunk order (deterministic; the sums run in another order than the one-pass product).
  auto skinny_store = [&] {
    if (!p.splitk || r.no_scratch || !(M <= 32 || N <= 32)) return false;
    const int S = gemm_skinny_split(K, tx64 * ty64, q.kc);
    if (S) set(GPMPC_GEMM_PATH_SPLITK, S, GPMPC_GEMM_GRID_2D, tx64, ty64, S, GT);
    return S != 0;
  };
  if (r.op == GPMPC_GEMM_OP_NN || r.op == GPMPC_GEMM_OP_TN || r.op == GPMPC_GEMM_OP_NN_BATCHED) {
    if (r.op == GPMPC_GEMM_OP_NN_BATCHED || !skinny_store())
      set(GPMPC_GEMM_PATH_64, 1, GPMPC_GEMM_GRID_2D, tx64, ty64, r.op == GPMPC_GEMM_OP_NN_BATCHED ? batch : 1, GT);
    return q;
  }

  // ---- NT and SUMSQ ----
  // a forced kind (SUMSQ, batch 1): that kernel, whatever the size (gemm_sumsq_kind)
  const int kind = (store || batch != 1) ? -1 : r.kind;
  const bool tg = r.lower_c && M == N && !r.tri_a;
  const int tx = (N + BT - 1) / BT, ty = (M + BT - 1) / BT;
  const int grid = tg ? GPMPC_GEMM_GRID_TRI : GPMPC_GEMM_GRID_2D;
  // stream-K for long accumulations into C on big tiles: measured 2000^2 x 4000
  // 60% (split-K 55%), 4000^2 x 4000 72%, 16 x 1000^2 x 1000 56% (64-tiles 52%);
  // smaller or shorter products (n ~ 500, K <= 256) keep the tiled kernels
  const bool sk_ok = store && r.beta1 && !r.tri_a && M >= 2 * BT && N >= 2 * BT && K >= 2 * BT;
  const bool sk_auto = M >= 768 && N >= 768 && K >= 512;
  if (sk_ok && (p.streamk >= 0 ? p.streamk > 0 : sk_auto)) {
    q.tx = tx, q.T = tg ? ty * (ty + 1) / 2 : tx * ty, q.tg = (int)tg;
    q.total = (int64_t)q.T * batch * ((K + GK - 1) / GK);
    const int nwg = (int)(q.total < 512 ? q.total : 512);
    set(GPMPC_GEMM_PATH_STREAMK, nwg, grid, nwg, 1, 1, BT);
    return q;
  }
  // a lower-triangular batch takes 128-tiles only when they fill >= 2 rounds
  // of 512 resident workgroups or K is long enough to split; otherwise they
  // quantise badly (1.1-1.25 rounds: 21-36% vs 44-50% for 64-tiles).  FITC
  // 2000 x 4000: 128-tiles + split-K 56% vs 39%
  const int t128 = ty * (ty + 1) / 2 * batch;
  const bool tri_ok = !tg || (p.syrk128 >= 0 ? p.syrk128 != 0 : t128 >= 1024 || K >= 1024);
  const bool fits128 = p.big && M >= 2 * BT && N >= 2 * BT && K >= p.kmin;
  if (kind >= 0 ? kind == 1 /* GEMM_SUMSQ_128 */ : fits128 && tri_ok) {
    // split K when the tiles cannot give each CU ~4 workgroups to interleave (STORE
    // with beta = 1: partial products are added atomically); >= 512 of K per split
    const int tiles = (r.lower_c ? ty * (ty + 1) / 2 : tx * ty) * batch;
    // cost model: rounds of 512 resident workgroups (2 per CU) x (K per split
    // + ~256 of fixed cost: prologue, atomic C update).  Measured on 2000^2 x
    // 4000: ks 1/2/3/4/6/8 -> 30/38/53/43/49/45% (ks 4 leaves a 32-WG tail)
    int ksplit = 1;
    if (store && r.beta1 && K >= 1024) {
      double best = 1e30;
      for (int ks = 1; ks <= K / 256 && ks <= 16; ++ks) {
        const double c = (double)((tiles * ks + 511) / 512) * ((double)K / ks + 256.0);
        if (c < best * 0.98) best = c, ksplit = ks;
      }
    }
    if (p.ksplit > 0 && store && r.beta1) ksplit = p.ksplit;
    // lower-triangular square products launch only their lower tiles, in a
    // 1-D order that interleaves them over the 8 XCDs (a 2-D grid whose
    // column count is a multiple of 8 pins columns to XCDs: 8x imbalance).
    // The SUMSQ kernel takes the column-grouped XCD mapping instead (reported as 2-D)
    q.tg = store ? (int)tg : (p.post_xcd && batch == 1 && tx % 8 == 0) ? 2 : 0;
    set(ksplit > 1 ? GPMPC_GEMM_PATH_128_KSPLIT : GPMPC_GEMM_PATH_128, ksplit, grid, tg ? ty * (ty + 1) / 2 : tx,
        tg ? 1 : ty, batch * ksplit, BT);
    return q;
  }
  if (store && batch == 1 && !r.tri_a && !r.lower_c && skinny_store()) return q;
  // The SUMSQ form of the same split for few columns (the posterior of one landing's 20
  // queries, a predict of a few points), in the 64-tile SUMSQ kernel's output layout
  // (a triangular A's zero chunks are multiplied: the split is latency work)
  if (!store && batch == 1 && (kind >= 0 ? kind == 2 /* GEMM_SUMSQ_SPLITK */ : !fits128) && p.splitk &&
      !r.no_scratch && N <= GT) {
    const int S = gemm_skinny_split(K, ty64, q.kc);
    if (S) {
      set(GPMPC_GEMM_PATH_SPLITK, S, GPMPC_GEMM_GRID_2D, 1, ty64, S, GT);
      return q;
    }
  }
  // 64-tiles.  remap (off: measured slower for the posterior GEMM, W blocks thrash)
  const bool remap = p.remap && batch == 1 && ty64 > 1 && tx64 % 8 == 0;
  const int T = ty64 * (ty64 + 1) / 2;
  q.xb = (tg && p.xcd_batch && batch >= 8) ? batch : 0;
  q.rt = tg ? -1 : remap ? ty64 : 0;
  if (q.xb) set(GPMPC_GEMM_PATH_64, 1, GPMPC_GEMM_GRID_XCD_BATCH, T * ((batch + 7) / 8) * 8, 1, 1, GT);
  else if (tg) set(GPMPC_GEMM_PATH_64, 1, GPMPC_GEMM_GRID_TRI, T, 1, batch, GT);
  else if (remap) set(GPMPC_GEMM_PATH_64, 1, GPMPC_GEMM_GRID_2D, tx64 * ty64, 1, 1, GT);
  else set(GPMPC_GEMM_PATH_64, 1, GPMPC_GEMM_GRID_2D, tx64, ty64, batch, GT);
  return q;
}
