// potrf_plan.h -- the policy of the batched Cholesky (launch_potrf_batched, chol.hip) without
// a launch in it: the resolved switches (PotrfPolicy) and, for the 128-column form, the
// sequence of launches for (n, batch) (potrf_plan).  Host-only and free of HIP types, so a
// plain C++17 compiler accepts it and gpmpc_potrf_plan reports the plan without a device.
#pragma once
#include <climits>
#include "../../include/gpmpc.h"

int gpmpc_env_int(const char *name, int dflt);  // internal.h
constexpr int POTRF_DB = 128;                   // column block (DB of chol.hip)

// The switches, in the order of gpmpc_potrf_plan's policy argument (GPMPC_POTRF_POLICY_N ints).
// Three-state switches keep their "auto" value (-1, or 0 for ob / fuse_min).
struct PotrfPolicy {
  int p128 = 1;       // GPMPC_POTRF128: 0 = the 32-column driver
  int persist = 0;    // GPMPC_POTRF_PERSIST: > 0 = one workgroup per matrix (k_potrf_persist)
  int lat = -1;       // GPMPC_POTRF_LAT: latency-form panel solve and trailing SYRK (auto: batch <= 16)
  int sweep = 1;      // GPMPC_DIAG_SWEEP: the diagonal kernel's column sweep, 0 = per-block inverse form
  int trsm = -1;      // GPMPC_POTRF_TRSM: TRSM-form panel solve (auto: batch <= 64)
  int pk = -1;        // GPMPC_DIAG_PK: the diagonal kernel on the packed lower layout (auto: batch > 256)
  int ob = 0;         // GPMPC_POTRF_OB: outer panel, a multiple of 128 in 128..1024 (0: auto)
  int ksplit = 0;     // GPMPC_POTRF_KSPLIT: 1 = never split K
  int fuse = 1;       // GPMPC_POTRF_FUSE: fused update + panel solve
  int la = 0;         // GPMPC_POTRF_LA: look-ahead diagonal update inside the fused step
  int syrk_diag = 1;  // GPMPC_SYRK_DIAG: the balanced diagonal-block update
  int fuse_min = 0;   // GPMPC_POTRF_FUSE_MIN: workgroups below a block column for it to fuse (0: 512)
  int stamps = 0;     // GPMPC_DIAG128_STAMPS: phase cycles to stderr (a diagnostic)
};

// This process's switches: read once, except persist (read per call, tests switch it).
inline PotrfPolicy potrf_policy_env() {
  static const PotrfPolicy once = [] {
    PotrfPolicy p;
    p.p128 = gpmpc_env_int("GPMPC_POTRF128", 1);
    p.lat = gpmpc_env_int("GPMPC_POTRF_LAT", -1);
    p.sweep = gpmpc_env_int("GPMPC_DIAG_SWEEP", 1);
    p.trsm = gpmpc_env_int("GPMPC_POTRF_TRSM", -1);
    p.pk = gpmpc_env_int("GPMPC_DIAG_PK", -1);
    const int ob = gpmpc_env_int("GPMPC_POTRF_OB", INT_MIN), m = ob / POTRF_DB;
    p.ob = ob == INT_MIN ? 0 : POTRF_DB * (m < 1 ? 1 : m > 8 ? 8 : m);
    p.ksplit = gpmpc_env_int("GPMPC_POTRF_KSPLIT", 0);
    p.fuse = gpmpc_env_int("GPMPC_POTRF_FUSE", 1);
    p.la = gpmpc_env_int("GPMPC_POTRF_LA", 0);
    p.syrk_diag = gpmpc_env_int("GPMPC_SYRK_DIAG", 1);
    p.fuse_min = gpmpc_env_int("GPMPC_POTRF_FUSE_MIN", 0);
    p.stamps = gpmpc_env_int("GPMPC_DIAG128_STAMPS", 0);
    return p;
  }();
  PotrfPolicy p = once;
  p.persist = gpmpc_env_int("GPMPC_POTRF_PERSIST", 0);
  return p;
}

// the three drivers of launch_potrf_batched
enum { POTRF_FORM_32 = 0, POTRF_FORM_PERSIST = 1, POTRF_FORM_128 = 2 };
// One workgroup per matrix is off by default: measured 3.67 ms per round of <= 256 matrices
// of n = 1000 (20.8% of FP64 peak at batch 256) against 3.9 ms (28%) for the
// launch-per-panel path -- one wave per SIMD (130 KB of LDS per workgroup) leaves the MFMA
// tile loop's LDS and barrier latency exposed, and the diagonal chain idles the CU.
inline int potrf_form(const PotrfPolicy &p) {
  return !p.p128 ? POTRF_FORM_32 : p.persist > 0 ? POTRF_FORM_PERSIST : POTRF_FORM_128;
}

// One launch of the 128-column driver.  c: the step's first column (a TRAIL_*: the first
// trailing column t0); K0: the outer panel's first column; a: the integers of its kind.
// The executor forms every address from c and K0.
enum PotrfStepKind {  // (the values gpmpc_potrf_plan reports)
  POTRF_DIAG = GPMPC_POTRF_DIAG,  // k_potrf_diag128 at c: a = {w, pk, mode = sweep | (tblk ? 2 : 0), Linv written}
  POTRF_UPD_SYRK_DIAG = GPMPC_POTRF_UPD_SYRK_DIAG,  // launch_syrk128_diag, the diagonal block alone: a = {w, K, ks}
  POTRF_UPD_ROWBLOCK = GPMPC_POTRF_UPD_ROWBLOCK,    // launch_gemm_nt_rowblock, lower_c = 1: a = {rows, w, K, ks}
  POTRF_UPDSOLVE = GPMPC_POTRF_UPDSOLVE,  // launch_gemm_updsolve over the rows below c + 128: a = {below, K, wn}
  POTRF_PSOLVE_TRSM = GPMPC_POTRF_PSOLVE_TRSM,  // k_potrf_psolve_lat: a = {rows}, the rows below c + 128
  POTRF_PSOLVE_LAT = GPMPC_POTRF_PSOLVE_LAT,    // launch_gemm_lat mode 0, in place: a = {rows}
  POTRF_PSOLVE_ROWBLOCK = GPMPC_POTRF_PSOLVE_ROWBLOCK,  // launch_gemm_nt_rowblock, in place: a = {rows}
  POTRF_TRAIL_LAT = GPMPC_POTRF_TRAIL_LAT,    // launch_gemm_lat mode 1 on A[c:n, c:n]: a = {M, K}
  POTRF_TRAIL_SYRK = GPMPC_POTRF_TRAIL_SYRK   // launch_gemm_nt, lower C, on A[c:n, c:n]: a = {M, K}
};
struct PotrfStep { int kind, c, K0, a[4]; };

// The launches of the 128-column driver for batch matrices of order n, in order, each handed
// to emit (a visitor: nothing is allocated per call).  Per 128-column block: its update by
// the outer panel's earlier columns, k_potrf_diag128 (L_cc to the matrix, Linv = L_cc^-1 to
// the scratch), the panel solve A[c+128:n, c:c+128] <- A[c+128:n, c:c+128] Linv^T (in
// place); per outer panel one trailing lower SYRK.
template <class Emit>
void potrf_plan(int n, int batch, const PotrfPolicy &p, Emit &&emit) {
  constexpr int B = POTRF_DB;
  auto step = [&](int kind, int c, int K0, int a0, int a1 = 0, int a2 = 0, int a3 = 0) {
    emit(PotrfStep{kind, c, K0, {a0, a1, a2, a3}});
  };
  // few matrices: the panel solve and the trailing SYRK in the latency form
  // (k_gemm_lat: one memory round trip per launch instead of K / 16);
  // GPMPC_POTRF_LAT = 0 / 1 forces it off / on, default for batch <= lat_max
  const bool lat = p.lat >= 0 ? p.lat > 0 : batch <= 16;
  // diagonal kernel: the column sweep (default) or the per-block inverse form.
  // Panel solve in the TRSM form (k_potrf_psolve_lat) with the diagonal kernel's
  // inverted 32 x 32 blocks, for the latency path (GPMPC_POTRF_TRSM=0: the full
  // inverse and the latency GEMM)
  // (measured: batch 32 0.99 -> 0.86 ms, 64 1.35 -> 1.28 ms, 256 3.64 -> 3.75 ms)
  const bool tblk = p.sweep && (p.trsm >= 0 ? p.trsm > 0 : batch <= 64);
  // the diagonal kernel on the packed lower layout (74 KB of LDS: two workgroups per CU)
  // where there are more matrices than CUs (GPMPC_DIAG_PK = 0 / 1: off / whenever the
  // sweep runs)
  const bool pk = p.sweep && (p.pk >= 0 ? p.pk > 0 : batch > 256);
  const int mode = p.sweep | (tblk ? 2 : 0);
  // Outer panels of OB = 128 m columns.  Inside a panel, 128-column steps are
  // left-looking (a step's columns take the update of the panel's earlier
  // steps, K = c - K0); across panels, one lower SYRK with K = OB, so the
  // O(n^3) work runs as K = OB products (fewer C read-modify-writes, longer K).
  // Default: 128 (right-looking, K = 128 SYRKs) below batch 128, 1024 (left-looking:
  // each 128-column block takes the update of all earlier columns, K = c, with no
  // trailing SYRK) from 256 on and from 128 for multiples of 8 (the fused steps) --
  // measured at n = 1000 (round 3, unfused): 64: 1.34 vs 1.60 ms, 256: 3.62 vs 3.58 ms,
  // 1024: 13.6 vs 13.2 ms.  256-512: no better than either.
  // Left-looking from batch 128 when the fused steps apply (a multiple of 8): measured at
  // n = 1000, 128: 2.13 -> 1.95 ms, 192: 2.89 -> 2.54 ms; 64 stays right-looking (1.25 vs 1.36)
  const int OBk = p.ob ? p.ob : ((batch >= 256 || (batch >= 128 && batch % 8 == 0)) ? 8 * B : B);
  // Left-looking block columns, fused: the diagonal block's update alone, the diagonal
  // kernel, then ONE pass over the rows below (update + panel solve, k_gemm128_updsolve)
  // instead of an update launch over all rows and a panel-solve launch; for batches that
  // are a multiple of 8 whose rows below fill >= 512 workgroups (GPMPC_POTRF_FUSE=0: off)
  const bool fuse_ok = p.fuse && OBk > B && !tblk && !lat && batch % 8 == 0;
  // a block column fuses when its rows below fill >= GPMPC_POTRF_FUSE_MIN workgroups (512)
  // (batch 128: 512 -> 1.88 ms, 1 -> 1.95 ms; 256-1024: no difference)
  const int fuse_min = p.fuse_min ? p.fuse_min : 512;
  auto fuses = [&](int c) {
    const int below = n - c - (B < n - c ? B : n - c);
    return fuse_ok && below > 0 && (below + B - 1) / B * batch >= fuse_min;
  };
  // K split (atomic partial sums) of an update whose tiles give fewer than ~2 workgroups
  // per CU, >= 128 of K per split (GPMPC_POTRF_KSPLIT=1: never)
  auto ksplit = [&](int K, int tiles) {
    int ks = 1;
    if (p.ksplit != 1)
      while (ks < K / B && tiles * ks < 512) ++ks;
    return ks;
  };
  for (int K0 = 0; K0 < n; K0 += OBk) {
    const int pw = OBk < n - K0 ? OBk : n - K0;
    bool la_prev = false;  // this step's diagonal update was applied by the previous step
    for (int c = K0; c < K0 + pw; c += B) {
      const int w = B < n - c ? B : n - c, below = n - c - w, K = c - K0;
      const bool fuse = fuses(c);
      // look-ahead (GPMPC_POTRF_LA=1): a fused step's first row tile also applies the next
      // fused step's diagonal-block update (k_gemm128_updsolve<true>), so that launch goes.
      // Off: the first row tiles become the launch's stragglers (batch 1024: 11.6 -> 15.0 ms)
      const bool la = p.la && fuse && w == B && c + B < K0 + pw && fuses(c + B);
      if (c > K0 && fuse && la_prev) {
        // the diagonal block's update came with the previous step's first row tile
      } else if (c > K0 && fuse) {
        // the diagonal block's rows only (one tile per matrix), K split to fill the device;
        // by the balanced lower-triangle kernel (k_syrk128_diag, 9 MFMA blocks per wave)
        // instead of the 128-tile kernel's quadrants (GPMPC_SYRK_DIAG=0)
        const int ks = ksplit(K, batch);
        if (p.syrk_diag) step(POTRF_UPD_SYRK_DIAG, c, K0, w, K, ks);
        else step(POTRF_UPD_ROWBLOCK, c, K0, w, w, K, ks);
      } else if (c > K0) {
        // the block column's update by all earlier columns of the outer panel
        const int ks = ksplit(K, (n - c + B - 1) / B * batch);
        // the last block column of a left-looking panel has no rows below: its diagonal block alone
        if (p.syrk_diag && OBk > B && n - c == w) step(POTRF_UPD_SYRK_DIAG, c, K0, w, K, ks);
        else step(POTRF_UPD_ROWBLOCK, c, K0, n - c, w, K, ks);
      }
      step(POTRF_DIAG, c, K0, w, pk, mode, c + B < n);
      if (fuse)
        step(POTRF_UPDSOLVE, c, K0, below, K, la ? (B < below ? B : below) : 0);
      else if (c + B < n)
        step(tblk ? POTRF_PSOLVE_TRSM : lat ? POTRF_PSOLVE_LAT : POTRF_PSOLVE_ROWBLOCK, c, K0, n - c - B);
      la_prev = la;
    }
    const int t0 = K0 + pw;
    if (t0 < n) step(lat && pw <= B ? POTRF_TRAIL_LAT : POTRF_TRAIL_SYRK, t0, K0, n - t0, pw);
  }
}
