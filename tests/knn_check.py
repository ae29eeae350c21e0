"""A plain restatement of the gpmpc_knn_query / gpmpc_knn_interp contract (include/gpmpc.h,
DESIGN §17), the oracle of the device tests.

Every numpy operation below is one rounded fp64 operation per element (no FMA), so the order
of the additions is the order written here:

- ``sq_kd``: scipy's KD-tree (sqeuclidean_distance_double): four accumulators from 0, every
  full block of four elements added lane-wise, ((a0+a1)+a2)+a3, the d % 4 tail one by one;
- ``sq_np``: numpy's add.reduce along a contiguous axis, the order of
  ``np.linalg.norm(A - x, axis=1)``: d < 8 left to right; d >= 8 eight accumulators over full
  blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the d % 8 tail one by one.

tests/test_knn_check.py pins the first to scipy.spatial.KDTree and the second to numpy."""
import numpy as np

KD, NP = 0, 1
MAXK = 64


def sq_kd(S, x):
    """s^2 of every row of S (n, d) to x (d,) in the KD-tree's order."""
    S = np.asarray(S, np.float64); x = np.asarray(x, np.float64)
    n, d = S.shape
    df = x[None, :] - S
    t = df * df
    a = [np.zeros(n) for _ in range(4)]
    for b in range(0, d - d % 4, 4):
        for j in range(4):
            a[j] = a[j] + t[:, b + j]
    s = ((a[0] + a[1]) + a[2]) + a[3]
    for k in range(d - d % 4, d):
        s = s + t[:, k]
    return s


def sq_np(S, x):
    """s^2 of every row of S (n, d) to x (d,) in numpy's order."""
    S = np.asarray(S, np.float64); x = np.asarray(x, np.float64)
    n, d = S.shape
    df = S - x[None, :]
    t = df * df
    if d < 8:
        s = t[:, 0].copy()
        for k in range(1, d):
            s = s + t[:, k]
        return s
    r = [t[:, j].copy() for j in range(8)]
    for b in range(8, d - d % 8, 8):
        for j in range(8):
            r[j] = r[j] + t[:, b + j]
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(d - d % 8, d):
        s = s + t[:, k]
    return s


def sqdist(order, S, x):
    return sq_kd(S, x) if order == KD else sq_np(S, x)


def knn_query(S, order, Xq, k, radius=0.0, fuel_req=None, avail_fuel=None):
    """-> idx (B, k) int64, dist (B, k), n_ball (B,), n_feasible (B,): the contract of
    gpmpc_knn_query, by a lexicographic sort on (s^2, index)."""
    S = np.asarray(S, np.float64); Xq = np.atleast_2d(np.asarray(Xq, np.float64))
    n, B = S.shape[0], Xq.shape[0]
    idx = np.full((B, k), n, np.int64); dist = np.full((B, k), np.inf)
    n_ball = np.zeros(B, np.int64); n_feas = np.zeros(B, np.int64)
    r2 = np.float64(radius) * np.float64(radius)
    for b in range(B):
        s2 = sqdist(order, S, Xq[b])
        ok = np.ones(n, bool) if avail_fuel is None else np.asarray(fuel_req) <= avail_fuel[b]
        rows = np.nonzero(ok)[0]
        n_feas[b] = rows.size
        n_ball[b] = int(np.sum(s2[rows] <= r2))
        rows = rows[np.isfinite(s2[rows])]   # an overflowed s^2 is never below the inf threshold
        pick = rows[np.lexsort((rows, s2[rows]))][:k]
        idx[b, :pick.size] = pick
        dist[b, :pick.size] = np.sqrt(s2[pick])
    return idx, dist, n_ball, n_feas


def k_rule(k_base, k_min, k_max, adaptive, n_ball, n_avail):
    """The K of LocalSafeSet.query: adaptive K from the ball count, then the three clamps."""
    K = k_base
    if adaptive and n_avail > 0:
        K = int(k_base * (1 + (n_ball / n_avail) * 2))
        K = min(max(K, k_min), k_max)
    K = min(K, n_avail)
    K = max(K, k_min)
    return min(K, k_max)


def knn_interp(S, q, order, Xq, k_base, k_min, k_max, adaptive, radius, fuel_req=None, avail_fuel=None):
    """-> q_out (B,), k_used (B,): the contract of gpmpc_knn_interp.  The weighted mean is
    summed here in ascending neighbour order; the device sums a wave tree, so the two agree
    to the roundings of K - 1 additions, not to the bit."""
    Xq = np.atleast_2d(np.asarray(Xq, np.float64)); q = np.asarray(q, np.float64)
    idx, dist, nb, nf = knn_query(S, order, Xq, MAXK, radius, fuel_req, avail_fuel)
    out = np.zeros(Xq.shape[0]); used = np.zeros(Xq.shape[0], np.int64)
    for b in range(Xq.shape[0]):
        K = k_rule(k_base, k_min, k_max, adaptive, int(nb[b]), int(nf[b]))
        if nf[b] == 0 or K == 0:
            out[b], used[b] = np.inf, 0
        elif K > nf[b]:
            out[b], used[b] = np.nan, -1
        elif dist[b, 0] < 1e-10:
            out[b], used[b] = q[idx[b, 0]], K
        else:
            w = 1.0 / (dist[b, :K] + 1e-10)
            tot = 0.0
            for v in w:
                tot = tot + v
            w = w / tot
            acc = 0.0
            for v, qq in zip(w, q[idx[b, :K]]):
                acc = acc + v * qq
            out[b], used[b] = acc, K
    return out, used
