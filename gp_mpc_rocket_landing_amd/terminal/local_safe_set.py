"""The local safe set: the K safe states nearest a query, for the convex-hull terminal
constraint and the interpolated cost-to-go of learning MPC (mirror of the reference's
src/terminal/local_safe_set.py by name, signature, default and return value).

The reference answers a query with one ``KDTree.query`` and one ``query_ball_point`` (and,
with a fuel filter, a tree built for that query).  Here one ``gpmpc_knn_query`` over the
weighted states resident on the device returns the 64 nearest, the ball count and the
feasible count; summed in the KD-tree's order they are the reference's bits, so
``query`` and ``interpolate_q`` return what the reference returns.  ``query_batch`` and
``interpolate_q_batch`` answer many states in one call.

``K_max`` > 64, more than 32 state entries, a ``distance_metric`` other than the default
(the reference ignores the field, so those keep its exact host code), or ``GPMPC_KNN=host``
take scipy's KD-tree on the host; ``GPMPC_KNN=device`` forces the device; unset, the device
serves calls of at least ``KNN_CROSSOVER`` queries or rows (docs/PERF_HISTORY.md).  ``query``
and ``interpolate_q`` return the same bits on both paths (``interpolate_q_batch``: see there);
``last_path`` says which one ran.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
from scipy.spatial import KDTree

from .safe_set import FuelAwareSafeSet, SampledSafeSet

KNN_MAXK = 64   # _lib.KNN_MAXK: the neighbours one device call returns
KNN_MAXD = 32   # _lib.KNN_MAXD
# unset GPMPC_KNN: the device serves a call of at least this many queries, or a set of at
# least this many rows; below both the call goes to the KD-tree.  Measured (docs/PERF_HISTORY.md):
# eight states win on the device at every set size from 512 rows on, four tie or lose up to 4096
# rows; one state loses up to 16 384 rows and wins from 65 536
KNN_CROSSOVER = {"queries": 8, "rows": 65536}


def knn_mode() -> str:
    """GPMPC_KNN: "host", "device" or "" (automatic)."""
    mode = os.environ.get("GPMPC_KNN", "").strip().lower()
    if mode not in ("", "host", "device"):
        raise ValueError(f"GPMPC_KNN={mode!r}: expected host or device")
    return mode


def use_device(n_rows: int, n_queries: int, fits: bool) -> bool:
    """Whether a call of n_queries over n_rows runs on the device.  fits: the kernel takes the
    configuration (K <= 64, d <= 32, the default metric); one it does not take is the host's
    under every setting of the switch, and ``last_path`` says so."""
    mode = knn_mode()
    if mode == "host" or not fits:
        return False
    return mode == "device" or n_queries >= KNN_CROSSOVER["queries"] or n_rows >= KNN_CROSSOVER["rows"]


@dataclass
class LocalSafeSetConfig:
    """Neighbour counts, the state weights of the distance, the density rule and the fuel filter."""

    K: int = 10
    K_min: int = 4
    K_max: int = 50
    distance_metric: str = "weighted_euclidean"
    position_weight: float = 1.0
    velocity_weight: float = 0.5
    attitude_weight: float = 0.3
    angular_rate_weight: float = 0.2
    fuel_weight: float = 0.1
    adaptive_K: bool = True  # noqa: N815
    density_radius: float = 1.0
    filter_by_fuel: bool = True
    fuel_margin: float = 0.1


class LocalSafeSet:
    """K nearest safe states around a query under a weighted Euclidean distance.

    >>> local_ss = LocalSafeSet(safe_set, config)
    >>> neighbors, q_values, distances = local_ss.query(x)
    >>> q = local_ss.interpolate_q(x)
    """

    def __init__(self, safe_set: SampledSafeSet, config: Optional[LocalSafeSetConfig] = None):
        self.safe_set = safe_set
        self.config = config or LocalSafeSetConfig()
        self._kdtree: Optional[KDTree] = None
        self._weighted_states: Optional[np.ndarray] = None
        self._weights = self._build_weight_vector()
        self._tree_valid = False
        self._knn = None            # the resident device set (_lib.KnnSet)
        self.last_path: Optional[str] = None

    def _build_weight_vector(self) -> np.ndarray:
        """sqrt of the per-entry weights: [m, r(3), v(3)] for 7 states, [m, r(3), v(3), q(4),
        w(3)] for 14, ones otherwise."""
        c, n_x = self.config, self.safe_set.n_x
        w = np.ones(n_x)
        if n_x in (7, 14):
            w[0] = c.fuel_weight
            w[1:4] = c.position_weight
            w[4:7] = c.velocity_weight
        if n_x == 14:
            w[7:11] = c.attitude_weight
            w[11:14] = c.angular_rate_weight
        return np.sqrt(w)

    # ---- the two holders of the weighted states ------------------------------------
    def _rebuild_tree(self) -> None:
        if self._tree_valid:
            return
        states = self.safe_set.get_all_states()
        self._kdtree = None
        self._drop_device_set()
        self._weighted_states = states * self._weights[np.newaxis, :] if len(states) else None
        self._tree_valid = True

    def _host_tree(self) -> KDTree:
        if self._kdtree is None:
            self._kdtree = KDTree(self._weighted_states)
        return self._kdtree

    def _device_set(self):
        if self._knn is None:
            from .. import _lib
            ss = self.safe_set
            fuel = ss.get_fuel_required() if isinstance(ss, FuelAwareSafeSet) else None
            self._knn = _lib.KnnSet(_lib.default_context(), self._weighted_states, ss.get_all_q_values(), fuel)
        return self._knn

    def _drop_device_set(self) -> None:
        if self._knn is not None:
            self._knn.close()
            self._knn = None

    def invalidate(self) -> None:
        """Call when the safe set changed: the tree and the resident device set are dropped."""
        self._tree_valid = False
        self._kdtree = None
        self._drop_device_set()

    def _fits_device(self) -> bool:
        c = self.config
        return (c.K_max <= KNN_MAXK and self.safe_set.n_x <= KNN_MAXD and c.distance_metric == "weighted_euclidean")

    def _filters(self, available_fuel) -> bool:
        return (self.config.filter_by_fuel and available_fuel is not None
                and isinstance(self.safe_set, FuelAwareSafeSet))

    def _clamp_K(self, K, n_ball, n_avail) -> int:
        """The reference's K rule in its order (local_safe_set.py:203-210, 236-249)."""
        c = self.config
        if c.adaptive_K:
            K = int(c.K * (1 + (n_ball / n_avail) * 2))
            K = int(np.clip(K, c.K_min, c.K_max))
        K = min(K, n_avail)
        K = max(K, c.K_min)
        return min(K, c.K_max)

    # ---- queries -----------------------------------------------------------------------
    def query(self, x, K: Optional[int] = None,
              available_fuel: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> neighbours (K, n_x), their Q (K,), their weighted distances (K,), nearest first.

        K is ``K or config.K``; with ``adaptive_K`` it is ``int(config.K * (1 + 2 * n_ball /
        n))`` clipped to [K_min, K_max] instead; then min with the number of available states,
        max with K_min, min with K_max.  With a fuel filter (a FuelAwareSafeSet and
        ``available_fuel``) n and the ball count are those of the feasible states.  An empty
        (or wholly infeasible) set returns three empty arrays.

        As in the reference, fewer available states than the resulting K (so: fewer than
        K_min) raises IndexError: its ``states[indices]`` indexes past the end with the KD-tree's
        padding index."""
        out = self.query_batch(np.asarray(x, float)[None], K, available_fuel)
        return out[0]

    def query_batch(self, X, K: Optional[int] = None, available_fuel=None) -> List[Tuple[np.ndarray, ...]]:
        """``[query(x, K, f) for x, f in zip(X, available_fuel)]`` (available_fuel: None, one
        value for all, or one per state), the device's part in one call."""
        X = np.atleast_2d(np.asarray(X, float))
        self._rebuild_tree()
        ss, c = self.safe_set, self.config
        empty = (np.zeros((0, ss.n_x)), np.zeros(0), np.zeros(0))
        if self._weighted_states is None or ss.num_states == 0:
            return [tuple(a.copy() for a in empty) for _ in X]
        K0 = K or c.K
        filt = self._filters(available_fuel)
        fuel = np.broadcast_to(np.asarray(available_fuel, float), (len(X),)) if filt else None
        n = ss.num_states
        if use_device(n, len(X), self._fits_device()):
            self.last_path = "device"
            idx, dist, n_ball, n_feas = self._device_set().query(X * self._weights, KNN_MAXK, c.density_radius, fuel)
        else:
            self.last_path = "host"
            idx, dist, n_ball, n_feas = self._host_neighbours(X * self._weights, fuel)
        states, q = ss.get_all_states(), ss.get_all_q_values()
        out = []
        for b in range(len(X)):
            n_avail = int(n_feas[b])
            if n_avail == 0:
                out.append(tuple(a.copy() for a in empty))
                continue
            Kb = self._clamp_K(K0, int(n_ball[b]), n_avail)
            if Kb == 0:
                out.append(tuple(a.copy() for a in empty))
                continue
            if Kb > n_avail:
                raise IndexError(f"index {n_avail} is out of bounds for axis 0 with size {n_avail}")
            ib = idx[b, :Kb]
            out.append((states[ib], q[ib], dist[b, :Kb].copy()))
        return out

    def _host_neighbours(self, Xw, fuel):
        """The host path: scipy's KD-tree, per state as the reference runs it (a tree of the
        feasible states per query with a fuel filter) -> the arrays of gpmpc_knn_query."""
        c, ss = self.config, self.safe_set
        B, n = len(Xw), ss.num_states
        kk = max(min(c.K_max, n), 1)
        idx = np.full((B, kk), n, np.int64); dist = np.full((B, kk), np.inf)
        n_ball = np.zeros(B, np.int64); n_feas = np.full(B, n, np.int64)
        for b in range(B):
            rows = None
            tree = self._host_tree()
            if fuel is not None:
                rows = np.where(ss.get_fuel_required() <= fuel[b])[0]
                n_feas[b] = len(rows)
                if len(rows) == 0:
                    continue
                tree = KDTree(self._weighted_states[rows])
            if c.adaptive_K:
                n_ball[b] = len(tree.query_ball_point(Xw[b], c.density_radius))
            k = min(kk, int(n_feas[b]))
            dd, ii = tree.query(Xw[b], k=k)
            dd, ii = np.atleast_1d(dd), np.atleast_1d(ii)
            idx[b, :k] = ii if rows is None else rows[ii]
            dist[b, :k] = dd
        return idx, dist, n_ball, n_feas

    @staticmethod
    def _weighted_mean(q_values, distances) -> float:
        """The reference's few numpy lines (local_safe_set.py:279-287)."""
        if distances[0] < 1e-10:
            return q_values[0]
        weights = 1.0 / (distances + 1e-10)
        weights = weights / np.sum(weights)
        return float(np.dot(weights, q_values))

    def interpolate_q(self, x, K: Optional[int] = None, method: str = "inverse_distance") -> float:
        """Q at ``x`` from its neighbours: "nearest", "inverse_distance" or "linear" (the
        reference's "linear" is the same inverse-distance convex combination).  inf without a
        safe state; ValueError for another method, raised (as there) after the query."""
        _, q_values, distances = self.query(x, K)
        if len(q_values) == 0:
            return np.inf
        if method == "nearest":
            return q_values[0]
        if method in ("inverse_distance", "linear"):
            return self._weighted_mean(q_values, distances)
        raise ValueError(f"Unknown interpolation method: {method}")

    def interpolate_q_batch(self, X, K: Optional[int] = None, method: str = "inverse_distance") -> np.ndarray:
        """``[interpolate_q(x, K, method) for x in X]``.  On the device "inverse_distance" and
        "linear" are one fused call (gpmpc_knn_interp: neighbours, K rule and weighting, no
        round trip through the host); its weighted mean is summed as a wave tree, so it agrees
        with the loop to the roundings of the K additions, not to the bit."""
        X = np.atleast_2d(np.asarray(X, float))
        if method not in ("nearest", "inverse_distance", "linear"):
            raise ValueError(f"Unknown interpolation method: {method}")
        self._rebuild_tree()
        n = self.safe_set.num_states
        if (method != "nearest" and self._weighted_states is not None and n > 0
                and use_device(n, len(X), self._fits_device())):
            c = self.config
            self.last_path = "device"
            # with adaptive K the rule scales config.K and the caller's K plays no part (_clamp_K)
            k_base = c.K if c.adaptive_K else (K or c.K)
            out, used = self._device_set().interp(X * self._weights, k_base, c.K_min, c.K_max, c.adaptive_K,
                                                  c.density_radius)
            if np.any(used < 0):
                raise IndexError(f"index {n} is out of bounds for axis 0 with size {n}")
            return out
        res = np.empty(len(X))
        for b, (_, q_values, distances) in enumerate(self.query_batch(X, K)):
            if len(q_values) == 0:
                res[b] = np.inf
            elif method == "nearest":
                res[b] = q_values[0]
            else:
                res[b] = self._weighted_mean(q_values, distances)
        return res

    def get_convex_hull_data(self, x, K: Optional[int] = None,
                             available_fuel: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The vertices (K, n_x) of the terminal constraint x_N in Conv{v_1 .. v_K}, and their Q."""
        neighbors, q_values, _ = self.query(x, K, available_fuel)
        return neighbors, q_values


class MultiResolutionLocalSafeSet:
    """Local safe sets of several sizes (K = 5, 10, 20, ... by default, adaptive K off) over
    one safe set, for estimates from coarse to fine."""

    def __init__(self, safe_set: SampledSafeSet, n_levels: int = 3, K_per_level: Optional[List[int]] = None):
        self.safe_set = safe_set
        self.n_levels = n_levels
        self.K_per_level = K_per_level or [5 * (2 ** i) for i in range(n_levels)]
        self._local_sets: List[LocalSafeSet] = [LocalSafeSet(safe_set, LocalSafeSetConfig(K=K, adaptive_K=False))
                                                for K in self.K_per_level]

    def query_hierarchical(self, x) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
        return [ls.query(x) for ls in self._local_sets]

    def interpolate_q_hierarchical(self, x, weights: Optional[np.ndarray] = None) -> float:
        """The levels' inverse-distance estimates combined with ``weights`` (default 1, 2, 4, ...
        normalised: more weight to the larger K); levels without a safe state are left out,
        inf when none has one."""
        if weights is None:
            weights = np.array([2 ** i for i in range(self.n_levels)])
            weights = weights / np.sum(weights)
        est = np.array([ls.interpolate_q(x) for ls in self._local_sets])
        ok = np.isfinite(est)
        if not np.any(ok):
            return np.inf
        w = weights[ok]
        w = w / np.sum(w)
        return float(np.dot(w, est[ok]))

    def invalidate(self) -> None:
        for ls in self._local_sets:
            ls.invalidate()
