"""Convex-hull terminal constraint of learning MPC, x_N in Conv{v_1 .. v_K} with x_N = sum
lambda_i v_i, sum lambda = 1, lambda >= 0 (mirror of the reference's src/terminal/convex_hull.py
by name, signature and default; ``CasADiConvexHullConstraint`` exists there only with CasADi and
is not restated).

Every question asked of a hull is one computation, the point of the hull nearest a query, and
every path takes it to the device (csrc/hull.hip): ``gpmpc_hull_project`` for a given
vertex set, ``gpmpc_knn_hull`` for the K nearest safe states of each of many queries in one call.
Sets of more than 64 vertices or 32 state entries are refused with ValueError; there is no host
fallback.

Rosolia, U., & Borrelli, F. (2017). Learning MPC for Iterative Tasks.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from .local_safe_set import LocalSafeSet, LocalSafeSetConfig, use_device
from .safe_set import SampledSafeSet

HULL_MAXK = 64   # _lib.HULL_MAXK: the vertices one device call takes
HULL_MAXD = 32   # _lib.HULL_MAXD


def _check_limits(K: int, n_x: int) -> None:
    if K > HULL_MAXK:
        raise ValueError(f"convex hull of {K} vertices: the device takes at most {HULL_MAXK}")
    if n_x > HULL_MAXD:
        raise ValueError(f"convex hull in {n_x} dimensions: the device takes at most {HULL_MAXD}")


@dataclass
class ConvexHullConfig:
    """Configuration for convex hull constraints."""

    n_vertices: int = 10
    use_slack: bool = True
    slack_weight: float = 1e4
    convex_tol: float = 1e-6
    lambda_min: float = 0.0
    lambda_max: float = 1.0


class ConvexHullConstraint:
    """The hull of ``vertices`` (K, n_x) with the cost-to-go ``q_values`` (K,) at them.

    >>> ch = ConvexHullConstraint(vertices, q_values)
    >>> x_proj, lambdas = ch.project_onto_hull(x)
    >>> terminal_cost = ch.get_interpolated_q(lambdas)
    """

    def __init__(self, vertices, q_values, config: Optional[ConvexHullConfig] = None):
        self.config = config or ConvexHullConfig()
        self.vertices = vertices
        self.q_values = q_values
        self.K = len(vertices)
        self.n_x = vertices.shape[1] if len(vertices) > 0 else 0
        _check_limits(self.K, self.n_x)

    def update_vertices(self, vertices, q_values) -> None:
        """Update vertices (for dynamic safe set).  As in the reference ``n_x`` keeps the value
        of construction."""
        _check_limits(len(vertices), vertices.shape[1] if len(vertices) > 0 else 0)
        self.vertices = vertices
        self.q_values = q_values
        self.K = len(vertices)

    def _project(self, X) -> Dict[str, np.ndarray]:
        from .. import _lib
        return _lib.hull_project(_lib.default_context(), np.asarray(self.vertices, float), X)

    def project_batch(self, X) -> Tuple[np.ndarray, np.ndarray]:
        """``[project_onto_hull(x) for x in X]`` in one device call -> X_proj (B, n_x), lambdas
        (B, K)."""
        X = np.atleast_2d(np.asarray(X, float))
        if self.K == 0:
            return X.copy(), np.zeros((len(X), 0))
        lam = self._project(X)["lam"]
        V = np.asarray(self.vertices, float)
        return np.stack([V.T @ lam_b for lam_b in lam]), lam

    def project_onto_hull(self, x) -> Tuple[np.ndarray, np.ndarray]:
        """The point of Conv(vertices) nearest x -> (x_proj, lambdas), x_proj = vertices.T @
        lambdas: the true projection, the meaning of the reference's IPOPT path.  It is not the
        reference's answer without CasADi, which is the nearest vertex.  K = 0: (x, array([]))."""
        if self.K == 0:
            return x, np.array([])
        X_proj, lam = self.project_batch(np.asarray(x, float)[None])
        return X_proj[0], lam[0]

    def contains_batch(self, X) -> np.ndarray:
        """``[check_feasibility(x) for x in X]`` in one device call."""
        X = np.atleast_2d(np.asarray(X, float))
        if self.K == 0:
            return np.zeros(len(X), bool)
        if self.n_x >= self.K:  # not enough points for a full-dimensional hull: the reference's lines
            out = np.empty(len(X), bool)
            for b, x in enumerate(X):
                distances = np.linalg.norm(self.vertices - x, axis=1)
                out[b] = np.min(distances) < self.config.convex_tol
            return out
        return self._project(X)["dist"] <= self.config.convex_tol

    def check_feasibility(self, x) -> bool:
        """Whether x is inside the hull: False with K = 0; with n_x >= K whether a vertex lies
        within ``convex_tol`` of x (the reference's rule); otherwise whether the distance to the
        hull is at most ``convex_tol`` (the reference triangulates)."""
        return bool(self.contains_batch(np.asarray(x, float)[None])[0])

    def get_interpolated_q(self, lambdas) -> float:
        """Q(x) = sum lambda_i Q(v_i)."""
        return float(np.dot(lambdas, self.q_values))


class TerminalSetManager:
    """The terminal set of learning MPC: the local safe set around a state and its hull.

    >>> manager = TerminalSetManager(safe_set)
    >>> vertices, q_values = manager.get_terminal_set(x, available_fuel)
    >>> is_safe = manager.is_in_terminal_set(x)
    >>> out = manager.project_batch(X)
    """

    def __init__(self, safe_set: SampledSafeSet, n_vertices: int = 10, use_fuel_aware: bool = True):
        self.safe_set = safe_set
        self.n_vertices = n_vertices
        self.use_fuel_aware = use_fuel_aware
        self._local_ss = LocalSafeSet(safe_set, LocalSafeSetConfig(K=n_vertices))
        self._ch_constraint = ConvexHullConstraint(np.zeros((0, safe_set.n_x)), np.zeros(0))
        self.last_path: Optional[str] = None

    def get_terminal_set(self, x, available_fuel: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
        """-> the vertices (K, n_x) of the terminal set around x and their Q (K,)."""
        if self.use_fuel_aware and available_fuel is not None:
            vertices, q_values, _ = self._local_ss.query(x, K=self.n_vertices, available_fuel=available_fuel)
        else:
            vertices, q_values, _ = self._local_ss.query(x, K=self.n_vertices)
        self._ch_constraint.update_vertices(vertices, q_values)
        return vertices, q_values

    def is_in_terminal_set(self, x, available_fuel: Optional[float] = None) -> bool:
        vertices, _ = self.get_terminal_set(x, available_fuel)
        if len(vertices) == 0:
            return False
        return self._ch_constraint.check_feasibility(x)

    def get_terminal_cost(self, x) -> float:
        return self._local_ss.interpolate_q(x)

    def invalidate(self) -> None:
        """Invalidate caches (call when safe set changes)."""
        self._local_ss.invalidate()

    # ---- many states at once -------------------------------------------------------------
    def project_batch(self, X, available_fuel=None) -> Dict[str, np.ndarray]:
        """Every state of X (B, n_x) projected onto the hull of its own terminal set ->
        dict(idx (B, K_max) the vertices' rows in the safe set, nearest first, num_states past
        k_used; k_used (B,); lam (B, K_max); proj (B, n_x); dist (B,); q (B,) the interpolated
        cost-to-go, inf without a safe state; status (B,), gpmpc_hull_project's).

        Where the local safe set's switch chooses the device (``use_device``, GPMPC_KNN) it is
        one gpmpc_knn_hull call; otherwise the host k-NN runs and one gpmpc_hull_project call
        follows.  ``last_path`` says which.  Fewer available states than K_min raises the
        IndexError of ``LocalSafeSet.interpolate_q_batch``."""
        from .. import _lib
        X = np.atleast_2d(np.asarray(X, float))
        ls, ss = self._local_ss, self.safe_set
        c = ls.config
        _check_limits(c.K_max, ss.n_x)
        B, n, km = len(X), ss.num_states, c.K_max
        ls._rebuild_tree()
        if ls._weighted_states is None or n == 0:
            self.last_path = "host"
            return dict(idx=np.full((B, km), n, np.int64), k_used=np.zeros(B, np.int64), lam=np.zeros((B, km)),
                        proj=X.copy(), dist=np.full(B, np.inf), q=np.full(B, np.inf), status=np.full(B, 2, np.int64))
        filt = self.use_fuel_aware and ls._filters(available_fuel)
        fuel = np.broadcast_to(np.asarray(available_fuel, float), (B,)) if filt else None
        Xw = X * ls._weights
        if use_device(n, B, ls._fits_device()):
            self.last_path = ls.last_path = "device"
            ks = ls._device_set()
            if ks.dp == 0:
                ks.set_points(ss.get_all_states())
            out = ks.hull(Xw, X, c.K if c.adaptive_K else self.n_vertices, c.K_min, c.K_max, c.adaptive_K,
                          c.density_radius, fuel)
            k_used, idx, q = out["k_used"], out["idx"], out["qhull"]
        else:
            self.last_path = ls.last_path = "host"
            near, _, n_ball, n_feas = ls._host_neighbours(Xw, fuel)
            states, qv = ss.get_all_states(), ss.get_all_q_values()
            k_used = np.zeros(B, np.int64); idx = np.full((B, km), n, np.int64)
            V = np.zeros((B, km, ss.n_x)); Q = np.zeros((B, km))
            for b in range(B):
                n_avail = int(n_feas[b])
                Kb = ls._clamp_K(self.n_vertices, int(n_ball[b]), n_avail) if n_avail else 0
                if Kb > n_avail:
                    k_used[b] = -1
                    continue
                k_used[b] = Kb
                idx[b, :Kb] = near[b, :Kb]
                V[b, :Kb] = states[near[b, :Kb]]
                Q[b, :Kb] = qv[near[b, :Kb]]
            out = _lib.hull_project(_lib.default_context(), V, X, Q, np.maximum(k_used, 0))
            q = out["qhull"]
        if np.any(k_used < 0):
            raise IndexError(f"index {n} is out of bounds for axis 0 with size {n}")
        return dict(idx=idx, k_used=k_used, lam=out["lam"], proj=out["proj"], dist=out["dist"], q=q,
                    status=out["status"])

    def is_in_terminal_set_batch(self, X, available_fuel=None) -> np.ndarray:
        """``[is_in_terminal_set(x, f) for x, f in zip(X, available_fuel)]`` on ``project_batch``."""
        X = np.atleast_2d(np.asarray(X, float))
        out = self.project_batch(X, available_fuel)
        states = self.safe_set.get_all_states()
        tol, n_x = self._ch_constraint.config.convex_tol, self._ch_constraint.n_x
        inside = np.zeros(len(X), bool)
        for b, K in enumerate(out["k_used"]):
            if K == 0:
                continue
            if n_x >= K:
                distances = np.linalg.norm(states[out["idx"][b, :K]] - X[b], axis=1)
                inside[b] = np.min(distances) < tol
            else:
                inside[b] = out["dist"][b] <= tol
        return inside
