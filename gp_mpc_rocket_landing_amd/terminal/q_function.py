"""Cost-to-go approximators over the safe set (mirror of the reference's
src/terminal/q_function.py by name, signature, default and return value).

``InverseDistanceQFunction`` and ``LocalLinearQFunction`` work on the K nearest stored states
under the plain Euclidean distance.  The reference finds them per state with
``np.linalg.norm`` over the whole set and ``np.argpartition``; here ``predict_batch`` is one
``gpmpc_knn_query`` in numpy's summation order (the distances are numpy's bits,
the exact-match branch takes the lowest index as ``np.argmin`` does) followed by the host
arithmetic on the (B, K) neighbours.  ``argpartition`` leaves the order within the K
unspecified, so the sums may be taken in another order than the reference's: results agree
to the rounding of those sums, not to the bit.  More than 64 neighbours, more than 32 state
entries or ``GPMPC_KNN=host`` run the reference's own numpy lines (local_safe_set.use_device).

``GPQFunction``: the reference's import of its GP classes fails, so there it always falls back
to inverse distance.  Here it fits this project's sparse GP as the reference's
text intends.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .local_safe_set import KNN_MAXD, KNN_MAXK, use_device
from .safe_set import SampledSafeSet


@dataclass
class QFunctionConfig:
    method: str = "inverse_distance"  # "inverse_distance", "gp", "local_linear"
    n_neighbors: int = 10
    idw_power: float = 2.0
    local_linear_reg: float = 1e-4
    gp_lengthscale: float = 1.0
    gp_variance: float = 1.0
    gp_noise: float = 0.01
    q_min: float = 0.0
    q_max: float = np.inf


class QFunctionApproximator(ABC):
    @abstractmethod
    def fit(self, states, q_values) -> None:
        """Take the safe set's states (n, n_x) and their cost-to-go (n,)."""

    @abstractmethod
    def predict(self, x) -> float:
        """Q at one state."""

    @abstractmethod
    def predict_batch(self, X) -> np.ndarray:
        """Q at every row of X."""


class _NeighbourQFunction(QFunctionApproximator):
    """Stored states and Q, and the K nearest of a batch of queries from either path."""

    def __init__(self, config: Optional[QFunctionConfig] = None):
        self.config = config or QFunctionConfig()
        self._states: Optional[np.ndarray] = None
        self._q_values: Optional[np.ndarray] = None
        self._knn = None
        self.last_path: Optional[str] = None

    def fit(self, states, q_values) -> None:
        self._states = states.copy()
        self._q_values = q_values.copy()
        if self._knn is not None:
            self._knn.close()
            self._knn = None

    def _neighbours(self, X):
        """-> idx (B, K) and dist (B, K), K = min(n_neighbors, n), nearest first."""
        n, d = self._states.shape
        K = min(self.config.n_neighbors, n)
        if use_device(n, len(X), 1 <= K <= KNN_MAXK and d <= KNN_MAXD):
            from .. import _lib
            self.last_path = "device"
            if self._knn is None:
                self._knn = _lib.KnnSet(_lib.default_context(), self._states, self._q_values)
            idx, dist, _, _ = self._knn.query(X, K, order=_lib.KNN_NUMPY)
            return idx, dist
        self.last_path = "host"
        idx = np.empty((len(X), K), np.int64); dist = np.empty((len(X), K))
        for b, x in enumerate(X):
            dn = np.linalg.norm(self._states - x, axis=1)
            idx[b] = np.lexsort((np.arange(n), dn))[:K]
            dist[b] = dn[idx[b]]
        return idx, dist

    def predict(self, x) -> float:
        if self._states is None or len(self._states) == 0:
            return self.config.q_max
        return self.predict_batch(np.asarray(x, float)[None])[0]


class InverseDistanceQFunction(_NeighbourQFunction):
    """Q(x) = sum w_i Q(x_i) / sum w_i over the K nearest, w_i = 1 / |x - x_i|^p; the stored Q
    itself within 1e-10 of a stored state; clipped to [q_min, q_max]."""

    def predict_batch(self, X) -> np.ndarray:
        X = np.atleast_2d(np.asarray(X, float))
        if self._states is None or len(self._states) == 0:
            return np.full(len(X), self.config.q_max)
        idx, dist = self._neighbours(X)
        q = self._q_values[idx]
        out = np.empty(len(X))
        hit = dist[:, 0] < 1e-10
        out[hit] = q[hit, 0]                       # an exact match is returned unclipped, as the reference does
        w = 1.0 / (dist[~hit] ** self.config.idw_power)
        w = w / np.sum(w, axis=1, keepdims=True)
        out[~hit] = np.clip(np.sum(w * q[~hit], axis=1), self.config.q_min, self.config.q_max)
        return out


class LocalLinearQFunction(_NeighbourQFunction):
    """Q(x) ~ a + b^T (x_i - x) fitted to the K nearest by least squares weighted with
    1 / (|x - x_i| + 1e-10) and a ridge ``local_linear_reg`` on b; the prediction is a.  A
    singular system falls back to the weighted mean, as the reference does."""

    def _assemble(self, X, idx, dist):
        """A = D^T W D + reg and b = D^T W y per query: D = [1, x_i - x], W = diag(1 / (d_i + 1e-10))."""
        w = 1.0 / (dist + 1e-10)
        design = np.concatenate([np.ones(idx.shape + (1,)), self._states[idx] - X[:, None, :]], axis=2)
        reg = self.config.local_linear_reg * np.eye(design.shape[2])
        reg[0, 0] = 0
        wd = design * w[:, :, None]
        return np.einsum("bki,bkj->bij", design, wd) + reg, np.einsum("bki,bk->bi", wd, self._q_values[idx])

    def predict_batch(self, X) -> np.ndarray:
        X = np.atleast_2d(np.asarray(X, float))
        if self._states is None or len(self._states) == 0:
            return np.full(len(X), self.config.q_max)
        idx, dist = self._neighbours(X)
        B = len(X)
        w = 1.0 / (dist + 1e-10)
        y = self._q_values[idx]
        A, rhs = self._assemble(X, idx, dist)
        try:
            out = np.linalg.solve(A, rhs[:, :, None])[:, 0, 0]
        except np.linalg.LinAlgError:
            out = np.empty(B)
            for b in range(B):
                try:
                    out[b] = np.linalg.solve(A[b], rhs[b])[0]
                except np.linalg.LinAlgError:
                    wb = w[b] / np.sum(w[b])
                    out[b] = float(np.dot(wb, y[b]))
        return np.clip(out, self.config.q_min, self.config.q_max)


class GPQFunction(QFunctionApproximator):
    """A sparse GP over (state, Q): SquaredExponentialARD with ``gp_lengthscale`` on every
    entry and ``gp_variance``, min(50, n // 2) inducing points.  Predictions are the posterior
    mean clipped to [q_min, q_max]; ``predict_with_uncertainty`` adds the variance.  As in the
    reference's text, ``gp_noise`` is carried by the config and not used: the sparse GP keeps
    its own default noise."""

    def __init__(self, config: Optional[QFunctionConfig] = None):
        self.config = config or QFunctionConfig()
        self._gp = None
        self._is_fitted = False

    def fit(self, states, q_values) -> None:
        from ..gp import SparseGP, SquaredExponentialARD
        n, n_x = states.shape
        kernel = SquaredExponentialARD(n_x, signal_variance=self.config.gp_variance,
                                       lengthscales=np.full(n_x, self.config.gp_lengthscale))
        self._gp = SparseGP(kernel, n_inducing=min(50, n // 2))
        self._gp.fit(states, q_values)
        self._is_fitted = True

    def predict(self, x) -> float:
        if not self._is_fitted:
            return self.config.q_max
        mean = self._gp.predict(np.asarray(x, float).reshape(1, -1)).mean
        return float(np.clip(mean[0], self.config.q_min, self.config.q_max))

    def predict_with_uncertainty(self, x) -> Tuple[float, float]:
        if not self._is_fitted:
            return self.predict(x), 0.0
        pred = self._gp.predict(np.asarray(x, float).reshape(1, -1))
        return float(pred.mean[0]), float(pred.variance[0])

    def predict_batch(self, X) -> np.ndarray:
        if not self._is_fitted:
            return np.full(len(X), self.config.q_max)
        return np.clip(self._gp.predict(X).mean, self.config.q_min, self.config.q_max)


class QFunctionManager:
    """Keeps an approximator (``config.method``) fitted to a safe set.

    >>> q_manager = QFunctionManager(safe_set)
    >>> q_manager.update()            # after a landing was added
    >>> q_manager.evaluate(x)
    """

    def __init__(self, safe_set: SampledSafeSet, config: Optional[QFunctionConfig] = None):
        self.safe_set = safe_set
        self.config = config or QFunctionConfig()
        kinds = {"inverse_distance": InverseDistanceQFunction, "local_linear": LocalLinearQFunction,
                 "gp": GPQFunction}
        if self.config.method not in kinds:
            raise ValueError(f"Unknown method: {self.config.method}")
        self._approximator = kinds[self.config.method](self.config)
        self._is_fitted = False
        self._last_update_iteration = -1

    def update(self) -> None:
        states = self.safe_set.get_all_states()
        if len(states) > 0:
            self._approximator.fit(states, self.safe_set.get_all_q_values())
            self._is_fitted = True
        self._last_update_iteration = self.safe_set.num_iterations

    def evaluate(self, x) -> float:
        if not self._is_fitted:
            self.update()
        return self._approximator.predict(x)

    def evaluate_batch(self, X) -> np.ndarray:
        if not self._is_fitted:
            self.update()
        return self._approximator.predict_batch(X)

    def needs_update(self) -> bool:
        return self.safe_set.num_iterations > self._last_update_iteration

    def get_min_q(self) -> float:
        if self.safe_set.num_states == 0:
            return np.inf
        return float(np.min(self.safe_set.get_all_q_values()))

    def get_statistics(self) -> dict:
        q = self.safe_set.get_all_q_values()
        if len(q) == 0:
            return {"n_points": 0}
        return {"n_points": len(q), "q_min": float(np.min(q)), "q_max": float(np.max(q)),
                "q_mean": float(np.mean(q)), "q_std": float(np.std(q))}


class IterativeQFunction:
    """Q^j: the inverse-distance Q-function over the landings of iterations <= j, kept per j
    (learning MPC improves it: Q^(j+1) <= Q^j)."""

    def __init__(self, safe_set: SampledSafeSet):
        self.safe_set = safe_set
        self._q_by_iteration: dict = {}

    def get_q_at_iteration(self, iteration: int) -> Optional[QFunctionApproximator]:
        if iteration not in self._q_by_iteration:
            ts = [t for t in self.safe_set._trajectories if t.iteration <= iteration]
            approx = None
            if ts:
                approx = InverseDistanceQFunction()
                approx.fit(np.vstack([t.states for t in ts]), np.concatenate([t.cost_to_go for t in ts]))
            self._q_by_iteration[iteration] = approx
        return self._q_by_iteration[iteration]

    def evaluate(self, x, iteration: Optional[int] = None) -> float:
        """Q^iteration(x) (the latest iteration without one); inf before any landing."""
        if iteration is None:
            iteration = self.safe_set.num_iterations - 1
        approx = self.get_q_at_iteration(iteration)
        return np.inf if approx is None else approx.predict(x)

    def get_improvement(self, x) -> float:
        """Q^0(x) - Q^J(x); 0 with fewer than two iterations."""
        n_iter = self.safe_set.num_iterations
        if n_iter < 2:
            return 0.0
        return self.evaluate(x, iteration=0) - self.evaluate(x, iteration=n_iter - 1)
