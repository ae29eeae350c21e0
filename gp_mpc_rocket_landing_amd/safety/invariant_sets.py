"""Invariant sets and the tube controller of the safety filter (mirror of the reference's
src/safety/invariant_sets.py by name, signature, default and return value; host numpy / scipy).

The backup set is the ellipsoid S = {x : (x - x_eq)' P (x - x_eq) <= alpha} of the backup
controller's Lyapunov matrix.  ``compute_maximal_alpha`` and ``get_boundary_points`` draw from
numpy's global generator in the reference's order, so a caller's ``np.random.seed`` gives the
reference's numbers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

try:
    from scipy.linalg import solve_discrete_are, solve_discrete_lyapunov

    HAS_SCIPY = True
except ImportError:  # pragma: no cover
    HAS_SCIPY = False


@dataclass
class InvariantSetConfig:
    alpha: float = 1.0
    constraint_margin: float = 0.1
    max_iter: int = 100
    tol: float = 1e-6
    w_max: float = 0.1


class EllipsoidalInvariantSet:
    """S = {x : (x - x_eq)' P (x - x_eq) <= alpha}.

    >>> inv_set = EllipsoidalInvariantSet(n_x=14)
    >>> inv_set.compute_from_lqr(P_lqr, x_eq)
    >>> inv_set.contains(x)
    """

    def __init__(self, n_x: int, config: Optional[InvariantSetConfig] = None):
        self.n_x = n_x
        self.config = config or InvariantSetConfig()
        self.P: Optional[np.ndarray] = None
        self.x_eq: Optional[np.ndarray] = None
        self.alpha: float = 1.0

    def compute_from_lqr(self, P_lqr, x_eq, alpha: Optional[float] = None) -> None:
        self.P = P_lqr.copy()
        self.x_eq = x_eq.copy()
        self.alpha = alpha if alpha is not None else self.config.alpha

    def compute_maximal_alpha(self, constraint_fn: Callable, n_samples: int = 1000) -> float:
        """The largest alpha in [0.01, 100] (50 bisections) at which ``constraint_fn`` holds on
        n_samples boundary points, times (1 - constraint_margin)."""
        if self.P is None:
            raise RuntimeError("Must call compute_from_lqr first")
        samples = np.random.randn(n_samples, self.n_x)
        samples = samples / np.linalg.norm(samples, axis=1, keepdims=True)
        try:
            P_inv_sqrt = np.linalg.cholesky(np.linalg.inv(self.P)).T
        except np.linalg.LinAlgError:
            eigvals, eigvecs = np.linalg.eigh(self.P)
            eigvals = np.maximum(eigvals, 1e-10)
            P_inv_sqrt = eigvecs @ np.diag(1.0 / np.sqrt(eigvals)) @ eigvecs.T
        alpha_low, alpha_high = 0.01, 100.0
        for _ in range(50):
            alpha_mid = (alpha_low + alpha_high) / 2
            all_feasible = True
            for z in samples:
                x = self.x_eq + np.sqrt(alpha_mid) * P_inv_sqrt @ z
                if not constraint_fn(x):
                    all_feasible = False
                    break
            if all_feasible:
                alpha_low = alpha_mid
            else:
                alpha_high = alpha_mid
        self.alpha = alpha_low * (1 - self.config.constraint_margin)
        return self.alpha

    def contains(self, x) -> bool:
        if self.P is None:
            return False
        dx = x - self.x_eq
        value = dx.T @ self.P @ dx
        return value <= self.alpha

    def get_value(self, x) -> float:
        if self.P is None:
            return np.inf
        dx = x - self.x_eq
        return float(dx.T @ self.P @ dx)

    def project(self, x) -> np.ndarray:
        """x itself inside the set, else x_eq + sqrt(alpha / V) (x - x_eq)."""
        if self.P is None:
            return x
        dx = x - self.x_eq
        value = dx.T @ self.P @ dx
        if value <= self.alpha:
            return x
        scale = np.sqrt(self.alpha / value)
        return self.x_eq + scale * dx

    def get_boundary_points(self, n_points: int = 100) -> np.ndarray:
        if self.P is None:
            return np.zeros((0, self.n_x))
        samples = np.random.randn(n_points, self.n_x)
        samples = samples / np.linalg.norm(samples, axis=1, keepdims=True)
        try:
            L = np.linalg.cholesky(np.linalg.inv(self.P))
            boundary = self.x_eq + np.sqrt(self.alpha) * (samples @ L.T)
        except np.linalg.LinAlgError:
            boundary = self.x_eq + np.sqrt(self.alpha) * samples
        return boundary


class TubeController:
    """x+ = (A + B K) x + w: the tube gain, a box bound of the robust positive invariant set
    (the geometric series of |A_cl|^k on the disturbance box) and the tightening it implies."""

    def __init__(self, A, B, config: Optional[InvariantSetConfig] = None):
        self.A = A
        self.B = B
        self.n_x = A.shape[0]
        self.n_u = B.shape[1]
        self.config = config or InvariantSetConfig()
        self.K: Optional[np.ndarray] = None
        self.A_cl: Optional[np.ndarray] = None
        self.rpi_set: Optional[np.ndarray] = None

    def compute_tube_gain(self, Q=None, R=None) -> np.ndarray:
        if Q is None:
            Q = np.eye(self.n_x)
        if R is None:
            R = np.eye(self.n_u)
        if HAS_SCIPY:
            try:
                P = solve_discrete_are(self.A, self.B, Q, R)
                BtP = self.B.T @ P
                self.K = -np.linalg.solve(R + BtP @ self.B, BtP @ self.A)
            except Exception:
                self.K = -0.1 * np.linalg.pinv(self.B) @ self.A
        else:
            self.K = -0.1 * np.linalg.pinv(self.B) @ self.A
        self.A_cl = self.A + self.B @ self.K
        return self.K

    def compute_rpi_set(self, W, n_iterations: int = 20) -> np.ndarray:
        """W: the disturbance box's half widths, or a matrix whose diagonal gives them."""
        if self.A_cl is None:
            raise RuntimeError("Must call compute_tube_gain first")
        w_bounds = W if W.ndim == 1 else np.abs(np.diag(W))
        rpi_bounds = w_bounds.copy()
        A_pow = self.A_cl.copy()
        for _ in range(n_iterations):
            rpi_bounds += np.abs(A_pow) @ w_bounds
            A_pow = A_pow @ self.A_cl
            if np.max(np.abs(A_pow)) < 1e-10:
                break
        self.rpi_set = rpi_bounds
        return rpi_bounds

    def get_constraint_tightening(self) -> np.ndarray:
        if self.rpi_set is None:
            return np.zeros(self.n_x)
        return self.rpi_set * (1 + self.config.constraint_margin)

    def get_control(self, x, x_nominal) -> np.ndarray:
        if self.K is None:
            return np.zeros(self.n_u)
        return self.K @ (x - x_nominal)


class PolytopeInvariantSet:
    """S = {x : H x <= h}."""

    def __init__(self):
        self.H: Optional[np.ndarray] = None
        self.h: Optional[np.ndarray] = None

    def from_box(self, x_min, x_max) -> None:
        n = len(x_min)
        self.H = np.vstack([np.eye(n), -np.eye(n)])
        self.h = np.concatenate([x_max, -x_min])

    def contains(self, x) -> bool:
        if self.H is None:
            return False
        return np.all(self.H @ x <= self.h)

    def get_violations(self, x) -> np.ndarray:
        """H x - h (positive = violated)."""
        if self.H is None:
            return np.array([])
        return self.H @ x - self.h


def compute_lmi_invariant_set(A, B, K, state_bounds: Optional[Tuple[np.ndarray, np.ndarray]] = None):
    """-> (P, alpha): P from the discrete Lyapunov equation of A + B K with Q = I (identity
    when it fails), alpha = 0.9 of the smallest positive corner value over the first 100
    corners of the state box (1.0 without a box)."""
    A_cl = A + B @ K
    n_x = A.shape[0]
    Q = np.eye(n_x)
    if HAS_SCIPY:
        try:
            P = solve_discrete_lyapunov(A_cl.T, Q)
        except Exception:
            P = np.eye(n_x)
    else:
        P = np.eye(n_x)
    alpha = 1.0
    if state_bounds is not None:
        x_min, x_max = state_bounds
        # the reference lists all 2^n corners and reads the first 100; the same 100 are built here
        n_corners = min(100, 2 ** n_x)
        min_alpha = np.inf
        for i in range(n_corners):
            corner = np.array([x_min[j] if (i >> j) & 1 else x_max[j] for j in range(n_x)])
            val = corner.T @ P @ corner
            if val > 0:
                min_alpha = min(min_alpha, val)
        if min_alpha < np.inf:
            alpha = min_alpha * 0.9
    return P, alpha
