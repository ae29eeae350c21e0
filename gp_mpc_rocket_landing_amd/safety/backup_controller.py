"""Backup controllers of the predictive safety filter (mirror of the reference's
src/safety/backup_controller.py by name, signature, default and return value; host numpy).

The backup law is u = u_eq - K (x - x_eq), saturated to the configured box; V(x) =
(x - x_eq)' P (x - x_eq) is its Lyapunov value and shapes the invariant set.

``LQRBackupController.compute_gains`` tries the discrete Riccati equation on
``dynamics.linearize(x_eq, u_eq, dt)`` = (I + A_c dt, B_c dt).  For the 14-state rocket the
mass and the quaternion's scalar part sit on the unit circle and are uncontrollable, so
``scipy.linalg.solve_discrete_are`` raises; the reference then prints a message and takes the
PD gains (2.0 on position, 1.0 on velocity, P = Q).  That behaviour is kept, message included.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

try:
    from scipy.linalg import solve_discrete_are

    HAS_SCIPY = True
except ImportError:  # pragma: no cover
    HAS_SCIPY = False


@dataclass
class BackupControllerConfig:
    """LQR weight diagonals (None: the defaults below), the control box, dt and the type."""

    Q_diag: Optional[np.ndarray] = None
    R_diag: Optional[np.ndarray] = None
    u_min: Optional[np.ndarray] = None
    u_max: Optional[np.ndarray] = None
    dt: float = 0.1
    controller_type: str = "lqr"  # "lqr", "pd", "emergency"


class LQRBackupController:
    """u = u_eq - K (x - x_eq) around the hover equilibrium.

    >>> backup = LQRBackupController(dynamics, config)
    >>> backup.compute_gains(x_eq, u_eq)
    >>> u_backup = backup.get_control(x)
    """

    def __init__(self, dynamics, config: Optional[BackupControllerConfig] = None):
        self.dynamics = dynamics
        self.config = config or BackupControllerConfig()
        self.n_x = 14
        self.n_u = 3
        self.x_eq: Optional[np.ndarray] = None
        self.u_eq: Optional[np.ndarray] = None
        self.K: Optional[np.ndarray] = None
        self.P: Optional[np.ndarray] = None
        self._setup_weights()

    def _setup_weights(self) -> None:
        """Q: nothing on the mass, 10 on position, 5 on velocity, (1, 2, 2, 1) on the
        quaternion, 0.5 on the rates; R = 0.1 I."""
        if self.config.Q_diag is not None:
            self.Q = np.diag(self.config.Q_diag)
        else:
            self.Q = np.diag(np.array([0.0, 10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 1.0, 2.0, 2.0, 1.0, 0.5, 0.5, 0.5]))
        if self.config.R_diag is not None:
            self.R = np.diag(self.config.R_diag)
        else:
            self.R = np.diag([0.1, 0.1, 0.1])

    def compute_gains(self, x_eq, u_eq=None) -> None:
        """Gains around (x_eq, u_eq); without u_eq the hover thrust [m g, 0, 0]."""
        self.x_eq = x_eq.copy()
        if u_eq is None:
            mass = x_eq[0]
            g = abs(self.dynamics.params.g_I[0] * self.dynamics.params.g0)
            self.u_eq = np.array([mass * g, 0.0, 0.0])
        else:
            self.u_eq = u_eq.copy()
        A, B = self._linearize_at_equilibrium()
        if HAS_SCIPY:
            try:
                self.P = solve_discrete_are(A, B, self.Q, self.R)
                BtP = B.T @ self.P
                self.K = np.linalg.solve(self.R + BtP @ B, BtP @ A)
            except Exception as e:
                print(f"LQR computation failed: {e}, using simple PD gains")
                self._compute_pd_gains()
        else:
            self._compute_pd_gains()

    def _linearize_at_equilibrium(self) -> Tuple[np.ndarray, np.ndarray]:
        if hasattr(self.dynamics, "linearize"):
            return self.dynamics.linearize(self.x_eq, self.u_eq, self.config.dt)
        return self._numerical_linearization()

    def _numerical_linearization(self, eps: float = 1e-6) -> Tuple[np.ndarray, np.ndarray]:
        """Forward differences of ``dynamics.step`` at the equilibrium."""
        A = np.zeros((self.n_x, self.n_x))
        B = np.zeros((self.n_x, self.n_u))
        x_next_nom = self.dynamics.step(self.x_eq, self.u_eq, self.config.dt)
        for i in range(self.n_x):
            x_pert = self.x_eq.copy()
            x_pert[i] += eps
            A[:, i] = (self.dynamics.step(x_pert, self.u_eq, self.config.dt) - x_next_nom) / eps
        for i in range(self.n_u):
            u_pert = self.u_eq.copy()
            u_pert[i] += eps
            B[:, i] = (self.dynamics.step(self.x_eq, u_pert, self.config.dt) - x_next_nom) / eps
        return A, B

    def _compute_pd_gains(self) -> None:
        """The fallback: position -> thrust 2.0, velocity -> thrust 1.0, P = Q."""
        self.K = np.zeros((self.n_u, self.n_x))
        for i in range(3):
            self.K[i, 1 + i] = 2.0
            self.K[i, 4 + i] = 1.0
        self.P = self.Q.copy()

    def get_control(self, x) -> np.ndarray:
        """The backup control at x, saturated to [u_min, u_max] where set."""
        if self.K is None:
            raise RuntimeError("Must call compute_gains() first")
        dx = x - self.x_eq
        u = self.u_eq - self.K @ dx
        if self.config.u_min is not None:
            u = np.maximum(u, self.config.u_min)
        if self.config.u_max is not None:
            u = np.minimum(u, self.config.u_max)
        return u

    def get_control_batch(self, X) -> np.ndarray:
        return np.array([self.get_control(x) for x in X])

    def get_value_function(self, x) -> float:
        """V(x) = (x - x_eq)' P (x - x_eq)."""
        if self.P is None:
            raise RuntimeError("Must call compute_gains() first")
        dx = x - self.x_eq
        return float(dx.T @ self.P @ dx)

    def simulate_backup(self, x0, n_steps: int = 50) -> Tuple[np.ndarray, np.ndarray]:
        """-> X (n_steps + 1, n_x), U (n_steps, n_u) under the backup law."""
        X = np.zeros((n_steps + 1, self.n_x))
        U = np.zeros((n_steps, self.n_u))
        X[0] = x0
        for k in range(n_steps):
            U[k] = self.get_control(X[k])
            X[k + 1] = self.dynamics.step(X[k], U[k], self.config.dt)
        return X, U


def _clamp_norm(u, T_min, T_max):
    """Scale u onto the thrust shell [T_min, T_max] (the lower side divides by max(|u|, 1e-6))."""
    T_mag = np.linalg.norm(u)
    if T_mag < T_min:
        u = u / max(T_mag, 1e-6) * T_min
    elif T_mag > T_max:
        u = u / T_mag * T_max
    return u


class PDBackupController:
    """u = Kp (x_target - r) - Kd v + gravity compensation, clamped to the thrust shell of
    ``dynamics.params`` (defaults 0.5, 5.0)."""

    def __init__(self, dynamics, Kp: float = 2.0, Kd: float = 1.0):
        self.dynamics = dynamics
        self.Kp = Kp
        self.Kd = Kd
        self.n_x = 14
        self.n_u = 3
        self.x_target = np.zeros(3)

    def get_control(self, x) -> np.ndarray:
        mass = x[0]
        pos = x[1:4]
        vel = x[4:7]
        g = abs(self.dynamics.params.g_I[0] * self.dynamics.params.g0)
        u = np.zeros(3)
        u[0] = mass * g + self.Kp * (self.x_target[0] - pos[0]) - self.Kd * vel[0]
        u[1] = self.Kp * (self.x_target[1] - pos[1]) - self.Kd * vel[1]
        u[2] = self.Kp * (self.x_target[2] - pos[2]) - self.Kd * vel[2]
        return _clamp_norm(u, getattr(self.dynamics.params, "T_min", 0.5), getattr(self.dynamics.params, "T_max", 5.0))


class EmergencyBrakingController:
    """Full thrust against the velocity on top of the gravity compensation; below 0.1 of
    speed the hover thrust alone."""

    def __init__(self, dynamics):
        self.dynamics = dynamics
        self.T_max = getattr(dynamics.params, "T_max", 5.0)

    def get_control(self, x) -> np.ndarray:
        mass = x[0]
        vel = x[4:7]
        g = abs(self.dynamics.params.g_I[0] * self.dynamics.params.g0)
        v_mag = np.linalg.norm(vel)
        if v_mag < 0.1:
            return np.array([mass * g, 0.0, 0.0])
        brake_dir = -vel / v_mag
        T_brake = self.T_max - mass * g
        if T_brake > 0:
            return np.array([mass * g, 0.0, 0.0]) + T_brake * brake_dir
        return np.array([self.T_max, 0.0, 0.0])


def create_backup_controller(dynamics, controller_type: str = "lqr", config: Optional[BackupControllerConfig] = None):
    """"lqr", "pd" or "emergency"."""
    config = config or BackupControllerConfig()
    config.controller_type = controller_type
    if controller_type == "lqr":
        return LQRBackupController(dynamics, config)
    if controller_type == "pd":
        return PDBackupController(dynamics)
    if controller_type == "emergency":
        return EmergencyBrakingController(dynamics)
    raise ValueError(f"Unknown controller type: {controller_type}")
