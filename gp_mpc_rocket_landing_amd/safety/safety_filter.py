"""Predictive safety filter (mirror of the reference's src/safety/safety_filter.py by name,
signature, default and return value; Wabersich & Zeilinger 2021).

A nominal control u is safe at x when (x, u) meets the constraints, the trajectory "u for
one step, then the backup controller" meets them along the way, and its terminal state lies
inside the backup ellipsoid.  An unsafe u is replaced by the result of at most 50 projected
gradient steps on V(x_N(u)) + |u - u_nom|^2 with forward-difference gradients (the reference's
``_solve_gradient_qp``, the path it takes without CasADi; the CasADi / IPOPT path is not
restated).  ``tube_propagator`` is None: ``filter`` never reads it (the tubes are
``tube_mpc.TubePropagator``'s).

Additions: ``filter_batch`` and ``simulate_filtered_batch`` answer B queries (B closed loops)
in one call, and every call is dispatched.  With ``Rocket6DoFDynamics``, an
``LQRBackupController`` with gains, the invariant set built from it and 1 <= N <= 31 the whole
filter runs in one device call (csrc/safety.hip: a quad of lanes per query); otherwise, or
with ``GPMPC_SAFETY=host``, the numpy path below runs, which is the reference's arithmetic
statement for statement (``dynamics.step``, ``K @ dx``, ``dx.T @ P @ dx``) and so returns its
bits.  ``last_path`` ("device" / "host") and ``last_reason`` say what ran and why.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from .backup_controller import BackupControllerConfig, LQRBackupController
from .invariant_sets import EllipsoidalInvariantSet, InvariantSetConfig

HAS_CASADI = False      # the CasADi / IPOPT path of _solve_safety_qp is not restated
MASK_WIDTH = 31         # path_k bits of violation_mask (bit 0: "immediate"), so N <= 31


def safety_mode() -> str:
    """GPMPC_SAFETY: "host", "device" or "" (both of the latter: the device where it applies)."""
    mode = os.environ.get("GPMPC_SAFETY", "").strip().lower()
    if mode not in ("", "host", "device"):
        raise ValueError(f"GPMPC_SAFETY={mode!r}: expected host or device")
    return mode


def rocket_gate(dynamics) -> Optional[str]:
    """None when csrc/fleet6.h's R6Rocket can express the plant (this package's
    ``Rocket6DoFDynamics`` itself, with an invertible inertia tensor), else why not.  The gate the
    safety filter and the tube propagator share."""
    from ..dynamics.rocket_6dof import Rocket6DoFDynamics
    if type(dynamics) is not Rocket6DoFDynamics:
        return "the dynamics is not Rocket6DoFDynamics"
    if not dynamics.matches_device_model():
        return "the rocket is not one the device model runs"
    return None


def rocket_vector(dynamics) -> np.ndarray:
    """The rocket's 17 doubles as the library takes them: J_B (9), r_T_B (3), g_I (3), alpha, g0."""
    p = dynamics.params
    return np.concatenate([np.asarray(p.J_B, float).reshape(9), np.asarray(p.r_T_B, float).reshape(3),
                           np.asarray(p.g_I, float).reshape(3), [float(p.alpha), float(p.g0)]])


@dataclass
class SafetyFilterConfig:
    N: int = 10
    dt: float = 0.1
    backup_type: str = "ellipsoid"  # "ellipsoid", "polytope"
    backup_margin: float = 0.9
    use_gp_uncertainty: bool = True
    gp_confidence: float = 0.95
    qp_max_iter: int = 50
    qp_tol: float = 1e-6
    filter_mode: str = "soft"  # "hard", "soft"
    soft_weight: float = 1e3


@dataclass
class SafetyFilterResult:
    u_safe: np.ndarray
    u_nominal: np.ndarray
    is_modified: bool
    is_safe: bool
    safety_margin: float
    solve_time: float
    backup_value: float
    constraint_violations: Dict[str, float]


def violations_to_mask(violations: Dict[str, float]) -> int:
    """bit 0: "immediate"; bit 1 + k: "path_k"."""
    mask = 1 if "immediate" in violations else 0
    for key in violations:
        if key.startswith("path_"):
            mask |= 1 << (1 + int(key[5:]))
    return mask


def mask_to_violations(mask: int, safety_margin: float) -> Dict[str, float]:
    """The reference's dictionary, in its key order."""
    out: Dict[str, float] = {}
    if mask & 1:
        out["immediate"] = -1.0
    out["terminal"] = safety_margin
    for k in range(MASK_WIDTH):
        if mask >> (1 + k) & 1:
            out[f"path_{k}"] = -1.0
    return out


@dataclass
class SafetyFilterBatch:
    """``filter_batch``'s answer: one row per query.  ``iterations``: the gradient steps taken
    (0 when unmodified, or when the terminal value was already inside the margin)."""

    u_safe: np.ndarray          # (B, 3)
    u_nominal: np.ndarray       # (B, 3)
    is_modified: np.ndarray     # (B,) bool
    is_safe: np.ndarray         # (B,) bool
    safety_margin: np.ndarray   # (B,)
    backup_value: np.ndarray    # (B,)
    violation_mask: np.ndarray  # (B,) int64
    iterations: np.ndarray      # (B,) int32
    solve_time: float

    def __len__(self) -> int:
        return len(self.u_safe)

    def result(self, i: int) -> SafetyFilterResult:
        margin = float(self.safety_margin[i])
        return SafetyFilterResult(
            u_safe=self.u_safe[i].copy(), u_nominal=self.u_nominal[i].copy(), is_modified=bool(self.is_modified[i]),
            is_safe=bool(self.is_safe[i]), safety_margin=margin, solve_time=self.solve_time,
            backup_value=float(self.backup_value[i]),
            constraint_violations=mask_to_violations(int(self.violation_mask[i]), margin))


@dataclass
class SafetySimulationBatch:
    """The per-step fields of ``simulate_filtered_batch``, each (B, T)."""

    is_modified: np.ndarray
    is_safe: np.ndarray
    safety_margin: np.ndarray
    iterations: np.ndarray
    solve_time: float


class PredictiveSafetyFilter:
    """
    >>> safety = PredictiveSafetyFilter(dynamics, config)
    >>> safety.initialize(x_eq)
    >>> u_apply = safety.filter(x, u_mpc).u_safe
    """

    def __init__(self, dynamics, config: Optional[SafetyFilterConfig] = None, constraint_params=None):
        self.dynamics = dynamics
        self.config = config or SafetyFilterConfig()
        self.constraint_params = constraint_params
        self.n_x = 14
        self.n_u = 3
        self.backup = LQRBackupController(dynamics, BackupControllerConfig(dt=self.config.dt))
        self.invariant_set = EllipsoidalInvariantSet(self.n_x, InvariantSetConfig())
        self.tube_propagator = None  # as in the reference: filter() never reads it (tube_mpc.TubePropagator)
        self._gp_model = None
        self._initialized = False
        self.ctx = None              # a _lib.Context; None: the default context
        self.last_path: Optional[str] = None
        self.last_reason: Optional[str] = None
        self._last_iterations = 0

    def initialize(self, x_eq, u_eq=None, backup_alpha: Optional[float] = None) -> None:
        """Backup gains at (x_eq, u_eq), the ellipsoid from them; without ``backup_alpha`` and
        with constraint parameters, the sampled maximal alpha."""
        self.backup.compute_gains(x_eq, u_eq)
        self.invariant_set.compute_from_lqr(self.backup.P, x_eq, backup_alpha)
        if backup_alpha is None and self.constraint_params is not None:

            def constraint_check(x):
                return self._check_constraints(x, self.backup.get_control(x))

            self.invariant_set.compute_maximal_alpha(constraint_check)
        self._initialized = True

    def set_gp_model(self, gp_model) -> None:
        self._gp_model = gp_model

    # ---- the reference's arithmetic (host) ---------------------------------------------
    def _filter_host(self, x, u_nominal) -> SafetyFilterResult:
        start_time = time.perf_counter()
        self._last_iterations = 0
        is_safe, safety_margin, violations = self._check_safety(x, u_nominal)
        if is_safe:
            return SafetyFilterResult(
                u_safe=u_nominal.copy(), u_nominal=u_nominal.copy(), is_modified=False, is_safe=True,
                safety_margin=safety_margin, solve_time=time.perf_counter() - start_time,
                backup_value=self._get_backup_value(x, u_nominal), constraint_violations=violations)
        u_safe = self._solve_safety_qp(x, u_nominal)
        is_safe_filtered, margin_filtered, violations_filtered = self._check_safety(x, u_safe)
        return SafetyFilterResult(
            u_safe=u_safe, u_nominal=u_nominal.copy(), is_modified=True, is_safe=is_safe_filtered,
            safety_margin=margin_filtered, solve_time=time.perf_counter() - start_time,
            backup_value=self._get_backup_value(x, u_safe), constraint_violations=violations_filtered)

    def _check_safety(self, x, u) -> Tuple[bool, float, Dict[str, float]]:
        """Safe: the immediate constraints hold, the predicted path meets them and ends inside
        the backup set."""
        violations: Dict[str, float] = {}
        constraint_ok = self._check_constraints(x, u)
        if not constraint_ok:
            violations["immediate"] = -1.0
        X_pred = self._predict_with_backup(x, u)
        backup_value = self.invariant_set.get_value(X_pred[-1])
        safety_margin = self.invariant_set.alpha - backup_value
        violations["terminal"] = safety_margin
        for k, x_k in enumerate(X_pred[:-1]):
            u_k = self.backup.get_control(x_k) if k > 0 else u
            if not self._check_constraints(x_k, u_k):
                violations[f"path_{k}"] = -1.0
        is_safe = (constraint_ok and safety_margin > 0
                   and all(v >= 0 for k, v in violations.items() if k.startswith("path")))
        return is_safe, safety_margin, violations

    def _predict_with_backup(self, x, u_first) -> np.ndarray:
        """(N + 1, n_x): the first step with u_first, the rest with the backup controller."""
        N = self.config.N
        dt = self.config.dt
        X_pred = np.zeros((N + 1, self.n_x))
        X_pred[0] = x
        X_pred[1] = self.dynamics.step(x, u_first, dt)
        for k in range(1, N):
            u_backup = self.backup.get_control(X_pred[k])
            X_pred[k + 1] = self.dynamics.step(X_pred[k], u_backup, dt)
        return X_pred

    def _constraint_values(self) -> Tuple[float, float, float, float]:
        """(T_min, T_max, cos theta_max, tan gamma_gs) as _check_constraints reads them:
        ``getattr`` with the reference's defaults, the angles in degrees."""
        cp = self.constraint_params
        return (getattr(cp, "T_min", 0.5), getattr(cp, "T_max", 5.0),
                np.cos(np.deg2rad(getattr(cp, "theta_max", 60.0))), np.tan(np.deg2rad(getattr(cp, "gamma_gs", 30.0))))

    def _check_constraints(self, x, u) -> bool:
        """Thrust shell, tilt (cos theta = 1 - 2 (qx^2 + qy^2)) and, above 0.1 of altitude, the
        glideslope."""
        if self.constraint_params is None:
            return True
        T_mag = np.linalg.norm(u)
        T_min = getattr(self.constraint_params, "T_min", 0.5)
        T_max = getattr(self.constraint_params, "T_max", 5.0)
        if T_mag < T_min or T_mag > T_max:
            return False
        q = x[7:11]
        cos_theta = 1 - 2 * (q[1] ** 2 + q[2] ** 2)
        theta_max = getattr(self.constraint_params, "theta_max", 60.0)
        if cos_theta < np.cos(np.deg2rad(theta_max)):
            return False
        pos = x[1:4]
        gamma = getattr(self.constraint_params, "gamma_gs", 30.0)
        tan_gamma = np.tan(np.deg2rad(gamma))
        if pos[0] > 0.1:  # noqa: SIM102
            if pos[0] ** 2 * tan_gamma**2 < pos[1] ** 2 + pos[2] ** 2:
                return False
        return True

    def _get_backup_value(self, x, u) -> float:
        return self.invariant_set.get_value(self._predict_with_backup(x, u)[-1])

    def _solve_safety_qp(self, x, u_nominal) -> np.ndarray:
        """min |u - u_nom|^2 s.t. V(x_N(u)) <= alpha: the gradient path only."""
        return self._solve_gradient_qp(x, u_nominal)

    def _thrust_shell(self) -> Tuple[float, float]:
        cp = self.constraint_params
        return (getattr(cp, "T_min", 0.5) if cp else 0.5), (getattr(cp, "T_max", 5.0) if cp else 5.0)

    def _solve_gradient_qp(self, x, u_nominal, n_iters: int = 50, lr: float = 0.1) -> np.ndarray:
        """Projected gradient steps on V(x_N(u)) + |u - u_nom|^2 until V <= backup_margin *
        alpha; the steps taken are left in ``_last_iterations``."""
        u = u_nominal.copy()
        self._last_iterations = 0
        for _ in range(n_iters):
            X_pred = self._predict_with_backup(x, u)
            V_terminal = self.invariant_set.get_value(X_pred[-1])
            if V_terminal <= self.invariant_set.alpha * self.config.backup_margin:
                break
            eps = 1e-4
            grad = np.zeros(self.n_u)
            for i in range(self.n_u):
                u_pert = u.copy()
                u_pert[i] += eps
                X_pert = self._predict_with_backup(x, u_pert)
                V_pert = self.invariant_set.get_value(X_pert[-1])
                grad[i] = (V_pert - V_terminal) / eps
            grad_total = grad + 2 * (u - u_nominal)
            u = u - lr * grad_total
            T_min, T_max = self._thrust_shell()
            T_mag = np.linalg.norm(u)
            if T_mag < T_min:
                u = u / max(T_mag, 1e-6) * T_min
            elif T_mag > T_max:
                u = u / T_mag * T_max
            self._last_iterations += 1
        return u

    def _linearize(self, x, u) -> Tuple[np.ndarray, np.ndarray]:
        """Forward differences (1e-6) of ``dynamics.step`` at (x, u)."""
        eps = 1e-6
        dt = self.config.dt
        A = np.zeros((self.n_x, self.n_x))
        B = np.zeros((self.n_x, self.n_u))
        x_next_nom = self.dynamics.step(x, u, dt)
        for i in range(self.n_x):
            x_pert = x.copy()
            x_pert[i] += eps
            A[:, i] = (self.dynamics.step(x_pert, u, dt) - x_next_nom) / eps
        for i in range(self.n_u):
            u_pert = u.copy()
            u_pert[i] += eps
            B[:, i] = (self.dynamics.step(x, u_pert, dt) - x_next_nom) / eps
        return A, B

    # ---- dispatch --------------------------------------------------------------------------
    def _device_gate(self) -> Tuple[bool, str]:
        """(True, why) when the device kernel restates this filter exactly, else (False, why).
        Host logic only: no device call."""
        if safety_mode() == "host":
            return False, "GPMPC_SAFETY=host"
        why = rocket_gate(self.dynamics)
        if why is not None:
            return False, why
        if type(self.backup) is not LQRBackupController:
            return False, "the backup controller is not LQRBackupController"
        b, s = self.backup, self.invariant_set
        if b.K is None or b.P is None or b.x_eq is None or b.u_eq is None:
            return False, "the backup gains are not set"
        if np.shape(b.K) != (3, 14) or np.shape(b.P) != (14, 14):
            return False, "the backup gains are not 3 x 14 and 14 x 14"
        if type(s) is not EllipsoidalInvariantSet or s.P is None or s.x_eq is None or not (
                np.array_equal(s.P, b.P) and np.array_equal(s.x_eq, b.x_eq)):
            return False, "the invariant set's P / x_eq are not the backup controller's"
        if not 1 <= int(self.config.N) <= MASK_WIDTH:
            return False, f"the horizon N = {self.config.N} is outside 1..{MASK_WIDTH}"
        try:
            from .. import _lib  # noqa: F401
        except (ImportError, OSError) as e:
            return False, f"the library does not load: {e}"
        return True, "Rocket6DoFDynamics with the LQR backup controller"

    def _device_config(self):
        """The gpmpc_safety_config of this filter and the rocket's 17 doubles."""
        from .. import _lib
        b = self.backup
        T_min, T_max = self._thrust_shell()
        kw = dict(horizon=int(self.config.N), dt=float(self.config.dt), K=b.K, P=b.P, x_eq=b.x_eq, u_eq=b.u_eq,
                  u_min=np.full(3, -np.inf) if b.config.u_min is None else np.broadcast_to(b.config.u_min, (3,)),
                  u_max=np.full(3, np.inf) if b.config.u_max is None else np.broadcast_to(b.config.u_max, (3,)),
                  alpha=float(self.invariant_set.alpha), backup_margin=float(self.config.backup_margin),
                  T_min=float(T_min), T_max=float(T_max))
        if self.constraint_params is not None:
            _, _, cos_theta_max, tan_gamma = self._constraint_values()
            kw.update(have_constraints=1, cos_theta_max=float(cos_theta_max), tan2_gamma=float(tan_gamma ** 2))
        return _lib.safety_default_config(**kw), rocket_vector(self.dynamics)

    def _context(self):
        from .. import _lib
        return self.ctx if self.ctx is not None else _lib.default_context()

    def _dispatch(self) -> bool:
        if not self._initialized:
            raise RuntimeError("Must call initialize() first")
        ok, why = self._device_gate()
        self.last_path, self.last_reason = ("device" if ok else "host"), why
        return ok

    def filter_batch(self, X, U_nominal) -> SafetyFilterBatch:
        """The filter at B states X (B, 14) with the nominal controls U_nominal (B, 3)."""
        X = np.atleast_2d(np.asarray(X, float))
        U_nominal = np.atleast_2d(np.asarray(U_nominal, float))
        B = len(X)
        if X.shape != (B, self.n_x) or U_nominal.shape != (B, self.n_u):
            raise ValueError(f"filter_batch: shapes X {X.shape}, U_nominal {U_nominal.shape}")
        start_time = time.perf_counter()
        if self._dispatch():
            from .. import _lib
            cfg, rocket = self._device_config()
            u_safe, margin, value, flags, mask, iters = _lib.safety_filter(self._context(), rocket, cfg, X, U_nominal)
            return SafetyFilterBatch(u_safe, U_nominal.copy(), (flags & 1) != 0, (flags & 2) != 0, margin, value,
                                     mask.astype(np.int64), iters, time.perf_counter() - start_time)
        out = SafetyFilterBatch(np.empty((B, 3)), U_nominal.copy(), np.zeros(B, bool), np.zeros(B, bool), np.empty(B),
                                np.empty(B), np.zeros(B, np.int64), np.zeros(B, np.int32), 0.0)
        for i in range(B):
            r = self._filter_host(X[i], U_nominal[i])
            out.u_safe[i], out.is_modified[i], out.is_safe[i] = r.u_safe, r.is_modified, r.is_safe
            out.safety_margin[i], out.backup_value[i] = r.safety_margin, r.backup_value
            out.violation_mask[i] = violations_to_mask(r.constraint_violations)
            out.iterations[i] = self._last_iterations
        out.solve_time = time.perf_counter() - start_time
        return out

    def filter(self, x, u_nominal) -> SafetyFilterResult:
        """The safe control for the nominal u_nominal at x (``filter_batch`` with B = 1)."""
        if not self._initialized:
            raise RuntimeError("Must call initialize() first")
        return self.filter_batch(np.asarray(x, float)[None], np.asarray(u_nominal, float)[None]).result(0)

    def simulate_filtered(self, x0, U_nominal) -> Tuple[np.ndarray, np.ndarray, List[SafetyFilterResult]]:
        """The closed loop filter -> dynamics.step over the nominal controls U_nominal (T, 3):
        X (T + 1, n_x), U (T, n_u) and every step's result."""
        N = len(U_nominal)
        dt = self.config.dt
        X = np.zeros((N + 1, self.n_x))
        U = np.zeros((N, self.n_u))
        results = []
        X[0] = x0
        for k in range(N):
            result = self.filter(X[k], U_nominal[k])
            U[k] = result.u_safe
            results.append(result)
            X[k + 1] = self.dynamics.step(X[k], U[k], dt)
        return X, U, results

    def simulate_filtered_batch(self, X0, U_nominal) -> Tuple[np.ndarray, np.ndarray, SafetySimulationBatch]:
        """``simulate_filtered`` for B starts X0 (B, 14) with nominal controls U_nominal
        (B, T, 3): X (B, T + 1, 14), U (B, T, 3) and the per-step fields.  On the device the
        whole flight of every start is one call."""
        X0 = np.atleast_2d(np.asarray(X0, float))
        U_nominal = np.asarray(U_nominal, float)
        B = len(X0)
        if U_nominal.ndim != 3 or X0.shape != (B, self.n_x) or U_nominal.shape[::2] != (B, self.n_u):
            raise ValueError(f"simulate_filtered_batch: shapes X0 {X0.shape}, U_nominal {U_nominal.shape}")
        T = U_nominal.shape[1]
        start_time = time.perf_counter()
        if self._dispatch():
            from .. import _lib
            cfg, rocket = self._device_config()
            X, U, margin, flags, iters = _lib.safety_simulate(self._context(), rocket, cfg, X0, U_nominal)
            return X, U, SafetySimulationBatch((flags & 1) != 0, (flags & 2) != 0, margin, iters,
                                               time.perf_counter() - start_time)
        X = np.zeros((B, T + 1, self.n_x))
        U = np.zeros((B, T, self.n_u))
        info = SafetySimulationBatch(np.zeros((B, T), bool), np.zeros((B, T), bool), np.zeros((B, T)),
                                     np.zeros((B, T), np.int32), 0.0)
        X[:, 0] = X0
        for b in range(B):
            for k in range(T):
                r = self._filter_host(X[b, k], U_nominal[b, k])
                U[b, k] = r.u_safe
                info.is_modified[b, k], info.is_safe[b, k] = r.is_modified, r.is_safe
                info.safety_margin[b, k], info.iterations[b, k] = r.safety_margin, self._last_iterations
                X[b, k + 1] = self.dynamics.step(X[b, k], U[b, k], self.config.dt)
        info.solve_time = time.perf_counter() - start_time
        return X, U, info


class SimpleSafetyFilter:
    """Constraint clamping only, no backup controller: the control scaled onto the thrust
    shell [T_min, T_max] of ``constraint_params`` (defaults 0.5, 5.0)."""

    def __init__(self, dynamics, constraint_params=None):
        self.dynamics = dynamics
        self.params = constraint_params

    def filter(self, x, u) -> np.ndarray:  # noqa: ARG002
        u_safe = u.copy()
        T_min = getattr(self.params, "T_min", 0.5) if self.params else 0.5
        T_max = getattr(self.params, "T_max", 5.0) if self.params else 5.0
        T_mag = np.linalg.norm(u_safe)
        if T_mag < T_min:
            u_safe = u_safe / max(T_mag, 1e-6) * T_min
        elif T_mag > T_max:
            u_safe = u_safe / T_mag * T_max
        return u_safe
