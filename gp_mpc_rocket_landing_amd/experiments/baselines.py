"""Baseline controllers of the comparison studies (reference src/experiments/baselines.py):
LQR about hover, a PID, open-loop replay and two thin wrappers, with the reference's names,
signatures, defaults and numpy statements in its order, so the host path gives its bits.

``MonteCarloSimulator.run``, ``compare_controllers`` and ``DispersionAnalysis.run_single`` fly
whole batches of landings under ``LQRController``, ``PIDController`` and ``OpenLoopController``
in one device call (csrc/baseline.hip); ``solve`` here is what the
per-landing loop calls and what that kernel restates.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
from scipy import linalg


@dataclass
class LQRConfig:
    """baselines.py:24-39."""
    Q_pos: float = 10.0
    Q_vel: float = 1.0
    Q_mass: float = 0.01
    R_thrust: float = 0.01
    R_gimbal: float = 0.1
    linearize_at_hover: bool = True
    use_gain_scheduling: bool = False


@dataclass
class LQRSolution:
    u0: np.ndarray
    K: np.ndarray
    cost_to_go: float = 0.0


class LQRController:
    """baselines.py:51-223: infinite-horizon discrete LQR of the forward-difference
    linearisation at (x_target, hover), hand-tuned gains when the Riccati solve raises."""

    def __init__(self, dynamics, config: Optional[LQRConfig] = None):
        self.dynamics = dynamics
        self.config = config or LQRConfig()
        self.n_x = getattr(dynamics, "n_x", 7)
        self.n_u = getattr(dynamics, "n_u", 3)
        self.x_target: Optional[np.ndarray] = None
        self.K: Optional[np.ndarray] = None
        self.u_hover: Optional[np.ndarray] = None
        self._initialized = False

    def initialize(self, x0, x_target) -> None:
        self.x_target = x_target.copy()
        g = getattr(self.dynamics.params, "g", 1.0) if hasattr(self.dynamics, "params") else 1.0
        mass = x0[0]
        self.u_hover = np.array([mass * g, 0.0, 0.0])
        A, B = self._linearize(x_target, self.u_hover)
        Q = self._build_Q()
        R = self._build_R()
        try:
            P = linalg.solve_discrete_are(A, B, Q, R)
            self.K = np.linalg.inv(R + B.T @ P @ B) @ B.T @ P @ A
        except Exception:
            # altitude is state 1 and the vertical rate state 4; thrust components steer y and z
            K = np.zeros((self.n_u, self.n_x))
            K[0, 1] = -1.0
            K[0, 4] = -2.0
            K[1, 2] = 0.2
            K[1, 5] = 0.5
            K[2, 3] = 0.2
            K[2, 6] = 0.5
            self.K = K
        self._initialized = True

    def _linearize(self, x, u, eps: float = 1e-6) -> Tuple[np.ndarray, np.ndarray]:
        dt = 0.1   # the reference's own step, whatever the simulation's
        A = np.zeros((self.n_x, self.n_x))
        B = np.zeros((self.n_x, self.n_u))
        x_nom = self.dynamics.step(x, u, dt)
        for i in range(self.n_x):
            x_pert = x.copy()
            x_pert[i] += eps
            A[:, i] = (self.dynamics.step(x_pert, u, dt) - x_nom) / eps
        for i in range(self.n_u):
            u_pert = u.copy()
            u_pert[i] += eps
            B[:, i] = (self.dynamics.step(x, u_pert, dt) - x_nom) / eps
        return A, B

    def _build_Q(self) -> np.ndarray:
        c = self.config
        return np.diag([c.Q_mass, c.Q_pos, c.Q_pos, c.Q_pos, c.Q_vel, c.Q_vel, c.Q_vel][: self.n_x])

    def _build_R(self) -> np.ndarray:
        c = self.config
        return np.diag([c.R_thrust, c.R_gimbal, c.R_gimbal][: self.n_u])

    def clips(self) -> Tuple[float, float, float]:
        """(T_min, T_max, gimbal_max) as ``solve`` reads them (the device call's clips)."""
        if hasattr(self.dynamics, "params"):
            p = self.dynamics.params
            return getattr(p, "T_min", 0.1), getattr(p, "T_max", 10.0), getattr(p, "gimbal_max", 0.5)
        return 0.1, 10.0, 0.5

    def solve(self, x, x_target=None) -> LQRSolution:
        if not self._initialized:
            raise RuntimeError("Controller not initialized")
        target = x_target if x_target is not None else self.x_target
        dx = x - target
        du = -self.K @ dx
        u = self.u_hover.copy()
        u += du
        if hasattr(self.dynamics, "params"):
            params = self.dynamics.params
            u[0] = np.clip(u[0], getattr(params, "T_min", 0.1), getattr(params, "T_max", 10.0))
            gimbal_max = getattr(params, "gimbal_max", 0.5)
            u[1:] = np.clip(u[1:], -gimbal_max, gimbal_max)
        else:
            u[0] = np.clip(u[0], 0.1, 10.0)
            u[1:] = np.clip(u[1:], -0.5, 0.5)
        return LQRSolution(u0=u, K=self.K)


@dataclass
class PIDConfig:
    """baselines.py:226-246."""
    Kp_z: float = 2.0
    Ki_z: float = 0.1
    Kd_z: float = 1.5
    Kp_xy: float = 0.5
    Ki_xy: float = 0.01
    Kd_xy: float = 0.3
    max_integral: float = 10.0
    thrust_min: float = 0.3
    thrust_max: float = 5.0
    gimbal_max: float = 0.35


@dataclass
class PIDSolution:
    u0: np.ndarray
    error: np.ndarray = field(default_factory=lambda: np.zeros(3))


class PIDController:
    """baselines.py:257-355: position PID with the derivative taken from the velocity error;
    state 1 is the altitude, so the first thrust component carries gravity."""

    def __init__(self, dynamics, config: Optional[PIDConfig] = None):
        self.dynamics = dynamics
        self.config = config or PIDConfig()
        self.n_x = getattr(dynamics, "n_x", 7)
        self.n_u = getattr(dynamics, "n_u", 3)
        self.x_target: Optional[np.ndarray] = None
        self.integral_error = np.zeros(3)
        self.prev_error = np.zeros(3)
        self.dt = 0.1   # its own step, whatever the simulation's
        if hasattr(dynamics, "params"):
            self.g = getattr(dynamics.params, "g", 1.0)
        else:
            self.g = 1.0

    def initialize(self, x0, x_target) -> None:
        self.x_target = x_target.copy()
        self.integral_error = np.zeros(3)
        self.prev_error = np.zeros(3)

    def solve(self, x, x_target=None) -> PIDSolution:
        target = x_target if x_target is not None else self.x_target
        cfg = self.config
        pos = x[1:4]
        vel = x[4:7]
        pos_error = target[1:4] - pos
        vel_error = target[4:7] - vel
        self.integral_error += pos_error * self.dt
        self.integral_error = np.clip(self.integral_error, -cfg.max_integral, cfg.max_integral)
        error_derivative = vel_error
        thrust_vert = cfg.Kp_z * pos_error[0] + cfg.Ki_z * self.integral_error[0] + cfg.Kd_z * error_derivative[0]
        mass = x[0]
        thrust_x = mass * (self.g + thrust_vert)
        thrust_x = np.clip(thrust_x, cfg.thrust_min, cfg.thrust_max)
        thrust_y = cfg.Kp_xy * pos_error[1] + cfg.Ki_xy * self.integral_error[1] + cfg.Kd_xy * error_derivative[1]
        thrust_z = cfg.Kp_xy * pos_error[2] + cfg.Ki_xy * self.integral_error[2] + cfg.Kd_xy * error_derivative[2]
        thrust_y = thrust_y * mass
        thrust_z = thrust_z * mass
        thrust_y = np.clip(thrust_y, -cfg.thrust_max * 0.3, cfg.thrust_max * 0.3)
        thrust_z = np.clip(thrust_z, -cfg.thrust_max * 0.3, cfg.thrust_max * 0.3)
        u = np.array([thrust_x, thrust_y, thrust_z])
        self.prev_error = pos_error.copy()
        return PIDSolution(u0=u, error=pos_error)


class NominalMPCWrapper:
    """baselines.py:358-383: NominalMPC behind the baselines' interface (host only)."""

    def __init__(self, mpc_controller):
        self.mpc = mpc_controller
        self.x_target = None

    def initialize(self, x0, x_target) -> None:
        self.x_target = x_target.copy()
        if hasattr(self.mpc, "initialize"):
            self.mpc.initialize(x0, x_target)

    def solve(self, x, x_target=None) -> Any:
        target = x_target if x_target is not None else self.x_target
        if hasattr(self.mpc, "step"):
            return self.mpc.step(x)
        return self.mpc.solve(x, target)


class _OpenLoopSolution:
    def __init__(self, u):
        self.u0 = u


class OpenLoopController:
    """baselines.py:386-431: replays reference_controls, holding the last row."""

    def __init__(self, reference_states, reference_controls, dt: float = 0.1):
        self.X_ref = reference_states
        self.U_ref = reference_controls
        self.dt = dt
        self.t = 0.0
        self.step_idx = 0

    def initialize(self, x0, x_target) -> None:
        self.t = 0.0
        self.step_idx = 0

    def solve(self, x, x_target=None) -> Any:
        idx = min(self.step_idx, len(self.U_ref) - 1)
        u = self.U_ref[idx].copy()
        self.step_idx += 1
        self.t += self.dt
        return _OpenLoopSolution(u)


class TubeMPCWrapper:
    """baselines.py:434-455: Tube-MPC behind the baselines' interface (host only)."""

    def __init__(self, tube_mpc_controller):
        self.tube_mpc = tube_mpc_controller
        self.x_target = None

    def initialize(self, x0, x_target) -> None:
        self.x_target = x_target.copy()
        if hasattr(self.tube_mpc, "initialize"):
            self.tube_mpc.initialize(x0, x_target)

    def solve(self, x, x_target=None) -> Any:
        target = x_target if x_target is not None else self.x_target
        return self.tube_mpc.solve(x, target)


def create_baseline_controllers(dynamics, mpc_config=None,
                                reference_trajectory: Optional[Tuple[np.ndarray, np.ndarray]] = None
                                ) -> Dict[str, Any]:
    """baselines.py:458-497: "LQR", "PID", "Nominal_MPC" with an mpc_config, "Open_Loop" with
    a reference trajectory (states, controls)."""
    baselines: Dict[str, Any] = {}
    baselines["LQR"] = LQRController(dynamics)
    baselines["PID"] = PIDController(dynamics)
    if mpc_config is not None:
        try:
            from ..mpc import NominalMPC3DoF
            baselines["Nominal_MPC"] = NominalMPCWrapper(NominalMPC3DoF(dynamics, mpc_config))
        except ImportError:
            pass
    if reference_trajectory is not None:
        states, controls = reference_trajectory
        baselines["Open_Loop"] = OpenLoopController(states, controls)
    return baselines


@dataclass
class BaselineComparison:
    """baselines.py:500-530."""
    controller_names: List[str]
    success_rates: Dict[str, float]
    fuel_means: Dict[str, float]
    fuel_stds: Dict[str, float]
    time_means: Dict[str, float]
    compute_means: Dict[str, float]

    def to_table(self) -> str:
        lines = ["Controller Comparison Results", "=" * 80,
                 f"{'Controller':<20} {'Success%':>10} {'Fuel (kg)':>15} {'Time (s)':>12} {'Compute (ms)':>15}",
                 "-" * 80]
        for name in self.controller_names:
            success = self.success_rates.get(name, 0) * 100
            fuel = self.fuel_means.get(name, 0)
            fuel_std = self.fuel_stds.get(name, 0)
            time = self.time_means.get(name, 0)
            compute = self.compute_means.get(name, 0)
            lines.append(f"{name:<20} {success:>9.1f}% {fuel:>7.3f}±{fuel_std:<6.3f} {time:>11.2f} {compute:>14.2f}")
        lines.append("=" * 80)
        return "\n".join(lines)


# ---- the device batch (csrc/baseline.hip) -------------------------------------------------------
KIND_LQR, KIND_PID, KIND_OPEN_LOOP = 0, 1, 2


def device_gate(controller) -> Tuple[Optional[int], str]:
    """(controller kind, "") when ``controller`` is one the device kernel restates, else
    (None, reason).  Host logic only."""
    from ..dynamics.rocket_3dof import Rocket3DoFDynamics
    t = type(controller)
    if t is OpenLoopController:
        if len(controller.U_ref) < 1:
            return None, "the open-loop table is empty"
        return KIND_OPEN_LOOP, ""
    if t is not LQRController and t is not PIDController:
        return None, "the controller is not this package's LQRController, PIDController or OpenLoopController"
    if type(controller.dynamics) is not Rocket3DoFDynamics:
        return None, "the controller's own dynamics is not a plain Rocket3DoFDynamics"
    return (KIND_LQR if t is LQRController else KIND_PID), ""


def controller_batch(controller, kind: int, x0s) -> Dict[str, Any]:
    """What the device call takes from the controller for the landings ``x0s``: the
    keyword arguments of ``_lib.baseline_fly``.  An LQR is initialised once per landing, as
    ``run_single`` does (K and u_hover depend on the initial mass)."""
    n = len(x0s)
    kw: Dict[str, Any] = dict(kind=kind)
    if kind == KIND_LQR:
        K = np.zeros((n, 3, 7))
        uh = np.zeros((n, 3))
        for i, x0 in enumerate(x0s):
            x_target = np.zeros(7)
            x_target[0] = x0[0]
            controller.initialize(x0, x_target)
            K[i] = controller.K
            uh[i] = controller.u_hover
        lo, hi, gm = controller.clips()
        kw.update(K=K, u_hover=uh, T_lo=lo, T_hi=hi, gimbal_max=gm)
    elif kind == KIND_PID:
        c = controller.config
        kw.update(pid=dict(Kp_z=c.Kp_z, Ki_z=c.Ki_z, Kd_z=c.Kd_z, Kp_xy=c.Kp_xy, Ki_xy=c.Ki_xy, Kd_xy=c.Kd_xy,
                           max_integral=c.max_integral, thrust_min=c.thrust_min, thrust_max=c.thrust_max,
                           pid_dt=controller.dt, pid_g=controller.g))
    else:
        kw.update(U_ref=np.array(controller.U_ref, dtype=float).reshape(-1, 3))
    return kw
