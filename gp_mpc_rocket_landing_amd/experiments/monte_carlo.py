"""Monte-Carlo landing protocol, batched and sharded (reference
src/experiments/monte_carlo.py).

The reference runs landings one after another in Python (``n_workers`` is
ignored, monte_carlo.py:617-631).  Here a whole shard of landings advances
together on one GPU (``gp_mpc_rocket_landing_amd.fleet``), shards are
contiguous blocks of landings per rank, and the fixed-size per-landing records
are gathered to rank 0 with one collective (RCCL over xGMI on MI355X).

``MonteCarloSimulator(dynamics, controller, config).run(n_runs, n_workers)`` is the
reference's entry point with its names and signatures.  ``run`` flies the landings
on the device fleet when the caller's objects are exactly what the fleet restates
(``_fleet_plan`` lists every condition; ``last_path`` says which path ran) and
otherwise loops ``run_single`` as the reference does.  DESIGN.md section 12.
"""
from __future__ import annotations

import pickle
import time
from dataclasses import dataclass, field, fields, is_dataclass
from enum import Enum
from typing import Any, Callable, Dict, List, Optional

import numpy as np


class LandingOutcome(Enum):
    """monte_carlo.py:25-33 (enum.auto starts at 1)."""
    SUCCESS = 1
    CRASH = 2
    FUEL_EXHAUSTED = 3
    CONSTRAINT_VIOLATION = 4
    TIMEOUT = 5
    DIVERGENCE = 6


@dataclass
class LandingConstraints:
    """monte_carlo.py:36-52."""
    pos_tol_xy: float = 5.0
    pos_tol_z: float = 1.0
    vel_tol_xy: float = 1.0
    vel_tol_z: float = 2.0
    tilt_max: float = 0.1
    min_fuel_margin: float = 0.05

    def check_landing(self, state, initial_mass):
        """monte_carlo.py:54-104: (success, reason) for a final state (x = altitude axis)."""
        m, alt, y, z, vv, vy, vz = [float(v) for v in np.asarray(state)[:7]]
        if abs(alt) > self.pos_tol_z:
            return False, f"Altitude error: {alt:.2f} m"
        if abs(y) > self.pos_tol_xy or abs(z) > self.pos_tol_xy:
            return False, f"Horizontal position error: ({y:.2f}, {z:.2f}) m"
        if abs(vv) > self.vel_tol_z:
            return False, f"Vertical velocity: {vv:.2f} m/s"
        if abs(vy) > self.vel_tol_xy or abs(vz) > self.vel_tol_xy:
            return False, f"Horizontal velocity: ({vy:.2f}, {vz:.2f}) m/s"
        used = 1.0 - m / initial_mass
        if used > (1.0 - self.min_fuel_margin):
            return False, f"Fuel margin: {(1 - used) * 100:.1f}%"
        return True, "Success"


@dataclass
class SimulationConfig:
    """monte_carlo.py:107-130."""
    dt: float = 0.1
    max_time: float = 100.0
    altitude_mean: float = 500.0
    altitude_std: float = 100.0
    horizontal_std: float = 50.0
    velocity_mean: np.ndarray = field(default_factory=lambda: np.array([0, 0, -75]))
    velocity_std: np.ndarray = field(default_factory=lambda: np.array([20, 20, 15]))
    mass_mean: float = 2.0
    mass_std: float = 0.1
    wind_enabled: bool = False
    aero_dispersion: float = 0.0
    thrust_dispersion: float = 0.0
    landing_constraints: LandingConstraints = field(default_factory=LandingConstraints)

    @classmethod
    def run_experiments(cls):
        """The SimulationConfig of scripts/run_experiments.py:359-371 (BASELINE C3/C4)."""
        return cls(dt=0.1, max_time=30.0, altitude_mean=30.0, altitude_std=5.0,
                   horizontal_std=3.0, velocity_mean=np.array([-3, 0, 0]),
                   velocity_std=np.array([1, 0.5, 0.5]),
                   landing_constraints=LandingConstraints(pos_tol_xy=5.0, vel_tol_z=3.0))


def sample_initial_condition(seed, cfg: SimulationConfig):
    """MonteCarloSimulator.sample_initial_condition (monte_carlo.py:368-399): seven
    legacy-MT19937 normal draws in the order m, altitude, r_y, r_z, v_x, v_y, v_z;
    m clipped to [1.5, 2.5], altitude to [10, 100], v_x <= -1."""
    rs = np.random.RandomState(seed)
    m = np.clip(cfg.mass_mean + rs.randn() * cfg.mass_std, 1.5, 2.5)
    alt = np.clip(cfg.altitude_mean + rs.randn() * cfg.altitude_std, 10, 100)
    ry = rs.randn() * cfg.horizontal_std
    rz = rs.randn() * cfg.horizontal_std
    vx = min(cfg.velocity_mean[0] + rs.randn() * cfg.velocity_std[0], -1)
    vy = cfg.velocity_mean[1] + rs.randn() * cfg.velocity_std[1]
    vz = cfg.velocity_mean[2] + rs.randn() * cfg.velocity_std[2]
    return np.array([m, alt, ry, rz, vx, vy, vz], dtype=float)


def mc_noise_table(seed, n_runs, cfg: SimulationConfig, max_steps=None):
    """The standard normals ``run`` (n_workers = 1) consumes after each landing's initial
    condition, as the device's noise table (n_runs, max_steps, 4): landing i continues
    ``RandomState(seed + i)`` past its seven initial-condition draws with one thrust draw
    (``thrust_dispersion > 0``) then three aero draws (``aero_dispersion > 0``) per control
    step (monte_carlo.py:531-537).  Column 0 the thrust draw, 1..3 the aero draws; unused
    columns are 0.  One flat ``randn`` call per landing: the legacy stream does not depend
    on how the draws are grouped."""
    ms = int(cfg.max_time / cfg.dt) if max_steps is None else int(max_steps)
    cols = ([0] if cfg.thrust_dispersion > 0 else []) + ([1, 2, 3] if cfg.aero_dispersion > 0 else [])
    table = np.zeros((int(n_runs), ms, 4))
    if not cols:
        return table
    for i in range(int(n_runs)):
        rs = np.random.RandomState(seed + i)
        rs.randn(7)
        table[i][:, cols] = rs.randn(ms * len(cols)).reshape(ms, len(cols))
    return table


@dataclass
class SimulationResult:
    """monte_carlo.py:133-161: one landing."""
    run_id: int
    outcome: LandingOutcome
    success: bool
    states: np.ndarray        # (T+1, n_x)
    controls: np.ndarray      # (T, n_u)
    times: np.ndarray         # (T+1,)
    fuel_used: float
    flight_time: float
    final_position_error: float
    final_velocity_error: float
    max_constraint_violation: float
    initial_state: np.ndarray
    compute_time_ms: float
    failure_reason: str = ""
    metadata: Dict[str, Any] = field(default_factory=dict)


@dataclass
class MonteCarloResults:
    """monte_carlo.py:164-325: the landings of one run and their statistics."""
    config: SimulationConfig
    results: List[SimulationResult]
    _stats_cache: Optional[Dict[str, Any]] = field(default=None, repr=False)

    @property
    def n_runs(self) -> int:
        return len(self.results)

    @property
    def n_success(self) -> int:
        return sum(1 for r in self.results if r.success)

    @property
    def success_rate(self) -> float:
        return self.n_success / self.n_runs if self.n_runs > 0 else 0.0

    def get_statistics(self) -> Dict[str, Any]:
        """monte_carlo.py:186-250: the same keys from the same numpy calls."""
        if self._stats_cache is not None:
            return self._stats_cache
        outcomes = {o.name: sum(1 for r in self.results if r.outcome == o) for o in LandingOutcome}
        ok = [r for r in self.results if r.success]
        if not ok:
            self._stats_cache = {"n_runs": self.n_runs, "n_success": 0, "success_rate": 0.0,
                                 "success_rate_ci": (0.0, 0.0), "outcomes": outcomes}
            return self._stats_cache
        fuel = np.array([r.fuel_used for r in ok])
        tof = np.array([r.flight_time for r in ok])
        pos = np.array([r.final_position_error for r in ok])
        vel = np.array([r.final_velocity_error for r in ok])
        comp = np.array([r.compute_time_ms for r in ok])
        self._stats_cache = {
            "n_runs": self.n_runs,
            "n_success": self.n_success,
            "success_rate": self.success_rate,
            "success_rate_ci": self._binomial_ci(self.n_success, self.n_runs),
            "outcomes": outcomes,
            "fuel_mean": float(np.mean(fuel)),
            "fuel_std": float(np.std(fuel)),
            "fuel_min": float(np.min(fuel)),
            "fuel_max": float(np.max(fuel)),
            "fuel_percentiles": {q: float(np.percentile(fuel, int(q))) for q in ("5", "50", "95")},
            "time_mean": float(np.mean(tof)),
            "time_std": float(np.std(tof)),
            "pos_error_mean": float(np.mean(pos)),
            "pos_error_std": float(np.std(pos)),
            "pos_error_max": float(np.max(pos)),
            "vel_error_mean": float(np.mean(vel)),
            "vel_error_std": float(np.std(vel)),
            "compute_mean_ms": float(np.mean(comp)),
            "compute_std_ms": float(np.std(comp)),
            "compute_max_ms": float(np.max(comp)),
        }
        return self._stats_cache

    def _binomial_ci(self, successes: int, trials: int, confidence: float = 0.95):
        """monte_carlo.py:252-272: Wilson score interval."""
        if trials == 0:
            return (0.0, 0.0)
        from scipy import stats
        z = stats.norm.ppf(1 - (1 - confidence) / 2)
        p_hat = successes / trials
        denominator = 1 + z**2 / trials
        center = (p_hat + z**2 / (2 * trials)) / denominator
        margin = z * np.sqrt(p_hat * (1 - p_hat) / trials + z**2 / (4 * trials**2)) / denominator
        return (max(0, center - margin), min(1, center + margin))

    def summary(self) -> str:
        """monte_carlo.py:274-314: the same report text."""
        st = self.get_statistics()
        bar = "=" * 60
        lo, hi = st["success_rate_ci"]
        out = [bar, "Monte Carlo Simulation Results", bar, "",
               f"Total runs:     {st['n_runs']}",
               f"Successful:     {st['n_success']}",
               f"Success rate:   {st['success_rate'] * 100:.1f}% (95% CI: [{lo * 100:.1f}%, {hi * 100:.1f}%])",
               "", "Outcome Breakdown:"]
        for name, count in st["outcomes"].items():
            out.append(f"  {name:20s}: {count:4d} ({count / st['n_runs'] * 100:5.1f}%)")
        if st["n_success"] > 0:
            out += ["", "Performance Metrics (successful runs):",
                    f"  Fuel used:      {st['fuel_mean']:.3f} ± {st['fuel_std']:.3f} kg",
                    f"  Flight time:    {st['time_mean']:.2f} ± {st['time_std']:.2f} s",
                    f"  Position error: {st['pos_error_mean']:.3f} ± {st['pos_error_std']:.3f} m",
                    f"  Velocity error: {st['vel_error_mean']:.3f} ± {st['vel_error_std']:.3f} m/s",
                    "", "Compute Time:",
                    f"  Mean:  {st['compute_mean_ms']:.2f} ms",
                    f"  Max:   {st['compute_max_ms']:.2f} ms"]
        out.append(bar)
        return "\n".join(out)

    def save(self, filepath: str) -> None:
        with open(filepath, "wb") as fh:
            pickle.dump(self, fh)

    @classmethod
    def load(cls, filepath: str) -> "MonteCarloResults":
        with open(filepath, "rb") as fh:
            return pickle.load(fh)


def _same(a, b) -> bool:
    """Field-by-field equality of two settings objects (dataclasses with array fields)."""
    if is_dataclass(a) and is_dataclass(b):
        return type(a) is type(b) and all(_same(getattr(a, f.name), getattr(b, f.name)) for f in fields(a))
    if a is None or b is None:
        return a is None and b is None
    try:
        return bool(np.array_equal(np.asarray(a), np.asarray(b)))
    except Exception:
        return False


# what the control kernels' QP assembly compiles in (k_fleet_control in csrc/fleet.hip,
# k_fleet_control2 and fleet_box in csrc/fleet_control.h), against mpc/qp_builder.py
_FLEET_QP = dict(Q_DIAG=[0.0, 10.0, 10.0, 10.0, 1.0, 1.0, 1.0], R_DIAG=[0.01, 0.01, 0.01], QF_SCALE=10.0,
                 X_MIN=[-np.inf, -100.0, -100.0, -100.0, -50.0, -50.0, -50.0],
                 X_MAX=[np.inf, 500.0, 100.0, 100.0, 50.0, 50.0, 50.0],
                 U_MIN=[0.3, -5.0, -5.0], U_MAX=[5.0, 5.0, 5.0])


class MonteCarloSimulator:
    """monte_carlo.py:328-676, same constructor and methods.

    ``run`` takes the batched device path (one ``Fleet`` of ``n_runs`` landings with the
    Monte-Carlo attachment: dispersions and trajectory log on the GPU) when ``_fleet_plan``
    finds the caller's objects to be exactly what the fleet restates, and the reference's
    loop over ``run_single`` otherwise; ``last_path`` is "fleet" or "loop",
    ``last_path_reason`` the first condition that sent a run to the loop.
    ``fleet_chunk``: control steps between termination polls of the batched path (1: the
    results' metadata also carry the per-step ADMM iterations)."""

    def __init__(self, dynamics, controller, config: Optional[SimulationConfig] = None,
                 safety_filter=None, gp_model=None):
        self.dynamics = dynamics
        self.controller = controller
        self.config = config or SimulationConfig()
        self.safety_filter = safety_filter
        self.gp = gp_model
        self.n_x = getattr(dynamics, "n_x", 7)
        self.n_u = getattr(dynamics, "n_u", 3)
        self.last_path: Optional[str] = None
        self.last_path_reason = ""
        self.fleet_chunk = 25
        self.keep_raw_log = False   # keep the batched run's records and NaN-padded log in last_raw_log
        self.last_raw_log = None

    def sample_initial_condition(self, seed: Optional[int] = None) -> np.ndarray:
        """monte_carlo.py:368-399 on numpy's global stream (seeded when ``seed`` is given)."""
        if seed is not None:
            np.random.seed(seed)
        cfg = self.config
        m = np.clip(cfg.mass_mean + np.random.randn() * cfg.mass_std, 1.5, 2.5)
        altitude = np.clip(cfg.altitude_mean + np.random.randn() * cfg.altitude_std, 10, 100)
        horiz_y = np.random.randn() * cfg.horizontal_std
        horiz_z = np.random.randn() * cfg.horizontal_std
        v_vert = min(cfg.velocity_mean[0] + np.random.randn() * cfg.velocity_std[0], -1)
        v_horiz_y = cfg.velocity_mean[1] + np.random.randn() * cfg.velocity_std[1]
        v_horiz_z = cfg.velocity_mean[2] + np.random.randn() * cfg.velocity_std[2]
        return np.array([m, altitude, horiz_y, horiz_z, v_vert, v_horiz_y, v_horiz_z])

    def run_single(self, run_id: int, x0: Optional[np.ndarray] = None,
                   seed: Optional[int] = None) -> SimulationResult:
        """monte_carlo.py:401-583, the loop as written: termination checks at the top of
        every step, the controller's ``step`` or ``solve`` protocol, the safety filter,
        ``dynamics.step`` and the dispersion draws from numpy's global stream.  One
        addition: a controller with ``reset_warm_start`` starts every
        landing cold, as the batched path does."""
        t_start = time.perf_counter()
        if x0 is None:
            x0 = self.sample_initial_condition(seed)
        initial_mass = x0[0]
        x_target = np.zeros(self.n_x)
        x_target[0] = initial_mass
        ctl = self.controller
        if hasattr(ctl, "reset_warm_start"):
            ctl.reset_warm_start()
        if hasattr(ctl, "initialize"):
            ctl.initialize(x0, x_target)
        if self.safety_filter is not None and hasattr(self.safety_filter, "initialize"):
            self.safety_filter.initialize(x0)
        cfg = self.config
        dt = cfg.dt
        max_steps = int(cfg.max_time / dt)
        states, controls, times = [x0.copy()], [], [0.0]
        x, t = x0.copy(), 0.0
        outcome, failure_reason, max_violation = LandingOutcome.SUCCESS, "", 0.0
        admm_iters: List[int] = []
        for _ in range(max_steps):
            altitude = x[1]
            if altitude < 0:
                outcome, failure_reason = LandingOutcome.CRASH, f"Crashed at altitude {altitude:.2f}m"
                break
            dry_mass = 1.0
            if x[0] <= dry_mass + 0.01:
                outcome, failure_reason = LandingOutcome.FUEL_EXHAUSTED, f"Fuel exhausted: mass={x[0]:.3f}"
                break
            if np.any(np.abs(x) > 1e6) or np.any(np.isnan(x)):
                outcome, failure_reason = LandingOutcome.DIVERGENCE, "State diverged"
                break
            velocity = x[4]
            if altitude < 1.0 and abs(velocity) < 5.0:
                ok, reason = cfg.landing_constraints.check_landing(x, initial_mass)
                if not ok:
                    outcome, failure_reason = LandingOutcome.CONSTRAINT_VIOLATION, reason
                break
            try:
                if hasattr(ctl, "step"):
                    u = ctl.step(x).u0
                elif hasattr(ctl, "solve"):
                    x_target = x.copy()
                    x_target[4:7] = 0
                    x_target[1] = max(0.5, altitude - 2.0)
                    sol = ctl.solve(x, x_target)
                    if sol is None:
                        outcome, failure_reason = LandingOutcome.DIVERGENCE, "Controller returned None"
                        break
                    if hasattr(sol, "success") and not sol.success:
                        outcome, failure_reason = LandingOutcome.DIVERGENCE, "MPC solve failed"
                        break
                    u = sol.u0
                else:
                    u = np.zeros(self.n_u)
            except Exception as e:
                outcome, failure_reason = LandingOutcome.DIVERGENCE, f"Controller failed: {e}"
                break
            if self.safety_filter is not None:
                try:
                    res = self.safety_filter.filter(x, u)
                    u = res.u_safe
                    max_violation = max(max_violation, res.constraint_violation)
                except Exception:
                    pass
            x_next = self.dynamics.step(x, u, dt)
            if cfg.thrust_dispersion > 0:
                thrust_noise = np.random.randn() * cfg.thrust_dispersion
                x_next[4:7] += thrust_noise * u[0] / x[0] * dt
            if cfg.aero_dispersion > 0:
                aero_noise = np.random.randn(3) * cfg.aero_dispersion
                x_next[4:7] += aero_noise * dt
            if hasattr(ctl, "last_iterations"):
                admm_iters.append(int(ctl.last_iterations))
            controls.append(u)
            x = x_next
            t += dt
            states.append(x.copy())
            times.append(t)
        else:
            outcome, failure_reason = LandingOutcome.TIMEOUT, f"Exceeded {cfg.max_time}s"
        compute_time = (time.perf_counter() - t_start) * 1000
        states = np.array(states)
        controls = np.array(controls) if controls else np.zeros((0, self.n_u))
        times = np.array(times)
        final_state = states[-1]
        metadata: Dict[str, Any] = {}
        if hasattr(ctl, "last_iterations"):
            metadata = {"admm_iterations": int(sum(admm_iters)), "admm_iterations_per_step": admm_iters,
                        "last_qp_status": int(getattr(ctl, "last_status", 0))}
        return SimulationResult(
            run_id=run_id, outcome=outcome, success=outcome == LandingOutcome.SUCCESS, states=states,
            controls=controls, times=times, fuel_used=initial_mass - final_state[0], flight_time=times[-1],
            final_position_error=np.linalg.norm(final_state[1:4]),
            final_velocity_error=np.linalg.norm(final_state[4:7]), max_constraint_violation=max_violation,
            initial_state=x0, compute_time_ms=compute_time, failure_reason=failure_reason, metadata=metadata)

    # ---- the batched path ------------------------------------------------------
    def _fleet_plan(self, n_workers: int = 1):
        """(fleet keyword arguments, GP device handle) when this simulator is exactly what
        the device fleet restates, else (None, reason).  Host logic only: no device call.

        The fleet compiles in (csrc/fleet_control.h, csrc/fleet.hip): the Simple3DoF features with v_ref 10,
        altitude and density on and the default atmosphere (features3); the Euler plant
        with alpha = 1/30, g = [-1, 0, 0] (plant_euler); the solve protocol with the
        incremental target; and k_fleet_control's QP -- Q = diag(0, 10, 10, 10, 1, 1, 1),
        R = 0.01 I, terminal 10 Q, the state box [-inf, -100 x3, -50 x3] .. [inf, 500,
        100, 100, 50 x3], the thrust box [0.3, -5, -5] .. [5, 5, 5], the analytic
        Jacobians on the structural 26-entry pattern, the hover first guess u = [m0, 0, 0],
        the GP mean with the GPMPC sign.  Runtime: N, dt, max_steps, use_gp_mean,
        max_sqp_iter / sqp_tol and the ADMM's max_iter / eps (``qp_settings()``; every
        other ADMM setting at the library default, which the host workspace shares)."""
        from .. import _lib
        from ..dynamics.rocket_3dof import Rocket3DoFDynamics
        from ..gp.features import Simple3DoFFeatureExtractor
        from ..gp.structured_gp import Simple3DoFGP
        from ..mpc import qp_builder
        from ..mpc.constraints import ConstraintParams
        from ..mpc.cost_functions import CostWeights
        from ..mpc.gp_mpc import GPMPC

        cfg, ctl, dyn = self.config, self.controller, self.dynamics
        if type(ctl) is not GPMPC:
            return None, "the controller is not the 3-DoF GPMPC adapter"
        if self.safety_filter is not None:
            return None, "a safety filter is set"
        disp = cfg.thrust_dispersion > 0 or cfg.aero_dispersion > 0
        if n_workers != 1 and disp:
            return None, "n_workers > 1 with dispersions: one serial noise stream"
        if type(dyn) is not Rocket3DoFDynamics:
            return None, "the plant is not Rocket3DoFDynamics"
        p = dyn.params
        if not (p.alpha == 1.0 / 30.0 and np.array_equal(np.asarray(p.g_vec, float), [-1.0, 0.0, 0.0])):
            return None, "the plant's alpha / gravity are not the fleet's 1/30, [-1, 0, 0]"
        qb = ctl._qp
        if not (type(qb) is qp_builder.RTIQPBuilder and not qb.dense and qb.alpha == 1.0 / 30.0
                and np.array_equal(qb.g_vec, [-1.0, 0.0, 0.0]) and ctl._g0 == 1.0):
            return None, "the controller's model is not the fleet's Euler 3-DoF model"
        c = ctl.config
        if not (c.dt == cfg.dt and qb.dt == cfg.dt):
            return None, "controller.config.dt differs from config.dt"
        if not (int(c.N) == c.N and c.N >= 1 and qb.N == c.N):
            return None, "the horizon is not a positive integer"
        if c.integration_method != "euler":
            return None, "integration_method is not euler"
        for name, val in _FLEET_QP.items():
            if not np.array_equal(np.asarray(getattr(qp_builder, name), float), np.asarray(val, float)):
                return None, f"qp_builder.{name} is not the fleet's compiled value"
        if not _same(ctl.cost_weights, CostWeights()):
            return None, "cost_weights are not the defaults"
        if not _same(ctl.constraint_params, ConstraintParams()):
            return None, "constraint_params are not the defaults"
        mi, eps = c.qp_settings()
        want = _lib.qp_default_settings(max_iter=int(mi), eps_abs=float(eps), eps_rel=float(eps))
        have = ctl._ws.settings
        if any(getattr(want, f[0]) != getattr(have, f[0]) for f in _lib.QPSettings._fields_):
            return None, "the controller's ADMM settings are not qp_settings() on the library defaults"
        gp = ctl.gp
        if type(gp) is not Simple3DoFGP or not gp._is_fitted:
            return None, "controller.gp is not a fitted Simple3DoFGP"
        fe = gp.feature_extractor
        if not (type(fe) is Simple3DoFFeatureExtractor and fe.v_ref == 10.0 and fe.include_altitude
                and fe.include_density and fe.atmosphere.rho_0 == 1.225 and fe.atmosphere.scale_height == 8500.0):
            return None, "the GP's features are not the default Simple3DoFFeatureExtractor"
        handle = gp.gp.device_handle
        if not isinstance(handle, (_lib.ExactGPHandle, _lib.FITCHandle)):
            return None, "the GP has no shared device handle"
        max_steps = int(cfg.max_time / cfg.dt)
        if max_steps < 1:
            return None, "no control step fits in max_time"
        kw = dict(horizon=int(c.N), dt=float(cfg.dt), target_mode=1, use_gp=int(bool(c.use_gp_mean)),
                  residual_model=0, max_steps=max_steps, sqp_iters=max(1, int(c.max_sqp_iter)),
                  sqp_tol=float(c.sqp_tol), max_iter=int(mi), eps_abs=float(eps), eps_rel=float(eps))
        return kw, handle

    def _result_from_record(self, i, rec, states, controls, compute_ms, iters_per_step=None):
        """One landing of the batched run: outcome from the record (1 and 4 re-decided by
        the caller's LandingConstraints on the final state), the rest from the log."""
        from ..fleet import REC_ADMM_ITERS, REC_LAST_STATUS, REC_M0, REC_OUTCOME
        cfg = self.config
        xf = states[-1]
        m0 = rec[REC_M0]
        code = int(rec[REC_OUTCOME])
        outcome, reason = LandingOutcome.SUCCESS, ""
        if code in (1, 4):
            ok, why = cfg.landing_constraints.check_landing(xf, m0)
            if not ok:
                outcome, reason = LandingOutcome.CONSTRAINT_VIOLATION, why
        elif code == 2:
            outcome, reason = LandingOutcome.CRASH, f"Crashed at altitude {xf[1]:.2f}m"
        elif code == 3:
            outcome, reason = LandingOutcome.FUEL_EXHAUSTED, f"Fuel exhausted: mass={xf[0]:.3f}"
        elif code == 5:
            outcome, reason = LandingOutcome.TIMEOUT, f"Exceeded {cfg.max_time}s"
        else:   # 6, or still running after max_steps + 1 steps (cannot happen)
            diverged = bool(np.any(np.abs(xf) > 1e6) or np.any(np.isnan(xf)))
            outcome, reason = LandingOutcome.DIVERGENCE, "State diverged" if diverged else "MPC solve failed"
        T = controls.shape[0]
        times = cfg.dt * np.arange(T + 1)
        meta = {"admm_iterations": int(rec[REC_ADMM_ITERS]), "last_qp_status": int(rec[REC_LAST_STATUS])}
        if iters_per_step is not None:
            meta["admm_iterations_per_step"] = [int(v) for v in iters_per_step[:T]]
        return SimulationResult(
            run_id=i, outcome=outcome, success=outcome == LandingOutcome.SUCCESS, states=states,
            controls=controls, times=times, fuel_used=m0 - xf[0], flight_time=times[-1],
            final_position_error=np.linalg.norm(xf[1:4]), final_velocity_error=np.linalg.norm(xf[4:7]),
            max_constraint_violation=0.0, initial_state=states[0].copy(), compute_time_ms=compute_ms,
            failure_reason=reason, metadata=meta)

    def _run_fleet(self, kw, handle, x0s, noise, progress_callback, log=True):
        from ..fleet import REC_ADMM_ITERS, REC_OUTCOME, Fleet
        cfg = self.config
        n = len(x0s)
        t0 = time.perf_counter()
        fl = Fleet(handle.ctx, handle, n, **kw)
        try:
            fl.attach_mc(cfg.thrust_dispersion, cfg.aero_dispersion, log=log, noise=noise)
            fl.reset(np.asarray(x0s, float))
            max_steps, chunk = kw["max_steps"], max(1, int(self.fleet_chunk))
            done, cum = 0, []
            rec = None
            while done < max_steps + 1:   # the (max_steps + 1)-th launch records the TIMEOUTs
                k = min(chunk, max_steps + 1 - done)
                fl.step(k)
                done += k
                rec, _ = fl.read()
                cum.append(rec[:, REC_ADMM_ITERS].copy())
                if progress_callback is not None:
                    progress_callback(int(np.sum(rec[:, REC_OUTCOME] != 0)), n)
                if np.all(rec[:, REC_OUTCOME] != 0):
                    break
            if log:
                states, controls, ns = fl.read_log()
            else:
                states = controls = ns = None
        finally:
            fl.close()
        wall_ms = (time.perf_counter() - t0) * 1000
        if not log:
            return rec, wall_ms
        if self.keep_raw_log:
            self.last_raw_log = dict(records=rec, states=states, controls=controls, nsteps=ns)
        per_step = None
        if chunk == 1:   # one poll per control step: the per-step ADMM iterations
            per_step = np.diff(np.vstack([np.zeros(n)] + cum), axis=0).T
        return [self._result_from_record(i, rec[i], states[i, :ns[i] + 1].copy(), controls[i, :ns[i]].copy(),
                                         wall_ms / n, None if per_step is None else per_step[i])
                for i in range(n)]

    # ---- the baseline controllers' batch (csrc/baseline.hip) ----------
    def _baseline_plan(self, n_workers: int = 1):
        """(controller kind, "") when the landings can fly in one ``baseline_fly`` call, else
        (None, reason).  Host logic only: no device call."""
        from ..dynamics.rocket_3dof import Rocket3DoFDynamics
        from .baselines import device_gate
        from .dispersion import DispersedDynamics
        cfg = self.config
        kind, why = device_gate(self.controller)
        if kind is None:
            return None, why
        if type(self.dynamics) is DispersedDynamics:
            return None, ("a DispersedDynamics instance's step_count runs on across landings: serial "
                          "(DispersionAnalysis.run_single batches one instance per landing)")
        if type(self.dynamics) is not Rocket3DoFDynamics:
            return None, "the plant is not Rocket3DoFDynamics"
        if self.safety_filter is not None:
            return None, "a safety filter is set"
        if n_workers != 1 and (cfg.thrust_dispersion > 0 or cfg.aero_dispersion > 0):
            return None, "n_workers > 1 with dispersions: one serial noise stream"
        if int(cfg.max_time / cfg.dt) < 1:
            return None, "no control step fits in max_time"
        return kind, ""

    def _run_baselines(self, kind, x0s, plant=None, noise=None, timing=None):
        """The landings from ``x0s`` in one device call -> [SimulationResult].  ``plant``: the
        ``DispersedDynamics`` batch (``dispersion.plant_batch``) or None for the bare plant
        with the config's own dispersions over ``noise``.  The controller is initialised per
        landing on the host, as ``run_single`` does.  ``timing``: a dict that receives the
        host preparation, kernel and total milliseconds."""
        from .. import _lib
        from .baselines import controller_batch
        cfg = self.config
        n = len(x0s)
        t0 = time.perf_counter()
        x0s = np.asarray(x0s, float).reshape(n, 7)
        p = self.dynamics.params
        kw = controller_batch(self.controller, kind, x0s)
        kw.update(plant or {})
        if plant is None and (cfg.thrust_dispersion > 0 or cfg.aero_dispersion > 0):
            kw.update(sim_thrust=cfg.thrust_dispersion, sim_aero=cfg.aero_dispersion, noise=noise)
        max_steps = int(cfg.max_time / cfg.dt)
        t1 = time.perf_counter()
        tm = {} if timing is not None else None
        rec, ns, log = _lib.baseline_fly(_lib.default_context(), x0s, max_steps=max_steps, dt=float(cfg.dt),
                                         alpha=float(p.alpha), g=np.asarray(p.g_vec, float), timing=tm, **kw)
        wall_ms = (time.perf_counter() - t0) * 1000
        if timing is not None:
            timing.update(prepare_ms=(t1 - t0) * 1000, kernel_ms=tm["kernel_ms"], call_ms=wall_ms - (t1 - t0) * 1000)
        if self.keep_raw_log:
            self.last_raw_log = dict(records=rec, log=log, nsteps=ns)
        out = []
        for i in range(n):
            T = int(ns[i])
            states = np.concatenate([x0s[i:i + 1], log[:T, i, :7]], axis=0)
            out.append(self._result_from_record(i, rec[i], states, log[:T, i, 7:].copy(), wall_ms / n))
            out[-1].metadata = {}
        return out

    def run(self, n_runs: int = 1000, n_workers: int = 1, seed: int = 42,
            progress_callback: Optional[Callable[[int, int], None]] = None,
            use_fleet: bool = True) -> MonteCarloResults:
        """monte_carlo.py:585-636.  ``use_fleet=False`` forces the reference's loop.  On
        the batched path ``progress_callback(terminated, n_runs)`` is called once per
        chunk of control steps and ``compute_time_ms`` is the run's wall time / n_runs.
        A baseline controller (``_baseline_plan``) flies its landings in one device call:
        ``last_path`` "baselines", one ``progress_callback(n_runs, n_runs)``."""
        from .. import _lib
        plan, second = self._fleet_plan(n_workers) if use_fleet else (None, "use_fleet=False")
        why = second if plan is None else ""
        kind, bwhy = self._baseline_plan(n_workers) if use_fleet and plan is None else (None, "")
        if kind is not None:
            cfg = self.config
            if n_workers == 1:
                x0s = [sample_initial_condition(seed + i, cfg) for i in range(n_runs)]
                disp = cfg.thrust_dispersion > 0 or cfg.aero_dispersion > 0
                noise = mc_noise_table(seed, n_runs, cfg) if disp else None
            else:   # the reference draws every initial condition from one stream seeded `seed`
                print(f"Running {n_runs} simulations with {n_workers} workers...")
                np.random.seed(seed)
                x0s = [self.sample_initial_condition() for _ in range(n_runs)]
                noise = None
            try:
                results = self._run_baselines(kind, x0s, noise=noise) if n_runs > 0 else []
                self.last_path, self.last_path_reason = "baselines", ""
                if progress_callback is not None:
                    progress_callback(n_runs, n_runs)
                return MonteCarloResults(config=self.config, results=results)
            except _lib.HIPError as e:
                if e.rc != -2:   # only "the library refuses these arguments" falls back
                    raise
                why = f"the device refused the configuration: {e}"
        elif use_fleet and plan is None and type(self.controller).__module__.endswith("experiments.baselines"):
            why = bwhy   # a baseline controller the batch does not admit: its own reason
        if plan is not None:
            cfg = self.config
            if n_workers == 1:
                x0s = [sample_initial_condition(seed + i, cfg) for i in range(n_runs)]
                disp = cfg.thrust_dispersion > 0 or cfg.aero_dispersion > 0
                noise = mc_noise_table(seed, n_runs, cfg, plan["max_steps"]) if disp else None
            else:   # the reference draws every initial condition from one stream seeded `seed`
                print(f"Running {n_runs} simulations with {n_workers} workers...")
                np.random.seed(seed)
                x0s = [self.sample_initial_condition() for _ in range(n_runs)]
                noise = None
            try:
                results = self._run_fleet(plan, second, x0s, noise, progress_callback) if n_runs > 0 else []
                self.last_path, self.last_path_reason = "fleet", ""
                return MonteCarloResults(config=self.config, results=results)
            except _lib.HIPError as e:
                if e.rc != -2:   # only "the fleet refuses these arguments" falls back
                    raise
                why = f"the fleet refused the configuration: {e}"
        self.last_path, self.last_path_reason = "loop", why
        results = []
        if n_workers == 1:
            for i in range(n_runs):
                results.append(self.run_single(i, seed=seed + i))
                if progress_callback is not None:
                    progress_callback(i + 1, n_runs)
                if (i + 1) % 100 == 0:
                    print(f"Completed {i + 1}/{n_runs} runs...")
        else:
            print(f"Running {n_runs} simulations with {n_workers} workers...")
            np.random.seed(seed)
            x0s = [self.sample_initial_condition() for _ in range(n_runs)]
            for i, x0 in enumerate(x0s):
                results.append(self.run_single(i, x0=x0))
                if progress_callback is not None:
                    progress_callback(i + 1, n_runs)
        return MonteCarloResults(config=self.config, results=results)

    def run_with_dispersions(self, n_runs: int = 100,
                             dispersion_configs: Optional[List[Dict[str, float]]] = None
                             ) -> Dict[str, MonteCarloResults]:
        """monte_carlo.py:638-676: ``run`` once per dispersion level (each run picks its
        own path: on the fleet the levels differ only in the attachment)."""
        if dispersion_configs is None:
            dispersion_configs = [
                {"name": "nominal", "thrust_dispersion": 0.0, "aero_dispersion": 0.0},
                {"name": "low_disp", "thrust_dispersion": 0.01, "aero_dispersion": 0.5},
                {"name": "med_disp", "thrust_dispersion": 0.02, "aero_dispersion": 1.0},
                {"name": "high_disp", "thrust_dispersion": 0.05, "aero_dispersion": 2.0},
            ]
        out = {}
        for entry in dispersion_configs:
            name = entry.pop("name", "unnamed")
            print(f"\nRunning configuration: {name}")
            for key, value in entry.items():
                setattr(self.config, key, value)
            res = self.run(n_runs=n_runs)
            out[name] = res
            print(f"  Success rate: {res.success_rate * 100:.1f}%")
        return out


def compare_controllers(dynamics, controllers: Dict[str, Any], n_runs: int = 100,
                        config: Optional[SimulationConfig] = None, seed: int = 42,
                        use_fleet: bool = True) -> Dict[str, MonteCarloResults]:
    """monte_carlo.py:679-732: every controller flies the same initial conditions (one
    stream seeded ``seed``), one ``run_single`` per landing.  With ``use_fleet`` a baseline
    controller that ``_baseline_plan`` admits (and a config without dispersions: those draw
    from one stream across landings) flies them in one device call; every other controller,
    the GP-MPC included, takes ``run_single`` as before.  ``compare_controllers.last_paths``
    holds the path of each controller of the last call."""
    from .. import _lib
    config = config or SimulationConfig()
    np.random.seed(seed)
    sampler = MonteCarloSimulator(dynamics, None, config)
    initial_states = [sampler.sample_initial_condition() for _ in range(n_runs)]
    out = {}
    paths = compare_controllers.last_paths = {}
    for name, controller in controllers.items():
        print(f"\nEvaluating controller: {name}")
        sim = MonteCarloSimulator(dynamics, controller, config)
        runs = None
        kind, why = sim._baseline_plan(1) if use_fleet else (None, "use_fleet=False")
        if kind is not None and (config.thrust_dispersion > 0 or config.aero_dispersion > 0):
            kind, why = None, "the config's dispersions draw from one stream across landings"
        if kind is not None and n_runs > 0:
            try:
                runs = sim._run_baselines(kind, [x0.copy() for x0 in initial_states])
                paths[name] = ("baselines", "")
            except _lib.HIPError as e:
                if e.rc != -2:
                    raise
                why = f"the device refused the configuration: {e}"
        if runs is None:
            paths[name] = ("loop", why)
            runs = []
            for i, x0 in enumerate(initial_states):
                runs.append(sim.run_single(i, x0=x0.copy()))
                if (i + 1) % 50 == 0:
                    print(f"  Completed {i + 1}/{n_runs}...")
        out[name] = MonteCarloResults(config=config, results=runs)
        print(f"  Success rate: {out[name].success_rate * 100:.1f}%")
    return out
