"""Dispersion analysis (reference src/experiments/dispersion.py): wind, aerodynamic, thrust
and initial-condition dispersions, the plant wrapper that applies them and the sweep over
dispersion levels, with the reference's names, defaults and numpy statements in its order.

``DispersedDynamics`` reseeds numpy's global generator from ``seed + step_count`` twice per
plant step, so landing i (seed ``seed + i``) at step s reads the draws of key ``i + s``: the
device batch (csrc/baseline.hip) takes one table row per key instead
of one per landing and step (``thrust_key_table``, ``wind_key_table``,
``wind_step_offsets``).  The state in which a run leaves numpy's global generator is not
reproduced on the device path.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from enum import Enum, auto
from typing import Dict, Optional, Tuple

import numpy as np


class WindModel(Enum):
    NONE = auto()
    CONSTANT = auto()
    GUST = auto()
    DRYDEN = auto()
    CUSTOM = auto()


@dataclass
class WindConfig:
    """dispersion.py:34-102."""
    model: WindModel = WindModel.NONE
    wind_velocity: np.ndarray = field(default_factory=lambda: np.array([0.0, 0.0, 0.0]))
    gust_amplitude: float = 10.0
    gust_duration: float = 2.0
    gust_probability: float = 0.1
    turbulence_intensity: float = 1.0
    altitude_ref: float = 500.0

    def get_wind(self, t: float, pos, seed: Optional[int] = None) -> np.ndarray:
        if self.model == WindModel.NONE:
            return np.zeros(3)
        elif self.model == WindModel.CONSTANT:
            return self.wind_velocity.copy()
        elif self.model == WindModel.GUST:
            if seed is not None:
                np.random.seed(seed + int(t * 10))
            if np.random.rand() < self.gust_probability * 0.1:
                direction = np.random.randn(3)
                direction /= np.linalg.norm(direction) + 1e-6
                return direction * self.gust_amplitude
            return np.zeros(3)
        elif self.model == WindModel.DRYDEN:
            altitude = max(pos[2], 10)   # pos = x[1:4]: the third position component, as written
            sigma_u = self.turbulence_intensity * 3.0
            if seed is not None:
                np.random.seed(seed + int(t * 100))
            wind = np.random.randn(3) * sigma_u
            wind *= min(1.0, altitude / 100)
            return wind
        return np.zeros(3)


@dataclass
class AeroDispersionConfig:
    """dispersion.py:105-138."""
    Cd_nominal: float = 0.5
    Cd_std: float = 0.1
    A_nominal: float = 1.0
    A_std: float = 0.05
    cp_offset_std: float = 0.05
    enabled: bool = False

    def sample(self, seed: Optional[int] = None) -> Dict[str, float]:
        if seed is not None:
            np.random.seed(seed)
        if not self.enabled:
            return {"Cd": self.Cd_nominal, "A": self.A_nominal, "cp_offset": np.zeros(3)}
        return {"Cd": self.Cd_nominal + np.random.randn() * self.Cd_std,
                "A": self.A_nominal + np.random.randn() * self.A_std,
                "cp_offset": np.random.randn(3) * self.cp_offset_std}


@dataclass
class ThrustDispersionConfig:
    """dispersion.py:141-190."""
    thrust_scale_std: float = 0.02
    misalignment_std: float = 0.01
    fluctuation_std: float = 0.01
    enabled: bool = False

    def apply_dispersion(self, thrust_cmd, seed: Optional[int] = None) -> np.ndarray:
        if not self.enabled:
            return thrust_cmd.copy()
        if seed is not None:
            np.random.seed(seed)
        thrust = thrust_cmd.copy()
        scale = 1.0 + np.random.randn() * self.thrust_scale_std
        thrust[0] *= scale
        thrust[1] += np.random.randn() * self.misalignment_std
        thrust[2] += np.random.randn() * self.misalignment_std
        thrust[0] *= 1.0 + np.random.randn() * self.fluctuation_std
        return thrust


@dataclass
class InitialConditionDispersion:
    """dispersion.py:193-229."""
    x_std: float = 10.0
    y_std: float = 10.0
    z_std: float = 20.0
    vx_std: float = 5.0
    vy_std: float = 5.0
    vz_std: float = 10.0
    mass_std: float = 0.05

    def sample(self, nominal, seed: Optional[int] = None) -> np.ndarray:
        if seed is not None:
            np.random.seed(seed)
        dispersed = nominal.copy()
        dispersed[0] += np.random.randn() * self.mass_std
        dispersed[1] += np.random.randn() * self.x_std
        dispersed[2] += np.random.randn() * self.y_std
        dispersed[3] += np.random.randn() * self.z_std
        dispersed[4] += np.random.randn() * self.vx_std
        dispersed[5] += np.random.randn() * self.vy_std
        dispersed[6] += np.random.randn() * self.vz_std
        return dispersed


@dataclass
class DispersionConfig:
    """dispersion.py:232-283 with its four presets."""
    wind: WindConfig = field(default_factory=WindConfig)
    aero: AeroDispersionConfig = field(default_factory=AeroDispersionConfig)
    thrust: ThrustDispersionConfig = field(default_factory=ThrustDispersionConfig)
    initial: InitialConditionDispersion = field(default_factory=InitialConditionDispersion)

    @classmethod
    def nominal(cls) -> "DispersionConfig":
        return cls()

    @classmethod
    def low(cls) -> "DispersionConfig":
        return cls(wind=WindConfig(model=WindModel.CONSTANT, wind_velocity=np.array([2.0, 1.0, 0.0])),
                   aero=AeroDispersionConfig(Cd_std=0.05, enabled=True),
                   thrust=ThrustDispersionConfig(thrust_scale_std=0.01, enabled=True))

    @classmethod
    def medium(cls) -> "DispersionConfig":
        return cls(wind=WindConfig(model=WindModel.DRYDEN, turbulence_intensity=1.0),
                   aero=AeroDispersionConfig(Cd_std=0.1, enabled=True),
                   thrust=ThrustDispersionConfig(thrust_scale_std=0.02, misalignment_std=0.01, enabled=True))

    @classmethod
    def high(cls) -> "DispersionConfig":
        return cls(wind=WindConfig(model=WindModel.DRYDEN, turbulence_intensity=2.0),
                   aero=AeroDispersionConfig(Cd_std=0.2, enabled=True),
                   thrust=ThrustDispersionConfig(thrust_scale_std=0.05, misalignment_std=0.02,
                                                 fluctuation_std=0.02, enabled=True))


class DispersedDynamics:
    """dispersion.py:286-370: the base plant under thrust dispersion (on the commanded
    control), wind (on the velocity) and extra drag (from the pre-step state)."""

    def __init__(self, base_dynamics, dispersion_config: DispersionConfig, seed: int = 42):
        self.base = base_dynamics
        self.config = dispersion_config
        self.seed = seed
        self.step_count = 0
        self.aero_params = self.config.aero.sample(seed)
        self.n_x = getattr(base_dynamics, "n_x", 7)
        self.n_u = getattr(base_dynamics, "n_u", 3)
        if hasattr(base_dynamics, "params"):
            self.params = base_dynamics.params

    def step(self, x, u, dt: float) -> np.ndarray:
        self.step_count += 1
        u_actual = self.config.thrust.apply_dispersion(u, seed=self.seed + self.step_count)
        x_next = self.base.step(x, u_actual, dt)
        t = self.step_count * dt
        pos = x[1:4]
        wind = self.config.wind.get_wind(t, pos, self.seed + self.step_count + 1000)
        x_next[4:7] += wind * dt
        if self.config.aero.enabled:
            vel = x[4:7]
            speed = np.linalg.norm(vel)
            if speed > 1.0:
                Cd = self.aero_params["Cd"]
                A = self.aero_params["A"]
                rho = 0.02
                drag = 0.5 * rho * Cd * A * speed**2
                drag_accel = drag / x[0] * (vel / speed)
                x_next[4:7] -= drag_accel * dt
        return x_next

    def continuous_dynamics(self, x, u) -> np.ndarray:
        return self.base.continuous_dynamics(x, u)

    def reset(self) -> None:
        self.step_count = 0


# ---- key tables of the device batch -------------------------------------------------------------
def thrust_key_table(cfg: ThrustDispersionConfig, seed: int, n_runs: int, max_steps: int) -> np.ndarray:
    """Rows r = 0 .. n_runs + max_steps - 1 of the factors ``apply_dispersion(., seed + r)``
    applies: [scale, misalignment 1, misalignment 2, fluctuation factor], each formed with
    numpy's roundings.  Landing i at plant step s (1-based) reads row i + s."""
    rows = int(n_runs) + int(max_steps)
    tab = np.zeros((rows, 4))
    rs = np.random.RandomState()
    for r in range(rows):
        rs.seed(seed + r)
        tab[r, 0] = 1.0 + rs.randn() * cfg.thrust_scale_std
        tab[r, 1] = rs.randn() * cfg.misalignment_std
        tab[r, 2] = rs.randn() * cfg.misalignment_std
        tab[r, 3] = 1.0 + rs.randn() * cfg.fluctuation_std
    return tab


def wind_step_offsets(model: WindModel, dt: float, max_steps: int) -> np.ndarray:
    """Per plant step s = 1 .. max_steps the key offset ``s + 1000 + int(t * k)`` of
    ``get_wind``'s reseed, t = s * dt in Python floats (0.29 * 100 truncates to 28), k = 10
    for GUST, 100 for DRYDEN; zeros for the models that draw nothing."""
    k = {WindModel.GUST: 10, WindModel.DRYDEN: 100}.get(model)
    if k is None:
        return np.zeros(int(max_steps), dtype=np.int64)
    return np.array([s + 1000 + int((s * dt) * k) for s in range(1, int(max_steps) + 1)], dtype=np.int64)


def wind_key_table(cfg: WindConfig, seed: int, n_runs: int, offsets: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(table, rows): landing i at plant step s reads table[i + rows[s - 1]].  CONSTANT: the
    wind itself; GUST: the complete gust vector of key ``seed + offset``; DRYDEN:
    ``randn(3) * sigma_u`` (the altitude factor is applied per landing on the device)."""
    n_runs = int(n_runs)
    if cfg.model == WindModel.CONSTANT:
        return np.tile(np.asarray(cfg.wind_velocity, float), (n_runs, 1)), np.zeros(len(offsets), dtype=np.int32)
    if cfg.model not in (WindModel.GUST, WindModel.DRYDEN) or len(offsets) == 0:
        return np.zeros((n_runs, 3)), np.zeros(len(offsets), dtype=np.int32)
    lo, hi = int(offsets.min()), int(offsets.max())
    tab = np.zeros((n_runs + hi - lo, 3))
    rs = np.random.RandomState()
    for r in range(len(tab)):
        rs.seed(seed + lo + r)
        if cfg.model == WindModel.GUST:
            if rs.rand() < cfg.gust_probability * 0.1:
                direction = rs.randn(3)
                direction /= np.linalg.norm(direction) + 1e-6
                tab[r] = direction * cfg.gust_amplitude
        else:
            tab[r] = rs.randn(3) * (cfg.turbulence_intensity * 3.0)
    return tab, (offsets - lo).astype(np.int32)


def plant_batch(dcfg: DispersionConfig, seed: int, n_runs: int, dt: float, max_steps: int) -> Dict[str, object]:
    """The ``DispersedDynamics(base, dcfg, seed + i)`` plants of landings i = 0 .. n_runs - 1
    as the keyword arguments of ``_lib.baseline_fly``, or raises ValueError for a wind model
    the device does not restate (none today: CUSTOM is zeros)."""
    kw: Dict[str, object] = {}
    if dcfg.thrust.enabled:
        kw["thrust_table"] = thrust_key_table(dcfg.thrust, seed, n_runs, max_steps)
    model = dcfg.wind.model
    if model in (WindModel.CONSTANT, WindModel.GUST, WindModel.DRYDEN):
        tab, rows = wind_key_table(dcfg.wind, seed, n_runs, wind_step_offsets(model, dt, max_steps))
        kw.update(wind_table=tab, wind_rows=rows, wind_altitude_factor=model == WindModel.DRYDEN)
    if dcfg.aero.enabled:
        cda = np.zeros(int(n_runs))
        state = np.random.get_state()
        for i in range(int(n_runs)):
            p = dcfg.aero.sample(seed + i)
            cda[i] = 0.5 * 0.02 * p["Cd"] * p["A"]
        np.random.set_state(state)
        kw["drag_cda"] = cda
    return kw


@dataclass
class DispersionAnalysisResults:
    """dispersion.py:373-445."""
    config_name: str
    dispersion_config: DispersionConfig
    final_positions: np.ndarray
    final_velocities: np.ndarray
    position_mean: np.ndarray
    position_cov: np.ndarray
    velocity_mean: np.ndarray
    velocity_cov: np.ndarray
    n_runs: int
    n_success: int
    success_rate: float

    def get_dispersion_ellipse(self, confidence: float = 0.95) -> Tuple[np.ndarray, float, float, float]:
        """(center, semi_major, semi_minor, angle) of the first two position components."""
        from scipy import stats
        positions_2d = self.final_positions[:, :2]
        center = np.mean(positions_2d, axis=0)
        cov_2d = np.cov(positions_2d.T)
        eigenvalues, eigenvectors = np.linalg.eigh(cov_2d)
        chi2 = stats.chi2.ppf(confidence, 2)
        semi_major = np.sqrt(eigenvalues[1] * chi2)
        semi_minor = np.sqrt(eigenvalues[0] * chi2)
        angle = np.arctan2(eigenvectors[1, 1], eigenvectors[0, 1])
        return center, semi_major, semi_minor, angle

    def get_3sigma_bounds(self) -> Dict[str, Tuple[float, float]]:
        bounds = {}
        for i, name in enumerate(["x", "y", "z"]):
            mean = self.position_mean[i]
            std = np.sqrt(self.position_cov[i, i])
            bounds[f"pos_{name}"] = (mean - 3 * std, mean + 3 * std)
        for i, name in enumerate(["vx", "vy", "vz"]):
            mean = self.velocity_mean[i]
            std = np.sqrt(self.velocity_cov[i, i])
            bounds[f"vel_{name}"] = (mean - 3 * std, mean + 3 * std)
        return bounds


class DispersionAnalysis:
    """dispersion.py:448-599.  ``run_single`` flies its landings in one device call when
    ``_baseline_plan`` admits the controller and plant (``last_path`` "baselines"), and as the
    reference's loop otherwise (``last_path`` "loop", ``last_path_reason`` why);
    ``use_fleet = False`` forces the loop."""

    def __init__(self, dynamics, controller, mc_config=None):
        self.base_dynamics = dynamics
        self.controller = controller
        self.mc_config = mc_config
        self.use_fleet = True
        self.last_path: Optional[str] = None
        self.last_path_reason = ""

    def _baseline_plan(self, mc_config):
        """(controller kind, "") or (None, reason): host logic only."""
        from ..dynamics.rocket_3dof import Rocket3DoFDynamics
        from .baselines import device_gate
        if not self.use_fleet:
            return None, "use_fleet=False"
        kind, why = device_gate(self.controller)
        if kind is None:
            return None, why
        if type(self.base_dynamics) is not Rocket3DoFDynamics:
            return None, "the plant is not Rocket3DoFDynamics"
        if mc_config.thrust_dispersion > 0 or mc_config.aero_dispersion > 0:
            return None, "the SimulationConfig's own dispersions would continue a reseeded stream"
        if int(mc_config.max_time / mc_config.dt) < 1:
            return None, "no control step fits in max_time"
        return kind, ""

    def _fly_batch(self, kind, mc_config, dispersion_config, n_runs, seed):
        """The landings of ``run_single`` in one device call -> [SimulationResult]."""
        from .monte_carlo import MonteCarloSimulator
        sim = MonteCarloSimulator(self.base_dynamics, self.controller, mc_config)
        state = np.random.get_state()
        x0s = []
        for i in range(n_runs):
            x0 = sim.sample_initial_condition(seed=seed + i)
            x0s.append(dispersion_config.initial.sample(x0, seed=seed + i + 10000))
        np.random.set_state(state)
        max_steps = int(mc_config.max_time / mc_config.dt)
        plant = plant_batch(dispersion_config, seed, n_runs, mc_config.dt, max_steps)
        return sim._run_baselines(kind, x0s, plant)

    def run_single(self, dispersion_config: DispersionConfig, n_runs: int = 100,
                   seed: int = 42) -> DispersionAnalysisResults:
        from .. import _lib
        from .monte_carlo import MonteCarloSimulator, SimulationConfig
        mc_config = self.mc_config or SimulationConfig()
        kind, why = self._baseline_plan(mc_config)
        results = None
        if kind is not None and n_runs > 0:
            try:
                results = self._fly_batch(kind, mc_config, dispersion_config, n_runs, seed)
                self.last_path, self.last_path_reason = "baselines", ""
            except _lib.HIPError as e:
                if e.rc != -2:   # only "the library refuses these arguments" falls back
                    raise
                why = f"the device refused the configuration: {e}"
        final_positions = []
        final_velocities = []
        n_success = 0
        if results is None:
            self.last_path, self.last_path_reason = "loop", why
            for i in range(n_runs):
                dispersed = DispersedDynamics(self.base_dynamics, dispersion_config, seed=seed + i)
                mc_config = self.mc_config or SimulationConfig()
                sim = MonteCarloSimulator(dispersed, self.controller, mc_config)
                x0 = sim.sample_initial_condition(seed=seed + i)
                x0 = dispersion_config.initial.sample(x0, seed=seed + i + 10000)
                result = sim.run_single(i, x0=x0)
                if result.success:
                    n_success += 1
                final_positions.append(result.states[-1, 1:4])
                final_velocities.append(result.states[-1, 4:7])
        else:
            for result in results:
                if result.success:
                    n_success += 1
                final_positions.append(result.states[-1, 1:4])
                final_velocities.append(result.states[-1, 4:7])
        final_positions = np.array(final_positions)
        final_velocities = np.array(final_velocities)
        return DispersionAnalysisResults(
            config_name="custom", dispersion_config=dispersion_config,
            final_positions=final_positions, final_velocities=final_velocities,
            position_mean=np.mean(final_positions, axis=0), position_cov=np.cov(final_positions.T),
            velocity_mean=np.mean(final_velocities, axis=0), velocity_cov=np.cov(final_velocities.T),
            n_runs=n_runs, n_success=n_success, success_rate=n_success / n_runs)

    def run_sweep(self, n_runs_per_level: int = 100, seed: int = 42) -> Dict[str, DispersionAnalysisResults]:
        levels = {"nominal": DispersionConfig.nominal(), "low": DispersionConfig.low(),
                  "medium": DispersionConfig.medium(), "high": DispersionConfig.high()}
        results = {}
        print("Dispersion Analysis Sweep")
        print("=" * 50)
        for name, config in levels.items():
            print(f"\nRunning {name} dispersion level...")
            result = self.run_single(config, n_runs_per_level, seed)
            result.config_name = name
            results[name] = result
            print(f"  Success rate: {result.success_rate * 100:.1f}%")
            print(f"  Position std: {np.sqrt(np.diag(result.position_cov))}")
        return results

    def summary_table(self, results: Dict[str, DispersionAnalysisResults]) -> str:
        lines = ["=" * 70, "Dispersion Analysis Summary", "=" * 70,
                 f"{'Level':<12} {'Success%':>10} {'Pos σ_xy (m)':>15} {'Pos σ_z (m)':>12} {'Vel σ (m/s)':>12}",
                 "-" * 70]
        for name, result in results.items():
            pos_std_xy = np.sqrt(result.position_cov[0, 0] + result.position_cov[1, 1])
            pos_std_z = np.sqrt(result.position_cov[2, 2])
            vel_std = np.sqrt(np.trace(result.velocity_cov))
            lines.append(f"{name:<12} {result.success_rate * 100:>9.1f}% {pos_std_xy:>14.2f} "
                         f"{pos_std_z:>11.2f} {vel_std:>11.2f}")
        lines.append("=" * 70)
        return "\n".join(lines)
