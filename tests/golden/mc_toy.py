"""Stand-ins for the Monte-Carlo driver fixture (mc_sim_golden.npz): a numpy 3-DoF
plant and a ``solve``-protocol feedback controller.  gen_mc_sim_golden.py drives the
reference MonteCarloSimulator with them and tests/test_mc_simulator.py the mirror, so
both sides run the same arithmetic.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np


class ToyPlant3:
    """Explicit-Euler point mass, x = [m, r(3), v(3)], gravity along -x."""
    n_x = 7
    n_u = 3
    alpha = 1.0 / 30.0
    g = np.array([-1.0, 0.0, 0.0])

    def step(self, x, u, dt):
        x = np.asarray(x, float); u = np.asarray(u, float)
        out = np.empty(7)
        out[0] = x[0] - dt * self.alpha * np.sqrt(u @ u)
        out[1:4] = x[1:4] + dt * x[4:7]
        out[4:7] = x[4:7] + dt * (u / x[0] + self.g)
        return out


class _Sol:
    def __init__(self, u0):
        self.u0 = u0


class FeedbackLander:
    """``solve(x, x_target)`` -> an object with ``u0``: descent-rate tracking on the
    altitude axis, PD on the two horizontal axes, thrust clipped to a box.  No
    ``step``, no ``initialize``, no ``reset_warm_start`` and no ``success`` flag: the
    simulator's plain ``solve`` branch."""

    def __init__(self, k_rate=0.35, v_touch=0.8, k_v=2.0, k_p=0.15, k_d=0.9):
        self.k_rate, self.v_touch, self.k_v, self.k_p, self.k_d = k_rate, v_touch, k_v, k_p, k_d

    def solve(self, x, x_target):
        m, alt = x[0], x[1]
        v_des = -(self.v_touch + self.k_rate * max(alt, 0.0))
        u = np.empty(3)
        u[0] = m * (1.0 + self.k_v * (v_des - x[4]))
        u[1] = m * (-self.k_p * x[2] - self.k_d * x[5])
        u[2] = m * (-self.k_p * x[3] - self.k_d * x[6])
        return _Sol(np.clip(u, [0.3, -5.0, -5.0], [5.0, 5.0, 5.0]))


def fixture_cases():
    """name -> (SimulationConfig keyword overrides on run_experiments(), run keywords)."""
    return {
        "nominal": (dict(), dict(n_runs=8, n_workers=1, seed=42)),
        "dispersed": (dict(thrust_dispersion=0.02, aero_dispersion=1.0), dict(n_runs=8, n_workers=1, seed=42)),
        "workers2": (dict(), dict(n_runs=6, n_workers=2, seed=7)),
    }


MAX_TIME = 7.0     # between the fastest and the slowest descents of the fixture: some time out
VEL_TOL_Z = 1.44   # inside the spread of the touchdown rates: some landings violate it


def without_compute(stats):
    """get_statistics() without the wall-clock keys, JSON-ready (tuples -> lists)."""
    out = {k: v for k, v in stats.items() if not k.startswith("compute_")}
    out["success_rate_ci"] = [float(v) for v in out["success_rate_ci"]]
    return out
