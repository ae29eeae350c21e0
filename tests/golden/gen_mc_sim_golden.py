"""Generate mc_sim_golden.npz from the reference's own MonteCarloSimulator.

Container-only, like gen_golden.py: imports /root/reference/src/experiments through the
same namespace shim; only the .npz written next to this script travels.  The reference
simulator flies the stand-in plant and controller of mc_toy.py (the reference's plants
need the absent simdyn) in three configurations -- nominal, dispersed, n_workers = 2 --
and the fixture keeps, per configuration: states / controls (NaN-padded), step counts,
outcomes, failure-reason prefixes, get_statistics() without the compute-time keys and
summary() above "Compute Time".  Run:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_mc_sim_golden.py
"""
from __future__ import annotations

import contextlib
import importlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src"
sys.path.insert(0, HERE)

from mc_toy import MAX_TIME, VEL_TOL_Z, FeedbackLander, ToyPlant3, fixture_cases, without_compute  # noqa: E402

pkg = types.ModuleType("refexp")
pkg.__path__ = [os.path.join(REF, "experiments")]
sys.modules["refexp"] = pkg
mc = importlib.import_module("refexp.monte_carlo")


def config(**over):
    # scripts/run_experiments.py:359-371, with the fixture's max_time and touchdown-rate tolerance
    return mc.SimulationConfig(dt=0.1, max_time=MAX_TIME, altitude_mean=30.0, altitude_std=5.0, horizontal_std=3.0,
                               velocity_mean=np.array([-3, 0, 0]), velocity_std=np.array([1, 0.5, 0.5]),
                               landing_constraints=mc.LandingConstraints(pos_tol_xy=5.0, vel_tol_z=VEL_TOL_Z), **over)


def main():
    out = {}
    for name, (over, run_kw) in fixture_cases().items():
        sim = mc.MonteCarloSimulator(ToyPlant3(), FeedbackLander(), config(**over))
        with contextlib.redirect_stdout(io.StringIO()):
            res = sim.run(**run_kw)
        n = res.n_runs
        T = np.array([len(r.controls) for r in res.results])
        S = np.full((n, T.max() + 1, 7), np.nan); U = np.full((n, max(T.max(), 1), 3), np.nan)
        for i, r in enumerate(res.results):
            S[i, :T[i] + 1] = r.states
            U[i, :T[i]] = r.controls
        out[f"{name}_states"] = S
        out[f"{name}_controls"] = U
        out[f"{name}_nsteps"] = T
        out[f"{name}_outcomes"] = np.array([r.outcome.value for r in res.results])
        out[f"{name}_reasons"] = np.array([r.failure_reason[:24] for r in res.results])
        out[f"{name}_flight_time"] = np.array([r.flight_time for r in res.results])
        out[f"{name}_stats"] = np.array(json.dumps(without_compute(res.get_statistics())))
        text = res.summary()
        out[f"{name}_summary"] = np.array(text.split("Compute Time:")[0])
        print(name, [r.outcome.name for r in res.results], T.tolist())
    np.savez_compressed(os.path.join(HERE, "mc_sim_golden.npz"), **out)


if __name__ == "__main__":
    main()
