"""Generate baselines.npz from the reference's own baselines.py, dispersion.py and
monte_carlo.py over this package's Rocket3DoFDynamics.

Container-only, like gen_mc_sim_golden.py: imports /root/reference/src/experiments through the
same namespace shim; only the .npz written next to this script travels.  The cases are the
groups of tests/baseline_cases.py.  Per group the fixture keeps, for every landing: outcome,
step count, initial and final state, fuel, flight time, the two error norms, the failure
reason; for the first N_FULL landings the whole trajectory; and the spread: per landing and
component, the largest change of the reference's own trajectory (states over every step,
controls over every step) under a relative perturbation 2^-52 z of every plant step's result,
over two perturbation streams.  For the dispersed groups also DispersionAnalysis.run_single's
statistics, and once the two tables' text and create_baseline_controllers' keys.

The generator asserts, with F and MARGIN of baseline_cases.py, that the perturbed flights keep
every outcome and step count and that every discrete decision of every case lies
>= MARGIN x F x its spread from its threshold: each termination comparison at each step, each
check_landing comparison on a final state inside the landing window, and speed > 1.0 at each
step when drag is on.  A case that fails is replaced in GROUPS, never excused.  Run:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_baselines_golden.py
"""
from __future__ import annotations

import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import baseline_cases as bc  # noqa: E402
from gp_mpc_rocket_landing_amd.dynamics.rocket_3dof import Rocket3DoFDynamics  # noqa: E402

pkg = types.ModuleType("refexp")
pkg.__path__ = [os.path.join(REF, "experiments")]
sys.modules["refexp"] = pkg
REFMODS = bc.Modules(importlib.import_module("refexp.monte_carlo"), importlib.import_module("refexp.baselines"),
                     importlib.import_module("refexp.dispersion"))
STREAMS = (1, 2)


def margins(group, r, sx, lc):
    """The smallest (distance to threshold) / spread over the decisions of one landing; sx: its
    per-component state spread."""
    plant = bc.GROUPS[group][2]
    drag = plant in bc.DISPERSED
    worst = np.inf

    def need(dist, spread):
        nonlocal worst
        if spread > 0:
            worst = min(worst, abs(dist) / spread)

    X = r.states
    for t, x in enumerate(X):
        need(x[1] - 0.0, sx[1])
        need(x[0] - 1.01, sx[0])
        need(x[1] - 1.0, sx[1])
        if x[1] < 1.0:
            need(abs(x[4]) - 5.0, sx[4])
        if drag and t < len(r.controls):
            need(np.linalg.norm(x[4:7]) - 1.0, sx[4] + sx[5] + sx[6])
    x = X[-1]
    if r.outcome.name in ("SUCCESS", "CONSTRAINT_VIOLATION"):   # check_landing, in its order, up to the failure
        m0 = r.initial_state[0]
        tests = [((abs(x[1]) - lc.pos_tol_z, sx[1]),), ((abs(x[2]) - lc.pos_tol_xy, sx[2]), (abs(x[3]) - lc.pos_tol_xy, sx[3])),
                 ((abs(x[4]) - lc.vel_tol_z, sx[4]),), ((abs(x[5]) - lc.vel_tol_xy, sx[5]), (abs(x[6]) - lc.vel_tol_xy, sx[6])),
                 (((1.0 - x[0] / m0) - (1.0 - lc.min_fuel_margin), sx[0] / m0),)]
        for line in tests:
            for d, s in line:
                need(d, s)
            if any(d > 0 for d, _ in line):
                break
    return worst


def main():
    dyn = Rocket3DoFDynamics()
    table = bc.open_loop_table(REFMODS, dyn)
    out = {"ol_table": table}
    worst_all, spread_all = np.inf, 0.0
    for group, (cfg_name, ctl_name, plant, seed, n) in bc.GROUPS.items():
        assert 42 <= seed and seed + n - 1 <= 65, group
        ref = bc.fly_group(REFMODS, dyn, group, table)
        sx = np.zeros((n, 7)); su = np.zeros((n, 3))
        for stream in STREAMS:
            per = bc.fly_group(REFMODS, dyn, group, table, perturb=stream)
            for i, (a, b) in enumerate(zip(ref, per)):
                assert a.outcome == b.outcome and len(a.controls) == len(b.controls), (group, i, "flips under the probe")
                sx[i] = np.maximum(sx[i], np.max(np.abs(a.states - b.states), axis=0))
                if len(a.controls):
                    su[i] = np.maximum(su[i], np.max(np.abs(a.controls - b.controls), axis=0))
        lc = bc.make_config(REFMODS, cfg_name).landing_constraints
        worst = min(margins(group, r, sx[i], lc) for i, r in enumerate(ref))
        assert worst >= bc.MARGIN * bc.F, (group, worst, [margins(group, r, sx[i], lc) for i, r in enumerate(ref)])
        worst_all = min(worst_all, worst); spread_all = max(spread_all, sx.max(), su.max())
        for k, v in bc.pack(ref).items():
            out[f"{group}_{k}"] = v
        out[f"{group}_spread_x"] = sx
        out[f"{group}_spread_u"] = su
        if plant in bc.DISPERSED:   # the analysis itself, through the reference's run_single
            ctl = bc.make_controller(REFMODS, ctl_name, dyn, table)
            an = REFMODS.dp.DispersionAnalysis(dyn, ctl, bc.make_config(REFMODS, cfg_name))
            res = an.run_single(bc.make_dispersion(REFMODS, plant), n_runs=n, seed=seed)
            for k in ("final_positions", "final_velocities", "position_mean", "position_cov", "velocity_mean", "velocity_cov"):
                out[f"{group}_an_{k}"] = getattr(res, k)
            out[f"{group}_an_n_success"] = np.array(res.n_success)
            out[f"{group}_an_3sigma"] = np.array([v for pair in res.get_3sigma_bounds().values() for v in pair])
            c, a, b, ang = res.get_dispersion_ellipse()
            out[f"{group}_an_ellipse"] = np.array([c[0], c[1], a, b, ang])
            if group == "exp_lqr_medium":
                out["summary_table"] = np.array(an.summary_table({"medium": res, "again": res}))
        print(group, [r.outcome.name for r in ref], [len(r.controls) for r in ref],
              f"spread {max(sx.max(), su.max()):.2e} margin/spread {worst:.3g}")
    cmp_ = REFMODS.bl.BaselineComparison(["LQR", "PID"], {"LQR": 0.875, "PID": 0.5}, {"LQR": 0.1234, "PID": 0.25},
                                         {"LQR": 0.01, "PID": 0.0321}, {"LQR": 12.3456, "PID": 30.0}, {"LQR": 0.051})
    out["to_table"] = np.array(cmp_.to_table())
    with contextlib.redirect_stdout(io.StringIO()):
        keys = list(REFMODS.bl.create_baseline_controllers(dyn, None, (np.zeros((3, 7)), table)))
    out["controller_keys"] = np.array(keys)
    # a wave whose lanes differ in speed > 1 at one step (the drag term's select)
    X = [out[f"exp_pid_high_states{i}"] for i in range(bc.N_FULL)]
    t_mixed = [t for t in range(min(len(x) for x in X) - 1)
               if len({bool(np.linalg.norm(x[t, 4:7]) > 1.0) for x in X}) == 2]
    assert t_mixed, "no step with speed > 1 on some stored lanes and not on others"
    np.savez_compressed(os.path.join(HERE, "baselines.npz"), **out)
    print(f"largest spread {spread_all:.2e}, smallest margin/spread {worst_all:.3g}, "
          f"{os.path.getsize(os.path.join(HERE, 'baselines.npz'))} bytes")


if __name__ == "__main__":
    main()
