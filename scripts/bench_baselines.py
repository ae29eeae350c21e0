"""Time the baseline controllers' device batch against the per-landing loop (DESIGN.md section
21, docs/PERF_HISTORY.md): run_experiments() with N landings under LQR and PID, and the
four-level DispersionAnalysis sweep.  The device path is split into host preparation (initial
conditions, the per-landing ``initialize`` with its Riccati solve, the key tables), the kernel
(between two events) and the rest of the call (staging, read-back, result objects).

    python scripts/bench_baselines.py [--n 1024] [--repeats 7] [--sweep-n 1024] [--no-loop]

One JSON line per measurement: median and range over the repeats after one warm-up."""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gp_mpc_rocket_landing_amd.dynamics.rocket_3dof import Rocket3DoFDynamics  # noqa: E402
from gp_mpc_rocket_landing_amd.experiments import (DispersionAnalysis, LQRController, MonteCarloSimulator,  # noqa: E402
                                                   PIDController, SimulationConfig, sample_initial_condition)


def stats(v):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sweep-n", type=int, default=1024)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    dyn = Rocket3DoFDynamics()
    cfg = SimulationConfig.run_experiments()
    for name, C in (("LQR", LQRController), ("PID", PIDController)):
        sim = MonteCarloSimulator(dyn, C(dyn), cfg)
        kind, why = sim._baseline_plan(1)
        assert kind is not None, why
        parts = {k: [] for k in ("x0_ms", "prepare_ms", "kernel_ms", "call_ms", "wall_ms")}
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            x0s = [sample_initial_condition(42 + i, cfg) for i in range(a.n)]
            t1 = time.perf_counter()
            tm = {}
            res = sim._run_baselines(kind, x0s, timing=tm)
            t2 = time.perf_counter()
            if rep:   # the first is the warm-up
                for k in ("prepare_ms", "kernel_ms", "call_ms"):
                    parts[k].append(tm[k])
                parts["x0_ms"].append((t1 - t0) * 1000)
                parts["wall_ms"].append((t2 - t0) * 1000)
        out = dict(what=f"run_experiments {name} device", n=a.n, repeats=a.repeats,
                   success=sum(r.success for r in res), **{k: stats(v) for k, v in parts.items()})
        print(json.dumps(out), flush=True)
        if not a.no_loop:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                host = sim.run(a.n, seed=42, use_fleet=False)
            print(json.dumps(dict(what=f"run_experiments {name} loop", n=a.n, wall_ms=round((time.perf_counter() - t0) * 1000, 1),
                                  success=host.n_success)), flush=True)
    an = DispersionAnalysis(dyn, LQRController(dyn), cfg)
    walls = []
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            sweep = an.run_sweep(a.sweep_n, seed=42)
        assert an.last_path == "baselines", an.last_path_reason
        if rep:
            walls.append((time.perf_counter() - t0) * 1000)
    print(json.dumps(dict(what="dispersion sweep LQR device", n=a.sweep_n, levels=4, wall_ms=stats(walls),
                          success={k: v.n_success for k, v in sweep.items()})), flush=True)
    if not a.no_loop:
        an.use_fleet = False
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            sweep = an.run_sweep(a.sweep_n, seed=42)
        print(json.dumps(dict(what="dispersion sweep LQR loop", n=a.sweep_n, levels=4,
                              wall_ms=round((time.perf_counter() - t0) * 1000, 1),
                              success={k: v.n_success for k, v in sweep.items()})), flush=True)


if __name__ == "__main__":
    main()
