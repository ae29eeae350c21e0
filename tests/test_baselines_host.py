"""The baseline controllers and the dispersion classes on the host (experiments/baselines.py,
experiments/dispersion.py) against what the reference's own classes recorded
(tests/golden/baselines.npz, gen_baselines_golden.py): every stored field bit for bit."""
import contextlib
import io

import numpy as np
import pytest
from scipy import linalg

import baseline_cases as bc
from gp_mpc_rocket_landing_amd import experiments as ex
from gp_mpc_rocket_landing_amd.dynamics.rocket_3dof import Rocket3DoFDynamics

PKG = bc.package_modules()
DYN = Rocket3DoFDynamics()


@pytest.fixture(scope="module")
def g():
    return bc.load()


def test_the_fixture_covers_the_outcomes_and_fits_the_size_limit(g):
    import os
    seen = set()
    for group in bc.GROUPS:
        seen |= set(g[f"{group}_outcomes"].tolist())
    assert seen == {1, 2, 3, 4, 5}   # every outcome but DIVERGENCE
    sizes = [os.path.getsize(os.path.join(os.path.dirname(bc.GOLDEN), f)) for f in os.listdir(os.path.dirname(bc.GOLDEN))]
    assert os.path.getsize(bc.GOLDEN) < max(sizes)
    assert np.array_equal(g["ol_table"], bc.open_loop_table(PKG, DYN)) and len(g["ol_table"]) == bc.OL_ROWS
    assert all(g[f"{gr}_nsteps"].max() > bc.OL_ROWS for gr in bc.GROUPS if bc.GROUPS[gr][1] == "ol")


@pytest.mark.parametrize("group", list(bc.GROUPS))
def test_host_landings_have_the_references_bits(g, group):
    res = bc.fly_group(PKG, DYN, group, g["ol_table"])
    for k, v in bc.pack(res).items():
        want = g[f"{group}_{k}"]
        assert v.shape == want.shape and np.array_equal(v, want), (group, k)


@pytest.mark.parametrize("group", ["exp_lqr_plain", "def_pid_sim", "short_lqr_plain"])
def test_run_on_the_loop_is_the_same_landings(g, group):
    cfg_name, ctl_name, plant, seed, n = bc.GROUPS[group]
    cfg = bc.make_config(PKG, cfg_name)
    if plant == "sim":
        cfg.thrust_dispersion, cfg.aero_dispersion = 0.02, 1.0
    sim = ex.MonteCarloSimulator(DYN, bc.make_controller(PKG, ctl_name, DYN, g["ol_table"]), cfg)
    res = sim.run(n, seed=seed, use_fleet=False)
    assert (sim.last_path, sim.last_path_reason) == ("loop", "use_fleet=False")
    assert np.array_equal([r.states[-1] for r in res.results], g[f"{group}_final"])
    assert [r.outcome.value for r in res.results] == g[f"{group}_outcomes"].tolist()
    assert np.array_equal(res.results[1].controls, g[f"{group}_controls1"])


@pytest.mark.parametrize("group", [gr for gr, v in bc.GROUPS.items() if v[2] in bc.DISPERSED])
def test_dispersion_analysis_on_the_loop_has_the_references_bits(g, group):
    cfg_name, ctl_name, plant, seed, n = bc.GROUPS[group]
    an = ex.DispersionAnalysis(DYN, bc.make_controller(PKG, ctl_name, DYN, g["ol_table"]), bc.make_config(PKG, cfg_name))
    an.use_fleet = False
    res = an.run_single(bc.make_dispersion(PKG, plant), n_runs=n, seed=seed)
    assert (an.last_path, an.last_path_reason) == ("loop", "use_fleet=False")
    for k in ("final_positions", "final_velocities", "position_mean", "position_cov", "velocity_mean", "velocity_cov"):
        assert np.array_equal(getattr(res, k), g[f"{group}_an_{k}"]), k
    assert res.n_success == int(g[f"{group}_an_n_success"]) and res.success_rate == res.n_success / n
    assert res.config_name == "custom" and res.n_runs == n
    assert np.array_equal([v for pair in res.get_3sigma_bounds().values() for v in pair], g[f"{group}_an_3sigma"])
    assert list(res.get_3sigma_bounds()) == ["pos_x", "pos_y", "pos_z", "vel_vx", "vel_vy", "vel_vz"]
    c, a, b, ang = res.get_dispersion_ellipse()
    assert np.array_equal([c[0], c[1], a, b, ang], g[f"{group}_an_ellipse"])
    if group == "exp_lqr_medium":
        assert an.summary_table({"medium": res, "again": res}) == str(g["summary_table"])


def test_the_tables_text(g):
    cmp_ = ex.BaselineComparison(["LQR", "PID"], {"LQR": 0.875, "PID": 0.5}, {"LQR": 0.1234, "PID": 0.25},
                                 {"LQR": 0.01, "PID": 0.0321}, {"LQR": 12.3456, "PID": 30.0}, {"LQR": 0.051})
    assert cmp_.to_table() == str(g["to_table"])


def test_create_baseline_controllers_returns_the_references_keys(g, monkeypatch):
    table = g["ol_table"]
    got = ex.create_baseline_controllers(DYN, None, (np.zeros((3, 7)), table))
    assert list(got) == g["controller_keys"].tolist() == ["LQR", "PID", "Open_Loop"]
    assert [type(v) for v in got.values()] == [ex.LQRController, ex.PIDController, ex.OpenLoopController]
    assert list(ex.create_baseline_controllers(DYN)) == ["LQR", "PID"]
    # with an MPC configuration the reference means this package's NominalMPC3DoF
    import gp_mpc_rocket_landing_amd.mpc as mpc
    made = []
    monkeypatch.setattr(mpc, "NominalMPC3DoF", lambda dyn, cfg: made.append((dyn, cfg)) or "the MPC")   # no device here
    got = ex.create_baseline_controllers(DYN, "a config")
    assert list(got) == ["LQR", "PID", "Nominal_MPC"] and type(got["Nominal_MPC"]) is ex.NominalMPCWrapper
    assert made == [(DYN, "a config")] and got["Nominal_MPC"].mpc == "the MPC"


def test_the_riccati_branch_is_the_live_one_and_the_fallback_runs(monkeypatch):
    x0 = np.array([2.0, 30.0, 1.0, -1.0, -3.0, 0.2, 0.1])
    xt = np.zeros(7); xt[0] = 2.0
    lqr = ex.LQRController(DYN)
    with pytest.raises(RuntimeError):
        lqr.solve(x0)
    lqr.initialize(x0, xt)
    assert np.array_equal(lqr.u_hover, [2.0, 0.0, 0.0]) and lqr.K.shape == (3, 7)
    A, B = lqr._linearize(xt, lqr.u_hover)
    P = linalg.solve_discrete_are(A, B, lqr._build_Q(), lqr._build_R())
    assert np.linalg.cond(P) < 100 and np.array_equal(lqr.K, np.linalg.inv(lqr._build_R() + B.T @ P @ B) @ B.T @ P @ A)
    assert lqr.clips() == (0.0, 6.5, 0.5)   # Rocket3DoFParams has no gimbal_max
    u = lqr.solve(x0, xt).u0
    assert 0.0 <= u[0] <= 6.5 and np.all(np.abs(u[1:]) <= 0.5)

    class Broken(Rocket3DoFDynamics):   # a plant whose Riccati solve raises: NaN in A
        def step(self, x, u, dt=None):
            return super().step(x, u, dt) * np.nan

    fb = ex.LQRController(Broken())
    fb.initialize(x0, xt)
    K = np.zeros((3, 7))
    K[0, 1], K[0, 4], K[1, 2], K[1, 5], K[2, 3], K[2, 6] = -1.0, -2.0, 0.2, 0.5, 0.2, 0.5
    assert np.array_equal(fb.K, K)
    dx = x0 - xt
    want = np.array([2.0, 0.0, 0.0]) + -K @ dx
    assert np.array_equal(fb.solve(x0, xt).u0, [np.clip(want[0], 0.0, 6.5), *np.clip(want[1:], -0.5, 0.5)])


def test_pid_state_open_loop_index_and_wrappers():
    xt = np.zeros(7); xt[0] = 2.0
    x = np.array([2.0, 30.0, 1.0, -1.0, -3.0, 0.2, 0.1])
    pid = ex.PIDController(DYN, ex.PIDConfig(max_integral=4.0))
    pid.initialize(x, xt)
    assert pid.dt == 0.1 and pid.g == 1.0
    for _ in range(3):
        sol = pid.solve(x, xt)
    want = np.zeros(3)
    for _ in range(3):   # the integral takes its own dt = 0.1 and is clipped every step
        want = np.clip(want + (xt[1:4] - x[1:4]) * 0.1, -4.0, 4.0)
    assert np.array_equal(pid.integral_error, want)
    assert pid.integral_error[0] == -4.0 and sol.u0[0] == 0.3 and np.all(np.abs(sol.u0[1:]) <= 1.5)
    assert np.array_equal(sol.error, xt[1:4] - x[1:4]) and np.array_equal(pid.prev_error, sol.error)
    pid.initialize(x, xt)
    assert np.array_equal(pid.integral_error, np.zeros(3))
    U = np.arange(6.0).reshape(2, 3)
    ol = ex.OpenLoopController(np.zeros((3, 7)), U)
    got = [ol.solve(x).u0 for _ in range(4)]
    assert np.array_equal(got, [U[0], U[1], U[1], U[1]]) and ol.step_idx == 4
    got[0][0] = 99.0
    assert U[0, 0] == 0.0   # a copy
    ol.initialize(x, xt)
    assert ol.step_idx == 0 and ol.t == 0.0

    class Stepper:
        def step(self, x):
            return "step"

    class Solver:
        def initialize(self, x0, xt):
            self.seen = (x0, xt)

        def solve(self, x, target):
            return target

    assert ex.NominalMPCWrapper(Stepper()).solve(x) == "step"
    w = ex.NominalMPCWrapper(Solver())
    w.initialize(x, xt)
    assert np.array_equal(w.solve(x), xt) and w.mpc.seen[0] is x
    t = ex.TubeMPCWrapper(Solver())
    t.initialize(x, xt)
    assert np.array_equal(t.solve(x), xt) and np.array_equal(t.solve(x, x), x)


def test_dispersion_configs_and_samples():
    assert [m.name for m in ex.WindModel] == ["NONE", "CONSTANT", "GUST", "DRYDEN", "CUSTOM"]
    assert [m.value for m in ex.WindModel] == [1, 2, 3, 4, 5]
    lo, me, hi = ex.DispersionConfig.low(), ex.DispersionConfig.medium(), ex.DispersionConfig.high()
    assert ex.DispersionConfig.nominal().wind.model is ex.WindModel.NONE and not ex.DispersionConfig.nominal().thrust.enabled
    assert lo.wind.model is ex.WindModel.CONSTANT and np.array_equal(lo.wind.wind_velocity, [2.0, 1.0, 0.0])
    assert (lo.aero.Cd_std, lo.thrust.thrust_scale_std, lo.thrust.misalignment_std) == (0.05, 0.01, 0.01)
    assert (me.wind.model, me.wind.turbulence_intensity, me.aero.Cd_std) == (ex.WindModel.DRYDEN, 1.0, 0.1)
    assert (hi.wind.turbulence_intensity, hi.aero.Cd_std, hi.thrust.thrust_scale_std, hi.thrust.misalignment_std,
            hi.thrust.fluctuation_std) == (2.0, 0.2, 0.05, 0.02, 0.02)
    assert np.array_equal(ex.WindConfig(model=ex.WindModel.CUSTOM).get_wind(1.0, np.ones(3), 3), np.zeros(3))
    off = ex.AeroDispersionConfig().sample(5)
    assert (off["Cd"], off["A"]) == (0.5, 1.0) and np.array_equal(off["cp_offset"], np.zeros(3))
    rs = np.random.RandomState(5)
    on = ex.AeroDispersionConfig(enabled=True).sample(5)
    assert (on["Cd"], on["A"]) == (0.5 + rs.randn() * 0.1, 1.0 + rs.randn() * 0.05)
    nominal = np.arange(7.0)
    rs = np.random.RandomState(9)
    want = nominal + rs.randn(7) * np.array([0.05, 10.0, 10.0, 20.0, 5.0, 5.0, 10.0])
    assert np.array_equal(ex.InitialConditionDispersion().sample(nominal, 9), want) and nominal[1] == 1.0
    u = np.array([3.0, 0.1, -0.1])
    assert np.array_equal(ex.ThrustDispersionConfig().apply_dispersion(u, 3), u)
    d = ex.DispersedDynamics(DYN, me, seed=7)
    assert d.params is DYN.params and d.step_count == 0
    d.step(np.array([2.0, 30, 0, 0, -3, 0, 0.0]), u, 0.1)
    assert d.step_count == 1
    d.reset()
    assert d.step_count == 0
    with contextlib.redirect_stdout(io.StringIO()) as out:
        an = ex.DispersionAnalysis(DYN, ex.PIDController(DYN), ex.SimulationConfig(max_time=0.5))
        an.use_fleet = False
        sweep = an.run_sweep(n_runs_per_level=3, seed=42)
    assert list(sweep) == ["nominal", "low", "medium", "high"] and [r.config_name for r in sweep.values()] == list(sweep)
    assert out.getvalue().startswith("Dispersion Analysis Sweep\n" + "=" * 50 + "\n\nRunning nominal dispersion level...")
