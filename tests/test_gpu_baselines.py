"""The baseline controllers' device batch (csrc/baseline.hip) against the reference's recorded
landings (tests/golden/baselines.npz).  The device rule (baseline_cases.py, DESIGN.md section
21): outcome and step count equal exactly; states and controls within F x the stored spread
+ 8 ulp, F = 64; no case is left out (the fixture's generator asserts every discrete decision
lies >= 1000 x F x its spread from its threshold).  Row i of every batch equals the B = 1 answer
bit for bit."""
import contextlib
import io

import numpy as np
import pytest

import baseline_cases as bc
from gp_mpc_rocket_landing_amd import _lib
from gp_mpc_rocket_landing_amd.dynamics.rocket_3dof import Rocket3DoFDynamics
from gp_mpc_rocket_landing_amd.experiments import (DispersionAnalysis, DispersionConfig, LQRController,
                                                   MonteCarloSimulator, PIDController, SimulationConfig,
                                                   compare_controllers, dispersion, mc_noise_table,
                                                   sample_initial_condition)
from gp_mpc_rocket_landing_amd.experiments.baselines import controller_batch, device_gate

pytestmark = pytest.mark.gpu
PKG = bc.package_modules()
DYN = Rocket3DoFDynamics()


@pytest.fixture(scope="module")
def g(gpu_ctx):
    return bc.load()


def fly_device(group, table):
    """The group's landings through the drivers' device path -> [SimulationResult]."""
    cfg_name, ctl_name, plant, seed, n = bc.GROUPS[group]
    cfg = bc.make_config(PKG, cfg_name)
    if plant == "sim":
        cfg.thrust_dispersion, cfg.aero_dispersion = 0.02, 1.0
    ctl = bc.make_controller(PKG, ctl_name, DYN, table)
    if plant in bc.DISPERSED:
        an = DispersionAnalysis(DYN, ctl, cfg)
        kind, why = an._baseline_plan(cfg)
        assert kind is not None, why
        return an._fly_batch(kind, cfg, bc.make_dispersion(PKG, plant), n, seed)
    sim = MonteCarloSimulator(DYN, ctl, cfg)
    res = sim.run(n, seed=seed)
    assert (sim.last_path, sim.last_path_reason) == ("baselines", "")
    return res.results


def check(what, got, want, spread, worst):
    got, want = np.asarray(got, float), np.asarray(want, float)
    lim = bc.bound(want, spread)
    err = np.abs(got - want)
    frac = float(np.max(err / lim)) if err.size else 0.0
    worst[0] = max(worst[0], frac)
    assert np.all(err <= lim), f"{what}: error {err.max():.3e} is {frac:.3g} of the bound"


@pytest.mark.parametrize("group", list(bc.GROUPS))
def test_every_fixture_case_meets_the_device_rule(g, group):
    res = fly_device(group, g["ol_table"])
    sx, su = g[f"{group}_spread_x"], g[f"{group}_spread_u"]
    assert [r.outcome.value for r in res] == g[f"{group}_outcomes"].tolist()
    assert [len(r.controls) for r in res] == g[f"{group}_nsteps"].tolist()
    assert [r.failure_reason for r in res] == g[f"{group}_reasons"].tolist()
    worst = [0.0]
    for i, r in enumerate(res):
        assert np.array_equal(r.initial_state, g[f"{group}_x0"][i]) and np.array_equal(r.states[0], r.initial_state)
        check(f"{group}[{i}] final state", r.states[-1], g[f"{group}_final"][i], sx[i], worst)
        check(f"{group}[{i}] fuel", r.fuel_used, g[f"{group}_fuel"][i], sx[i, 0], worst)
        ft = g[f"{group}_flight_time"][i]   # T accumulated additions of dt against T x dt: half an ulp each
        assert abs(r.flight_time - ft) <= (0.5 * len(r.controls) + 1) * np.spacing(ft) and r.success == (r.outcome.value == 1)
        check(f"{group}[{i}] position error", r.final_position_error, g[f"{group}_pos_err"][i], sx[i, 1:4].sum(), worst)
        check(f"{group}[{i}] velocity error", r.final_velocity_error, g[f"{group}_vel_err"][i], sx[i, 4:7].sum(), worst)
        if i < bc.N_FULL:
            check(f"{group}[{i}] states", r.states, g[f"{group}_states{i}"], sx[i], worst)
            check(f"{group}[{i}] controls", r.controls, g[f"{group}_controls{i}"], su[i], worst)
    print(f"{group}: largest error {worst[0]:.3g} of the bound")


def raw_fly(ctx, kind_name, x0s, plant_kw, cfg, table, noise=None):
    ctl = bc.make_controller(PKG, kind_name, DYN, table)
    kind, why = device_gate(ctl)
    assert kind is not None, why
    kw = controller_batch(ctl, kind, x0s)
    kw.update(plant_kw)
    if noise is not None:
        kw.update(sim_thrust=0.02, sim_aero=1.0, noise=noise)
    return _lib.baseline_fly(ctx, x0s, max_steps=int(cfg.max_time / cfg.dt), dt=cfg.dt, **kw)


def same_rows(big, small, i):
    (rec, ns, log), (rec1, ns1, log1) = big, small
    T = int(ns1[0])
    return ns[i] == T and np.array_equal(rec[i], rec1[0]) and np.array_equal(log[:T, i], log1[:T, 0])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind_name,plant", [("lqr", "high"), ("pid", "gust"), ("ol", "sim")])
def test_batch_rows_equal_the_single_landing_bit_for_bit(gpu_ctx, g, B, kind_name, plant):
    """B = 130 is three workgroups, the last partial; the landings of one wave end at
    different steps.  A single landing of a dispersed plant is the batch of its own seed."""
    cfg = SimulationConfig.run_experiments()
    seed, T = 42, 300
    x0s = np.array([sample_initial_condition(seed + i, cfg) for i in range(B)])
    if plant == "sim":
        cfg.thrust_dispersion, cfg.aero_dispersion = 0.02, 1.0
        noise = mc_noise_table(seed, B, cfg)
        big = raw_fly(gpu_ctx, kind_name, x0s, {}, cfg, g["ol_table"], noise)
        rows = sorted({0, B // 2, B - 1})
        assert all(same_rows(big, raw_fly(gpu_ctx, kind_name, x0s[i:i + 1], {}, cfg, g["ol_table"], noise[i:i + 1]), i)
                   for i in rows)
    else:
        dcfg = bc.make_dispersion(PKG, plant)
        big = raw_fly(gpu_ctx, kind_name, x0s, dispersion.plant_batch(dcfg, seed, B, cfg.dt, T), cfg, g["ol_table"])
        rows = sorted({0, B // 2, B - 1})
        assert all(same_rows(big, raw_fly(gpu_ctx, kind_name, x0s[i:i + 1],
                                          dispersion.plant_batch(dcfg, seed + i, 1, cfg.dt, T), cfg, g["ol_table"]), i)
                   for i in rows)
    rec, ns, log = big
    assert np.all(rec[:, 0] >= 1) and np.all(rec[:, 1] == ns) and np.all(rec[:, 3] == ns * cfg.dt)
    assert np.all(rec[:, [11, 12, 14, 15]] == 0) and np.array_equal(rec[:, 13], x0s[:, 0])
    if B >= 63:
        assert len(set(ns[:64].tolist())) > 8   # one wave, many different last steps


def test_a_wave_with_lanes_that_run_to_max_steps_beside_early_finishers(g):
    """short_lqr_plain is one wave: TIMEOUT at max_steps beside FUEL_EXHAUSTED before it."""
    ns, out = g["short_lqr_plain_nsteps"], g["short_lqr_plain_outcomes"]
    assert ns.max() == 55 and ns.min() < 55 and set(out.tolist()) == {3, 5}
    res = fly_device("short_lqr_plain", g["ol_table"])
    assert [len(r.controls) for r in res] == ns.tolist() and [r.outcome.value for r in res] == out.tolist()
    assert all(r.failure_reason == "Exceeded 5.5s" for r in res if r.outcome.value == 5)


def test_records_without_the_log(gpu_ctx, g):
    """log = 0: no log buffer on either side.  The records of the first two short_lqr_plain
    landings against the fixture, under the device rule."""
    group = "short_lqr_plain"
    cfg = bc.make_config(PKG, "short")
    x0s = g[f"{group}_x0"][:2]
    ctl = bc.make_controller(PKG, "lqr", DYN, g["ol_table"])
    kind, why = device_gate(ctl)
    assert kind is not None, why
    rec, ns, log = _lib.baseline_fly(gpu_ctx, x0s, max_steps=int(cfg.max_time / cfg.dt), dt=cfg.dt, log=False,
                                     alpha=float(DYN.params.alpha), g=np.asarray(DYN.params.g_vec, float),
                                     **controller_batch(ctl, kind, x0s))
    assert log is None
    assert ns.tolist() == g[f"{group}_nsteps"][:2].tolist() and np.array_equal(rec[:, 1], ns)
    worst = [0.0]
    for i in range(2):
        sx = g[f"{group}_spread_x"][i]
        check(f"{group}[{i}] final state", rec[i, 4:11], g[f"{group}_final"][i], sx, worst)
        check(f"{group}[{i}] fuel", rec[i, 2], g[f"{group}_fuel"][i], sx[0], worst)


def test_a_wave_where_the_drag_term_is_on_for_some_lanes_only(g):
    """exp_pid_high: at some step speed > 1 holds on some lanes and not on others; every lane's
    whole trajectory meets the rule through that step (the stored lanes) and to the end."""
    X = [g[f"exp_pid_high_states{i}"] for i in range(bc.N_FULL)]
    mixed = [t for t in range(min(len(x) for x in X) - 1)
             if len({bool(np.linalg.norm(x[t, 4:7]) > 1.0) for x in X}) == 2]
    assert mixed
    res = fly_device("exp_pid_high", g["ol_table"])
    worst = [0.0]
    for i in range(bc.N_FULL):
        check(f"lane {i}", res[i].states, X[i], g["exp_pid_high_spread_x"][i], worst)


def agree(a, b, spreads_x, spreads_u):
    worst = [0.0]
    assert [r.outcome for r in a] == [r.outcome for r in b] and [len(r.controls) for r in a] == [len(r.controls) for r in b]
    for i, (r, h) in enumerate(zip(a, b)):
        check(f"states {i}", r.states, h.states, spreads_x[i], worst)
        check(f"controls {i}", r.controls, h.controls, spreads_u[i], worst)


def test_run_takes_the_device_and_agrees_with_its_loop(g):
    for group, C in (("exp_lqr_plain", LQRController), ("exp_pid_plain", PIDController)):
        _, _, _, seed, n = bc.GROUPS[group]
        sim = MonteCarloSimulator(DYN, C(DYN), SimulationConfig.run_experiments())
        seen = []
        dev = sim.run(n, seed=seed, progress_callback=lambda k, m: seen.append((k, m)))
        assert sim.last_path == "baselines" and seen == [(n, n)]
        with contextlib.redirect_stdout(io.StringIO()):
            host = sim.run(n, seed=seed, use_fleet=False)
        assert (sim.last_path, sim.last_path_reason) == ("loop", "use_fleet=False")
        agree(dev.results, host.results, g[f"{group}_spread_x"], g[f"{group}_spread_u"])
        assert dev.get_statistics()["outcomes"] == host.get_statistics()["outcomes"]
    # n_workers = 2 without dispersions: the one-stream initial conditions, still on the device
    sim = MonteCarloSimulator(DYN, LQRController(DYN), SimulationConfig.run_experiments())
    with contextlib.redirect_stdout(io.StringIO()):
        dev = sim.run(5, n_workers=2, seed=43)
        assert sim.last_path == "baselines"
        host = sim.run(5, n_workers=2, seed=43, use_fleet=False)
    assert all(np.array_equal(a.initial_state, b.initial_state) and a.outcome == b.outcome and
               len(a.controls) == len(b.controls) for a, b in zip(dev.results, host.results))


def test_compare_controllers_takes_the_device_for_the_baselines(g):
    class Lander:   # any other controller keeps run_single
        def solve(self, x, x_target):
            return type("S", (), {"u0": np.array([x[0], 0.0, 0.0])})()

    cfg = SimulationConfig.run_experiments()
    ctl = {"LQR": LQRController(DYN), "PID": PIDController(DYN), "other": Lander()}
    with contextlib.redirect_stdout(io.StringIO()):
        dev = compare_controllers(DYN, ctl, n_runs=6, config=cfg, seed=42)
        paths = dict(compare_controllers.last_paths)
        host = compare_controllers(DYN, ctl, n_runs=6, config=cfg, seed=42, use_fleet=False)
    assert paths["LQR"] == ("baselines", "") and paths["PID"] == ("baselines", "") and paths["other"][0] == "loop"
    assert all(v == ("loop", "use_fleet=False") for v in compare_controllers.last_paths.values())
    # these landings are not fixture cases: their spread is measured here, by the fixture's probe
    sx = {name: np.zeros((6, 7)) for name in ("LQR", "PID")}
    su = {name: np.zeros((6, 3)) for name in ("LQR", "PID")}
    for stream in (1, 2):
        with contextlib.redirect_stdout(io.StringIO()):
            per = compare_controllers(bc.Perturbed(DYN, stream), {k: ctl[k] for k in sx}, n_runs=6, config=cfg, seed=42)
        for name in sx:
            for i, (a, b) in enumerate(zip(host[name].results, per[name].results)):
                assert len(a.controls) == len(b.controls)
                sx[name][i] = np.maximum(sx[name][i], np.abs(a.states - b.states).max(axis=0))
                su[name][i] = np.maximum(su[name][i], np.abs(a.controls - b.controls).max(axis=0))
    for name in ("LQR", "PID"):
        agree(dev[name].results, host[name].results, sx[name], su[name])
    assert all(np.array_equal(a.states, b.states) for a, b in zip(dev["other"].results, host["other"].results))


@pytest.mark.parametrize("group", ["exp_lqr_medium", "exp_pid_high", "exp_lqr_gust", "exp_pid_low"])
def test_dispersion_analysis_takes_the_device_and_agrees_with_its_loop(g, group):
    cfg_name, ctl_name, plant, seed, n = bc.GROUPS[group]
    an = DispersionAnalysis(DYN, bc.make_controller(PKG, ctl_name, DYN, g["ol_table"]), bc.make_config(PKG, cfg_name))
    dev = an.run_single(bc.make_dispersion(PKG, plant), n_runs=n, seed=seed)
    assert (an.last_path, an.last_path_reason) == ("baselines", "")
    an.use_fleet = False
    host = an.run_single(bc.make_dispersion(PKG, plant), n_runs=n, seed=seed)
    assert (an.last_path, an.last_path_reason) == ("loop", "use_fleet=False")
    sx = g[f"{group}_spread_x"]
    worst = [0.0]
    check("final positions", dev.final_positions, host.final_positions, sx[:, 1:4], worst)
    check("final velocities", dev.final_velocities, host.final_velocities, sx[:, 4:7], worst)
    assert dev.n_success == host.n_success == int(g[f"{group}_an_n_success"])
    assert np.array_equal(host.position_cov, g[f"{group}_an_position_cov"])
    assert np.array_equal(dev.position_cov, np.cov(dev.final_positions.T))
    assert np.array_equal(dev.velocity_mean, np.mean(dev.final_velocities, axis=0))


def test_refusals_return_minus_two_with_a_message_before_any_launch(gpu_ctx):
    x0 = np.array([[2.0, 30.0, 0.0, 0.0, -3.0, 0.0, 0.0]])
    K, uh = np.zeros((1, 3, 7)), np.array([[2.0, 0.0, 0.0]])
    ok = dict(kind=0, max_steps=5, dt=0.1, K=K, u_hover=uh)
    rec, ns, log = _lib.baseline_fly(gpu_ctx, x0, **ok)
    assert rec[0, 0] == 5 and ns[0] == 5
    bad = [(dict(kind=3), "unknown controller kind"), (dict(max_steps=0), "max_steps"), (dict(dt=0.0), "dt must be"),
           (dict(dt=float("nan")), "dt must be"), (dict(K=None), "needs K"), (dict(K=K * np.nan), "not finite"),
           (dict(u_hover=np.full((1, 3), np.inf)), "not finite"), (dict(kind=2), "open-loop table is empty"),
           (dict(thrust_table=np.ones((5, 4))), "thrust table needs"),
           (dict(wind_table=np.zeros((1, 3)), wind_rows=np.array([0, 0, 1, 0, 0])), "wind row"),
           (dict(wind_table=np.zeros((1, 3)), wind_rows=np.array([0, 0, -1, 0, 0])), "wind row"),
           (dict(sim_thrust=0.1), "noise table")]
    for change, text in bad:
        with pytest.raises(_lib.HIPError, match=text) as e:
            _lib.baseline_fly(gpu_ctx, x0, **{**ok, **change})
        assert e.value.rc == -2
    with pytest.raises(_lib.HIPError, match="x0 is not finite") as e:
        _lib.baseline_fly(gpu_ctx, x0 * np.nan, **ok)
    assert e.value.rc == -2
    cfg = _lib.baseline_default_config(batch=0)
    none = (None,) * 8
    assert _lib._L.gpmpc_baseline_fly(gpu_ctx.h, cfg, None, *none, None, None, None, None) == -2
    assert b"must not be null" in _lib._L.gpmpc_last_error()
    r, n = np.zeros(16), np.zeros(1, np.int32)
    assert _lib._L.gpmpc_baseline_fly(gpu_ctx.h, cfg, _lib._d(x0), *none, _lib._d(r), _lib._i(n), None, None) == -2
    assert b"batch = 0" in _lib._L.gpmpc_last_error()
    rec2, ns2, _ = _lib.baseline_fly(gpu_ctx, x0, **ok)   # the context stays usable
    assert np.array_equal(rec, rec2)
