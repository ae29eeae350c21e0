"""MonteCarloSimulator.run on the device fleet: the Monte-Carlo attachment (trajectory log,
plant dispersions) of csrc/fleet.hip through Fleet.attach_mc / read_log and through the
reference's driver classes.  Exact GP at 1000 training rows, N = 20, at most 8 landings."""
import contextlib
import io

import numpy as np
import pytest

from conftest import close

pytestmark = pytest.mark.gpu

N, DT, B = 20, 0.1, 8


def _euler(x, u, dt):
    """numpy explicit Euler of the 3-DoF plant (rocket_3dof.py): x + dt f(x, u)."""
    f = np.empty(7)
    f[0] = -(1.0 / 30.0) * np.sqrt(u @ u)
    f[1:4] = x[4:7]
    f[4:7] = u / x[0] + np.array([-1.0, 0.0, 0.0])
    return x + dt * f


def _euler_bound(x):
    # fewer than ~20 fp64 roundings a component, FMA contraction allowed: 1e-12 max(|x|, 1)
    return 1e-12 * np.maximum(np.abs(x), 1.0)


def _fly(fl, max_steps, chunk=25):
    from gp_mpc_rocket_landing_amd.fleet import REC_OUTCOME
    done = 0
    while done < max_steps + 1:
        k = min(chunk, max_steps + 1 - done)
        fl.step(k)
        done += k
        rec, _ = fl.read()
        if np.all(rec[:, REC_OUTCOME] != 0):
            break
    return rec


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    """The host GP (its device handle is the fleet's GP), the plant and a simulator factory."""
    from gp_mpc_rocket_landing_amd import _lib
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.experiments import MonteCarloSimulator, SimulationConfig
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import GPMPC, GPMPCConfig
    _lib._default_ctx = gpu_ctx
    X, U, D = synthetic_training_data(1000, seed=0)
    gp = Simple3DoFGP(use_sparse=False)
    gp.add_data(X, U, D)
    gp.fit()
    dyn = create_normalized_rocket()

    def simulator(config=None, **mpc):
        ctl = GPMPC(dyn, gp, GPMPCConfig(N=N, dt=DT, **mpc), ctx=gpu_ctx)
        sim = MonteCarloSimulator(dyn, ctl, config or SimulationConfig.run_experiments())
        sim.keep_raw_log = True
        return sim
    return dict(ctx=gpu_ctx, gp=gp, handle=gp.gp.device_handle, dyn=dyn, simulator=simulator)


@pytest.fixture(scope="module")
def nominal(rig):
    """run(8, seed 42) under run_experiments() on the fleet, and the same landings on a
    plain Fleet(residual_model=0) with nothing attached.  Computed once, never modified."""
    from gp_mpc_rocket_landing_amd.fleet import Fleet, initial_conditions
    sim = rig["simulator"]()
    calls = []
    res = sim.run(n_runs=B, seed=42, progress_callback=lambda d, n: calls.append((d, n)))
    x0 = initial_conditions(B, 42)
    fl = Fleet(rig["ctx"], rig["handle"], B, horizon=N, dt=DT, residual_model=0, max_steps=300)
    try:
        fl.reset(x0)
        rec = _fly(fl, 300)
    finally:
        fl.close()
    return dict(sim=sim, res=res, x0=x0, plain=rec, raw=sim.last_raw_log, calls=calls)


def test_run_takes_the_fleet_and_attaching_changes_no_result(nominal):
    from gp_mpc_rocket_landing_amd.experiments import LandingOutcome, MonteCarloResults, SimulationResult
    from gp_mpc_rocket_landing_amd.fleet import (REC_ADMM_ITERS, REC_FUEL, REC_LAST_STATUS, REC_OUTCOME, REC_STATE,
                                                 REC_STEPS, REC_TIME)
    sim, res, rec = nominal["sim"], nominal["res"], nominal["plain"]
    assert sim.last_path == "fleet" and res.n_runs == B
    np.testing.assert_array_equal(nominal["raw"]["records"], rec)      # every record slot, bit for bit
    built = []
    for i, r in enumerate(res.results):
        code = int(rec[i, REC_OUTCOME])
        assert code != 0
        ok, why = sim.config.landing_constraints.check_landing(rec[i, REC_STATE], rec[i, 13])
        want = {1: LandingOutcome.SUCCESS if ok else LandingOutcome.CONSTRAINT_VIOLATION,
                4: LandingOutcome.SUCCESS if ok else LandingOutcome.CONSTRAINT_VIOLATION}.get(
                    code, LandingOutcome(code))
        assert code != 1 or ok     # the compiled tolerances are run_experiments()'s
        assert r.outcome == want and r.success == (want == LandingOutcome.SUCCESS)
        assert len(r.controls) == int(rec[i, REC_STEPS])
        assert r.fuel_used == rec[i, REC_FUEL] and r.flight_time == rec[i, REC_TIME]
        np.testing.assert_array_equal(r.states[-1], rec[i, REC_STATE])
        np.testing.assert_array_equal(r.initial_state, nominal["x0"][i])
        assert r.metadata["admm_iterations"] == int(rec[i, REC_ADMM_ITERS])
        assert r.metadata["last_qp_status"] == int(rec[i, REC_LAST_STATUS])
        np.testing.assert_array_equal(r.times, DT * np.arange(len(r.controls) + 1))
        xf = rec[i, REC_STATE]
        built.append(SimulationResult(
            run_id=i, outcome=want, success=want == LandingOutcome.SUCCESS, states=np.vstack([nominal["x0"][i], xf]),
            controls=np.zeros((0, 3)), times=np.zeros(2), fuel_used=rec[i, REC_FUEL], flight_time=rec[i, REC_TIME],
            final_position_error=np.linalg.norm(xf[1:4]), final_velocity_error=np.linalg.norm(xf[4:7]),
            max_constraint_violation=0.0, initial_state=nominal["x0"][i], compute_time_ms=r.compute_time_ms))
    assert res.get_statistics() == MonteCarloResults(config=sim.config, results=built).get_statistics()
    assert "Monte Carlo Simulation Results" in res.summary()
    # progress: once per chunk, the count of terminated landings, ending with all of them
    calls = nominal["calls"]
    assert calls and calls[-1] == (B, B) and all(n == B for _, n in calls)
    assert [d for d, _ in calls] == sorted(d for d, _ in calls)
    assert len(calls) <= -(-301 // sim.fleet_chunk)


def test_log_is_consistent_with_the_records_and_the_plant(nominal):
    from gp_mpc_rocket_landing_amd.fleet import REC_STATE, REC_STEPS
    raw, rec = nominal["raw"], nominal["plain"]
    assert raw["states"].shape == (B, 301, 7) and raw["controls"].shape == (B, 300, 3)
    for i, r in enumerate(nominal["res"].results):
        T = int(rec[i, REC_STEPS])
        assert raw["nsteps"][i] == T == len(r.controls) and r.states.shape == (T + 1, 7)
        np.testing.assert_array_equal(r.states[0], nominal["x0"][i])
        np.testing.assert_array_equal(r.states[-1], rec[i, REC_STATE])
        np.testing.assert_array_equal(raw["states"][i, :T + 1], r.states)
        np.testing.assert_array_equal(raw["controls"][i, :T], r.controls)
        assert np.all(np.isnan(raw["states"][i, T + 1:])) and np.all(np.isnan(raw["controls"][i, T:]))
        assert np.all(np.isfinite(r.states)) and np.all(np.isfinite(r.controls))
        for t in range(T):
            want = _euler(r.states[t], r.controls[t], DT)
            assert np.all(np.abs(r.states[t + 1] - want) <= _euler_bound(want)), (i, t)


def test_dispersions_match_the_loop_and_the_noise_table(rig):
    """thrust 0.02 / aero 1.0, max_time 1.0: ten steps, every landing times out.  Fleet
    against run(use_fleet=False): outcomes, steps and per-step ADMM iterations equal,
    states within close(a, b, 1.0); and the logged dispersion terms are the noise table's
    (pins the draw order on the device)."""
    from gp_mpc_rocket_landing_amd.experiments import LandingOutcome, SimulationConfig, mc_noise_table
    cfg = SimulationConfig.run_experiments()
    cfg.max_time, cfg.thrust_dispersion, cfg.aero_dispersion = 1.0, 0.02, 1.0
    sim = rig["simulator"](cfg)
    sim.fleet_chunk = 1
    dev = sim.run(n_runs=B, seed=42)
    assert sim.last_path == "fleet"
    host = sim.run(n_runs=B, seed=42, use_fleet=False)
    assert sim.last_path == "loop"
    table = mc_noise_table(42, B, cfg)
    for i, (a, b) in enumerate(zip(dev.results, host.results)):
        assert a.outcome == b.outcome == LandingOutcome.TIMEOUT and a.failure_reason == b.failure_reason
        assert len(a.controls) == len(b.controls) == 10
        print(i, "ADMM/step fleet", a.metadata["admm_iterations_per_step"], "loop",
              b.metadata["admm_iterations_per_step"], "state ratio", close(a.states, b.states, 1.0)[1])
        assert a.metadata["admm_iterations_per_step"] == b.metadata["admm_iterations_per_step"]
        assert a.metadata["admm_iterations"] == b.metadata["admm_iterations"]
        np.testing.assert_array_equal(a.states[0], b.states[0])
        assert close(a.states, b.states, 1.0)[0], i
        assert close(a.controls, b.controls, 1.0)[0], i
        for t in range(10):
            x, u, n = a.states[t], a.controls[t], table[i, t]
            got = a.states[t + 1] - _euler(x, u, DT)
            want = n[0] * cfg.thrust_dispersion * u[0] / x[0] * DT + n[1:4] * cfg.aero_dispersion * DT
            assert np.all(np.abs(got[:4]) <= _euler_bound(a.states[t + 1][:4])), (i, t)
            assert np.all(np.abs(got[4:7] - want) <= _euler_bound(a.states[t + 1][4:7])), (i, t)
    # the dispersions did something: the nominal flight of the same landings differs
    cfg0 = SimulationConfig.run_experiments()
    cfg0.max_time = 1.0
    nom = rig["simulator"](cfg0).run(n_runs=2, seed=42)
    assert not np.array_equal(nom.results[0].states[1], dev.results[0].states[1])
    np.testing.assert_array_equal(nom.results[0].states[0], dev.results[0].states[0])


def test_run_with_dispersions_flies_every_level_on_the_fleet(rig):
    from gp_mpc_rocket_landing_amd.experiments import SimulationConfig
    cfg = SimulationConfig.run_experiments()
    cfg.max_time = 1.0
    sim = rig["simulator"](cfg)
    paths, run = [], sim.run

    def recorded(**kw):
        out = run(**kw)
        paths.append(sim.last_path)
        return out
    sim.run = recorded
    with contextlib.redirect_stdout(io.StringIO()):
        out = sim.run_with_dispersions(n_runs=4, dispersion_configs=[
            {"name": "nominal", "thrust_dispersion": 0.0, "aero_dispersion": 0.0},
            {"name": "med_disp", "thrust_dispersion": 0.02, "aero_dispersion": 1.0}])
    assert list(out) == ["nominal", "med_disp"] and paths == ["fleet", "fleet"]
    assert all(r.n_runs == 4 for r in out.values())
    a, b = out["nominal"].results[0], out["med_disp"].results[0]
    np.testing.assert_array_equal(a.states[0], b.states[0])
    assert not np.array_equal(a.states[1], b.states[1])


def test_sqp_mode_appends_once_per_control_step(rig):
    """max_sqp_iter = 3, 4 landings, 5 steps: up to three control launches a step, one append.
    sqp_tol = 1.0 so that the loop converges and the plant steps: at the reference's 1e-4 the
    1e-4 ADMM never converges the loop, and every landing ends DIVERGENCE before its first
    step (test_fleet_sqp_mode_matches_oracle), which would append nothing at all."""
    from gp_mpc_rocket_landing_amd.experiments import SimulationConfig
    from gp_mpc_rocket_landing_amd.fleet import REC_STATE, REC_STEPS
    cfg = SimulationConfig.run_experiments()
    cfg.max_time = 0.5
    sim = rig["simulator"](cfg, max_sqp_iter=3, sqp_tol=1.0)
    res = sim.run(n_runs=4, seed=42)
    assert sim.last_path == "fleet"
    raw = sim.last_raw_log
    assert raw["states"].shape == (4, 6, 7)
    print("SQP steps", raw["nsteps"].tolist(), "outcomes", raw["records"][:, 0].tolist())
    assert np.sum(raw["nsteps"]) > 4      # the converged branch ran, more than once a landing
    for i, r in enumerate(res.results):
        T = int(raw["records"][i, REC_STEPS])
        assert raw["nsteps"][i] == T == len(r.controls) <= 5
        np.testing.assert_array_equal(r.states[-1], raw["records"][i, REC_STATE])
        assert np.all(np.isnan(raw["states"][i, T + 1:]))
        for t in range(T):
            want = _euler(r.states[t], r.controls[t], DT)
            assert np.all(np.abs(r.states[t + 1] - want) <= _euler_bound(want)), (i, t)


def test_custom_landing_constraints_are_decided_on_the_host(rig, nominal):
    """vel_tol_z = 0.5 on the run of the first test: the device flies the same landings
    (states untouched), the host turns landed-but-too-fast ones into CONSTRAINT_VIOLATION
    with the reference's reason text."""
    from gp_mpc_rocket_landing_amd.experiments import LandingConstraints, LandingOutcome, SimulationConfig
    cfg = SimulationConfig.run_experiments()
    cfg.landing_constraints = LandingConstraints(pos_tol_xy=5.0, vel_tol_z=0.5)
    sim = rig["simulator"](cfg)
    res = sim.run(n_runs=B, seed=42)
    assert sim.last_path == "fleet"
    turned = 0
    for a, b in zip(nominal["res"].results, res.results):
        np.testing.assert_array_equal(a.states, b.states)
        np.testing.assert_array_equal(a.controls, b.controls)
        if a.outcome == LandingOutcome.SUCCESS and abs(a.states[-1][4]) > 0.5:
            turned += 1
            assert b.outcome == LandingOutcome.CONSTRAINT_VIOLATION and not b.success
            assert b.failure_reason == f"Vertical velocity: {a.states[-1][4]:.2f} m/s"
        else:
            assert b.outcome == a.outcome
    assert turned >= 1


def test_mid_flight_reset_restarts_only_those_logs(rig):
    from gp_mpc_rocket_landing_amd import _lib
    from gp_mpc_rocket_landing_amd.fleet import REC_STATE, REC_STEPS, Fleet, initial_conditions
    x0 = initial_conditions(4, 42)
    x1 = initial_conditions(2, 142)
    fl = Fleet(rig["ctx"], rig["handle"], 4, horizon=N, dt=DT, residual_model=0, max_steps=20)
    try:
        with pytest.raises(_lib.HIPError) as e:     # no log attached
            fl.read_log()
        assert e.value.rc == -2
        with pytest.raises(_lib.HIPError) as e:     # a dispersion without its noise
            fl.attach_mc(thrust_dispersion=0.02)
        assert e.value.rc == -2
        with pytest.raises(_lib.HIPError) as e:
            fl.attach_mc(aero_dispersion=-1.0, noise=np.zeros((4, 20, 4)))
        assert e.value.rc == -2
        fl.attach_mc()
        fl.reset(x0)
        fl.step(5)
        S5, U5, n5 = fl.read_log()
        assert n5.tolist() == [5, 5, 5, 5]
        fl.reset(x1, first=2)
        S, U, n = fl.read_log()
        assert n.tolist() == [5, 5, 0, 0]
        np.testing.assert_array_equal(S[2:, 0], x1)
        assert np.all(np.isnan(S[2:, 1:])) and np.all(np.isnan(U[2:]))
        fl.step(3)
        S, U, n = fl.read_log()
        rec, _ = fl.read()
        assert n.tolist() == [8, 8, 3, 3] == rec[:, REC_STEPS].astype(int).tolist()
        np.testing.assert_array_equal(S[:2, :6], S5[:2, :6])     # the others' logs went on
        np.testing.assert_array_equal(U[:2, :5], U5[:2, :5])
        np.testing.assert_array_equal(S[:2, 0], x0[:2])
        np.testing.assert_array_equal(S[2:, 0], x1)
        for i in range(4):
            T = n[i]
            np.testing.assert_array_equal(S[i, T], rec[i, REC_STATE])
            assert np.all(np.isnan(S[i, T + 1:])) and np.all(np.isnan(U[i, T:]))
            for t in range(T):
                want = _euler(S[i, t], U[i, t], DT)
                assert np.all(np.abs(S[i, t + 1] - want) <= _euler_bound(want)), (i, t)
        # a sub-range read returns the same rows
        S12, U12, n12 = fl.read_log(first=1, count=2)
        np.testing.assert_array_equal(S12, S[1:3]); np.testing.assert_array_equal(U12, U[1:3])
        assert n12.tolist() == [8, 3]
        fl.detach_mc()
        with pytest.raises(_lib.HIPError):
            fl.read_log()
    finally:
        fl.close()
    # the restarted landings flew what a fresh fleet flies from the same states
    fresh = Fleet(rig["ctx"], rig["handle"], 2, fleet_batch=4, horizon=N, dt=DT, residual_model=0, max_steps=20)
    try:
        fresh.reset(x1)
        fresh.step(3)
        r2, _ = fresh.read()
    finally:
        fresh.close()
    np.testing.assert_array_equal(r2[:, REC_STATE], rec[2:, REC_STATE])

