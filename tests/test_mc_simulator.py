"""MonteCarloSimulator / MonteCarloResults (reference src/experiments/monte_carlo.py) without
a GPU: the loop path against a fixture the reference's own simulator wrote
(tests/golden/gen_mc_sim_golden.py, plant and controller of tests/golden/mc_toy.py), the
device noise table against the draws that run consumed, and the dispatch gate."""
import contextlib
import io
import json

import numpy as np
import pytest

from conftest import golden
from mc_toy import MAX_TIME, VEL_TOL_Z, FeedbackLander, ToyPlant3, fixture_cases, without_compute

from gp_mpc_rocket_landing_amd.experiments import (LandingConstraints, LandingOutcome, MonteCarloResults,
                                                   MonteCarloSimulator, SimulationConfig, SimulationResult,
                                                   compare_controllers, mc_noise_table)

CASES = list(fixture_cases())


def _config(**over):
    c = SimulationConfig.run_experiments()
    c.max_time = MAX_TIME
    c.landing_constraints = LandingConstraints(pos_tol_xy=5.0, vel_tol_z=VEL_TOL_Z)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _run(name):
    over, run_kw = fixture_cases()[name]
    sim = MonteCarloSimulator(ToyPlant3(), FeedbackLander(), _config(**over))
    with contextlib.redirect_stdout(io.StringIO()):
        res = sim.run(**run_kw)
    assert sim.last_path == "loop"   # a plain controller never reaches the fleet
    return res


@pytest.fixture(scope="module")
def gold():
    return golden("mc_sim_golden.npz")


def test_fixture_covers_the_outcomes(gold):
    seen = set()
    for name in CASES:
        seen |= set(gold[f"{name}_outcomes"].tolist())
    assert {LandingOutcome.SUCCESS.value, LandingOutcome.TIMEOUT.value} <= seen
    assert seen & {LandingOutcome.CRASH.value, LandingOutcome.CONSTRAINT_VIOLATION.value}


@pytest.mark.parametrize("name", CASES)
def test_loop_path_reproduces_the_reference(gold, name):
    """Arrays and statistics bit-equal, summary() line for line above "Compute Time"."""
    res = _run(name)
    T = gold[f"{name}_nsteps"]
    assert res.n_runs == len(T)
    for i, r in enumerate(res.results):
        assert isinstance(r, SimulationResult) and r.run_id == i
        assert len(r.controls) == T[i] and r.states.shape == (T[i] + 1, 7) and r.times.shape == (T[i] + 1,)
        np.testing.assert_array_equal(r.states, gold[f"{name}_states"][i, :T[i] + 1])
        np.testing.assert_array_equal(r.controls, gold[f"{name}_controls"][i, :T[i]])
        np.testing.assert_array_equal(r.initial_state, gold[f"{name}_states"][i, 0])
        assert r.outcome.value == gold[f"{name}_outcomes"][i]
        assert r.success == (r.outcome == LandingOutcome.SUCCESS)
        assert r.failure_reason[:24] == str(gold[f"{name}_reasons"][i])
        assert r.flight_time == gold[f"{name}_flight_time"][i]
    want = json.loads(str(gold[f"{name}_stats"]))
    have = json.loads(json.dumps(without_compute(res.get_statistics())))
    assert have == want and list(have) == list(want)
    assert res.summary().split("Compute Time:")[0].split("\n") == str(gold[f"{name}_summary"]).split("\n")
    assert res.summary().endswith("=" * 60)


def test_results_container(tmp_path):
    res = _run("nominal")
    assert res.n_success == sum(r.success for r in res.results) and res.success_rate == res.n_success / res.n_runs
    assert res.get_statistics() is res.get_statistics()   # cached
    lo, hi = res._binomial_ci(res.n_success, res.n_runs)
    assert 0.0 <= lo <= res.success_rate <= hi <= 1.0 and res._binomial_ci(0, 0) == (0.0, 0.0)
    p = tmp_path / "mc.pkl"
    res.save(str(p))
    back = MonteCarloResults.load(str(p))
    assert back.summary().split("Compute Time:")[0] == res.summary().split("Compute Time:")[0]
    none = MonteCarloResults(config=res.config, results=[r for r in res.results if not r.success])
    st = none.get_statistics()
    assert st["n_success"] == 0 and st["success_rate_ci"] == (0.0, 0.0) and "fuel_mean" not in st
    assert "Performance Metrics" not in none.summary()


def test_compare_controllers_shares_initial_conditions():
    with contextlib.redirect_stdout(io.StringIO()):
        out = compare_controllers(ToyPlant3(), {"a": FeedbackLander(), "b": FeedbackLander(k_rate=0.3)},
                                  n_runs=3, config=_config(), seed=5)
    assert set(out) == {"a", "b"}
    for ra, rb in zip(out["a"].results, out["b"].results):
        np.testing.assert_array_equal(ra.initial_state, rb.initial_state)
    np.random.seed(5)
    sim = MonteCarloSimulator(ToyPlant3(), None, _config())
    np.testing.assert_array_equal(out["a"].results[0].initial_state, sim.sample_initial_condition())


def test_noise_table_is_what_the_reference_drew(gold):
    """Row i of the table against the dispersion terms the reference's run applied:
    x_next - step(x, u) on the velocity rows = n0 sigma_T u[0] / m dt + n[1:4] sigma_A dt.
    1e-12 relative to max(|x_next|, 1): the difference of two O(1..10) doubles carries a
    few 1e-16 |x| of rounding, the term itself is formed from four products."""
    over, run_kw = fixture_cases()["dispersed"]
    cfg = _config(**over)
    max_steps = int(cfg.max_time / cfg.dt)
    table = mc_noise_table(run_kw["seed"], run_kw["n_runs"], cfg)
    assert table.shape == (run_kw["n_runs"], max_steps, 4)
    S, U, T = gold["dispersed_states"], gold["dispersed_controls"], gold["dispersed_nsteps"]
    plant = ToyPlant3()
    for i in range(run_kw["n_runs"]):
        for t in range(T[i]):
            x, u = S[i, t], U[i, t]
            got = S[i, t + 1] - plant.step(x, u, cfg.dt)
            n = table[i, t]
            want = n[0] * cfg.thrust_dispersion * u[0] / x[0] * cfg.dt + n[1:4] * cfg.aero_dispersion * cfg.dt
            assert np.all(got[:4] == 0.0)
            assert np.all(np.abs(got[4:7] - want) <= 1e-12 * np.maximum(np.abs(S[i, t + 1, 4:7]), 1.0)), (i, t)
    # the columns a configuration does not draw stay 0, and the stream shifts accordingly
    only_aero = mc_noise_table(42, 2, _config(aero_dispersion=1.0), 5)
    assert np.all(only_aero[:, :, 0] == 0.0) and np.all(only_aero[:, :, 1:] != 0.0)
    rs = np.random.RandomState(43); rs.randn(7)
    np.testing.assert_array_equal(only_aero[1, 0, 1:], rs.randn(3))
    only_thrust = mc_noise_table(42, 2, _config(thrust_dispersion=0.02), 5)
    assert np.all(only_thrust[:, :, 1:] == 0.0)
    rs = np.random.RandomState(42); rs.randn(7)
    np.testing.assert_array_equal(only_thrust[0, :, 0], [rs.randn() for _ in range(5)])
    assert np.all(mc_noise_table(42, 2, _config(), 5) == 0.0)


# ---- the dispatch gate ---------------------------------------------------------------
def _gate_fixture(monkeypatch):
    """A simulator that passes every gate condition, built without a device: the
    controller's context is a placeholder and the GP's device handle a bare object."""
    from gp_mpc_rocket_landing_amd import _lib, fleet
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import GPMPC, GPMPCConfig

    class Reached(Exception):
        pass

    def refuse(self, *a, **k):
        raise Reached("the fleet constructor was reached")
    monkeypatch.setattr(fleet.Fleet, "__init__", refuse)
    gp = Simple3DoFGP(use_sparse=False)
    gp._is_fitted = True
    handle = object.__new__(_lib.ExactGPHandle)
    handle.ctx = object()

    class Inner:
        device_handle = handle
    gp.gp = Inner()
    dyn = create_normalized_rocket()
    ctl = GPMPC(dyn, gp, GPMPCConfig(N=20, dt=0.1), ctx=object())
    sim = MonteCarloSimulator(dyn, ctl, SimulationConfig.run_experiments())
    return sim, Reached


def test_gate_passes_the_reference_setup(monkeypatch):
    sim, Reached = _gate_fixture(monkeypatch)
    kw, handle = sim._fleet_plan(1)
    assert kw == dict(horizon=20, dt=0.1, target_mode=1, use_gp=1, residual_model=0, max_steps=300, sqp_iters=1,
                      sqp_tol=1e-4, max_iter=50, eps_abs=1e-4, eps_rel=1e-4)
    assert handle is sim.controller.gp.gp.device_handle
    with pytest.raises(Reached):
        sim.run(n_runs=1)
    with pytest.raises(Reached), contextlib.redirect_stdout(io.StringIO()):
        sim.run(n_runs=1, n_workers=2)           # no dispersions: still the fleet
    sim.run(n_runs=0)
    assert sim.last_path == "fleet"


def _flips():
    from gp_mpc_rocket_landing_amd.dynamics import Rocket3DoFConfig, Rocket3DoFDynamics
    from gp_mpc_rocket_landing_amd.gp.features import AtmosphereModel, Simple3DoFFeatureExtractor
    from gp_mpc_rocket_landing_amd.mpc import GPMPC, ConstraintParams, CostWeights, qp_builder

    class SubGPMPC(GPMPC):
        pass

    class SubDyn(Rocket3DoFDynamics):
        pass

    class SubFeat(Simple3DoFFeatureExtractor):
        pass

    def setc(**kw):
        return lambda s, mp: [setattr(s.controller.config, k, v) for k, v in kw.items()]

    def setfe(**kw):
        return lambda s, mp: [setattr(s.controller.gp.feature_extractor, k, v) for k, v in kw.items()]

    return {
        "controller subclass": lambda s, mp: setattr(s.controller, "__class__", SubGPMPC),
        "other controller": lambda s, mp: setattr(s, "controller", FeedbackLander()),
        "safety filter": lambda s, mp: setattr(s, "safety_filter", object()),
        "plant subclass": lambda s, mp: setattr(s.dynamics, "__class__", SubDyn),
        "plant I_sp": lambda s, mp: setattr(s, "dynamics", Rocket3DoFDynamics(Rocket3DoFConfig(I_sp=25.0))),
        "plant gravity": lambda s, mp: setattr(s, "dynamics", Rocket3DoFDynamics(
            Rocket3DoFConfig(g_I=np.array([-1.2, 0.0, 0.0])))),
        "controller model alpha": lambda s, mp: setattr(s.controller._qp, "alpha", 0.04),
        "controller model gravity": lambda s, mp: setattr(s.controller._qp, "g_vec", np.array([-1.2, 0.0, 0.0])),
        "dense pattern": lambda s, mp: setattr(s.controller._qp, "dense", True),
        "hover guess g0": lambda s, mp: setattr(s.controller, "_g0", 1.1),
        "dt mismatch": lambda s, mp: setattr(s.config, "dt", 0.05),
        "integration method": setc(integration_method="rk4"),
        "cost weights": lambda s, mp: setattr(s.controller, "cost_weights", CostWeights(w_position=20.0)),
        "constraint params": lambda s, mp: setattr(s.controller, "constraint_params", ConstraintParams(T_max=6.0)),
        "Q": lambda s, mp: mp.setattr(qp_builder, "Q_DIAG", qp_builder.Q_DIAG * 2),
        "R": lambda s, mp: mp.setattr(qp_builder, "R_DIAG", qp_builder.R_DIAG * 2),
        "terminal scale": lambda s, mp: mp.setattr(qp_builder, "QF_SCALE", 5.0),
        "state box": lambda s, mp: mp.setattr(qp_builder, "X_MAX", qp_builder.X_MAX * 2),
        "thrust box": lambda s, mp: mp.setattr(qp_builder, "U_MIN", np.array([0.5, -5.0, -5.0])),
        "ADMM setting": lambda s, mp: setattr(s.controller._ws.settings, "alpha", 1.5),
        "ADMM max_iter": lambda s, mp: setattr(s.controller._ws.settings, "max_iter", 60),
        "GP missing": lambda s, mp: setattr(s.controller, "gp", None),
        "GP unfitted": lambda s, mp: setattr(s.controller.gp, "_is_fitted", False),
        "GP without device handle": lambda s, mp: setattr(s.controller.gp.gp, "device_handle", None),
        "feature subclass": lambda s, mp: setattr(s.controller.gp.feature_extractor, "__class__", SubFeat),
        "feature v_ref": setfe(v_ref=20.0),
        "feature altitude": setfe(include_altitude=False),
        "feature density": setfe(include_density=False),
        "atmosphere": setfe(atmosphere=AtmosphereModel(rho_0=1.0)),
        "no step fits": lambda s, mp: setattr(s.config, "max_time", 0.05),
    }


@pytest.mark.parametrize("flip", list(_flips()))
def test_gate_conditions_flipped_one_at_a_time(monkeypatch, flip):
    """Each condition alone sends run to the loop; the (patched) fleet constructor is never
    reached.  n_runs = 0: the loop path itself then flies nothing."""
    sim, _ = _gate_fixture(monkeypatch)
    _flips()[flip](sim, monkeypatch)
    plan, why = sim._fleet_plan(1)
    assert plan is None and isinstance(why, str) and why
    sim.run(n_runs=0)
    assert sim.last_path == "loop" and sim.last_path_reason == why


def test_gate_dispersions_with_workers_and_override(monkeypatch):
    sim, Reached = _gate_fixture(monkeypatch)
    sim.config.thrust_dispersion = 0.02
    assert sim._fleet_plan(1)[0] is not None     # n_workers = 1: the noise table
    assert sim._fleet_plan(2)[0] is None         # one serial stream: the loop
    with contextlib.redirect_stdout(io.StringIO()):
        sim.run(n_runs=0, n_workers=2)
    assert sim.last_path == "loop"
    sim.config.thrust_dispersion = 0.0
    sim.run(n_runs=0, use_fleet=False)
    assert sim.last_path == "loop" and sim.last_path_reason == "use_fleet=False"


def test_only_refused_arguments_fall_back(monkeypatch):
    """HIPError.rc == -2 from the fleet goes to the loop; any other error is the caller's."""
    from gp_mpc_rocket_landing_amd import _lib, fleet
    sim, _ = _gate_fixture(monkeypatch)

    def refused(self, *a, **k):
        raise _lib.HIPError("fleet_create failed (-2): refused", -2)

    def broken(self, *a, **k):
        raise _lib.HIPError("fleet_create failed (-1): out of device memory", -1)
    monkeypatch.setattr(fleet.Fleet, "__init__", refused)
    monkeypatch.setattr(MonteCarloSimulator, "run_single", lambda self, i, x0=None, seed=None: "flown")
    res = sim.run(n_runs=2)
    assert sim.last_path == "loop" and res.results == ["flown", "flown"] and "refused" in sim.last_path_reason
    monkeypatch.setattr(fleet.Fleet, "__init__", broken)
    with pytest.raises(_lib.HIPError):
        sim.run(n_runs=2)


def test_run_single_starts_a_resettable_controller_cold():
    """DESIGN D15: a controller with reset_warm_start is reset before every landing."""
    class Counting(FeedbackLander):
        resets = 0

        def reset_warm_start(self):
            Counting.resets += 1
    sim = MonteCarloSimulator(ToyPlant3(), Counting(), _config())
    sim.run(n_runs=3)
    assert Counting.resets == 3 and sim.last_path == "loop"


def test_run_with_dispersions_levels():
    sim = MonteCarloSimulator(ToyPlant3(), FeedbackLander(), _config())
    with contextlib.redirect_stdout(io.StringIO()):
        out = sim.run_with_dispersions(n_runs=2, dispersion_configs=[
            {"name": "a", "thrust_dispersion": 0.0, "aero_dispersion": 0.0},
            {"name": "b", "thrust_dispersion": 0.02, "aero_dispersion": 1.0}])
    assert list(out) == ["a", "b"] and all(r.n_runs == 2 for r in out.values())
    assert sim.config.aero_dispersion == 1.0
    assert not np.array_equal(out["a"].results[0].states[:5], out["b"].results[0].states[:5])
