"""The safety package's host path against the reference's recorded results
(tests/golden/safety.npz, gen_safety_golden.py): equal bits for every field of every case,
since the host path is the reference's arithmetic over the same plant.  No GPU."""
import numpy as np
import pytest
from conftest import golden

import safety_cases as sc
from gp_mpc_rocket_landing_amd import safety
from gp_mpc_rocket_landing_amd.dynamics.rocket_6dof import Rocket6DoFDynamics
from gp_mpc_rocket_landing_amd.mpc.constraints import ConstraintParams

FIELDS = (("u_safe", "u_safe"), ("is_modified", "is_modified"), ("is_safe", "is_safe"), ("margin", "safety_margin"),
          ("value", "backup_value"), ("mask", "violation_mask"), ("iters", "iterations"))


@pytest.fixture(scope="module")
def g():
    return golden("safety.npz")


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    monkeypatch.setenv("GPMPC_SAFETY", "host")


@pytest.fixture(scope="module")
def batches(g):
    """filter_batch over every configuration's cases, computed once."""
    import os
    old = os.environ.get("GPMPC_SAFETY")
    os.environ["GPMPC_SAFETY"] = "host"
    try:
        out = {}
        for name in sc.CONFIGS:
            f = sc.make_filter(sc.load_spec(g, name), safety)
            out[name] = (f, f.filter_batch(g[f"{name}_X"], g[f"{name}_U"]))
            assert f.last_path == "host" and f.last_reason == "GPMPC_SAFETY=host"
        return out
    finally:
        if old is None:
            del os.environ["GPMPC_SAFETY"]
        else:
            os.environ["GPMPC_SAFETY"] = old


def test_fixture_specs_are_the_shared_ones(g):
    for name in sc.CONFIGS:
        sp, ld = sc.spec(name), sc.load_spec(g, name)
        for k in sc.SPEC_KEYS:
            assert np.array_equal(sp[k], ld[k]), (name, k)


def test_fixture_coverage_and_gaps(g):
    for k in ("safe", "modified_0", "early_exit_safe", "full_unsafe", "low", "high", "tilt", "glideslope",
              "path_k_ge_1", "low_altitude", "saturation", "project_low", "project_high"):
        assert int(g[f"coverage_{k}"]) > 0, k
    assert len(g["coverage_early_exit_counts"]) >= 3
    assert float(g["decision_gap_v"]) >= 1000 * float(g["spread_value"])
    assert float(g["decision_gap_margin"]) >= 1000 * float(g["spread_margin"])
    assert float(g["decision_gap_constraint"]) >= 1000 * float(g["spread_u"])
    it, mod = g["B_iters"][g["mix_idx"]], g["B_is_modified"][g["mix_idx"]]
    assert len(it) == 16 and np.any(~mod) and np.any(mod & (it > 0) & (it < 50)) and np.any(it == 50)


@pytest.mark.parametrize("name", sc.CONFIGS)
def test_filter_batch_rows_have_the_reference_bits(g, batches, name):
    _, out = batches[name]
    assert len(out) == len(g[f"{name}_X"])
    for key, attr in FIELDS:
        assert np.array_equal(getattr(out, attr), g[f"{name}_{key}"]), (name, key)
    assert np.array_equal(out.u_nominal, g[f"{name}_U"])


@pytest.mark.parametrize("name", sc.CONFIGS)
def test_filter_has_the_reference_bits(g, batches, name):
    """The single-call surface on a spread of cases (every outcome's first case and the last),
    and result(i) of the batch on all of them."""
    f, out = batches[name]
    X, U, it, mod = g[f"{name}_X"], g[f"{name}_U"], g[f"{name}_iters"], g[f"{name}_is_modified"]
    for i in range(len(X)):
        r = out.result(i)
        assert np.array_equal(r.u_safe, g[f"{name}_u_safe"][i]) and r.is_modified == bool(mod[i])
        assert r.safety_margin == g[f"{name}_margin"][i] and r.backup_value == g[f"{name}_value"][i]
        assert safety.safety_filter.violations_to_mask(r.constraint_violations) == int(g[f"{name}_mask"][i])
        assert r.constraint_violations["terminal"] == r.safety_margin
    picks = {len(X) - 1}
    for sel in (~mod, mod & (it == 0), mod & (it > 0) & (it < 50), it == 50):
        if np.any(sel):
            picks.add(int(np.where(sel)[0][0]))
    for i in sorted(picks):
        r = f.filter(X[i], U[i])
        assert f.last_path == "host"
        assert np.array_equal(r.u_safe, g[f"{name}_u_safe"][i]) and np.array_equal(r.u_nominal, U[i])
        assert (r.is_modified, r.is_safe) == (bool(mod[i]), bool(g[f"{name}_is_safe"][i]))
        assert r.safety_margin == g[f"{name}_margin"][i] and r.backup_value == g[f"{name}_value"][i]
        assert safety.safety_filter.violations_to_mask(r.constraint_violations) == int(g[f"{name}_mask"][i])
        assert f._last_iterations == int(it[i]) and r.solve_time >= 0.0


def test_filter_needs_initialize():
    f = safety.PredictiveSafetyFilter(Rocket6DoFDynamics())
    with pytest.raises(RuntimeError, match="initialize"):
        f.filter(sc.X_EQ, sc.U_EQ)
    assert f.tube_propagator is None


def test_compute_gains_falls_back_to_pd_gains(capsys):
    b = safety.LQRBackupController(Rocket6DoFDynamics(), safety.BackupControllerConfig())
    b.compute_gains(sc.X_EQ.copy())
    assert capsys.readouterr().out == "LQR computation failed: Failed to find a finite solution., using simple PD gains\n"
    K = np.zeros((3, 14))
    for i in range(3):
        K[i, 1 + i], K[i, 4 + i] = 2.0, 1.0
    assert np.array_equal(b.K, K) and np.array_equal(b.P, b.Q) and b.P is not b.Q
    assert np.array_equal(np.diag(b.Q), [0, 10, 10, 10, 5, 5, 5, 1, 2, 2, 1, .5, .5, .5])
    assert np.array_equal(b.u_eq, sc.U_EQ) and np.array_equal(np.diag(b.R), [0.1] * 3)
    # weights with Q[0, 0] > 0 fail the same way
    q = sc.Q400.copy(); q[0] = 1.0
    b = safety.LQRBackupController(Rocket6DoFDynamics(), safety.BackupControllerConfig(Q_diag=q))
    b.compute_gains(sc.X_EQ.copy(), sc.U_EQ.copy())
    assert "using simple PD gains" in capsys.readouterr().out and np.array_equal(b.P, np.diag(q))


def test_numerical_linearization_without_linearize():
    class Plant:
        def __init__(self):
            self._d = Rocket6DoFDynamics()
            self.params = self._d.params

        def step(self, x, u, dt):
            return self._d.step(x, u, dt)

    b = safety.LQRBackupController(Plant())
    b.x_eq, b.u_eq = sc.X_EQ.copy(), sc.U_EQ.copy()
    A, B = b._linearize_at_equilibrium()
    Ad, Bd = Rocket6DoFDynamics().linearize(sc.X_EQ, sc.U_EQ, 0.1)
    assert A.shape == (14, 14) and B.shape == (14, 3)
    assert np.allclose(B[4:7], Bd[4:7], atol=1e-3) and np.allclose(A[1:4, 4:7], Ad[1:4, 4:7], atol=1e-3)


def test_backup_controller_and_invariant_set_values(g):
    f = sc.make_filter(sc.load_spec(g, "D"), safety)
    X = g["D_X"][-8:]
    U = f.backup.get_control_batch(X)
    assert np.array_equal(U, g["misc_get_control"])
    assert np.all(U >= g["D_u_min"]) and np.all(U <= g["D_u_max"])
    assert np.any(U == g["D_u_min"]) and np.any(U == g["D_u_max"])
    s = f.invariant_set
    assert np.array_equal([s.get_value(x) for x in X], g["misc_value"])
    assert np.array_equal([bool(s.contains(x)) for x in X], g["misc_contains"])
    assert np.array_equal([s.project(x) for x in X], g["misc_project"])
    assert np.array_equal([f.backup.get_value_function(x) for x in X], g["misc_backup_value"])
    Xs, Us = f.backup.simulate_backup(X[0], n_steps=4)
    assert np.array_equal(Xs, g["misc_simulate_backup_X"]) and np.array_equal(Us, g["misc_simulate_backup_U"])
    assert safety.EllipsoidalInvariantSet(14).get_value(X[0]) == np.inf


def test_compute_maximal_alpha_draws_in_the_reference_order(g):
    f = sc.make_filter(sc.load_spec(g, "A"), safety)
    np.random.seed(20240)
    a = f.invariant_set.compute_maximal_alpha(lambda x: f._check_constraints(x, f.backup.get_control(x)), n_samples=200)
    assert a == float(g["misc_maximal_alpha"]) == f.invariant_set.alpha
    np.random.seed(20241)
    assert np.array_equal(f.invariant_set.get_boundary_points(5), g["misc_boundary"])


def test_simulate_filtered_matches_the_recorded_closed_loop(g):
    f = sc.make_filter(sc.load_spec(g, "B"), safety)
    X, U, results = f.simulate_filtered(g["sim_X0"][0], g["sim_U_nom"][0])
    assert f.last_path == "host"
    assert np.array_equal(X, g["sim_X"][0]) and np.array_equal(U, g["sim_U"][0])
    assert [r.is_modified for r in results] == g["sim_is_modified"][0].tolist()
    assert [r.safety_margin for r in results] == g["sim_margin"][0].tolist()
    Xb, Ub, info = f.simulate_filtered_batch(g["sim_X0"], g["sim_U_nom"])
    assert np.array_equal(Xb, g["sim_X"]) and np.array_equal(Ub, g["sim_U"])
    assert np.array_equal(info.is_modified, g["sim_is_modified"]) and np.array_equal(info.is_safe, g["sim_is_safe"])
    assert np.array_equal(info.safety_margin, g["sim_margin"]) and np.array_equal(info.iterations, g["sim_iters"])


def test_simple_safety_filter_at_both_thrust_bounds():
    s = safety.SimpleSafetyFilter(None, ConstraintParams(T_min=1.0, T_max=4.0))
    u = np.array([0.3, 0.0, 0.4])
    assert np.array_equal(s.filter(None, u), u / 0.5 * 1.0) and np.array_equal(u, [0.3, 0.0, 0.4])
    u = np.array([6.0, 8.0, 0.0])
    assert np.array_equal(s.filter(None, u), u / 10.0 * 4.0)
    inside = np.array([2.0, 0.0, 0.0])
    assert np.array_equal(s.filter(None, inside), inside)
    d = safety.SimpleSafetyFilter(None)   # the defaults 0.5, 5.0; a zero control divides by 1e-6
    assert np.array_equal(d.filter(None, np.zeros(3)), np.zeros(3))
    assert np.array_equal(d.filter(None, np.array([0.0, 0.25, 0.0])), [0.0, 0.5, 0.0])
    assert np.allclose(np.linalg.norm(d.filter(None, np.array([30.0, 40.0, 0.0]))), 5.0, rtol=1e-15)


def test_backup_controller_factory():
    d = Rocket6DoFDynamics()
    assert type(safety.create_backup_controller(d, "lqr")) is safety.LQRBackupController
    pd = safety.create_backup_controller(d, "pd")
    u = pd.get_control(sc.X_EQ)
    assert np.allclose(u, [2.0, 0.0, 0.0])     # hover, inside the rocket's own thrust shell [1.5, 6.5]
    em = safety.create_backup_controller(d, "emergency")
    assert np.array_equal(em.get_control(sc.X_EQ), [2.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        safety.create_backup_controller(d, "other")
    box = safety.PolytopeInvariantSet()
    box.from_box(-np.ones(3), np.ones(3))
    assert box.contains(np.zeros(3)) and not box.contains(np.array([2.0, 0, 0]))


def test_monte_carlo_simulator_with_a_filter_keeps_the_per_landing_loop(g):
    """_fleet_plan's refusal is unchanged: a simulator with a safety filter does not take the
    device fleet (host logic only, no landing is flown)."""
    from gp_mpc_rocket_landing_amd.experiments.monte_carlo import MonteCarloSimulator
    from gp_mpc_rocket_landing_amd.mpc.gp_mpc import GPMPC
    f = sc.make_filter(sc.load_spec(g, "A"), safety)
    sim = MonteCarloSimulator.__new__(MonteCarloSimulator)
    sim.config, sim.dynamics, sim.safety_filter = None, Rocket6DoFDynamics(), f
    sim.controller = GPMPC.__new__(GPMPC)
    plan, reason = sim._fleet_plan()
    assert plan is None and reason == "a safety filter is set"
