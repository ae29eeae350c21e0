"""Every gate of tube_mpc's device dispatch and what each call hands to the library, without a
device call: the ``_lib`` entry points are replaced by recorders."""
import numpy as np
import pytest

import tube_cases as tc
from gp_mpc_rocket_landing_amd import _lib
from gp_mpc_rocket_landing_amd.dynamics.rocket_6dof import Rocket6DoFDynamics
from gp_mpc_rocket_landing_amd.gp.exact_gp import MultiOutputExactGP
from gp_mpc_rocket_landing_amd.gp.structured_gp import StructuredRocketGP
from gp_mpc_rocket_landing_amd.safety import RobustTubeMPC, TubeMPCConfig, TubePropagator
from gp_mpc_rocket_landing_amd.safety.safety_filter import rocket_vector

N = 3
X = np.stack([tc.nominal("hover")[0][:N + 1], tc.nominal("tilted")[0][:N + 1]])
U = np.stack([tc.nominal("hover")[1][:N], tc.nominal("tilted")[1][:N]])


@pytest.fixture
def calls(monkeypatch):
    """The library calls, recorded: tube_linear answers with tubes of ones, tube_mc of twos."""
    monkeypatch.delenv("GPMPC_TUBE", raising=False)
    log = []

    def tube_linear(ctx, rocket, X_nom, U_nom, dt, eps=1e-6, w=None, w_max=0.1, K=None, return_AB=False):
        log.append(("linear", dict(ctx=ctx, rocket=rocket, X=X_nom, U=U_nom, dt=dt, eps=eps, w=w, w_max=w_max, K=K,
                                   AB=return_AB)))
        B, n = U_nom.shape[:2]
        tubes = np.ones((B, n + 1, 14))
        return (tubes, np.full((B, n, 14, 14), 3.0), np.full((B, n, 14, 3), 4.0)) if return_AB else tubes

    def tube_mc(ctx, rocket, X_nom, U_nom, noise, dt, quantile=0.95):
        log.append(("mc", dict(ctx=ctx, rocket=rocket, X=X_nom, U=U_nom, noise=noise, dt=dt, quantile=quantile)))
        return np.full((len(U_nom), U_nom.shape[1] + 1, 14), 2.0)

    monkeypatch.setattr(_lib, "tube_linear", tube_linear)
    monkeypatch.setattr(_lib, "tube_mc", tube_mc)
    monkeypatch.setattr(_lib, "default_context", lambda: "default context")
    return log


def test_the_standard_plant_takes_the_device(calls):
    p = TubePropagator(Rocket6DoFDynamics())
    got = p.propagate_linear_batch(X, U, tc.W_VEC, tc.K_DENSE)
    assert (p.last_path, p.last_reason) == ("device", "Rocket6DoFDynamics") and np.all(got == 1.0)
    (kind, c), = calls
    assert kind == "linear" and c["ctx"] == "default context" and np.array_equal(c["rocket"], rocket_vector(p.dynamics))
    assert np.array_equal(c["X"], X) and np.array_equal(c["U"], U) and (c["dt"], c["AB"]) == (0.1, False)
    assert np.array_equal(c["w"], tc.W_VEC) and np.array_equal(c["K"], tc.K_DENSE)
    # w_bounds None is the reference's np.ones(14) * w_max; the single call is the batch of one
    p.ctx = "mine"
    assert p.propagate_linear(X[1], U[1]).shape == (N + 1, 14)
    c = calls[-1][1]
    assert c["ctx"] == "mine" and np.array_equal(c["w"], np.ones(14) * 0.1) and c["K"] is None and c["X"].shape == (1, N + 1, 14)
    p.propagate_linear_batch(X, U, np.zeros((2, N, 14)))
    assert calls[-1][1]["w"].shape == (2, N, 14)
    for name in ("inertia",):
        assert TubePropagator(tc.make_dynamics(name))._device_gate()[0]


def test_linearize_goes_through_the_linear_entry_point(calls):
    p = TubePropagator(Rocket6DoFDynamics(), TubeMPCConfig(dt=0.05))
    A, B = p.linearize_batch(X[:, 0], U[:, 0], eps=1e-3)
    assert p.last_path == "device" and A.shape == (2, 14, 14) and B.shape == (2, 14, 3) and np.all(A == 3.0) and np.all(B == 4.0)
    c = calls[-1][1]
    assert (c["dt"], c["eps"], c["AB"]) == (0.05, 1e-3, True) and np.array_equal(c["X"][:, 0], X[:, 0]) and c["U"].shape == (2, 1, 3)
    A, B = p._linearize(X[0, 0], U[0, 0])
    assert A.shape == (14, 14) and calls[-1][1]["eps"] == 1e-6


def test_env_override_forces_the_host_and_rejects_other_values(calls, monkeypatch):
    p = TubePropagator(Rocket6DoFDynamics())
    monkeypatch.setenv("GPMPC_TUBE", "host")
    assert p._device_gate() == (False, "GPMPC_TUBE=host")
    got = p.propagate_linear_batch(X, U)
    assert (p.last_path, p.last_reason) == ("host", "GPMPC_TUBE=host") and not calls and not np.all(got == 1.0)
    monkeypatch.setenv("GPMPC_TUBE", "device")
    assert p._device_gate()[0]
    monkeypatch.setenv("GPMPC_TUBE", "gpu")
    with pytest.raises(ValueError, match="GPMPC_TUBE"):
        p.propagate_linear_batch(X, U)


def test_foreign_plants_run_on_the_host_and_say_why(calls):
    class Sub(Rocket6DoFDynamics):
        pass

    p = TubePropagator(Sub())
    got = p.propagate_linear_batch(X, U)
    assert (p.last_path, p.last_reason) == ("host", "the dynamics is not Rocket6DoFDynamics") and not calls
    assert np.array_equal(got[0], TubePropagator(Rocket6DoFDynamics())._linear_host(X[0], U[0], np.ones(14) * 0.1, None))
    p = TubePropagator(Rocket6DoFDynamics())
    p.dynamics._params.J_B = np.zeros((3, 3))
    assert p._device_gate() == (False, "the rocket is not one the device model runs")
    mpc = RobustTubeMPC(Sub())
    mpc.compute_tubes(X[0], U[0])
    assert (mpc.last_path, mpc.last_reason) == ("host", "the dynamics is not Rocket6DoFDynamics")


@pytest.mark.parametrize("dt", [0.0, -0.1, np.inf, np.nan])
def test_a_bad_dt_stays_on_the_host(calls, dt):
    ok, why = TubePropagator(Rocket6DoFDynamics(), TubeMPCConfig(dt=dt))._device_gate()
    assert not ok and why.startswith("dt = ")


@pytest.mark.parametrize("eps", [0.0, np.inf, np.nan])
def test_a_bad_eps_stays_on_the_host(calls, eps):
    p = TubePropagator(Rocket6DoFDynamics())
    ok, why = p._device_gate(eps=eps)
    assert not ok and why.startswith("eps = ")
    with np.errstate(all="ignore"):
        p.linearize_batch(X[:1, 0], U[:1, 0], eps=eps)
    assert p.last_path == "host" and not calls


def test_monte_carlo_gates_and_draws(calls):
    p = TubePropagator(Rocket6DoFDynamics(), TubeMPCConfig(w_max=0.2))
    k_tile, cap = _lib.tube_plan()
    assert cap == tc.MC_CAP
    np.random.seed(5)
    got = p.propagate_monte_carlo_batch(X, U, None, n_samples=4, quantile=0.5)
    assert p.last_path == "device" and np.all(got == 2.0)
    c = calls[-1][1]
    np.random.seed(5)
    want = np.array([[[np.random.randn(14) * 0.2 for _ in range(4)] for _ in range(N)] for _ in range(2)])
    assert np.array_equal(c["noise"], want) and (c["quantile"], c["dt"]) == (0.5, 0.1)
    # n_samples at the cap goes, one more does not (no run: the gate alone)
    assert p._device_gate(n_samples=cap) == (True, "Rocket6DoFDynamics")
    assert p._device_gate(n_samples=cap + 1) == (False, f"n_samples = {cap + 1} is outside 1..{cap}")
    assert not p._device_gate(n_samples=0)[0]

    class Sampler:
        def sample(self, x, u):
            return np.zeros(6)

    n_calls = len(calls)
    p.propagate_monte_carlo_batch(X[:, :2], U[:, :1], Sampler(), n_samples=2)
    assert (p.last_path, p.last_reason) == ("host", "gp_model.sample draws on the host") and len(calls) == n_calls
    with pytest.raises(ValueError):
        p.propagate_monte_carlo_batch(X[:, :2], U[:, :1], None, n_samples=2, quantile=-0.1)
    assert p.last_path == "host" and "quantile" in p.last_reason and len(calls) == n_calls


def test_package_gps_take_one_batched_call(calls, monkeypatch):
    seen = []

    def predict(self, Xq):
        seen.append(np.array(Xq))
        return np.zeros((len(Xq), 6)), np.full((len(Xq), 6), 0.25)

    monkeypatch.setattr(MultiOutputExactGP, "predict", predict)
    monkeypatch.setattr(MultiOutputExactGP, "device_handle", property(lambda self: object()))
    p = TubePropagator(Rocket6DoFDynamics())
    gp = MultiOutputExactGP(14, 6)
    tubes, gp_vars = p.propagate_with_gp_batch(X, U, gp, n_sigma=3.0)
    assert p.last_path == "device" and len(seen) == 1 and np.array_equal(seen[0], X[:, :N].reshape(2 * N, 14))
    assert gp_vars.shape == (2, N, 6) and np.all(gp_vars == 0.25)
    c = calls[-1][1]
    w = np.zeros((2, N, 14))
    w[..., 4:7] = w[..., 11:14] = 0.5 * 3.0
    assert np.array_equal(c["w"], w) and c["K"] is None
    # the single-trajectory surface too
    seen.clear()
    p.propagate_with_gp(X[0], U[0], gp)
    assert len(seen) == 1 and seen[0].shape == (N, 14)
    # another input dimension, or no shared handle: row by row, as the reference asks
    seen.clear()
    p.propagate_with_gp_batch(X, U, MultiOutputExactGP(13, 6))
    assert [s.shape for s in seen] == [(1, 14)] * (2 * N)
    seen.clear()
    monkeypatch.setattr(MultiOutputExactGP, "device_handle", property(lambda self: None))
    p.propagate_with_gp_batch(X, U, gp)
    assert len(seen) == 2 * N
    # and on the host path
    seen.clear()
    monkeypatch.setattr(MultiOutputExactGP, "device_handle", property(lambda self: object()))
    monkeypatch.setenv("GPMPC_TUBE", "host")
    p.propagate_with_gp_batch(X[:1, :2], U[:1, :1], gp)
    assert p.last_path == "host" and [s.shape for s in seen] == [(1, 14)]


def test_a_structured_gp_is_read_through_predict_batch(calls, monkeypatch):
    seen = []

    def predict_batch(self, Xq, Uq):
        seen.append((np.array(Xq), np.array(Uq)))
        z = np.zeros((len(Xq), 3))
        return z, z, z + 0.01, z + 0.04

    monkeypatch.setattr(StructuredRocketGP, "predict_batch", predict_batch)
    p = TubePropagator(Rocket6DoFDynamics())
    gp = StructuredRocketGP()
    _, gp_vars = p.propagate_with_gp_batch(X, U, gp)
    assert len(seen) == 1 and seen[0][0].shape == (2 * N, 14) and np.array_equal(seen[0][1], U.reshape(2 * N, 3))
    assert np.array_equal(gp_vars[1, 2], [0.01] * 3 + [0.04] * 3)
    w = calls[-1][1]["w"]
    assert np.array_equal(w[0, 0, 4:7], np.sqrt(np.full(3, 0.01)) * 2.0)
    assert np.array_equal(w[0, 0, 11:14], np.sqrt(np.full(3, 0.04)) * 2.0)
    with pytest.raises(TypeError):      # the reference's single-trajectory call: predict(X) alone
        p.propagate_with_gp(X[0], U[0], gp)
    mpc = RobustTubeMPC(Rocket6DoFDynamics())
    mpc.set_gp_model(gp)
    assert np.all(mpc.compute_tubes_batch(X, U) == 1.0) and mpc.last_path == "device"


def test_a_stub_takes_single_row_calls_in_the_references_order(calls):
    p = TubePropagator(Rocket6DoFDynamics())
    stub = tc.StubUncertainty()
    tubes, gp_vars = p.propagate_with_gp_batch(X, U, stub)
    assert p.last_path == "device" and len(stub.calls) == 2 * N
    order = [(b, k) for b in range(2) for k in range(N)]
    for (b, k), (cx, cu) in zip(order, stub.calls):
        assert np.array_equal(cx, X[b, k:k + 1]) and np.array_equal(cu, U[b, k:k + 1])
    assert np.array_equal(gp_vars[1, 0], tc._smooth(X[1, :1], U[1, :1], 6)[0])
    tubes, gp_vars = p.propagate_with_gp_batch(X, U, tc.StubNothing())
    assert np.all(gp_vars == 0.1 ** 2) and gp_vars.shape == (2, N, 6)


def test_empty_calls_make_no_device_call(calls):
    p = TubePropagator(Rocket6DoFDynamics())
    assert p.propagate_linear_batch(np.zeros((0, 3, 14)), np.zeros((0, 2, 3))).shape == (0, 3, 14)
    assert np.array_equal(p.propagate_linear_batch(X[:, :1], U[:, :0]), np.zeros((2, 1, 14)))
    assert np.array_equal(p.propagate_monte_carlo_batch(X[:, :1], U[:, :0], None, 5), np.zeros((2, 1, 14)))
    assert p.linearize_batch(np.zeros((0, 14)), np.zeros((0, 3)))[0].shape == (0, 14, 14)
    assert not calls and p.last_path == "host"
