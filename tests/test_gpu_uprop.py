"""Uncertainty propagation (uncertainty_prop.py:117-315) on the device path:
the mirror vs the reference's own output (F9), the batched covariance kernel
vs numpy, and the batched 3-DoF propagation vs the numpy restatement."""
import os
import sys

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))


def _ctx_default(gpu_ctx):
    from gp_mpc_rocket_landing_amd import _lib
    _lib._default_ctx = gpu_ctx


@pytest.mark.parametrize("method", ["linear", "unscented", "monte_carlo"])
def test_propagation_vs_f9(gpu_ctx, method):
    _ctx_default(gpu_ctx)
    from toy_dynamics import ToyRocket14
    from gp_mpc_rocket_landing_amd.gp import StructuredGPConfig, StructuredRocketGP
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    f5 = golden("f5_structured_6dof.npz"); f9 = golden("f9_uncertainty_prop.npz")
    g = StructuredRocketGP(StructuredGPConfig(use_sparse=False))
    g.add_data(f5["X"], f5["U"], f5["Dv"], f5["Dw"])
    g.fit()
    p = UncertaintyPropagator(ToyRocket14(), g, method=method, ctx=gpu_ctx)
    np.random.seed(123)                                   # as the fixture (MC draws)
    r = p.propagate(f9["x0"], f9["U"], Sigma_0=f9["S0_unscented"] if method == "unscented" else None, dt=0.1)
    if method == "unscented":
        # the reference's UT (alpha = 1e-3, uncertainty_prop.py:196-210) weights the
        # centre sigma point by lambda/(n+lambda) ~ -1e6, so 1e-13 differences in the
        # features reach the mean at ~1e-6: the numpy restatement of the same
        # arithmetic lands 5.5e-7 from the fixture (covariances 1.3e-10 of 6.9e-4)
        np.testing.assert_allclose(r.means, f9[f"{method}_means"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(r.covariances, f9[f"{method}_covs"], rtol=0, atol=1e-9)
    else:
        # GP parity is 1e-6 relative on the residual; the states carry it times dt
        np.testing.assert_allclose(r.means, f9[f"{method}_means"], rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(r.covariances, f9[f"{method}_covs"], rtol=1e-6, atol=1e-12)
    lo, hi = r.get_confidence_bounds(5)
    assert np.all(lo < r.means[5]) and np.all(hi > r.means[5])


@pytest.mark.parametrize("nx,B,N", [(7, 300, 30), (14, 64, 20), (16, 5, 3), (7, 1, 0)])
def test_cov_propagate_kernel(gpu_ctx, nx, B, N):
    from gp_mpc_rocket_landing_amd import _lib
    rs = np.random.RandomState(nx * 100 + B)
    A = np.eye(nx) + 0.1 * rs.randn(B, N, nx, nx)
    q = rs.rand(B, N, nx) * 1e-3
    S0 = None if nx != 14 else np.einsum("bij,bkj->bik", *(2 * [rs.randn(B, nx, nx) * 0.01]))
    out = _lib.cov_propagate(gpu_ctx, A, q, S0)
    S = np.broadcast_to(np.eye(nx) * 1e-6, (B, nx, nx)).copy() if S0 is None else S0.copy()
    np.testing.assert_array_equal(out[:, 0], S)
    for k in range(N):
        S = A[:, k] @ S @ A[:, k].transpose(0, 2, 1) + np.einsum("bi,ij->bij", q[:, k], np.eye(nx))
        np.testing.assert_allclose(out[:, k + 1], S, rtol=1e-12, atol=1e-18)


def test_propagate_batch_3dof_vs_oracle(gpu_ctx):
    """16 horizons of the normalised 3-DoF rocket with the exact Simple3DoFGP (F1
    data): one batched GP call per step + one covariance launch, vs the numpy
    restatement per trajectory."""
    _ctx_default(gpu_ctx)
    from oracle import uprop_oracle
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    f1 = golden("f1_exact_simple3dof.npz")
    gp = Simple3DoFGP(use_sparse=False)
    gp.add_data(f1["X"], f1["U"], f1["D"]); gp.fit()
    dyn = create_normalized_rocket()
    rs = np.random.RandomState(4)
    B, N = 16, 20
    X0 = f1["X"][:B] + 0.01 * rs.randn(B, 7)
    U = np.repeat(f1["U"][:B, None, :], N, axis=1) * (1 + 0.05 * rs.randn(B, N, 1))
    means, covs = UncertaintyPropagator(dyn, gp, ctx=gpu_ctx).propagate_batch(X0, U, None, 0.1)
    orc = uprop_oracle.simple3dof_exact_predictor(f1["X"], f1["U"], f1["D"])
    for b in range(B):
        m, c = uprop_oracle.propagate_linear(dyn, orc, X0[b], U[b], None, 0.1)
        np.testing.assert_allclose(means[b], m, rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(covs[b], c, rtol=1e-6, atol=1e-14)


def test_gpmpc_propagates_and_tightens(gpu_ctx):
    """GPMPC.solve propagates along its linearisation controls (gp_mpc.py:284-290)
    and derives the step-0 tightened parameters (gp_mpc.py:177-215, 414)."""
    _ctx_default(gpu_ctx)
    from scipy.stats import norm
    from oracle import uprop_oracle
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import GPMPC, GPMPCConfig
    f1 = golden("f1_exact_simple3dof.npz")
    gp = Simple3DoFGP(use_sparse=False)
    gp.add_data(f1["X"], f1["U"], f1["D"]); gp.fit()
    dyn = create_normalized_rocket()
    mpc = GPMPC(dyn, gp, GPMPCConfig(N=20), ctx=gpu_ctx)
    x0 = np.array([2.0, 30.0, 1.0, -1.0, -3.0, 0.2, 0.1]); xt = np.zeros(7); xt[0] = 1.5
    _, U0 = mpc._initial(x0, xt)
    sol = mpc.solve(x0, xt)
    assert sol.success
    orc = uprop_oracle.simple3dof_exact_predictor(f1["X"], f1["U"], f1["D"])
    m, c = uprop_oracle.propagate_linear(dyn, orc, x0, U0, None, 0.1)
    np.testing.assert_allclose(mpc.last_uncertainty.means, m, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(mpc.last_uncertainty.covariances, c, rtol=1e-6, atol=1e-14)
    np.testing.assert_allclose(mpc.get_uncertainty_at_horizon(20), c[20], rtol=1e-6, atol=1e-14)
    kappa = norm.ppf(0.95)
    assert mpc.last_tightened_params.v_max == pytest.approx(50.0 - kappa * 1e-3, abs=1e-12)
    assert mpc.last_tightened_params.T_max == 5.0 and mpc.last_tightened_params.gamma_gs == 30.0


def test_simple_gp_predictor_rollout_vs_f9(gpu_ctx):
    """SimpleGPPredictor.simulate (gp_mpc.py:505-574) is the mean recursion of the
    reference's _propagate_linear (uncertainty_prop.py:150-160): same x_nom + d dt on
    v-dot / omega-dot, so F9's linear means pin it (gp_mpc.py itself needs CasADi)."""
    _ctx_default(gpu_ctx)
    from toy_dynamics import ToyRocket14
    from gp_mpc_rocket_landing_amd.gp import StructuredGPConfig, StructuredRocketGP
    from gp_mpc_rocket_landing_amd.mpc import SimpleGPPredictor
    f5 = golden("f5_structured_6dof.npz"); f9 = golden("f9_uncertainty_prop.npz")
    g = StructuredRocketGP(StructuredGPConfig(use_sparse=False))
    g.add_data(f5["X"], f5["U"], f5["Dv"], f5["Dw"]); g.fit()
    X, Dm, Dv = SimpleGPPredictor(ToyRocket14(), g).simulate(f9["x0"], f9["U"], 0.1)
    np.testing.assert_allclose(X, f9["linear_means"], rtol=1e-7, atol=1e-9)
    assert Dm.shape == (10, 14) and np.all(Dv[:, [0, 1, 2, 3, 7, 8, 9, 10]] == 0)
    np.testing.assert_allclose(np.diff(X, axis=0)[:, 4:7] - (np.array([ToyRocket14().step(X[k], f9["U"][k], 0.1) for k in range(10)]) - X[:-1])[:, 4:7],
                               Dm[:, 4:7] * 0.1, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("B,N,s0", [(16, 20, False), (3, 20, True), (2, 0, False), (1, 1, True)])
def test_propagate_batch_3dof_device_vs_host_loop(gpu_ctx, monkeypatch, B, N, s0):
    """gpmpc_uprop3_linear (the whole 3-DoF linear propagation in one device call) vs
    the per-step host loop over the same GP handle: the same recursion, equal up to
    the GP mean's summation order -- alpha . k over 1000 rows cancels, so 1e-15 of the
    terms reaches the residual at ~1e-12 absolute, carried through N steps."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd import _lib
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    f1 = golden("f1_exact_simple3dof.npz")
    gp = Simple3DoFGP(use_sparse=False)
    gp.add_data(f1["X"], f1["U"], f1["D"]); gp.fit()
    dyn = create_normalized_rocket()
    rs = np.random.RandomState(B * 10 + N)
    X0 = f1["X"][:B] + 0.01 * rs.randn(B, 7)
    U = np.repeat(f1["U"][:B, None, :], N, axis=1) * (1 + 0.05 * rs.randn(B, N, 1))
    S0 = None
    if s0:
        L = rs.randn(B, 7, 7) * 1e-3
        S0 = np.einsum("bij,bkj->bik", L, L)
    calls = []
    real = _lib.uprop3_linear
    monkeypatch.setattr(_lib, "uprop3_linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    p = UncertaintyPropagator(dyn, gp, ctx=gpu_ctx)
    md, cd = p.propagate_batch(X0, U, S0, 0.1)
    assert calls, "the device path was not taken"
    p.use_device = False
    mh, ch = p.propagate_batch(X0, U, S0, 0.1)
    assert len(calls) == 1
    assert md.shape == (B, N + 1, 7) and cd.shape == (B, N + 1, 7, 7)
    np.testing.assert_array_equal(md[:, 0], X0)
    np.testing.assert_allclose(md, mh, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(cd, ch, rtol=1e-7, atol=1e-15)


def test_propagate_3dof_sparse_gp_stays_on_host_loop(gpu_ctx, monkeypatch):
    """A FITC Simple3DoFGP has no exact device handle: the host loop runs."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd import _lib
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    f1 = golden("f1_exact_simple3dof.npz")
    gp = Simple3DoFGP(use_sparse=True)
    gp.add_data(f1["X"], f1["U"], f1["D"]); gp.fit()
    monkeypatch.setattr(_lib, "uprop3_linear", lambda *a, **k: pytest.fail("device path on a sparse GP"))
    m, c = UncertaintyPropagator(create_normalized_rocket(), gp, ctx=gpu_ctx).propagate_batch(
        f1["X"][:2], np.repeat(f1["U"][:2, None], 5, axis=1), None, 0.1)
    assert m.shape == (2, 6, 7) and np.all(np.isfinite(c))


@pytest.mark.parametrize("n", [1000, 1100])
def test_propagate_batch_3dof_device_training_sizes(gpu_ctx, n):
    """The device propagation's training rows in registers (n <= 1024) and read per
    step (n > 1024), vs the host loop."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.fleet import initial_conditions
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    X, U, D = synthetic_training_data(n, seed=1)
    gp = Simple3DoFGP(use_sparse=False)
    gp.add_data(X, U, D); gp.fit()
    X0 = initial_conditions(3)
    rs = np.random.RandomState(n)
    Uh = np.tile((-X0[:, 0:1] * np.array([-1.0, 0, 0]))[:, None, :], (1, 12, 1)) * (1 + 0.1 * rs.randn(3, 12, 1))
    p = UncertaintyPropagator(create_normalized_rocket(), gp, ctx=gpu_ctx)
    md, cd = p.propagate_batch(X0, Uh, None, 0.1)
    p.use_device = False
    mh, ch = p.propagate_batch(X0, Uh, None, 0.1)
    np.testing.assert_allclose(md, mh, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(cd, ch, rtol=1e-7, atol=1e-15)


@pytest.mark.parametrize("sparse,full_j,s0", [(True, False, False), (False, False, True), (True, True, False)])
def test_propagate_batch_6dof_device_vs_host_loop(gpu_ctx, sparse, full_j, s0):
    """gpmpc_uprop6_linear (the 14-state linear propagation in one device call) vs the
    per-step host loop over the same StructuredRocketGP device pair: FITC (the reference
    default) and exact, a diagonal and a full inertia tensor, with and without Sigma_0.
    The device features and Jacobian are restated expressions of the host's (rounding
    aside) and the GP means sum in another order, so the two agree to ~1e-12."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd import _lib
    from gp_mpc_rocket_landing_amd.dynamics import Rocket6DoFConfig, Rocket6DoFDynamics
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    from gp_mpc_rocket_landing_amd.rollouts6 import fit_structured_gp, initial_conditions_6dof
    gp = fit_structured_gp(300, 50, seed=0, use_sparse=sparse)
    rc = Rocket6DoFConfig()
    if full_j:
        J = np.array(rc.J_B, float)
        J = J + 0.05 * np.sqrt(np.outer(np.diag(J), np.diag(J))) * np.array([[0, 1, -1], [1, 0, 0.5], [-1, 0.5, 0]])
        rc = Rocket6DoFConfig(J_B=J)
    dyn = Rocket6DoFDynamics(rc)
    B, N = 3, 12
    X0 = initial_conditions_6dof(B)
    X0[:, 11:14] = np.array([0.02, -0.01, 0.03])
    rs = np.random.RandomState(7)
    U = np.zeros((B, N, 3))
    U[:, :, 2] = 0.9 * X0[:, 0:1] * rc.g0
    U[:, :, :2] = 0.05 * rs.randn(B, N, 2)
    S0 = None
    if s0:
        L = rs.randn(B, 14, 14) * 1e-3
        S0 = np.einsum("bij,bkj->bik", L, L)
    calls = []
    real = _lib.uprop6_linear
    monkeypatch = pytest.MonkeyPatch()
    monkeypatch.setattr(_lib, "uprop6_linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    try:
        p = UncertaintyPropagator(dyn, gp, ctx=gpu_ctx)
        md, cd = p.propagate_batch(X0, U, S0, 0.1)
        assert calls, "the device path was not taken"
        p.use_device = False
        mh, ch = p.propagate_batch(X0, U, S0, 0.1)
    finally:
        monkeypatch.undo()
    assert md.shape == (B, N + 1, 14) and cd.shape == (B, N + 1, 14, 14)
    np.testing.assert_array_equal(md[:, 0], X0)
    np.testing.assert_allclose(md, mh, rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(cd, ch, rtol=1e-7, atol=1e-15)


# ---- what the three propagators share (csrc/uprop.h), at its edges ------------------------
def _hover3(B, N, seed):
    from gp_mpc_rocket_landing_amd.fleet import initial_conditions
    X0 = initial_conditions(B)
    rs = np.random.RandomState(seed)
    return X0, np.tile((-X0[:, 0:1] * np.array([-1.0, 0, 0]))[:, None, :], (1, N, 1)) * (1 + 0.1 * rs.randn(B, N, 1))


def _gp3_synthetic(n):
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    X, U, D = synthetic_training_data(n, seed=1)
    gp = Simple3DoFGP(use_sparse=False)
    gp.add_data(X, U, D); gp.fit()
    return gp


def _hover6(B, N, seed):
    from gp_mpc_rocket_landing_amd.dynamics import Rocket6DoFConfig
    from gp_mpc_rocket_landing_amd.rollouts6 import initial_conditions_6dof
    X0 = initial_conditions_6dof(B)
    X0[:, 11:14] = np.array([0.02, -0.01, 0.03])
    rs = np.random.RandomState(seed)
    U = np.zeros((B, N, 3))
    U[:, :, 2] = 0.9 * X0[:, 0:1] * Rocket6DoFConfig().g0
    U[:, :, :2] = 0.05 * rs.randn(B, N, 2)
    return X0, U


def _staged_horizon_edge(p, X0, U, dt, atol_m):
    """N = 257 (one step past the 256 whose controls a kernel stages in LDS: it reads them
    from global memory) against N = 256 on the first 256 controls (staged): the arithmetic
    is the same and only the source of u_k differs, so rows 0..256 are equal bit for bit.
    Row 257 against the host loop at the file's tolerances for the model."""
    assert U.shape[1] == 257
    m257, c257 = p.propagate_batch(X0, U, None, dt)
    m256, c256 = p.propagate_batch(X0, U[:, :256], None, dt)
    np.testing.assert_array_equal(m257[:, :257], m256)
    np.testing.assert_array_equal(c257[:, :257], c256)
    p.use_device = False
    mh, ch = p.propagate_batch(X0, U, None, dt)
    print(f"row 257: means {np.abs(m257[:, 257] - mh[:, 257]).max():.3e}, covs rel "
          f"{(np.abs(c257[:, 257] - ch[:, 257]) / np.maximum(np.abs(ch[:, 257]), 1e-300)).max():.3e}")
    np.testing.assert_allclose(m257[:, 257], mh[:, 257], rtol=1e-10, atol=atol_m)
    np.testing.assert_allclose(c257[:, 257], ch[:, 257], rtol=1e-7, atol=1e-15)


def test_horizon_past_staged_controls_3dof(gpu_ctx):
    """gpmpc_uprop3_linear, exact n = 300, B = 2, dt = 0.01."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    X0, U = _hover3(2, 257, 257)
    p = UncertaintyPropagator(create_normalized_rocket(), _gp3_synthetic(300), ctx=gpu_ctx)
    assert p._gate_3dof() is not None, "the device path would not be taken"
    _staged_horizon_edge(p, X0, U, 0.01, 1e-10)


def test_horizon_past_staged_controls_6dof(gpu_ctx):
    """gpmpc_uprop6_linear, FITC M = 50, B = 2, dt = 0.01."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd.dynamics import Rocket6DoFConfig, Rocket6DoFDynamics
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    from gp_mpc_rocket_landing_amd.rollouts6 import fit_structured_gp
    X0, U = _hover6(2, 257, 257)
    p = UncertaintyPropagator(Rocket6DoFDynamics(Rocket6DoFConfig()), fit_structured_gp(300, 50, seed=0, use_sparse=True),
                              ctx=gpu_ctx)
    assert p._gate_6dof() is not None, "the device path would not be taken"
    _staged_horizon_edge(p, X0, U, 0.01, 1e-11)


@pytest.mark.parametrize("n", [1024, 1025], ids=["n1024-last-count-in-registers", "n1025-first-count-read-per-step"])
def test_row_count_boundary_3dof(gpu_ctx, n):
    """The two sides of the 3-DoF register branch (4 rows a thread, 256 threads), vs the host loop."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    X0, U = _hover3(2, 3, n)
    p = UncertaintyPropagator(create_normalized_rocket(), _gp3_synthetic(n), ctx=gpu_ctx)
    assert p._gate_3dof() is not None, "the device path would not be taken"
    md, cd = p.propagate_batch(X0, U, None, 0.1)
    p.use_device = False
    mh, ch = p.propagate_batch(X0, U, None, 0.1)
    np.testing.assert_allclose(md, mh, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(cd, ch, rtol=1e-7, atol=1e-15)


@pytest.mark.parametrize("M", [256, 257], ids=["fitc-M256-last-count-in-registers", "fitc-M257-first-count-read-per-step"])
def test_row_count_boundary_6dof(gpu_ctx, M):
    """The two sides of the 14-state register branch (one row a thread), vs the host loop."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd.dynamics import Rocket6DoFConfig, Rocket6DoFDynamics
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    from gp_mpc_rocket_landing_amd.rollouts6 import fit_structured_gp
    X0, U = _hover6(2, 3, M)
    p = UncertaintyPropagator(Rocket6DoFDynamics(Rocket6DoFConfig()), fit_structured_gp(600, M, seed=1, use_sparse=True),
                              ctx=gpu_ctx)
    assert p._gate_6dof() is not None, "the device path would not be taken"
    md, cd = p.propagate_batch(X0, U, None, 0.1)
    p.use_device = False
    mh, ch = p.propagate_batch(X0, U, None, 0.1)
    np.testing.assert_allclose(md, mh, rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(cd, ch, rtol=1e-7, atol=1e-15)


def test_one_row_gp_3dof(gpu_ctx):
    """n = 1 through gpmpc_uprop3_linear (B = 1, N = 2): every thread but one has no row.  The
    fit is well posed: K = sigma^2 + 1e-4 on one row, the target's std at its floor."""
    _ctx_default(gpu_ctx)
    from gp_mpc_rocket_landing_amd.dynamics import create_normalized_rocket
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    X0, U = _hover3(1, 2, 1)
    p = UncertaintyPropagator(create_normalized_rocket(), _gp3_synthetic(1), ctx=gpu_ctx)
    assert p._gate_3dof() is not None, "the device path would not be taken"
    md, cd = p.propagate_batch(X0, U, None, 0.1)
    p.use_device = False
    mh, ch = p.propagate_batch(X0, U, None, 0.1)
    assert np.all(np.isfinite(md)) and np.all(np.isfinite(cd))
    np.testing.assert_allclose(md, mh, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(cd, ch, rtol=1e-7, atol=1e-15)
