"""BASELINE configs[4] on the device: 6-DoF GP-MPC rollouts (csrc/fleet6.hip)
against the CPU restatement (oracle/sixdof_oracle.py: RK4 of nominal_mpc.py
:163-203, GPMPC.solve's forward simulation with the StructuredRocketGP FITC
means, the QP subproblem of gp_mpc.py:394-460 made linear, the C OSQP-0.6
restatement, the truth plant).

Every control step is checked from the device's own previous state (x, the
warm-start controls U, OSQP's persistent scaled y and rho, the record), so the
inputs are identical: ADMM iterations, status, outcome and step count exact;
the forward-simulated X_pred, its GP means, the QP plan X, the new U, the next
state, rho and the duals within the SURVEY 8c tolerance (1e-6 relative, unit
floor; duals floored at max |y|).

No rollout here is flown to its end: the termination ladder, a QP without a solution, the
record at termination and rows frozen beside flying ones are test_gpu_rollouts6_termination.py."""
import numpy as np
import pytest

from conftest import close

pytestmark = pytest.mark.gpu


def oracle_gps(surface):
    """The oracle FITC pair of a fitted StructuredRocketGP: the same training
    rows and the surface's own inducing points (kmeans2, sparse_gp.py:122-148)."""
    from oracle import gp_oracle
    X, U = np.array(surface.X_data), np.array(surface.U_data)
    Zv = gp_oracle.features_translational(X, U); Zw = gp_oracle.features_rotational(X, U)
    Dv, Dw = np.array(surface.D_v_data), np.array(surface.D_omega_data)
    if not surface.config.use_sparse:
        ev, ew = gp_oracle.exact_fit(Zv, Dv), gp_oracle.exact_fit(Zw, Dw)
        # the exact mean K* alpha is the as-written FITC mean over Zi = the training rows
        return tuple(dict(st, Zi=st["Z"]) for st in (ev, ew))
    return (gp_oracle.fitc_fit(surface.gp_v.gps[0].inducing_points, Zv, Dv),
            gp_oracle.fitc_fit(surface.gp_omega.gps[0].inducing_points, Zw, Dw))


def _one(S, b):
    return {k: (v[b] if k != "rho" else float(v[b])) for k, v in S.items()}


def _run(gpu_ctx, n_train, n_inducing, nb, steps, tol=1e-6, as_written=False, horizon=30, rocket=None, qp=None):
    """tol: one relative bound for every continuous field, or a dict of per-field bounds
    (X_pred, gm, X, U, x, rho, y).  Prints the worst ratio to the bound per field."""
    tols = tol if isinstance(tol, dict) else {k: tol for k in ("X_pred", "gm", "X", "U", "x", "rho", "y")}
    worst_seen = {k: 0.0 for k in tols}

    def check(tag, key, got, want, scale):
        ok, worst = close(got, want, scale, rtol=tols[key])
        worst_seen[key] = max(worst_seen[key], worst)
        assert ok, (tag, key, worst)

    from gp_mpc_rocket_landing_amd.rollouts6 import Rollouts6, fit_structured_fitc, initial_conditions_6dof
    from oracle import sixdof_oracle as so
    gv, gw = fit_structured_fitc(gpu_ctx, n_train=n_train, n_inducing=n_inducing)
    ov, ow = oracle_gps(gv.surface)
    x0 = initial_conditions_6dof(nb)
    kw = {}
    rk = None
    if rocket is not None:   # (J diagonal or 3 x 3, r_T, g_I, I_sp, g0) through the config and the oracle alike
        J, rT, gI, isp, g0 = rocket
        rk = so.rocket_params(J, rT, gI, isp, g0)
        kw = dict(rocket_j=rk["J"], rocket_r_t=rk["r_T"], rocket_g_i=rk["g_I"], rocket_alpha=rk["alpha"],
                  rocket_g0=rk["g0"])
        if "Jf" in rk:
            kw["rocket_J"] = rk["Jf"].reshape(9)
    qs = None
    if qp:   # the same ADMM settings on both sides
        from oracle import admm_ref
        kw.update(qp)
        qs = admm_ref.default_settings(**qp)
    ro = Rollouts6(gpu_ctx, gv, gw, nb, fitc_mean_as_written=int(as_written), horizon=horizon, **kw)
    seen = 0
    try:
        ro.reset(x0)
        S = ro.state()
        for k in range(steps):
            if np.all(S["rec"][:, 0] != 0):
                break
            ro.step(1)
            T = ro.state()
            for b in np.nonzero(S["rec"][:, 0] == 0)[0]:
                st = dict(x=S["x"][b], U=S["U"][b], y=S["y"][b], rho=float(S["rho"][b]), rec=S["rec"][b], X=None)
                want, info = so.rollout_step(ov, ow, st, corrected=not as_written, rk=rk, qp_settings=qs)
                got = _one(T, b)
                tag = (k, int(b))
                np.testing.assert_array_equal(got["rec"][[0, 1, 11, 12, 13, 14]],
                                              want["rec"][[0, 1, 11, 12, 13, 14]], err_msg=str(tag))
                if info is None or want["rec"][0] != 0:
                    continue
                seen += 1
                for key in ("X_pred", "gm", "X", "U", "x"):
                    check(tag, key, got[key], want[key], 1.0)
                check(tag, "rho", got["rho"], want["rho"], 0.0)
                check(tag, "y", got["y"], want["y"], np.abs(want["y"]).max())
            S = T
    finally:
        ro.close()
    print("worst |a - b| / bound per field:", {k: round(v, 4) for k, v in worst_seen.items()})
    return seen, S


def test_rollouts6_match_oracle_small_gp(gpu_ctx):
    """4 rollouts x 40 control steps on a FITC pair with M = 50, N = 300, the
    FITC posterior mean (default)."""
    seen, S = _run(gpu_ctx, 300, 50, 4, 40)
    assert seen >= 40, seen


def test_rollouts6_match_oracle_fitc_mean_as_written(gpu_ctx):
    """The reference's K*u alpha mean (sparse_gp.py:280-283) behind
    fitc_mean_as_written: same parity, 4 rollouts x 10 steps."""
    seen, S = _run(gpu_ctx, 300, 50, 4, 10, as_written=True)
    assert seen >= 10, seen


def test_rollouts6_match_oracle_config5_gp(gpu_ctx):
    """The config-5 GP size (M = 2000 kmeans2 inducing points, N = 4000 training
    rows, two GPs), each side with its own fit: 16 rollouts x 12 control steps.
    K_uu of 2000 inducing points at unit length scales is badly conditioned
    (jitter 1e-6), so the device fit (W = L_uu^-1, beta = W^T alpha) and the numpy
    fit (triangular solves) agree on the GP means to ~2e-9 absolute, and the plans
    to ~1e-8 (measured): inside the 1e-6 spec.  The as-written mean K*u alpha at
    this size is the next test."""
    seen, S = _run(gpu_ctx, 4000, 2000, 16, 12)
    assert seen >= 100, seen


# The as-written mean's sensitivity at config-5 size, measured on the oracle against
# itself (scripts/fitc_as_written_sensitivity.py, profiles/r6_fitc_as_written_sensitivity.json,
# the 16 rollouts x 12 steps below, step-locked): every kernel value of the fit and the
# predictions changed by at most one ulp moves the plans U by up to 5.8e-5 relative (58x the
# 1e-6 spec), the GP means by 9.1e-6, X by 1.8e-6, X_pred by 0.99e-6, the duals by 1.3e-6
# (of max |y|), the next state by 0.53e-6, rho not at all; the integer fields never change.
# alpha itself scaled by one ulp moves nothing above 1e-11.  The device is a second correct
# implementation of the same arithmetic, so its outputs can sit anywhere inside that band:
# each field's bound is ~2x its own measured band, and never below the 1e-6 spec.
AS_WRITTEN_M2000_RTOL = dict(X_pred=2e-6, gm=2e-5, X=4e-6, U=1.2e-4, x=1.1e-6, rho=1e-6, y=2.7e-6)


def test_rollouts6_match_oracle_config5_gp_mean_as_written(gpu_ctx):
    """The reference's as-written FITC mean K*u alpha (sparse_gp.py:280-283, SURVEY D1,
    fitc_mean_as_written=1) at the config-5 GP size (M = 2000, N = 4000), each side
    with its own fit, 16 rollouts x 12 control steps: ADMM iterations, status, outcome
    and step count exact; continuous outputs within AS_WRITTEN_M2000_RTOL, the per-field
    bounds the oracle's own one-ulp sensitivity sets (above).  (Round 4 measured the device
    at 2.7e-6 relative on U here: 2.7x the 1e-6 spec, 20x inside the band.)"""
    seen, S = _run(gpu_ctx, 4000, 2000, 16, 12, tol=AS_WRITTEN_M2000_RTOL, as_written=True)
    assert seen >= 100, seen


def test_rollouts6_shards_reproduce_the_whole_batch(gpu_ctx):
    """Sharding invariance for configs[4]: 64 rollouts flown as one
    batch and as two shards [0, 32), [32, 64) (initial conditions by global
    index, as each rank of run_monte_carlo --six-dof builds its shard) give
    bit-identical records and states."""
    from gp_mpc_rocket_landing_amd.rollouts6 import Rollouts6, fit_structured_fitc, initial_conditions_6dof
    from gp_mpc_rocket_landing_amd.sharding import shard_range
    gv, gw = fit_structured_fitc(gpu_ctx, n_train=300, n_inducing=50)

    def fly(first, count, steps=30):
        r = Rollouts6(gpu_ctx, gv, gw, count)
        try:
            r.reset(initial_conditions_6dof(count, first=first))
            r.step(steps)
            return r.read()
        finally:
            r.close()

    whole_r, whole_x = fly(0, 64)
    parts = [fly(*shard_range(64, rk, 2)) for rk in range(2)]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), whole_r)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), whole_x)


def test_rollouts6_horizon20_nondefault_rocket(gpu_ctx):
    """The N = 20 instance of the 6-DoF kernels (GPMPCConfig's default horizon,
    gp_mpc.py:110) with a non-default Rocket6DoFConfig through the config's rocket
    fields (ABI 3): J_B = diag(0.03, 1.1, 0.9) 0.168, r_T = (-0.3, 0, 0.02),
    g_I = (-1, 0.01, 0), I_sp 25, g0 1.05.  4 rollouts x 25 steps, per step vs
    the oracle with the same rocket (a hover guess m0 g0 and the dynamics)."""
    rocket = (np.array([0.03, 1.1, 0.9]) * 0.168, [-0.3, 0.0, 0.02], [-1.0, 0.01, 0.0], 25.0, 1.05)
    seen, S = _run(gpu_ctx, 300, 50, 4, 25, horizon=20, rocket=rocket)
    assert seen >= 25, seen


def test_rollouts6_full_inertia_tensor(gpu_ctx):
    """VERDICT r5 missing #1: a non-diagonal J_B (rocket_J, ABI 4) in the configs[4]
    rollouts at N = 30: 4 rollouts x 25 steps vs the oracle with the same tensor."""
    from test_gpu_gpmpc6 import J_FULL
    seen, S = _run(gpu_ctx, 300, 50, 4, 25, rocket=(J_FULL, [-0.25, 0.0, 0.0], [-1.0, 0.0, 0.0], 30.0, 1.0))
    assert seen >= 25, seen


def test_rollouts6_horizon20_default_rocket(gpu_ctx):
    """N = 20 with the default rocket: 4 rollouts x 25 steps vs the oracle."""
    seen, S = _run(gpu_ctx, 300, 50, 4, 25, horizon=20)
    assert seen >= 25, seen


@pytest.mark.parametrize("horizon", [15, 7, 2])
def test_rollouts6_odd_and_short_horizons(gpu_ctx, horizon):
    """Rollouts at a horizon other than the two round-4 instances: odd N (the
    bottom end of the twisted factor one block step shorter) and the shortest,
    N = 2; 4 rollouts x 20 steps, small GP, vs the oracle."""
    seen, S = _run(gpu_ctx, 300, 50, 4, 20, horizon=horizon)
    assert seen >= 20, seen


def test_rollouts6_solved_setting(gpu_ctx):
    """the configs[4] controller at the ADMM setting where >= 90% of
    its QPs return "solved" (bench.SOLVED_QP6: max_iter 4000, eps 1e-4), 4 rollouts
    x 8 steps vs the oracle with the same settings: iterations / status exact,
    plans and duals 1e-6."""
    import bench
    seen, S = _run(gpu_ctx, 300, 50, 4, 8, qp=dict(bench.SOLVED_QP6))
    assert seen >= 8, seen


def test_rollouts6_rejects_nonpositive_max_iter(gpu_ctx):
    """OSQP's settings check refuses max_iter <= 0 ("max_iter must be positive"); the
    device controller, which runs its final termination checks inside the last ADMM
    iteration, refuses it at creation the same way."""
    from gp_mpc_rocket_landing_amd import _lib
    from gp_mpc_rocket_landing_amd.rollouts6 import Rollouts6, fit_structured_fitc
    gv, gw = fit_structured_fitc(gpu_ctx, n_train=120, n_inducing=20)
    with pytest.raises(_lib.HIPError, match="max_iter must be positive"):
        Rollouts6(gpu_ctx, gv, gw, 2, max_iter=0)


@pytest.mark.gpu
def test_rollouts6_split_predict_is_bit_identical(gpu_ctx, monkeypatch):
    """The predict kernel's split (each rollout's kernel rows over four co-resident
    workgroups, per-wave sums exchanged as tagged granules; on by default when four
    workgroups per rollout fit the device) gives the same bits as one workgroup per
    rollout (GPMPC_R6_SPLIT=0): the rows are split by whole waves and every part sums
    the same per-wave values in the same order.  M = 1000 inducing rows: past the LDS
    row cache, so both the LDS and the global row paths run; the Monte-Carlo steps and
    a GPMPC.solve loop (modes 1 and 2) both checked."""
    from gp_mpc_rocket_landing_amd.rollouts6 import Rollouts6, fit_structured_fitc, initial_conditions_6dof
    gv, gw = fit_structured_fitc(gpu_ctx, n_train=2000, n_inducing=1000)

    def fly(split):
        monkeypatch.setenv("GPMPC_R6_SPLIT", "1" if split else "0")
        r = Rollouts6(gpu_ctx, gv, gw, 64)
        try:
            x0 = initial_conditions_6dof(64)
            r.reset(x0)
            r.step(6)
            rec, x = r.read()
            st = r.state()
            tgt = np.zeros_like(x0)
            tgt[:, 0] = x0[:, 0]
            sol = r.solve(x0, tgt, cold=1, max_sqp_iter=3)
            return rec, x, st, sol
        finally:
            r.close()

    a, b = fly(True), fly(False)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    for k in a[2]:
        np.testing.assert_array_equal(a[2][k], b[2][k], err_msg=k)
    for k in a[3]:
        np.testing.assert_array_equal(a[3][k], b[3][k], err_msg=k)
