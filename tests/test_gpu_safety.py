"""The safety filter on the device (csrc/safety.hip) against the reference's recorded results
(tests/golden/safety.npz).  The discrete fields (flags, violation masks, iteration counts) are
equal exactly: the fixture's decision gaps are >= 1000 x the spread of one rounding per step.
The continuous ones are within 64 x that spread plus 8 ulp of the value: the device differs
from numpy in several hundred operations per step (fused multiply-adds, the summation order of
K dx and dx' P dx, the division, the square root), about sqrt(300) roundings with a factor 4
of margin, still 15 times inside the decision gaps."""
import numpy as np
import pytest
from conftest import golden

import safety_cases as sc
from gp_mpc_rocket_landing_amd import safety

pytestmark = pytest.mark.gpu

DISCRETE = (("is_modified", "is_modified"), ("is_safe", "is_safe"), ("mask", "violation_mask"), ("iters", "iterations"))
CONTINUOUS = (("u_safe", "u_safe", "spread_u"), ("margin", "safety_margin", "spread_margin"),
              ("value", "backup_value", "spread_value"))
ROW_FIELDS = ("u_safe", "is_modified", "is_safe", "safety_margin", "backup_value", "violation_mask", "iterations")


@pytest.fixture(scope="module")
def g():
    return golden("safety.npz")


@pytest.fixture(scope="module")
def filters(g, gpu_ctx):
    import os
    assert os.environ.get("GPMPC_SAFETY", "") in ("", "device")
    out = {}
    for name in sc.CONFIGS:
        f = sc.make_filter(sc.load_spec(g, name), safety)
        f.ctx = gpu_ctx
        out[name] = f
    return out


@pytest.fixture(scope="module")
def singles(g, filters):
    """The B = 1 device answer of every case, computed once: {name: [SafetyFilterBatch]}."""
    out = {}
    for name, f in filters.items():
        out[name] = [f.filter_batch(x[None], u[None]) for x, u in zip(g[f"{name}_X"], g[f"{name}_U"])]
        assert f.last_path == "device"
    return out


def within(got, want, spread, what):
    """|got - want| <= 64 spread + 8 ulp(want); prints the achieved share of the bound."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    tol = 64.0 * float(spread) + 8.0 * np.spacing(np.abs(want))
    err = np.abs(got - want)
    print(f"{what}: max error {np.max(err):.3e}, largest share of the bound {np.max(err / tol):.3f}")
    assert np.all(err <= tol), (what, float(np.max(err)), float(np.max(err / tol)))


def rows_equal(batch, singles, idx, what):
    for j, i in enumerate(idx):
        for k in ROW_FIELDS:
            assert np.array_equal(getattr(batch, k)[j], getattr(singles[i], k)[0]), (what, j, i, k)


class SimpleRows:
    """Rows ``idx`` of a batch, with the batch's field names."""

    def __init__(self, batch, idx):
        for k in ROW_FIELDS:
            setattr(self, k, getattr(batch, k)[idx])


@pytest.mark.parametrize("name", sc.CONFIGS)
def test_filter_batch_against_the_reference(g, filters, name):
    f = filters[name]
    out = f.filter_batch(g[f"{name}_X"], g[f"{name}_U"])
    assert f.last_path == "device", f.last_reason
    for key, attr in DISCRETE:
        assert np.array_equal(getattr(out, attr), g[f"{name}_{key}"]), (name, key, getattr(out, attr), g[f"{name}_{key}"])
    for key, attr, spread in CONTINUOUS:
        within(getattr(out, attr), g[f"{name}_{key}"], g[spread], f"{name} {key}")
    # an unmodified control is returned as given
    keep = ~g[f"{name}_is_modified"]
    assert np.array_equal(out.u_safe[keep], g[f"{name}_U"][keep])


@pytest.mark.parametrize("B", [1, 15, 16, 17])
def test_batch_rows_do_not_depend_on_their_neighbours(g, filters, singles, B):
    """One quad, a partial wave, a full wave, a wave and a single quad: row i is the B = 1 answer."""
    out = filters["B"].filter_batch(g["B_X"][:B], g["B_U"][:B])
    assert len(out) == B
    rows_equal(out, singles["B"], range(B), f"B={B}")


def test_mixed_divergence_wave(g, filters, singles):
    """A safe, an early-exit and a 50-iteration quad in one wave."""
    idx = g["mix_idx"]
    out = filters["B"].filter_batch(g["B_X"][idx], g["B_U"][idx])
    rows_equal(out, singles["B"], idx, "mix")
    assert np.array_equal(out.iterations, g["B_iters"][idx]) and np.array_equal(out.is_modified, g["B_is_modified"][idx])


def test_tiled_batch_over_several_workgroups(g, filters, singles):
    n = len(g["A_X"])
    idx = np.arange(130) % n
    out = filters["A"].filter_batch(g["A_X"][idx], g["A_U"][idx])
    rows_equal(out, singles["A"], idx, "tiled")
    assert np.array_equal(out.iterations, g["A_iters"][idx])


@pytest.mark.parametrize("name", sc.CONFIGS)
def test_single_call_surface(g, filters, name):
    f = filters[name]
    it, mod = g[f"{name}_iters"], g[f"{name}_is_modified"]
    picks = {len(it) - 1}
    for sel in (~mod, mod & (it == 0), mod & (it > 0) & (it < 50), it == 50):
        if np.any(sel):
            picks.add(int(np.where(sel)[0][0]))
    for i in sorted(picks):
        r = f.filter(g[f"{name}_X"][i], g[f"{name}_U"][i])
        assert f.last_path == "device"
        assert (r.is_modified, r.is_safe) == (bool(mod[i]), bool(g[f"{name}_is_safe"][i]))
        assert safety.safety_filter.violations_to_mask(r.constraint_violations) == int(g[f"{name}_mask"][i])
        within(r.u_safe, g[f"{name}_u_safe"][i], g["spread_u"], f"{name}[{i}] u_safe")
        within(r.safety_margin, g[f"{name}_margin"][i], g["spread_margin"], f"{name}[{i}] margin")
        within(r.backup_value, g[f"{name}_value"][i], g["spread_value"], f"{name}[{i}] value")
        assert r.constraint_violations["terminal"] == r.safety_margin


def test_simulate_filtered_batch(g, filters):
    f = filters["B"]
    X, U, info = f.simulate_filtered_batch(g["sim_X0"], g["sim_U_nom"])
    assert f.last_path == "device" and X.shape == (3, 6, 14) and U.shape == (3, 5, 3)
    assert np.array_equal(info.is_modified, g["sim_is_modified"]) and np.array_equal(info.is_safe, g["sim_is_safe"])
    assert np.array_equal(info.iterations, g["sim_iters"])
    assert np.array_equal(X[:, 0], g["sim_X0"])
    within(X, g["sim_X"], g["sim_spread_X"], "closed loop X")
    within(U, g["sim_U"], g["sim_spread_U"], "closed loop U")
    within(info.safety_margin, g["sim_margin"], g["spread_margin"], "closed loop margin")
    # a start's flight does not depend on its neighbours, and T = 0 is the start alone
    X1, U1, _ = f.simulate_filtered_batch(g["sim_X0"][1:2], g["sim_U_nom"][1:2])
    assert np.array_equal(X1[0], X[1]) and np.array_equal(U1[0], U[1])
    X0, U0, _ = f.simulate_filtered_batch(g["sim_X0"], np.zeros((3, 0, 3)))
    assert np.array_equal(X0[:, 0], g["sim_X0"]) and U0.shape == (3, 0, 3)


def test_refusals_leave_the_context_usable(g, filters, gpu_ctx):
    from gp_mpc_rocket_landing_amd import _lib
    f = filters["B"]
    cfg, rocket = f._device_config()
    X, U = g["B_X"][:2], g["B_U"][:2]
    Un = np.tile(U[:, None, :], (1, 2, 1))

    def both(rk, c, x, u, un, match):
        with pytest.raises(_lib.HIPError, match=match) as e:
            _lib.safety_filter(gpu_ctx, rk, c, x, u)
        assert e.value.rc == -2
        with pytest.raises(_lib.HIPError, match=match) as e:
            _lib.safety_simulate(gpu_ctx, rk, c, x, un)
        assert e.value.rc == -2

    for horizon in (0, 32):
        bad, _ = f._device_config()
        bad.horizon = horizon
        both(rocket, bad, X, U, Un, "horizon")
    both(rocket, cfg, np.zeros((0, 14)), np.zeros((0, 3)), np.zeros((0, 2, 3)), "batch")
    singular = rocket.copy()
    singular[:9] = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 1.0]]).ravel()
    both(singular, cfg, X, U, Un, "J_B")
    bad, _ = f._device_config()
    bad.dt = 0.0
    both(rocket, bad, X, U, Un, "dt")
    out = f.filter_batch(X, U)
    assert np.array_equal(out.iterations, g["B_iters"][:2]) and np.array_equal(out.is_modified, g["B_is_modified"][:2])


def test_a_nan_state_follows_the_ieee_comparisons(g, filters, singles, monkeypatch):
    """A NaN velocity: every comparison with V fails, so the loop runs out with a NaN control,
    as in numpy; the query's neighbours in the wave do not notice."""
    f = filters["A"]
    X, U = g["A_X"][:3].copy(), g["A_U"][:3].copy()
    X[1, 5] = np.nan
    out = f.filter_batch(X, U)
    assert f.last_path == "device"
    monkeypatch.setenv("GPMPC_SAFETY", "host")
    ref = f.filter_batch(X[1:2], U[1:2])
    assert f.last_path == "host"
    assert ref.iterations[0] == 50 and np.all(np.isnan(ref.u_safe[0])) and not ref.is_safe[0]
    for k in ("is_modified", "is_safe", "violation_mask", "iterations"):
        assert getattr(out, k)[1] == getattr(ref, k)[0], k
    assert np.all(np.isnan(out.u_safe[1])) and np.isnan(out.safety_margin[1]) and np.isnan(out.backup_value[1])
    rows_equal(SimpleRows(out, [0, 2]), singles["A"], [0, 2], "beside a NaN")
