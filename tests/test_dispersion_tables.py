"""The key tables of the device batch (experiments/dispersion.py: thrust_key_table,
wind_step_offsets, wind_key_table, plant_batch) against DispersedDynamics itself: the control
the wrapper applies and the wind it adds, read back from a recording plant, bit for bit.

The reseed key of DRYDEN is seed + int(t * 100) with t = step_count * dt in floats.  At dt = 0.1
the truncation never differs from 10 s (checked below for every step up to 5000); at dt = 0.01
it does (s = 29: 0.29 * 100 truncates to 28), so the tables are checked at both."""
import numpy as np
import pytest

from gp_mpc_rocket_landing_amd.experiments import (AeroDispersionConfig, DispersedDynamics, DispersionConfig,
                                                   ThrustDispersionConfig, WindConfig, WindModel, dispersion)


class Params:
    g = 1.0


class Recorder:
    """A plant that moves nothing: x_next = 0, so DispersedDynamics' result is wind x dt (aero
    off) and the applied control is on record."""
    params = Params()

    def __init__(self):
        self.applied = []

    def step(self, x, u, dt):
        self.applied.append(np.array(u))
        return np.zeros(7)


def configs():
    thrust = ThrustDispersionConfig(thrust_scale_std=0.05, misalignment_std=0.02, fluctuation_std=0.03, enabled=True)
    return {
        "constant": DispersionConfig(wind=WindConfig(model=WindModel.CONSTANT, wind_velocity=np.array([2.0, 1.0, -0.5])),
                                     thrust=thrust),
        "gust": DispersionConfig(wind=WindConfig(model=WindModel.GUST, gust_amplitude=7.0, gust_probability=3.0), thrust=thrust),
        "dryden": DispersionConfig(wind=WindConfig(model=WindModel.DRYDEN, turbulence_intensity=2.0), thrust=thrust),
    }


@pytest.mark.parametrize("dt", [0.1, 0.01])
@pytest.mark.parametrize("name", ["constant", "gust", "dryden"])
def test_tables_reproduce_the_applied_control_and_the_wind(name, dt):
    dcfg = configs()[name]
    seed, B, T = 42, 5, 40
    kw = dispersion.plant_batch(dcfg, seed, B, dt, T)
    ttab, wtab, wrow = kw["thrust_table"], kw["wind_table"], kw["wind_rows"]
    assert ttab.shape == (B + T, 4) and wrow.shape == (T,) and wrow.min() == 0 and len(wtab) == B + wrow.max()
    assert kw["wind_altitude_factor"] == (name == "dryden") and "drag_cda" not in kw
    rs = np.random.RandomState(0)
    gusts = 0
    for i in range(B):
        rec = Recorder()
        d = DispersedDynamics(rec, dcfg, seed=seed + i)
        for s in range(1, T + 1):
            x = np.concatenate([[2.0], rs.randn(3) * 60.0, rs.randn(3)])   # x[3] on both sides of 10 and 100
            u = rs.randn(3) + [3.0, 0.0, 0.0]
            x_next = d.step(x, u, dt)
            t = ttab[i + s]
            ua = u.copy()
            ua[0] *= t[0]; ua[1] += t[1]; ua[2] += t[2]; ua[0] *= t[3]
            assert np.array_equal(rec.applied[-1], ua), (i, s)
            w = wtab[i + wrow[s - 1]].copy()
            if name == "dryden":
                w *= min(1.0, max(x[3], 10) / 100)
            assert np.array_equal(x_next[4:7], np.zeros(3) + w * dt), (i, s)
            gusts += name == "gust" and bool(np.any(w != 0))
    if name == "gust":
        assert 0 < gusts < B * T   # both branches of the gust draw


def test_the_offsets_truncate_as_python_floats_do():
    off = dispersion.wind_step_offsets(WindModel.DRYDEN, 0.1, 60)
    s = np.arange(1, 61)
    assert np.array_equal(off, [k + 1000 + int((k * 0.1) * 100) for k in s])
    big = np.arange(1, 5001)
    assert np.array_equal(dispersion.wind_step_offsets(WindModel.DRYDEN, 0.1, 5000), big + 1000 + 10 * big)
    fine = dispersion.wind_step_offsets(WindModel.DRYDEN, 0.01, 40)
    assert int((29 * 0.01) * 100) == 28 and fine[28] == 29 + 1000 + 28 and fine[27] == 28 + 1000 + 28   # one key twice
    g = dispersion.wind_step_offsets(WindModel.GUST, 0.1, 60)
    assert np.array_equal(g, [k + 1000 + int((k * 0.1) * 10) for k in s])
    assert np.all(np.diff(off) >= 1) and np.all(np.diff(g) >= 1)
    for model in (WindModel.NONE, WindModel.CONSTANT, WindModel.CUSTOM):
        assert not dispersion.wind_step_offsets(model, 0.1, 5).any()
    assert dispersion.plant_batch(DispersionConfig(wind=WindConfig(model=WindModel.CUSTOM)), 42, 3, 0.1, 5) == {}
    assert dispersion.plant_batch(DispersionConfig.nominal(), 42, 3, 0.1, 5) == {}


def test_the_drag_coefficients_are_the_wrappers_samples_and_leave_the_stream_alone():
    dcfg = DispersionConfig(aero=AeroDispersionConfig(Cd_std=0.2, A_std=0.1, enabled=True))
    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    kw = dispersion.plant_batch(dcfg, 50, 4, 0.1, 10)
    assert np.array_equal(np.random.get_state()[1], before) and set(kw) == {"drag_cda"}
    for i in range(4):
        p = DispersedDynamics(Recorder(), dcfg, seed=50 + i).aero_params
        assert kw["drag_cda"][i] == 0.5 * 0.02 * p["Cd"] * p["A"]
