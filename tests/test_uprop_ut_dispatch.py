"""Which unscented propagations take the one-call device recursion (gpmpc_uprop3_unscented /
gpmpc_uprop6_unscented) and which keep the per-step host loop: the selection is host logic,
checked here without a GPU (every case below is refused before any device call)."""
import os
import sys

import numpy as np
import pytest

from gp_mpc_rocket_landing_amd import _lib
from gp_mpc_rocket_landing_amd.dynamics import Rocket6DoFDynamics, create_normalized_rocket
from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP, StructuredGPConfig, StructuredRocketGP
from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))


def _no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device propagation was attempted")
    monkeypatch.setattr(_lib, "uprop3_unscented", refuse)
    monkeypatch.setattr(_lib, "uprop6_unscented", refuse)


def test_ut_params_default_to_the_references_constants():
    assert UncertaintyPropagator.ut_params == (1e-3, 2.0, 0.0)
    p = UncertaintyPropagator(create_normalized_rocket(), Simple3DoFGP(), method="unscented", ctx=object())
    assert p.ut_params == (1e-3, 2.0, 0.0)


def test_unfitted_gps_keep_the_host_loop(monkeypatch):
    _no_device(monkeypatch)
    X0 = np.zeros((1, 7)); U = np.zeros((1, 3, 3))
    dyn = create_normalized_rocket()
    for gp in (Simple3DoFGP(use_sparse=False), Simple3DoFGP(use_sparse=True)):
        p = UncertaintyPropagator(dyn, gp, method="unscented", ctx=object())
        assert p._device_unscented(X0, U, None, 0.1) is None
    p = UncertaintyPropagator(Rocket6DoFDynamics(), StructuredRocketGP(), method="unscented", ctx=object())
    assert p._device_unscented(np.zeros((1, 14)), U, None, 0.1) is None


def test_other_models_and_feature_settings_keep_the_host_loop(monkeypatch):
    _no_device(monkeypatch)
    from toy_dynamics import ToyRocket14
    X0 = np.zeros((1, 14)); U = np.zeros((1, 3, 3))

    class Other(Rocket6DoFDynamics):   # a subclass is another model: the device restates only the base
        pass

    def fitted(**cfg):
        g = StructuredRocketGP(StructuredGPConfig(**cfg))
        g._is_fitted = True
        return g

    for dyn, g in ((Other(), fitted()), (ToyRocket14(), fitted()), (Rocket6DoFDynamics(), fitted(reference_velocity=20.0)),
                   (Rocket6DoFDynamics(), fitted(include_altitude=False))):
        p = UncertaintyPropagator(dyn, g, method="unscented", ctx=object())
        assert p._device_unscented(X0, U, None, 0.1) is None


def test_use_device_false_is_honoured(monkeypatch):
    _no_device(monkeypatch)
    gp = Simple3DoFGP(use_sparse=False)
    gp._is_fitted = True
    p = UncertaintyPropagator(create_normalized_rocket(), gp, method="unscented", ctx=object())
    p.use_device = False
    assert p._device_unscented(np.zeros((1, 7)), np.zeros((1, 2, 3)), None, 0.1) is None


def test_host_loop_runs_the_batch_and_reads_ut_params(monkeypatch):
    """An unfitted GP without data predicts zeros / 0.1 on the host: the batch surface, its
    shapes, its Sigma_0 forms and ut_params without any device."""
    _no_device(monkeypatch)
    dyn = create_normalized_rocket()
    p = UncertaintyPropagator(dyn, Simple3DoFGP(use_sparse=False), method="unscented", ctx=object())
    rs = np.random.RandomState(0)
    X0 = np.array([2.0, 30.0, 1.0, -1.0, -3.0, 0.2, 0.1]) + 0.01 * rs.randn(2, 7)
    U = np.tile(np.array([2.0, 0.1, 0.0]), (2, 3, 1))
    m, c = p.propagate_unscented_batch(X0, U, None, 0.1)
    assert m.shape == (2, 4, 7) and c.shape == (2, 4, 7, 7)
    np.testing.assert_array_equal(m[:, 0], X0)
    np.testing.assert_array_equal(c[:, 0], np.broadcast_to(np.eye(7) * 1e-6, (2, 7, 7)))
    S = np.eye(7) * 1e-4
    m1, c1 = p.propagate_unscented_batch(X0, U, S, 0.1)
    m2, c2 = p.propagate_unscented_batch(X0, U, np.broadcast_to(S, (2, 7, 7)), 0.1)
    np.testing.assert_array_equal(m1, m2); np.testing.assert_array_equal(c1, c2)
    r = p.propagate(X0[1], U[1], S, 0.1)            # the single-trajectory surface: a batch of one
    np.testing.assert_array_equal(r.means, m1[1]); np.testing.assert_array_equal(r.covariances, c1[1])
    # ut_params is read: other constants, another result; r + dt v is linear, so at alpha = 1
    # (weights O(1)) the first step's position mean is the nominal step's to rounding
    p.ut_params = (1.0, 2.0, 0.0)
    m3, _ = p.propagate_unscented_batch(X0, U, S, 0.1)
    assert np.any(m3 != m1)
    np.testing.assert_allclose(m3[0, 1, 1:4], dyn.step(X0[0], U[0, 0], 0.1)[1:4], rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        p.propagate_unscented_batch(X0, U, np.eye(6), 0.1)
    Sbad = S.copy(); Sbad[2, 2] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        p.propagate_unscented_batch(X0, U, Sbad, 0.1)
