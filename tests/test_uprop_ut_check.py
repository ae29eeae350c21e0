"""The numpy restatement of the unscented propagation (tests/uprop_ut_check.py) against the
reference's own output (F9: exact StructuredRocketGP on F5, toy 14-state plant), without a
GPU.  The bounds are those of the device test of the same fixture
(test_gpu_uprop.py::test_propagation_vs_f9): the reference's alpha = 1e-3 weights the centre
point by ~ -1e6, so 1e-13 in the sigma points' images is ~1e-7 in the mean."""
import os
import sys

import numpy as np
import pytest

from conftest import golden

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

import uprop_ut_check  # noqa: E402


@pytest.fixture(scope="module")
def f9_runs():
    from toy_dynamics import ToyRocket14
    from oracle import uprop_oracle
    f5 = golden("f5_structured_6dof.npz"); f9 = golden("f9_uncertainty_prop.npz")
    gp = uprop_oracle.structured_exact_predictor(f5["X"], f5["U"], f5["Dv"], f5["Dw"])
    args = (ToyRocket14(), gp, f9["x0"], f9["U"], f9["S0_unscented"], 0.1)
    return f9, uprop_ut_check.propagate_unscented(*args), uprop_ut_check.propagate_unscented(*args, reverse_sum=True)


def test_restatement_reproduces_f9(f9_runs):
    f9, (means, covs), _ = f9_runs
    print("restatement vs F9: means", np.abs(means - f9["unscented_means"]).max(),
          "covs", np.abs(covs - f9["unscented_covs"]).max())
    np.testing.assert_allclose(means, f9["unscented_means"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(covs, f9["unscented_covs"], rtol=0, atol=1e-9)


def test_reverse_order_sum_stays_within_the_same_bounds(f9_runs):
    """The order of the additions of x_next alone moves the result by the noise floor of the
    reference's arithmetic: not zero (the sum is not exact), and inside the F9 bounds."""
    f9, (means, covs), (mr, cr) = f9_runs
    dm, dc = np.abs(mr - means).max(), np.abs(cr - covs).max()
    print("reverse-order sum vs forward: means", dm, "covs", dc)
    assert 0 < dm <= 2e-6 and dc <= 1e-9
    np.testing.assert_allclose(mr, f9["unscented_means"], rtol=0, atol=2e-6 + dm)
    np.testing.assert_array_equal(mr[0], means[0])


def test_weights_are_the_references():
    lam, w_m, w_c = uprop_ut_check.ut_weights(14)
    assert lam == 1e-3 ** 2 * 14 - 14
    assert np.isclose(w_m.sum(), 1.0, rtol=0, atol=1e-9)
    assert w_c[0] - w_m[0] == pytest.approx(1 - 1e-6 + 2.0, abs=1e-9)
    lam1, w1, _ = uprop_ut_check.ut_weights(7, (1.0, 2.0, 0.0))
    assert lam1 == 0 and w1[0] == 0 and np.all(w1[1:] == 1 / 14)


def test_indefinite_covariance_raises():
    from toy_dynamics import ToyRocket14
    S = np.eye(14) * 1e-4
    S[3, 3] = -1e-4
    with pytest.raises(np.linalg.LinAlgError):
        uprop_ut_check.propagate_unscented(ToyRocket14(), lambda x, u: (np.zeros(3), np.zeros(3), np.ones(3), np.ones(3)),
                                           np.ones(14), np.zeros((2, 3)), S, 0.1, (1.0, 2.0, 0.0))
