"""The numpy restatement of the Monte-Carlo propagation (tests/uprop_mc_check.py) against the
reference's own output (F9) and its draw order; no GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import golden

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))


def test_restatement_reproduces_f9():
    """Under the fixture's seed the restatement lands on F9's monte_carlo_means / _covs at the
    tolerances of test_gpu_uprop.py::test_propagation_vs_f9: the draw order is the reference's."""
    import uprop_mc_check
    from oracle import uprop_oracle
    from toy_dynamics import ToyRocket14
    f5 = golden("f5_structured_6dof.npz"); f9 = golden("f9_uncertainty_prop.npz")
    gp = uprop_oracle.structured_exact_predictor(f5["X"], f5["U"], f5["Dv"], f5["Dw"])
    np.random.seed(123)
    particles0, z = uprop_mc_check.draw(f9["x0"], None, len(f9["U"]), 100, 2)
    means, covs, paths = uprop_mc_check.propagate_mc(ToyRocket14(), gp, particles0, z, f9["U"], 0.1, f9["x0"], None)
    gm = np.abs(means - f9["monte_carlo_means"]).max(); gc = np.abs(covs - f9["monte_carlo_covs"]).max()
    print(f"restatement vs F9: means {gm:.3e}, covs {gc:.3e}")
    np.testing.assert_allclose(means, f9["monte_carlo_means"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(covs, f9["monte_carlo_covs"], rtol=1e-6, atol=1e-12)
    assert paths.shape == (11, 100, 14)
    np.testing.assert_array_equal(paths[0], particles0)


@pytest.mark.parametrize("G,S", [(1, 5), (1, 100), (2, 7)], ids=["G1-odd-count-per-step", "G1-S100", "G2"])
def test_draw_is_the_references_per_particle_sequence(G, S):
    """One randn(S, G, 3) per step is the reference's per-particle randn(3) (, randn(3)) -- also
    when a step draws an odd count of normals and the legacy generator carries its cached
    second normal into the next call."""
    import uprop_mc_check
    n, N = (7, 4) if G == 1 else (14, 3)
    rs = np.random.RandomState(G * 10 + S)
    x0 = rs.randn(n); L = 0.1 * rs.randn(n, n); S0 = L @ L.T
    np.random.seed(7)
    particles0, z = uprop_mc_check.draw(x0, S0, N, S, G)
    after = np.random.get_state()
    np.random.seed(7)
    want0 = np.random.multivariate_normal(x0, S0, S)
    want = np.empty((N, S, G, 3))
    for k in range(N):
        for i in range(S):
            for g in range(G):
                want[k, i, g] = np.random.randn(3)
    np.testing.assert_array_equal(particles0, want0)
    np.testing.assert_array_equal(z, want)
    ref_after = np.random.get_state()
    assert after[0] == ref_after[0] and np.array_equal(after[1], ref_after[1]) and after[2:] == ref_after[2:]


@pytest.mark.parametrize("S", [2, 65, 100, 4096])
def test_sequential_mean_is_numpys_axis0_mean(S):
    import uprop_mc_check
    rs = np.random.RandomState(S)
    a = rs.randn(S, 14) * np.logspace(-3, 3, 14) + rs.randn(14)
    np.testing.assert_array_equal(uprop_mc_check.sequential_mean(a), np.mean(a, axis=0))
    np.testing.assert_array_equal(uprop_mc_check.sequential_mean(a[:, :7].copy()), np.mean(a[:, :7].copy(), axis=0))
