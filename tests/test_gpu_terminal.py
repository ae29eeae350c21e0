"""gp_mpc_rocket_landing_amd.terminal on the device (GPMPC_KNN=device) against the reference's
own outputs in tests/golden/safeset.npz: the checks of tests/test_terminal_host.py with the
neighbours from gpmpc_knn_query, the batch forms against the loop, and the host path for a
configuration the kernel does not take."""
import numpy as np
import pytest
from scipy.spatial import KDTree

from conftest import golden
from test_terminal_host import U, build_set, check_interp, check_q_functions, check_queries, gamma

pytestmark = pytest.mark.gpu
SETS = ("s7", "s14")


@pytest.fixture()
def device_knn(monkeypatch, gpu_ctx):
    from gp_mpc_rocket_landing_amd import _lib
    monkeypatch.setenv("GPMPC_KNN", "device")
    monkeypatch.setattr(_lib, "_default_ctx", gpu_ctx)       # one context for the session


@pytest.mark.parametrize("name", SETS)
def test_query_and_interpolate_q_are_the_references_bits(device_knn, name):
    """query, query_batch (equal to the loop over query) and single interpolate_q."""
    g = golden("safeset.npz")
    ss = build_set(g, name)
    check_queries(g, name, ss, "device")
    check_interp(g, name, ss)


@pytest.mark.parametrize("name", SETS)
def test_interpolate_q_batch_within_the_rounding_of_its_sums(device_knn, name):
    """The fused call against the fixture.  Both sides form the same weights 1 / (d + 1e-10)
    from equal distances; then K - 1 additions for their sum, a division, a product and K - 1
    additions of non-negative terms (q is a cost-to-go of non-negative stage costs): 2K
    roundings a side, the two within 2 gamma(2K) (1 + gamma(2K)) relative, K the number of
    neighbours the reference took for that query (the fixture's query count)."""
    from gp_mpc_rocket_landing_amd.terminal import LocalSafeSet, LocalSafeSetConfig
    g = golden("safeset.npz")
    ss = build_set(g, name)
    Xq = g[f"{name}_Xq"].astype(np.float64)
    k10 = list(g["ks"]).index(10)                             # interpolate_q's K is config.K = 10
    for a, adaptive in enumerate((True, False)):
        ls = LocalSafeSet(ss, LocalSafeSetConfig(adaptive_K=adaptive))
        assert np.array_equal(ls.interpolate_q_batch(Xq, method="nearest"), g[f"{name}_interp"][a, 0])
        K = g[f"{name}_query_count"][a, 0, k10].astype(np.int64)   # the reference's K of every query
        bound = 2 * gamma(2 * K) * (1 + gamma(2 * K))
        for m, method in ((1, "inverse_distance"), (2, "linear")):
            want = g[f"{name}_interp"][a, m]
            got = ls.interpolate_q_batch(Xq, method=method)
            assert ls.last_path == "device"
            err = np.abs(got - want) / np.abs(want)
            print(name, adaptive, method, "max error", float(np.max(err / U)), "u; bounds", bound / U, "u")
            assert np.all(err <= bound)
            assert np.array_equal(got[-2:], want[-2:])         # the stored states: their own q
        ls.invalidate()
        assert ls._knn is None


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("name", SETS)
def test_interpolate_q_batch_with_a_k_of_the_callers(device_knn, name, adaptive):
    """K = 20 against config.K = 10: with adaptive K the rule scales config.K and the caller's K
    plays no part, as in the reference; without it the caller's K counts.  Against the loop over
    interpolate_q (the reference's numpy lines on the device's neighbours), each query within the
    2 gamma(2K) (1 + gamma(2K)) of its own K; "nearest" for equal bits."""
    from gp_mpc_rocket_landing_amd.terminal import LocalSafeSet, LocalSafeSetConfig
    g = golden("safeset.npz")
    ss = build_set(g, name)
    Xq = g[f"{name}_Xq"].astype(np.float64)
    ls = LocalSafeSet(ss, LocalSafeSetConfig(adaptive_K=adaptive))
    K = np.array([len(ls.query(x, 20)[1]) for x in Xq])
    K10 = np.array([len(ls.query(x)[1]) for x in Xq])
    assert np.array_equal(K, K10) if adaptive else np.all(K == 20)
    assert np.any(K != 20) or not adaptive
    for method in ("inverse_distance", "linear", "nearest"):
        want = np.array([ls.interpolate_q(x, 20, method=method) for x in Xq])
        got = ls.interpolate_q_batch(Xq, 20, method=method)
        assert ls.last_path == "device"
        if method == "nearest":
            assert np.array_equal(got, want)
            continue
        err = np.abs(got - want) / np.abs(want)
        bound = 2 * gamma(2 * K) * (1 + gamma(2 * K))
        print(name, adaptive, method, "K", K.tolist(), "max error", float(np.max(err / U)), "u")
        assert np.all(err <= bound), (err / U, bound / U)
    # the host path takes the same K
    host = LocalSafeSet(ss, LocalSafeSetConfig(adaptive_K=adaptive, K_max=50, distance_metric="euclidean"))
    hq = host.interpolate_q_batch(Xq, 20)
    assert host.last_path == "host"
    assert np.array_equal(hq, np.array([ls.interpolate_q(x, 20) for x in Xq]))


def test_gp_q_function(device_knn):
    """GPQFunction fits this project's sparse GP: its mean is that of a SparseGP built
    the same way, clipped to [q_min, q_max]; unfitted it returns q_max."""
    from gp_mpc_rocket_landing_amd.gp import SparseGP, SquaredExponentialARD
    from gp_mpc_rocket_landing_amd.terminal import GPQFunction, QFunctionConfig, QFunctionManager
    g = golden("safeset.npz")
    ss = build_set(g, "s7")
    states, q = ss.get_all_states(), ss.get_all_q_values()
    Xq = g["s7_Xq"].astype(np.float64)
    cfg = QFunctionConfig(method="gp", gp_lengthscale=2.0, gp_variance=4.0)
    blank = GPQFunction(QFunctionConfig(q_max=123.0))
    assert blank.predict(Xq[0]) == 123.0 and np.array_equal(blank.predict_batch(Xq[:3]), np.full(3, 123.0))
    assert blank.predict_with_uncertainty(Xq[0]) == (123.0, 0.0)
    np.random.seed(11)
    gq = GPQFunction(cfg)
    gq.fit(states, q)
    np.random.seed(11)                                        # the same inducing-point draw
    ref = SparseGP(SquaredExponentialARD(7, signal_variance=4.0, lengthscales=np.full(7, 2.0)),
                   n_inducing=min(50, len(states) // 2))
    ref.fit(states, q)
    pred = ref.predict(Xq)
    assert gq._gp.n_inducing == 50
    got = gq.predict_batch(Xq)
    assert np.array_equal(got, np.clip(pred.mean, 0.0, np.inf))
    assert gq.predict(Xq[1]) == got[1]
    m, v = gq.predict_with_uncertainty(Xq[1])
    assert m == pred.mean[1] and v == pred.variance[1] and v >= 0.0
    tight = GPQFunction(QFunctionConfig(gp_lengthscale=2.0, gp_variance=4.0, q_min=5.0, q_max=6.0))
    np.random.seed(11)
    tight.fit(states, q)
    assert np.array_equal(tight.predict_batch(Xq), np.clip(pred.mean, 5.0, 6.0))
    assert np.any(pred.mean < 5.0) or np.any(pred.mean > 6.0)
    man = QFunctionManager(ss, cfg)
    np.random.seed(11)
    assert np.array_equal(man.evaluate_batch(Xq), got) and isinstance(man._approximator, GPQFunction)


@pytest.mark.parametrize("name", SETS)
def test_q_functions_within_their_bounds(device_knn, name):
    g = golden("safeset.npz")
    check_q_functions(g, name, build_set(g, name), "device")


def test_k_max_past_the_kernel_takes_the_host_and_matches_scipy(device_knn):
    from gp_mpc_rocket_landing_amd.terminal import LocalSafeSet, LocalSafeSetConfig
    g = golden("safeset.npz")
    ss = build_set(g, "s7")
    ls = LocalSafeSet(ss, LocalSafeSetConfig(K=70, K_max=80, adaptive_K=False))
    x = g["s7_Xq"][1].astype(np.float64)
    nb, qv, dd = ls.query(x)
    assert ls.last_path == "host" and len(dd) == 70
    W = ss.get_all_states() * ls._weights
    want_d, want_i = KDTree(W).query(x * ls._weights, k=70)
    assert np.array_equal(dd, want_d) and np.array_equal(nb, ss.get_all_states()[want_i])
    assert np.array_equal(qv, ss.get_all_q_values()[want_i])
    # the same set within the kernel: the device, and the same first 64
    ls64 = LocalSafeSet(ss, LocalSafeSetConfig(K=64, K_max=64, adaptive_K=False))
    nb2, _, dd2 = ls64.query(x)
    assert ls64.last_path == "device" and np.array_equal(dd2, want_d[:64]) and np.array_equal(nb2, nb[:64])


def test_fewer_states_than_k_min_raise_on_the_device_too(device_knn):
    from gp_mpc_rocket_landing_amd.terminal import LocalSafeSet, SampledSafeSet
    X = golden("safeset.npz")["tiny_states"].astype(np.float64)
    ss = SampledSafeSet(n_x=7, n_u=3)
    ss.add_trajectory(X, np.zeros((2, 3)), np.ones(2))
    ls = LocalSafeSet(ss)
    with pytest.raises(IndexError):
        ls.query(X[1])
    assert ls.last_path == "device"
    with pytest.raises(IndexError):
        ls.interpolate_q_batch(X[:2])
    with pytest.raises(ValueError):
        ls.query(np.full(7, np.nan))
