"""k-means for the inducing points without a GPU: the numpy restatement the GPU tests use as
their oracle (kmeans_check.lloyd) pinned to the installed scipy, the draw's use of the global
RNG, the argument checks of gpmpc_kmeans_lloyd (it refuses before any device call), the
guard constant, and SparseGP.optimize_inducing_locations on an unfitted model."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
from scipy.cluster.vq import kmeans2

import kmeans_check as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,d,k,seed", kc.TABLE)
def test_restatement_is_scipy_bit_for_bit(n, d, k, seed):
    """Pins scipy's algorithm and its draw: a scipy that changes either fails here."""
    X = kc.make_data(n, d, seed)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # none of these inputs empties a cluster
        C, label, idx = kc.scipy_points(X, k, seed)
    Cr, lr, empties, margin = kc.lloyd(X, X[idx])
    print(n, d, k, seed, "min margin", margin)
    assert np.array_equal(Cr, C) and np.array_equal(lr, label)
    assert not empties.any()
    assert margin >= kc.MIN_MARGIN


def test_restatement_keeps_empty_clusters_like_scipy():
    rng = np.random.RandomState(7)
    X = rng.randn(90, 11)
    C0 = X[rng.choice(90, 12, replace=False)]
    C0[3] += 50; C0[9] -= 80
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        C, label = kmeans2(X, C0, minit="matrix")
    assert len([x for x in w if "clusters is empty" in str(x.message)]) == 10
    Cr, lr, empties, margin = kc.lloyd(X, C0)
    assert np.array_equal(Cr, C) and np.array_equal(lr, label)
    assert np.array_equal(empties, [2] * 10)
    assert np.array_equal(Cr[[3, 9]], C0[[3, 9]])
    assert margin >= kc.MIN_MARGIN


@pytest.mark.parametrize("n,k,seed", [(300, 50, 1234), (4000, 2000, 3), (65, 64, 9)])
def test_the_draw_leaves_the_global_rng_where_kmeans2_does(n, k, seed):
    from gp_mpc_rocket_landing_amd.gp import kmeans as km
    X = kc.make_data(n, 3, seed)
    np.random.seed(seed)
    idx = km.draw_points(n, k)
    after_draw = np.random.get_state()
    np.random.seed(seed)
    C, _ = kmeans2(X, k, iter=1, minit="points")
    after_scipy = np.random.get_state()
    assert after_draw[0] == after_scipy[0] and np.array_equal(after_draw[1], after_scipy[1])
    assert after_draw[2:] == after_scipy[2:]
    # the same indices: with one iteration every drawn row is its own nearest centre
    np.random.seed(seed)
    assert np.array_equal(idx, np.random.choice(n, size=k, replace=False))


def _fake_ctx():
    return ctypes.create_string_buffer(256)   # never read: every call below is refused first


def test_kmeans_lloyd_refuses_bad_arguments():
    from gp_mpc_rocket_landing_amd import _lib
    f = _lib._L.gpmpc_kmeans_lloyd
    n, k, it = 6, 3, 2
    X = np.zeros((n, 33)); C0 = np.zeros((k, 33)); C = np.zeros((k, 33))
    lab = np.zeros(n, np.int32); emp = np.zeros(it, np.int32); mm = np.zeros(1); un = np.zeros(1, np.int32)
    ctx = _fake_ctx(); c = ctypes.addressof(ctx)
    d, i = _lib._d, _lib._i
    good = [c, d(X), n, 5, d(C0), k, it, d(C), i(lab), i(emp), d(mm), i(un)]
    for pos in (0, 1, 4, 7, 8, 9, 10, 11):       # every pointer, null
        a = list(good); a[pos] = None
        assert f(*a) == -2, pos
    for pos, bad in ((3, 0), (3, 33), (3, -1), (2, 0), (2, -4), (5, 0), (5, -1), (6, 0), (6, -3)):
        a = list(good); a[pos] = bad
        assert f(*a) == -2, (pos, bad)
    assert b"bad argument" in _lib._L.gpmpc_last_error()


def test_wrapper_refuses_non_finite_and_mismatched_input():
    from gp_mpc_rocket_landing_amd import _lib

    class NoCtx:
        h = None
    X = np.zeros((4, 3)); bad = X.copy(); bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        _lib.kmeans_lloyd(NoCtx, bad, X[:2])
    with pytest.raises(ValueError):
        _lib.kmeans_lloyd(NoCtx, X, bad[1:3])
    with pytest.raises(ValueError):
        _lib.kmeans_lloyd(NoCtx, X, np.array([[0.0, np.inf, 0.0]]))
    with pytest.raises(ValueError):
        _lib.kmeans_lloyd(NoCtx, X, np.zeros((2, 4)))


@pytest.mark.parametrize("d", [1, 13, 32])
def test_guard_constant(d):
    from gp_mpc_rocket_landing_amd import _lib
    assert _lib.kmeans_tau(d) == 16 * (d + 2) * 2.0 ** -53


def test_binding_constants_match_the_kernels():
    from gp_mpc_rocket_landing_amd import _lib
    src = open(os.path.join(REPO, "gp_mpc_rocket_landing_amd", "csrc", "kmeans.hip")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (KM_MAXD|KM_TILE|KM_OBS|KM_WAVES) (\d+)", src)}
    assert val == {"KM_MAXD": _lib.KMEANS_MAXD, "KM_TILE": _lib.KMEANS_TILE, "KM_OBS": _lib.KMEANS_OBS,
                   "KM_WAVES": _lib.KMEANS_WAVES}


def test_device_eligibility_and_switch(monkeypatch):
    from gp_mpc_rocket_landing_amd.gp import kmeans as km
    X = np.zeros((5, 3))
    assert km.device_eligible(X, 2)
    assert not km.device_eligible(X.astype(np.float32), 2)
    assert not km.device_eligible(np.zeros((5, 33)), 2)
    assert not km.device_eligible(np.full((5, 3), np.inf), 2)
    assert not km.device_eligible(X, 0) and not km.device_eligible(X, 2.0)
    monkeypatch.delenv("GPMPC_KMEANS", raising=False)
    assert km.mode() == "device"
    monkeypatch.setenv("GPMPC_KMEANS", "host")
    assert km.mode() == "host"
    monkeypatch.setenv("GPMPC_KMEANS", "gpu")
    with pytest.raises(ValueError):
        km.mode()


def test_host_switch_is_kmeans2_verbatim(monkeypatch):
    from gp_mpc_rocket_landing_amd.gp import SparseGP, SquaredExponentialARD
    monkeypatch.setenv("GPMPC_KMEANS", "host")
    X = kc.make_data(300, 11, 0)
    gp = SparseGP(SquaredExponentialARD(11), n_inducing=50)
    np.random.seed(5)
    Z = gp._initialize_inducing_points(X)
    state = np.random.get_state()
    np.random.seed(5)
    want, _ = kmeans2(X, 50, minit="points")
    assert np.array_equal(Z, want)
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]
    assert gp._initialize_inducing_points(X[:50]) is not X and np.array_equal(gp._initialize_inducing_points(X[:50]), X[:50])


def test_optimize_inducing_locations_on_an_unfitted_model():
    from gp_mpc_rocket_landing_amd.gp import SparseGP, SquaredExponentialARD
    gp = SparseGP(SquaredExponentialARD(3), n_inducing=5)
    assert gp.optimize_inducing_locations() == {"n_iterations": 0, "method": "kmeans"}
    assert gp.optimize_inducing_locations(n_iterations=3, learning_rate=0.1, verbose=True) == {
        "n_iterations": 0, "method": "kmeans"}
    assert gp.inducing_points is None and gp.X_train is None
