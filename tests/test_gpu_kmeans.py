"""gpmpc_kmeans_lloyd and gp.kmeans.kmeans2_points on the device against scipy's kmeans2, for
equal bits: code book and labels.

Every case that expects the device's result first asserts that the numpy restatement's
smallest margin (kmeans_check.lloyd, pinned to scipy in test_kmeans_host.py) is >= 1e-9, far
above the guard's tau ~ 1e-14, and that the device reported unsafe == 0 / last_path ==
"device": a silent hand-back to scipy cannot pass for parity."""
import warnings

import numpy as np
import pytest
from scipy.cluster.vq import kmeans2

import kmeans_check as kc

pytestmark = pytest.mark.gpu

# widths 1 and 32, n on both sides of a multiple of the assign kernel's 64 observations a
# workgroup (257, 513, 130, 65), k on both sides of its 128-centre LDS tile (129, 130), k = n - 1;
# k = 9 and 13 leave waves of the workgroup's eight with one centre or none, k = 1 (below) seven;
# seeds 10-13 as drawn, none had a margin below 1e-9
EDGE = [(257, 1, 9, 10), (513, 32, 130, 11), (130, 8, 129, 12), (65, 2, 64, 13)]


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


def _quiet_scipy(X, k, seed, iters=10):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return kc.scipy_points(X, k, seed, iters)


@pytest.mark.parametrize("n,d,k,seed", kc.TABLE + EDGE)
def test_device_is_scipy_bit_for_bit(gpu_ctx, n, d, k, seed):
    lib = _lib()
    assert lib.KMEANS_OBS == 64 and lib.KMEANS_TILE == 128   # what EDGE straddles
    X = kc.make_data(n, d, seed)
    want_C, want_l, idx = _quiet_scipy(X, k, seed)
    Cr, lr, er, margin = kc.lloyd(X, X[idx])
    assert margin >= kc.MIN_MARGIN
    C, label, empties, dev_margin, unsafe = lib.kmeans_lloyd(gpu_ctx, X, X[idx])
    print(n, d, k, seed, "margin: restatement", margin, "device", dev_margin, "unsafe", unsafe)
    assert unsafe == 0
    assert label.dtype == np.int64 and label.shape == (n,) and C.shape == (k, d)
    assert np.array_equal(label, want_l)
    assert np.array_equal(C, want_C), np.max(np.abs(C - want_C))
    assert np.array_equal(empties, er)
    # the two margins are the same quantity up to the rounding of a distance
    assert abs(dev_margin - margin) <= 1e-12


@pytest.mark.parametrize("iters", [1, 3])
def test_iteration_count(gpu_ctx, iters):
    n, d, k, seed = kc.TABLE[0]
    X = kc.make_data(n, d, seed)
    want_C, want_l, idx = _quiet_scipy(X, k, seed, iters)
    assert kc.lloyd(X, X[idx], iters)[3] >= kc.MIN_MARGIN
    C, label, empties, _, unsafe = _lib().kmeans_lloyd(gpu_ctx, X, X[idx], iters=iters)
    assert unsafe == 0 and empties.shape == (iters,)
    assert np.array_equal(label, want_l) and np.array_equal(C, want_C)


def _empty_case():
    rng = np.random.RandomState(7)
    X = rng.randn(90, 11)
    C0 = X[rng.choice(90, 12, replace=False)]
    C0[3] += 50; C0[9] -= 80
    return X, C0


def test_empty_clusters_keep_their_rows(gpu_ctx):
    X, C0 = _empty_case()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        want_C, want_l = kmeans2(X, C0, minit="matrix")
    assert len([x for x in w if "clusters is empty" in str(x.message)]) == 10
    assert kc.lloyd(X, C0)[3] >= kc.MIN_MARGIN
    C, label, empties, margin, unsafe = _lib().kmeans_lloyd(gpu_ctx, X, C0)
    print("margin", margin)
    assert unsafe == 0
    assert np.array_equal(empties, [2] * 10)
    assert np.array_equal(label, want_l) and np.array_equal(C, want_C)
    assert np.array_equal(C[[3, 9]], C0[[3, 9]])


def test_more_centres_than_observations(gpu_ctx):
    """k > n (scipy's minit="matrix" takes it): the centres beyond the data stay empty."""
    X = kc.make_data(7, 3, 21)
    C0 = np.vstack([X + 0.01, X[:4] + 40.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_C, want_l = kmeans2(X, C0, minit="matrix")
    assert kc.lloyd(X, C0)[3] >= kc.MIN_MARGIN
    C, label, empties, _, unsafe = _lib().kmeans_lloyd(gpu_ctx, X, C0)
    assert unsafe == 0 and np.array_equal(empties, [4] * 10)
    assert np.array_equal(label, want_l) and np.array_equal(C, want_C)


def test_the_guard_fires_on_exact_ties(gpu_ctx):
    X, _ = _empty_case()
    Xd = np.vstack([X, X[:20]])
    C0 = np.vstack([X[:6], X[:6]])   # duplicate centres: every first decision is a tie
    _, _, _, margin, unsafe = _lib().kmeans_lloyd(gpu_ctx, Xd, C0)
    assert unsafe > 0 and margin == 0.0
    # all-zero data: the scale is 0, every decision unsafe
    _, _, _, margin, unsafe = _lib().kmeans_lloyd(gpu_ctx, np.zeros((5, 2)), np.zeros((1, 2)), iters=2)
    assert unsafe == 10 and margin == 0.0
    # a single centre away from zero has no second nearest: nothing to get wrong
    C, label, _, margin, unsafe = _lib().kmeans_lloyd(gpu_ctx, X, X[:1], iters=2)
    assert unsafe == 0 and margin == np.inf and not label.any()


def test_wrapper_hands_a_tied_draw_to_scipy(gpu_ctx):
    """Rows 40-59 repeat rows 0-19; under seed 8 (found by a search over seeds on the host)
    the draw of 12 picks both copies of a row, two equal centres: exact ties, the guard fires."""
    from gp_mpc_rocket_landing_amd.gp import kmeans as km
    base = kc.make_data(40, 5, 20)
    X = np.vstack([base, base[:20]])
    np.random.seed(8)
    idx = km.draw_points(60, 12)
    assert len({tuple(X[i]) for i in idx}) < 12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(8)
        want_C, want_l = kmeans2(X, 12, minit="points")
        want_state = np.random.get_state()
        np.random.seed(8)
        C, label = km.kmeans2_points(X, 12)
    assert km.kmeans2_points.last_path == "host"
    assert np.array_equal(C, want_C) and np.array_equal(label, want_l)
    assert np.array_equal(np.random.get_state()[1], want_state[1])


def test_wrapper_warns_once_per_iteration_with_an_empty_cluster(gpu_ctx):
    """60 x 1 -> 45 centres under seed 104 (found by a search over seeds on the host): from the
    third iteration on one cluster is empty, margin 1.5e-6."""
    from gp_mpc_rocket_landing_amd.gp import kmeans as km
    X = kc.make_data(60, 1, 104)
    np.random.seed(104)
    _, _, want_empty, margin = kc.lloyd(X, X[km.draw_points(60, 45)])
    assert margin >= kc.MIN_MARGIN and np.array_equal(want_empty, [0, 0] + [1] * 8)
    with warnings.catch_warnings(record=True) as ws:
        warnings.simplefilter("always")
        np.random.seed(104)
        want_C, want_l = kmeans2(X, 45, minit="points")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        np.random.seed(104)
        C, label = km.kmeans2_points(X, 45)
    assert km.kmeans2_points.last_path == "device"
    assert np.array_equal(C, want_C) and np.array_equal(label, want_l) and label.dtype == want_l.dtype
    assert [(str(x.message), x.category) for x in w] == [(str(x.message), x.category) for x in ws]
    assert len(w) == 8 and str(w[0].message) == km.EMPTY_WARNING


def test_sparse_gp_surface(gpu_ctx, monkeypatch):
    from gp_mpc_rocket_landing_amd.gp import MultiOutputSparseGP, SparseGP, SquaredExponentialARD
    from gp_mpc_rocket_landing_amd.gp import kmeans as km
    X = kc.make_data(300, 11, 30)
    Y = np.stack([np.sin(X[:, 0]), X[:, 1] * 0.3, np.cos(X[:, 2])], axis=1)
    np.random.seed(1234)
    assert kc.lloyd(X, X[km.draw_points(300, 50)])[3] >= kc.MIN_MARGIN

    def fit(mode):
        monkeypatch.setenv("GPMPC_KMEANS", mode)
        km.kmeans2_points.last_path = None
        np.random.seed(1234)
        m = MultiOutputSparseGP(11, 3, n_inducing=50).fit(X, Y)
        return m, np.random.get_state()
    host, host_state = fit("host")
    assert km.kmeans2_points.last_path is None
    dev, dev_state = fit("device")
    assert km.kmeans2_points.last_path == "device"
    assert np.array_equal(dev.gps[0].inducing_points, host.gps[0].inducing_points)
    assert np.array_equal(dev_state[1], host_state[1]) and dev_state[2:] == host_state[2:]
    np.random.seed(1234)
    assert np.array_equal(dev.gps[0].inducing_points, kmeans2(X, 50, minit="points")[0])

    gp = SparseGP(SquaredExponentialARD(11), n_inducing=50).fit(X, Y[:, 0])
    np.random.seed(77)
    assert kc.lloyd(X, X[km.draw_points(300, 50)])[3] >= kc.MIN_MARGIN
    np.random.seed(77)
    km.kmeans2_points.last_path = None
    assert gp.optimize_inducing_locations() == {"n_iterations": 0, "method": "kmeans"}
    assert km.kmeans2_points.last_path == "device"
    np.random.seed(77)
    assert np.array_equal(gp.inducing_points, kmeans2(X, 50, minit="points")[0])
    pred = gp.predict(X[:7])
    assert np.all(np.isfinite(pred.mean)) and np.all(pred.variance >= 0)


def test_production_shape(gpu_ctx):
    """BASELINE configs[4]: 4000 x 13 -> 2000 centres.  The restatement takes seconds here, so
    the margin comes from kmeans_check.margin_expanded (the same quantity to ~1e-15)."""
    n, d, k, seed = kc.PRODUCTION
    X = kc.make_data(n, d, seed)
    want_C, want_l, idx = _quiet_scipy(X, k, seed)
    assert kc.margin_expanded(X, X[idx]) >= kc.MIN_MARGIN
    C, label, empties, margin, unsafe = _lib().kmeans_lloyd(gpu_ctx, X, X[idx])
    print("device margin", margin, "empties", empties)
    assert unsafe == 0 and margin >= kc.MIN_MARGIN
    assert np.array_equal(label, want_l) and np.array_equal(C, want_C)
