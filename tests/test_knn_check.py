"""tests/knn_check.py, the oracle of the device k-nearest-neighbour tests, pinned to what it
restates: scipy.spatial.KDTree (query, query_ball_point) for the KD order, np.linalg.norm for
numpy's.  Every comparison is for equal bits."""
import numpy as np
import pytest
from scipy.spatial import KDTree

import knn_check as kc

DS = [1, 3, 4, 5, 7, 8, 14, 17, 32]
NS = [1, 5, 16, 17, 300]


def _data(d, n, nq=12):
    rng = np.random.default_rng(100 * d + n)
    S = rng.standard_normal((n, d))
    X = rng.standard_normal((nq, d))
    X[0] = S[n // 2]                       # an exact hit
    return S, X


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_kd_order_is_the_kd_trees_bits(d, n):
    S, X = _data(d, n)
    tree = KDTree(S)
    radius = float(np.sqrt(d)) * 0.9
    for k in sorted({1, min(n, 50), n + 3}):       # the last: k > n, scipy pads with inf / n
        idx, dist, nb, nf = kc.knn_query(S, kc.KD, X, k, radius)
        for b, x in enumerate(X):
            dd, ii = tree.query(x, k=k)
            dd, ii = np.atleast_1d(dd), np.atleast_1d(ii)
            assert np.array_equal(ii, idx[b]), (d, n, k, b)
            assert np.array_equal(dd, dist[b]), (d, n, k, b)
            assert len(tree.query_ball_point(x, radius)) == nb[b], (d, n, b)
            assert nf[b] == n


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_numpy_order_is_linalg_norm(d, n):
    S, X = _data(d, n)
    for x in X:
        assert np.array_equal(np.sqrt(kc.sq_np(S, x)), np.linalg.norm(S - x, axis=1)), (d, n)
    k = min(n, 10)
    idx, dist, _, _ = kc.knn_query(S, kc.NP, X, k)
    for b, x in enumerate(X):
        dn = np.linalg.norm(S - x, axis=1)
        order = np.lexsort((np.arange(n), dn))[:k]
        assert np.array_equal(idx[b], order) and np.array_equal(dist[b], dn[order])
        assert idx[b, 0] == np.argmin(dn)        # the exact-match branch's lowest index


def test_ties_go_to_the_lower_index_and_the_radius_row_counts():
    rng = np.random.default_rng(5)
    S = rng.standard_normal((40, 7))
    S[25] = S[3]; S[11] = S[3]                    # three copies of one row
    x = S[3] + 0.25
    idx, dist, _, _ = kc.knn_query(S, kc.KD, x[None], 40)
    p = [int(np.nonzero(idx[0] == r)[0][0]) for r in (3, 11, 25)]
    assert p[1] == p[0] + 1 and p[2] == p[0] + 2 and dist[0, p[0]] == dist[0, p[2]]
    # a row exactly at the radius: float32-representable offsets make s^2 and r * r exact
    S2 = np.zeros((3, 4)); S2[0, 0] = 3.0; S2[1, 1] = 3.0 + 2.0 ** -20; S2[2, 2] = 3.0 - 2.0 ** -20
    _, _, nb, _ = kc.knn_query(S2, kc.KD, np.zeros((1, 4)), 1, radius=3.0)
    assert nb[0] == 2 == len(KDTree(S2).query_ball_point(np.zeros(4), 3.0))


def test_fuel_filter_counts_and_pads():
    rng = np.random.default_rng(6)
    S = rng.standard_normal((30, 5)); fuel = np.arange(30.0)
    X = rng.standard_normal((3, 5))
    idx, dist, nb, nf = kc.knn_query(S, kc.KD, X, 8, 10.0, fuel, np.array([4.0, 7.0, -1.0]))
    assert list(nf) == [5, 8, 0] and list(nb) == [5, 8, 0]
    assert np.all(idx[0, :5] < 5) and np.all(idx[0, 5:] == 30) and np.all(np.isinf(dist[0, 5:]))
    assert np.all(idx[2] == 30)
    sub = KDTree(S[:8])
    dd, ii = sub.query(X[1], k=8)
    assert np.array_equal(ii, idx[1]) and np.array_equal(dd, dist[1])   # positions in the full set


def test_k_rule_follows_the_reference_order():
    assert kc.k_rule(10, 4, 50, False, 0, 1000) == 10
    assert kc.k_rule(10, 4, 50, True, 500, 1000) == 20
    assert kc.k_rule(10, 4, 50, True, 1000, 1000) == 30
    assert kc.k_rule(30, 4, 50, True, 1000, 1000) == 50
    assert kc.k_rule(10, 4, 50, False, 0, 3) == 4           # fewer rows than K_min: K_min (the caller raises)
    assert kc.k_rule(1, 0, 50, False, 0, 7) == 1
    q = np.arange(6.0)
    S = np.arange(6.0)[:, None] * np.ones((1, 3))
    out, used = kc.knn_interp(S, q, kc.KD, S[2:3], 3, 1, 5, False, 1.0)
    assert out[0] == 2.0 and used[0] == 3                    # exact hit
    out, used = kc.knn_interp(S, q, kc.KD, S[2:3] + 0.5, 2, 1, 5, False, 1.0)
    assert used[0] == 2 and abs(out[0] - 2.5) < 1e-9
