"""gpmpc_knn_query / gpmpc_knn_interp on the device against the plain restatement of their
contract (tests/knn_check.py, pinned to scipy's KD-tree and to numpy in test_knn_check.py).
Indices, distance bits, ball counts and feasible counts are compared for equality, in both
summation orders.  The shapes are the smallest at which the kernels take another path: every
list length around k, the 64-row chunk, the workgroup's 256-row stride, the first split of the
rows (tests/test_knn_plan.py pins the part counts claimed here) and a ragged last part."""
import numpy as np
import pytest

import knn_check as kc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KS = [1, 4, 50, 64]
# k - 1, k, k + 1 of every k; the chunk; the workgroup stride; P = 1 | 2 at 1024 | 1025; P = 2 | 3 at
# 2048 | 2049 (the last part of 2049: 513 rows)
NS = [1, 2, 3, 4, 5, 49, 50, 51, 63, 64, 65, 255, 256, 257, 1024, 1025, 2048, 2049]
# the most parts the plan makes (P = 64: every single query over a large set), and 33 of them
BIG = [(65500, 7), (33000, 14)]


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


def _batches():
    q = _lib().KNN_Q
    return [1, q - 1, q, q + 1, 70]


def _same(got, want, tag):
    for g, w, name in zip(got, want, ("idx", "dist", "n_ball", "n_feasible")):
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:4])


def _prefix(want, B, k):
    return want[0][:B, :k], want[1][:B, :k], want[2][:B], want[3][:B]


@pytest.mark.parametrize("order", [kc.KD, kc.NP])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 7, 8, 14, 32])
def test_query_is_the_restatement(gpu_ctx, d, order):
    L = _lib()
    rng = np.random.default_rng(10 * d + order)
    X = rng.standard_normal((70, d))
    radius = 0.8 * np.sqrt(d)
    for n in NS:
        S = rng.standard_normal((n, d))
        X[7] = S[n // 2]                        # an exact hit at distance 0
        want = kc.knn_query(S, order, X, 64, radius)
        assert want[1][7, 0] == 0.0
        ks = L.KnnSet(gpu_ctx, S)
        for B in _batches():
            _same(ks.query(X[:B], 64, radius, order=order), _prefix(want, B, 64), (d, n, B, 64))
        for k in KS[:-1]:
            _same(ks.query(X[:5], k, radius, order=order), _prefix(want, 5, k), (d, n, 5, k))
        ks.close()


@pytest.mark.parametrize("order", [kc.KD, kc.NP])
@pytest.mark.parametrize("pattern", ["spread", "clustered", "duplicated"])
def test_many_parts_merge(gpu_ctx, pattern, order):
    """P = 64 and P = 33 lists through k_knn_merge: every column's bound on the answer's 64th
    entry and the gather of up to 64 x 64 survivors.  spread: the neighbours lie evenly over the
    parts (about one a part); clustered: all of them in one part, behind a far first part;
    duplicated: every row many times, so the bounds tie and nearly every entry survives."""
    rng = np.random.default_rng(91)
    for n, d in BIG:
        S = rng.standard_normal((n, d))
        X = rng.standard_normal((3, d)) * 0.3
        if pattern == "clustered":
            S += 4.0
            at = n // 2 + 100
            S[at:at + 200] = X[0] + 0.01 * rng.standard_normal((200, d))
        elif pattern == "duplicated":
            S = S[rng.integers(0, 40, n)]
        fuel = rng.permutation(n).astype(np.float64)
        avail = np.array([n, n // 3, 40.0])                       # all rows, a third of them, 41 rows
        want = kc.knn_query(S, order, X, 64, 1.5, fuel, avail)
        ks = _lib().KnnSet(gpu_ctx, S, fuel_req=fuel)
        for B in (1, 3):
            _same(ks.query(X[:B], 64, 1.5, avail[:B], order=order), _prefix(want, B, 64), (pattern, n, d, B))
        _same(ks.query(X[:1], 50, 1.5, order=order), kc.knn_query(S, order, X[:1], 50, 1.5), (pattern, n, d, "k50"))
        ks.close()


def _sorted_rows(rng, n, d, x, descending):
    S = x + rng.standard_normal((n, d))
    s2 = kc.sq_kd(S, x)
    o = np.argsort(s2)
    return S[o[::-1] if descending else o]


@pytest.mark.parametrize("order", [kc.KD, kc.NP])
@pytest.mark.parametrize("pattern", ["descending", "ascending"])
def test_every_row_inserts_or_none_after_the_first_k(gpu_ctx, pattern, order):
    rng = np.random.default_rng(77)
    for d, n in ((7, 700), (8, 2049)):
        x = rng.standard_normal(d)
        S = _sorted_rows(rng, n, d, x, pattern == "descending")
        X = np.repeat(x[None], 5, axis=0)
        X[1:] += 1e-3 * rng.standard_normal((4, d))
        want = kc.knn_query(S, order, X, 64, 1.5)
        ks = _lib().KnnSet(gpu_ctx, S)
        for B in (1, 5):
            _same(ks.query(X[:B], 64, 1.5, order=order), _prefix(want, B, 64), (pattern, d, n, B))
        ks.close()


@pytest.mark.parametrize("order", [kc.KD, kc.NP])
def test_duplicated_rows_go_to_the_lower_index(gpu_ctx, order):
    """scipy leaves the order of equal distances unspecified: the restatement alone is the oracle."""
    rng = np.random.default_rng(3)
    for d, n in ((7, 300), (4, 1300)):
        base = rng.standard_normal((n // 5, d))
        S = base[rng.integers(0, n // 5, n)]              # every row about five times
        X = rng.standard_normal((6, d))
        want = kc.knn_query(S, order, X, 64, 1.0)
        assert np.any(want[1][:, 1:] == want[1][:, :-1])
        ks = _lib().KnnSet(gpu_ctx, S)
        for B in (1, 6):
            _same(ks.query(X[:B], 64, 1.0, order=order), _prefix(want, B, 64), (d, n, B))
        ks.close()


@pytest.mark.parametrize("order", [kc.KD, kc.NP])
def test_a_row_exactly_at_the_radius_is_counted(gpu_ctx, order):
    """Small integer coordinates: every s^2 is an exact integer in either order, so the rows
    at s^2 = 25 lie exactly on the radius 5 (and tie, which the index order resolves)."""
    rng = np.random.default_rng(4)
    for d, n in ((3, 257), (7, 1100)):
        S = rng.integers(-4, 5, (n, d)).astype(np.float64)
        X = rng.integers(-2, 3, (5, d)).astype(np.float64)
        S[n - 1] = X[0]; S[n - 1, 0] += 3.0; S[n - 1, 1] += 4.0
        want = kc.knn_query(S, order, X, 50, 5.0)
        on = sum(int(np.sum(kc.sqdist(order, S, x) == 25.0)) for x in X)
        inside = sum(int(np.sum(kc.sqdist(order, S, x) < 25.0)) for x in X)
        assert on > 0 and want[2].sum() == on + inside
        ks = _lib().KnnSet(gpu_ctx, S)
        _same(ks.query(X, 50, 5.0, order=order), want, (d, n))
        ks.close()


@pytest.mark.parametrize("order", [kc.KD, kc.NP])
@pytest.mark.parametrize("k", [4, 50])
def test_fuel_filter_leaving_more_fewer_and_no_rows(gpu_ctx, k, order):
    rng = np.random.default_rng(5)
    for d, n in ((7, 257), (14, 1500)):
        S = rng.standard_normal((n, d))
        fuel = rng.permutation(n).astype(np.float64)
        X = rng.standard_normal((3, d))
        avail = np.array([k, k - 2, -1], np.float64)      # fuel <= avail: k + 1, k - 1 and 0 rows
        want = kc.knn_query(S, order, X, k, 2.0 * np.sqrt(d), fuel, avail)
        assert list(want[3]) == [k + 1, k - 1, 0]
        assert want[0][1, k - 1] == n and np.isinf(want[1][1, k - 1]) and np.all(want[0][2] == n)
        ks = _lib().KnnSet(gpu_ctx, S, fuel_req=fuel)
        _same(ks.query(X, k, 2.0 * np.sqrt(d), avail, order=order), want, (d, n, k))
        _same(ks.query(X[:1], k, 2.0 * np.sqrt(d), avail[:1], order=order), _prefix(want, 1, k), (d, n, k, 1))
        ks.close()


def _gamma(m):
    return m * U / (1.0 - m * U)


@pytest.mark.parametrize("adaptive", [False, True])
def test_interp_is_the_k_rule_and_the_weighted_mean(gpu_ctx, adaptive):
    """k_used is exact.  q_out: both sides form the same weights 1 / (d + 1e-10) from equal
    distances, then K - 1 additions for their sum, a division, a product and K - 1 additions
    of non-negative terms: 2K roundings a side, so each is within gamma(2K) of the exact
    value and the two within 2 gamma(2K) (1 + gamma(2K)), relative because q >= 0."""
    rng = np.random.default_rng(8)
    worst = 0.0
    for d, n in ((7, 300), (14, 1500), (3, 6)):
        S = rng.standard_normal((n, d))
        q = rng.random(n) * 100.0
        fuel = rng.permutation(n).astype(np.float64)
        X = rng.standard_normal((9, d)) * 0.5
        X[2] = S[n // 3]
        radius = 0.9 * np.sqrt(d)
        ks = _lib().KnnSet(gpu_ctx, S, q, fuel)
        for avail in (None, np.full(9, n // 2, np.float64), np.full(9, 2.0), np.full(9, -1.0)):
            want, used = kc.knn_interp(S, q, kc.KD, X, 10, 4, 50, adaptive, radius, fuel, avail)
            got, gused = ks.interp(X, 10, 4, 50, adaptive, radius, avail)
            assert np.array_equal(gused, used), (d, n, gused, used)
            fin = np.isfinite(want)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)],
                                                                                   want[~fin & ~np.isnan(want)])
            K = np.maximum(used[fin], 1)
            bound = 2 * _gamma(2 * K) * (1 + _gamma(2 * K))
            err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
            worst = max(worst, float(np.max(err / U, initial=0.0)))
            assert np.all(err <= bound), (d, n, err / U, bound / U)
            if avail is None:
                assert got[2] == q[n // 3]            # the exact hit returns its q
        ks.close()
    print("interp: max relative error", worst, "u; bound 4K u, K <= 50")


def test_refusals(gpu_ctx):
    L = _lib()
    S = np.random.default_rng(0).standard_normal((20, 3))
    ks = L.KnnSet(gpu_ctx, S)
    for k in (0, 65):
        with pytest.raises(L.HIPError) as e:
            ks.query(S[:2], k)
        assert e.value.rc == -2
    with pytest.raises(L.HIPError) as e:
        L.KnnSet(gpu_ctx, np.zeros((4, 33)))
    assert e.value.rc == -2
    with pytest.raises(L.HIPError) as e:
        ks.query(S[:2], 4, avail_fuel=np.ones(2))          # the set has no fuel_req
    assert e.value.rc == -2
    with pytest.raises(L.HIPError) as e:
        ks.interp(S[:2], 10, 4, 50, True, 1.0)             # the set has no q
    assert e.value.rc == -2
    bad = S[:2].copy(); bad[1, 1] = np.nan
    with pytest.raises(ValueError):
        ks.query(bad, 4)
    with pytest.raises(ValueError):
        ks.query(S[:2], 4, radius=np.inf)
    with pytest.raises(ValueError):
        L.KnnSet(gpu_ctx, bad)
    with pytest.raises(ValueError):
        ks.query(np.zeros((2, 4)), 4)
    assert ks.query(np.zeros((0, 3)), 4)[0].shape == (0, 4)
    ks.close()
