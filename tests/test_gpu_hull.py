"""gpmpc_hull_project / gpmpc_knn_hull on the device (csrc/hull.hip) and the Python
surface over them (terminal/convex_hull.py).

Validity is checked on every case from lambda alone in np.longdouble (tests/hull_check.py
``certificate``): status 0, lambda >= 0 exactly, |sum lambda - 1| <= 2 K 2^-53 and a relative gap
<= 2 tol at tol = 1e-12.  The factor 2: the kernel's fp64 evaluation of the gap differs from the
exact one for the same lambda by about (K + 2 d) 2^-52 max |w|^2 < 1e-13 max |w|^2.  Accuracy:
``proj`` against the exact answers (face enumeration for K <= 8, the closed forms of the simplex,
the cross-polytope and the segment), or against the restatement where none exists, within
hull_check.DEVICE_BOUND = 8 E (E measured on the CPU, header of hull_check.py).  The cases are
those tests/test_hull_check.py certifies on the CPU; layout and fusion are checked bit for bit."""
import numpy as np
import pytest

import hull_check as hc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


def _valid(out, b, V, x, tag):
    K = len(V)
    assert out["status"][b] == 0, (tag, out["status"][b], out["gap"][b], out["iters"][b])
    lam = out["lam"][b, :K]
    mn, sm, gap = hc.certificate(V, x, lam)
    assert mn >= 0.0 and sm <= 2 * K * U and gap <= 2 * hc.TOL, (tag, mn, sm, gap)
    assert np.all(out["lam"][b, K:] == 0.0)
    assert out["gap"][b] <= hc.TOL


def _same(a, b, tag, keys=("lam", "proj", "dist", "gap", "iters", "status", "qhull")):
    for k in keys:
        if a.get(k) is None and b.get(k) is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _rows(out, sel):
    return {k: (v[sel] if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("d", hc.DS)
def test_families_on_every_shape(gpu_ctx, d):
    """Interior, vertex, far and near queries, duplicated and identical vertices, the three
    magnitudes, for every K of the shape list; B = 1, Q - 1, Q, Q + 1 and 70."""
    L = _lib()
    for K in hc.ks_of(d):
        cases = hc.random_cases(d, K)
        Q = L.hull_plan(d, K, hc.BATCH)
        pick = [b % hc.DISTINCT for b in range(hc.BATCH)]
        V = np.stack([cases[c][1] for c in pick]); X = np.stack([cases[c][2] for c in pick])
        qv = np.cos(np.arange(hc.BATCH * K, dtype=float)).reshape(hc.BATCH, K)
        out = L.hull_project(gpu_ctx, V, X, qv)
        for b, (tag, Vb, xb) in enumerate(cases):
            _valid(out, b, Vb, xb, (d, K, tag))
            exact = hc.face_enum(Vb, xb) if K <= 8 else hc.wolfe(Vb, xb)["proj"]
            e = hc.rel_err(out["proj"][b], exact, Vb, xb)
            assert e <= hc.DEVICE_BOUND, (d, K, tag, e)
            mw = hc.max_w(Vb, xb)
            # dist = |p| summed over d terms; proj - x carries the rounding of proj = x + p
            assert (abs(out["dist"][b] - float(np.linalg.norm(out["proj"][b] - xb)))
                    <= (d + 4) * U * (mw + np.linalg.norm(xb))), (d, K, tag)
            assert abs(out["qhull"][b] - out["lam"][b] @ qv[b]) <= 2 * K * U * np.abs(qv[b]).max()
            if tag.startswith("vertex"):          # bit-equal to a vertex: the lowest such index
                i = int(np.nonzero(np.all(Vb == xb, axis=1))[0][0])
                assert out["dist"][b] == 0.0 and np.array_equal(out["lam"][b], np.eye(K)[i]), (d, K, tag)
                assert np.array_equal(out["proj"][b], xb)
        for b in range(hc.DISTINCT, hc.BATCH):   # the repeats: the same bits from another wave and workgroup
            _same(_rows(out, b), _rows(out, b % hc.DISTINCT), (d, K, b),
                  keys=("lam", "proj", "dist", "gap", "iters", "status"))
        for B in sorted({1, Q - 1, Q, Q + 1}):
            _same(L.hull_project(gpu_ctx, V[:B], X[:B], qv[:B]), _rows(out, slice(0, B)), (d, K, B))


@pytest.mark.parametrize("family", ["simplex", "cross", "segment", "trajectory"])
def test_sets_with_closed_forms_and_trajectories(gpu_ctx, family):
    L = _lib()
    cases = {"simplex": hc.simplex_cases, "cross": hc.cross_cases, "segment": hc.segment_cases,
             "trajectory": lambda: [c + (None,) for c in hc.trajectory_cases()]}[family]()
    for tag, V, x, exact in cases:
        out = L.hull_project(gpu_ctx, V, x[None])
        _valid(out, 0, V, x, tag)
        if exact is None:
            exact = hc.wolfe(V, x)["proj"]
        e = hc.rel_err(out["proj"][0], exact, V, x)
        assert e <= hc.DEVICE_BOUND, (tag, e)


def test_ragged_sets_and_shared_layout(gpu_ctx):
    """nv covers 0, 1 and K with the unused rows NaN: the results of the trimmed sets, bit for
    bit; one shared set equals the same set replicated."""
    L = _lib()
    for d, K in hc.RAGGED:
        V, qv, X, nv = hc.ragged_sets(d, K)
        B = len(nv)
        Vn, qn = V.copy(), qv.copy()
        for b in range(B):
            Vn[b, nv[b]:] = np.nan
            qn[b, nv[b]:] = np.nan
        out = L.hull_project(gpu_ctx, Vn, X, qn, nv)
        for b in range(B):
            k = int(nv[b])
            if k == 0:
                assert out["status"][b] == 2 and out["dist"][b] == np.inf and np.array_equal(out["proj"][b], X[b])
                assert np.all(out["lam"][b] == 0.0) and out["iters"][b] == 0 and out["qhull"][b] == np.inf
                continue
            one = L.hull_project(gpu_ctx, V[b:b + 1, :k], X[b:b + 1], qv[b:b + 1, :k])
            assert np.array_equal(out["lam"][b, :k], one["lam"][0]) and np.all(out["lam"][b, k:] == 0.0)
            _same(_rows(out, b), _rows(one, 0), (d, K, b), keys=("proj", "dist", "gap", "iters", "status", "qhull"))
            _valid(one, 0, V[b, :k], X[b], (d, K, b))
        shared = L.hull_project(gpu_ctx, V[0], X, qv[0])
        _same(shared, L.hull_project(gpu_ctx, np.broadcast_to(V[0], (B, K, d)), X, np.broadcast_to(qv[0], (B, K))),
              (d, K, "shared"))


def test_cycle_cap_and_non_finite_input(gpu_ctx):
    L = _lib()
    V, X = hc.cap_case()
    K, d = V.shape
    out = L.hull_project(gpu_ctx, V, X, max_iter=1)
    for b in range(2):
        assert out["status"][b] == 1 and out["iters"][b] == 1 and out["gap"][b] > hc.TOL
        mn, sm, gap = hc.certificate(V, X[b], out["lam"][b])
        assert mn >= 0.0 and sm <= 2 * K * U and gap > hc.TOL
    full = L.hull_project(gpu_ctx, V, X)
    assert np.all(full["status"] == 0) and np.all(full["iters"] > 1)
    # a NaN and an inf, in x and in a used vertex: status 3 for that query only
    B = 6
    Vb = np.broadcast_to(V, (B, K, d)).copy(); Xb = np.broadcast_to(X[0], (B, d)).copy()
    nv = np.full(B, K); nv[5] = 4
    Xb[1, 2] = np.nan; Xb[2, 0] = np.inf; Vb[3, 7, 1] = np.nan; Vb[4, 0, 4] = -np.inf
    Vb[5, 6, 0] = np.nan                         # past nv[5]: not used
    out = L.hull_project(gpu_ctx, Vb, Xb, nv=nv)
    assert np.array_equal(out["status"], [0, 3, 3, 3, 3, 0])
    for b in (1, 2, 3, 4):
        assert np.all(np.isnan(out["proj"][b])) and np.isnan(out["dist"][b]) and np.isnan(out["gap"][b])
        assert np.all(np.isnan(out["lam"][b]))
    _same(_rows(out, 0), _rows(full, 0), "clean row")
    _valid(out, 5, V[:4], X[0], "ragged beside NaN")


def _safe_set(n_traj=6):
    from gp_mpc_rocket_landing_amd.terminal import FuelAwareSafeSet
    S, _ = hc.trajectory_set(n_traj=n_traj)
    ss = FuelAwareSafeSet(n_x=7, n_u=3)
    steps = 40
    for j in range(len(S) // steps):
        X = S[j * steps:(j + 1) * steps]
        ss.add_trajectory(X, np.zeros((steps - 1, 3)), np.ones(steps - 1))
    return ss


def _host_k_rule(n_ball, n_avail, k_base, k_min, k_max, adaptive):
    if n_avail == 0:
        return 0
    K = k_base
    if adaptive:
        K = int(k_base * (1 + (n_ball / n_avail) * 2))
        K = int(np.clip(K, k_min, k_max))
    K = min(max(min(K, n_avail), k_min), k_max)
    return -1 if K > n_avail else K


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("with_fuel", [False, True])
def test_fused_call_is_query_rule_and_projection(gpu_ctx, order, with_fuel):
    """gpmpc_knn_hull = gpmpc_knn_query + the K rule on the host + gpmpc_hull_project on the
    gathered rows, bit for bit; a wholly infeasible query (status 2) and one with fewer rows than
    k_min (k_used -1) among them."""
    L = _lib()
    S, q = hc.trajectory_set()
    n = len(S)
    rng = np.random.default_rng(20 + order)
    w = np.sqrt(np.array([0.1, 1, 1, 1, 0.5, 0.5, 0.5]))
    fuel_req = np.sort(rng.random(n)) * 10.0
    ks = L.KnnSet(gpu_ctx, S * w, q, fuel_req)
    ks.set_points(S)
    B = 70
    Xp = S[rng.integers(n, size=B)] + 0.4 * rng.standard_normal((B, 7))
    Xq = Xp * w
    avail = None
    if with_fuel:
        avail = rng.random(B) * 10.0 + 1.0
        avail[3] = -1.0                      # no feasible row
        avail[5] = fuel_req[1]               # two feasible rows: fewer than k_min = 4
    for k_base, k_min, k_max, adaptive, radius in ((10, 4, 50, 1, 2.0), (7, 4, 64, 0, 1.0)):
        idx, dist, n_ball, n_feas = ks.query(Xq, 64, radius, avail, order=order)
        used = np.array([_host_k_rule(int(n_ball[b]), int(n_feas[b]), k_base, k_min, k_max, adaptive) for b in range(B)])
        if with_fuel:
            assert used[3] == 0 and used[5] == -1
        got = ks.hull(Xq, Xp, k_base, k_min, k_max, adaptive, radius, avail, order=order)
        assert np.array_equal(got["k_used"], used)
        nv = np.maximum(used, 0)
        V = np.full((B, k_max, 7), np.nan); Q = np.full((B, k_max), np.nan)
        for b in range(B):
            V[b, :nv[b]] = S[idx[b, :nv[b]]]
            Q[b, :nv[b]] = q[idx[b, :nv[b]]]
            assert np.array_equal(got["idx"][b, :nv[b]], idx[b, :nv[b]]) and np.all(got["idx"][b, nv[b]:] == n)
        want = L.hull_project(gpu_ctx, V, Xp, Q, nv)
        _same(got, want, (order, with_fuel, k_base))
        assert np.all(got["status"][nv > 0] == 0) and np.all(got["status"][nv == 0] == 2)
    ks.close()


def test_fused_call_on_a_set_without_q(gpu_ctx):
    """A set created without q: the fused call stages no qhull.  The vertex rows and the K rule
    against the restatement of the search (tests/knn_check.py), the projection certified from
    lambda alone and held to the restatement's, on two of the trajectory cases."""
    import knn_check as kc
    L = _lib()
    S, _ = hc.trajectory_set()
    n, K = len(S), 10
    X = np.stack([x for _, _, x in hc.trajectory_cases(K)[:2]])
    ks = L.KnnSet(gpu_ctx, S)
    ks.set_points(S)
    got = ks.hull(X, X, K, 4, K, 0, 1.0)
    ks.close()
    assert got["qhull"] is None
    idx, _, n_ball, n_feas = kc.knn_query(S, kc.KD, X, K, 1.0)
    for b in range(2):
        assert got["k_used"][b] == _host_k_rule(int(n_ball[b]), int(n_feas[b]), K, 4, K, 0) == K
        assert np.array_equal(got["idx"][b], idx[b])
        V = S[idx[b]]
        _valid(got, b, V, X[b], ("no q", b))
        e = hc.rel_err(got["proj"][b], hc.wolfe(V, X[b])["proj"], V, X[b])
        assert e <= hc.DEVICE_BOUND, (b, e)


def test_constraint_single_calls_are_rows_of_the_batch(gpu_ctx):
    from gp_mpc_rocket_landing_amd.terminal import ConvexHullConstraint
    rng = np.random.default_rng(4)
    V = rng.standard_normal((12, 3)); qv = rng.standard_normal(12)
    ch = ConvexHullConstraint(V, qv)
    X = np.concatenate([rng.dirichlet(np.ones(12), size=4) @ V, 3.0 * rng.standard_normal((4, 3)), V[2:3]])
    Xp, Lam = ch.project_batch(X)
    inside = ch.contains_batch(X)
    assert list(inside) == [True] * 4 + [False] * 4 + [True]
    for b, x in enumerate(X):
        xp, lam = ch.project_onto_hull(x)
        assert np.array_equal(xp, Xp[b]) and np.array_equal(lam, Lam[b])
        assert np.array_equal(xp, V.T @ lam)
        assert ch.check_feasibility(x) == inside[b]
        assert ch.get_interpolated_q(lam) == float(np.dot(lam, qv))
        exact = hc.wolfe(V, x)["proj"]
        assert hc.rel_err(xp, exact, V, x) <= hc.DEVICE_BOUND + 4 * 12 * U


def test_manager_agrees_on_both_settings_of_the_switch(gpu_ctx, monkeypatch):
    """TerminalSetManager.project_batch: the fused device call and the host k-NN followed by
    gpmpc_hull_project see the same vertices and return the same bits."""
    from gp_mpc_rocket_landing_amd.terminal import TerminalSetManager
    ss = _safe_set()
    S = ss.get_all_states()
    rng = np.random.default_rng(8)
    X = S[rng.integers(len(S), size=20)] + 0.3 * rng.standard_normal((20, 7))
    X[4] = S[17]
    res = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("GPMPC_KNN", mode)
        tm = TerminalSetManager(ss)
        for fuel in (None, 1e9):
            res[mode, fuel] = tm.project_batch(X, fuel)
            assert tm.last_path == mode
        res[mode, "in"] = tm.is_in_terminal_set_batch(X)
        one = [tm.is_in_terminal_set(x) for x in X[:6]]
        assert one == list(res[mode, "in"][:6])
    for fuel in (None, 1e9):
        a, b = res["device", fuel], res["host", fuel]
        for k in ("idx", "k_used", "lam", "proj", "dist", "q", "status"):
            assert np.array_equal(a[k], b[k]), (fuel, k)
        assert np.all(a["status"] == 0) and np.all(a["k_used"] >= 4)
    assert np.array_equal(res["device", "in"], res["host", "in"]) and res["device", "in"][4]
    # three landings: with fuel for their last states alone, three feasible rows < K_min = 4
    thin = _safe_set(n_traj=3)
    assert int(np.sum(thin.get_fuel_required() <= 0.1000001)) == 3
    for mode in ("device", "host"):
        monkeypatch.setenv("GPMPC_KNN", mode)
        with pytest.raises(IndexError):
            TerminalSetManager(thin).project_batch(X[:3], 0.1000001)
        out = TerminalSetManager(thin).project_batch(X[:3], 0.0)      # no feasible row at all
        assert np.array_equal(out["status"], [2, 2, 2]) and np.all(np.isinf(out["q"]))
