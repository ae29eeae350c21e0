"""The oracles of the device hull test (tests/hull_check.py) against each other, on the CPU:
the restatement of the contract matches every exact answer to E, it certifies every case the
device test runs (so no device case may end "not certified"), and the ``convex_tol`` membership
rule agrees with scipy's Delaunay triangulation where that is defined."""
import numpy as np
import pytest

import hull_check as hc


def _all_random():
    for d in hc.DS:
        for K in hc.ks_of(d):
            for tag, V, x in hc.random_cases(d, K):
                yield d, K, tag, V, x


def test_restatement_certifies_every_device_case():
    """Status 0, lambda a convex combination, the longdouble gap <= 2 tol: a condition on the
    cases, not a measurement."""
    worst_it = 0
    special = [(t, V, x) for t, V, x, _ in hc.simplex_cases() + hc.cross_cases() + hc.segment_cases()]
    ragged = []
    for d, K in hc.RAGGED:
        V, _, X, nv = hc.ragged_sets(d, K)
        ragged += [("ragged", V[b, :nv[b]], X[b]) for b in range(len(nv)) if nv[b]]
    Vc, Xc = hc.cap_case()
    ragged += [("cap", Vc, Xc[0]), ("cap", Vc, Xc[1]), ("cap", Vc[:4], Xc[0])]
    everything = ([(tag, V, x) for _, _, tag, V, x in _all_random()] + special + hc.trajectory_cases()
                  + hc.trajectory_cases(K=50, n_queries=6) + hc.trajectory_cases(K=4, n_queries=6) + ragged)
    for tag, V, x in everything:
        r = hc.wolfe(V, x)
        K = len(V)
        assert r["status"] == 0, (tag, V.shape, r["status"], r["gap"], r["iters"])
        mn, sm, gap = hc.certificate(V, x, r["lam"])
        assert mn >= 0.0 and sm <= 2 * K * 2.0 ** -53 and gap <= 2 * hc.TOL, (tag, V.shape, mn, sm, gap)
        worst_it = max(worst_it, r["iters"])
    print("cases", len(everything), "most cycles", worst_it)
    assert worst_it < hc.MAX_ITER // 8


def test_restatement_matches_the_exact_answers():
    """E per family (the figures in the header of hull_check.py).  Held to 2 E_MEASURED, not to
    E_MEASURED itself: the last digit of a figure is not promised across numpy builds."""
    E = {}
    for d, K, tag, V, x in _all_random():
        if K <= 8:
            e = hc.rel_err(hc.wolfe(V, x)["proj"], hc.face_enum(V, x), V, x)
            E["face"] = max(E.get("face", 0.0), e)
    for fam, cases in (("simplex", hc.simplex_cases()), ("cross", hc.cross_cases()), ("segment", hc.segment_cases())):
        for tag, V, x, exact in cases:
            E[fam] = max(E.get(fam, 0.0), hc.rel_err(hc.wolfe(V, x)["proj"], exact, V, x))
    print("E per family", E)
    assert set(E) == {"face", "simplex", "cross", "segment"}
    assert max(E.values()) <= 2 * hc.E_MEASURED, E


def test_exact_answers_agree_where_two_apply():
    """Face enumeration against the closed forms on small instances of their sets."""
    rng = np.random.default_rng(3)
    for d in (2, 3, 4):
        x = rng.standard_normal(d) * 2
        V = 1.5 * np.eye(d)
        assert float(np.max(np.abs(hc.face_enum(V, x) - hc.simplex_answer(x, 1.5)))) < 1e-17 * 100
        V = np.concatenate([np.eye(d), -np.eye(d)])
        assert float(np.max(np.abs(hc.face_enum(V, x) - hc.cross_answer(x, 1.0)))) < 1e-17 * 100
    for tag, V, x, exact in hc.segment_cases()[:3]:
        assert float(np.max(np.abs(hc.face_enum(V, x) - exact))) < 1e-17 * 100


def test_statuses_of_the_restatement():
    V = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    r = hc.wolfe(np.zeros((0, 2)), np.array([1.0, 2.0]))
    assert r["status"] == 2 and r["dist"] == np.inf and np.array_equal(r["proj"], [1.0, 2.0])
    for bad in (np.nan, np.inf):
        assert hc.wolfe(V, np.array([bad, 0.0]))["status"] == 3
        Vb = V.copy(); Vb[1, 1] = bad
        assert hc.wolfe(Vb, np.array([0.2, 0.2]))["status"] == 3
    r = hc.wolfe(V, np.array([2.0, 2.0]), max_iter=1)
    assert r["status"] == 1 and r["gap"] > hc.TOL and r["iters"] == 1
    assert np.all(r["lam"] >= 0) and abs(r["lam"].sum() - 1.0) == 0.0
    Vc, Xc = hc.cap_case()                      # the device test's cap cases: one cycle is not enough
    for x in Xc:
        r = hc.wolfe(Vc, x, max_iter=1)
        assert r["status"] == 1 and r["gap"] > hc.TOL and r["iters"] == 1 and hc.wolfe(Vc, x)["iters"] >= 3
    r = hc.wolfe(V, V[2].copy(), q=np.array([1.0, 2.0, 3.0]))
    assert r["status"] == 0 and r["dist"] == 0.0 and np.array_equal(r["lam"], [0.0, 0.0, 1.0]) and r["qhull"] == 3.0


def test_convex_tol_rule_agrees_with_delaunay():
    """Full-dimensional sets, interior points as Dirichlet combinations, exterior points at a
    clear margin: dist <= convex_tol (1e-6, the reference's default) answers as find_simplex."""
    from scipy.spatial import Delaunay
    cases = hc.membership_cases()
    tri = {}
    for V, x, inside in cases:
        key = id(V)
        if key not in tri:
            tri[key] = Delaunay(V) if V.shape[1] > 1 else None
        r = hc.wolfe(V, x)
        assert r["status"] == 0
        rule = r["dist"] <= 1e-6
        if tri[key] is not None:
            assert bool(tri[key].find_simplex(x) >= 0) == rule, (V.shape, inside, r["dist"])
        else:
            assert (V.min() <= x[0] <= V.max()) == rule
        assert rule == inside, (V.shape, r["dist"])
    assert len(cases) >= 80
