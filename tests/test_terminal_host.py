"""gp_mpc_rocket_landing_amd.terminal on the host path (GPMPC_KNN=host: scipy's KD-tree and
numpy, no device call) against the reference's own outputs in tests/golden/safeset.npz
(tests/golden/gen_safeset_golden.py), and the host-only parts of the package.

Everything on the KD-tree path is compared for equal bits.  The two neighbour Q-functions sum
their K terms in another order than the reference (whose argpartition leaves the order of
the K unspecified): ``q_function_bounds`` derives their bounds."""
import numpy as np
import pytest

from conftest import golden

U = 2.0 ** -53
SETS = ("s7", "s14")
FUEL_SLOTS = (None, 0, 1)            # available_fuel: none, fuels[0], fuels[1]
METHODS = ("nearest", "inverse_distance", "linear")


def build_set(g, name):
    from gp_mpc_rocket_landing_amd.terminal import FuelAwareSafeSet
    X = g[f"{name}_traj_states"].astype(np.float64)
    Uc = g[f"{name}_traj_controls"].astype(np.float64)
    C = g[f"{name}_traj_costs"].astype(np.float64)
    ss = FuelAwareSafeSet(n_x=X.shape[2], n_u=3)
    for j in range(len(X)):
        ss.add_trajectory(X[j], Uc[j], C[j])
    return ss


def check_queries(g, name, ss, want_path):
    """LocalSafeSet.query / query_batch against every recorded query of the set."""
    from gp_mpc_rocket_landing_amd.terminal import LocalSafeSet, LocalSafeSetConfig
    Xq = g[f"{name}_Xq"].astype(np.float64)
    states, q = ss.get_all_states(), ss.get_all_q_values()
    idx, dist, cnt = g[f"{name}_query_idx"], g[f"{name}_query_dist"], g[f"{name}_query_count"]
    for a, adaptive in enumerate((True, False)):
        ls = LocalSafeSet(ss, LocalSafeSetConfig(adaptive_K=adaptive))
        for f, slot in enumerate(FUEL_SLOTS):
            fuel = None if slot is None else float(g["fuels"][slot])
            for c, K in enumerate(g["ks"]):
                batch = ls.query_batch(Xq, int(K), fuel)
                assert ls.last_path == want_path
                for b, x in enumerate(Xq):
                    m = int(cnt[a, f, c, b])
                    ii = idx[a, f, c, b, :m].astype(np.int64)
                    got = ls.query(x, int(K), fuel)
                    assert ls.last_path == want_path
                    for res in (got, batch[b]):
                        assert np.array_equal(res[0], states[ii]), (name, adaptive, fuel, K, b)
                        assert np.array_equal(res[1], q[ii])
                        assert np.array_equal(res[2], dist[a, f, c, b, :m])
        for x in Xq[:3]:
            nb, qv, dd = ls.query(x, 10, float(g["fuels"][2]))        # no feasible state
            assert nb.shape == (0, ss.n_x) and qv.shape == (0,) and dd.shape == (0,)


def check_interp(g, name, ss):
    """interpolate_q (single: the reference's bits) for the three methods, and the hierarchy."""
    from gp_mpc_rocket_landing_amd.terminal import LocalSafeSet, LocalSafeSetConfig, MultiResolutionLocalSafeSet
    Xq = g[f"{name}_Xq"].astype(np.float64)
    for a, adaptive in enumerate((True, False)):
        ls = LocalSafeSet(ss, LocalSafeSetConfig(adaptive_K=adaptive))
        for m, method in enumerate(METHODS):
            got = np.array([ls.interpolate_q(x, method=method) for x in Xq])
            assert np.array_equal(got, g[f"{name}_interp"][a, m]), (name, adaptive, method)
    mr = MultiResolutionLocalSafeSet(ss)
    got = np.array([mr.interpolate_q_hierarchical(x) for x in Xq])
    assert np.array_equal(got, g[f"{name}_hierarchical"])
    assert len(mr.query_hierarchical(Xq[0])) == 3 and [len(r[1]) for r in mr.query_hierarchical(Xq[0])] == [5, 10, 20]


def gamma(m):
    return m * U / (1.0 - m * U)


def q_function_bounds(g, name, ss):
    """-> (idw bound, local-linear bound) per query, relative to |want|.

    Inverse distance: both sides form the same K weights 1 / d^p from equal distances, then
    K - 1 additions for their sum, one division, one product and K - 1 additions of
    non-negative terms (q is a cost-to-go of non-negative stage costs): 2K roundings a side,
    each result within gamma(2K) of the exact value, the two within 2 gamma(2K)(1 + gamma(2K)).

    Local linear: both sides solve the same normal equations A c = b (A = X^T W X + reg,
    m = n_x + 1 unknowns) assembled from the same K rows in a different order, by LU with
    partial pivoting.  An entry of A or b is K products of three factors summed: at most
    2K + 1 roundings with the ridge, an entrywise relative perturbation gamma(2K + 1) of the
    non-negative-weighted sums; the solve is backward stable, 3 m gamma(m) in the standard
    (growth-free) bound.  To first order |dc| / |c| <= cond(A) (2 gamma(2K + 1) + 3 m gamma(m))
    a side (perturbed A and perturbed b), twice that between the two sides.  The prediction is
    the entry c_0 (clipping is 1-Lipschitz), so |got - want| <= factor * cond(A) * |c|_2 with
    cond(A) and c computed here in numpy per query, from the fixture's states alone.  -> idw
    bound, local-linear factor * cond, |c|_2, cond."""
    K = int(g[f"{name}_n_neighbors"])
    Xq = g[f"{name}_Xq"].astype(np.float64)
    states, q = ss.get_all_states(), ss.get_all_q_values()
    idw = np.full(len(Xq), 2 * gamma(2 * K) * (1 + gamma(2 * K)))
    nl = len(g[f"{name}_local_linear"])
    # the systems from the data alone (numpy's neighbours, the reference's formula), not from the
    # package: the bound must not depend on the code it checks
    A = np.empty((nl, states.shape[1] + 1, states.shape[1] + 1)); rhs = np.empty(A.shape[:2])
    for b, x in enumerate(Xq[:nl]):
        dn = np.linalg.norm(states - x, axis=1)
        near = np.argsort(dn, kind="stable")[:K]
        D = np.hstack([np.ones((K, 1)), states[near] - x])
        W = np.diag(1.0 / (dn[near] + 1e-10))
        reg = 1e-4 * np.eye(A.shape[1]); reg[0, 0] = 0
        A[b] = D.T @ W @ D + reg
        rhs[b] = D.T @ W @ q[near]
    m = A.shape[1]
    cond = np.linalg.cond(A)
    # the generator's own figure (computed beside the reference): the same systems to rounding
    assert np.allclose(cond, g[f"{name}_local_linear_cond"], rtol=1e-6) and np.all(cond <= 1e8)
    coeffs = np.linalg.solve(A, rhs[:, :, None])[:, :, 0]
    factor = 2 * (2 * gamma(2 * K + 1) + 3 * m * gamma(m))
    return idw, factor * cond, np.linalg.norm(coeffs, axis=1), cond


def check_q_functions(g, name, ss, want_path):
    from gp_mpc_rocket_landing_amd.terminal import InverseDistanceQFunction, LocalLinearQFunction, QFunctionConfig
    K = int(g[f"{name}_n_neighbors"])
    Xq = g[f"{name}_Xq"].astype(np.float64)
    states, q = ss.get_all_states(), ss.get_all_q_values()
    b_idw, b_ll, cnorm, cond = q_function_bounds(g, name, ss)
    idw = InverseDistanceQFunction(QFunctionConfig(n_neighbors=K)); idw.fit(states, q)
    got, want = idw.predict_batch(Xq), g[f"{name}_idw"]
    assert idw.last_path == want_path
    err = np.abs(got - want) / np.abs(want)
    print(name, "inverse distance: max error", float(np.max(err / U)), "u; bound", float(b_idw[0] / U), "u")
    assert np.all(err <= b_idw)
    assert np.array_equal(got[-2:], want[-2:])                   # the two stored states: their own q
    assert idw.predict(Xq[1]) == got[1]
    ll = LocalLinearQFunction(QFunctionConfig(n_neighbors=K)); ll.fit(states, q)
    want = g[f"{name}_local_linear"]
    got = ll.predict_batch(Xq[:len(want)])
    assert ll.last_path == want_path
    err = np.abs(got - want) / cnorm
    print(name, "local linear: max error", float(np.max(err / U)), "u of |c|; bound", float(np.max(b_ll / U)),
          "u; max cond", float(np.max(cond)))
    assert np.all(err <= b_ll)


@pytest.fixture()
def host_knn(monkeypatch):
    monkeypatch.setenv("GPMPC_KNN", "host")


@pytest.mark.parametrize("name", SETS)
def test_safe_set_reproduces_the_reference(name):
    g = golden("safeset.npz")
    ss = build_set(g, name)
    assert np.array_equal(ss.get_all_q_values(), g[f"{name}_q"])
    assert np.array_equal(ss.get_fuel_required(), g[f"{name}_fuel_required"])
    states, q = ss.get_all_states(), ss.get_all_q_values()
    for j, fuel in enumerate(g["fuels"]):
        fs, fq, fi = ss.get_feasible_states(float(fuel))
        assert np.array_equal(fi, g[f"{name}_feasible_{j}"])
        assert np.array_equal(fs, states[fi]) and np.array_equal(fq, q[fi])
    assert float(g[f"{name}_min_gap"]) > 0 and float(g[f"{name}_radius_gap"]) > 0
    assert ss.num_states == len(states) <= 600 and ss.num_trajectories == ss.num_iterations


@pytest.mark.parametrize("name", SETS)
def test_local_safe_set_on_the_host_reproduces_the_reference(host_knn, name):
    g = golden("safeset.npz")
    ss = build_set(g, name)
    check_queries(g, name, ss, "host")
    check_interp(g, name, ss)


@pytest.mark.parametrize("name", SETS)
def test_q_functions_on_the_host_reproduce_the_reference(host_knn, name):
    g = golden("safeset.npz")
    check_q_functions(g, name, build_set(g, name), "host")


def test_fewer_states_than_k_min_raise_as_the_reference_does(host_knn):
    from gp_mpc_rocket_landing_amd.terminal import LocalSafeSet, SampledSafeSet
    g = golden("safeset.npz")
    X = g["tiny_states"].astype(np.float64)
    assert str(g["tiny_raises"]) == "IndexError"
    ss = SampledSafeSet(n_x=7, n_u=3)
    ls = LocalSafeSet(ss)
    assert ls.query(X[1])[0].shape == (0, 7) and ls.interpolate_q(X[1]) == np.inf     # empty set
    ss.add_trajectory(X, np.zeros((2, 3)), np.ones(2))
    ls.invalidate()
    with pytest.raises(IndexError):
        ls.query(X[1])
    with pytest.raises(ValueError):
        LocalSafeSet(ss, ls.config.__class__(K_min=1)).interpolate_q(X[1], method="cubic")


def test_knn_switch(monkeypatch):
    from gp_mpc_rocket_landing_amd.terminal import local_safe_set as m
    monkeypatch.setenv("GPMPC_KNN", "host")
    assert not m.use_device(10 ** 6, 10 ** 4, True)
    monkeypatch.setenv("GPMPC_KNN", "device")
    assert m.use_device(5, 1, True) and not m.use_device(5, 1, False)
    monkeypatch.delenv("GPMPC_KNN")
    assert m.use_device(100, m.KNN_CROSSOVER["queries"], True)
    assert not m.use_device(min(100, m.KNN_CROSSOVER["rows"] - 1), m.KNN_CROSSOVER["queries"] - 1, True)
    assert not m.use_device(10 ** 6, 10 ** 4, False)
    monkeypatch.setenv("GPMPC_KNN", "gpu")
    with pytest.raises(ValueError):
        m.use_device(5, 1, True)
    from gp_mpc_rocket_landing_amd import _lib
    assert (m.KNN_MAXK, m.KNN_MAXD) == (_lib.KNN_MAXK, _lib.KNN_MAXD)


def test_add_monte_carlo_results():
    """The landings of tests/golden/mc_sim_golden.npz as a MonteCarloResults: successes are
    added with a direct backward sum as cost-to-go, failures skipped."""
    from gp_mpc_rocket_landing_amd.experiments.monte_carlo import (LandingOutcome, MonteCarloResults,
                                                                   SimulationConfig, SimulationResult)
    from gp_mpc_rocket_landing_amd.terminal import SampledSafeSet
    g = golden("mc_sim_golden.npz")
    results = []
    for name in ("nominal", "dispersed"):
        for i, ns in enumerate(g[f"{name}_nsteps"]):
            X, Uc = g[f"{name}_states"][i, :ns + 1], g[f"{name}_controls"][i, :ns]
            oc = LandingOutcome(int(g[f"{name}_outcomes"][i]))
            results.append(SimulationResult(run_id=len(results), outcome=oc, success=oc == LandingOutcome.SUCCESS,
                                            states=X, controls=Uc, times=0.1 * np.arange(ns + 1), fuel_used=0.0,
                                            flight_time=0.1 * ns, final_position_error=0.0, final_velocity_error=0.0,
                                            max_constraint_violation=0.0, initial_state=X[0], compute_time_ms=0.0))
    ok = [r for r in results if r.success]
    assert 0 < len(ok) < len(results)

    def stage_cost(x, u):
        return float(x[1:4] @ x[1:4]) + 0.1 * float(u @ u)

    ss = SampledSafeSet(n_x=7, n_u=3)
    assert ss.add_monte_carlo_results(MonteCarloResults(SimulationConfig(), results), stage_cost) == len(ok)
    assert ss.num_trajectories == len(ok) and ss.num_states == sum(len(r.states) for r in ok)
    assert np.array_equal(ss.get_all_states(), np.vstack([r.states for r in ok]))
    q = ss.get_all_q_values()
    at = 0
    for r in ok:
        costs = [stage_cost(x, u) for x, u in zip(r.states[:-1], r.controls)]
        want = np.zeros(len(r.states))
        for k in range(len(costs) - 1, -1, -1):                # the direct backward sum
            want[k] = costs[k] + want[k + 1]
        assert np.array_equal(q[at:at + len(want)], want) and want[-1] == 0.0
        at += len(want)
    assert np.array_equal(ss.get_all_controls()[:len(ok[0].controls)], ok[0].controls)
    assert np.all(ss.get_all_controls()[len(ok[0].controls)] == 0.0)      # the terminal state's row


def test_safe_set_bookkeeping(tmp_path):
    from gp_mpc_rocket_landing_amd.terminal import FuelAwareSafeSet, SampledSafeSet, TrajectoryData
    rng = np.random.default_rng(0)
    ss = FuelAwareSafeSet(n_x=7, n_u=3, fuel_margin=0.25)
    assert ss.get_statistics() == {"num_trajectories": 0, "num_states": 0, "num_iterations": 0}
    assert ss.get_best_trajectory() is None and ss.get_all_states().shape == (0, 7)
    costs = []
    for j in range(3):
        X = rng.standard_normal((6, 7)); X[:, 0] = np.linspace(2.0, 1.5, 6)
        c = rng.random(5) + j
        ss.add_trajectory(X, rng.standard_normal((5, 3)), c, metadata={"j": j})
        costs.append(float(ss._trajectories[-1].total_cost))
    ss.add_trajectory(X, np.zeros((5, 3)), np.ones(5), iteration=7)
    assert ss.num_iterations == 8 and ss.num_trajectories == 4 and ss.num_states == 24
    st = ss.get_statistics()
    assert st["best_cost"] == min(costs + [5.0]) and st["cost_improvement"] == costs[0] - st["best_cost"]
    assert ss.get_best_trajectory().metadata == {"j": 0} and ss.get_trajectory(7).iteration == 7
    assert ss.get_trajectory(5) is None
    assert len(ss.get_states_from_iteration(1)[0]) == 6
    assert len(ss.get_states_with_min_fuel(1.75)[0]) == 4 * 3
    assert np.allclose(ss.get_fuel_required()[:6], np.linspace(0.5, 0.0, 6) + 0.25)
    path = str(tmp_path / "ss.pkl")
    ss.save(path)
    back = SampledSafeSet.load(path)
    assert np.array_equal(back.get_all_states(), ss.get_all_states()) and back.num_iterations == 8
    assert isinstance(back._trajectories[0], TrajectoryData) and back._trajectories[0].T == 5
    ss.clear()
    assert ss.num_states == 0 and ss.get_fuel_required().shape == (0,)
    with pytest.raises(AssertionError):
        TrajectoryData(0, np.zeros((3, 7)), np.zeros((3, 3)), np.zeros(3), np.zeros(4), 0.0)


def test_q_function_manager_and_iterations(host_knn):
    from gp_mpc_rocket_landing_amd.terminal import (IterativeQFunction, QFunctionConfig, QFunctionManager,
                                                    SampledSafeSet)
    g = golden("safeset.npz")
    X = g["s7_traj_states"].astype(np.float64); Uc = g["s7_traj_controls"].astype(np.float64)
    C = g["s7_traj_costs"].astype(np.float64)
    ss = SampledSafeSet(n_x=7, n_u=3)
    man = QFunctionManager(ss)
    assert man.get_min_q() == np.inf and man.get_statistics() == {"n_points": 0} and man.needs_update()
    assert man.evaluate(X[0, 0]) == np.inf                      # nothing fitted: q_max
    for j in range(3):
        ss.add_trajectory(X[j], Uc[j], C[j])
    assert man.needs_update()
    man.update()
    assert not man.needs_update() and man.get_min_q() == 0.0 and man.get_statistics()["n_points"] == 123
    assert man.evaluate(X[1, 5]) == ss.get_all_q_values()[41 + 5]
    assert man.evaluate_batch(X[1, 5:7] + 0.01).shape == (2,)
    with pytest.raises(ValueError):
        QFunctionManager(ss, QFunctionConfig(method="spline"))
    it = IterativeQFunction(ss)
    x = X[2, 4]
    assert it.evaluate(x) == ss.get_all_q_values()[82 + 4]      # the latest iteration holds landing 2
    assert it.evaluate(x, iteration=0) != it.evaluate(x) and it.get_q_at_iteration(-1) is None
    assert it.get_improvement(x) == it.evaluate(x, 0) - it.evaluate(x, 2)
