"""gpmpc_nn_dist / gpmpc_select_diverse and learning.novelty_selector on the device.

Oracles: numpy's brute-force distance; the numpy restatement of the reference's greedy loop
(test_select_host.greedy_ref, pinned there to the reference's own picks); the reference's
results in tests/golden/novelty.npz.  The kernels sum in numpy's order, so every comparison
with numpy is for equal bits."""
import numpy as np
import pytest

from conftest import golden
from test_select_host import KEYS, case_data, greedy_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


# ---- nn_dist -----------------------------------------------------------------
def _tile_counts():
    t = _lib().NN_TILE
    return [1, t - 1, t, t + 1, 2 * t + 44]   # the last: three tiles, a ragged end


@pytest.mark.parametrize("d", [1, 7, 8, 9, 13, 16, 17, 32])
@pytest.mark.parametrize("ri", range(5))
def test_nn_dist_is_numpy_brute_force(gpu_ctx, d, ri):
    r = _tile_counts()[ri]
    rng = np.random.default_rng(1000 * d + r)
    R = rng.standard_normal((r, d))
    for n in (1, 65, 257):
        X = rng.standard_normal((n, d))
        X[n // 2] = R[r // 2]   # one exact hit: distance 0
        want = np.min(np.linalg.norm(X[:, None] - R, axis=2), axis=1)
        got = _lib().nn_dist(gpu_ctx, X, R)
        assert got.dtype == np.float64 and got.shape == (n,)
        assert np.array_equal(got, want), (d, r, n, np.max(np.abs(got - want)))


@pytest.mark.parametrize("data", ["ac", "bd"])
def test_nn_dist_against_the_reference_kd_tree(gpu_ctx, data):
    """The fixture's distances come from scipy's KD-tree, whose summation order is its own.
    Either side rounds d differences (relative error u = 2^-53 each), d squares (each term
    then carries 3u) and d - 1 sums (u each, so the sum of squares is within (d + 2)u),
    halves that in the square root and adds the root's own u: (d + 4)u / 2 a side,
    (d + 4)u between the two."""
    g = golden("novelty.npz")
    X, R = g[f"{data}_X"].astype(np.float64), g[f"{data}_R"].astype(np.float64)
    want = g[f"{data}_kd_dist"]
    got = _lib().nn_dist(gpu_ctx, X, R)
    d = X.shape[1]
    err = np.abs(got - want) / want
    print(data, "max relative error", err.max() / U, "u; bound", d + 4, "u")
    assert np.all(err <= (d + 4) * U)


def test_nn_dist_no_candidates(gpu_ctx):
    assert _lib().nn_dist(gpu_ctx, np.zeros((0, 3)), np.ones((2, 3))).shape == (0,)


# ---- select_diverse against the fixture ------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("key", KEYS)
def test_select_diverse_reproduces_the_reference(gpu_ctx, key, path):
    g = golden("novelty.npz")
    X, _, _, n_select = case_data(g, key)
    idx, comb = _lib().select_diverse(gpu_ctx, X, g[f"{key}_scores"], n_select, path=path)
    assert np.array_equal(idx, g[f"{key}_diverse"])
    assert np.array_equal(comb, g[f"{key}_combined"])


# ---- select_diverse against the numpy restatement ----------------------------------
_inputs = {}


def _case(d, n, kind):
    """(X, scores, reference picks, reference values) for n - 1 picks (n = 1: one pick);
    greedy picks are a prefix of any longer run's, so one reference serves every n_select."""
    key = (d, n, kind)
    if key not in _inputs:
        rng = np.random.default_rng(7919 * d + 31 * n + len(kind))
        X = rng.standard_normal((n, d))
        scores = rng.uniform(0.0, 1.0, n)
        if kind == "dup":      # duplicated rows with equal scores: ties at minimum distance 0
            src = rng.integers(0, max(n // 3, 1), n)
            X = X[src]
            scores = np.round(scores[src], 1)
        elif kind == "equal":  # all scores equal
            scores = np.full(n, 0.25)
        _inputs[key] = (X, scores) + greedy_ref(X, scores, max(n - 1, 1))
    return _inputs[key]


def _ns():
    L = _lib()
    t, s = L.SELECT_ONE_THREADS, L.SELECT_GRID_SLICE
    # path 1: below / at / above the thread count, 700 = a ragged number of candidates a
    # thread; path 2: one workgroup, one above it = a last workgroup of one candidate,
    # three workgroups with a single-candidate last one
    return {1: [1, 2, t - 1, t, t + 1, t + 188], 2: [1, 2, s, s + 1, 2 * s + 1]}, {1: [2, t + 1], 2: [2, s + 1]}


def _select_cases():
    normal, special = {1: [1, 2, 511, 512, 513, 700], 2: [1, 2, 1024, 1025, 2049]}, {1: [2, 513], 2: [2, 1025]}
    out = []
    for path in (1, 2):
        out += [(path, n, "normal") for n in normal[path]]
        out += [(path, n, kind) for n in special[path] for kind in ("dup", "equal")]
    return out


def test_case_sizes_follow_the_kernel_constants():
    normal, special = _ns()
    got = _select_cases()
    for path in (1, 2):
        assert [n for p, n, k in got if p == path and k == "normal"] == normal[path]
        assert sorted({n for p, n, k in got if p == path and k != "normal"}) == special[path]


@pytest.mark.parametrize("d", [1, 7, 8, 13, 17, 32])
@pytest.mark.parametrize("path,n,kind", _select_cases())
def test_select_diverse_is_the_greedy_loop(gpu_ctx, d, path, n, kind):
    X, scores, ref_idx, ref_comb = _case(d, n, kind)
    for n_select in sorted({k for k in (1, 2, n - 1) if 1 <= k <= max(n - 1, 1)}):
        idx, comb = _lib().select_diverse(gpu_ctx, X, scores, n_select, path=path)
        assert idx.shape == (n_select,)
        assert np.array_equal(idx, ref_idx[:n_select]), (d, n, kind, n_select)
        assert np.array_equal(comb, ref_comb[:n_select]), (d, n, kind, n_select)
    if n > 1:   # every candidate: the last pick is whatever is left
        idx, _ = _lib().select_diverse(gpu_ctx, X, scores, n, path=path)
        assert np.array_equal(idx[:-1], ref_idx) and sorted(idx) == list(range(n))


def test_automatic_path_agrees_with_both_forced_paths(gpu_ctx):
    L = _lib()
    rng = np.random.default_rng(5)
    for n in (L.SELECT_CROSSOVER, L.SELECT_CROSSOVER + 1):
        X = rng.standard_normal((n, 5)); scores = rng.uniform(0, 1, n)
        auto = L.select_diverse(gpu_ctx, X, scores, 20, path=0)
        ref = greedy_ref(X, scores, 20)
        assert np.array_equal(auto[0], ref[0]) and np.array_equal(auto[1], ref[1])
        for path in [1, 2] if n <= L.SELECT_ONE_MAXN else [2]:
            forced = L.select_diverse(gpu_ctx, X, scores, 20, path=path)
            assert np.array_equal(auto[0], forced[0]) and np.array_equal(auto[1], forced[1]), (n, path)
    with pytest.raises(L.HIPError) as e:   # path 1 forced past its register budget
        L.select_diverse(gpu_ctx, np.zeros((L.SELECT_ONE_MAXN + 1, 2)), np.zeros(L.SELECT_ONE_MAXN + 1), 2, path=1)
    assert e.value.rc == -2


def test_select_diverse_without_combined_out(gpu_ctx):
    """combined_out is nullable in the C-ABI."""
    L = _lib()
    X, scores, ref_idx, _ = _case(7, 513, "normal")
    for path in (1, 2):
        idx = np.zeros(9, np.int32)
        rc = L._L.gpmpc_select_diverse(gpu_ctx.h, L._d(X), 513, 7, L._d(scores), 9, 0.5, path, L._i(idx), None)
        assert rc == 0 and np.array_equal(idx, ref_idx[:9])


# ---- the surface against the reference ------------------------------------------------
@pytest.mark.parametrize("key", KEYS[2:])
def test_selector_matches_the_reference_end_to_end(key):
    """Scores within 1e-13 of the reference's: the device distance and the KD-tree's differ
    by at most (d + 4) 2^-53 relative (test_nn_dist_against_the_reference_kd_tree), which
    1 - exp(-dist / 3) (slope <= 1/3, dist < 10) and the division by the maximum keep below
    1e-14.  The picks are equal: the fixture's smallest gap between the best and the second
    combined value is >= 1e-6."""
    from gp_mpc_rocket_landing_amd.learning import NoveltyConfig, NoveltySelector
    g = golden("novelty.npz")
    X, R, Y, n_select = case_data(g, key)
    method = key[2:]
    sel = NoveltySelector(NoveltyConfig(method=method, distance_threshold=3.0))
    sel.set_reference_data(R)
    Yc = Y if method == "combined" else None
    scores = sel.compute_novelty_scores(X, Yc)
    print(key, "max score difference", np.max(np.abs(scores - g[f"{key}_scores"])))
    assert np.all(np.abs(scores - g[f"{key}_scores"]) <= 1e-13)
    assert np.array_equal(sel.select_diverse(X, Yc, n_select=n_select), g[f"{key}_diverse"])
    idx, sc = sel.select(X, Yc, n_select=n_select, return_scores=True)
    assert np.array_equal(sc, scores)
    assert np.array_equal(np.sort(idx), np.sort(g[f"{key}_select"]))
    assert np.array_equal(sel.select(X, Yc), g[f"{key}_select_threshold"])


def test_data_buffer_matches_the_reference():
    from gp_mpc_rocket_landing_amd.learning import DataBuffer
    g = golden("novelty.npz")
    buf = DataBuffer(max_size=48)
    counts = [int(buf.add(g[f"buffer_X{k}"].astype(np.float64), g[f"buffer_Y{k}"].astype(np.float64)))
              for k in range(2)]
    assert counts == list(g["buffer_counts"])
    Xb, Yb = buf.get_data()
    assert buf.size == 48 and np.array_equal(Xb, g["buffer_X"]) and np.array_equal(Yb, g["buffer_Y"])


def test_active_selector_on_a_fitted_gp():
    from gp_mpc_rocket_landing_amd.gp import ExactGP, SquaredExponentialARD
    from gp_mpc_rocket_landing_amd.learning import ActiveDataSelector, NoveltyConfig, NoveltySelector
    rng = np.random.default_rng(11)
    Xt = rng.standard_normal((40, 11)); yt = np.sin(Xt[:, 0]) + 0.1 * Xt[:, 1]
    gp = ExactGP(SquaredExponentialARD(11)).fit(Xt, yt)
    Xq = 2.0 * rng.standard_normal((60, 11))
    pred = gp.predict(Xq)
    act = ActiveDataSelector(gp)
    assert np.array_equal(act.compute_acquisition(Xq), pred.variance)
    assert np.array_equal(act.select(Xq, 7), np.argsort(pred.variance)[-7:])
    assert np.array_equal(act.select(Xq, 60), np.arange(60))
    from scipy.stats import norm
    std = np.sqrt(pred.variance)
    z = (0 - pred.mean) / (std + 1e-10)
    ei = (0 - pred.mean) * norm.cdf(z) + std * norm.pdf(z)
    assert np.array_equal(ActiveDataSelector(gp, "expected_improvement").compute_acquisition(Xq), ei)
    sel = NoveltySelector(NoveltyConfig(method="uncertainty"))
    sel.set_gp_model(gp)
    want = np.minimum(pred.variance / 0.5, 1.0)
    assert np.array_equal(sel.compute_novelty_scores(Xq), want / want.max())
