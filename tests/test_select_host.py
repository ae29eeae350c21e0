"""Novelty / diverse-subset selection without a GPU: the argument checks of gpmpc_nn_dist and
gpmpc_select_diverse (they refuse before any device call), the host-only branches of
learning.novelty_selector, and the numpy restatement of the greedy loop that the GPU tests
use as their oracle, pinned here to every select_diverse result of the reference in
tests/golden/novelty.npz (gen_novelty_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["a_combined", "b_combined", "c_combined", "c_distance", "d_combined", "d_distance"]


def greedy_ref(X, scores, n_select, w=0.5):
    """The reference's greedy loop (novelty_selector.py:264-296) with a running minimum:
    pick 0 = argmax(scores), pick t = argmax over the unselected of scores + w * (distance to
    the nearest pick), np.argmax = lowest index on ties.  Returns (indices, winning values)."""
    X = np.ascontiguousarray(X, np.float64)
    mind = np.full(len(X), np.inf)
    free = np.ones(len(X), bool)
    idx, comb = [], []
    for t in range(n_select):
        v = scores.copy() if t == 0 else scores + w * mind
        v[~free] = -np.inf
        p = int(np.argmax(v))
        idx.append(p); comb.append(v[p])
        free[p] = False
        mind = np.minimum(mind, np.linalg.norm(X - X[p], axis=1))
    return np.array(idx), np.array(comb)


def case_data(g, key):
    data = {"a": "ac", "b": "bd", "c": "ac", "d": "bd"}[key[0]]
    return (g[f"{data}_X"].astype(np.float64), g[f"{data}_R"].astype(np.float64),
            g[f"{data}_Y"].astype(np.float64), int(g[f"{key[0]}_n_select"]))


@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_the_reference_picks(key):
    g = golden("novelty.npz")
    X, _, _, n_select = case_data(g, key)
    idx, comb = greedy_ref(X, g[f"{key}_scores"], n_select)
    assert np.array_equal(idx, g[f"{key}_diverse"])
    assert np.array_equal(comb, g[f"{key}_combined"])


def test_fixture_is_tie_heavy_and_gapped():
    g = golden("novelty.npz")
    assert 6 <= int(g["b_combined_ties_at_one"]) <= 15
    assert int(np.sum(g["a_combined_scores"] > 1 - 1e-3)) > 100     # saturated
    for key in KEYS[2:]:
        assert float(g[f"{key}_gap"]) >= 1e-6


def _fake_ctx():
    return ctypes.create_string_buffer(256)   # never read: every call below is refused first


def test_nn_dist_refuses_bad_arguments():
    from gp_mpc_rocket_landing_amd import _lib
    f = _lib._L.gpmpc_nn_dist
    X = np.zeros((4, 33)); R = np.zeros((3, 33)); out = np.zeros(4)
    ctx = _fake_ctx(); c = ctypes.addressof(ctx)
    d = _lib._d
    assert f(None, d(X), 4, d(R), 3, 5, d(out)) == -2
    assert f(c, None, 4, d(R), 3, 5, d(out)) == -2
    assert f(c, d(X), 4, None, 3, 5, d(out)) == -2
    assert f(c, d(X), 4, d(R), 3, 5, None) == -2
    assert f(c, d(X), 4, d(R), 3, 0, d(out)) == -2
    assert f(c, d(X), 4, d(R), 3, 33, d(out)) == -2
    assert f(c, d(X), -1, d(R), 3, 5, d(out)) == -2
    assert f(c, d(X), 4, d(R), 0, 5, d(out)) == -2
    assert b"bad argument" in _lib._L.gpmpc_last_error()


def test_select_diverse_refuses_bad_arguments():
    from gp_mpc_rocket_landing_amd import _lib
    f = _lib._L.gpmpc_select_diverse
    n = 6
    X = np.zeros((n, 33)); sc = np.zeros(n); idx = np.zeros(n, np.int32); comb = np.zeros(n)
    ctx = _fake_ctx(); c = ctypes.addressof(ctx)
    d, i = _lib._d, _lib._i
    assert f(None, d(X), n, 5, d(sc), 2, 0.5, 0, i(idx), d(comb)) == -2
    assert f(c, None, n, 5, d(sc), 2, 0.5, 0, i(idx), d(comb)) == -2
    assert f(c, d(X), n, 5, None, 2, 0.5, 0, i(idx), d(comb)) == -2
    assert f(c, d(X), n, 5, d(sc), 2, 0.5, 0, None, d(comb)) == -2
    assert f(c, d(X), n, 0, d(sc), 2, 0.5, 0, i(idx), d(comb)) == -2
    assert f(c, d(X), n, 33, d(sc), 2, 0.5, 0, i(idx), d(comb)) == -2
    assert f(c, d(X), n, 5, d(sc), 0, 0.5, 0, i(idx), d(comb)) == -2
    assert f(c, d(X), n, 5, d(sc), n + 1, 0.5, 0, i(idx), d(comb)) == -2
    assert f(c, d(X), n, 5, d(sc), 2, 0.5, 3, i(idx), d(comb)) == -2
    assert f(c, d(X), n, 5, d(sc), 2, 0.5, -1, i(idx), d(comb)) == -2
    # path 1 forced past its register budget (the buffers are not reached)
    assert f(c, d(X), _lib.SELECT_ONE_MAXN + 1, 5, d(sc), 2, 0.5, 1, i(idx), d(comb)) == -2


def test_wrappers_refuse_non_finite_input():
    from gp_mpc_rocket_landing_amd import _lib

    class NoCtx:
        h = None
    X = np.zeros((4, 3)); bad = X.copy(); bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        _lib.nn_dist(NoCtx, bad, X)
    with pytest.raises(ValueError):
        _lib.nn_dist(NoCtx, X, bad)
    with pytest.raises(ValueError):
        _lib.select_diverse(NoCtx, bad, np.zeros(4), 2)
    with pytest.raises(ValueError):
        _lib.select_diverse(NoCtx, X, np.array([0.0, np.inf, 0.0, 0.0]), 2)
    with pytest.raises(ValueError):
        _lib.select_diverse(NoCtx, X, np.zeros(3), 2)


def test_binding_constants_match_the_kernels():
    from gp_mpc_rocket_landing_amd import _lib
    src = open(os.path.join(REPO, "gp_mpc_rocket_landing_amd", "csrc", "select.hip")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (SEL_MAXD|NN_TILE|SEL1_THREADS|SEL1_CPT|SEL2_THREADS|SEL2_CPT|"
                                            r"SEL_CROSSOVER) (\d+)", src)}
    assert val["SEL_MAXD"] == _lib.SELECT_MAXD and val["NN_TILE"] == _lib.NN_TILE
    assert val["SEL1_THREADS"] == _lib.SELECT_ONE_THREADS
    assert val["SEL1_THREADS"] * val["SEL1_CPT"] == _lib.SELECT_ONE_MAXN
    assert val["SEL2_THREADS"] * val["SEL2_CPT"] == _lib.SELECT_GRID_SLICE
    assert val["SEL_CROSSOVER"] == _lib.SELECT_CROSSOVER <= _lib.SELECT_ONE_MAXN


def test_host_only_branches_of_the_selector():
    from gp_mpc_rocket_landing_amd.learning import DataBuffer, NoveltyConfig, NoveltySelector
    sel = NoveltySelector()
    assert sel.config == NoveltyConfig()
    empty = sel.compute_novelty_scores(np.zeros((0, 4)))
    assert empty.shape == (0,)
    X = np.arange(12.0).reshape(6, 2)
    assert np.array_equal(sel._compute_distance_novelty(X), np.ones(6))      # no reference data
    assert np.array_equal(sel._compute_uncertainty_novelty(X), np.ones(6))   # no model
    assert np.array_equal(sel.select_diverse(X, n_select=6), np.arange(6))
    assert np.array_equal(sel.select_diverse(X, n_select=9), np.arange(6))
    buf = DataBuffer(max_size=10)
    assert buf.size == 0 and buf.get_data()[0].shape == (0,)
    assert buf.add(X, X[:, :1]) == 6 and buf.add(X[:4], X[:4, :1]) == 4 and buf.size == 10


def test_select_thresholds_and_top_k():
    """select with the residual method only (host numpy): the scores are min(|Y| / 0.1, 1)
    over their maximum."""
    from gp_mpc_rocket_landing_amd.learning import NoveltyConfig, NoveltySelector
    sel = NoveltySelector(NoveltyConfig(method="residual", score_threshold=0.5))
    X = np.zeros((5, 2))
    Y = np.array([0.01, 0.08, 0.04, 0.2, 0.05])
    want = np.minimum(np.abs(Y) / 0.1, 1.0) * 0.5
    want = want / want.max()
    idx, scores = sel.select(X, Y, return_scores=True)
    assert np.array_equal(scores, want)
    assert np.array_equal(idx, [1, 3, 4])                      # scores >= 0.5
    assert np.array_equal(sel.select(X, Y, n_select=2), [1, 3])  # argsort's last two
    assert np.array_equal(sel.select(X, Y, n_select=5), np.arange(5))
    Y2 = np.stack([Y, np.zeros(5)], axis=1)                    # 2-D residuals: row norms
    assert np.array_equal(sel.compute_novelty_scores(X, Y2), want)


def test_uncertainty_term_and_failing_model():
    from gp_mpc_rocket_landing_amd.learning import ActiveDataSelector, NoveltyConfig, NoveltySelector

    class Model:
        def predict(self, X):
            return np.zeros((len(X), 2)), np.tile([[0.1, 0.2]], (len(X), 1)) * np.arange(len(X))[:, None]

    class Broken:
        def predict(self, X):
            raise RuntimeError("no fit")
    X = np.zeros((4, 2))
    sel = NoveltySelector(NoveltyConfig(method="uncertainty"))
    sel.set_gp_model(Model())
    var = 0.3 * np.arange(4)
    assert np.allclose(sel._compute_uncertainty_novelty(X), np.minimum(var / 0.5, 1.0), rtol=0, atol=1e-15)
    sel.set_gp_model(Broken())
    assert np.array_equal(sel._compute_uncertainty_novelty(X), np.ones(4))
    act = ActiveDataSelector(Model())
    assert np.array_equal(act.select(X, 2), [2, 3]) and np.array_equal(act.select(X, 4), np.arange(4))
    assert np.array_equal(ActiveDataSelector(Model(), "anything").compute_acquisition(X), act.compute_acquisition(X))
