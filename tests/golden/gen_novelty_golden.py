"""Generate novelty.npz from the reference's own novelty_selector.py.

Needs the reference checkout and scipy (so the reference takes its KD-tree branch); only the
.npz written next to this script travels.  The reference module is loaded by file path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_novelty_golden.py <reference>/src/learning/novelty_selector.py

Cases (standard-normal data, fixed seeds):

    a  d 5,  n 300, r 64, n_select 40, NoveltyConfig()               tie-heavy: the scores saturate
    b  d 13, n 257, r 65, n_select 33, NoveltyConfig()               tie-heavy: several scores exactly 1.0
    c  d 5,  n 300, r 64, n_select 40, distance_threshold 3.0, methods "combined" (with residuals Y) and "distance"
    d  d 13, n 257, r 65, n_select 33, the same

c shares a's data and d shares b's; inputs are float32-representable and stored as float32.
Per data set it keeps the KD-tree's nearest-reference distances; per case and method X, R, Y, the scores, select(n_select), select(None) and
select_diverse(n_select) of the reference, and the winning combined value of every pick from
the numpy restatement of the greedy loop (tests/test_select_host.py: greedy_ref), whose picks
are asserted equal to the reference's here.  For c and d the smallest gap between the best
and the second-best combined value over all picks is asserted >= 1e-6 and stored: picks
with that margin do not depend on the last bits of the scores.  One DataBuffer case:
max_size 48, two add() calls of 40 rows, d 5.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_select_host import greedy_ref  # noqa: E402

CASES = {"a": (5, 300, 64, 40, {}, ("combined",)),
         "b": (13, 257, 65, 33, {}, ("combined",)),
         "c": (5, 300, 64, 40, {"distance_threshold": 3.0}, ("combined", "distance")),
         "d": (13, 257, 65, 33, {"distance_threshold": 3.0}, ("combined", "distance"))}
SEEDS = {"a": 101, "b": 127, "c": 101, "d": 127, "buffer": 105}   # c shares a's data, d shares b's


def draw(rng, shape):
    return rng.standard_normal(shape)


def f32(a):
    """The inputs are float32-representable and stored as float32 (half the bytes); the
    tests widen them back to the same float64 values."""
    return np.asarray(a, np.float32)


def min_gap(X, scores, n_select):
    """The smallest (best - second best) combined value over the picks of the greedy loop."""
    idx, _ = greedy_ref(X, scores, n_select)
    gap = np.inf
    taken = np.zeros(len(X), bool)
    mind = np.full(len(X), np.inf)
    for t, p in enumerate(idx):
        v = scores.copy() if t == 0 else scores + 0.5 * mind
        v[taken] = -np.inf
        top = np.sort(v)[-2:]
        gap = min(gap, top[1] - top[0])
        taken[p] = True
        mind = np.minimum(mind, np.linalg.norm(X - X[p], axis=1))
    return gap


def main(ref_path):
    spec = importlib.util.spec_from_file_location("ref_novelty_selector", ref_path)
    ref = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = ref
    spec.loader.exec_module(ref)
    assert ref.HAS_SCIPY, "scipy is needed: the fixture records the KD-tree branch"
    out = {}
    for name, (d, n, r, n_select, over, methods) in CASES.items():
        rng = np.random.default_rng(SEEDS[name])
        X, R, Y = draw(rng, (n, d)), draw(rng, (r, d)), 0.05 * draw(rng, (n, 3))
        data = {"a": "ac", "b": "bd", "c": "ac", "d": "bd"}[name]
        out[f"{data}_X"], out[f"{data}_R"], out[f"{data}_Y"] = f32(X), f32(R), f32(Y)
        X, R, Y = (f32(v).astype(np.float64) for v in (X, R, Y))
        out[f"{name}_n_select"] = np.array(n_select)
        for method in methods:
            sel = ref.NoveltySelector(ref.NoveltyConfig(method=method, **over))
            sel.set_reference_data(R)
            Yc = Y if (over and method == "combined") else None   # a, b: no residual term
            scores = sel.compute_novelty_scores(X, Yc)
            picks = sel.select_diverse(X, Yc, n_select=n_select)
            idx, comb = greedy_ref(X, scores, n_select)
            assert np.array_equal(idx, picks), (name, method)
            key = f"{name}_{method}"
            out[f"{key}_scores"] = scores
            out[f"{data}_kd_dist"] = sel._kdtree.query(X, k=1)[0]   # the distances behind the scores
            out[f"{key}_select"] = sel.select(X, Yc, n_select=n_select).astype(np.int32)
            out[f"{key}_select_threshold"] = sel.select(X, Yc).astype(np.int32)
            out[f"{key}_diverse"] = picks.astype(np.int32)
            out[f"{key}_combined"] = comb
            if over:
                gap = min_gap(X, scores, n_select)
                assert gap >= 1e-6, (name, method, gap)
                out[f"{key}_gap"] = np.array(gap)
            else:
                out[f"{key}_ties_at_one"] = np.array(int(np.sum(scores == 1.0)))
    rng = np.random.default_rng(SEEDS["buffer"])
    buf = ref.DataBuffer(max_size=48)
    counts = []
    for k in range(2):
        Xn = f32(draw(rng, (40, 5))).astype(np.float64); Yn = f32(0.05 * draw(rng, (40, 3))).astype(np.float64)
        out[f"buffer_X{k}"], out[f"buffer_Y{k}"] = f32(Xn), f32(Yn)
        counts.append(int(buf.add(Xn, Yn)))
    out["buffer_counts"] = np.array(counts)
    out["buffer_X"], out["buffer_Y"] = buf.get_data()
    path = os.path.join(HERE, "novelty.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;",
          {k: (int(v) if v.dtype.kind == "i" else float(v)) for k, v in out.items() if v.ndim == 0})


if __name__ == "__main__":
    main(sys.argv[1])
