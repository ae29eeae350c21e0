"""Generate safeset.npz from the reference's own src/terminal modules.

Needs the reference checkout and scipy; only the .npz written next to this script travels.
The three numpy / scipy modules are loaded by file path (the package's __init__ would pull
in the CasADi convex hull):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_safeset_golden.py <reference>

Two FuelAwareSafeSets built by add_trajectory from short synthetic landings (a noisy decay of
a random start towards the pad, the mass falling along the way; float32-representable and
stored as float32):

    s7   n_x 7,  12 landings of 41 states (492 states)
    s14  n_x 14, 10 landings of 31 states (310 states)

and per set 12 query states: four stored states plus small noise, three near the pad (the
dense end), three far from everything, one stored state itself, one stored start.  Recorded
per set, all from the reference's objects:

    q, fuel_required, get_feasible_states(fuel) indices for FUELS
    LocalSafeSet.query for adaptive_K on / off x available_fuel (None, FUELS[0], FUELS[1]) x
        K (1, 4, 10, 50): the neighbours as row indices (the states are asserted distinct, the
        test checks states[idx] and q[idx]), the distances, the count; FUELS[2] leaves no state
    LocalSafeSet.interpolate_q for its three methods, adaptive_K on / off
    MultiResolutionLocalSafeSet.interpolate_q_hierarchical
    InverseDistanceQFunction / LocalLinearQFunction predict_batch (QCFG neighbours; the local-
        linear one on the ten queries that are no stored state) and the condition number of
        every local-linear system (asserted <= 1e8)
    tiny: one landing of three states, where LocalSafeSet.query raises IndexError

Two facts about every recorded query are asserted and stored (they are conditions on the
inputs; the seeds were changed until the reference alone satisfied them): among the K + 1
nearest no two squared distances are equal (``*_min_gap`` > 0: the neighbours do not depend on
a tie rule), and no stored row lies exactly on the density radius (``*_radius_gap`` > 0).
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import knn_check as kc  # noqa: E402

SETS = {"s7": (7, 12, 40, 701), "s14": (14, 10, 30, 1402)}     # n_x, landings, steps, seed
FUELS = (0.6, 0.1, 0.05)          # about half the states; the landings' last states only; none
KS = (1, 4, 10, 50)
QCFG = {"s7": 10, "s14": 30}      # n_neighbors of the two Q-functions
NQ_LINEAR = 10                    # the local-linear fit takes the first ten queries: at a stored state itself its
                                  # weight 1 / (0 + 1e-10) puts the condition number past any useful bound


def load_reference(root):
    """The reference's terminal package without its __init__: safe_set, local_safe_set, q_function."""
    pkg_dir = os.path.join(root, "src", "terminal")
    pkg = types.ModuleType("ref_terminal")
    pkg.__path__ = [pkg_dir]
    sys.modules["ref_terminal"] = pkg
    mods = {}
    for name in ("safe_set", "local_safe_set", "q_function"):
        spec = importlib.util.spec_from_file_location(f"ref_terminal.{name}", os.path.join(pkg_dir, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def f32(a):
    return np.asarray(a, np.float32)


def landings(n_x, count, steps, rng):
    """count synthetic landings: states (count, steps + 1, n_x), controls (count, steps, 3),
    non-negative stage costs (count, steps); all float32-representable."""
    X = np.zeros((count, steps + 1, n_x)); U = np.zeros((count, steps, 3)); C = np.zeros((count, steps))
    for j in range(count):
        x = rng.standard_normal(n_x) * 2.5
        x[0] = 2.0 + 0.3 * rng.random()
        if n_x == 14:
            x[7:11] = [1.0, 0.0, 0.0, 0.0] + 0.2 * rng.standard_normal(4)
        for k in range(steps + 1):
            X[j, k] = x
            if k == steps:
                break
            u = rng.standard_normal(3)
            U[j, k] = u
            C[j, k] = 0.1 * float(x[1:] @ x[1:]) + 0.01 * float(u @ u)
            m = x[0] - 0.02 * (1.0 + rng.random())
            x = 0.88 * x + 0.08 * rng.standard_normal(n_x)
            x[0] = m
    return (f32(v).astype(np.float64) for v in (X, U, C))


def queries(states, rng):
    n, d = states.shape
    near = states[rng.choice(n, 4, replace=False)] + 0.05 * rng.standard_normal((4, d))
    pad = 0.3 * rng.standard_normal((3, d)); pad[:, 0] = 1.2
    far = 6.0 * rng.standard_normal((3, d))
    return f32(np.vstack([near, pad, far, states[n // 3][None], states[0][None]])).astype(np.float64)


def gaps(W, xw, k, radius):
    """(smallest difference between consecutive s^2 among the k + 1 nearest, smallest
    |s^2 - radius^2|) of the weighted rows W to the weighted query xw."""
    s2 = np.sort(kc.sq_kd(W, xw))
    head = s2[:min(k + 1, len(s2))]
    return (float(np.min(np.diff(head))) if len(head) > 1 else np.inf), float(np.min(np.abs(s2 - radius * radius)))


def main(root):
    ref = load_reference(root)
    ss_mod, ls_mod, qf_mod = ref["safe_set"], ref["local_safe_set"], ref["q_function"]
    out = {"fuels": np.array(FUELS), "ks": np.array(KS)}
    for name, (n_x, count, steps, seed) in SETS.items():
        rng = np.random.default_rng(seed)
        X, U, C = landings(n_x, count, steps, rng)
        ss = ss_mod.FuelAwareSafeSet(n_x=n_x, n_u=3)
        for j in range(count):
            ss.add_trajectory(X[j], U[j], C[j])
        states, q = ss.get_all_states(), ss.get_all_q_values()
        assert len(states) <= 600 and len(np.unique(states, axis=0)) == len(states)
        assert np.all(q >= 0.0)
        Xq = queries(states, rng)
        nq = len(Xq)
        out[f"{name}_traj_states"], out[f"{name}_traj_controls"], out[f"{name}_traj_costs"] = f32(X), f32(U), f32(C)
        out[f"{name}_Xq"] = f32(Xq)
        out[f"{name}_q"] = q
        out[f"{name}_fuel_required"] = ss.get_fuel_required()
        for j, fuel in enumerate(FUELS):
            fs, fq, fi = ss.get_feasible_states(fuel)
            assert np.array_equal(fs, states[fi]) and np.array_equal(fq, q[fi])
            out[f"{name}_feasible_{j}"] = fi.astype(np.int32)
        assert len(out[f"{name}_feasible_1"]) == count and len(out[f"{name}_feasible_2"]) == 0

        def row_index(rows):
            idx = np.array([int(np.nonzero(np.all(states == r, axis=1))[0][0]) for r in rows], np.int16)
            assert np.array_equal(states[idx], rows)
            return idx

        # LocalSafeSet.query / interpolate_q
        fuels = (None, FUELS[0], FUELS[1])
        idx = np.full((2, len(fuels), len(KS), nq, 50), -1, np.int16)
        dist = np.full((2, len(fuels), len(KS), nq, 50), np.nan)
        cnt = np.zeros((2, len(fuels), len(KS), nq), np.int16)
        interp = np.zeros((2, 3, nq))
        min_gap, radius_gap = np.inf, np.inf
        for a, adaptive in enumerate((True, False)):
            cfg = ls_mod.LocalSafeSetConfig(adaptive_K=adaptive)
            ls = ls_mod.LocalSafeSet(ss, cfg)
            W = states * ls._weights[np.newaxis, :]
            for f, fuel in enumerate(fuels):
                rows = np.arange(len(states)) if fuel is None else ss.get_feasible_states(fuel)[2]
                for b, x in enumerate(Xq):
                    g, r = gaps(W[rows], x * ls._weights, 50, cfg.density_radius)
                    min_gap, radius_gap = min(min_gap, g), min(radius_gap, r)
                    for c, K in enumerate(KS):
                        nb, qv, dd = ls.query(x, K, fuel)
                        ii = row_index(nb)
                        assert np.array_equal(qv, q[ii]) and len(dd) == len(ii) <= 50
                        idx[a, f, c, b, :len(ii)] = ii
                        dist[a, f, c, b, :len(ii)] = dd
                        cnt[a, f, c, b] = len(ii)
            for b, x in enumerate(Xq):
                assert len(ls.query(x, 10, FUELS[2])[0]) == 0
                for m, method in enumerate(("nearest", "inverse_distance", "linear")):
                    interp[a, m, b] = ls.interpolate_q(x, method=method)
        assert min_gap > 0.0 and radius_gap > 0.0, (name, min_gap, radius_gap)
        out[f"{name}_query_idx"], out[f"{name}_query_dist"], out[f"{name}_query_count"] = idx, dist, cnt
        out[f"{name}_interp"] = interp
        out[f"{name}_min_gap"], out[f"{name}_radius_gap"] = np.array(min_gap), np.array(radius_gap)
        mr = ls_mod.MultiResolutionLocalSafeSet(ss)
        out[f"{name}_hierarchical"] = np.array([mr.interpolate_q_hierarchical(x) for x in Xq])

        # the two neighbour Q-functions (plain Euclidean distance)
        qcfg = qf_mod.QFunctionConfig(n_neighbors=QCFG[name])
        idw = qf_mod.InverseDistanceQFunction(qcfg); idw.fit(states, q)
        ll = qf_mod.LocalLinearQFunction(qcfg); ll.fit(states, q)
        out[f"{name}_idw"] = idw.predict_batch(Xq)
        out[f"{name}_local_linear"] = ll.predict_batch(Xq[:NQ_LINEAR])
        out[f"{name}_n_neighbors"] = np.array(QCFG[name])
        conds, qgap = [], np.inf
        for b, x in enumerate(Xq):
            s2 = np.sort(kc.sq_np(states, x))
            qgap = min(qgap, float(np.min(np.diff(s2[:QCFG[name] + 1]))))
            if b >= NQ_LINEAR:
                continue
            dn = np.linalg.norm(states - x, axis=1)
            near = np.argsort(dn)[:QCFG[name]]
            D = np.hstack([np.ones((len(near), 1)), states[near] - x])
            reg = qcfg.local_linear_reg * np.eye(n_x + 1); reg[0, 0] = 0
            conds.append(np.linalg.cond(D.T @ np.diag(1.0 / (dn[near] + 1e-10)) @ D + reg))
        assert qgap > 0.0 and max(conds) <= 1e8, (name, qgap, max(conds))
        out[f"{name}_qf_min_gap"] = np.array(qgap)
        out[f"{name}_local_linear_cond"] = np.array(conds)

    # fewer states than K_min: the reference's states[indices] raises
    tiny = ss_mod.SampledSafeSet(n_x=7, n_u=3)
    tiny.add_trajectory(X7 := np.arange(21.0).reshape(3, 7) / 8.0, np.zeros((2, 3)), np.ones(2))
    try:
        ls_mod.LocalSafeSet(tiny).query(X7[1])
        raised = ""
    except IndexError as e:
        raised = type(e).__name__
    assert raised == "IndexError"
    out["tiny_states"] = f32(X7)
    out["tiny_raises"] = np.array(raised)

    path = os.path.join(HERE, "safeset.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;",
          {k: float(v) for k, v in out.items() if v.ndim == 0 and v.dtype.kind == "f"},
          {k: float(np.max(v)) for k, v in out.items() if k.endswith("_cond")})


if __name__ == "__main__":
    main(sys.argv[1])
