"""Generate tube.npz from the reference's own src/safety/tube_mpc.py.

Needs the reference checkout; only the .npz written next to this script travels.  The
reference's module is loaded by file path and driven with this package's Rocket6DoFDynamics
(the reference's 6-DoF class needs simdyn, which is not installed):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_tube_golden.py <reference> [quick]

(quick: coverage only, no spreads, nothing written.)  The trajectories, horizons, bounds, gains,
GP stand-ins and Monte-Carlo cases are tests/tube_cases.py's.  Recorded:

    lin_<traj>_<w>_<K>      propagate_linear at N = 15 (tube_cases.linear_combos); every shorter horizon
                            of tube_cases.HORIZONS is asserted here to return the first N + 1 rows of
                            it bit for bit, so one array serves them all
    linz_*                  _linearize at four (x, u) with eps = 1e-6 and eps = 1e-3 (the coarse eps
                            divides rounding noise by a thousand times less: it pins the arithmetic)
    gp_<stub>_tubes / _vars propagate_with_gp over the stand-ins (the order of tries, the tuple, three /
                            six outputs, the w_max^2 fallback); two outputs raise ValueError
                            in the reference (a broadcast of 2 onto 3 rows): gp_two_raises
    mc_S<n>_q<q>_N<N>       propagate_monte_carlo under np.random.seed(tube_cases.mc_seed(...)), and
    mc_batch                two trajectories under one seed, the reference called twice in a row
    tight_<a|b>_*           get_tightened_params at every step of two tubes (default w_max: the tube is
                            lin_tilted_wmax_none; w_max = 1e-3: tight_b_tubes)

Asserted and stored as ``coverage_*``: every branch of the tightener occurred (the glideslope
untouched at zero position uncertainty, tightened, clamped at 10 degrees; the altitude floor of
1.0 taken and not; the tilt tightened and clamped at 10 degrees), the order of the GP calls, and
that the global RNG's block draw has the bits of the per-particle draws.

    spread_*: the largest change of the recorded numbers over three more runs of the reference
        with a plant whose ``step`` output is multiplied by (1 + 2^-52 z), z standard normal
        (gen_safety_golden.py's rule): what one rounding per plant step does to the answer.  The
        finite differences divide that noise by eps.  Per horizon for the linear and GP tubes
        (spread_lin_N<N>, spread_gp_N<N>), per eps for A and B, one for the Monte-Carlo tubes.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import tube_cases as tc  # noqa: E402


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_tube_mpc", os.path.join(root, "src", "safety", "tube_mpc.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class NoisyPlant:
    """The plant with every ``step`` output multiplied by (1 + 2^-52 z)."""

    def __init__(self, base, seed):
        self._base = base
        self._rng = np.random.default_rng(seed)

    def __getattr__(self, name):
        return getattr(self._base, name)

    def step(self, x, u, dt=None):
        return self._base.step(x, u, dt) * (1.0 + 2.0 ** -52 * self._rng.standard_normal(14))


def run_all(ref, plant_of, check):
    """Every recorded quantity with the plants ``plant_of(name)``.  check: assert what only the
    clean run must satisfy (prefixes, call orders) and collect the coverage."""
    out, cov = {}, {}
    trajs = {name: tc.nominal(name) for name in tc.TRAJECTORIES}
    props = {name: ref.TubePropagator(plant_of(name), ref.TubeMPCConfig()) for name in tc.TRAJECTORIES}
    # linear tubes
    for name, (X, U) in trajs.items():
        for wk, w, kk, K in tc.linear_combos(name):
            full = props[name].propagate_linear(X, U, None if w is None else w.copy(), K)
            out[f"lin_{name}_{wk}_{kk}"] = full
            if check:
                for N in tc.HORIZONS:
                    part = props[name].propagate_linear(X[:N + 1], U[:N], None if w is None else w.copy(), K)
                    assert np.array_equal(part, full[:N + 1]), (name, wk, kk, N)
    # _linearize
    pts = tc.linearize_points()
    out["linz_x"] = np.array([trajs[n][0][k] for n, k in pts])
    out["linz_u"] = np.array([trajs[n][1][k] for n, k in pts])
    for ek, eps in tc.EPS.items():
        AB = [props[n]._linearize(trajs[n][0][k].copy(), trajs[n][1][k].copy(), eps) for n, k in pts]
        out[f"linz_A_{ek}"] = np.array([a for a, _ in AB])
        out[f"linz_B_{ek}"] = np.array([b for _, b in AB])
    # GP tubes
    X, U = trajs[tc.GP_TRAJECTORY]
    p = props[tc.GP_TRAJECTORY]
    for sname, stub in tc.gp_stubs().items():
        tubes, gp_vars = p.propagate_with_gp(X, U, stub)
        out[f"gp_{sname}_tubes"], out[f"gp_{sname}_vars"] = tubes, gp_vars
        if check:
            if sname == "uncertainty":
                assert len(stub.calls) == tc.N_MAX and all(
                    np.array_equal(cx, X[k:k + 1]) and np.array_equal(cu, U[k:k + 1]) for k, (cx, cu) in enumerate(stub.calls))
                cov["gp_call_order"] = 1
            for N in tc.HORIZONS:
                fresh = tc.gp_stubs()[sname]
                t2, v2 = p.propagate_with_gp(X[:N + 1], U[:N], fresh)
                assert np.array_equal(t2, tubes[:N + 1]) and np.array_equal(v2, gp_vars[:N]), (sname, N)
    if check:
        try:
            p.propagate_with_gp(X, U, tc.StubPredict(2))
            raised = False
        except ValueError:
            raised = True
        assert raised
        out["gp_two_raises"] = np.array(raised)
        try:
            p.propagate_with_gp(X, U, tc.StubTwoArguments())
            raised = False
        except TypeError:
            raised = True
        assert raised
        cov["gp_two_argument_predict_raises"] = 1
    # Monte-Carlo tubes
    X, U = trajs["hover"]
    for n, q in tc.MC_CASES:
        for N in tc.MC_HORIZONS:
            np.random.seed(tc.mc_seed(n, q, N))
            out[f"mc_S{n}_q{q}_N{N}"] = props["hover"].propagate_monte_carlo(X[:N + 1], U[:N], None, n, q)
    names, N, n, q = tc.MC_BATCH
    np.random.seed(tc.mc_seed(n, q, N) + 1)
    out["mc_batch"] = np.array([props[nm].propagate_monte_carlo(trajs[nm][0][:N + 1], trajs[nm][1][:N], None, n, q)
                                for nm in names])
    if check:
        np.random.seed(77)
        per = np.array([[np.random.randn(14) * 0.1 for _ in range(5)] for _ in range(3)])
        np.random.seed(77)
        assert np.array_equal(per, np.random.randn(3, 5, 14) * 0.1)
        cov["block_draw_has_the_per_particle_bits"] = 1
    # tightener
    for key, w_max in tc.TIGHTEN.items():
        cfg = ref.TubeMPCConfig() if w_max is None else ref.TubeMPCConfig(w_max=w_max)
        mpc = ref.RobustTubeMPC(plant_of("tilted"), cfg)
        tubes = mpc.compute_tubes(*trajs["tilted"])
        dicts = mpc.get_tightened_constraints(tubes)
        if w_max is None:      # the default tube is the linear one already recorded
            assert not check or np.array_equal(tubes, out["lin_tilted_wmax_none"])
        else:
            out[f"tight_{key}_tubes"] = tubes
        for f in tc.TIGHT_FIELDS:
            out[f"tight_{key}_{f}"] = np.array([d[f] for d in dicts], float)
        if check:
            assert all(np.array_equal(d["tube_width"], tubes[k]) for k, d in enumerate(dicts))
            g, th = out[f"tight_{key}_gamma_gs"], out[f"tight_{key}_theta_max"]
            cov[f"{key}_gamma_untouched"] = int(np.sum(g == 30.0))
            cov[f"{key}_gamma_clamped"] = int(np.sum(g == np.rad2deg(np.deg2rad(10))))
            cov[f"{key}_gamma_tightened"] = int(np.sum((g < 30.0) & (g > np.rad2deg(np.deg2rad(10)))))
            cov[f"{key}_theta_clamped"] = int(np.sum(th == 10.0))
            cov[f"{key}_theta_tightened"] = int(np.sum((th > 10.0) & (th < 60.0)))
            cov[f"{key}_altitude_above_floor"] = int(np.sum(tubes[:, 1] > 1.0))
            cov[f"{key}_altitude_floor"] = int(np.sum(tubes[1:, 1] <= 1.0))
    return out, cov


def main(root, quick=False):
    ref = load_reference(root)
    out, cov = run_all(ref, tc.make_dynamics, True)
    print("coverage", cov, flush=True)
    # the default tube clamps both angles, the 1e-3 tube clamps nothing, step 0 is untouched
    assert cov["a_gamma_untouched"] == 1 and cov["b_gamma_untouched"] == 1, cov
    assert cov["a_gamma_clamped"] > 0 and cov["a_theta_clamped"] > 0, cov
    assert cov["b_gamma_clamped"] == 0 and cov["b_theta_clamped"] == 0, cov
    assert cov["b_gamma_tightened"] == tc.N_MAX and cov["b_theta_tightened"] == tc.N_MAX, cov
    assert cov["a_gamma_tightened"] + cov["a_gamma_clamped"] == tc.N_MAX, cov
    assert cov["a_altitude_above_floor"] > 0 and cov["a_altitude_floor"] > 0 and cov["b_altitude_floor"] > 0, cov
    for k, v in cov.items():
        out[f"coverage_{k}"] = np.array(v)
    for name in tc.TRAJECTORIES:
        out[f"traj_{name}_X"], out[f"traj_{name}_U"] = tc.nominal(name)
    out["w_vec"], out["K_dense"] = tc.W_VEC, tc.K_DENSE
    if quick:
        return
    spread = {}

    def grow(key, a, b):
        spread[key] = max(spread.get(key, 0.0), float(np.max(np.abs(np.asarray(a) - np.asarray(b)))))

    for seed in range(3):
        plants = {name: NoisyPlant(tc.make_dynamics(name), 4400 + 10 * i + seed) for i, name in enumerate(tc.TRAJECTORIES)}
        noisy, _ = run_all(ref, plants.__getitem__, False)
        for key, val in noisy.items():
            if key.startswith("lin_") or (key.startswith("gp_") and key.endswith("_tubes")):
                kind = "lin" if key.startswith("lin_") else "gp"
                for N in tc.HORIZONS:      # a horizon's tubes are the first N + 1 rows
                    grow(f"{kind}_N{N}", val[:N + 1], out[key][:N + 1])
            elif key.startswith("linz_A_") or key.startswith("linz_B_"):
                grow(key[5:], val, out[key])
            elif key.startswith("mc_"):
                grow("mc", val, out[key])
            elif key.startswith("gp_") and key.endswith("_vars"):
                assert np.array_equal(val, out[key])
    print("spreads", spread, flush=True)
    for k, v in spread.items():
        out[f"spread_{k}"] = np.array(v)
    path = os.path.join(HERE, "tube.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], quick=len(sys.argv) > 2 and sys.argv[2] == "quick")
