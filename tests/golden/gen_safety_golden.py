"""Generate safety.npz from the reference's own src/safety modules.

Needs the reference checkout and scipy; only the .npz written next to this script travels.
The reference's four modules are loaded by file path under a synthetic package and driven with
this package's Rocket6DoFDynamics (the reference's 6-DoF class needs simdyn, which is not
installed):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_safety_golden.py <reference> [quick]

(quick: coverage only, no spreads, nothing written.)  The configurations A-D are
tests/safety_cases.py's.  Per configuration a list of (x, u_nominal) cases, built by category
(near the equilibrium, thrust too low / too high, tilted, outside the glideslope, below 0.1 of
altitude, just outside and far outside the ellipsoid, nominal controls of small norm), and per
case from PredictiveSafetyFilter.filter: u_safe, is_modified, is_safe, safety_margin,
backup_value, the violation keys as a mask (bit 0 "immediate", bit 1 + k "path_k"), and the
gradient iterations taken, counted by an instrumented copy of _solve_gradient_qp that is
asserted to return the reference's u_safe bit for bit.

Also recorded: a closed loop (simulate_filtered, T = 5, three starts of configuration B), and
small values of the backup controller and the invariant set (saturated controls, contains /
get_value / project, compute_maximal_alpha under np.random.seed).

Asserted and stored as ``coverage_*`` (the seeds were changed until the reference alone
satisfied every item): the four outcomes (unmodified and safe; modified with 0 iterations;
modified with an early exit, ending safe; modified with 50 iterations, still unsafe), at least
three distinct early-exit counts, both projections of the gradient loop, every constraint test
failing somewhere (thrust low, thrust high, tilt, glideslope, a path_k with k >= 1), a case at
altitude <= 0.1, saturation by u_min / u_max inside a rollout, and sixteen cases of B
(``mix_idx``) that put a safe, an early-exit and a 50-iteration query into one wave.

Two measured quantities:

    spread_u / spread_margin / spread_value (and sim_spread_X / sim_spread_U for the closed
        loop): the largest change of the recorded numbers over three more runs of the reference
        with a plant whose ``step`` output is multiplied by (1 + 2^-52 z), z standard normal:
        what one rounding per step does to the answer (the finite difference divides rounding
        noise by 1e-4, fifty times over).
    decision_gap_*: the smallest distance of any discrete decision from its threshold over all
        cases and iterations: V_j against 0.9 alpha (gap_v) and the margin against 0
        (gap_margin), both compared with spread_value / spread_margin; |u| against T_min and
        T_max, cos theta against its bound, the glideslope inequality and the altitude against
        0.1 in every constraint test (gap_constraint), compared with spread_u (the tested
        states depend on the control through one step: |dx| <= dt |du| / m).  Every gap is
        asserted >= 1000 x its spread, so flags, masks and counts do not depend on rounding.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import safety_cases as sc  # noqa: E402

SIM_T, SIM_B = 5, 3


def load_reference(root):
    """The reference's safety package without its __init__."""
    pkg_dir = os.path.join(root, "src", "safety")
    pkg = types.ModuleType("ref_safety")
    pkg.__path__ = [pkg_dir]
    sys.modules["ref_safety"] = pkg
    mods = {}
    for name in ("backup_controller", "invariant_sets", "tube_mpc", "safety_filter"):
        spec = importlib.util.spec_from_file_location(f"ref_safety.{name}", os.path.join(pkg_dir, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    assert not mods["safety_filter"].HAS_CASADI
    return mods


class NoisyPlant:
    """The plant with every ``step`` output multiplied by (1 + 2^-52 z)."""

    def __init__(self, base, seed):
        self._base = base
        self._rng = np.random.default_rng(seed)

    def __getattr__(self, name):
        return getattr(self._base, name)

    def step(self, x, u, dt=None):
        return self._base.step(x, u, dt) * (1.0 + 2.0 ** -52 * self._rng.standard_normal(14))


def quat_tilt(angle, axis):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def state(rng, r_scale, v_scale, mass=None, q=None, w_scale=0.05):
    x = sc.X_EQ.copy()
    x[0] = 1.5 + 0.5 * rng.random() if mass is None else mass
    x[1:4] = r_scale * rng.standard_normal(3)
    x[1] = abs(x[1])
    x[4:7] = v_scale * rng.standard_normal(3)
    qq = np.array([1.0, 0, 0, 0]) + 0.03 * rng.standard_normal(4) if q is None else np.asarray(q, float)
    x[7:11] = qq / np.linalg.norm(qq)
    x[11:14] = w_scale * rng.standard_normal(3)
    return x


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def cases(name, rng):
    """(X, U) of configuration ``name`` by category."""
    X, U = [], []

    def add(x, u):
        X.append(x); U.append(np.asarray(u, float))

    hover = sc.U_EQ
    if name in ("A", "C"):
        n = {"A": (8, 4, 3, 4, 4, 3, 10), "C": (3, 2, 1, 2, 2, 1, 3)}[name]
        for _ in range(n[0]):   # near the equilibrium
            add(state(rng, 0.04, 0.04), hover + 0.1 * rng.standard_normal(3))
        for _ in range(n[1]):   # thrust too low
            add(state(rng, 0.04, 0.04), (0.15 + 0.3 * rng.random()) * unit(rng))
        for _ in range(n[2]):   # thrust too high
            add(state(rng, 0.04, 0.04), (5.3 + rng.random()) * np.array([1.0, 0.05, -0.05]))
        for _ in range(n[3]):   # tilted past theta_max
            add(state(rng, 0.04, 0.04, q=quat_tilt(np.deg2rad(62 + 20 * rng.random()), [rng.random(), 1.0, 0.0])),
                hover + 0.1 * rng.standard_normal(3))
        for _ in range(n[4]):   # outside the glideslope, above 0.1
            x = state(rng, 0.02, 0.03)
            x[1] = 0.12 + 0.1 * rng.random()
            phi = 6.28 * rng.random()
            x[2:4] = x[1] * (0.7 + 0.3 * rng.random()) * np.array([np.cos(phi), np.sin(phi)])
            add(x, hover + 0.1 * rng.standard_normal(3))
        for _ in range(n[5]):   # at or below 0.1 of altitude, far off the axis
            x = state(rng, 0.02, 0.03)
            x[1] = 0.09 * rng.random()
            x[2:4] = [0.12, -0.1]
            add(x, hover + 0.1 * rng.standard_normal(3))
        for _ in range(n[6]):   # outside the ellipsoid
            add(state(rng, 0.25, 0.3), hover + 0.5 * rng.standard_normal(3))
    else:
        for _ in range(6):      # near the equilibrium
            add(state(rng, 0.04, 0.008, mass=2.0 if name == "D" else None), hover + 0.05 * rng.standard_normal(3))
        for i in range(12):     # just outside: the velocity weights of 400 make one control step count
            add(state(rng, 0.05, 0.02 + 0.004 * i, mass=2.0 + 0.01 * rng.standard_normal() if name == "D" else None),
                hover + 0.3 * rng.standard_normal(3))
        for _ in range(6):      # nominal controls of small norm
            add(state(rng, 0.05, 0.03, mass=2.0 if name == "D" else None), (0.55 + 0.3 * rng.random()) * unit(rng))
        for _ in range(8):      # far outside
            add(state(rng, 0.3, 0.3), hover + 1.5 * rng.standard_normal(3))
    return np.array(X), np.array(U)


class Gaps:
    def __init__(self):
        self.v = self.margin = self.constraint = np.inf


def constraint_gaps(f, x, u, gaps):
    """The distances of _check_constraints' comparisons from their thresholds (all of them,
    also those the reference's early returns skip) -> which tests fail."""
    if f.constraint_params is None:
        return ()
    cp = f.constraint_params
    T = np.linalg.norm(u)
    ct = 1 - 2 * (x[8] ** 2 + x[9] ** 2)
    cb = np.cos(np.deg2rad(cp.theta_max))
    t2 = np.tan(np.deg2rad(cp.gamma_gs)) ** 2
    g = [abs(T - cp.T_min), abs(T - cp.T_max), abs(ct - cb), abs(x[1] - 0.1)]
    fails = []
    if T < cp.T_min:
        fails.append("low")
    if T > cp.T_max:
        fails.append("high")
    if ct < cb:
        fails.append("tilt")
    if x[1] > 0.1:
        g.append(abs(x[1] ** 2 * t2 - (x[2] ** 2 + x[3] ** 2)))
        if x[1] ** 2 * t2 < x[2] ** 2 + x[3] ** 2:
            fails.append("glideslope")
    gaps.constraint = min(gaps.constraint, min(g))
    return tuple(fails)


def check_rollout(f, x, u, gaps, cov):
    """The comparisons of _check_safety's trajectory; saturation inside it."""
    Xp = f._predict_with_backup(x, u)
    for k, xk in enumerate(Xp[:-1]):
        uk = f.backup.get_control(xk) if k > 0 else u
        if k > 0:
            raw = f.backup.u_eq - f.backup.K @ (xk - f.backup.x_eq)
            cov["saturation"] += int(np.any(raw != uk))
        fails = constraint_gaps(f, xk, uk, gaps)
        for name in fails:
            cov[name] += 1
        if k >= 1 and fails:
            cov["path_k_ge_1"] += 1
        if k == 0 and x[1] <= 0.1:
            cov["low_altitude"] += 1
    gaps.margin = min(gaps.margin, abs(f.invariant_set.alpha - f.invariant_set.get_value(Xp[-1])))


def gradient_qp(f, x, u_nominal, gaps, cov, n_iters=50, lr=0.1):
    """_solve_gradient_qp with a counter, the decision gaps and the projection hits."""
    u = u_nominal.copy()
    iters = 0
    for _ in range(n_iters):
        V = f.invariant_set.get_value(f._predict_with_backup(x, u)[-1])
        thr = f.invariant_set.alpha * f.config.backup_margin
        gaps.v = min(gaps.v, abs(V - thr))
        if V <= thr:
            break
        eps = 1e-4
        grad = np.zeros(3)
        for i in range(3):
            up = u.copy()
            up[i] += eps
            grad[i] = (f.invariant_set.get_value(f._predict_with_backup(x, up)[-1]) - V) / eps
        u = u - lr * (grad + 2 * (u - u_nominal))
        cp = f.constraint_params
        T_min = getattr(cp, "T_min", 0.5) if cp else 0.5
        T_max = getattr(cp, "T_max", 5.0) if cp else 5.0
        T = np.linalg.norm(u)
        if T < T_min:
            u = u / max(T, 1e-6) * T_min
            cov["project_low"] += 1
        elif T > T_max:
            u = u / T * T_max
            cov["project_high"] += 1
        iters += 1
    return u, iters


def mask_of(violations):
    m = 1 if "immediate" in violations else 0
    for k in violations:
        if k.startswith("path_"):
            m |= 1 << (1 + int(k[5:]))
    return m


def record(f, x, u, gaps, cov):
    """One reference filter call -> its fields, with the instrumented loop beside it."""
    r = f.filter(x, u)
    check_rollout(f, x, u, gaps, cov)
    iters = 0
    if r.is_modified:
        u2, iters = gradient_qp(f, x, u, gaps, cov)
        assert np.array_equal(u2, r.u_safe), "the instrumented loop left the reference's bits"
        check_rollout(f, x, r.u_safe, gaps, cov)
    return r, iters


def main(root, quick=False):
    ref = load_reference(root)["safety_filter"]
    out = {}
    gaps = Gaps()
    cov = {k: 0 for k in ("low", "high", "tilt", "glideslope", "path_k_ge_1", "low_altitude", "saturation",
                          "project_low", "project_high")}
    outcome = {"safe": 0, "modified_0": 0, "early_exit_safe": 0, "full_unsafe": 0}
    early = set()
    spreads = {"u": 0.0, "margin": 0.0, "value": 0.0}
    per_cfg = {}
    for ci, name in enumerate(sc.CONFIGS):
        sp = sc.spec(name)
        f = sc.make_filter(sp, ref)
        X, U = cases(name, np.random.default_rng(7100 + ci))
        n = len(X)
        res = dict(u_safe=np.zeros((n, 3)), is_modified=np.zeros(n, bool), is_safe=np.zeros(n, bool),
                   margin=np.zeros(n), value=np.zeros(n), mask=np.zeros(n, np.int64), iters=np.zeros(n, np.int32))
        sat0 = cov["saturation"]
        for i in range(n):
            r, it = record(f, X[i], U[i], gaps, cov)
            res["u_safe"][i], res["is_modified"][i], res["is_safe"][i] = r.u_safe, r.is_modified, r.is_safe
            res["margin"][i], res["value"][i] = r.safety_margin, r.backup_value
            res["mask"][i], res["iters"][i] = mask_of(r.constraint_violations), it
            if not r.is_modified:
                outcome["safe"] += 1
            elif it == 0:
                outcome["modified_0"] += 1
            elif it < 50 and r.is_safe:
                outcome["early_exit_safe"] += 1
                early.add(it)
            elif it == 50 and not r.is_safe:
                outcome["full_unsafe"] += 1
        if name != "D":
            assert cov["saturation"] == sat0
        print(name, n, "iters", res["iters"].tolist(), "modified", int(res["is_modified"].sum()), "safe",
              int(res["is_safe"].sum()), flush=True)
        for k, v in sp.items():
            out[f"{name}_{k}"] = v
        out[f"{name}_X"], out[f"{name}_U"] = X, U
        for k, v in res.items():
            out[f"{name}_{k}"] = v
        per_cfg[name] = (sp, X, U, res)
        if not quick:
            for seed in range(3):
                fn = sc.make_filter(sp, ref, dynamics=NoisyPlant(sc.make_dynamics(sp), 900 + 10 * ci + seed))
                for i in range(n):
                    r = fn.filter(X[i], U[i])
                    spreads["u"] = max(spreads["u"], float(np.max(np.abs(r.u_safe - res["u_safe"][i]))))
                    spreads["margin"] = max(spreads["margin"], abs(r.safety_margin - res["margin"][i]))
                    spreads["value"] = max(spreads["value"], abs(r.backup_value - res["value"][i]))

    # one wave of B with a safe, an early-exit and a 50-iteration quad
    it_b, mod_b = per_cfg["B"][3]["iters"], per_cfg["B"][3]["is_modified"]
    kinds = [np.where(~mod_b)[0], np.where(mod_b & (it_b > 0) & (it_b < 50))[0], np.where(it_b == 50)[0]]
    assert all(len(k) for k in kinds), [len(k) for k in kinds]
    mix = [int(k[0]) for k in kinds]
    mix += [i for i in range(len(it_b)) if i not in mix][:16 - len(mix)]
    out["mix_idx"] = np.array(sorted(mix[:3]) + mix[3:], np.int32)

    # the closed loop
    sp, Xb, Ub, resb = per_cfg["B"]
    f = sc.make_filter(sp, ref)
    starts = [int(kinds[1][0]), int(kinds[1][-1]), int(kinds[2][0])]
    rng = np.random.default_rng(7200)
    sim_U_nom = np.tile(Ub[starts][:, None, :], (1, SIM_T, 1)) + 0.1 * rng.standard_normal((SIM_B, SIM_T, 3))
    sim = dict(X=np.zeros((SIM_B, SIM_T + 1, 14)), U=np.zeros((SIM_B, SIM_T, 3)), is_modified=np.zeros((SIM_B, SIM_T), bool),
               is_safe=np.zeros((SIM_B, SIM_T), bool), margin=np.zeros((SIM_B, SIM_T)),
               iters=np.zeros((SIM_B, SIM_T), np.int32))
    for b in range(SIM_B):
        Xs, Us, results = f.simulate_filtered(Xb[starts[b]], sim_U_nom[b])
        sim["X"][b], sim["U"][b] = Xs, Us
        for k, r in enumerate(results):
            r2, it = record(f, Xs[k], sim_U_nom[b, k], gaps, cov)
            assert np.array_equal(r2.u_safe, r.u_safe)
            sim["is_modified"][b, k], sim["is_safe"][b, k] = r.is_modified, r.is_safe
            sim["margin"][b, k], sim["iters"][b, k] = r.safety_margin, it
    out["sim_X0"], out["sim_U_nom"] = Xb[starts], sim_U_nom
    for k, v in sim.items():
        out[f"sim_{k}"] = v
    print("closed loop iters", sim["iters"].tolist(), flush=True)
    sim_spread = {"X": 0.0, "U": 0.0}
    if not quick:
        for seed in range(3):
            fn = sc.make_filter(sp, ref, dynamics=NoisyPlant(sc.make_dynamics(sp), 990 + seed))
            for b in range(SIM_B):
                Xs, Us, results = fn.simulate_filtered(Xb[starts[b]], sim_U_nom[b])
                sim_spread["X"] = max(sim_spread["X"], float(np.max(np.abs(Xs - sim["X"][b]))))
                sim_spread["U"] = max(sim_spread["U"], float(np.max(np.abs(Us - sim["U"][b]))))
                d = max(abs(r.safety_margin - sim["margin"][b, k]) for k, r in enumerate(results))
                spreads["margin"], spreads["value"] = max(spreads["margin"], d), max(spreads["value"], d)

    # small values of the backup controller and the invariant set (configuration D: a box, a full P)
    f = sc.make_filter(sc.spec("D"), ref)
    Xd = per_cfg["D"][1][-8:]    # the far cases: the box is active
    out["misc_get_control"] = f.backup.get_control_batch(Xd)
    out["misc_value"] = np.array([f.invariant_set.get_value(x) for x in Xd])
    out["misc_contains"] = np.array([bool(f.invariant_set.contains(x)) for x in Xd])
    out["misc_project"] = np.array([f.invariant_set.project(x) for x in Xd])
    out["misc_backup_value"] = np.array([f.backup.get_value_function(x) for x in Xd])
    Xs, Us = f.backup.simulate_backup(Xd[0], n_steps=4)
    out["misc_simulate_backup_X"], out["misc_simulate_backup_U"] = Xs, Us
    fa = sc.make_filter(sc.spec("A"), ref)
    np.random.seed(20240)
    out["misc_maximal_alpha"] = np.array(fa.invariant_set.compute_maximal_alpha(
        lambda x: fa._check_constraints(x, fa.backup.get_control(x)), n_samples=200))
    np.random.seed(20241)
    out["misc_boundary"] = fa.invariant_set.get_boundary_points(5)

    print("outcomes", outcome, "early exits", sorted(early), "coverage", cov, flush=True)
    print("gaps", gaps.v, gaps.margin, gaps.constraint, "spreads", spreads, sim_spread, flush=True)
    assert all(v > 0 for v in outcome.values()), outcome
    assert len(early) >= 3, early
    assert all(v > 0 for v in cov.values()), cov
    for k, v in {**outcome, **cov}.items():
        out[f"coverage_{k}"] = np.array(v)
    out["coverage_early_exit_counts"] = np.array(sorted(early), np.int32)
    if quick:
        return
    assert gaps.v >= 1000 * spreads["value"] and gaps.margin >= 1000 * spreads["margin"], (gaps.v, gaps.margin, spreads)
    assert gaps.constraint >= 1000 * spreads["u"], (gaps.constraint, spreads)
    out["spread_u"], out["spread_margin"], out["spread_value"] = (np.array(spreads[k]) for k in ("u", "margin", "value"))
    out["sim_spread_X"], out["sim_spread_U"] = np.array(sim_spread["X"]), np.array(sim_spread["U"])
    out["decision_gap_v"], out["decision_gap_margin"] = np.array(gaps.v), np.array(gaps.margin)
    out["decision_gap_constraint"] = np.array(gaps.constraint)
    path = os.path.join(HERE, "safety.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], quick=len(sys.argv) > 2 and sys.argv[2] == "quick")
