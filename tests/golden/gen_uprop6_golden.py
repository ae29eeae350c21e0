"""Generate f9b_uprop6.npz: the reference's own UncertaintyPropagator (src/mpc/uncertainty_prop.py,
all three methods) over the reference's own StructuredRocketGP (src/gp, exact and FITC M = 50) on
the 14-state rocket.

Needs the reference checkout and scipy; only the .npz written next to this script travels.  The
reference's modules are loaded by path under a namespace shim (gen_golden.py's) and driven with
this package's Rocket6DoFDynamics (the reference's 6-DoF class needs simdyn, which is not
installed), the arrangement of gen_tube_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_uprop6_golden.py <reference> [quick]

(quick: the cases and the coverage assertions only, no spreads, nothing written.)  The cases are
tests/uprop6_cases.py's.  Recorded per GP kind (exact / fitc):

    inducing_v / inducing_w          the FITC fit's inducing points (kmeans2 under np.random.seed(0))
    <method>_<gp>_<plant>_<s0>_means / _covs
                                     propagate() of every trajectory of the case at N = 8, stacked;
                                     monte_carlo under np.random.seed(uprop6_cases.mc_seed) immediately
                                     before each propagate(), the "batch" case two trajectories one after
                                     the other under one seed
    x0 / U / sigma0_<method> / J_full / mc_seeds
                                     the inputs, as uprop6_cases builds them

Asserted on the clean run (coverage_*): N = 1 returns the first two rows of N = 8 bit for bit for
every method, so one array serves both horizons; the second trajectory of the Monte-Carlo batch
differs from the same trajectory under the seed alone (the batch pins the draw order).

    spread_<method>_<gp>_means / _covs
        the largest change of the recorded arrays over three more runs of the reference in which X, U,
        D_v and D_omega are each multiplied elementwise by (1 + 2^-52 z) before the fit and the plant's
        ``step`` output is multiplied the same way (gen_safety_golden.py's NoisyPlant): what one
        rounding per input does to the answer.  inducing_move: the largest move of an inducing point.
    restatement_<method>_<gp>_means / _covs
        the largest distance of the numpy restatement (tests/uprop6_check.py, on
        oracle.uprop_oracle.SixDofPlant over oracle.gp_oracle fits) from the recorded arrays; asserted
        within uprop6_check's bound before
    spread_sharp_<gp>_means / _covs
        the same perturbations applied to the restatement at ut = (1, 2, 0), Sigma_0 = L L^T,
        L = 1e-2 randn: the reference hard-codes alpha = 1e-3, so the sharp transform exists only there.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import uprop6_cases as uc  # noqa: E402
import uprop6_check as chk  # noqa: E402


def load_reference(root):
    """(structured_gp, uncertainty_prop) of the reference, without its __init__ files."""
    for name, sub in (("refgp", "gp"), ("refmpc", "mpc")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(root, "src", sub)]
        sys.modules[name] = pkg
    return importlib.import_module("refgp.structured_gp"), importlib.import_module("refmpc.uncertainty_prop")


class NoisyPlant:
    """The plant with every ``step`` output multiplied by (1 + 2^-52 z)."""

    def __init__(self, base, seed):
        self._base = base
        self._rng = np.random.default_rng(seed)

    def __getattr__(self, name):
        return getattr(self._base, name)

    def step(self, x, u, dt=None):
        return self._base.step(x, u, dt) * (1.0 + 2.0 ** -52 * self._rng.standard_normal(14))


def fit_reference(sg, gpkind, data):
    cfg = sg.StructuredGPConfig(n_inducing=uc.N_INDUCING, max_data_points=uc.N_TRAIN, use_sparse=gpkind == "fitc")
    g = sg.StructuredRocketGP(cfg)
    g.add_data(*data)
    np.random.seed(uc.FIT_SEED)
    g.fit()
    return g


def run_reference(up, gp, gpkind, plant_of, check):
    """key -> (means, covs) of every case of every method; check: the clean run's assertions."""
    out, cov = {}, {}
    for method in uc.METHODS:
        for plant, s0 in uc.cases(method):
            X0, U, S0 = uc.inputs(method, s0)
            prop = up.UncertaintyPropagator(plant_of(plant), gp, method=method)
            if method == "monte_carlo" and s0 == "batch":
                np.random.seed(uc.mc_seed(plant, "batch"))
            M, C = [], []
            for b in range(len(X0)):
                if method == "monte_carlo" and s0 != "batch":
                    np.random.seed(uc.mc_seed(plant, b))
                r = prop.propagate(X0[b].copy(), U[b].copy(), None if S0 is None else S0[b].copy(), uc.DT)
                M.append(r.means); C.append(r.covariances)
            out[uc.key(method, gpkind, plant, s0)] = (np.array(M), np.array(C))
            if check and s0 != "batch":
                for b in range(len(X0)):          # N = 1 is the first step of N = 8
                    if method == "monte_carlo":
                        np.random.seed(uc.mc_seed(plant, b))
                    r = prop.propagate(X0[b].copy(), U[b, :1].copy(), None if S0 is None else S0[b].copy(), uc.DT)
                    assert np.array_equal(r.means, M[b][:2]) and np.array_equal(r.covariances, C[b][:2]), (method, plant, s0, b)
                cov[f"{method}_N1_is_a_prefix"] = 1
            if check and method == "monte_carlo" and s0 == "batch":
                b = uc.MC_BATCH[1]                # the second trajectory alone under the batch's seed: other draws
                np.random.seed(uc.mc_seed(plant, "batch"))
                r = prop.propagate(X0[1].copy(), U[1].copy(), S0[1].copy(), uc.DT)
                assert np.abs(r.means - M[1]).max() > 1e-6, (plant, b)
                cov["batch_pins_the_draw_order"] = 1
    return out, cov


def run_restatement(pred, gpkind, plant_of, methods):
    out = {}
    for method in methods:
        for plant, s0 in (uc.sharp_cases() if method == "sharp" else uc.cases(method)):
            out[uc.key(method, gpkind, plant, s0)] = chk.restate(method, plant_of(plant), pred, plant, s0)
    return out


def main(root, quick=False):
    sg, up = load_reference(root)
    data = uc.training_data()
    out = {}
    X0, U = uc.starts()
    out["x0"], out["U"], out["J_full"] = X0, U, uc.J_FULL
    for m in ("linear", "unscented", "sharp"):
        out[f"sigma0_{m}"] = uc.sigma0(m, "dense")
    out["mc_seeds"] = np.array([[uc.mc_seed(p, b) for b in (0, 1, 2, "batch")] for p in uc.PLANTS])
    for gpkind in uc.GP_KINDS:
        g = fit_reference(sg, gpkind, data)
        base, cov = run_reference(up, g, gpkind, uc.make_dynamics, True)
        print(gpkind, "coverage", cov, flush=True)
        assert all(cov.get(f"{m}_N1_is_a_prefix") for m in uc.METHODS) and cov.get("batch_pins_the_draw_order"), cov
        assert set(base) == {uc.key(m, gpkind, p, s) for m in uc.METHODS for p, s in uc.cases(m)}
        for k, v in cov.items():
            out[f"coverage_{gpkind}_{k}"] = np.array(v)
        for k, (mm, cc) in base.items():
            assert np.all(np.isfinite(mm)) and np.all(np.isfinite(cc)), k
            out[f"{k}_means"], out[f"{k}_covs"] = mm, cc
        Zv = Zw = None
        if gpkind == "fitc":
            Zv, Zw = np.array(g.gp_v.gps[0].inducing_points), np.array(g.gp_omega.gps[0].inducing_points)
            assert Zv.shape == (uc.N_INDUCING, 13) and Zw.shape == (uc.N_INDUCING, 12)
            out["inducing_v"], out["inducing_w"] = Zv, Zw
        if quick:
            continue
        # spreads of the reference
        spread, move = {}, 0.0

        def grow(key, a, b):
            spread[key] = max(spread.get(key, 0.0), float(np.max(np.abs(np.asarray(a) - np.asarray(b)))))

        perturbed = []
        for t in range(3):
            rng = np.random.default_rng(9600 + t)
            pdata = tuple(uc.perturb(rng, A) for A in data)
            g2 = fit_reference(sg, gpkind, pdata)
            Z2 = None
            if gpkind == "fitc":
                Z2 = (np.array(g2.gp_v.gps[0].inducing_points), np.array(g2.gp_omega.gps[0].inducing_points))
                move = max(move, float(np.abs(Z2[0] - Zv).max()), float(np.abs(Z2[1] - Zw).max()))
            perturbed.append((pdata, Z2))
            noisy, _ = run_reference(up, g2, gpkind, lambda p, t=t: NoisyPlant(uc.make_dynamics(p), 9700 + 10 * t + uc.PLANTS.index(p)), False)
            for k, (mm, cc) in noisy.items():
                method = k.split(f"_{gpkind}_")[0]
                grow(f"{method}_{gpkind}_means", mm, base[k][0]); grow(f"{method}_{gpkind}_covs", cc, base[k][1])
        print(gpkind, "spreads", spread, "largest move of an inducing point", move, flush=True)
        for k, v in spread.items():
            out[f"spread_{k}"] = np.array(v)
        if gpkind == "fitc":
            out["inducing_move"] = np.array(move)
        # the restatement against the recorded arrays, within the bound
        pred = chk.oracle_predictor(gpkind, Zv, Zw, data)
        rest = run_restatement(pred, gpkind, chk.oracle_plant, uc.METHODS)
        err = {}
        for k, (mm, cc) in rest.items():
            method = k.split(f"_{gpkind}_")[0]
            sm, sc = chk.shares((mm, cc), base[k], {f"spread_{a}": b for a, b in spread.items()}, method, gpkind)
            print(f"  restatement {k}: {sm:.3f} / {sc:.3f} of the bound", flush=True)
            assert sm <= 1.0 and sc <= 1.0, (k, sm, sc)
            err[f"{method}_{gpkind}_means"] = max(err.get(f"{method}_{gpkind}_means", 0.0), float(np.abs(mm - base[k][0]).max()))
            err[f"{method}_{gpkind}_covs"] = max(err.get(f"{method}_{gpkind}_covs", 0.0), float(np.abs(cc - base[k][1]).max()))
        for k, v in err.items():
            out[f"restatement_{k}"] = np.array(v)
        # the sharp transform's spread, on the restatement
        sharp = run_restatement(pred, gpkind, chk.oracle_plant, ("sharp",))
        sp = [0.0, 0.0]
        for t, (pdata, Z2) in enumerate(perturbed):
            p2 = chk.oracle_predictor(gpkind, *(Z2 or (None, None)), pdata)
            noisy = run_restatement(p2, gpkind, lambda p, t=t: NoisyPlant(chk.oracle_plant(p), 9800 + 10 * t + uc.PLANTS.index(p)), ("sharp",))
            for k in sharp:
                sp[0] = max(sp[0], float(np.abs(noisy[k][0] - sharp[k][0]).max()))
                sp[1] = max(sp[1], float(np.abs(noisy[k][1] - sharp[k][1]).max()))
        print(gpkind, "sharp spread", sp, flush=True)
        out[f"spread_sharp_{gpkind}_means"], out[f"spread_sharp_{gpkind}_covs"] = np.array(sp[0]), np.array(sp[1])
    if quick:
        return
    path = os.path.join(HERE, "f9b_uprop6.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], quick=len(sys.argv) > 2 and sys.argv[2] == "quick")
