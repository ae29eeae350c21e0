"""The 14-state uncertainty propagation against tests/golden/f9b_uprop6.npz: the bound, the
numpy restatements of the three methods on a plant and GP fits that share no code with the
package under test, and the mutants of the restatement that show what the bound can see.

Shared by tests/golden/gen_uprop6_golden.py (the sharp transform's spread, measured on the
restatement), tests/test_uprop6_check.py (no GPU: restatement and mutants against the
reference's own output) and tests/test_gpu_uprop6_reference.py (the device recursions).

The bound, for one method, GP kind and field (means / covariances), entrywise:

    |got - want| <= 16 * spread + 8 * ulp(want)

spread is f9b's spread_<method>_<gpkind>_<field>: the largest change of the reference's own
output when its training data and every plant step are multiplied by (1 + 2^-52 z), i.e. what
one rounding per input does to the answer.  Neither the device nor the package's host loop
takes part in it.  The factor is 16: an independent float64 implementation (the restatement)
lands at 0.01-1.2 x spread (f9b's restatement_* keys; test_uprop6_check.py prints it as a
share of the bound, 0.075 at most), the device adds another summation order of the GP mean
and FMA contraction, each of the size of the one-rounding perturbation, and the mildest
mutant below (sigma points from the factor's rows, at alpha = 1e-3) is 12.7 x outside the
bound in the means and 1e5 x in the covariances; nothing measured asks for another factor.

Every mutant is rejected on a case the fixture holds.  One needed a case of its own: the
linear recursion meets the quaternion's renormalisation only in the mean of a unit quaternion,
where RK4's norm error at the starts' body rates (~0.05 rad/s) is below one rounding, so
uprop6_cases has the "spin" start (|omega| = 3.5 rad/s) for it.

The restatements: oracle.uprop_oracle.propagate_linear, uprop_ut_check.propagate_unscented and
uprop_mc_check.propagate_mc on oracle.uprop_oracle.SixDofPlant, over oracle.gp_oracle fits
(structured_exact_predictor / structured_fitc_predictor on the fixture's inducing points).
"""
import numpy as np

import uprop6_cases as uc
import uprop_mc_check
import uprop_ut_check
from oracle import gp_oracle, sixdof_oracle, uprop_oracle

FACTOR = 16.0


def bound(want, spread):
    return FACTOR * float(spread) + 8.0 * np.spacing(np.abs(np.asarray(want, float)))


def share(got, want, spread):
    """The largest |got - want| / bound: <= 1 passes."""
    want = np.asarray(want, float)
    return float(np.max(np.abs(np.asarray(got, float) - want) / bound(want, spread)))


def spreads(fix, method, gpkind):
    return float(fix[f"spread_{method}_{gpkind}_means"]), float(fix[f"spread_{method}_{gpkind}_covs"])


def shares(got, want, fix, method, gpkind):
    """(share of the means' bound, share of the covariances' bound)."""
    sm, sc = spreads(fix, method, gpkind)
    return share(got[0], want[0], sm), share(got[1], want[1], sc)


# ---- the plant and the GP of the restatement -----------------------------------------------
def rocket_params(plant):
    rc = uc.rocket_config(plant)
    return sixdof_oracle.rocket_params(np.asarray(rc.J_B, float), rc.r_T_B, rc.g_I, rc.I_sp, rc.g0)


def oracle_plant(plant):
    return uprop_oracle.SixDofPlant(rocket_params(plant))


def oracle_predictor(gpkind, Zi_v=None, Zi_w=None, data=None):
    X, U, Dv, Dw = data or uc.training_data()
    if gpkind == "exact":
        return uprop_oracle.structured_exact_predictor(X, U, Dv, Dw)
    return uprop_oracle.structured_fitc_predictor(Zi_v, Zi_w, X, U, Dv, Dw)


def fixture_predictor(fix, gpkind):
    return oracle_predictor(gpkind, fix["inducing_v"], fix["inducing_w"])


# ---- one case through the restatement --------------------------------------------------------
def restate(method, plant_obj, pred, plant, s0, N=uc.N, ut=None, factor=np.linalg.cholesky,
            weights=uprop_ut_check.ut_weights, swap_draws=False, divide_by_S=False, particles=False, inputs_of=None):
    """means (b, N+1, 14), covs (b, N+1, 14, 14) of case (method, plant, s0) at horizon N; method
    "sharp" is the unscented transform at SHARP_UT (or ``ut``).  With particles also the
    Monte-Carlo paths (b, N+1, S, 14).  inputs_of: the method whose Sigma_0 the case takes."""
    X0, U, S0 = uc.inputs(inputs_of or method, s0)
    U = U[:, :N]
    M, C, P = [], [], []
    if method == "monte_carlo" and s0 == "batch":
        np.random.seed(uc.mc_seed(plant, "batch"))
    for b in range(len(X0)):
        S0b = None if S0 is None else S0[b]
        if method == "linear":
            m, c = uprop_oracle.propagate_linear(plant_obj, pred, X0[b], U[b], S0b, uc.DT)
        elif method in ("unscented", "sharp"):
            par = ut or (uc.SHARP_UT if method == "sharp" else uprop_ut_check.REFERENCE_UT)
            m, c = uprop_ut_check.propagate_unscented(plant_obj, pred, X0[b], U[b], S0b, uc.DT, par,
                                                      factor=factor, weights=weights)
        else:
            if s0 != "batch":
                np.random.seed(uc.mc_seed(plant, b))
            p0, z = uprop_mc_check.draw(X0[b], S0b, N, uc.N_SAMPLES, 2)
            if swap_draws:
                z = z[:, :, ::-1]
            m, c, paths = uprop_mc_check.propagate_mc(plant_obj, pred, p0, z, U[b], uc.DT, X0[b], S0b)
            if divide_by_S:
                c[1:] *= (uc.N_SAMPLES - 1) / uc.N_SAMPLES
            P.append(paths)
        M.append(m); C.append(c)
    out = (np.array(M), np.array(C))
    return out + (np.array(P),) if particles else out


# ---- mutants ---------------------------------------------------------------------------------
class _Plant(uprop_oracle.SixDofPlant):
    """SixDofPlant with one thing wrong."""

    def __init__(self, rk, no_norm=False, a_at_next=False):
        super().__init__(rk)
        self.no_norm, self.a_at_next = no_norm, a_at_next

    def step(self, x, u, dt):
        if not self.no_norm:
            return super().step(x, u, dt)
        x = np.asarray(x, float); f = sixdof_oracle.f
        k1 = f(x, u, self.rk); k2 = f(x + dt * k1 / 2, u, self.rk)
        k3 = f(x + dt * k2 / 2, u, self.rk); k4 = f(x + dt * k3, u, self.rk)
        return x + (dt / 6) * (k1 + 2 * k2 + 2 * k3 + k4)

    def linearize(self, x, u, dt=0.1):
        return super().linearize(super().step(x, u, dt) if self.a_at_next else x, u, dt)


def _pred_mutant(pred, plant_obj, kind):
    def predict(x, u):
        dv, dw, vv, vw = pred(x, u)
        if kind == "no_noise_w":
            vw = np.zeros(3)
        elif kind == "var_dt":
            vv, vw = vv / uc.DT, vw / uc.DT          # var dt instead of var dt^2
        elif kind == "var_at_next":
            xn = plant_obj.step(x, u, uc.DT).copy()
            xn[4:7] += dv * uc.DT; xn[11:14] += dw * uc.DT
            _, _, vv, vw = pred(xn, u)
        elif kind == "fitc_corrected_mean":
            sv, sw = pred.states
            x2 = np.atleast_2d(x); u2 = np.atleast_2d(u)
            dv = sixdof_oracle.fitc_mean(sv, gp_oracle.features_translational(x2, u2), corrected=True)[0]
            dw = sixdof_oracle.fitc_mean(sw, gp_oracle.features_rotational(x2, u2), corrected=True)[0]
        return dv, dw, vv, vw
    return predict


def _wc0_without_correction(n, ut):
    lam, w_m, w_c = uprop_ut_check.ut_weights(n, ut)
    w_c[0] = w_m[0]
    return lam, w_m, w_c


# name -> (what is wrong, the cases (method, gpkind, plant, s0) it is judged on)
MUTANTS = {
    "no_noise_w": ("no process noise on rows 11:14", [("linear", "exact", "diag", "none"), ("unscented", "fitc", "diag", "none")]),
    "var_dt": ("var dt instead of var dt^2", [("linear", "fitc", "diag", "none"), ("unscented", "exact", "diag", "dense")]),
    "var_at_next": ("the variance taken at x_{k+1} (unscented: at the propagated centre) instead of x_k",
                    [("linear", "exact", "diag", "none"), ("unscented", "exact", "diag", "none"),
                     ("monte_carlo", "exact", "diag", "none")]),
    "no_quat_norm": ("the quaternion not renormalised after RK4",
                     [("linear", "exact", "diag", "spin"), ("unscented", "fitc", "diag", "none"),
                      ("monte_carlo", "fitc", "diag", "none")]),
    "a_at_next": ("A_k evaluated at x_{k+1}", [("linear", "fitc", "diag", "dense")]),
    "inv_diag_J": ("J^-1 replaced by 1 / diag(J)", [("linear", "fitc", "full", "dense"), ("unscented", "exact", "full", "dense"),
                                                    ("monte_carlo", "fitc", "full", "batch")]),
    "fitc_corrected_mean": ("the corrected FITC mean instead of the one as written",
                            [("linear", "fitc", "diag", "none"), ("unscented", "fitc", "diag", "dense"),
                             ("monte_carlo", "fitc", "diag", "batch")]),
    "chol_rows": ("sigma points from the rows of the Cholesky factor", [("unscented", "exact", "diag", "dense"),
                                                                       ("sharp", "fitc", "full", "dense")]),
    "wc0": ("w_c[0] without (1 - alpha^2 + beta)", [("sharp", "exact", "diag", "dense"), ("sharp", "fitc", "full", "dense")]),
    "swap_draws": ("the d_v and d_omega draws swapped", [("monte_carlo", "exact", "diag", "none"),
                                                        ("monte_carlo", "fitc", "full", "batch")]),
    "div_S": ("division by S instead of S - 1", [("monte_carlo", "exact", "diag", "none"), ("monte_carlo", "fitc", "diag", "batch")]),
}


def mutant(name, method, plant, pred, N=uc.N, s0="none"):
    """Case (method, plant, s0) through the restatement with mutant ``name`` applied."""
    rk = rocket_params(plant)
    if name == "inv_diag_J":
        assert "Jf" in rk
        rk = dict(rk, Ji=np.diag(1.0 / np.diag(rk["Jf"])))
    po = _Plant(rk, no_norm=name == "no_quat_norm", a_at_next=name == "a_at_next")
    kw = {}
    if name in ("no_noise_w", "var_dt", "var_at_next", "fitc_corrected_mean"):
        pred = _pred_mutant(pred, po, name)
    elif name == "chol_rows":
        kw["factor"] = lambda A: np.linalg.cholesky(A).T
    elif name == "wc0":
        kw["weights"] = _wc0_without_correction
    elif name == "swap_draws":
        kw["swap_draws"] = True
    elif name == "div_S":
        kw["divide_by_S"] = True
    return restate(method, po, pred, plant, s0, N, **kw)


# ---- the device runs of tests/test_gpu_uprop6_reference.py -----------------------------------
def gpu_runs():
    """(method, gpkind, plant, s0, N, form) of every device call the GPU tests make.  form:
    "batch" (all trajectories of the case in one call) or "single" (each alone at B = 1; for
    monte_carlo through propagate() under the trajectory's own seed)."""
    runs = []
    for gpkind in uc.GP_KINDS:
        for plant, s0 in uc.cases("linear"):
            runs += [("linear", gpkind, plant, s0, N, form) for N in uc.HORIZONS for form in ("batch", "single")]
        for plant, s0 in uc.cases("unscented"):
            runs += [("unscented", gpkind, plant, s0, N, "batch") for N in uc.HORIZONS]
        runs += [("sharp", gpkind, plant, s0, uc.N, "batch") for plant, s0 in uc.sharp_cases()]
        for plant, s0 in uc.cases("monte_carlo"):
            runs.append(("monte_carlo", gpkind, plant, s0, uc.N, "batch" if s0 == "batch" else "single"))
    return runs


def device_run(p, method, plant, s0, N, form, particles=False):
    """One gpu_runs() entry through the propagator p (this package's UncertaintyPropagator, its
    method already set) -> (means, covs[, particles]) stacked over the case's trajectories."""
    X0, U, S0 = uc.inputs(method, s0)
    U = U[:, :N]
    if method == "monte_carlo":
        if form == "batch":
            np.random.seed(uc.mc_seed(plant, "batch"))
            return p.propagate_monte_carlo_batch(X0, U, S0, uc.DT, uc.N_SAMPLES, return_particles=particles)
        M, C = [], []
        for b in range(len(X0)):
            np.random.seed(uc.mc_seed(plant, b))
            r = p.propagate(X0[b], U[b], None if S0 is None else S0[b], uc.DT)
            M.append(r.means); C.append(r.covariances)
        return np.array(M), np.array(C)
    batch = p.propagate_batch if method == "linear" else p.propagate_unscented_batch
    if form == "batch":
        return batch(X0, U, S0, uc.DT)
    M, C = [], []
    for b in range(len(X0)):
        r = p.propagate(X0[b], U[b], None if S0 is None else S0[b], uc.DT)
        M.append(r.means); C.append(r.covariances)
    return np.array(M), np.array(C)


def device_calls(runs_entry):
    """How many uprop6_* calls device_run makes for the entry."""
    method, _, _, s0, _, form = runs_entry
    return 1 if form == "batch" else len(uc.inputs(method, s0)[0])
