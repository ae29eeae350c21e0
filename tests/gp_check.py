"""References, cases and the pass/fail rules for the GP layer of csrc/gp.hip, in numpy.

Shared by tests/test_gp_check.py (no GPU: the rules accept a float64 restatement of what
gp.hip does and oracle/gp_oracle.py, and reject subtly wrong ones) and tests/test_gpu_gp.py
(ExactGPHandle, FITCHandle, gp_lml_batched and append on the device).  The layer under test
is the glue around the Gram, GEMM and Cholesky building blocks (which have their own
checkers): k_normalise, k_lml_exact, k_lml_fitc, k_lml_vfe, k_lml_trsv, k_fitc_lambda,
k_fitc_yl, k_scale_cols, k_colsumsq, k_post_finish, k_fitc_finish, k_fitc_post_small and the
host sequences exact_fit, sparse_fit, vfe_tail, gpmpc_gp_predict_cov, gpmpc_gp_lml_batched,
gpmpc_gp_append.

References.  np.longdouble throughout: the Gram from gram_check's direct-difference form, a
plain column Cholesky, the two substitutions, and the formulas of oracle/gp_oracle.py as
written (exact_fit, exact_predict, exact_predict_cov, fitc_fit, vfe_fit, fitc_predict,
lml_at): the population std with "std < 1e-10 -> 1", the variance clamp at 1e-10, the Lambda
clamp, the sparse mean K*u alpha "as written".  The jitter ladder takes the fp64 ladder
values (1e-6, then *= 10 in fp64) and the reference's own longdouble Cholesky decides the
step.  References are cached per case (functools.lru_cache on the case builders).

Restatement.  restate_exact / restate_sparse / restate_append / restate_lml are float64
numpy restatements of what gp.hip does where it differs from LAPACK: W = L^-1 formed
explicitly (chol_check.restate_tri_inverse for n > 128, restate_trsm on the identity
otherwise), alpha through W with one refinement step (restate_cho_solve_inv), var from
|W k*|^2 summed as per-row-tile partials (gemm_row_tiles), FITC's w = W2 k* with
W2 = L_B^-1 L_uu^-1, and the append's block update as the comment above gpmpc_gp_append
gives it (alpha = W^T (W y), no refinement).  The constants below were measured on it and on
gp_oracle; it carries the hooks (mut=...) for the wrong variants of tests/test_gp_check.py.

Rules of type (a): derived, free of any condition number.  u = 2^-53, t = ceil(n / 256) the
terms one thread of the 256-thread strided loop adds; block_sum adds 6 shuffle levels and 4
wave sums, so an n-term sum carries at most t + 10 roundings on any path.
* y_mean: the sum, then the division: |m^ - m| <= (t + 12) u mean|y|.
* y_std: sd = sqrt(sum (y - m^)^2 / n).  Each term has 3 relative roundings (difference,
  square, add), the sum t + 10, the division and the square root 1.5 more, all halved by the
  square root; the error of m^ enters through sum (y - m)^2 + n (m - m^)^2 only in second
  order.  |sd^ - sd| <= (t + 20) u sd (a factor 2 above the count).  Where the reference's
  std is below 1e-10 both sides must be exactly 1.
* The exact fit's lml from the device's own state: with L^ and alpha^ as state() returns
  them and yn = (Y - m^) / sd^ in longdouble from the device's own mean and std,
      l = -1/2 sum yn_i alpha^_i - sum log L^_ii - (n / 2) log 2 pi     (longdouble)
      |lml^ - l| <= u ((t + 16) / 2 sum |yn_i alpha^_i| + (t + 14) sum |log L^_ii|
                       + 4 (n / 2) log 2 pi + 2 |l|):
  the device's yn has two roundings per element and the product one (3, + t + 10 + the final
  scaling); log is good to one ulp = 2u, + t + 10 for the sum; the constant term is three
  roundings and a log; the final sum of three terms rounds twice relative to partial sums
  that |l| plus the other terms bound.  The same rule holds for an appended handle: the
  append runs k_lml_exact on its grown L and alpha.  These rules pin k_normalise and
  k_lml_exact at any conditioning.

Rules of type (b): forward error against the longdouble reference,
    |q^ - q_ref| <= c N u kappa s_q,
N the order of the factorised matrix, kappa the 2-norm condition number (fp64, from the
reference matrix) of K + (noise + jitter) I for the exact GP and the larger of those of
K_uu + jitter I and B for the sparse ones, and s_q the natural scale of q: alpha: max
|alpha_ref| of the column; mean: ystd (|k*| . |alpha_ref|); var: max(lat_ref, sigma2) ystd^2
(the VFE predict body gives latent variances of many sigma2); lml: |lml_ref|; cov: sigma2;
Lambda: sigma2 + |noise|; L of an appended handle: max |L_ref|.  One c per family: the
smallest power of two at which both gp_oracle (LAPACK) and the restatement reach a ratio
<= 1/4 on every case of the family; the factor 4 is headroom for the summation orders the
restatement does not reproduce (MFMA tiles, split-K chunks).  Measured on the CPU against the
longdouble reference, never against the library (tests/test_gp_check.py prints and asserts
them):

    family    c    worst ratio at c: gp_oracle   restatement
    exact    16                      0.215       0.215     (var at n = 1, kappa = 1)
    fitc     16                      0.161       0.161     (Lambda at m = 1)
    vfe      16                      0.101       0.202     (mean at m = 1)
    append    2                      0.189       0.189     (alpha at n0 = 1, k = 1)
    batched   4                      0.193       0.193     (n = 1)

The constants are set by the cases with N = 1 and 2: kappa = 1 there and the handful of
roundings of the Gram and the epilogue is all the error there is.  From N = 12 on
oracle and restatement stay below 0.09 at c = 1 (exact 0.015, fitc 0.087, vfe 0.050, batched
0.011, append 0.009).

Cases.  Every builder asserts: >= 90 % of the entries of every reference Gram exceed
1e-3 sigma2 (lengthscales of the order of sqrt(d) times the spread; unit lengthscales at
d = 11 give an almost diagonal Gram with kappa about 7, a GP that exercises nothing);
c N u kappa <= 1e-8 for the exact, FITC, batched and append families and <= 1e-6
for VFE, met by the choice of noise, jitter and lengthscales and never by a run-time skip;
at least half of the queries lie within 0.05 of a training row (an inducing row for the
sparse GPs) and those rows include the last ones, so a dropped last row or block moves a
variance by far more than the bound.  The Lambda clamp (lam = 1e-10) is left out: reaching it
puts 1e10 into B, and no such case can meet the cap.
"""
import functools
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import scipy.linalg as sla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chol_check as cc  # noqa: E402
import gram_check as gk  # noqa: E402
from gram_check import LD, U, longdouble_ok  # noqa: E402,F401
from oracle import gp_oracle as go  # noqa: E402

C = {"exact": 16, "fitc": 16, "vfe": 16, "append": 2, "batched": 4}   # measured: module docstring
CAP = {"exact": 1e-8, "fitc": 1e-8, "vfe": 1e-6, "append": 1e-8, "batched": 1e-8}
LOG2PI = np.log(2 * LD(np.pi)) if longdouble_ok() else np.log(2 * np.pi)
CLAMP = 1e-10


def strided_terms(n):
    return (n + 255) // 256


# ---- longdouble linear algebra -----------------------------------------------------------------
def ld_chol(A):
    """Plain column Cholesky in longdouble; None at the first non-positive pivot."""
    A = np.asarray(A, LD)
    n = len(A)
    L = np.zeros((n, n), LD)
    for j in range(n):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        if not piv > 0:
            return None
        L[j, j] = np.sqrt(piv)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def ld_fwd(L, B):
    X = np.array(B, LD, copy=True)
    for i in range(len(L)):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def ld_bwd(L, B):
    X = np.array(B, LD, copy=True)
    for i in reversed(range(len(L))):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def ladder():
    return [0.0] + go.jitter_ladder()


def ld_chol_ladder(K, noise):
    """(L, jitter, steps) by exact_gp.py's ladder with the fp64 ladder values; None: exhausted."""
    n = len(K)
    for steps, j in enumerate(ladder()):
        L = ld_chol(K + (LD(noise) + LD(j)) * np.eye(n, dtype=LD))
        if L is not None:
            return L, j, steps
    return None


def spec_sigma2(kind, sigma2):
    return go.composite_diag(kind) if isinstance(kind, tuple) else sigma2


def ld_gram(kind, X1, X2, ls, sigma2):
    """gram_check's direct-difference reference; composite specs as gp_oracle.gram."""
    if isinstance(kind, tuple):
        if kind[0] in ("sum", "prod"):
            a, b = ld_gram(kind[1], X1, X2, None, None), ld_gram(kind[2], X1, X2, None, None)
            return a + b if kind[0] == "sum" else a * b
        if kind[0] == "white":
            return LD(kind[1]) * np.eye(len(X1), dtype=LD) if X2 is None else np.zeros((len(X1), len(X2)), LD)
        return ld_gram(kind[0], X1, X2, kind[2], kind[1])
    return gk.reference(kind, X1, X2, np.atleast_1d(np.asarray(ls, np.float64)), sigma2)[0]


def ld_normalise(Y):
    """(yn, mean, std, degenerate) per column: population std, std < 1e-10 -> 1."""
    Y = np.asarray(Y, LD)
    m = Y.sum(axis=0) / len(Y)
    s = np.sqrt(((Y - m) ** 2).sum(axis=0) / len(Y))
    deg = s < 1e-10
    s = np.where(deg, LD(1), s)
    return (Y - m) / s, m, s, deg


def kappa(A):
    w = np.linalg.eigvalsh(np.asarray(A, np.float64))
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


def well_scaled(K, sigma2, tag):
    assert np.mean(np.asarray(K, np.float64) > 1e-3 * sigma2) >= 0.9, f"{tag}: badly scaled Gram, most entries vanish"


# ---- the longdouble exact GP ------------------------------------------------------------------
def ld_exact(kind, X, Y, ls, sigma2, noise, tag=""):
    """exact_fit of gp_oracle in longdouble.  None where the ladder is exhausted."""
    sigma2 = spec_sigma2(kind, sigma2)
    K = ld_gram(kind, X, None, ls, sigma2)
    well_scaled(K, sigma2, tag)
    fac = ld_chol_ladder(K, noise)
    if fac is None:
        return None
    L, jit, steps = fac
    n = len(X)
    yn, m, s, deg = ld_normalise(Y)
    alpha = ld_bwd(L, ld_fwd(L, yn))
    lml = -0.5 * (yn * alpha).sum(axis=0) - np.log(np.diag(L)).sum() - 0.5 * n * LOG2PI
    kap = kappa(K + (LD(noise) + LD(jit)) * np.eye(n, dtype=LD))
    return NS(kind=kind, X=X, ls=ls, sigma2=sigma2, noise=noise, n=n, n_out=Y.shape[1], L=L, jitter=jit, steps=steps,
              yn=yn, ymean=m, ystd=s, degenerate=deg, alpha=alpha, lml=lml, kappa=kap)


def ld_exact_predict(r, Xq, cov_out=None):
    """exact_predict (and exact_predict_cov for output cov_out) in longdouble."""
    Ks = ld_gram(r.kind, Xq, r.X, r.ls, r.sigma2)
    v = ld_fwd(r.L, Ks.T)
    lat = r.sigma2 - (v ** 2).sum(axis=0)
    out = NS(Ks=Ks, mean=(Ks @ r.alpha) * r.ystd + r.ymean, lat=lat, absdot=np.abs(Ks) @ np.abs(r.alpha),
             var=np.maximum(lat, LD(CLAMP))[:, None] * r.ystd ** 2)
    if cov_out is not None:
        out.cov_n = ld_gram(r.kind, Xq, None, r.ls, r.sigma2) - v.T @ v     # normalised units
    return out


# ---- data --------------------------------------------------------------------------------------
SIGMA2 = 1.7


def make_data(seed, n, d, n_out, p, kind, near_rows=None):
    """(X, Y, ls, Xq): unit-normal rows, lengthscales of the order of sqrt(d), smooth targets
    of different scale and offset per column, and queries of which the first ceil(p / 2) lie
    within 0.05 of the last training rows (near_rows: of those rows instead)."""
    rng = np.random.default_rng([seed, n, d, n_out, p])
    X = rng.standard_normal((n, d))
    ls = 0.8 * np.sqrt(d) * rng.uniform(1.0, 1.3, d)
    if kind in ("matern32", "matern52"):
        ls = ls * 2.0
    if kind == "se_iso":
        ls = ls[:1].copy()
    Wt = rng.standard_normal((d, n_out)) / np.sqrt(d)
    c = np.arange(n_out)
    Y = (1.0 + 0.5 * c) * np.sin(X @ Wt + c) + 0.05 * rng.standard_normal((n, n_out)) + 0.3 * c
    R = X if near_rows is None else near_rows
    k = (p + 1) // 2
    idx = (len(R) - 1 - np.arange(k)) % len(R)
    near = R[idx] + (0.03 / np.sqrt(d)) * rng.uniform(-1, 1, (k, d))
    Xq = np.vstack([near, rng.standard_normal((p - k, d))])
    assert np.all(np.sqrt(((Xq[:k] - R[idx]) ** 2).sum(axis=1)) <= 0.05) and 2 * k >= p and (len(R) - 1) in idx
    return X, Y, ls, Xq


def default_noise(n):
    return 1e-3 if n < 100 else 1e-2


PROG_D = 3


def prog_spec(ls, sigma2=1.1, white=0.02):
    """SumKernel(SE-ARD, WhiteNoise) as gp_oracle's composite spec."""
    return ("sum", ("se_ard", sigma2, tuple(float(x) for x in ls)), ("white", white))


def prog_arrays(spec):
    """(ops, par) of prog_spec for _lib.KernelProgram (gpmpc.h: SE_ARD 0, WHITE 4, SUM 10)."""
    _, (_, s2, ls), (_, w) = spec
    return [(0, 0), (4, len(ls) + 1), (10, 0)], [s2, *ls, w]


# ---- exact cases --------------------------------------------------------------------------------
class ExactCase:
    """One exact GP: data, parameters, the longdouble fit, its predictions at Xq and (cov)
    the covariance of output cov_out at the first pc queries."""

    family = "exact"

    def __init__(self, n, n_out, d, kind, p, noise=None, opt="", pc=0, seed=0):
        self.n, self.n_out, self.d, self.kind, self.p, self.opt, self.pc = n, n_out, d, kind, p, opt, pc
        self.tag = f"exact {kind} n {n} out {n_out} d {d} p {p}{' ' + opt if opt else ''}"
        self.noise = default_noise(n) if noise is None else noise
        self.sigma2 = SIGMA2
        kd = "se_ard" if kind == "prog" else kind
        self.X, self.Y, self.ls, self.Xq = make_data(seed, n, d, n_out, p, kd)
        if opt == "const":
            self.Y[:, 1] = 2.0
        if opt in ("dup1", "dup5", "exhaust", "refuse"):   # rows 1..3 repeat rows 4..6
            self.X[1:4] = self.X[4:7]
        if opt == "dup1":
            self.sigma2 = 1e-3
        if opt in ("clamp", "above"):
            self.Xq[0] = self.X[0]
        self.spec = prog_spec(self.ls) if kind == "prog" else kind
        self.code = None if kind == "prog" else gk.KINDS.index(kind)
        self.ref = ld_exact(self.spec, self.X, self.Y, self.ls, self.sigma2, self.noise, self.tag)
        if self.ref is None:
            return
        self.sigma2 = self.ref.sigma2
        self.pred = ld_exact_predict(self.ref, self.Xq)
        self.cov = ld_exact_predict(self.ref, self.Xq[:pc], cov_out=0) if pc else None
        self.b = C[self.family] * n * U * self.ref.kappa
        assert self.b <= CAP[self.family], f"{self.tag}: c N u kappa = {self.b:.2e} (kappa {self.ref.kappa:.2e})"

    def fit_args(self):
        return self.X, self.Y, self.ls, self.sigma2, self.noise


def check_norm(tag, n, Y, ymean, ystd):
    """Rule (a) on y_mean / y_std: [(name, ratio)] (ratio <= 1 passes)."""
    yn, m, s, deg = ld_normalise(Y)
    t = strided_terms(n)
    tiny = np.finfo(np.float64).tiny
    rm = np.abs(np.asarray(ymean, LD) - m) / np.maximum((t + 12) * U * np.abs(np.asarray(Y, LD)).mean(axis=0), tiny)
    rs = np.abs(np.asarray(ystd, LD) - s) / ((t + 20) * U * s)
    rs = np.where(deg, np.where(np.asarray(ystd) == 1.0, 0.0, np.inf), rs)
    return [(f"{tag}: y_mean", _f(rm)), (f"{tag}: y_std", _f(rs))]


def _f(r):
    r = np.asarray(r, np.float64)
    return float("inf") if (r.size and not np.all(np.isfinite(r))) else float(r.max()) if r.size else 0.0


def ratio(got, ref, bound):
    """max |got - ref| / bound; 0 / 0 passes, x / 0 and nan fail."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, LD)
    if got.shape != ref.shape:
        return float("inf")
    err = np.abs(got.astype(LD) - ref)
    b = np.broadcast_to(np.asarray(bound, LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / b)
    return _f(r)


def check_state_lml(tag, n, Y, ymean, ystd, L, alpha, lml):
    """Rule (a): the lml recomputed in longdouble from the device's own L, alpha, mean, std."""
    Ld, a = np.diag(np.asarray(L, LD)), np.asarray(alpha, LD)
    yn = (np.asarray(Y, LD) - np.asarray(ymean, LD)) / np.asarray(ystd, LD)
    t = strided_terms(n)
    logs = np.log(Ld)
    l = -0.5 * (yn * a).sum(axis=0) - logs.sum() - 0.5 * n * LOG2PI
    bound = U * ((t + 16) / 2 * np.abs(yn * a).sum(axis=0) + (t + 14) * np.abs(logs).sum() + 4 * 0.5 * n * LOG2PI
                 + 2 * np.abs(l))
    return [(f"{tag}: lml from the state", ratio(lml, l, bound))]


def check_exact_fit(case, got, ref=None, b=None, tag=None):
    """got: NS(ymean, ystd, L, alpha, lml, steps).  [(name, ratio)]."""
    ref, b, tag = ref or case.ref, b or case.b, tag or case.tag
    Y = got.Y if hasattr(got, "Y") else case.Y
    out = [(f"{tag}: jitter steps", 0.0 if int(got.steps) == ref.steps else float("inf"))]
    out += check_norm(tag, ref.n, Y, got.ymean, got.ystd)
    out += check_state_lml(tag, ref.n, Y, got.ymean, got.ystd, got.L, got.alpha, got.lml)
    out.append((f"{tag}: alpha", ratio(got.alpha, ref.alpha, b * np.abs(ref.alpha).max(axis=0))))
    out.append((f"{tag}: lml", ratio(got.lml, ref.lml, b * np.abs(ref.lml))))
    return out


def check_exact_predict(case, mean, var, ref=None, pred=None, b=None, tag=None):
    ref, pred, b, tag = ref or case.ref, pred or case.pred, b or case.b, tag or case.tag
    s_var = np.maximum(pred.lat, ref.sigma2)[:, None] * ref.ystd ** 2
    return [(f"{tag}: mean", ratio(mean, pred.mean, b * ref.ystd * pred.absdot)),
            (f"{tag}: var", ratio(var, pred.var, b * s_var))]


def check_cov(case, mean, cov, var):
    """predict_cov: the means of every output, the covariance in normalised units (as the
    library returns it; gp_oracle's is that times ystd^2), symmetric to the rule, and its
    diagonal against predict's variance / ystd^2 where that is unclamped."""
    r, c = case.ref, case.cov
    s = r.sigma2
    out = [(f"{case.tag}: cov mean", ratio(mean, c.mean, case.b * r.ystd * c.absdot)),
           (f"{case.tag}: cov", ratio(cov, c.cov_n, case.b * s)),
           (f"{case.tag}: cov symmetry", ratio(cov, np.asarray(cov, LD).T, 2 * case.b * s))]
    lat = np.asarray(var, LD)[:case.pc, 0] / r.ystd[0] ** 2
    free = np.asarray(c.lat > 2 * CLAMP)
    out.append((f"{case.tag}: cov diagonal vs predict", ratio(np.diag(cov)[free], lat[free], 2 * case.b * s)))
    return out


# ---- float64 restatement of the exact GP ----------------------------------------------------------
def restate_W(L):
    n = len(L)
    return cc.restate_tri_inverse(L) if n > 128 else np.tril(cc.restate_trsm(L, np.eye(n), False))


def block_sum(Y):
    """Column sums as k_normalise adds them: thread i mod 256 its strided terms in order, then
    the tree over the 256 threads (numpy's pairwise sum)."""
    n = len(Y)
    t = strided_terms(n)
    P = np.zeros((t * 256,) + Y.shape[1:])
    P[:n] = Y
    per_thread = P.reshape((t, 256) + Y.shape[1:]).sum(axis=0)
    return np.array([per_thread[:, c].copy().sum() for c in range(Y.shape[1])])


def fp_normalise(Y, ddof=0):
    m = block_sum(Y) / len(Y)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(block_sum((Y - m) ** 2) / (len(Y) - ddof))
    s = np.where(s < 1e-10, 1.0, s)
    return (Y - m) / s, m, s


def fp_gram(kind, X1, X2, ls, sigma2):
    return go.gram(kind, X1, X2, sigma2, ls)


def restate_exact(case, mut=None, XY=None):
    """exact_fit of gp.hip in float64 -> NS(L, W, alpha, ymean, ystd, lml, steps, ...).
    mut: sample_std, noise_twice, no_jitter (the jitter left off the first diagonal entry of
    the matrix the kept factor is of), lml_no_2pi, lml_n1."""
    X, Y = XY if XY is not None else (case.X, case.Y)
    n = len(X)
    noise = case.noise * (2.0 if mut == "noise_twice" else 1.0)
    K = fp_gram(case.spec, X, None, case.ls, case.sigma2)
    steps, L = 0, None
    for steps, j in enumerate(ladder()):
        try:
            A = K + noise * np.eye(n)
            A[np.diag_indices(n)] += j
            L = np.linalg.cholesky(A)
            break
        except np.linalg.LinAlgError:
            L = None
    if L is None:
        raise ValueError("Kernel matrix is not positive definite even with jitter")
    if mut == "no_jitter":
        A[0, 0] -= j
        L = np.linalg.cholesky(A)
    W = restate_W(L)
    yn, m, s = fp_normalise(Y, ddof=1 if mut == "sample_std" else 0)
    alpha = cc.restate_cho_solve_inv(L, W, yn)
    ld = np.log(np.diag(L)[:n - 1 if mut == "lml_n1" else n]).sum()
    lml = -0.5 * (yn * alpha).sum(axis=0) - ld - (0.0 if mut == "lml_no_2pi" else 0.5 * n * np.log(2 * np.pi))
    return NS(X=X, Y=Y, L=L, W=W, alpha=alpha, yn=yn, ymean=m, ystd=s, lml=lml, steps=steps, n=n)


def row_tiles(M, p, K, plans):
    """(number of partial rows the consumer sums, tile height) of an M x p x K SUMSQ product."""
    nrt, kind = plans(M, p, K)
    return nrt, (128 if kind == 1 else 64)


def default_plans(M, p, K):
    """64-row tiles (the plan of the library where it is not loaded)."""
    return (M + 63) // 64, 0


def sumsq_partials(V, M, p, K, plans):
    """Column sums of V^2 (rows of W k*) as the partial rows k_post_finish sums."""
    nrt, th = row_tiles(M, p, K, plans)
    return np.stack([(V[t * th:(t + 1) * th] ** 2).sum(axis=0) for t in range(nrt)]), th


PREDICT_MUTANTS = ("drop_last_row", "drop_last_block", "omit_partial", "stale_partial", "alpha_last", "std_next",
                   "std_not_squared", "no_clamp", "clamp_1e12")
FIT_MUTANTS = ("sample_std", "noise_twice", "no_jitter", "lml_no_2pi", "lml_n1")


def restate_predict(st, kind_spec, ls, sigma2, Xq, mut=None, plans=default_plans):
    """gpmpc_gp_predict in float64 from a restated state -> (mean, var), or None where mut is
    not defined for the shape."""
    n, no, p = st.n, st.alpha.shape[1], len(Xq)
    Ks = fp_gram(kind_spec, Xq, st.X, ls, sigma2)
    V = st.W @ Ks.T
    if mut == "drop_last_row":
        V = V[:-1]
    if mut == "drop_last_block":
        V = V[:-16] if n > 16 else V[:0]
    part, th = sumsq_partials(V, n + no, p, n, plans)
    if mut == "omit_partial":
        if len(part) < 2 or (len(part) - 1) * th >= n:
            return None
        part = part[:-1]
    ss = part.sum(axis=0)
    if mut == "stale_partial":
        ss = ss + 1e-9 * sigma2
    lat = sigma2 - ss
    floor = {"no_clamp": -np.inf, "clamp_1e12": 1e-12}.get(mut, CLAMP)
    if mut in ("no_clamp", "clamp_1e12") and not np.any(lat < CLAMP):
        return None
    lat = np.where(lat > floor, lat, floor)
    a = st.alpha.copy()
    if mut == "alpha_last":
        a[-1] = 0.0
    sd = st.ystd
    if mut == "std_next":
        if no < 2:
            return None
        sd = np.roll(st.ystd, -1)
    mean = (Ks @ a) * sd + st.ymean
    var = lat[:, None] * (st.ystd if mut == "std_not_squared" else st.ystd ** 2)
    return mean, var


def restate_cov(st, case):
    Xq = case.Xq[:case.pc]
    Ks = fp_gram(case.spec, Xq, st.X, case.ls, case.sigma2)
    Vt = Ks @ st.W.T
    return (Ks @ st.alpha) * st.ystd + st.ymean, fp_gram(case.spec, Xq, None, case.ls, case.sigma2) - Vt @ Vt.T


def oracle_exact(case, XY=None):
    """gp_oracle's exact_fit as the NS the checks take (with the oracle's own state)."""
    X, Y = XY if XY is not None else (case.X, case.Y)
    st = go.exact_fit(X, Y, kind=case.spec, sigma2=case.sigma2, ls=case.ls, noise=case.noise)
    return NS(Y=Y, L=st["L"], alpha=st["alpha"], ymean=st["y_mean"], ystd=st["y_std"], lml=st["lml"],
              steps=st["jitter_steps"], st=st)


# ---- the case tables -------------------------------------------------------------------------------
K4 = gk.KINDS
EXACT_FIT = [  # (n, n_out, d, kind, p, noise, opt, pc)
    (1, 1, 1, "se_ard", 3, 1e-3, "", 0), (2, 3, 11, "se_iso", 4, 1e-3, "", 0),
    (31, 8, 13, "matern32", 37, None, "", 0), (32, 15, 32, "matern52", 37, None, "", 0),
    (33, 16, 1, "se_ard", 37, 1e-2, "", 0), (128, 1, 11, "se_iso", 37, None, "", 0),
    (129, 3, 13, "matern32", 37, None, "", 0), (255, 8, 32, "matern52", 37, None, "", 0),
    (256, 15, 11, "se_ard", 37, None, "", 0), (257, 16, 1, "se_iso", 37, 2e-2, "", 0),
    (300, 3, 11, "matern52", 37, 3e-2, "", 0), (300, 3, 13, "se_ard", 257, None, "", 0),
    (70, 2, PROG_D, "prog", 19, 1e-3, "", 0), (33, 3, 11, "se_ard", 9, None, "const", 0),
    (8, 2, 11, "se_ard", 5, -1e-7, "dup1", 0), (40, 2, 11, "se_ard", 9, -5e-3, "dup5", 0),
]
EXACT_EXHAUST = (12, 2, 11, "se_ard", 3, -4.0, "exhaust", 0)
_P = (1, 63, 64, 65, 255, 256, 257)
EXACT_PREDICT = [(n, no, (11, 13, 32, 1)[i % 4], K4[i % 4], _P[i], None, "", 0)
                 for i, (n, no) in enumerate([(61, 3), (62, 3), (127, 1), (126, 3), (113, 16), (250, 6), (253, 3)])]
EXACT_PREDICT += [(257, 8, 11, "se_ard", 256, None, "", 0), (257, 8, 11, "se_ard", 64, None, "", 0),
                  (1, 1, 11, "se_ard", 2, 1e-11, "clamp", 0), (1, 1, 11, "se_ard", 2, 2e-10, "above", 0)]
EXACT_COV = [(120, 1, 11, "se_ard", 1, None, "", 1), (128, 3, 13, "matern52", 33, None, "", 33),
             (129, 1, 11, "se_iso", 65, None, "", 65), (140, 3, 32, "matern32", 33, None, "", 33)]
EXACT_ALL = EXACT_FIT + EXACT_PREDICT + EXACT_COV


@functools.lru_cache(maxsize=None)
def exact_case(spec):
    n, no, d, kind, p, noise, opt, pc = spec
    return ExactCase(n, no, d, kind, p, noise, opt, pc)


def case_id(spec):
    return "-".join(str(x) for x in spec if x not in ("", None))


# ---- sparse GPs ----------------------------------------------------------------------------------
class SparseCase:
    """One FITC or VFE GP over m inducing rows: the longdouble fit and predictions."""

    def __init__(self, method, m, n, n_out, d, p, noise, jitter, kind="se_ard", seed=1):
        self.method, self.m, self.n, self.n_out, self.d, self.p = method, m, n, n_out, d, p
        self.noise, self.jitter, self.family, self.kind = noise, jitter, method, kind
        self.tag = f"{method} {kind} m {m} n {n} out {n_out} d {d} p {p}"
        rng = np.random.default_rng([seed, m, n, d])
        self.Z = rng.standard_normal((m, d))
        self.X, self.Y, self.ls, self.Xq = make_data(seed, n, d, n_out, p, "se_ard", near_rows=self.Z)
        self.spec = prog_spec(self.ls) if kind == "prog" else kind
        self.sigma2 = spec_sigma2(self.spec, SIGMA2)
        r = self.ref = ld_sparse(self)
        self.pred = ld_sparse_predict(self, r, self.Xq)
        self.b = C[method] * m * U * max(r.kappa_uu, r.kappa_B)
        self.b_lam = C[method] * m * U * r.kappa_uu
        assert self.b <= CAP[method], (f"{self.tag}: c N u kappa = {self.b:.2e} (kappa K_uu {r.kappa_uu:.2e}, "
                                       f"B {r.kappa_B:.2e})")
        assert method == "vfe" or float(r.lam.min()) > 1e-6, f"{self.tag}: Lambda near its clamp"


def ld_sparse(c):
    """fitc_fit / vfe_fit of gp_oracle in longdouble."""
    m, n, s2 = c.m, c.n, c.sigma2
    Kuu = ld_gram(c.spec, c.Z, None, c.ls, s2)
    Kuf = ld_gram(c.spec, c.Z, c.X, c.ls, s2)
    well_scaled(Kuf, s2, c.tag)
    well_scaled(Kuu, s2, c.tag)
    I = np.eye(m, dtype=LD)
    Auu = Kuu + LD(c.jitter) * I
    Luu = ld_chol(Auu)
    A = ld_fwd(Luu, Kuf)
    yn, ym, ys, deg = ld_normalise(c.Y)
    if c.method == "fitc":
        lam = np.maximum(s2 - (A ** 2).sum(axis=0) + LD(c.noise), LD(CLAMP))
        As = A / np.sqrt(lam)
        B = I + As @ As.T
        LB = ld_chol(B)
        cv = A @ (yn / lam[:, None])
        alpha = ld_bwd(LB, ld_fwd(LB, cv))
        fit = -0.5 * ((yn ** 2 / lam[:, None]).sum(axis=0) - (cv * alpha).sum(axis=0))
        lml = fit - np.log(np.diag(LB)).sum() - 0.5 * np.log(lam).sum() - 0.5 * n * LOG2PI
    else:
        lam = None
        B = Kuu + Kuf @ Kuf.T / LD(c.noise) + LD(c.jitter) * I
        LB = ld_chol(B)
        trace = (n * LD(s2) - (A ** 2).sum()) / LD(c.noise)
        cv = Kuf @ yn / LD(c.noise)
        alpha = ld_bwd(LB, ld_fwd(LB, cv))
        fit = (-0.5 / LD(c.noise) * (yn * yn).sum(axis=0) + (cv * alpha).sum(axis=0)
               - 0.5 * (alpha * (Kuu @ alpha)).sum(axis=0))
        cplx = -np.log(np.diag(LB)).sum() + np.log(np.diag(Luu)).sum() - 0.5 * n * np.log(LD(c.noise))
        lml = fit - 0.5 * trace + cplx - 0.5 * n * LOG2PI
    return NS(Luu=Luu, LB=LB, lam=lam, alpha=alpha, lml=lml, ymean=ym, ystd=ys, kappa_uu=kappa(Auu), kappa_B=kappa(B))


def ld_sparse_predict(c, r, Xq):
    Ksu = ld_gram(c.spec, Xq, c.Z, c.ls, c.sigma2)
    v = ld_fwd(r.Luu, Ksu.T)
    w = ld_fwd(r.LB, v)
    lat = c.sigma2 - (v ** 2).sum(axis=0) + (w ** 2).sum(axis=0)
    return NS(mean=(Ksu @ r.alpha) * r.ystd + r.ymean, lat=lat, absdot=np.abs(Ksu) @ np.abs(r.alpha),
              var=np.maximum(lat, LD(CLAMP))[:, None] * r.ystd ** 2)


SPARSE_MUTANTS = ("lam_no_noise", "trace_n1", "w2_upper", "drop_last_row", "alpha_last", "std_next", "std_not_squared",
                  "sample_std")


def restate_sparse(c, mut=None):
    """sparse_fit / vfe_tail of gp.hip in float64.  mut: lam_no_noise (FITC), trace_n1 (VFE),
    w2_upper, sample_std."""
    m, n, s2 = c.m, c.n, c.sigma2
    Kuu = fp_gram(c.spec, c.Z, None, c.ls, s2)
    Kuf = fp_gram(c.spec, c.Z, c.X, c.ls, s2)
    Luu = np.linalg.cholesky(Kuu + c.jitter * np.eye(m))
    W = restate_W(Luu)
    A = cc.restate_trsm(Luu, Kuf, False)
    yn, ym, ys = fp_normalise(c.Y, ddof=1 if mut == "sample_std" else 0)
    if c.method == "fitc":
        if mut == "trace_n1":
            return None
        lam = s2 - (A ** 2).sum(axis=0) + (0.0 if mut == "lam_no_noise" else c.noise)
        lam = np.where(lam > CLAMP, lam, CLAMP)
        cv = A @ (yn / lam[:, None])
        As = A * (1.0 / np.sqrt(lam))
        LB = np.linalg.cholesky(np.eye(m) + As @ As.T)
        alpha = cc.restate_potrs(LB, cv)
        lml = (-0.5 * ((yn * yn / lam[:, None]).sum(axis=0) - (cv * alpha).sum(axis=0)) - np.log(np.diag(LB)).sum()
               - 0.5 * np.log(lam).sum() - 0.5 * n * np.log(2 * np.pi))
    else:
        if mut == "lam_no_noise":
            return None
        lam = None
        B = Kuu + Kuf @ Kuf.T * (1.0 / c.noise)
        B[np.diag_indices(m)] += c.jitter
        LB = np.linalg.cholesky(B)
        cv = Kuf @ (yn / c.noise)
        q = (A ** 2).sum(axis=0)
        alpha = cc.restate_potrs(LB, cv)
        fit = (-0.5 / c.noise * (yn * yn).sum(axis=0) + (cv * alpha).sum(axis=0)
               - 0.5 * (alpha * (Kuu @ alpha)).sum(axis=0))
        trace = (n * s2 - (q[:-1] if mut == "trace_n1" else q).sum()) / c.noise
        lml = (fit - 0.5 * trace - np.log(np.diag(LB)).sum() + np.log(np.diag(Luu)).sum() - 0.5 * n * np.log(c.noise)
               - 0.5 * n * np.log(2 * np.pi))
    W2 = np.tril(cc.restate_trsm(LB, W, False))
    if mut == "w2_upper":
        if m < 2:
            return None
        W2 = W2 + 1e-9 * np.triu(np.ones((m, m)), 1)
    return NS(W=W, W2=W2, lam=lam, alpha=alpha, lml=lml, ymean=ym, ystd=ys)


def restate_sparse_predict(c, st, Xq, mut=None):
    """fitc_posterior_dev in float64 (both forms read W over its lower triangle and W2 in full)."""
    Ksu = fp_gram(c.spec, Xq, c.Z, c.ls, c.sigma2)
    V, Wv = st.W @ Ksu.T, st.W2 @ Ksu.T
    if mut == "drop_last_row":
        V = V[:-1]
    lat = c.sigma2 - (V ** 2).sum(axis=0) + (Wv ** 2).sum(axis=0)
    lat = np.where(lat > CLAMP, lat, CLAMP)
    a, sd = st.alpha.copy(), st.ystd
    if mut == "alpha_last":
        a[-1] = 0.0
    if mut == "std_next":
        if c.n_out < 2:
            return None
        sd = np.roll(sd, -1)
    return (Ksu @ a) * sd + st.ymean, lat[:, None] * (st.ystd if mut == "std_not_squared" else st.ystd ** 2)


def oracle_sparse(c):
    f = go.fitc_fit if c.method == "fitc" else go.vfe_fit
    st = f(c.Z, c.X, c.Y, sigma2=c.sigma2, ls=c.ls, noise=c.noise, jitter=c.jitter, kind=c.spec)
    return NS(lam=st["lam"], alpha=st["alpha"], lml=st["lml"], ymean=st["y_mean"], ystd=st["y_std"], st=st)


def check_sparse_fit(c, got):
    r = c.ref
    out = check_norm(c.tag, c.n, c.Y, got.ymean, got.ystd)
    out.append((f"{c.tag}: alpha", ratio(got.alpha, r.alpha, c.b * np.abs(r.alpha).max(axis=0))))
    out.append((f"{c.tag}: lml", ratio(got.lml, r.lml, c.b * np.abs(r.lml))))
    if c.method == "fitc":
        out.append((f"{c.tag}: lam", ratio(got.lam, r.lam, c.b_lam * (c.sigma2 + abs(c.noise)))))
    return out


def check_sparse_predict(c, mean, var, what=""):
    r, pr = c.ref, c.pred
    s_var = np.maximum(pr.lat, c.sigma2)[:, None] * r.ystd ** 2
    return [(f"{c.tag}: mean{what}", ratio(mean, pr.mean, c.b * r.ystd * pr.absdot)),
            (f"{c.tag}: var{what}", ratio(var, pr.var, c.b * s_var))]


# (m, n, n_out, d, p); noise and jitter per method below
SPARSE_SHAPES = [(1, 33, 1, 1, 1), (16, 33, 8, 11, 37), (16, 33, 1, 1, 37), (17, 257, 9, 11, 37),
                 (128, 300, 16, 32, 257), (129, 300, 1, 11, 37), (255, 300, 8, 11, 1), (256, 300, 8, 32, 37), (257, 300, 9, 11, 257),
                 (40, 33, 3, 11, 37)]
SPARSE_PROG = (20, 50, 2, PROG_D, 11)


def sparse_params(method, m, d):
    """(noise, jitter): found on the CPU so that every case meets its cap."""
    if m == 1:
        return 1.0, 1e-2
    if method == "fitc":
        return 1e-2, (1e-3 if d == 1 else 3e-3 if m >= 128 else 1e-5)
    if d == 1:
        return 1e-1, 1e-2
    return (3e-1, 1e-1) if m >= 128 else (1e-2, 1e-4)


SPARSE_ALL = [(meth,) + s + ("se_ard",) for meth in ("fitc", "vfe") for s in SPARSE_SHAPES]
SPARSE_ALL += [("fitc",) + SPARSE_PROG + ("prog",), ("vfe",) + SPARSE_PROG + ("prog",)]


@functools.lru_cache(maxsize=None)
def sparse_case(spec):
    method, m, n, no, d, p, kind = spec
    noise, jitter = sparse_params(method, m, d)
    return SparseCase(method, m, n, no, d, p, noise, jitter, kind)


# ---- gp_lml_batched ---------------------------------------------------------------------------------
class BatchCase:
    """B parameter sets over one (X, y): per set the longdouble lml_at and the bound."""

    family = "batched"

    def __init__(self, n, B, d, kind, opt="", seed=2):
        self.n, self.B, self.d, self.kind, self.opt = n, B, d, kind, opt
        self.tag = f"lml_batched {kind} n {n} B {B} d {d}{' ' + opt if opt else ''}"
        self.code = gk.KINDS.index(kind)
        self.X, Y, ls, _ = make_data(seed, n, d, 1, 1, kind)
        self.y = Y[:, 0]
        rng = np.random.default_rng([seed, n, B])
        self.ls = ls[None, :] * rng.uniform(0.9, 1.2, (B, 1))
        self.sigma2 = SIGMA2 * rng.uniform(0.8, 1.2, B)
        self.noise = default_noise(n) * rng.uniform(1.0, 2.0, B)
        if opt == "ladder":   # set 0 plain, set 1: one step, set 3: exhausted
            self.X[1:4] = self.X[4:7]
            self.noise[0] = 1e-2
            self.sigma2[1], self.noise[1] = 1e-3, -1e-7
            self.noise[2] = 1e-2
            self.noise[3] = -4.0
        self.refs = [ld_exact(kind, self.X, self.y[:, None], self.ls[b], self.sigma2[b], self.noise[b], self.tag)
                     for b in range(B)]
        self.steps = np.array([-1 if r is None else r.steps for r in self.refs])
        self.lml = np.array([-np.inf if r is None else r.lml[0] for r in self.refs], LD)
        self.b = np.array([0.0 if r is None else C[self.family] * n * U * r.kappa for r in self.refs])
        assert self.b.max() <= CAP[self.family], f"{self.tag}: c N u kappa = {self.b.max():.2e}"


def check_batched(c, lml, steps):
    out = [(f"{c.tag}: jitter steps", 0.0 if np.array_equal(np.asarray(steps), c.steps) else float("inf"))]
    ok = c.steps >= 0
    out.append((f"{c.tag}: exhausted sets", 0.0 if np.all(np.asarray(lml)[~ok] == -np.inf) else float("inf")))
    out.append((f"{c.tag}: lml", ratio(np.asarray(lml)[ok], c.lml[ok], c.b[ok] * np.abs(c.lml[ok]))))
    return out


def restate_lml(c, b, mut=None):
    """One set of gpmpc_gp_lml_batched in float64: (lml, steps); x = L^-1 yn by substitution."""
    n = c.n
    K = fp_gram(c.kind, c.X, None, c.ls[b], c.sigma2[b])
    yn, _, _ = fp_normalise(c.y[:, None])
    for steps, j in enumerate(ladder()):
        try:
            A = K + c.noise[b] * np.eye(n)
            if not (mut == "no_jitter" and steps):
                A[np.diag_indices(n)] += j
            elif steps:
                A[np.diag_indices(n)] += j
                A[0, 0] -= j
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        x = sla.solve_triangular(L, yn[:, 0], lower=True)
        ld = np.log(np.diag(L)[:n - 1 if mut == "lml_n1" else n]).sum()
        return -0.5 * x @ x - ld - (0.0 if mut == "lml_no_2pi" else 0.5 * n * np.log(2 * np.pi)), steps
    return -np.inf, -1


def oracle_lml(c, b):
    return go.lml_at(c.X, c.y, c.sigma2[b], c.ls[b], c.noise[b], kind=c.kind)


BATCH_ALL = [(1, 3, 11, "se_ard", ""), (31, 17, 13, "se_iso", ""), (32, 3, 32, "matern32", ""),
             (33, 1, 1, "matern52", ""), (256, 3, 11, "se_ard", ""), (257, 1, 11, "se_iso", ""),
             (12, 5, 11, "se_ard", "ladder")]


@functools.lru_cache(maxsize=None)
def batch_case(spec):
    return BatchCase(*spec)


# ---- append ------------------------------------------------------------------------------------------
class AppendCase:
    """A GP fitted on n0 rows and grown by the blocks ks: after every block the longdouble GP
    of the concatenated data.  refuse: the appended row repeats a training row of a GP
    fitted with a slightly negative noise -- the concatenated matrix is not positive
    definite and the append must return False."""

    family = "append"

    def __init__(self, n0, ks, n_out, d, kind, opt="", seed=3):
        self.n0, self.ks, self.n_out, self.d, self.kind, self.opt = n0, ks, n_out, d, kind, opt
        self.tag = f"append {kind} n0 {n0} k {'+'.join(map(str, ks))} out {n_out} d {d}{' ' + opt if opt else ''}"
        self.code = gk.KINDS.index(kind)
        n = n0 + sum(ks)
        self.p = 9
        self.X, self.Y, self.ls, self.Xq = make_data(seed, n, d, n_out, self.p, kind)
        self.sigma2, self.noise = SIGMA2, default_noise(n)
        self.stages = []
        if opt == "refuse":
            self.noise = -1e-9
            self.X[n0:] = self.X[:n - n0]
            self.Xq = self.Xq[self.p // 2 + 1:]   # fresh draws only
            return
        m = n0
        for k in ks:
            m += k
            ref = ld_exact(kind, self.X[:m], self.Y[:m], self.ls, self.sigma2, self.noise, self.tag)
            assert ref is not None and ref.steps == 0
            b = C[self.family] * m * U * ref.kappa
            assert b <= CAP[self.family], f"{self.tag}: c N u kappa = {b:.2e}"
            self.stages.append(NS(n=m, ref=ref, pred=ld_exact_predict(ref, self.Xq), b=b))
    spec = property(lambda self: self.kind)


def restate_append(c, st, k, mut=None):
    """gpmpc_gp_append in float64 from the restated state st of the first n rows.
    mut: w_sign, old_norm."""
    n = st.n
    m = n + k
    X, Y = c.X[:m], c.Y[:m]
    K21 = fp_gram(c.kind, X[n:], X[:n], c.ls, c.sigma2)
    Bt = K21 @ st.W.T
    S = fp_gram(c.kind, X[n:], None, c.ls, c.sigma2) + c.noise * np.eye(k) - Bt @ Bt.T
    Ls = np.linalg.cholesky(S)
    Li = np.tril(cc.restate_trsm(Ls, np.eye(k), False))
    L = np.zeros((m, m))
    W = np.zeros((m, m))
    L[:n, :n], L[n:, :n], L[n:, n:] = st.L, Bt, Ls
    W[:n, :n], W[n:, n:] = st.W, Li
    W[n:, :n] = (1.0 if mut == "w_sign" else -1.0) * (Li @ (Bt @ st.W))
    if mut == "old_norm":
        ym, ys = st.ymean, st.ystd
        yn = (Y - ym) / ys
    else:
        yn, ym, ys = fp_normalise(Y)
    alpha = W.T @ (W @ yn)
    lml = -0.5 * (yn * alpha).sum(axis=0) - np.log(np.diag(L)).sum() - 0.5 * m * np.log(2 * np.pi)
    return NS(X=X, Y=Y, L=L, W=W, alpha=alpha, yn=yn, ymean=ym, ystd=ys, lml=lml, steps=0, n=m)


def check_append(c, stage, got, mean, var):
    """got: the grown handle's NS(Y, ymean, ystd, L, alpha, lml, steps)."""
    out = check_exact_fit(c, got, ref=stage.ref, b=stage.b, tag=f"{c.tag} at n {stage.n}")
    out.append((f"{c.tag} at n {stage.n}: L", ratio(np.tril(got.L), stage.ref.L, stage.b * np.abs(stage.ref.L).max())))
    return out + check_exact_predict(c, mean, var, ref=stage.ref, pred=stage.pred, b=stage.b,
                                     tag=f"{c.tag} at n {stage.n}")


# (n0, ks, n_out, d, kind, opt)
APPEND_ALL = [(1, (1,), 1, 1, "se_ard", ""), (31, (2, 3), 16, 32, "se_iso", ""), (120, (9,), 1, 32, "matern52", ""),
              (128, (1,), 16, 1, "se_ard", ""), (129, (127,), 1, 11, "se_iso", ""), (250, (7,), 16, 11, "matern52", ""),
              (40, (60,), 1, 11, "se_ard", "")]
APPEND_REFUSE = (30, (1,), 2, 11, "se_ard", "refuse")


@functools.lru_cache(maxsize=None)
def append_case(spec):
    return AppendCase(*spec)


def worst(results):
    """(name, ratio) of the largest ratio."""
    return max(results, key=lambda r: r[1])


def failures(results):
    return [f"{name}: ratio {r:.3g} > 1" for name, r in results if not r <= 1.0]
