"""Uncertainty propagation for GP-MPC (reference src/mpc/uncertainty_prop.py).

Same classes, arguments and results as the reference:

* ``UncertaintyPropagator`` -- linear (uncertainty_prop.py:117-177), unscented
  (:179-264) and Monte-Carlo (:266-315) propagation of the state distribution
  along a control sequence, with the GP variance as process noise;
* ``ConstraintTightening`` (:318-411) and ``TubeBasedRobustness`` (:414-468).

The linear method is the one GPMPC calls (gp_mpc.py:284-290, 348-353).  Its
mean recursion needs one GP evaluation per horizon step -- a device call,
batched over trajectories in ``propagate_batch`` -- and its covariance
recursion Sigma_{k+1} = A_k Sigma_k A_k^T + Q_k runs for every trajectory in
one launch of the device kernel (``gpmpc_cov_propagate``, csrc/uprop.hip).

The unscented method runs its whole recursion -- Cholesky factor, sigma points,
model step, GP means and the variance at the centre -- in one device call for a
batch of trajectories (``propagate_unscented_batch``; ``gpmpc_uprop3_unscented`` /
``gpmpc_uprop6_unscented``, csrc/uprop_ut.hip) where the linear device paths'
gates accept, and the per-step host loop elsewhere.

The Monte-Carlo method draws on the host -- numpy's global RNG in the reference's
order, so a seed means what it means there -- and under the same gates runs the
particles of a batch of trajectories in one device call
(``propagate_monte_carlo_batch``; ``gpmpc_uprop3_mc`` / ``gpmpc_uprop6_mc``,
csrc/uprop_mc.hip): per horizon step one GP posterior at all B * n_samples
particles, the per-particle plant step with the sampled residual, and the sample
statistics at the end.  Elsewhere the per-step host loop consumes the same draws.

Both model shapes work: the reference's 14-state 6-DoF model with a 4-tuple GP
(StructuredRocketGP: residuals on v-dot 4:7 and omega-dot 11:14), and the
7-state 3-DoF model with a 2-tuple GP (Simple3DoFGP: residual on v-dot only).
The reference hard-codes n_x = 14 (uncertainty_prop.py:87); here n_x is the
dynamics' ``n_state`` (default 14).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import numpy as np

from .. import _lib


@dataclass
class PropagatedUncertainty:
    """uncertainty_prop.py:35-55."""
    means: np.ndarray        # (N+1, n_x)
    covariances: np.ndarray  # (N+1, n_x, n_x)

    def get_std(self, k: int) -> np.ndarray:
        return np.sqrt(np.diag(self.covariances[k]))

    def get_confidence_bounds(self, k: int, confidence: float = 0.95) -> Tuple[np.ndarray, np.ndarray]:
        from scipy.stats import norm
        kappa = norm.ppf((1 + confidence) / 2)
        std = self.get_std(k)
        return self.means[k] - kappa * std, self.means[k] + kappa * std


def _gp_batch(gp, X, U):
    """GP residual mean/variance at P points -> (d_v, d_w, var_v, var_w); d_w and
    var_w are None for a 2-tuple (3-DoF) GP.  One device call when the GP has
    predict_batch."""
    X = np.atleast_2d(X); U = np.atleast_2d(U)
    if hasattr(gp, "predict_batch"):
        r = gp.predict_batch(X, U)
    else:
        rows = [gp.predict(X[i], U[i]) for i in range(X.shape[0])]
        r = tuple(np.array([row[j] for row in rows]) for j in range(len(rows[0])))
    if len(r) == 4:
        return (np.atleast_2d(r[0]), np.atleast_2d(r[1]), np.atleast_2d(r[2]), np.atleast_2d(r[3]))
    return np.atleast_2d(r[0]), None, np.atleast_2d(r[1]), None


class UncertaintyPropagator:
    """uncertainty_prop.py:58-315."""

    def __init__(self, dynamics, gp_model, method: str = "linear", ctx=None):
        self.dynamics = dynamics
        self.gp = gp_model
        self.method = method
        self.n_x = int(getattr(dynamics, "n_state", 14))
        self.n_u = 3
        self._ctx = ctx

    @property
    def ctx(self):
        return self._ctx or _lib.default_context()

    # residual rows of the state: v-dot, and omega-dot for the 14-state model
    def _rows(self):
        return (slice(4, 7), slice(11, 14)) if self.n_x == 14 else (slice(4, 7), None)

    def propagate(self, x0, U, Sigma_0=None, dt: float = 0.1) -> PropagatedUncertainty:
        """uncertainty_prop.py:91-115."""
        if self.method == "linear":
            return self._propagate_linear(x0, U, Sigma_0, dt)
        if self.method == "unscented":
            return self._propagate_unscented(x0, U, Sigma_0, dt)
        if self.method == "monte_carlo":
            return self._propagate_monte_carlo(x0, U, Sigma_0, dt)
        raise ValueError(f"Unknown method: {self.method}")

    # the whole linear propagation in one device call (gpmpc_uprop3_linear) for the 3-DoF
    # explicit-Euler model over the 3-DoF exact GP: the N sequential GP predictions of the
    # host loop below become one kernel; the same recursion, rounding aside
    use_device = True

    def _gate_6dof(self):
        """(hv, hw, exact, rocket) when the 14-state device recursions apply:
        Rocket6DoFDynamics over a fitted StructuredRocketGP at its default feature set (the
        device features are features.py's at reference velocity 10 with altitude and
        density), its residual groups each one shared device GP.  Else None."""
        if not self.use_device or self.n_x != 14:
            return None
        from ..dynamics.rocket_6dof import Rocket6DoFDynamics
        from ..gp.structured_gp import StructuredRocketGP
        gp = self.gp
        if type(self.dynamics) is not Rocket6DoFDynamics or type(gp) is not StructuredRocketGP:
            return None
        c = gp.config
        if not (gp._is_fitted and c.reference_velocity == 10.0 and c.include_altitude and c.include_density):
            return None
        hv, hw = gp.gp_v.device_handle, gp.gp_omega.device_handle
        if hv is None or hw is None:
            return None
        p = self.dynamics.params
        rocket = np.concatenate([np.asarray(p.J_B, float).reshape(9), np.asarray(p.r_T_B, float).reshape(3),
                                 np.asarray(p.g_I, float).reshape(3),
                                 [float(p.alpha), float(p.g0)]])
        return hv, hw, not c.use_sparse, rocket

    def _device_6dof(self, X0, U, Sigma_0, dt):
        """gpmpc_uprop6_linear where _gate_6dof accepts."""
        gate = self._gate_6dof()
        if gate is None:
            return None
        hv, hw, exact, rocket = gate
        S0 = None
        if Sigma_0 is not None:
            S0 = np.broadcast_to(np.asarray(Sigma_0, float), (X0.shape[0], 14, 14))
        try:
            return _lib.uprop6_linear(self.ctx, hv, hw, exact, rocket, X0, U, S0, dt)
        except _lib.HIPError:
            return None   # (a composite-kernel GP: the host loop)

    def _gate_3dof(self, sparse_ok=False):
        """(handle, exact) when the 3-DoF device recursions apply: Rocket3DoFDynamics over a
        fitted Simple3DoFGP with a device handle -- the exact GP's, or with sparse_ok the
        shared FITC one (the linear recursion takes a gpmpc_gp only).  Else None."""
        if not self.use_device or self.n_x != 7:
            return None
        from ..dynamics.rocket_3dof import Rocket3DoFDynamics
        from ..gp.exact_gp import MultiOutputExactGP
        from ..gp.features import Simple3DoFFeatureExtractor
        from ..gp.sparse_gp import MultiOutputSparseGP
        gp = self.gp
        inner = getattr(gp, "gp", None)
        exact = isinstance(inner, MultiOutputExactGP)
        if (type(self.dynamics) is not Rocket3DoFDynamics
                or not (exact or (sparse_ok and isinstance(inner, MultiOutputSparseGP)))
                or type(getattr(gp, "feature_extractor", None)) is not Simple3DoFFeatureExtractor
                or not getattr(gp, "_is_fitted", False)):
            return None
        h = inner.device_handle
        if h is None:
            return None
        return h, exact

    def _device_3dof(self, X0, U, Sigma_0, dt):
        # (only the exact GP's handle is a gpmpc_gp; a FITC handle is another type)
        gate = self._gate_3dof()
        if gate is None:
            return None
        p = self.dynamics.params
        S0 = None
        if Sigma_0 is not None:
            S0 = np.broadcast_to(np.asarray(Sigma_0, float), (X0.shape[0], 7, 7))
        try:
            return _lib.uprop3_linear(self.ctx, gate[0], X0, U, S0, dt, float(p.alpha), np.asarray(p.g_vec, float))
        except _lib.HIPError:
            return None   # (a composite-kernel GP: the host loop)

    # ------------------------------------------------------------------ linear
    def _propagate_linear(self, x0, U, Sigma_0, dt) -> PropagatedUncertainty:
        """uncertainty_prop.py:117-177 for one trajectory (a batch of one)."""
        S0 = None if Sigma_0 is None else np.asarray(Sigma_0, float)[None]
        means, covs = self.propagate_batch(np.asarray(x0, float)[None], np.asarray(U, float)[None], S0, dt)
        return PropagatedUncertainty(means=means[0], covariances=covs[0])

    def propagate_batch(self, X0, U, Sigma_0=None, dt: float = 0.1):
        """Linear propagation of B trajectories at once.

        X0 (B, n_x), U (B, N, n_u), Sigma_0 None (the reference's 1e-6 I),
        (n_x, n_x) or (B, n_x, n_x) -> means (B, N+1, n_x), covariances
        (B, N+1, n_x, n_x).  Per horizon step: one batched GP evaluation on the
        device and the nominal step / Jacobian of every trajectory; then one
        device launch for all covariance recursions."""
        X0 = np.atleast_2d(np.asarray(X0, float)); U = np.asarray(U, float)
        if U.ndim == 2:
            U = U[None]
        B, N = U.shape[0], U.shape[1]
        nx = self.n_x
        if X0.shape != (B, nx):
            raise ValueError(f"X0 shape {X0.shape}, expected {(B, nx)}")
        dev = self._device_3dof(X0, U, Sigma_0, dt)
        if dev is None:
            dev = self._device_6dof(X0, U, Sigma_0, dt)
        if dev is not None:
            return dev
        rv, rw = self._rows()
        means = np.zeros((B, N + 1, nx)); means[:, 0] = X0
        A = np.zeros((B, N, nx, nx)); q = np.zeros((B, N, nx))
        x = X0.copy()
        for k in range(N):
            u = U[:, k]
            d_v, d_w, var_v, var_w = _gp_batch(self.gp, x, u)
            xn = np.empty_like(x)
            for b in range(B):
                A[b, k], _ = self.dynamics.linearize(x[b], u[b], dt=dt)
                xn[b] = self.dynamics.step(x[b], u[b], dt)
            xn[:, rv] += d_v * dt
            q[:, k, rv] = var_v * dt ** 2
            if rw is not None:
                xn[:, rw] += d_w * dt
                q[:, k, rw] = var_w * dt ** 2
            means[:, k + 1] = xn
            x = xn
        S0 = None
        if Sigma_0 is not None:
            S0 = np.asarray(Sigma_0, float)
            if S0.ndim == 2:
                S0 = np.broadcast_to(S0, (B, nx, nx))
        covs = _lib.cov_propagate(self.ctx, A, q, S0, 1e-6)
        return means, covs

    # --------------------------------------------------------------- unscented
    # the transform's (alpha, beta, kappa): the reference's constants (uncertainty_prop.py:196-198)
    ut_params = (1e-3, 2.0, 0.0)

    def _propagate_unscented(self, x0, U, Sigma_0, dt) -> PropagatedUncertainty:
        """uncertainty_prop.py:179-264 for one trajectory (a batch of one)."""
        S0 = None if Sigma_0 is None else np.asarray(Sigma_0, float)[None]
        U = np.atleast_2d(np.asarray(U, float))
        means, covs = self.propagate_unscented_batch(np.asarray(x0, float)[None], U[None], S0, dt)
        return PropagatedUncertainty(means=means[0], covariances=covs[0])

    def _device_unscented(self, X0, U, S0, dt):
        """The whole unscented recursion of every trajectory in one device call
        (gpmpc_uprop3_unscented / gpmpc_uprop6_unscented, csrc/uprop_ut.hip) where the gates
        of the linear device paths accept -- and for the 3-DoF model a sparse GP too.
        (means, covs, info), or None: the host loop."""
        try:
            gate = self._gate_3dof(sparse_ok=True)
            if gate is not None:
                p = self.dynamics.params
                return _lib.uprop3_unscented(self.ctx, gate[0], gate[1], X0, U, S0, dt, float(p.alpha),
                                             np.asarray(p.g_vec, float), self.ut_params)
            gate = self._gate_6dof()
            if gate is not None:
                hv, hw, exact, rocket = gate
                return _lib.uprop6_unscented(self.ctx, hv, hw, exact, rocket, X0, U, S0, dt, self.ut_params)
        except _lib.HIPError:
            pass   # (a composite-kernel GP: the host loop)
        return None

    def propagate_unscented_batch(self, X0, U, Sigma_0=None, dt: float = 0.1):
        """Unscented propagation of B trajectories at once.

        X0 (B, n_x), U (B, N, n_u), Sigma_0 None (the reference's 1e-6 I), (n_x, n_x) or
        (B, n_x, n_x) -> means (B, N+1, n_x), covariances (B, N+1, n_x, n_x).  One device
        call where _device_unscented accepts, else the host loop once per trajectory.  A
        covariance whose scaled Cholesky factor does not exist raises np.linalg.LinAlgError
        on either path."""
        X0 = np.atleast_2d(np.asarray(X0, float)); U = np.asarray(U, float)
        if U.ndim == 2:
            U = U[None]
        B, N = U.shape[0], U.shape[1]
        nx = self.n_x
        if X0.shape != (B, nx):
            raise ValueError(f"X0 shape {X0.shape}, expected {(B, nx)}")
        S0 = None
        if Sigma_0 is not None:
            S0 = np.asarray(Sigma_0, float)
            if S0.shape not in ((nx, nx), (B, nx, nx)):
                raise ValueError(f"Sigma_0 shape {S0.shape}, expected {(nx, nx)} or {(B, nx, nx)}")
            S0 = np.broadcast_to(S0, (B, nx, nx))
        dev = self._device_unscented(X0, U, S0, dt)
        if dev is not None:
            means, covs, info = dev
            bad = np.flatnonzero(info)
            if bad.size:
                b = int(bad[0])
                raise np.linalg.LinAlgError(f"unscented propagation: trajectory {b}, step {int(info[b]) - 1}: "
                                            "the scaled covariance is not positive definite")
            return means, covs
        means = np.zeros((B, N + 1, nx)); covs = np.zeros((B, N + 1, nx, nx))
        for b in range(B):
            means[b], covs[b] = self._unscented_host(X0[b], U[b], None if S0 is None else S0[b], dt)
        return means, covs

    def _unscented_host(self, x0, U, Sigma_0, dt):
        """uncertainty_prop.py:179-264; the 2n+1 sigma points and the mean point
        of a step go to the GP as one batch."""
        U = np.atleast_2d(np.asarray(U, float)).reshape(-1, 3)
        N, n = len(U), self.n_x
        if Sigma_0 is None:
            Sigma_0 = np.eye(n) * 1e-6
        alpha, beta, kappa = self.ut_params
        lam = alpha ** 2 * (n + kappa) - n
        w_m = np.full(2 * n + 1, 1 / (2 * (n + lam)))
        w_c = w_m.copy()
        w_m[0] = lam / (n + lam)
        w_c[0] = lam / (n + lam) + (1 - alpha ** 2 + beta)
        rv, rw = self._rows()
        means = np.zeros((N + 1, n)); covs = np.zeros((N + 1, n, n))
        means[0] = x0; covs[0] = Sigma_0
        x_k = np.array(x0, float); S_k = np.array(Sigma_0, float)
        for k in range(N):
            u_k = U[k]
            sq = np.linalg.cholesky((n + lam) * S_k + 1e-10 * np.eye(n))
            sp = np.zeros((2 * n + 1, n))
            sp[0] = x_k
            for i in range(n):
                sp[i + 1] = x_k + sq[:, i]
                sp[n + i + 1] = x_k - sq[:, i]
            pts = np.vstack([sp, x_k[None]])
            d_v, d_w, var_v, var_w = _gp_batch(self.gp, pts, np.broadcast_to(u_k, (len(pts), 3)))
            spn = np.array([self.dynamics.step(sp[i], u_k, dt) for i in range(2 * n + 1)])
            spn[:, rv] += d_v[:-1] * dt
            if rw is not None:
                spn[:, rw] += d_w[:-1] * dt
            x_next = np.sum(w_m[:, None] * spn, axis=0)
            S_next = np.zeros((n, n))
            for i in range(2 * n + 1):
                diff = spn[i] - x_next
                S_next += w_c[i] * np.outer(diff, diff)
            Q = np.zeros((n, n))
            Q[rv, rv] = np.diag(var_v[-1]) * dt ** 2
            if rw is not None:
                Q[rw, rw] = np.diag(var_w[-1]) * dt ** 2
            S_next += Q
            means[k + 1] = x_next; covs[k + 1] = S_next
            x_k, S_k = x_next, S_next
        return means, covs

    # ------------------------------------------------------------- Monte Carlo
    def _propagate_monte_carlo(self, x0, U, Sigma_0, dt, n_samples: int = 100) -> PropagatedUncertainty:
        """uncertainty_prop.py:266-315 for one trajectory (a batch of one)."""
        S0 = None if Sigma_0 is None else np.asarray(Sigma_0, float)[None]
        U = np.atleast_2d(np.asarray(U, float))
        means, covs = self.propagate_monte_carlo_batch(np.asarray(x0, float)[None], U[None], S0, dt, n_samples)
        return PropagatedUncertainty(means=means[0], covariances=covs[0])

    def _monte_carlo_draw(self, X0, S0, N, n_samples):
        """The draws of B trajectories from numpy's global RNG, in the order of a caller who
        loops over them with the reference: per trajectory the particles of step 0
        (multivariate_normal), then per step and particle 3 normals for d_v and, for the
        14-state model, 3 for d_omega.  -> particles0 (B, S, n), z (B, N, S, G, 3)."""
        B, n = X0.shape
        G = 2 if n == 14 else 1
        particles0 = np.empty((B, n_samples, n)); z = np.empty((B, N, n_samples, G, 3))
        for b in range(B):
            particles0[b] = np.random.multivariate_normal(X0[b], np.eye(n) * 1e-6 if S0 is None else S0[b], n_samples)
            for k in range(N):
                z[b, k] = np.random.randn(n_samples, G, 3)
        return particles0, z

    def _device_monte_carlo(self, X0, U, S0, dt, particles0, z, return_particles):
        """The whole Monte-Carlo propagation of every trajectory in one device call
        (gpmpc_uprop3_mc / gpmpc_uprop6_mc, csrc/uprop_mc.hip) where the gates of the
        unscented device path accept.  (means, covs, particles | None), or None: the host loop."""
        try:
            gate = self._gate_3dof(sparse_ok=True)
            if gate is not None:
                p = self.dynamics.params
                return _lib.uprop3_mc(self.ctx, gate[0], gate[1], X0, U, S0, particles0, z, dt, float(p.alpha),
                                      np.asarray(p.g_vec, float), return_particles)
            gate = self._gate_6dof()
            if gate is not None:
                hv, hw, exact, rocket = gate
                return _lib.uprop6_mc(self.ctx, hv, hw, exact, rocket, X0, U, S0, particles0, z, dt,
                                      return_particles)
        except _lib.HIPError:
            pass   # (a composite-kernel GP: the host loop)
        return None

    def propagate_monte_carlo_batch(self, X0, U, Sigma_0=None, dt: float = 0.1, n_samples: int = 100,
                                    return_particles: bool = False):
        """Monte-Carlo propagation of B trajectories at once.

        X0 (B, n_x), U (B, N, n_u), Sigma_0 None (the reference's 1e-6 I), (n_x, n_x) or
        (B, n_x, n_x) -> means (B, N+1, n_x), covariances (B, N+1, n_x, n_x), and with
        return_particles the particles (B, N+1, n_samples, n_x).  The draws come from numpy's
        global RNG exactly as for a caller looping over the trajectories with the reference
        (_monte_carlo_draw), on either path.  One device call where _device_monte_carlo
        accepts, else the host loop once per trajectory over the same draws."""
        X0 = np.atleast_2d(np.asarray(X0, float)); U = np.asarray(U, float)
        if U.ndim == 2:
            U = U[None]
        B, N = U.shape[0], U.shape[1]
        nx = self.n_x
        if X0.shape != (B, nx):
            raise ValueError(f"X0 shape {X0.shape}, expected {(B, nx)}")
        if n_samples < 2:
            raise ValueError(f"n_samples {n_samples}: the sample covariance needs at least 2")
        S0 = None
        if Sigma_0 is not None:
            S0 = np.asarray(Sigma_0, float)
            if S0.shape not in ((nx, nx), (B, nx, nx)):
                raise ValueError(f"Sigma_0 shape {S0.shape}, expected {(nx, nx)} or {(B, nx, nx)}")
            S0 = np.broadcast_to(S0, (B, nx, nx))
        particles0, z = self._monte_carlo_draw(X0, S0, N, n_samples)
        dev = self._device_monte_carlo(X0, U, S0, dt, particles0, z, return_particles)
        if dev is None:
            means = np.zeros((B, N + 1, nx)); covs = np.zeros((B, N + 1, nx, nx))
            paths = np.zeros((B, N + 1, n_samples, nx)) if return_particles else None
            for b in range(B):
                r = self._monte_carlo_host(X0[b], U[b], None if S0 is None else S0[b], dt, particles0[b], z[b],
                                           return_particles)
                means[b], covs[b] = r[0], r[1]
                if return_particles:
                    paths[b] = r[2]
            dev = (means, covs, paths)
        return dev if return_particles else dev[:2]

    def _monte_carlo_host(self, x0, U, Sigma_0, dt, particles0, z, return_particles=False):
        """uncertainty_prop.py:266-315 over given draws: particles0 (S, n), z (N, S, G, 3);
        the particles' GP evaluations are one batch per step.  -> (means, covs, and the
        particles (N+1, S, n) or None)."""
        U = np.atleast_2d(np.asarray(U, float)).reshape(-1, 3)
        N, n = len(U), self.n_x
        n_samples = len(particles0)
        if Sigma_0 is None:
            Sigma_0 = np.eye(n) * 1e-6
        rv, rw = self._rows()
        particles = particles0
        means = np.zeros((N + 1, n)); covs = np.zeros((N + 1, n, n))
        paths = np.zeros((N + 1, n_samples, n)) if return_particles else None
        means[0] = x0; covs[0] = Sigma_0
        if return_particles:
            paths[0] = particles0
        for k in range(N):
            u_k = U[k]
            d_v, d_w, var_v, var_w = _gp_batch(self.gp, particles, np.broadcast_to(u_k, (n_samples, 3)))
            nxt = np.array([self.dynamics.step(particles[i], u_k, dt) for i in range(n_samples)])
            nxt[:, rv] += (d_v + np.sqrt(var_v) * z[k][:, 0]) * dt
            if rw is not None:
                nxt[:, rw] += (d_w + np.sqrt(var_w) * z[k][:, 1]) * dt
            means[k + 1] = np.mean(nxt, axis=0)
            diff = nxt - means[k + 1]
            covs[k + 1] = (diff.T @ diff) / (n_samples - 1)
            if return_particles:
                paths[k + 1] = nxt
            particles = nxt
        return means, covs, paths


class ConstraintTightening:
    """uncertainty_prop.py:318-411."""

    def __init__(self, confidence: float = 0.95):
        from scipy.stats import norm
        self.confidence = confidence
        self.kappa = norm.ppf(confidence)

    def tighten_linear_constraint(self, a, b: float, mu, Sigma) -> float:
        """a^T x >= b under x ~ N(mu, Sigma): returns b + kappa sqrt(a^T Sigma a)."""
        a = np.asarray(a, float)
        return b + self.kappa * np.sqrt(a.T @ np.asarray(Sigma, float) @ a)

    def tighten_quadratic_constraint(self, x_mu, x_Sigma, constraint_func: Callable, n_samples: int = 100) -> float:
        samples = np.random.multivariate_normal(x_mu, x_Sigma, n_samples)
        g = np.array([constraint_func(s) for s in samples])
        return np.percentile(g, (1 - self.confidence) * 100)

    def compute_back_offs(self, uncertainty: PropagatedUncertainty, constraint_gradients: List) -> np.ndarray:
        N = len(uncertainty.means) - 1
        n_c = len(constraint_gradients[0]) if constraint_gradients else 0
        back = np.zeros((N, n_c))
        for k in range(N):
            S = uncertainty.covariances[k]
            for j, grad in enumerate(constraint_gradients[k] if k < len(constraint_gradients) else []):
                back[k, j] = self.kappa * np.sqrt(grad.T @ S @ grad)
        return back


class TubeBasedRobustness:
    """uncertainty_prop.py:414-468: w_{k+1} = |A_k| w_k + d_max dt on the residual rows."""

    def __init__(self, dynamics, d_max: float = 0.1):
        self.dynamics = dynamics
        self.d_max = d_max

    def compute_tube(self, X_nom, U_nom, dt: float) -> np.ndarray:
        X_nom = np.asarray(X_nom, float)
        N, n_x = len(U_nom), X_nom.shape[1]
        widths = np.zeros((N + 1, n_x))
        w = np.zeros(n_x)
        for k in range(N):
            A_d, _ = self.dynamics.linearize(X_nom[k], U_nom[k], dt=dt)
            w = np.abs(A_d) @ w
            w[4:7] += self.d_max * dt
            if n_x >= 14:
                w[11:14] += self.d_max * dt
            widths[k + 1] = w
        return widths
