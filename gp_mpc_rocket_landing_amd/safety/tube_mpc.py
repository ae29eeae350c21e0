"""Tube MPC with GP uncertainty propagation (mirror of the reference's src/safety/tube_mpc.py by
name, signature, default and return value; Mayne 2014).

A tube X_k = {x : |x - x_k^nom| <= e_k} around a nominal trajectory, from one of
    e_(k+1) = |A + B K| e_k + w            (``propagate_linear``),
    e_(k+1) = |A| e_k + n_sigma sqrt(var)  (``propagate_with_gp``: the GP variance on the velocity
                                            and angular-rate rows; K is not used),
    a quantile of |x - x_nom| over particles (``propagate_monte_carlo``),
with A, B the forward differences of ``dynamics.step``; the tube then tightens the thrust,
glideslope and tilt bounds (``TubeConstraintTightener``).  The reference's quirks stay:
tubes[0] = 0, the fixed order of tries for the GP variance, the ``len(gp_std) >= 6`` mapping,
noise on all 14 rows after ``step``, the ``gp_model.sample`` branch.

Additions: the ``*_batch`` surfaces answer B trajectories (leading axis) in one call, and every
call is dispatched.  With ``Rocket6DoFDynamics`` the linearisations and the recursion, or the
particles and their quantiles, run in one device call (csrc/tube.hip); otherwise, or
with ``GPMPC_TUBE=host``, the numpy path runs, which is the reference's arithmetic statement for
statement and so returns its bits.  A ``gp_model`` with ``sample`` always runs on the host.
``last_path`` ("device" / "host") and ``last_reason`` say what ran and why; ``ctx`` is the
device context (None: the default one).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .safety_filter import rocket_gate, rocket_vector


def tube_mode() -> str:
    """GPMPC_TUBE: "host", "device" or "" (both of the latter: the device where it applies)."""
    mode = os.environ.get("GPMPC_TUBE", "").strip().lower()
    if mode not in ("", "host", "device"):
        raise ValueError(f"GPMPC_TUBE={mode!r}: expected host or device")
    return mode


@dataclass
class TubeMPCConfig:
    N: int = 15
    dt: float = 0.1
    tube_method: str = "linear"  # "linear", "nonlinear", "gp"
    w_max: float = 0.1
    gp_confidence: float = 0.95
    tightening_method: str = "additive"  # "additive", "multiplicative"


def _trajectories(X_nom, U_nom) -> Tuple[np.ndarray, np.ndarray]:
    X_nom = np.asarray(X_nom, float)
    U_nom = np.asarray(U_nom, float)
    if X_nom.ndim != 3 or U_nom.ndim != 3 or X_nom.shape[2] != 14 or U_nom.shape[2] != 3 or (
            X_nom.shape[0] != U_nom.shape[0] or X_nom.shape[1] != U_nom.shape[1] + 1):
        raise ValueError(f"shapes X_nom {X_nom.shape}, U_nom {U_nom.shape}: expected (B, N+1, 14) and (B, N, 3)")
    return X_nom, U_nom


class TubePropagator:
    """
    >>> propagator = TubePropagator(dynamics, config)
    >>> tubes, gp_vars = propagator.propagate_with_gp(X_nom, U_nom, gp_model)
    """

    def __init__(self, dynamics, config: Optional[TubeMPCConfig] = None):
        self.dynamics = dynamics
        self.config = config or TubeMPCConfig()
        self.n_x = 14  # 6-DoF
        self.n_u = 3
        self.ctx = None              # a _lib.Context; None: the default context
        self.last_path: Optional[str] = None
        self.last_reason: Optional[str] = None

    # ---- dispatch --------------------------------------------------------------------------
    def _device_gate(self, eps: float = 1e-6, gp_model=None, n_samples: Optional[int] = None) -> Tuple[bool, str]:
        """(True, why) when csrc/tube.hip restates the call exactly, else (False, why).  Host
        logic only: no device call."""
        if tube_mode() == "host":
            return False, "GPMPC_TUBE=host"
        why = rocket_gate(self.dynamics)
        if why is not None:
            return False, why
        dt = self.config.dt
        if not (isinstance(dt, (int, float, np.floating, np.integer)) and np.isfinite(dt) and dt > 0):
            return False, f"dt = {dt!r} is not positive and finite"
        if not (np.isfinite(eps) and eps != 0):
            return False, f"eps = {eps!r} is not finite and non-zero"
        if gp_model is not None and hasattr(gp_model, "sample"):
            return False, "gp_model.sample draws on the host"
        try:
            from .. import _lib
        except (ImportError, OSError) as e:
            return False, f"the library does not load: {e}"
        if n_samples is not None:
            cap = _lib.tube_plan(0, 0)[1]
            if not 1 <= int(n_samples) <= cap:
                return False, f"n_samples = {n_samples} is outside 1..{cap}"
        return True, "Rocket6DoFDynamics"

    def _dispatch(self, **kw) -> bool:
        ok, why = self._device_gate(**kw)
        self.last_path, self.last_reason = ("device" if ok else "host"), why
        return ok

    def _context(self):
        from .. import _lib
        return self.ctx if self.ctx is not None else _lib.default_context()

    # ---- the reference's arithmetic (host) ---------------------------------------------
    def _linearize_host(self, x, u, eps: float = 1e-6) -> Tuple[np.ndarray, np.ndarray]:
        dt = self.config.dt
        A = np.zeros((self.n_x, self.n_x))
        B = np.zeros((self.n_x, self.n_u))
        x_next_nom = self.dynamics.step(x, u, dt)
        for i in range(self.n_x):
            x_pert = x.copy()
            x_pert[i] += eps
            x_next = self.dynamics.step(x_pert, u, dt)
            A[:, i] = (x_next - x_next_nom) / eps
        for i in range(self.n_u):
            u_pert = u.copy()
            u_pert[i] += eps
            x_next = self.dynamics.step(x, u_pert, dt)
            B[:, i] = (x_next - x_next_nom) / eps
        return A, B

    def _linear_host(self, X_nom, U_nom, w_bounds, K) -> np.ndarray:
        """propagate_linear for one trajectory; w_bounds (14,) or one row per step (N, 14)."""
        N = len(U_nom)
        tubes = np.zeros((N + 1, self.n_x))
        tubes[0] = 0  # No uncertainty at initial state
        for k in range(N):
            A, B = self._linearize_host(X_nom[k], U_nom[k])
            A_cl = A + B @ K if K is not None else A
            tubes[k + 1] = np.abs(A_cl) @ tubes[k] + (w_bounds if w_bounds.ndim == 1 else w_bounds[k])
        return tubes

    def _monte_carlo_host(self, X_nom, U_nom, gp_model, n_samples, quantile, noise) -> np.ndarray:
        """propagate_monte_carlo for one trajectory; noise (N, n_samples, 14): the trajectory's
        draws, already times w_max (None with ``gp_model.sample``)."""
        N = len(U_nom)
        particles = np.tile(X_nom[0], (n_samples, 1))
        tubes = np.zeros((N + 1, self.n_x))
        tubes[0] = 0
        for k in range(N):
            next_particles = np.zeros_like(particles)
            for i, x in enumerate(particles):
                x_next = self.dynamics.step(x, U_nom[k], self.config.dt)
                if hasattr(gp_model, "sample"):
                    d = gp_model.sample(x.reshape(1, -1), U_nom[k:k + 1])
                    x_next[4:7] += d[:3].flatten() * self.config.dt
                    x_next[11:14] += d[3:6].flatten() * self.config.dt
                else:
                    x_next += noise[k, i]
                next_particles[i] = x_next
            particles = next_particles
            deviations = np.abs(particles - X_nom[k + 1])
            tubes[k + 1] = np.quantile(deviations, quantile, axis=0)
        return tubes

    # ---- the GP variance along the nominal points ------------------------------------------
    def _gp_variances(self, X_nom, U_nom, gp_model, batched: bool, structured_ok: bool) -> np.ndarray:
        """(B, N, n_outputs): the variance the reference reads at every nominal point, by its
        order of tries.  batched: this package's GPs answer all B N points in one posterior;
        otherwise, and for any other object, row by row exactly as the reference asks."""
        from ..gp.exact_gp import MultiOutputExactGP
        from ..gp.sparse_gp import MultiOutputSparseGP
        from ..gp.structured_gp import StructuredRocketGP
        B, N = U_nom.shape[:2]
        structured = structured_ok and type(gp_model) is StructuredRocketGP
        if batched and N:
            Xf, Uf = X_nom[:, :N].reshape(B * N, 14), U_nom.reshape(B * N, 3)
            if structured:
                _, _, vv, vw = gp_model.predict_batch(Xf, Uf)
                return np.concatenate([vv, vw], axis=1).reshape(B, N, 6)
            if (type(gp_model) in (MultiOutputExactGP, MultiOutputSparseGP) and gp_model.input_dim == 14
                    and gp_model.device_handle is not None):
                _, var = gp_model.predict(Xf)
                return np.asarray(var, float).reshape(B, N, -1)
        out = []
        for b in range(B):
            gp_vars = []
            for k in range(N):
                if structured:
                    _, _, vv, vw = gp_model.predict_batch(X_nom[b, k:k + 1], U_nom[b, k:k + 1])
                    d_var = np.concatenate([vv, vw], axis=1)
                elif hasattr(gp_model, "predict_with_uncertainty"):
                    _, d_var = gp_model.predict_with_uncertainty(X_nom[b, k:k + 1], U_nom[b, k:k + 1])
                elif hasattr(gp_model, "predict"):
                    # Assume predict returns (mean, var)
                    _, d_var = gp_model.predict(X_nom[b, k:k + 1])
                    if isinstance(d_var, tuple):
                        d_var = d_var[0]
                else:
                    # No GP - use constant bounds
                    d_var = np.ones(6) * self.config.w_max**2
                gp_vars.append(d_var.flatten())
            out.append(np.array(gp_vars))
        return np.array(out)

    def _gp_bounds(self, gp_vars, n_sigma) -> np.ndarray:
        """The reference's mapping of the GP's standard deviations onto the state rows: six or
        more outputs on rows 4:7 and 11:14, fewer on rows 4:7 (numpy's broadcast: one output
        fills the three rows, two raise)."""
        gp_std = np.sqrt(gp_vars)
        w = np.zeros(gp_vars.shape[:2] + (self.n_x,))
        n = gp_vars.shape[2] if gp_vars.ndim == 3 else 0
        if n >= 6:
            w[..., 4:7] = gp_std[..., :3] * n_sigma
            w[..., 11:14] = gp_std[..., 3:6] * n_sigma
        elif w.shape[1]:
            w[..., 4:7] = gp_std[..., :min(3, n)] * n_sigma
        return w

    # ---- batch surfaces --------------------------------------------------------------------
    def linearize_batch(self, X, U, eps: float = 1e-6) -> Tuple[np.ndarray, np.ndarray]:
        """``_linearize`` at P points X (P, 14), U (P, 3): A (P, 14, 14), B (P, 14, 3)."""
        X = np.atleast_2d(np.asarray(X, float))
        U = np.atleast_2d(np.asarray(U, float))
        P = len(X)
        if X.shape != (P, self.n_x) or U.shape != (P, self.n_u):
            raise ValueError(f"linearize_batch: shapes X {X.shape}, U {U.shape}")
        if P and self._dispatch(eps=eps):
            from .. import _lib
            X2 = np.zeros((P, 2, self.n_x))
            X2[:, 0] = X
            _, A, Bm = _lib.tube_linear(self._context(), rocket_vector(self.dynamics), X2, U[:, None, :],
                                        self.config.dt, eps=eps, w_max=0.0, return_AB=True)
            return A[:, 0], Bm[:, 0]
        if not P:
            self.last_path, self.last_reason = "host", "no points"
        A = np.zeros((P, self.n_x, self.n_x))
        Bm = np.zeros((P, self.n_x, self.n_u))
        for p in range(P):
            A[p], Bm[p] = self._linearize_host(X[p], U[p], eps)
        return A, Bm

    def _tubes(self, X_nom, U_nom, w, K, device: bool) -> np.ndarray:
        """e_(k+1) = |A + B K| e_k + w_k for every trajectory; w: (14,) or (B, N, 14)."""
        B, N = U_nom.shape[:2]
        if device and B and N:
            from .. import _lib
            return _lib.tube_linear(self._context(), rocket_vector(self.dynamics), X_nom, U_nom, self.config.dt,
                                    w=w, K=K)
        if device:
            self.last_path, self.last_reason = "host", "nothing to propagate"
        tubes = np.zeros((B, N + 1, self.n_x))
        for b in range(B):
            tubes[b] = self._linear_host(X_nom[b], U_nom[b], w if w.ndim == 1 else w[b], K)
        return tubes

    def propagate_linear_batch(self, X_nom, U_nom, w_bounds=None, K=None) -> np.ndarray:
        """``propagate_linear`` for B trajectories X_nom (B, N+1, 14), U_nom (B, N, 3); w_bounds
        None (w_max), (14,) or (B, N, 14); K None or (3, 14) -> tubes (B, N+1, 14)."""
        X_nom, U_nom = _trajectories(X_nom, U_nom)
        B, N = U_nom.shape[:2]
        if w_bounds is None:
            w_bounds = np.ones(self.n_x) * self.config.w_max
        w_bounds = np.asarray(w_bounds, float)
        if w_bounds.shape not in ((self.n_x,), (B, N, self.n_x)):
            raise ValueError(f"w_bounds shape {w_bounds.shape}, expected {(self.n_x,)} or {(B, N, self.n_x)}")
        if K is not None:
            K = np.asarray(K, float)
            if K.shape != (self.n_u, self.n_x):
                raise ValueError(f"K shape {K.shape}, expected {(self.n_u, self.n_x)}")
        return self._tubes(X_nom, U_nom, w_bounds, K, self._dispatch())

    def _with_gp(self, X_nom, U_nom, gp_model, n_sigma, structured_ok) -> Tuple[np.ndarray, np.ndarray]:
        X_nom, U_nom = _trajectories(X_nom, U_nom)
        device = self._dispatch()
        gp_vars = self._gp_variances(X_nom, U_nom, gp_model, device, structured_ok)
        w = self._gp_bounds(gp_vars, n_sigma)
        return self._tubes(X_nom, U_nom, w, None, device), gp_vars

    def propagate_with_gp_batch(self, X_nom, U_nom, gp_model, n_sigma: float = 2.0) -> Tuple[np.ndarray, np.ndarray]:
        """``propagate_with_gp`` for B trajectories -> tubes (B, N+1, 14), gp_vars (B, N,
        n_outputs).  Besides what the reference reads, a ``StructuredRocketGP`` is accepted:
        ``predict_batch(X, U)`` as [var_v, var_w]."""
        return self._with_gp(X_nom, U_nom, gp_model, n_sigma, True)

    def _monte_carlo_draw(self, B, N, n_samples) -> np.ndarray:
        """The draws of B trajectories from numpy's global RNG, in the order of a caller who loops
        over them with the reference (per step and particle ``randn(14) * w_max``): one block
        per trajectory has those bits.  -> (B, N, n_samples, 14)."""
        noise = np.empty((B, N, n_samples, self.n_x))
        for b in range(B):
            noise[b] = np.random.randn(N, n_samples, self.n_x) * self.config.w_max
        return noise

    def propagate_monte_carlo_batch(self, X_nom, U_nom, gp_model, n_samples: int = 100,
                                    quantile: float = 0.95) -> np.ndarray:
        """``propagate_monte_carlo`` for B trajectories -> tubes (B, N+1, 14).  Trajectory b draws
        after trajectory b - 1, so the result is the reference's called in a loop."""
        X_nom, U_nom = _trajectories(X_nom, U_nom)
        B, N = U_nom.shape[:2]
        device = self._dispatch(gp_model=gp_model, n_samples=n_samples)
        if device and not 0.0 <= quantile <= 1.0:   # np.quantile raises, as in the reference
            device, self.last_path, self.last_reason = False, "host", f"quantile = {quantile!r} is outside [0, 1]"
        if device and not (B and N):
            device, self.last_path, self.last_reason = False, "host", "nothing to propagate"
        sampled = hasattr(gp_model, "sample")
        noise = None if sampled else self._monte_carlo_draw(B, N, n_samples)
        if device:
            from .. import _lib
            return _lib.tube_mc(self._context(), rocket_vector(self.dynamics), X_nom, U_nom, noise, self.config.dt,
                                quantile)
        tubes = np.zeros((B, N + 1, self.n_x))
        for b in range(B):
            tubes[b] = self._monte_carlo_host(X_nom[b], U_nom[b], gp_model, n_samples, quantile,
                                              None if sampled else noise[b])
        return tubes

    # ---- the reference's surfaces: the batch of one ------------------------------------------
    def propagate_linear(self, X_nom, U_nom, w_bounds=None, K=None) -> np.ndarray:
        """e_{k+1} = |A_cl| @ e_k + w_max: X_nom (N+1, n_x), U_nom (N, n_u) -> tubes (N+1, n_x)."""
        return self.propagate_linear_batch(np.asarray(X_nom, float)[None], np.asarray(U_nom, float)[None],
                                           w_bounds, K)[0]

    def propagate_with_gp(self, X_nom, U_nom, gp_model, n_sigma: float = 2.0) -> Tuple[np.ndarray, np.ndarray]:
        """Tubes from the GP's predictive variance -> tubes (N+1, n_x), gp_vars (N, n_gp_outputs)."""
        tubes, gp_vars = self._with_gp(np.asarray(X_nom, float)[None], np.asarray(U_nom, float)[None], gp_model,
                                       n_sigma, False)
        return tubes[0], gp_vars[0]

    def propagate_monte_carlo(self, X_nom, U_nom, gp_model, n_samples: int = 100, quantile: float = 0.95) -> np.ndarray:
        """Tubes as a quantile of the particles' deviation from the nominal -> (N+1, n_x)."""
        return self.propagate_monte_carlo_batch(np.asarray(X_nom, float)[None], np.asarray(U_nom, float)[None],
                                                gp_model, n_samples, quantile)[0]

    def _linearize(self, x, u, eps: float = 1e-6) -> Tuple[np.ndarray, np.ndarray]:
        """Numerical linearization."""
        A, B = self.linearize_batch(np.asarray(x, float)[None], np.asarray(u, float)[None], eps)
        return A[0], B[0]


class TubeConstraintTightener:
    """Given constraints g(x) >= 0, the tightened ones that hold for every x in the tube.  Host
    arithmetic throughout (``get_tightened_params_batch``: vectorised numpy)."""

    def __init__(self, constraint_params=None):
        self.params = constraint_params
        self.ctx = None
        self.last_path: Optional[str] = None
        self.last_reason: Optional[str] = None

    def _ran(self):
        self.last_path, self.last_reason = "host", "constraint tightening is host arithmetic"

    def tighten_thrust_bounds(self, tube_u) -> Tuple[float, float]:
        T_min = getattr(self.params, "T_min", 0.5) if self.params else 0.5
        T_max = getattr(self.params, "T_max", 5.0) if self.params else 5.0
        margin = np.linalg.norm(tube_u)
        return T_min + margin, T_max - margin

    def tighten_glideslope(self, tube_x, gamma: float) -> float:
        pos_uncertainty = np.linalg.norm(tube_x[1:4])
        gamma_rad = np.deg2rad(gamma)
        if pos_uncertainty > 0:
            altitude = max(tube_x[1], 1.0)  # Avoid division by zero
            angle_margin = np.arctan(pos_uncertainty / altitude)
            gamma_tight = gamma_rad - angle_margin
            return np.rad2deg(max(gamma_tight, np.deg2rad(10)))
        return gamma

    def tighten_tilt_angle(self, tube_x, theta_max: float) -> float:
        quat_uncertainty = np.linalg.norm(tube_x[7:11])
        omega_uncertainty = np.linalg.norm(tube_x[11:14])
        theta_margin = np.rad2deg(quat_uncertainty + 0.1 * omega_uncertainty)
        return max(theta_max - theta_margin, 10.0)

    def get_tightened_params(self, tubes, timestep: int) -> dict:
        self._ran()
        tube_x = tubes[timestep]
        gamma = getattr(self.params, "gamma_gs", 30.0) if self.params else 30.0
        theta = getattr(self.params, "theta_max", 60.0) if self.params else 60.0
        tube_u = tube_x[4:7] * 0.5  # Heuristic
        T_min_t, T_max_t = self.tighten_thrust_bounds(tube_u)
        gamma_t = self.tighten_glideslope(tube_x, gamma)
        theta_t = self.tighten_tilt_angle(tube_x, theta)
        return {"T_min": T_min_t, "T_max": T_max_t, "gamma_gs": gamma_t, "theta_max": theta_t, "tube_width": tube_x}

    def get_tightened_params_batch(self, tubes) -> dict:
        """``get_tightened_params`` at every tube width of tubes (..., 14) at once: a dict of
        arrays of the leading shape (``tube_width``: tubes itself)."""
        self._ran()
        tubes = np.asarray(tubes, float)
        if tubes.ndim < 1 or tubes.shape[-1] != 14:
            raise ValueError(f"tubes shape {tubes.shape}, expected (..., 14)")
        T_min = getattr(self.params, "T_min", 0.5) if self.params else 0.5
        T_max = getattr(self.params, "T_max", 5.0) if self.params else 5.0
        gamma = getattr(self.params, "gamma_gs", 30.0) if self.params else 30.0
        theta = getattr(self.params, "theta_max", 60.0) if self.params else 60.0

        def norm(v):
            return np.sqrt(np.sum(v * v, axis=-1))

        margin = norm(tubes[..., 4:7] * 0.5)
        pos = norm(tubes[..., 1:4])
        with np.errstate(invalid="ignore"):
            altitude = np.maximum(tubes[..., 1], 1.0)
            tight = np.rad2deg(np.maximum(np.deg2rad(gamma) - np.arctan(pos / altitude), np.deg2rad(10)))
            gamma_t = np.where(pos > 0, tight, gamma)
            theta_margin = np.rad2deg(norm(tubes[..., 7:11]) + 0.1 * norm(tubes[..., 11:14]))
            theta_t = np.maximum(theta - theta_margin, 10.0)
        return {"T_min": T_min + margin, "T_max": T_max - margin, "gamma_gs": gamma_t, "theta_max": theta_t,
                "tube_width": tubes}


class RobustTubeMPC:
    """
    >>> tube_mpc = RobustTubeMPC(dynamics, config)
    >>> tube_mpc.set_gp_model(gp)
    >>> tubes = tube_mpc.compute_tubes(X_nom, U_nom)
    >>> tightened = tube_mpc.get_tightened_constraints(tubes)
    """

    def __init__(self, dynamics, config: Optional[TubeMPCConfig] = None, constraint_params=None):
        self.dynamics = dynamics
        self.config = config or TubeMPCConfig()
        self.propagator = TubePropagator(dynamics, self.config)
        self.tightener = TubeConstraintTightener(constraint_params)
        self._gp_model = None
        self._K_tube: Optional[np.ndarray] = None

    # what ran is the propagator's; the context is handed on to it
    @property
    def ctx(self):
        return self.propagator.ctx

    @ctx.setter
    def ctx(self, value):
        self.propagator.ctx = value

    @property
    def last_path(self) -> Optional[str]:
        return self.propagator.last_path

    @property
    def last_reason(self) -> Optional[str]:
        return self.propagator.last_reason

    def set_gp_model(self, gp_model) -> None:
        self._gp_model = gp_model

    def set_tube_controller(self, K) -> None:
        self._K_tube = K

    def compute_tubes(self, X_nom, U_nom) -> np.ndarray:
        if self._gp_model is not None:
            tubes, _ = self.propagator.propagate_with_gp(X_nom, U_nom, self._gp_model)
        else:
            tubes = self.propagator.propagate_linear(X_nom, U_nom, K=self._K_tube)
        return tubes

    def compute_tubes_batch(self, X_nom, U_nom) -> np.ndarray:
        """``compute_tubes`` for B trajectories -> tubes (B, N+1, 14)."""
        if self._gp_model is not None:
            tubes, _ = self.propagator.propagate_with_gp_batch(X_nom, U_nom, self._gp_model)
        else:
            tubes = self.propagator.propagate_linear_batch(X_nom, U_nom, K=self._K_tube)
        return tubes

    def get_tightened_constraints(self, tubes) -> List[dict]:
        return [self.tightener.get_tightened_params(tubes, k) for k in range(len(tubes))]

    def get_tightened_constraints_batch(self, tubes) -> dict:
        """The tightened parameters at every step of every tube of tubes (B, N+1, 14): a dict of
        (B, N+1) arrays."""
        return self.tightener.get_tightened_params_batch(tubes)

    def check_tube_containment(self, x_actual, x_nominal, tube_width) -> bool:
        deviation = np.abs(x_actual - x_nominal)
        return np.all(deviation <= tube_width * 1.1)  # Small margin
