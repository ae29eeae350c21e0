"""numpy restatement of the reference's unscented uncertainty propagation, for tests.

UncertaintyPropagator._propagate_unscented, uncertainty_prop.py:179-264, with the transform's
(alpha, beta, kappa) as an argument (the reference hard-codes 1e-3, 2, 0):

    L = chol((n + lambda) Sigma_k + 1e-10 I)
    sp_0 = x_k,  sp_{i+1} = x_k + L[:, i],  sp_{n+i+1} = x_k - L[:, i]
    spn_i = step(sp_i, u_k) + dt d(sp_i, u_k)             on the residual rows
    x_{k+1} = sum_i w_m,i spn_i
    Sigma_{k+1} = sum_i w_c,i (spn_i - x_{k+1})(spn_i - x_{k+1})^T + diag(var(x_k, u_k) dt^2)

with the residual rows 4:7 (v-dot) and, for a 14-state GP, 11:14 (omega-dot).

Shared by tests/test_uprop_ut_check.py (no GPU: the restatement against the reference's own
output, F9) and tests/test_gpu_uprop_ut.py (the device recursion, csrc/uprop_ut.hip, against
the restatement over oracle.uprop_oracle's predictors).

gp_predict(x, u) -> (d_v, d_w, var_v, var_w), d_w / var_w None for a velocity-only GP: the
callables oracle.uprop_oracle.*_predictor return.

reverse_sum adds the terms of x_{k+1} from the last sigma point to the first.  At the
reference's alpha = 1e-3 the centre weight is lambda / (n + lambda) ~ -1e6 and the others
~ +3.6e4 each: the sum cancels six digits, and the order of the additions alone moves the
result by the noise floor of the reference's arithmetic (measured on F9: 5.0e-7 in the
means, 1.2e-10 in the covariances).  At alpha = 1 the weights are O(1) and two float64
evaluations agree to ~1e-13.
"""
from __future__ import annotations

import numpy as np

REFERENCE_UT = (1e-3, 2.0, 0.0)


def ut_weights(n, ut=REFERENCE_UT):
    """uncertainty_prop.py:196-210 -> (lambda, w_m, w_c)."""
    alpha, beta, kappa = ut
    lam = alpha ** 2 * (n + kappa) - n
    w_m = np.full(2 * n + 1, 1 / (2 * (n + lam)))
    w_c = w_m.copy()
    w_m[0] = lam / (n + lam)
    w_c[0] = lam / (n + lam) + (1 - alpha ** 2 + beta)
    return lam, w_m, w_c


def propagate_unscented(dynamics, gp_predict, x0, U, Sigma_0=None, dt=0.1, ut=REFERENCE_UT, reverse_sum=False,
                        factor=np.linalg.cholesky, weights=ut_weights):
    """uncertainty_prop.py:179-264 -> means (N+1, n), covariances (N+1, n, n).  Raises
    np.linalg.LinAlgError where the reference's np.linalg.cholesky does.  factor / weights:
    the two places a mutant of the transform replaces (tests/uprop6_check.py)."""
    x0 = np.asarray(x0, float); U = np.asarray(U, float).reshape(-1, 3)
    n, N = x0.size, len(U)
    S = np.eye(n) * 1e-6 if Sigma_0 is None else np.array(Sigma_0, float)
    lam, w_m, w_c = weights(n, ut)
    means = np.zeros((N + 1, n)); covs = np.zeros((N + 1, n, n))
    means[0] = x0; covs[0] = S
    x = x0.copy()
    for k in range(N):
        u = U[k]
        L = factor((n + lam) * S + 1e-10 * np.eye(n))
        sp = np.zeros((2 * n + 1, n))
        sp[0] = x
        for i in range(n):
            sp[i + 1] = x + L[:, i]
            sp[n + i + 1] = x - L[:, i]
        spn = np.zeros_like(sp)
        for i in range(2 * n + 1):
            d_v, d_w, _, _ = gp_predict(sp[i], u)
            spn[i] = dynamics.step(sp[i], u, dt)
            spn[i, 4:7] += d_v * dt
            if d_w is not None:
                spn[i, 11:14] += d_w * dt
        terms = w_m[:, None] * spn
        if reverse_sum:
            x_next = np.zeros(n)
            for i in range(2 * n, -1, -1):
                x_next = x_next + terms[i]
        else:
            x_next = np.sum(terms, axis=0)
        S_next = np.zeros((n, n))
        for i in range(2 * n + 1):
            diff = spn[i] - x_next
            S_next += w_c[i] * np.outer(diff, diff)
        _, _, var_v, var_w = gp_predict(x, u)
        Q = np.zeros((n, n))
        Q[4:7, 4:7] = np.diag(var_v) * dt ** 2
        if var_w is not None:
            Q[11:14, 11:14] = np.diag(var_w) * dt ** 2
        S_next += Q
        means[k + 1] = x_next; covs[k + 1] = S_next
        x, S = x_next, S_next
    return means, covs
