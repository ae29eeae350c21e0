"""numpy restatement of the reference's Monte-Carlo uncertainty propagation
(UncertaintyPropagator._propagate_monte_carlo, uncertainty_prop.py:266-315), with the draws
taken out of the loop (TEST INFRASTRUCTURE ONLY): the CPU tests pin it to the reference's
own output (F9), the GPU tests compare the device call against it over the same draws.

The reference draws from numpy's global RNG: the particles of step 0 in one
multivariate_normal call, then per step and per particle randn(3) for d_v and randn(3) for
d_omega (a velocity-only GP: the d_v ones alone).  Per step that is one randn(S, G, 3)."""
import numpy as np


def draw(x0, Sigma_0, N, S, G):
    """The draws of one trajectory from the global RNG in the reference's order ->
    particles0 (S, n), z (N, S, G, 3)."""
    x0 = np.asarray(x0, float)
    n = x0.size
    particles0 = np.random.multivariate_normal(x0, np.eye(n) * 1e-6 if Sigma_0 is None else Sigma_0, S)
    z = np.empty((N, S, G, 3))
    for k in range(N):
        z[k] = np.random.randn(S, G, 3)
    return particles0, z


def sequential_mean(a):
    """(((a_0 + a_1) + a_2) + ...) / S over axis 0: the order the device sums in, and the
    bits of np.mean(a, axis=0) for a C-contiguous (S, n) array."""
    s = np.array(a[0], float)
    for row in a[1:]:
        s = s + row
    return s / len(a)


def propagate_mc(dynamics, gp_predict, particles0, z, U, dt, x0, Sigma_0):
    """uncertainty_prop.py:266-315 over given draws.  gp_predict(x, u) -> (d_v, d_w, var_v,
    var_w) with d_w / var_w None for a velocity-only GP (the callables of
    oracle.uprop_oracle).  -> means (N+1, n), covs (N+1, n, n), paths (N+1, S, n)."""
    x0 = np.asarray(x0, float); U = np.atleast_2d(np.asarray(U, float)).reshape(-1, 3)
    N, n, S = len(U), x0.size, len(particles0)
    means = np.zeros((N + 1, n)); covs = np.zeros((N + 1, n, n)); paths = np.zeros((N + 1, S, n))
    means[0] = x0
    covs[0] = np.eye(n) * 1e-6 if Sigma_0 is None else Sigma_0
    paths[0] = particles0
    for k in range(N):
        nxt = np.zeros((S, n))
        for i in range(S):
            x = paths[k, i]
            d_v, d_w, var_v, var_w = gp_predict(x, U[k])
            nxt[i] = dynamics.step(x, U[k], dt)
            nxt[i, 4:7] += (d_v + np.sqrt(var_v) * z[k, i, 0]) * dt
            if d_w is not None:
                nxt[i, 11:14] += (d_w + np.sqrt(var_w) * z[k, i, 1]) * dt
        means[k + 1] = sequential_mean(nxt)
        diff = nxt - means[k + 1]
        covs[k + 1] = (diff.T @ diff) / (S - 1)
        paths[k + 1] = nxt
    return means, covs, paths


def stats_bound(paths_k, means_k):
    """(numpy's covariance, the a-priori bound on another summation order of it) for one
    step's particles (S, n): two length-S dot products summed in different orders differ by
    at most 2 (S + 2) 2^-53 |D|^T |D| / (S - 1) entrywise."""
    S = len(paths_k)
    D = paths_k - means_k
    return D.T @ D / (S - 1), 2 * (S + 2) * 2.0 ** -53 * (np.abs(D).T @ np.abs(D)) / (S - 1)


def particle_tolerance(x):
    """The linear device path's tolerance (test_gpu_uprop.py: rtol 1e-9, atol 1e-10), as an array."""
    return 1e-10 + 1e-9 * np.abs(x)


def cov_perturbation_bound(paths_k, means_k):
    """The perturbation bound of the sample covariance when every particle moves by at most
    E = particle_tolerance(X) entrywise: (|D|^T E + E^T |D| + E^T E) / (S - 1), formed from
    the tolerance and the reference's particles, not from the output under test."""
    S = len(paths_k)
    D = np.abs(paths_k - means_k)
    E = particle_tolerance(paths_k)
    return (D.T @ E + E.T @ D + E.T @ E) / (S - 1)
