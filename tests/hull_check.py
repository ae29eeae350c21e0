"""A plain restatement of the gpmpc_hull_project contract (include/gpmpc.h), exact
independent answers for it, and the cases the device test runs.  Not itself a test.

``wolfe`` is the contract: Wolfe's minimum-norm-point method on w_i = v_i - x, started at the
vertex nearest x, the corral's system (s e e' + Q Q') u = e with s = max |w_i|^2 solved afresh
each minor cycle by elimination without pivoting, ties to the lower index, one cycle a major or
a minor step, the statuses 0 .. 3.  It follows the device's steps, not its summation order.

Exact answers, none of which shares a line with ``wolfe``:
- ``face_enum``: every affinely independent subset's minimum-norm point in np.longdouble, the
  nearest of those with non-negative weights (K <= 8);
- ``simplex_answer``: vertices c e_1 .. c e_d, the sort-based projection onto the simplex;
- ``cross_answer``: vertices +-c e_i, the sort-based projection onto the l1 ball;
- ``segment_answer``: collinear vertices, the clamped foot of the perpendicular.
``certificate`` recomputes min lambda, |sum lambda - 1| and the relative gap from lambda alone
in np.longdouble.

Accuracy measured on the CPU (tests/test_hull_check.py prints it):
E = max ``rel_err`` (|p_wolfe - p_exact| / max |w|) per family, over the cases below:
    face enumeration (K <= 8)  8.3e-16
    simplex                    9.3e-16
    cross-polytope             1.2e-15
    segment                    3.0e-17
E is the largest of them, 1.2e-15, and the device gets 8 E: DEVICE_BOUND = 9.6e-15 (its sums run
in another order and with FMA contraction, which changes roundings and now and then the pivot
path, not the conditioning).  Where no closed form exists the device is held to the
restatement by the same bound.  tests/test_hull_check.py prints the figures and holds the
restatement to 2 E: its sums are numpy reductions, not BLAS calls, so that they do not depend on
the machine's BLAS kernels, but the last digit of a figure is not promised across numpy builds.
"""
import itertools

import numpy as np

TOL = 1e-12
MAX_ITER = 4096
E_MEASURED = 1.2e-15
DEVICE_BOUND = 8 * E_MEASURED
LD = np.longdouble


# ---- the contract ---------------------------------------------------------------------
def wolfe(V, x, q=None, tol=TOL, max_iter=MAX_ITER):
    """-> dict(lam (K,), proj (d,), dist, gap, qhull, iters, status)."""
    V = np.asarray(V, np.float64).reshape(-1, len(x)); x = np.asarray(x, np.float64)
    K, d = V.shape
    if K == 0:
        return dict(lam=np.zeros(0), proj=x.copy(), dist=np.inf, gap=0.0, qhull=np.inf, iters=0, status=2)
    with np.errstate(all="ignore"):
        W = V - x
        nrm2 = np.sum(W * W, axis=1)
    if not np.all(np.isfinite(nrm2)):
        nan = np.full(K, np.nan)
        return dict(lam=nan, proj=np.full(d, np.nan), dist=np.nan, gap=np.nan, qhull=np.nan, iters=0, status=3)
    maxn = float(np.max(nrm2)); s = maxn
    lam = np.zeros(K)
    j0 = int(np.argmin(nrm2))                       # ties: the lower index
    lam[j0] = 1.0
    S = [j0]                                        # the corral, by slot
    G = np.zeros((d + 2, d + 2))
    G[0, 0] = s + nrm2[j0]

    def evaluate():                                 # sums written as numpy reductions, not BLAS calls:
        p = np.sum(lam[S][:, None] * W[S], axis=0)  # the same bits on every machine
        return p, float(np.sum(p * p)), np.sum(W * p, axis=1)

    status, minor, cycle = 1, False, 0
    for cycle in range(max_iter):
        if not minor:
            p, pp, pw = evaluate()
            j = int(np.argmin(pw))
            if pp - pw[j] <= tol * maxn:
                status = 0
                break
            if j in S or len(S) == d + 1:
                break
            m = len(S)
            g = s + np.sum(W[S + [j]] * W[j], axis=1)
            G[:m + 1, m] = g
            G[m, :m + 1] = g
            S.append(j)
            minor = True
            continue
        m = len(S)
        A = np.concatenate([G[:m, :m], np.ones((m, 1))], axis=1)
        ok = True
        diag = np.ones(m)
        for k in range(m):
            piv = A[k, k]
            if not piv > 0.0:
                ok = False
                break
            f = A[:, k] / piv
            f[k] = 0.0
            diag[k] = piv
            A = A - np.outer(f, A[k])
        if not ok:
            break
        u = A[:, m] / diag
        su = float(np.sum(u))
        if not su > 0.0 or not np.all(np.isfinite(u / su)):
            break
        al = u / su
        if np.all(al > 0.0):
            lam[:] = 0.0
            lam[S] = al
            minor = False
            continue
        cur = lam[S]
        den = cur - al
        th = np.where(al > 0.0, np.inf, np.where(den > 0.0, cur / np.where(den > 0.0, den, 1.0), 0.0))
        theta = float(np.min(th))
        cand = [S[c] for c in range(m) if th[c] == theta]
        r = min(cand)                               # ties: the lower index
        new = np.maximum(cur + min(theta, 1.0) * (al - cur), 0.0)
        lam[S] = new
        lam[r] = 0.0
        rs, last = S.index(r), m - 1
        if rs != last:                              # the last slot moves into the freed one
            G[rs, :m] = G[last, :m]
            G[:m, rs] = G[:m, last]
            G[rs, rs] = G[last, last]
            S[rs] = S[last]
        S.pop()
    p, pp, pw = evaluate()
    gap = (pp - float(np.min(pw))) / maxn if maxn > 0.0 else 0.0
    return dict(lam=lam, proj=x + p, dist=float(np.sqrt(pp)), gap=gap,
                qhull=float(np.sum(lam * np.asarray(q, np.float64))) if q is not None else None,
                iters=min(cycle + 1, max_iter), status=status)


# ---- exact answers ------------------------------------------------------------------------
def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in longdouble; None when singular to 1e-15."""
    A = np.array(A, LD); b = np.array(b, LD)
    n = len(b)
    scale = np.max(np.abs(A)) if n else LD(1)
    for k in range(n):
        i = k + int(np.argmax(np.abs(A[k:, k])))
        if not np.abs(A[i, k]) > LD(1e-15) * scale:
            return None
        if i != k:
            A[[k, i]] = A[[i, k]]
            b[[k, i]] = b[[i, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:] -= np.outer(f, A[k])
        b[k + 1:] -= f * b[k]
    y = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        y[k] = (b[k] - A[k, k + 1:] @ y[k + 1:]) / A[k, k]
    return y


def face_enum(V, x):
    """The projection of x onto Conv(V) (longdouble), K <= 8: the nearest minimum-norm point of
    an affinely independent subset whose weights are non-negative."""
    W = np.asarray(V, LD) - np.asarray(x, LD)
    K = len(W)
    assert 1 <= K <= 8
    best, best_n = None, None
    for size in range(1, K + 1):
        for sub in itertools.combinations(range(K), size):
            w0 = W[sub[0]]
            if size == 1:
                p = w0
            else:
                Bm = W[list(sub[1:])] - w0
                beta = _solve_ld(Bm @ Bm.T, -(Bm @ w0))
                if beta is None or np.any(beta < 0) or np.sum(beta) > 1:
                    continue
                p = w0 + beta @ Bm
            n2 = p @ p
            if best is None or n2 < best_n:
                best, best_n = p, n2
    return np.asarray(x, LD) + best


def _simplex_ld(y, c):
    """Euclidean projection of y onto {z >= 0, sum z = c} (sort-based), longdouble."""
    y = np.asarray(y, LD)
    u = np.sort(y)[::-1]
    css = np.cumsum(u) - LD(c)
    k = np.arange(1, len(y) + 1).astype(LD)
    rho = int(np.nonzero(u - css / k > 0)[0][-1])
    return np.maximum(y - css[rho] / LD(rho + 1), LD(0))


def simplex_answer(x, c):
    """Vertices c e_1 .. c e_d."""
    return _simplex_ld(x, c)


def cross_answer(x, c):
    """Vertices +-c e_i: the l1 ball of radius c."""
    x = np.asarray(x, LD)
    if np.sum(np.abs(x)) <= LD(c):
        return x
    return np.sign(x) * _simplex_ld(np.abs(x), c)


def segment_answer(V, x):
    """Collinear vertices: the clamped foot of the perpendicular on the longest chord."""
    V = np.asarray(V, LD); x = np.asarray(x, LD)
    i, j = max(itertools.combinations(range(len(V)), 2), key=lambda ij: np.sum((V[ij[0]] - V[ij[1]]) ** 2))
    u = V[j] - V[i]
    t = np.clip(((x - V[i]) @ u) / (u @ u), LD(0), LD(1))
    return V[i] + t * u


def certificate(V, x, lam):
    """(min lambda, |sum lambda - 1|, relative gap) from lambda alone, longdouble."""
    W = np.asarray(V, LD) - np.asarray(x, LD)
    lam = np.asarray(lam, LD)
    p = lam @ W
    maxn = np.max(np.sum(W * W, axis=1))
    gap = (p @ p - np.min(W @ p)) / maxn if maxn > 0 else LD(0)
    return float(np.min(lam)), float(np.abs(np.sum(lam) - 1)), float(gap)


def max_w(V, x):
    return float(np.sqrt(np.max(np.sum((np.asarray(V, np.float64) - x) ** 2, axis=1))))


def rel_err(proj, exact, V, x):
    """|proj - exact| / max |w|, less the one rounding fp64 cannot avoid when it stores proj = x + p
    (2^-53 |exact|: what shows at an offset of 1e4 and |w| of order 1 is that rounding alone)."""
    exact = np.asarray(exact, LD)
    e = float(np.sqrt(np.sum((np.asarray(proj, LD) - exact) ** 2))) - 2.0 ** -53 * float(np.sqrt(exact @ exact))
    mw = max_w(V, x)
    return max(e, 0.0) / mw if mw > 0 else max(e, 0.0)


# ---- the cases of the device test ----------------------------------------------------------
DS = [1, 2, 3, 7, 14, 31, 32]
DISTINCT = 10      # distinct cases of a (d, K); the batch of 70 cycles through them
BATCH = 70


def ks_of(d):
    return sorted({min(k, 64) for k in (1, 2, d, d + 1, d + 2, 10, 50, 63, 64)})


def random_cases(d, K):
    """DISTINCT cases (tag, V, x) of K vertices in d dimensions: the families of the device test."""
    rng = np.random.default_rng(1000 * d + K)
    out = []
    V = rng.standard_normal((K, d))
    out.append(("interior", V, rng.dirichlet(np.ones(K)) @ V))
    i = int(rng.integers(K))
    out.append(("vertex", V, V[i].copy()))
    out.append(("far", V, 50.0 * rng.standard_normal(d) + 100.0))
    out.append(("near", V, 1.5 * rng.standard_normal(d)))
    half = (K + 1) // 2
    Vd = np.concatenate([V[:half], V[:half]])[:K] if K > 1 else V
    out.append(("duplicated", Vd, 2.0 * rng.standard_normal(d)))
    out.append(("identical", np.tile(V[:1], (K, 1)), rng.standard_normal(d)))
    out.append(("vertex_dup", Vd, Vd[K - 1].copy()))
    for mag, off in ((1e-3, 0.0), (1.0, 1e4), (1e6, 1e4)):
        Vm = mag * rng.standard_normal((K, d)) + off
        out.append((f"mag{mag:g}", Vm, mag * 1.5 * rng.standard_normal(d) + off))
    assert len(out) == DISTINCT
    return out


def simplex_cases():
    """(tag, V, x, exact): c e_1 .. c e_d for d = K in 2 .. 32."""
    rng = np.random.default_rng(5)
    out = []
    for d in (2, 3, 7, 14, 31, 32):
        for c in (1.0, 3.5):
            for scale in (0.3, 2.0):
                x = scale * c * rng.standard_normal(d)
                out.append((f"simplex{d}", c * np.eye(d), x, simplex_answer(x, c)))
    return out


def cross_cases():
    """(tag, V, x, exact): +-c e_i, K = 2 d (64 at d = 32)."""
    rng = np.random.default_rng(6)
    out = []
    for d in (1, 3, 14, 32):
        for c, scale in ((1.0, 2.0), (2.5, 1.0), (1.0, 0.02)):
            x = scale * c * rng.standard_normal(d)
            V = np.concatenate([c * np.eye(d), -c * np.eye(d)])
            out.append((f"cross{d}", V, x, cross_answer(x, c)))
    return out


def segment_cases():
    """(tag, V, x, exact): K collinear vertices at dyadic parameters (the rows are exactly collinear)."""
    rng = np.random.default_rng(7)
    out = []
    for d, K in ((2, 3), (7, 10), (14, 50), (32, 64)):
        a = np.round(rng.standard_normal(d) * 8) / 8
        u = np.round(rng.standard_normal(d) * 8) / 8
        u[0] = 1.0
        t = rng.permutation(K).astype(float) / 64.0
        V = a + t[:, None] * u
        for x in (a + 0.37 * u + rng.standard_normal(d), a - 3.0 * u + rng.standard_normal(d),
                  a + 4.0 * u + 0.1 * rng.standard_normal(d)):
            out.append((f"segment{d}", V, x, segment_answer(V, x)))
    return out


def trajectory_set(n_traj=6, steps=40, seed=11):
    """A small synthetic 7-state safe set [m, r(3), v(3)]: descents to the pad; -> states, Q."""
    rng = np.random.default_rng(seed)
    rows, q = [], []
    for _ in range(n_traj):
        r = np.array([30.0, 4.0, -3.0]) + rng.standard_normal(3) * np.array([5.0, 2.0, 2.0])
        v = np.array([-6.0, 0.0, 0.0]) + rng.standard_normal(3)
        m = 2.0 + 0.2 * rng.standard_normal()
        for k in range(steps):
            rows.append(np.concatenate([[m], r, v]))
            q.append(float(steps - k))
            acc = -0.4 * r - 0.9 * v
            v = v + 0.1 * acc
            r = r + 0.1 * v
            m = m - 0.002 * np.linalg.norm(acc)
    return np.array(rows), np.array(q)


def trajectory_cases(K=10, n_queries=12):
    """(tag, V, x): the K nearest rows of the trajectory set around states near it."""
    S, _ = trajectory_set()
    rng = np.random.default_rng(12)
    out = []
    for _ in range(n_queries):
        x = S[int(rng.integers(len(S)))] + 0.3 * rng.standard_normal(7)
        near = np.argsort(np.sum((S - x) ** 2, axis=1), kind="stable")[:K]
        out.append(("trajectory", S[near], x))
    return out


RAGGED = ((3, 10), (14, 50), (32, 64))


def ragged_sets(d, K):
    """-> V (B, K, d), q (B, K), X (B, d), nv (B,): sets of which query b uses its first nv[b] rows;
    nv covers 0, 1 and K."""
    rng = np.random.default_rng(d)
    nv = np.array([0, 1, K, 2, K - 1, d + 1, 1, 0, K])
    B = len(nv)
    return rng.standard_normal((B, K, d)), rng.standard_normal((B, K)), 1.5 * rng.standard_normal((B, d)), nv


def cap_case():
    """-> V (12, 5), X (2, 5): two exterior queries whose projections lie inside a face of two and
    of three vertices (so no single cycle certifies them), for the cycle cap and the non-finite
    inputs."""
    rng = np.random.default_rng(0)
    V = np.concatenate([2.0 * np.eye(5), 0.2 * rng.standard_normal((7, 5))])
    return V, np.array([[1.5, 1.4, 0.0, 0.1, 0.0], [1.2, 1.3, 1.25, 0.2, 0.0]])


def membership_cases():
    """(V, x, inside): full-dimensional sets, interior points as Dirichlet combinations, exterior
    points a clear margin outside (beyond the farthest vertex from the centroid)."""
    rng = np.random.default_rng(13)
    out = []
    for d, K in ((1, 3), (2, 5), (2, 10), (3, 10), (3, 50), (5, 12), (7, 10)):
        V = rng.standard_normal((K, d))
        c = V.mean(axis=0)
        rad = np.max(np.linalg.norm(V - c, axis=1))
        for _ in range(6):
            out.append((V, rng.dirichlet(np.ones(K)) @ V, True))
            u = rng.standard_normal(d)
            out.append((V, c + (1.05 + rng.random()) * rad * u / np.linalg.norm(u), False))
    return out
