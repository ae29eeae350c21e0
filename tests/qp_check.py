"""Patterns, problems and references for the batched QP's KKT factor paths (csrc/qp.hip,
qp_pattern.h, qp_device.h, qp_block.h), in numpy.

Shared by tests/test_qp_check.py (no GPU: the pattern analysis against a restatement, the C
oracle against a dense high-precision solve) and tests/test_gpu_qp_paths.py (the device
solvers through gpmpc_qp_solve_batched).

Paths.  gpmpc_qp_solve_batched factors the reduced KKT matrix M = P + sigma I + A' R A
  mode 0  as a banded LDL^T (qp_factor) solved in a 64-lane modular window (qp_band_solve):
          windows of 64 rows, groups of 16 steps, a partial top window -- the edges are
          n < 64, 64, 65, 128, 129, 216 and w < 16 against w = 16;
  mode 1  block-tridiagonally in blocks of 10 variables coupled through their first 7
          (blk_factor / blk_solve): a two-way ping-pong chain over the blocks (odd / even
          block counts leave it by different exits), the one-block shortcut, identity pad
          rows in a ragged last block, and, for the 3-DoF MPC at N = 20, an unrolled solve
          and the fleet's two register solvers.
classify() restates the host analysis that chooses between them; table() lists the smallest
patterns that reach each edge, and test_qp_check asserts that they do.

Reference of one KKT solve.  With max_iter = 1, scaling = 0, alpha = 1, warm_start = 0 and
no adaptive rho the first (and only) iterate is x = -M^-1 q, with R = diag(rho_r) by row type
as qp_row_rho states it.  kkt_reference forms M densely in np.longdouble and refines a
float64 solve with longdouble residuals, so its own error is a few longdouble roundings
times cond(M), far below the fp64 solvers' cond(M) 2^-53.

Decision stability.  Status and iteration count are integers decided by comparisons of
residuals with tolerances; a problem whose residual lands within rounding of a tolerance
may legitimately differ between two correct solvers.  decision_stable keeps a problem only
if the C oracle's (status, iter, rho) do not move when every eps, or the adaptive-rho
tolerance, moves by +-5%: 5% is many orders above any rounding difference, so the kept
problems' integers can be demanded exactly.  One decision escapes that test: once an iterate
has converged to rounding (residuals of 1e-12, reached without termination checks), the
adaptive-rho estimate rho sqrt(pri / dua) is a quotient of rounding noise and no tolerance
is near it.  So a kept problem's rho must also stay within 1e-7 when q moves by 1e-12
relative.  1e-12 is the size of what a different rounding path does (the oracle against its own
-ffp-contract=fast build moves x by up to 4e-12); on the table's problems it moves a
well-determined rho by 1e-11 .. 5e-8 and a noise-dominated one by tens of percent, and 1e-7
leaves a factor of ten to the tests' 1e-6.
"""
import ctypes
import functools

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
LD = np.longdouble
# csrc/qp.h, qp_device.h, qp_block.h
NMAX, MMAX, NNZMAX, WMAX, ROWMAX, COLMAX = 216, 360, 896, 16, 8, 12
SZ, CM = 10, 7
BS = SZ * SZ + SZ * CM
FAC_CAP = NMAX * (WMAX + 1) + 64
INFTY, MIN_SCALING, RHO_MIN, RHO_TOL, RHO_EQ = 1e30, 1e-4, 1e-6, 1e-4, 1e3
PER_PATTERN = 4                      # problems per pattern
ONE_ITER = dict(max_iter=1, scaling=0, check_termination=0, adaptive_rho=0, alpha=1.0, warm_start=0)
HAS_SOLUTION = (1, 2, -2)


# ---- the analysis, restated ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _mpc_pattern(N):
    from test_gpu_parity import _qp_batch
    A = _qp_batch(1, N=N)[0][2]
    A.sort_indices()
    return A.shape[1], A.shape[0], tuple(int(v) for v in A.indptr), tuple(int(v) for v in A.indices)


def classify(n, m, rowptr, colidx):
    """What gpmpc_qp_pattern_info must answer for the CSR pattern (its keys, _lib.QP_PATTERN_INFO)."""
    rowptr = [int(v) for v in rowptr]; colidx = [int(v) for v in colidx]
    rows = [colidx[rowptr[r]:rowptr[r + 1]] for r in range(m)]
    nnz = rowptr[m]
    w = max([max(r) - min(r) for r in rows if r] + [0])
    maxrow = max(len(r) for r in rows)
    maxcol = int(np.bincount(np.asarray(colidx[:nnz], int), minlength=n).max()) if nnz else 0
    nblk = -(-n // SZ)
    pairs = [(i, j) for r in rows for i in r for j in r if j <= i]
    blk = all(i // SZ == j // SZ or (i // SZ == j // SZ + 1 and i % SZ < CM) for i, j in pairs)
    if blk and nblk * BS - SZ * CM > FAC_CAP:
        blk = False
    if blk and nblk * SZ > NMAX and w <= WMAX and n * (WMAX + 1) <= FAC_CAP:
        blk = False                  # whole blocks pass the variable cap: the band takes it
    fac_len = nblk * BS - SZ * CM if blk else n * (WMAX + 1)
    n_offd = -1
    if blk and fac_len < 2 ** 15 and nnz < 2 ** 16:
        terms = {}                   # off-diagonal slot -> number of rho_r A_a A_b terms
        for i, j in pairs:
            if i == j:
                continue
            terms[(i, j)] = terms.get((i, j), 0) + 1
            if i // SZ == j // SZ:   # a diagonal block is stored whole, both triangles
                terms[(j, i)] = terms.get((j, i), 0) + 1
        if max(list(terms.values()) + [0]) <= 3:
            n_offd = len(terms) + nblk * SZ - n     # + the identity pads of the last block
    fits = (n <= NMAX and m <= MMAX and nnz <= NNZMAX and maxrow <= ROWMAX and maxcol <= COLMAX
            and (nblk * SZ <= NMAX if blk else (w <= WMAX and fac_len <= FAC_CAP)))
    fleet = (n, m, tuple(rowptr), tuple(colidx[:nnz])) == _mpc_pattern(20)
    return dict(mode=int(blk), w=w, nblk=nblk, fac_len=fac_len, maxrow=maxrow, maxcol=maxcol,
                n_offd=n_offd, fits=int(fits), is_fleet_pattern=int(fleet))


# ---- patterns -------------------------------------------------------------------------------------

def band_pattern(n, w, seed, ncoup=None, row8=False, col12=False, rowlen=None):
    """(n, m, rowptr, colidx): ncoup coupling rows of 2..8 entries spanning exactly w columns,
    their first columns spread evenly over 0..n-w-1 (so the band is full everywhere), then one
    identity bound row per variable.  At most COLMAX entries per column.  row8: the first
    coupling row has 8 entries; col12: eleven coupling rows (and its bound row) share one
    column; rowlen: every coupling row has that many entries.  Seeded, deterministic."""
    rs = np.random.RandomState(seed)
    if w == 0 or n <= w:
        ncoup = 0
    elif ncoup is None:
        ncoup = max(1, (n - w) // 2)
    cnt = np.ones(n, int)            # the bound rows
    c = n // 2
    if col12:                        # rows starting at c-10 .. c all hold column c; no other row ends on it
        assert w >= 10 and ncoup > 11
        rest = [int(round(s)) for s in np.linspace(0, n - w - 1, ncoup - 11)]
        starts = list(range(c - 10, c + 1)) + [s + 1 if s in (c, c - w) else s for s in rest]
    else:
        starts = [int(round(s)) for s in np.linspace(0, n - w - 1, ncoup)] if ncoup else []
    rows = []
    for k, s in enumerate(starts):
        ln = rowlen or int(rs.randint(2, min(ROWMAX, w + 1) + 1))
        if row8 and k == 0:
            ln = 8
        ln = min(ln, w + 1)
        row = {s, s + w}
        if col12 and k < 11:
            row.add(c)
        free = [j for j in range(s + 1, s + w) if j not in row and cnt[j] < COLMAX - (2 if col12 else 0)]
        rs.shuffle(free)
        row |= set(free[:max(0, ln - len(row))])
        assert all(cnt[j] < COLMAX for j in row), (n, w, seed, "column full")
        for j in row:
            cnt[j] += 1
        rows.append(sorted(row))
    rows += [[j] for j in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colidx = np.asarray([j for r in rows for j in r], np.int32)
    return n, len(rows), rowptr, colidx


def _pat(name, cls, p, **expect):
    n, m, rp, ci = p
    return dict(name=name, cls=cls, n=n, m=m, rowptr=np.asarray(rp, np.int32), colidx=np.asarray(ci, np.int32),
                expect=expect)


def _mpc(N):
    n, m, rp, ci = _mpc_pattern(N)
    return _pat(f"mpc_N{N}", "mpc", (n, m, rp, ci), mode=1, nblk=N + 1, fits=1, is_fleet_pattern=int(N == 20))


def _refused():
    out = [_pat("w17", "refused", band_pattern(40, 17, 1), mode=0, w=17, fits=0)]
    n, m, rp, ci = band_pattern(40, 12, 2)
    rows = [list(ci[rp[r]:rp[r + 1]]) for r in range(m)]
    rows[0] = list(range(0, 8)) + [12]                       # nine entries
    out.append(_pat("row9", "refused", _from_rows(n, rows), maxrow=9, fits=0))
    rows = [[20 - k, 20] for k in range(1, 13)] + [[j] for j in range(40)]  # column 20: 12 + its bound row
    out.append(_pat("col13", "refused", _from_rows(40, rows), maxcol=13, fits=0))
    out.append(_pat("m361", "refused", band_pattern(200, 9, 3, ncoup=161, rowlen=2), fits=0))
    out.append(_pat("n217", "refused", band_pattern(217, 9, 4, ncoup=40), fits=0))
    return out


def _from_rows(n, rows):
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return n, len(rows), rowptr, np.asarray([j for r in rows for j in r], np.int32)


@functools.lru_cache(maxsize=None)
def table():
    """The pattern table: name, class, pattern, and what classify / qp_pattern_info must say.
    Mode 0: bands of half-bandwidth 8..16 (narrower ones are block-structured); the last row is
    the narrow band at n = 216, whose 22 whole blocks pass the variable cap.  Mode 1, not MPC:
    bands of w <= 7 (always inside the block structure); many coupling rows put more than three
    terms on a slot (n_offd < 0), few keep the fleet's assembly list (n_offd >= 0)."""
    B = band_pattern
    t = [
        _pat("band_n23_w9", "mode0", B(23, 9, 10), mode=0, w=9, fits=1),
        _pat("band_n63_w12", "mode0", B(63, 12, 11), mode=0, w=12, fits=1),
        _pat("band_n64_w16_col12", "mode0", B(64, 16, 12, col12=True), mode=0, w=16, maxcol=12, fits=1),
        _pat("band_n65_w8", "mode0", B(65, 8, 13, row8=True), mode=0, w=8, maxrow=8, fits=1),
        _pat("band_n127_w15", "mode0", B(127, 15, 14), mode=0, w=15, fits=1),
        _pat("band_n128_w16", "mode0", B(128, 16, 15, row8=True), mode=0, w=16, maxrow=8, fits=1),
        _pat("band_n129_w11", "mode0", B(129, 11, 16), mode=0, w=11, fits=1),
        _pat("band_n192_w13", "mode0", B(192, 13, 17), mode=0, w=13, fits=1),
        _pat("band_n216_w16", "mode0", B(216, 16, 18), mode=0, w=16, fits=1),
        _pat("band_n216_w3", "mode0", B(216, 3, 19), mode=0, w=3, nblk=22, fits=1),
        _pat("blk_n1", "mode1", B(1, 0, 20), mode=1, nblk=1, fits=1),
        _pat("blk_n7_w3", "mode1", B(7, 3, 21), mode=1, nblk=1, fits=1),
        _pat("blk_n10_w7", "mode1", B(10, 7, 22), mode=1, nblk=1, fits=1),
        _pat("blk_n11_w4", "mode1", B(11, 4, 23), mode=1, nblk=2, fits=1),
        _pat("blk_n40_w6", "mode1", B(40, 6, 24), mode=1, nblk=4, fits=1),
        _pat("blk_n65_w5_dense", "mode1", B(65, 5, 25, ncoup=90, rowlen=5), mode=1, nblk=7, n_offd=-1, fits=1),
        _pat("blk_n129_w4_sparse", "mode1", B(129, 4, 26, ncoup=40), mode=1, nblk=13, fits=1),
    ]
    t += [_mpc(N) for N in (1, 2, 3, 4, 8, 19, 20)]
    t += _refused()
    return tuple(t)


def fitting():
    return [p for p in table() if p["cls"] != "refused"]


def by_name(name):
    return next(p for p in table() if p["name"] == name)


# ---- problems -------------------------------------------------------------------------------------

def _csr(pat, data):
    return sp.csr_matrix((np.asarray(data, float), pat["colidx"].copy(), pat["rowptr"].copy()),
                         shape=(pat["m"], pat["n"]))


def band_problem(pat, seed):
    """(Pdiag, q, A, l, u, x_ws) on a band_pattern: diagonal P >= 0 with about a fifth zero;
    coupling rows equalities / ranges / one-sided around a feasible point; boxes on the
    variables, about 15% of them free (and then P > 0: the problem stays bounded)."""
    rs = np.random.RandomState(seed)
    n, m = pat["n"], pat["m"]
    nc = m - n
    data = np.where(rs.rand(pat["colidx"].size) < 0.5, -1.0, 1.0) * rs.uniform(0.5, 1.5, pat["colidx"].size)
    data[pat["rowptr"][nc]:] = 1.0
    A = _csr(pat, data)
    P = rs.uniform(0.5, 2.0, n) * (rs.rand(n) >= 0.2)
    x0 = rs.randn(n)
    ax = A @ x0
    l = np.empty(m); u = np.empty(m)
    kind = rs.randint(0, 4, nc)      # 0 equality, 1 range, 2 upper only, 3 lower only
    lo = ax[:nc] - rs.uniform(0.05, 1.0, nc); hi = ax[:nc] + rs.uniform(0.05, 1.0, nc)
    l[:nc] = np.where(kind == 0, ax[:nc], np.where(kind == 2, -np.inf, lo))
    u[:nc] = np.where(kind == 0, ax[:nc], np.where(kind == 3, np.inf, hi))
    free = rs.rand(n) < 0.15
    P[free] = np.maximum(P[free], 0.5)
    l[nc:] = np.where(free, -np.inf, x0 - rs.uniform(0.05, 1.0, n))
    u[nc:] = np.where(free, np.inf, x0 + rs.uniform(0.05, 1.0, n))
    q = rs.randn(n)
    return P, q, A, l, u, x0 + 0.1 * rs.randn(n)


@functools.lru_cache(maxsize=None)
def problems(name):
    """The PER_PATTERN problems of a fitting table pattern (read-only)."""
    pat = by_name(name)
    if pat["cls"] == "mpc":
        from test_gpu_parity import _qp_batch
        probs = _qp_batch(PER_PATTERN, N=pat["n"] // SZ)
        for p in probs:
            p[2].sort_indices()
            assert np.array_equal(p[2].indptr, pat["rowptr"]) and np.array_equal(p[2].indices, pat["colidx"])
    else:
        base = sum(ord(c) for c in name)
        probs = [band_problem(pat, 1000 * base + b) for b in range(PER_PATTERN)]
    out = []
    for P, q, A, l, u, xw in probs:
        A = sp.csr_matrix(A)
        for v in (P, q, A.data, l, u, xw):
            v.setflags(write=False)
        out.append((P, q, A, l, u, xw))
    return tuple(out)


def primal_infeasible(pat, prob):
    """An equality coupling row moved off the (tightened) boxes of its variables."""
    P, q, A, l, u, xw = prob
    l, u = l.copy(), u.copy()
    nc = pat["m"] - pat["n"]
    r = next(r for r in range(nc) if l[r] == u[r])
    cols = A.indices[A.indptr[r]:A.indptr[r + 1]]; vals = A.data[A.indptr[r]:A.indptr[r + 1]]
    fin = np.isfinite(l[nc:]) & np.isfinite(u[nc:])
    x0 = 0.5 * (np.where(fin, l[nc:], 0.0) + np.where(fin, u[nc:], 0.0))
    l[nc + cols] = x0[cols] - 0.1; u[nc + cols] = x0[cols] + 0.1
    l[r] = u[r] = vals @ x0[cols] + 10.0 * np.abs(vals).sum()
    return P, q, A, l, u, xw


def dual_infeasible(pat, prob, seed=0):
    """P = 0, every bound row +-1e30, q random: unbounded along the coupling rows' null space."""
    P, q, A, l, u, xw = prob
    l, u = l.copy(), u.copy()
    nc = pat["m"] - pat["n"]
    l[nc:], u[nc:] = -1e30, 1e30
    return np.zeros_like(P), np.random.RandomState(seed).randn(q.size), A, l, u, xw


def factor_fails(prob, first=True, y0=None):
    """The oracle's KKT factorisation fails.  first: the first one (one iteration, no adaptive
    rho); otherwise any one before the last iteration of a default solve (max_iter 49: the
    refactorisation after the rho adaptation at iteration 25).  The last iteration is left out
    because there the two differ: the oracle refactors after an adaptation at max_iter too,
    the device skips that factorisation because nothing would use it."""
    try:
        oracle_run(prob, y0=y0, **(dict(max_iter=1, adaptive_rho=0) if first else dict(max_iter=49)))
    except RuntimeError:
        return True
    return False


def not_convex(pat, prob, j=None, value=-1e3, first=True, y0=None):
    """Pdiag[j] = -1e3: negative curvature that A' R A does not cover, so the KKT factor fails.
    j: the first variable from the middle on for which the oracle's factor fails (factor_fails)
    at -1e3 and also at half and at twice that, so that no rounding decides it.  A failure
    after an adaptation (first = False) depends on where rho went, not monotonically on the
    value: there the margin is 10% either way, still 1e11 roundings."""
    P, q, A, l, u, xw = prob
    if j is None:
        values = (-1e3, -5e2, -2e3) if first else (-1e3, -9e2, -1.1e3)
        j = next(j for j in range(pat["n"] // 2, pat["n"])
                 if all(factor_fails(not_convex(pat, prob, j, v), first, y0) for v in values))
    P = P.copy()
    P[j] = value
    return P, q, A, l, u, xw


# ---- references -----------------------------------------------------------------------------------

def row_rho(l, u, rho):
    """qp_rules.h qp_row_rho on the clamped bounds."""
    l = np.maximum(l, -INFTY); u = np.minimum(u, INFTY)
    loose = (l < -INFTY * MIN_SCALING) & (u > INFTY * MIN_SCALING)
    return np.where(loose, RHO_MIN, np.where(u - l < RHO_TOL, RHO_EQ * rho, rho))


def kkt_reference(P, A, l, u, q, rho, sigma):
    """(-M^-1 q, cond_inf(M)) for M = P + sigma I + A' diag(rho_r) A, formed densely in
    longdouble; numpy.linalg.solve refined five times with longdouble residuals."""
    Ad = np.asarray(sp.csr_matrix(A).todense()).astype(LD)
    n = Ad.shape[1]
    M = np.diag(np.asarray(P, LD) + LD(sigma)) + Ad.T @ (row_rho(l, u, rho).astype(LD)[:, None] * Ad)
    b = -np.asarray(q, LD)
    M64 = M.astype(np.float64)
    x = np.linalg.solve(M64, b.astype(np.float64)).astype(LD)
    for _ in range(5):
        x = x + np.linalg.solve(M64, (b - M @ x).astype(np.float64)).astype(LD)
    cond = float(np.abs(M64).sum(1).max() * np.abs(np.linalg.inv(M64)).sum(1).max())
    return x.astype(np.float64), cond


def oracle_settings(**kw):
    from oracle import admm_ref
    return admm_ref.default_settings(**kw)


def oracle_run(prob, solves=1, x_ws="given", y0=None, **kw):
    """The C oracle on one problem: `solves` consecutive solves that carry rho, the scaled y and
    x (the last solution as the next warm start); prob may be a list, one problem per solve
    (the same rows: the dual carries over).  x_ws: "given" (the problem's) or None (the
    oracle's zeros).  y0: the scaled dual passed in.  Returns one result dict per solve, each
    with "y_scaled" added; raises RuntimeError when the KKT factor fails."""
    from oracle import admm_ref
    seq = list(prob) if isinstance(prob, list) else [prob] * solves
    ref = admm_ref.RefQP(seq[0][2].shape[0], admm_ref.default_settings(**kw))
    if y0 is not None:
        ref.y[:] = y0
    xw = np.zeros_like(seq[0][1]) if x_ws is None else seq[0][5]
    out = []
    for P, q, A, l, u, _ in seq:
        r = ref.solve(P, q, A, l, u, xw)
        r["y_scaled"] = ref.y.copy()
        out.append(r)
        xw = r["x"] if r["status"] in HAS_SOLUTION else xw
    return out


def decisions(prob, solves=1, **kw):
    return tuple((r["status"], r["iter"], float(f"{r['rho']:.5e}")) for r in oracle_run(prob, solves, **kw))


def decision_stable(prob, solves=1, **kw):
    """True when the oracle's (status, iter, rho to 6 digits) of every solve are the same as
    given, with the four eps scaled by 0.95 and 1.05, and with adaptive_rho_tolerance scaled
    by 0.95 and 1.05; and when a 1e-12 relative change of q moves rho by less than 1e-7."""
    s = oracle_settings(**{k: v for k, v in kw.items() if k not in ("x_ws", "y0")})
    eps = ("eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf")
    runs = [dict(kw)]
    for f in (0.95, 1.05):
        runs.append(dict(kw, **{k: f * getattr(s, k) for k in eps}))
        runs.append(dict(kw, adaptive_rho_tolerance=f * s.adaptive_rho_tolerance))
    first = decisions(prob, solves, **runs[0])
    if not all(decisions(prob, solves, **r) == first for r in runs[1:]):
        return False
    # ... and none of it is rounding noise: q moved by 1e-12 relative leaves status and
    # iterations alone and rho within 1e-7 (see the module docstring)
    base = oracle_run(prob, solves, **kw)
    seq = list(prob) if isinstance(prob, list) else [prob]
    for f in (1.0 - 1e-12, 1.0 + 1e-12):
        moved = [(P, q * f, A, l, u, xw) for P, q, A, l, u, xw in seq]
        for r, r0 in zip(oracle_run(moved if isinstance(prob, list) else moved[0], solves, **kw), base):
            if (r["status"], r["iter"]) != (r0["status"], r0["iter"]) or abs(r["rho"] - r0["rho"]) > 1e-7 * r0["rho"]:
                return False
    return True


@functools.lru_cache(maxsize=None)
def stable_problems(name, solves=1, settings=()):
    """Indices of the pattern's problems that are decision-stable under settings (a tuple of items)."""
    return tuple(b for b, p in enumerate(problems(name)) if decision_stable(p, solves, **dict(settings)))


# ---- the device call ------------------------------------------------------------------------------

def device_solve(L, ctx, pat, probs, settings=None, x_ws="given", rho=None, y_scaled=None, nnz=None, fill=None):
    """One raw gpmpc_qp_solve_batched call on len(probs) problems of one pattern.  Returns
    (rc, outputs); rho / y_scaled in the outputs are the carried state after the call.  fill:
    a value every output starts from (the refusal tests' sentinel)."""
    B, n, m = len(probs), pat["n"], pat["m"]
    rp = np.ascontiguousarray(pat["rowptr"], np.int32); ci = np.ascontiguousarray(pat["colidx"], np.int32)
    k = int(rp[-1])
    st = L.qp_default_settings(**(settings or {}))
    Av = np.stack([np.asarray(p[2].data, float)[:k] for p in probs]); Pd = np.stack([p[0] for p in probs])
    qv = np.stack([p[1] for p in probs]); lv = np.stack([p[3] for p in probs]); uv = np.stack([p[4] for p in probs])
    xw = None if x_ws is None else np.ascontiguousarray(np.stack([p[5] for p in probs]) if isinstance(x_ws, str) else x_ws)
    rho = np.full(B, float(st.rho)) if rho is None else np.array(rho, float)
    ysc = np.zeros((B, m)) if y_scaled is None else np.array(y_scaled, float)
    f = np.nan if fill is None else fill
    x = np.full((B, n), f); y = np.full((B, m), f); obj = np.full(B, f)
    it = np.full(B, 0 if fill is None else int(fill), np.int32); stt = it.copy()
    rc = L._L.gpmpc_qp_solve_batched(ctx.h, B, n, m, k if nnz is None else nnz, L._i(rp), L._i(ci), L._d(Av),
                                     L._d(Pd), L._d(qv), L._d(lv), L._d(uv), ctypes.byref(st),
                                     None if xw is None else L._d(xw), L._d(rho), L._d(ysc), L._d(x), L._d(y),
                                     L._i(it), L._i(stt), L._d(obj))
    return rc, dict(x=x, y=y, iter=it, status=stt, obj=obj, rho=rho, y_scaled=ysc)
