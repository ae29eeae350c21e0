"""Cases, references and the pass/fail rules for the batched Cholesky (csrc/chol.hip), the
triangular solves and the solve helpers of csrc/gp.hip, in numpy.

Shared by tests/test_chol_check.py (no GPU: the rules accept float64 restatements of every
algorithm form and reject subtly wrong ones) and tests/test_gpu_chol.py (runs the kernels
through gpmpc_potrf_diag and gpmpc_tri_diag).  The poison pattern, the flat buffers with
guard bands and ld gaps (Buf) and the "everything else keeps its bits" check come from
gemm_check.

Notation: u = 2^-53; |.| elementwise; first order in u throughout (the u^2 terms are below
1e-10 of the bounds at these sizes).  A dot product of K terms accumulated by fma in any
order, in any number of passes over a stored value, has |error| <= (K + P) u S where P is
the number of extra roundings (one per pass that re-reads the stored partial sum, one per
atomic partial add) and S the sum of the absolute values of its terms (gemm_check uses the
same count for one product).

The factor rule.  There is no exact family for the factor: the diagonal kernels take
1 / sqrt by v_rsq_f64 and two Newton steps, a few ulp, so equality would test the hardware's
rsq.  The check is the elementwise backward error on the lower triangle,

    |A - L^ L^^T|_ij <= c1 u (|L^| |L^^T|)_ij + c2(b) u (|L^_i,blk| |L_bb^T| |L_bb^-T| |L_bb^T|)_j

* c1: entry (i, j) of the factor is s = a_ij - sum_{k<j} l_ik l_jk, then l_jj = sqrt(s) or
  l_ij = s / l_jj.  The sum has j <= n fma terms and is carried through at most
  P = ceil(n / 32) + 4 passes (one per 32-column step of the two-level driver, or one per
  outer panel plus one per block column, plus the four 32-column steps inside the diagonal
  kernel) and at most 16 atomic partial adds (K splits), so
  |s^ - s| <= (n + P + 16) u (|a_ij| + sum |l_ik| |l_jk|) <= 2 (n + P + 16) u (|L^| |L^^T|)_ij,
  the last step because |a_ij| <= (|L| |L^T|)_ij.  The square root (rsq + two Newton steps and
  a multiplication) and the division (a multiplication by the rounded reciprocal) add at most
  8 u |l_ij| |l_jj| <= 8 u (|L^| |L^^T|)_ij.  c1(n) = 2 (n + ceil(n / 32) + 20) + 8.
* c2: where the rows below a diagonal block L_bb (b x b) are solved by a product with its
  explicit inverse, X^ = fl(Y T^^T) with T^ = fl(L_bb^-1): |X^ - Y T^^T| <= g |Y| |T^^T| for the
  product and |L_bb T^ - I| <= g' |L_bb| |T^| for the inverse formed column by column (its
  right residual), so X^ L_bb^T - Y = Y (L_bb T^ - I)^T + (X^ - Y T^^T) L_bb^T is bounded by
  (g + g') |Y| |L_bb^-T| |L_bb^T| and |Y| <= |X^| |L_bb^T|.  g = (b + 8) u (a K = b product),
  g' <= (2 b + 16) u (a column of the 32 x 32 inverse is a b-term substitution; the 128 x 128
  inverse is assembled from the 32 x 32 ones by X_ij = -T_i sum_k L_ik X_kj, a b-term sum
  inside a 32-term product), both rounded up to (2 b + 16) u: c2(b) = 4 b + 32.
  Which block a path inverts ("kind", read from the plan that ran):
    inv128  the column-sweep diagonal kernel, rows below the 128-column block by the
            128 x 128 inverse (none inside the diagonal block: the sweep substitutes)
    trsm32  the same with the TRSM-form panel solve: the 32 x 32 inverses
    core    diag128_core (GPMPC_DIAG_SWEEP=0, the persistent form): 32 x 32 inverses inside
            the 128-column block, the 128 x 128 inverse below it
    col32   the 32-column driver: the 32 x 32 inverse for every row below the block
* worst ratio |A - L L^T| / bound seen when this file was written (tests/test_chol_check.py,
  every family, n in 1..420): LAPACK 0.035, the float64 restatements of the four kinds 0.036
  (both at n <= 33, where c1's constant part counts most; below 0.02 at n = 420) -- the
  constants are worst-case counts, the errors behave like their square roots.  Against
  u |L| |L^T| alone (no second term) at n = 420: wishart / graded LAPACK 3.4 / 4.1, 128-inverse
  restatement 3.6 / 3.7; gp6 / gp8 LAPACK 22 / 20, 128-inverse restatement 343 / 342 -- the
  explicit inverse costs a factor of ~15 there, which only the second term admits.
  Triangular rules, same test: blocked TRSM 0.013, LAPACK's 0.016, doubling inverse 0.017,
  two substitutions 0.019, inverse solve with refinement 0.030.

The triangular rule is the residual form of the same two terms: with op(L) = L or L^T and
the 32 x 32 diagonal blocks L_ii whose inverses the panel walk multiplies by,

    |op(L) X^ - B|_i <= c1(n) u (|op(L)| |X^|)_i + c2(32) u (|op(L_ii)| |op(L_ii)^-1| |op(L_ii)| |X^_i|)

(same derivation: acc = B_i - sum L_ik X_k is the dot product, X_i = T_i acc the product with
the explicit inverse).  The doubling inverse W = L^-1 is checked as |L W^ - I| <= E with E
built level by level as the launcher builds W: the 128 x 128 diagonal blocks by the rule
above (B = I), then for a pair A (b rows), C (the next mc rows), W_CA = -W_CC (L_CA W_AA):
with P = |L_CA| |W^_AA| and g = (2 b + 8) u (gemm_check's bound of a K = b product)
    E_CA = g P + E_CC P + g |L_CC| (|W^_CC| P)
(tmp^ = L_CA W_AA + d1, |d1| <= g P; W^_CA = -W_CC tmp^ + d2, |d2| <= g |W_CC| |tmp^|;
L_CC W^_CA = -(I + (L_CC W^_CC - I)) tmp^ + L_CC d2).  The strict upper triangle of W^ must be
exactly zero.  The two solve helpers are held to one bound,
    |L L^T a^ - y| <= cs(n) u |L| |L^T| |a^|,   cs(n) = 2 (n + ceil(n / 32) + 8) + 8:
each substitution solves (L + dL) z = y with |dL| <= (n + ceil(n / 32) + 8) u |L| (n fma terms,
one pass per 32-row block, the division), and gp.hip claims that one refinement step makes
the explicit-inverse solve "as accurate as the two substitutions".

The exact family: L = (I + N) D with N integers in -3..3 only at (i not in S, j in S, j < i)
for a random half S, so N^2 = 0 and L^-1 = D^-1 (I - N); D powers of two in 1/2..4, B
integers in -3..3.  Every partial sum of every order, the 32 x 32 inverses, the doubling
products and the refinement residual (exactly zero) are multiples of 2^-6 far below 2^47, so
fp64 arithmetic is exact and the result must EQUAL D^-1 (I - N) B (tolerance zero).
"""
import functools

import numpy as np
import scipy.linalg as sla

import gemm_check as gc
from gemm_check import LD, POISON, U, Buf, T, bits, ld_for, poison  # noqa: F401  (re-exported)

NB, DB = 32, 128
KINDS = ("inv128", "trsm32", "core", "col32")
FAMILIES = ("wishart", "graded", "gp6", "gp8")


def c1(n):
    return 2 * (n + (n + 31) // 32 + 20) + 8


def c2(b):
    return 4 * b + 32


def cs(n):
    return 2 * (n + (n + 31) // 32 + 8) + 8


def tri_inv(Lb):
    """The inverse of a lower-triangular block, every column by forward substitution (so its
    right residual L T - I is small), all columns at once."""
    b = len(Lb)
    X = np.zeros((b, b))
    for r in range(b):
        X[r] = -(Lb[r, :r] @ X[:r])
        X[r, r] += 1.0
        X[r] /= Lb[r, r]
    return X


def cond_block(Lb, trans=False):
    """|op(L_bb)| |op(L_bb)^-1| |op(L_bb)|, the factor of the explicit-inverse term."""
    a, ai = np.abs(Lb), np.abs(tri_inv(Lb))
    if trans:
        a, ai = a.T, ai.T
    return a @ ai @ a


# ---- the factor rule ---------------------------------------------------------------------
def inverse_blocks(n, kind):
    """(c0, c1, r0, r1): rows r0..r1 of columns c0..c1 were solved with the explicit inverse
    of the diagonal block at c0..c1."""
    assert kind in KINDS
    out = []
    if kind in ("inv128", "core"):
        out += [(c, c + DB, c + DB, n) for c in range(0, n - DB, DB)]
    if kind == "trsm32":
        out += [(c, c + NB, (c // DB + 1) * DB, n) for c in range(0, (n - 1) // DB * DB, NB)]
    if kind == "core":
        out += [(c, c + NB, c + NB, min(n, (c // DB + 1) * DB)) for c in range(0, n - NB, NB)
                if c + NB < min(n, (c // DB + 1) * DB)]
    if kind == "col32":
        out += [(c, c + NB, c + NB, n) for c in range(0, n - NB, NB)]
    return out


def factor_bound(Lh, kind, c1_scale=1.0):
    """The right-hand side of the factor rule for a computed factor Lh (float64, lower)."""
    n = len(Lh)
    aL = np.abs(np.tril(Lh))
    bound = c1_scale * c1(n) * U * (aL @ aL.T)
    for c0, c1_, r0, r1 in inverse_blocks(n, kind):
        M = cond_block(Lh[c0:c1_, c0:c1_]).T     # |L_bb^T| |L_bb^-T| |L_bb^T|
        bound[r0:r1, c0:c1_] += c2(c1_ - c0) * U * (aL[r0:r1, c0:c1_] @ M)
    return bound


def factor_ratios(A, Lh, kind, longdouble=True):
    """(max over the lower triangle of |A - Lh Lh^T| / bound, the same against u |Lh| |Lh^T|
    alone -- the figure a backward-stable factor keeps near n-independent tens); nan when Lh has
    a nan.  The residual in longdouble, or in float64 with c1 doubled for the evaluation's own
    rounding."""
    n = len(Lh)
    L = np.tril(Lh)
    if not np.all(np.isfinite(L)):
        return float("nan"), float("nan")
    low = np.tril(np.ones((n, n), bool))
    with np.errstate(all="ignore"):
        if longdouble:
            Ll = L.astype(LD)
            res = np.abs(np.tril(A).astype(LD) - np.matmul(Ll, Ll.T)).astype(np.float64)
            bound = factor_bound(L, kind)
        else:
            res = np.abs(np.tril(A) - L @ L.T)
            bound = factor_bound(L, kind, 2.0)
        tiny = np.finfo(np.float64).tiny
        r = res[low] / np.maximum(bound[low], tiny)
        plain = res[low] / np.maximum(U * (np.abs(L) @ np.abs(L).T)[low], tiny)
    if not np.all(np.isfinite(r)):
        return float("nan"), float("nan")
    return float(np.max(r)), float(np.max(plain))


def factor_ratio(A, Lh, kind, longdouble=True):
    return factor_ratios(A, Lh, kind, longdouble)[0]


def check_factor(A, Lh, kind, longdouble=True, tag=""):
    """Violations of the factor rule (empty: pass): positive diagonal, residual inside the bound."""
    bad = []
    d = np.diagonal(Lh)
    if not np.all(d > 0):       # nan fails
        bad.append(f"{tag}: diag(L) not positive at {int(np.argmin(d > 0))}")
    r = factor_ratio(A, Lh, kind, longdouble)
    if not r <= 1.0:            # nan fails
        bad.append(f"{tag}: |A - L L^T| / bound = {r:.3g} ({'longdouble' if longdouble else 'float64'}, {kind})")
    return bad


# ---- factor families ---------------------------------------------------------------------
def _family(rng, family, n):
    if family in ("wishart", "graded"):
        G = rng.standard_normal((n, n))
        A = G @ G.T / n + np.eye(n)
        if family == "graded":
            d = 10.0 ** rng.uniform(-3, 3, n)
            A = A * d[:, None] * d[None, :]
        return A
    noise = {"gp6": 1e-6, "gp8": 1e-8}[family]
    X = rng.uniform(-1, 1, (n, 3))
    d2 = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=2)
    K = np.exp(-0.5 * d2 / 0.25)
    return (K + K.T) / 2 + noise * np.eye(n)


@functools.lru_cache(maxsize=None)
def factor_mats(family, n, batch, seed=0):
    """batch symmetric positive definite matrices of a family (read-only).  The builder
    asserts, on the first one, that LAPACK's factor and the float64 restatements of the
    block-inverse algorithm pass the rule with a factor 2 to spare."""
    rng = np.random.default_rng([FAMILIES.index(family), n, batch, seed])
    A = np.stack([_family(rng, family, n) for _ in range(batch)])
    for kind in KINDS:
        r = factor_ratio(A[0], restate_potrf(A[0], kind), kind, longdouble=False)
        assert r <= 0.5, (family, n, kind, r)
    assert factor_ratio(A[0], np.linalg.cholesky(A[0]), "inv128", longdouble=False) <= 0.5
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def family_L(family, n, seed=0):
    """A lower-triangular L of a factor family (LAPACK's factor of its first matrix)."""
    L = np.linalg.cholesky(factor_mats(family, n, 1, seed + 1)[0])
    L.setflags(write=False)
    return L


# ---- float64 restatements of the factor's forms --------------------------------------------
def _chol(S):
    """LAPACK's factor of a block given by its lower triangle; all nan where it has none (a
    mutant's block may be indefinite or hold a nan)."""
    try:
        return np.linalg.cholesky(np.tril(S) + np.tril(S, -1).T)
    except np.linalg.LinAlgError:
        return np.full(S.shape, np.nan)


def _chol_core(S):
    """diag128_core: four 32-column steps, the rows below a step by its explicit inverse."""
    S = S.copy()
    w = len(S)
    for j in range(0, w, NB):
        j1 = min(w, j + NB)
        S[j:j1, j:j1] = _chol(S[j:j1, j:j1])
        if j1 < w:
            S[j1:, j:j1] = S[j1:, j:j1] @ tri_inv(S[j:j1, j:j1]).T
            S[j1:, j1:] -= np.tril(S[j1:, j:j1] @ S[j1:, j:j1].T)
    return np.tril(S)


def restate_potrf(A, kind, left=False, mut=None, diag_from=None):
    """The blocked factor in float64 as the device forms it: column blocks of 128 (32 for
    col32), right-looking (one trailing update per block) or left-looking (each block
    column updated by all earlier columns), the rows below a diagonal block by its explicit
    inverse(s).  Reads the lower triangle of A only; returns a copy of A with the lower
    triangle replaced.  mut: None or (name, ...) -- a mutant, see MUTANTS; diag_from: another
    matrix's factor whose first diagonal block this one takes (the batch mutant).
    The dict restate_potrf.met counts the places where a mutant applied."""
    n = len(A)
    bs = NB if kind == "col32" else DB
    M = np.tril(A).astype(np.float64)
    name = mut[0] if mut else None
    if name == "poison":                      # an element outside the matrix read in its place
        M[n - 1, 0] = np.nan
        _met(name)
    Tprev = None
    for bi, c in enumerate(range(0, n, bs)):
        c1_ = min(n, c + bs)
        w = c1_ - c
        if left and c > 0:
            Lr, Lc = M[c:, :c], M[c:c1_, :c].copy()
            if name == "kslice" and bi == 1:  # one 16-wide K slice of the first row tile
                upd = Lr @ Lc.T
                upd[:bs] -= Lr[:bs, 16:32] @ Lc[:, 16:32].T
                _met(name)
            else:
                upd = Lr @ Lc.T
            M[c:, c:c1_] -= upd
            M[c:c1_, c:c1_] = np.tril(M[c:c1_, c:c1_])
        if name == "skiplast" and w < bs and c > 0:
            _met(name)                        # the ragged last block left unfactored
            break
        S = M[c:c1_, c:c1_]
        Lbb = _chol_core(S) if kind == "core" else _chol(S)
        if diag_from is not None and c == 0:
            Lbb = np.tril(diag_from[:w, :w])
            _met("batchdiag")
        M[c:c1_, c:c1_] = Lbb
        if c1_ < n:
            Y = M[c1_:, c:c1_]
            if kind == "trsm32":
                Ts = [tri_inv(Lbb[j:j + NB, j:j + NB]) for j in range(0, bs, NB)]
                use = Ts
                if name == "previnv" and Tprev is not None and bi == 1:
                    use = Tprev
                    _met(name)
                X = np.empty_like(Y)
                for q, j in enumerate(range(0, bs, NB)):
                    acc = Y[:, j:j + NB] - X[:, :j] @ Lbb[j:j + NB, :j].T
                    X[:, j:j + NB] = acc @ use[q].T
                Tprev = Ts
            else:
                Tb = tri_inv(Lbb)
                X = Y @ Tb.T
                if name == "previnv" and Tprev is not None and bi == 1:
                    X[:bs] = Y[:bs] @ Tprev.T   # one row block with the previous block's inverse
                    _met(name)
                Tprev = Tb
            M[c1_:, c:c1_] = X
            if not left:
                Xu = X
                upd = X @ X.T
                if name == "kslice" and bi == 0:
                    upd[:bs, :bs] -= Xu[:bs, 16:32] @ Xu[:bs, 16:32].T
                    _met(name)
                M[c1_:, c1_:] -= np.tril(upd)
    out = np.array(A, np.float64, copy=True)
    low = np.tril(np.ones((n, n), bool))
    out[low] = M[low]
    if name == "nudge":                       # one element of the factor moved by 1e-9 relative
        i = (n - 1 - mut[1]) % n
        j = i // 2
        out[i, j] *= 1.0 + 1e-9
        if out[i, j] != 0.0:
            _met(name)
    return out


def _met(name):
    restate_potrf.met[name] = restate_potrf.met.get(name, 0) + 1


restate_potrf.met = {}
MUTANTS = ("kslice", "previnv", "skiplast", "batchdiag", "nudge", "gapwrite", "poison")


# ---- the factor's cases on flat buffers ----------------------------------------------------
LAYOUTS = ("packed", "even", "odd", "shift")


def layout(cols, rows, variant, batch):
    """(ld, stride, shift): ld packed / next even / next odd above cols; the batch stride
    always leaves a gap behind the last row (and is odd for 'odd', so alternate members
    change their 16-byte alignment); 'shift': even ld, the base one double past a 16-byte
    boundary."""
    ld = ld_for(cols, "even" if variant == "shift" else variant)
    stride = rows * ld + (3 if variant == "odd" else 6)
    return ld, stride, 1 if variant == "shift" else 0


def bad_matrix(A, col, value):
    """A with a bad pivot at 1-based column col: row and column zeroed, the diagonal value
    (-1 or nan), so the first col - 1 columns factor cleanly and column col fails."""
    A = np.array(A, copy=True)
    k = col - 1
    A[k, :] = 0.0
    A[:, k] = 0.0
    A[k, k] = value
    return A


class FactorCase:
    """batch matrices of order n in a poisoned flat buffer: the lower triangles hold the
    matrices, the strict upper triangles, ld gaps, stride gaps and bands the poison.
    bad: {member: 1-based column} of the members with a bad pivot."""

    def __init__(self, A, variant="even", bad=None, tag=""):
        A = np.asarray(A, np.float64)
        self.batch, self.n, _ = A.shape
        self.A, self.bad, self.tag, self.variant = A, dict(bad or {}), tag, variant
        self.low = np.broadcast_to(np.tril(np.ones((self.n, self.n), bool)), A.shape).copy()
        ld, stride, shift = layout(self.n, self.n, variant, self.batch)
        self.buf = Buf(np.where(self.low, A, poison(A.shape)), ld, stride, shift)

    def want_info(self):
        return [self.bad.get(b, 0) for b in range(self.batch)]

    def verify(self, after, info, kind, report=None, longdouble=True):
        """after: the flat array after the factorisation; info: its info array.  Violations.
        The residual of the first and last good member is evaluated in longdouble (unless
        longdouble is False), of the others in float64."""
        bad = [f"{self.tag}: {m}" for m in gc.check_untouched(self.buf, after, self.low, "factor")]
        info = [int(v) for v in np.asarray(info)[:self.batch]]
        if info != self.want_info():
            bad.append(f"{self.tag}: info {info}, expected {self.want_info()}")
        got = self.buf.get(after)
        good = [b for b in range(self.batch) if b not in self.bad]
        for b in good:
            ld_ = longdouble and gc.longdouble_ok() and b in (good[0], good[-1])
            bad += check_factor(self.A[b], got[b], kind, ld_, f"{self.tag} member {b}")
            if report is not None and ld_:
                report.append((self.tag, kind) + factor_ratios(self.A[b], got[b], kind, True))
        return bad

    def perfect_after(self, kind, left=False, mut=None):
        """The flat image a float64 restatement of the form leaves (good members only)."""
        mats = self.buf.mats.copy()
        prev = None
        for b in range(self.batch):
            if b in self.bad:
                continue
            m = mut
            df = None
            if mut and mut[0] == "batchdiag":
                m, df = None, (prev if b == self.batch - 1 else None)
            elif mut and b != mut[1] % self.batch:
                m = None
            Lb = restate_potrf(self.A[b], kind, left, m, df)
            prev = Lb
            mats[b][self.low[b]] = Lb[self.low[b]]
        after = self.buf.with_values(mats, self.low)
        if mut and mut[0] == "gapwrite":
            g = gap_index(self.buf)
            if g is not None:
                after[g] = 0.0
                _met("gapwrite")
        return after


def gap_index(buf):
    """The flat index of an element of an ld gap (or, packed, of the stride gap); None when
    the layout has neither."""
    if buf.ld > buf.cols:
        return buf.offset + (buf.rows // 2) * buf.ld + buf.cols
    if buf.batch > 1 and buf.stride > buf.rows * buf.ld:
        return buf.offset + buf.rows * buf.ld
    return None


# the factor runs of tests/test_gpu_chol.py: (switches, [(n, batch), ...]).  Every n of the
# issue's list at every batch under the default policy, every switch at the sizes where its
# path differs.  test_factor_coverage reads the plans back and asserts what they contain.
SIZES = (1, 31, 33, 127, 128, 129, 255, 257, 300, 420)
FACTOR_RUNS = [
    ("default_b1", {}, [(n, 1) for n in SIZES]),
    ("default_b3", {}, [(n, 3) for n in SIZES]),
    ("default_b8", {}, [(n, 8) for n in SIZES]),
    ("default_b17", {}, [(n, 17) for n in SIZES]),
    ("default_b72", {}, [(300, 72)]),
    ("inv_lat", {"trsm": 0, "lat": 1}, [(n, 3) for n in SIZES]),
    ("inv_tiled", {"trsm": 0, "lat": 0}, [(n, 8) for n in SIZES]),
    ("trsm_lat", {"trsm": 1, "lat": 1}, [(257, 17), (420, 17)]),
    ("trsm_tiled", {"trsm": 1, "lat": 0}, [(257, 3), (420, 3)]),
    ("sweep0", {"sweep": 0}, [(n, 3) for n in SIZES] + [(300, 17), (420, 17)]),
    ("packed_trsm", {"pk": 1}, [(n, 3) for n in SIZES]),
    ("packed_inv", {"pk": 1, "trsm": 0}, [(129, 17), (300, 17), (420, 17)]),
    ("ob256", {"ob": 256}, [(300, 3), (420, 3), (420, 17)]),
    ("ob1024", {"ob": 1024}, [(300, 3), (420, 3), (420, 17)]),
    ("ob1024_ksplit1", {"ob": 1024, "ksplit": 1}, [(420, 3)]),
    ("fused", {"ob": 1024, "trsm": 0, "lat": 0, "fuse_min": 1}, [(300, 8), (420, 8)]),
    ("fused_la", {"ob": 1024, "trsm": 0, "lat": 0, "fuse_min": 1, "la": 1}, [(300, 8), (420, 8)]),
    ("fused_rowblock", {"ob": 1024, "trsm": 0, "lat": 0, "fuse_min": 1, "syrk_diag": 0}, [(300, 8), (420, 8)]),
    ("unfused_b8", {"ob": 1024, "trsm": 0, "lat": 0, "fuse": 0}, [(300, 8), (420, 8)]),
    ("col32", {"p128": 0}, [(n, 3) for n in SIZES] + [(300, 8)]),
    ("persist", {"persist": 1}, [(n, 3) for n in SIZES]),
]


def plan_kind(form, steps):
    """The rule's kind for a plan as gpmpc_potrf_plan reports it."""
    if form == "32":
        return "col32"
    if form == "persist":
        return "core"
    modes = {s[3 + 2] for s in steps if s[0] == "diag"}
    assert len(modes) == 1, modes
    return {0: "core", 1: "inv128", 3: "trsm32"}[modes.pop()]


def plan_coverage(plans):
    """What a list of (form, steps) plans contains, as a set of labels."""
    have = set()
    for form, steps in plans:
        have.add(f"form:{form}")
        for kind, c, K0, a0, a1, a2, a3 in steps:
            have.add(f"step:{kind}")
            if kind == "diag":
                have.add(f"diag:mode{a2}:{'packed' if a1 else 'full'}")
            if kind == "upd_syrk_diag":
                have.add(f"upd_syrk_diag:ks{'>1' if a2 > 1 else '=1'}")
            if kind == "upd_rowblock":
                have.add(f"upd_rowblock:ks{'>1' if a3 > 1 else '=1'}")
            if kind == "updsolve":
                have.add(f"updsolve:K{'>0' if a1 > 0 else '=0'}")
                if a2 > 0:
                    have.add("updsolve:wn>0")
            if kind == "trail_syrk":
                have.add(f"trail_syrk:K{a1}")
    return have


COVERAGE = {"form:32", "form:persist", "form:128",
            "step:diag", "step:upd_syrk_diag", "step:upd_rowblock", "step:updsolve", "step:psolve_trsm",
            "step:psolve_lat", "step:psolve_rowblock", "step:trail_lat", "step:trail_syrk",
            "diag:mode0:full", "diag:mode1:full", "diag:mode1:packed", "diag:mode3:full", "diag:mode3:packed",
            "upd_syrk_diag:ks=1", "upd_syrk_diag:ks>1", "upd_rowblock:ks=1", "upd_rowblock:ks>1",
            "updsolve:K=0", "updsolve:K>0", "updsolve:wn>0", "trail_syrk:K256", "trail_syrk:K128"}
# (mode 0, the per-block inverse form, has no packed kernel: the plan packs only under the sweep)


def run_params(name, i):
    """The family and layout of the i-th case of a factor run: a fixed rotation, so every
    family and layout meets every path over the sizes of a run."""
    h = sum(map(ord, name))
    return FAMILIES[(h + i) % len(FAMILIES)], LAYOUTS[(h // 4 + i) % len(LAYOUTS)]


def factor_case(name, i, n, batch):
    family, variant = run_params(name, i)
    return FactorCase(factor_mats(family, n, batch), variant, tag=f"{name} n {n} b{batch} {family} {variant}")


# ---- the triangular rules ------------------------------------------------------------------
def trsm_bound(L, Xh, trans):
    n = len(L)
    aL, aX = np.abs(np.tril(L)), np.abs(Xh)
    bound = c1(n) * U * ((aL.T if trans else aL) @ aX)
    for r0 in range(0, n, NB):
        r1 = min(n, r0 + NB)
        bound[r0:r1] += c2(NB) * U * (cond_block(L[r0:r1, r0:r1], trans) @ aX[r0:r1])
    return bound


def _ratio(res, bound):
    with np.errstate(all="ignore"):
        r = (res / np.maximum(bound, np.finfo(np.float64).tiny)).astype(np.float64)
    return float(np.max(r)) if r.size and np.all(np.isfinite(r)) else (0.0 if not r.size else float("nan"))


def _mm(a, b):
    dt = LD if gc.longdouble_ok() else np.float64
    return np.matmul(np.asarray(a).astype(dt), np.asarray(b).astype(dt))


def trsm_ratio(L, B, Xh, trans):
    L = np.tril(L)
    if not np.all(np.isfinite(Xh)):
        return float("nan")
    res = np.abs(_mm(L.T if trans else L, Xh) - B)
    return _ratio(res, trsm_bound(L, Xh, trans))


def tri_inverse_bound(L, Wh):
    n = len(L)
    aL, aW = np.abs(np.tril(L)), np.abs(Wh)
    E = np.zeros((n, n))
    for d0 in range(0, n, DB):
        d1 = min(n, d0 + DB)
        E[d0:d1, d0:d1] = trsm_bound(L[d0:d1, d0:d1], Wh[d0:d1, d0:d1], False)
    b = DB
    while b < n:
        g = (2 * b + 8) * U
        for s0 in range(0, n, 2 * b):
            c0, c1_ = s0 + b, min(n, s0 + 2 * b)
            if c0 >= n:
                break
            P = (1 + g) * (aL[c0:c1_, s0:c0] @ aW[s0:c0, s0:c0])
            E[c0:c1_, s0:c0] = g * P + E[c0:c1_, c0:c1_] @ P + g * (aL[c0:c1_, c0:c1_] @ (aW[c0:c1_, c0:c1_] @ P))
        b *= 2
    return E


def tri_inverse_ratio(L, Wh):
    n = len(L)
    if not np.all(np.isfinite(Wh)) or np.any(np.triu(Wh, 1) != 0.0):
        return float("nan")
    res = np.abs(_mm(np.tril(L), Wh) - np.eye(n))
    low = np.tril(np.ones((n, n), bool))
    return _ratio(res[low], tri_inverse_bound(L, Wh)[low])


def cho_ratio(L, y, ah):
    L = np.tril(L)
    if not np.all(np.isfinite(ah)):
        return float("nan")
    res = np.abs(_mm(L, _mm(L.T, ah)) - y)
    aL = np.abs(L)
    return _ratio(res, cs(len(L)) * U * (aL @ (aL.T @ np.abs(ah))))


# ---- float64 restatements of the triangular forms ------------------------------------------
def _walk32(L, X, trans, rhs_lower=False, mut=None, met=None):
    """k_trsm_panel on one <= 128-row block, in place: 32-row blocks, each by the product
    with its block's explicit inverse."""
    n = len(L)
    blocks = list(range(0, n, NB))
    Ts = [tri_inv(L[r:r + NB, r:r + NB]) for r in blocks]
    for q in (reversed(range(len(blocks))) if trans else range(len(blocks))):
        r0 = blocks[q]
        r1 = min(n, r0 + NB)
        if mut == "skiplast" and r1 - r0 < NB and len(blocks) > 1:
            met.append(1)
            continue
        Tq = Ts[q]
        if mut == "previnv" and q == 1 and r1 - r0 == NB:
            Tq = Ts[0]
            met.append(1)
        if trans:
            acc = X[r0:r1] - L[r1:, r0:r1].T @ X[r1:]
            X[r0:r1] = Tq.T @ acc
        else:
            acc = X[r0:r1] - L[r0:r1, :r0] @ X[:r0]
            X[r0:r1] = Tq @ acc


def restate_trsm(L, B, trans, mut=None, met=None):
    """launch_trsm_lower_ex in float64: 128-row blocks, the panel walk on each, one product
    to update the rows below (forward) or above (backward).  mut: previnv, skiplast, kslice."""
    L = np.tril(L)
    n = len(L)
    X = np.array(B, np.float64, copy=True)
    met = [] if met is None else met
    starts = list(range(0, n, DB))
    for r0 in (reversed(starts) if trans else starts):
        r1 = min(n, r0 + DB)
        _walk32(L[r0:r1, r0:r1], X[r0:r1], trans, mut=mut, met=met)
        if trans and r0 > 0:
            Lu = L[r0:r1, :r0]
            upd = Lu.T @ X[r0:r1]
            if mut == "kslice" and r0 == starts[-1] and r1 - r0 >= 16:
                upd[:DB] -= Lu[:16, :DB].T @ X[r0:r0 + 16]
                met.append(1)
            X[:r0] -= upd
        if not trans and r1 < n:
            Ld = L[r1:, r0:r1]
            upd = Ld @ X[r0:r1]
            if mut == "kslice" and r0 == 0:
                upd[:DB] -= Ld[:DB, 16:32] @ X[16:32]
                met.append(1)
            X[r1:] -= upd
    return X


def restate_tri_inverse(L, mut=None, met=None):
    """launch_tri_inverse in float64: the 128 x 128 diagonal blocks by the panel walk on the
    identity, then the doubling levels W_CA = -W_CC (L_CA W_AA).  mut: previnv, skiplast (the
    ragged last pair of a level left out), kslice."""
    L = np.tril(L)
    n = len(L)
    W = np.eye(n)
    met = [] if met is None else met
    for d0 in range(0, n, DB):
        d1 = min(n, d0 + DB)
        _walk32(L[d0:d1, d0:d1], W[d0:d1, d0:d1], False, mut=mut if mut == "previnv" else None, met=met)
    b = DB
    while b < n:
        for s0 in range(0, n, 2 * b):
            c0, c1_ = s0 + b, min(n, s0 + 2 * b)
            if c0 >= n:
                break
            if mut == "skiplast" and c1_ - c0 < b:
                met.append(1)
                continue
            tmp = L[c0:c1_, s0:c0] @ W[s0:c0, s0:c0]
            if mut == "kslice" and s0 == 0 and b == DB:
                tmp -= L[c0:c1_, 16:32] @ W[16:32, s0:c0]
                met.append(1)
            W[c0:c1_, s0:c0] = -(W[c0:c1_, c0:c1_] @ tmp)
        b *= 2
    return W


def restate_cho_solve_inv(L, W, y, refine=True):
    """cho_solve_inv in float64: a1 = W^T (W y); r = y - L (L^T a1); a = a1 + W^T (W r)."""
    L, W = np.tril(L), np.tril(W)
    a1 = W.T @ (W @ y)
    if not refine:
        return a1
    r = y - L @ (L.T @ a1)
    return a1 + W.T @ (W @ r)


def restate_potrs(L, y):
    """The two substitutions in float64."""
    z = sla.solve_triangular(np.tril(L), y, lower=True)
    return sla.solve_triangular(np.tril(L), z, lower=True, trans="T")


# ---- the exact family ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_L(n, seed=0):
    """(L, L^-1) of the exact family, both exact in fp64."""
    rng = np.random.default_rng([n, seed, 77])
    S = rng.random(n) < 0.5
    N = rng.integers(-3, 4, size=(n, n)).astype(np.float64)
    N *= np.tril(np.ones((n, n)), -1) * (~S)[:, None] * S[None, :]
    D = 2.0 ** rng.integers(-1, 3, n)
    L = (np.eye(n) + N) * D[None, :]
    Linv = (np.eye(n) - N) / D[:, None]
    assert np.array_equal(L @ Linv, np.eye(n)) and np.array_equal(Linv @ L, np.eye(n))
    for a in (L, Linv):
        a.setflags(write=False)
    return L, Linv


def integer_rhs(n, nrhs, seed=0, lower=False):
    B = np.random.default_rng([n, nrhs, seed, 78]).integers(-3, 4, size=(n, nrhs)).astype(np.float64)
    return np.tril(B) if lower else B


def assert_exact_range(L, Linv, B):
    """Every sum of absolute values that any order of the operations can form stays below
    2^47 in units of 2^-6: fp64 is exact on them."""
    aL, aI, aB = np.abs(L), np.abs(Linv), np.abs(B)
    a1 = aI.T @ (aI @ aB)
    big = max(np.max(aL @ (aL.T @ a1), initial=0.0), np.max(aL @ (aI @ aB), initial=0.0))
    assert big * 64 < 2.0 ** 53, big
    for a in (L, Linv, B):
        assert np.array_equal(a * 64, np.round(a * 64))


# ---- triangular cases on flat buffers --------------------------------------------------------
class TriCase:
    """One gpmpc_tri_diag call: L (n x n, strict upper poisoned), X = B (n x nrhs), W (the
    inverse, cho_solve_inv only) in poisoned flat buffers.  exact: the result must equal
    want; else the op's residual rule against L and B."""

    def __init__(self, op, L, B, flags=0, W=None, want=None, variant="even", tag=""):
        self.op, self.flags, self.want, self.tag = op, flags, want, tag
        self.L, self.B = np.asarray(L, np.float64), np.asarray(B, np.float64)
        self.n, self.nrhs = self.B.shape
        n = self.n
        low = np.tril(np.ones((n, n), bool))
        packed = op in ("cho_solve_inv", "potrs_cols")
        vl = "packed" if op == "cho_solve_inv" and variant != "shift" else variant
        ld, _, sh = layout(n, n, vl, 1)
        self.bL = Buf(np.where(low, self.L, poison((n, n)))[None], n if op == "cho_solve_inv" else ld, None, sh)
        ldx, _, shx = layout(self.nrhs, n, "packed" if packed and variant != "shift" else variant, 1)
        self.bX = Buf(self.B[None], self.nrhs if packed else ldx, None, shx)
        self.bW = None
        if W is not None:
            self.bW = Buf(np.where(low, np.asarray(W, np.float64), poison((n, n)))[None], n, None, sh)
        # what the operation may write: all of X; a lower-triangular right-hand side and the
        # inverse keep the zeros above the diagonal (never written)
        self.written = np.ones((1, n, self.nrhs), bool)
        if op == "tri_inverse" or flags & 2:
            self.written = (np.arange(self.nrhs)[None, :] <= np.arange(n)[:, None])[None].copy()

    def bufs(self):
        return [b for b in (self.bL, self.bX, self.bW) if b is not None]

    def ratio(self, Xh):
        trans = bool(self.flags & 1)
        if self.op == "trsm":
            return trsm_ratio(self.L, self.B, Xh, trans)
        if self.op == "tri_inverse":
            return tri_inverse_ratio(self.L, Xh)
        return cho_ratio(self.L, self.B, Xh)

    def verify(self, after, report=None):
        """after: {id(buf): flat array}.  Violations (empty: pass)."""
        bad = []
        for b in self.bufs():
            w = self.written if b is self.bX else None
            bad += gc.check_untouched(b, after[id(b)], w, "X" if b is self.bX else "input")
        Xh = self.bX.get(after[id(self.bX)])[0]
        if self.want is not None:
            bad += gc.check_values(Xh[None], np.asarray(self.want)[None], self.written)
        else:
            r = self.ratio(Xh)
            if report is not None:
                report.append((self.tag, r))
            if not r <= 1.0:
                bad.append(f"residual / bound = {r:.3g}")
        return [f"{self.tag}: {m}" for m in bad]

    def after_with(self, Xh):
        """The buffers after an operation that left Xh in X's written part."""
        after = {id(b): b.flat.copy() for b in self.bufs()}
        after[id(self.bX)] = self.bX.with_values(np.asarray(Xh, np.float64)[None], self.written)
        return after


TRI_N = (1, 31, 33, 64, 128, 129, 256, 257, 300, 385, 517)
REAL_FAMILIES = ("wishart", "graded", "gp6", "gp8")


def tri_nrhs(n):
    return sorted({1, 5, 63, 64, 65, n})


def trsm_case(n, nrhs, trans, family, variant, rhs_lower=False, seed=0):
    """family 'integer': exact; else L from a factor family and a standard normal B."""
    flags = (1 if trans else 0) | (2 if rhs_lower else 0)
    tag = f"trsm n {n} nrhs {nrhs} {'bwd' if trans else 'fwd'}{' rhs_lower' if rhs_lower else ''} {family} {variant}"
    if family == "integer":
        L, Linv = integer_L(n, seed)
        B = integer_rhs(n, nrhs, seed, rhs_lower)
        assert_exact_range(L, Linv, B)
        return TriCase("trsm", L, B, flags, want=(Linv.T if trans else Linv) @ B, variant=variant, tag=tag)
    B = np.random.default_rng([n, nrhs, seed, 79]).standard_normal((n, nrhs))
    return TriCase("trsm", family_L(family, n, seed), np.tril(B) if rhs_lower else B, flags, variant=variant, tag=tag)


def tri_inverse_case(n, family, variant, seed=0):
    tag = f"tri_inverse n {n} {family} {variant}"
    if family == "integer":
        L, Linv = integer_L(n, seed)
        return TriCase("tri_inverse", L, np.eye(n), want=Linv, variant=variant, tag=tag)
    return TriCase("tri_inverse", family_L(family, n, seed), np.eye(n), variant=variant, tag=tag)


def cho_case(op, n, nc, family, variant, seed=0):
    """op: cho_solve_inv (W = the float64 doubling inverse of L, as the fit forms it) or potrs_cols."""
    tag = f"{op} n {n} nc {nc} {family} {variant}"
    if family == "integer":
        L, Linv = integer_L(n, seed)
        y = integer_rhs(n, nc, seed)
        assert_exact_range(L, Linv, y)
        return TriCase(op, L, y, W=Linv if op == "cho_solve_inv" else None, want=Linv.T @ (Linv @ y),
                       variant=variant, tag=tag)
    L = family_L(family, n, seed)
    y = np.random.default_rng([n, nc, seed, 80]).standard_normal((n, nc))
    return TriCase(op, L, y, W=restate_tri_inverse(L) if op == "cho_solve_inv" else None, variant=variant, tag=tag)
