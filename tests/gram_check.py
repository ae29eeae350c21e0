"""References, cases and the pass/fail rule for the Gram kernels (csrc/gram.hip), in numpy.

Shared by tests/test_gram_check.py (no GPU: the rule accepts a float64 restatement of the
kernels' arithmetic and rejects subtly wrong ones) and tests/test_gpu_gram.py (the kernels
through gpmpc_gram / gpmpc_gram_grad).

Reference.  np.longdouble from the raw inputs with direct differences,
    d2 = sum_k ((x1_k - x2_k) / l_k)^2            (SE iso: l_k = 1, the raw rows)
and the kind's formula as oracle/gp_oracle.gram states it:
    se_ard    sigma2 exp(-d2 / 2)                          s = d2 / 2
    se_iso    sigma2 exp(-d2 / (2 l^2))                    s = d2 / (2 l^2)
    matern32  sigma2 (1 + s) exp(-s),            s = sqrt(3 d2)
    matern52  sigma2 (1 + s + s^2 / 3) exp(-s),  s = sqrt(5 d2)
(s: the magnitude of the exponent).  The direct form has no cancellation, so the reference
is good to a few longdouble roundings relative.

Rule.  |K - K_ref| <= sigma2 c_kind (2d + 10) u (na + nb) + (8 + 4 s) u |K_ref|,  u = 2^-53,
elementwise, with na / nb the squared norms of the scaled rows.  It is derived from what
the kernels compute, f(clamp(d2^)) with d2^ = (na^ + nb^) - 2 dot^ of rows scaled in fp64:

* a^_k = fl(x_k / l_k) = a_k (1 + e), |e| <= u (SE iso: exact).  na^ is a d-term fma sum of
  a^_k^2: |na^ - na| <= (d + 3) u na (2u from the squares of the rounded rows, d + 1 from
  the sum), the same for nb.  dot^ is a d-term fma chain: |dot^ - dot| <= (d + 2) u
  sum |a_k b_k| <= (d + 2) u (na + nb) / 2.  The sum na^ + nb^ rounds once, u (na + nb); the
  subtraction rounds once, u |d2^| <= 2 u (na + nb).  Together
      |d2^ - d2| <= ((d + 3) + (d + 2) + 1 + 2) u (na + nb) = (2d + 8) u (na + nb)
  to first order; the rule takes 2d + 10 for the higher orders.  This error is absolute
  and does not shrink with d2: where |x| >> |x1 - x2| the expansion form cancels.
* d2 >= 0 and the clamp max(., 0) is 1-Lipschitz, so the clamped value is no further from
  d2.  By the mean value theorem the kernel value moves by at most sigma2 sup |df/d(d2)|
  times that: f = exp(-d2 / 2): 1/2;  exp(-d2 c), c = 1 / (2 l^2): c;  matern32,
  df/d(d2) = -(3/2) exp(-s): 3/2;  matern52, df/d(d2) = -(5/6)(1 + s) exp(-s): 5/6.
  That is c_kind.
* The epilogue's own roundings are relative to the value.  Not scaled by s: the final
  sum(s) of the Matern polynomial (<= 2u), exp itself (<= 1 ulp = 2u), the two products
  (2u): <= 6u.  Scaled by s, because a relative error e in the argument of exp(-s) is s e
  in the value: se_ard none (d2 / 2 is exact); se_iso 3u (l l, the reciprocal, the
  product); Matern 3u (sqrt, the rounded constant, the product), and through the polynomial
  (3 s + 5 s^2 / 3) / (1 + s + s^2 / 3) u <= (2 + s) u for matern52, 3 s / (1 + s) u for
  matern32.  Every kind stays below (8 + 4 s) u to first order.

Gradients (gpmpc_gram_grad), from the same terms: SE-ARD plane i is K q_i with
q_i = (x1_i - x2_i)^2 / l_i^2 formed from the raw rows (the difference, its square, l l, the
quotient and the product with K: 7u relative to first order), so
    |G_i - G_ref_i| <= bound_K q_i + 8 u |G_ref_i|;
SE iso is K d2 / l^2 with d2 the expansion form of the raw rows again, so
    |G - G_ref| <= bound_K d2 / l^2 + |K_ref| (2d + 10) u (na + nb) / l^2 + 8 u |G_ref|.

Cases.  Four data families: centred (unit normal), offset (|x| about 10, spread 1e-2: the
expansion form cancels), cluster (three centres, spread 1e-3) and integer.  The integer
family is exact by construction: inputs are integers in -4..4, lengthscales powers of two,
sigma2 = 1, so the scaled rows, norms, dot product and d2 are exact in fp64 and only the
relative term is allowed.  Lengthscales are of the order of sqrt(d) times the spread: every
builder asserts that >= 90% of the reference entries exceed 1e-3 sigma2 (with unit
lengthscales at d = 32 every entry would be about e^-32 and an absolute bound would pass
any kernel) and that the bound stays below sigma2 / 2 * 1e-9.  A cross case has rows of X2
that equal rows of X1 (d2 = 0, the clamp); a self case (X2 None) has two equal rows and a
diagonal that must be exactly sigma2.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
POISON = np.uint64(0x7FF8C0DEC0DE0BAD)
KINDS = ("se_ard", "se_iso", "matern32", "matern52")   # index = the library's kind code
FAMILIES = ("centred", "offset", "cluster", "integer")
SQRT3, SQRT5 = 1.7320508075688772, 2.23606797749979     # the kernels' constants (internal.h)


def longdouble_ok():
    """The rule needs a reference clearly finer than fp64 (x87: 1.08e-19)."""
    return float(np.finfo(LD).eps) < 1e-18


def poison(shape):
    return np.full(shape, POISON, np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def c_kind(kind, l_iso=None):
    """sup |dk / d(d2)| / sigma2."""
    if kind == "se_iso":
        return 1.0 / (2.0 * float(l_iso) ** 2)
    return {"se_ard": 0.5, "matern32": 1.5, "matern52": 5.0 / 6.0}[kind]


# ---- longdouble references ---------------------------------------------------------------
def _value(kind, d2, sigma2, l_iso):
    """(k, s) of d2 in the dtype of d2."""
    if kind == "se_ard":
        s = d2 / 2
        return sigma2 * np.exp(-s), s
    if kind == "se_iso":
        s = d2 / (2 * d2.dtype.type(l_iso) ** 2)
        return sigma2 * np.exp(-s), s
    if kind == "matern32":
        s = np.sqrt(3 * d2)
        return sigma2 * (1 + s) * np.exp(-s), s
    if kind == "matern52":
        s = np.sqrt(5 * d2)
        return sigma2 * (1 + s + s * s / 3) * np.exp(-s), s
    raise ValueError(kind)


def sqdist_planes(X1, X2, ls):
    """q (d, n1, n2) = ((x1_k - x2_k) / l_k)^2 in longdouble, direct differences."""
    X1, X2, ls = X1.astype(LD), X2.astype(LD), np.asarray(ls, LD)
    return np.stack([((X1[:, k, None] - X2[None, :, k]) / ls[k]) ** 2 for k in range(X1.shape[1])])


def reference(kind, X1, X2, ls, sigma2):
    """(K_ref, s, q) in longdouble; X2 None: X1.  ls: d lengthscales (se_iso: one, the
    distance is that of the raw rows)."""
    X2 = X1 if X2 is None else X2
    d = X1.shape[1]
    iso = kind == "se_iso"
    q = sqdist_planes(X1, X2, np.ones(d) if iso else ls)
    K, s = _value(kind, q.sum(axis=0), LD(sigma2), ls[0] if iso else None)
    return K, s, q


def norms(kind, X, ls):
    """Squared norms of the rows as the kernels scale them (se_iso: raw)."""
    a = X.astype(LD) if kind == "se_iso" else X.astype(LD) / np.asarray(ls, LD)
    return (a * a).sum(axis=1)


# ---- cases ---------------------------------------------------------------------------------
class Case:
    """One Gram: inputs, the longdouble reference and the elementwise bound (grad: also
    those of every gradient plane)."""

    def __init__(self, kind, X1, X2, ls, sigma2, family, grad=False):
        self.kind, self.X1, self.X2, self.sigma2, self.family = kind, X1, X2, float(sigma2), family
        self.ls = np.asarray(ls, np.float64)
        self.n1, self.d = X1.shape
        self.n2 = self.n1 if X2 is None else X2.shape[0]
        self.code = KINDS.index(kind)
        self.exact = family == "integer"
        self.tag = (f"{kind} {self.n1}x{'self' if X2 is None else self.n2} d {self.d} {family}"
                    f"{' grad' if grad else ''}")
        self.ref, self.s, q = reference(kind, X1, X2, self.ls, sigma2)
        iso = kind == "se_iso"
        nsum = norms(kind, X1, self.ls)[:, None] + norms(kind, X1 if X2 is None else X2, self.ls)[None, :]
        # |d2^ - d2|: zero in the family whose d2 is exact in fp64
        self.e_d2 = np.zeros_like(nsum) if self.exact else (2 * self.d + 10) * U * nsum
        self.bound = sigma2 * c_kind(kind, self.ls[0]) * self.e_d2 + (8 + 4 * self.s) * U * np.abs(self.ref)
        assert np.mean(self.ref > 1e-3 * sigma2) >= 0.9, f"{self.tag}: badly scaled, most entries vanish"
        assert float(self.bound.max()) < 0.5e-9 * sigma2, f"{self.tag}: bound {float(self.bound.max()):.2e}"
        if X2 is not None and self.n2 >= 2:
            assert np.count_nonzero(q.sum(axis=0) == 0) >= 1, f"{self.tag}: no row of X2 equals a row of X1"
        if grad:
            assert kind in ("se_ard", "se_iso")
            if iso:
                l2 = LD(self.ls[0]) ** 2
                d2 = q.sum(axis=0)
                self.gref = (self.ref * d2 / l2)[None]
                self.gbound = (self.bound * d2 / l2 + np.abs(self.ref) * self.e_d2 / l2)[None] + 8 * U * np.abs(self.gref)
            else:
                self.gref = self.ref[None] * q
                self.gbound = self.bound[None] * q + 8 * U * np.abs(self.gref)


def lengthscales(kind, d, family, rng):
    """Of the order of sqrt(d) times the spread, not all equal; the integer family's are
    powers of two."""
    if family == "integer":
        p = 2.0 ** np.ceil(np.log2(3.0 * np.sqrt(d)))
        ls = p * np.where(np.arange(d) % 2 == 0, 1.0, 2.0)
    else:
        base = 10.0 * np.sqrt(d) * 1e-2 if family == "offset" else 1.5 * np.sqrt(d)
        ls = base * rng.uniform(1.0, 1.5, d)
    return ls[:1].copy() if kind == "se_iso" else ls


def rows(rng, n, d, family, centres):
    if family == "centred":
        return rng.standard_normal((n, d))
    if family == "offset":
        return 10.0 + 1e-2 * rng.standard_normal((n, d))
    if family == "cluster":
        return centres[rng.integers(0, 3, n)] + 1e-3 * rng.standard_normal((n, d))
    return rng.integers(-4, 5, size=(n, d)).astype(np.float64)


def make_case(kind, n1, n2, d, family, seed=0, grad=False):
    """n2 None: the self-Gram (X2 = None), with X1[1] = X1[0].  Else rows j = 2 mod 3 of X2
    and its last row (n2 >= 2) are rows of X1."""
    rng = np.random.default_rng([seed, KINDS.index(kind), n1, n2 or 0, d, FAMILIES.index(family)])
    centres = rng.standard_normal((3, d))
    X1 = rows(rng, n1, d, family, centres)
    sigma2 = 1.0 if family == "integer" else 1.7
    ls = lengthscales(kind, d, family, rng)
    if n2 is None:
        if n1 >= 2:
            X1[1] = X1[0]
        return Case(kind, X1, None, ls, sigma2, family, grad)
    X2 = rows(rng, n2, d, family, centres)
    for j in range(n2):
        if n2 >= 2 and (j % 3 == 2 or j == n2 - 1):
            X2[j] = X1[(5 * j + 1) % n1]
    return Case(kind, X1, X2, ls, sigma2, family, grad)


SHAPES = ((1, 1), (64, 64), (63, 65), (65, 63), (129, 130))   # one tile, its edges, three tiles
WIDTHS = (1, 2, 3, 10, 11, 12, 13, 14, 32)
FULL_GRID = (3, 11, 14)


def kgram_specs(d):
    """(kind, n1, n2, d, family) of the k_gram cases of width d: for d in FULL_GRID every
    kind x shape x {cross, self}; else per kind the three-tile cross shape, one of the
    other shapes in turn and the 65-row self-Gram.  The family rotates."""
    out, i = [], WIDTHS.index(d)
    for ki, kind in enumerate(KINDS):
        if d in FULL_GRID:
            shapes = [s for s in SHAPES] + [(n1, None) for n1, _ in SHAPES]
        else:
            shapes = [SHAPES[4], SHAPES[(i + ki) % 4], (65, None)]
        for n1, n2 in shapes:
            out.append((kind, n1, n2, d, FAMILIES[i % 4]))
            i += 1
    return out


ROWS_N1 = (512, 513, 640, 767)   # four full row tiles; a last tile of one row; five full; a 127-row tile
ROWS_N2 = (1, 64, 65, 130)


def rows_specs(d):
    """The k_gram_rows cases of width d (11, 12, 13): every kind x n1, n2 in turn so that
    every (n1, n2) pair occurs."""
    out = []
    for ki, kind in enumerate(KINDS):
        for ni, n1 in enumerate(ROWS_N1):
            i = (d - 11) * 4 + ki + ni
            out.append((kind, n1, ROWS_N2[i % 4], d, FAMILIES[(i + ki) % 4]))
    return out


GRAD_SHAPES = ((3, 257), (65, 300), (70, None))
GRAD_WIDTHS = (1, 3, 11, 32)


def grad_specs(kind):
    out, i = [], 0
    for n1, n2 in GRAD_SHAPES:
        for d in GRAD_WIDTHS:
            out.append((kind, n1, n2, d, FAMILIES[(i + KINDS.index(kind)) % 4]))
            i += 1
    return out


# ---- the rule --------------------------------------------------------------------------------
def violations(got, ref, bound, tag, what="K"):
    """[] when every element of got lies within bound of ref (NaN compares false: fails)."""
    got = np.asarray(got, np.float64)
    if got.shape != ref.shape:
        return [f"{tag}: {what} has shape {got.shape}, want {ref.shape}"]
    err = np.abs(got.astype(LD) - ref)
    ok = err <= bound
    n = int(np.count_nonzero(~ok))
    if n == 0:
        return []
    i = tuple(int(x) for x in np.argwhere(~ok)[0])
    return [f"{tag}: {what}: {n} element(s) outside the bound, first at {i}: got {got[i]!r}, want "
            f"{float(ref[i])!r}, |err| {float(err[i]):.3e} > {float(bound[i]):.3e}"]


def worst_ratio(got, ref, bound):
    """max |err| / bound (a figure for reports)."""
    err = np.abs(np.asarray(got, np.float64).astype(LD) - ref)
    return float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))) if err.size else 0.0


def check_gram(case, got):
    bad = violations(got, case.ref, case.bound, case.tag)
    if case.X2 is None and not bad:
        dg = np.diagonal(np.asarray(got, np.float64))
        if not np.all(dg == case.sigma2):
            bad.append(f"{case.tag}: the self-Gram's diagonal is not exactly sigma2 (first {dg[dg != case.sigma2][0]!r})")
    return bad


def check_grad(case, G):
    return violations(G, case.gref, case.gbound, case.tag, "G")


# ---- float64 restatement of the kernels' arithmetic -------------------------------------------
def fma(a, b, c):
    """a * b + c rounded once to float64 (through longdouble; a second rounding there is
    2^-11 of an fp64 ulp)."""
    return (np.asarray(a, LD) * b + c).astype(np.float64)


def scale_rows(kind, X, ls):
    """k_scale_rows: (rows over the lengthscales, their squared norms as an fma sum)."""
    a = X.copy() if kind == "se_iso" else X / ls
    s = np.zeros(X.shape[0])
    for k in range(X.shape[1]):
        s = fma(a[:, k], a[:, k], s)
    return a, s


def epilogue(kind, d2, sigma2, iso_scale):
    """kernel_epilogue (internal.h) in float64."""
    d2 = np.where(d2 > 0.0, d2, 0.0)
    if kind == "se_ard":
        return sigma2 * np.exp(-0.5 * d2)
    if kind == "se_iso":
        return sigma2 * np.exp(-d2 * iso_scale)
    r = np.sqrt(d2)
    if kind == "matern32":
        s3 = SQRT3 * r
        return sigma2 * (1.0 + s3) * np.exp(-s3)
    s5 = SQRT5 * r
    return sigma2 * (1.0 + s5 + 5.0 * (r * r) / 3.0) * np.exp(-s5)


def restate(case, nfeat=None, ls=None, a_rows=None):
    """The Gram as k_gram / k_gram_rows compute it.  Hooks for wrong kernels: nfeat (the
    features the loops run over), ls (other lengthscales), a_rows(a) -> the a-rows the dot
    product reads."""
    ls = case.ls if ls is None else ls
    d = case.d if nfeat is None else nfeat
    a, na = scale_rows(case.kind, case.X1[:, :d], ls[:d])
    b, nb = (a, na) if case.X2 is None else scale_rows(case.kind, case.X2[:, :d], ls[:d])
    ad = a if a_rows is None else a_rows(a)
    dot = np.zeros((case.n1, case.n2))
    for k in range(d):
        dot = fma(ad[:, k, None], b[None, :, k], dot)
    d2 = (na[:, None] + nb[None, :]) - 2.0 * dot
    iso_scale = 1.0 / (2.0 * case.ls[0] * case.ls[0]) if case.kind == "se_iso" else 0.0
    return epilogue(case.kind, d2, case.sigma2, iso_scale)


def restate_grad(case, K):
    """k_gram_grad from K in float64: (d or 1, n1, n2)."""
    X2 = case.X1 if case.X2 is None else case.X2
    if case.kind == "se_ard":
        return np.stack([K * (((case.X1[:, i, None] - X2[None, :, i]) ** 2) / (case.ls[i] * case.ls[i]))
                         for i in range(case.d)])
    _, na = scale_rows("se_iso", case.X1, None)
    _, nb = scale_rows("se_iso", X2, None)
    dot = np.zeros((case.n1, case.n2))
    for k in range(case.d):
        dot = fma(case.X1[:, k, None], X2[None, :, k], dot)
    d2 = (na[:, None] + nb[None, :]) - 2.0 * dot
    d2 = np.where(d2 > 0.0, d2, 0.0)
    return ((K * d2) / (case.ls[0] * case.ls[0]))[None]


def aliased_rows(a, tile=64):
    """The a-rows a kernel would read whose LDS tile is one double wide while it indexes
    [r][k]: row r, feature k is row r + k, feature 0 of the same tile (zero past it)."""
    n, d = a.shape
    out = np.zeros_like(a)
    for r in range(n):
        t0 = r - r % tile
        for k in range(d):
            j = r + k
            if j < t0 + tile and j < n:
                out[r, k] = a[j, 0]
    return out


def first_tile_rows(a, tile):
    """Rows of the second row tile served from the first tile's."""
    out = a.copy()
    hi = min(2 * tile, a.shape[0])
    out[tile:hi] = a[:hi - tile]
    return out


# ---- the GP at the width of the runtime-width kernel ------------------------------------------
def gp_case():
    """(X, Y, ls, sigma2, noise, Xq): d = 3, n = 70, three outputs, SE-ARD, noise 1e-4 --
    data for which gp_oracle's plain Cholesky succeeds (jitter ladder step 0;
    tests/test_gram_check.py asserts it)."""
    rs = np.random.RandomState(3)
    X = rs.randn(70, 3)
    Y = np.stack([np.sin(X[:, 0]) + 0.3 * X[:, 1], np.cos(X[:, 1] * X[:, 2]), X[:, 2] ** 2], 1) + 0.01 * rs.randn(70, 3)
    Xq = np.vstack([X[::9] + 0.05, rs.randn(9, 3)])
    return X, Y, np.array([1.1, 1.6, 2.1]), 1.3, 1e-4, Xq
