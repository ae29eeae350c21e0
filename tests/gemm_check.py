"""References and the pass/fail rule for the FP64 GEMM family (csrc/gemm.hip), in numpy.

Shared by tests/test_gemm_check.py (no GPU: proves the rule rejects subtly wrong
results) and tests/test_gpu_gemm.py (runs the kernels through gpmpc_gemm_diag).

Two checks:

* exact -- operands are integers in -3..3 stored as fp64, alpha and beta come from
  {0, 1, -1, 2, 0.5}, C0 is small integers.  Up to K = 1100 every partial sum of every
  summation order (tiles, K splits, atomics, stream-K segments) is a multiple of 1/2 far
  below 2^53, so fp64 arithmetic is exact and the result must EQUAL
  alpha * (A @ B.T) + beta * C0 as numpy float64 computes it (itself exact).  Tolerance
  zero.  (Equality of values: the sign of an exact zero is not compared, it depends on
  whether a kernel adds beta * C0 = 0 or skips it.)
* real -- these integers are exact in fp32 too, so a second check uses standard normal
  operands against a numpy longdouble reference, elementwise
      |C - ref| <= (2K + 8) u (|alpha| |A| |B|^T + |beta| |C0|),   u = 2^-53:
  K u is the fma dot-product bound for any summation order, + 3 u for the epilogue,
  + at most 16 u for atomic partial adds (rounded up to 8 + K u of margin: the factor 2).

Every operand lives in a flat buffer with a band of >= 128 * ld doubles on both sides;
band, ld gaps and every element the operation must not write hold one fixed NaN bit
pattern (POISON) and must be bit-unchanged afterwards; a poisoned element read into a
product shows up as NaN in the result.
"""
import numpy as np

U = 2.0 ** -53
POISON = np.uint64(0x7FF8C0DEC0DE0BAD)
SCALARS = (0.0, 1.0, -1.0, 2.0, 0.5)
LD = np.longdouble


def longdouble_ok():
    """The real-valued check needs a reference clearly finer than fp64 (x87: 1.08e-19)."""
    return float(np.finfo(LD).eps) < 1e-18


def poison(shape):
    return np.full(shape, POISON, np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ld_for(cols, variant):
    """Leading dimension of a cols-wide operand: 'packed' cols; 'even' / 'odd' the next
    even / odd number above cols (so a poisoned gap follows every row)."""
    if variant == "packed":
        return max(cols, 1)
    ld = cols + 1
    if (ld & 1) != (variant == "odd"):
        ld += 1
    return ld


class Desc:
    """A batch of rows x cols matrices inside buf's flat array (ld, stride, offset)."""

    def __init__(self, buf, offset, rows, cols):
        self.buf, self.offset, self.rows, self.cols = buf, offset, rows, cols
        self.ld, self.stride, self.batch = buf.ld, buf.stride, buf.batch

    def last(self):
        if self.rows <= 0 or self.cols <= 0:
            return self.offset - 1
        return self.offset + (self.batch - 1) * self.stride + (self.rows - 1) * self.ld + self.cols - 1


class Buf:
    """mats (batch, rows, cols) laid out at leading dimension ld, stride apart, behind a
    band of >= 128 * ld poisoned doubles (and before another); shift = 1 moves the first
    element one double past a 16-byte boundary (the band is even, device allocations are
    16-byte aligned).  mats may itself hold POISON where nothing may be read."""

    def __init__(self, mats, ld=None, stride=None, shift=0):
        mats = np.asarray(mats, np.float64)
        assert mats.ndim == 3
        self.batch, self.rows, self.cols = mats.shape
        self.ld = int(ld) if ld is not None else max(self.cols, 1)
        assert self.ld >= max(self.cols, 1)
        self.stride = int(stride) if stride is not None else self.rows * self.ld
        assert self.batch == 1 or self.stride >= self.rows * self.ld, "batch members must not overlap"
        band = 128 * self.ld
        band += band & 1
        self.offset = band + int(shift)
        self.size = self.offset + (self.batch - 1) * self.stride + self.rows * self.ld + band
        b, r, c = np.meshgrid(np.arange(self.batch), np.arange(self.rows), np.arange(self.cols), indexing="ij")
        self.idx = (self.offset + b * self.stride + r * self.ld + c).astype(np.int64)
        self.mats = mats
        self.flat = poison(self.size)
        self.flat[self.idx] = mats

    def desc(self):
        return self.sub(0, 0, self.rows, self.cols)

    def sub(self, r, c, rows, cols):
        assert r + rows <= self.rows and c + cols <= self.cols
        return Desc(self, self.offset + r * self.ld + c, rows, cols)

    def get(self, flat):
        return np.asarray(flat)[self.idx]

    def with_values(self, mats, written):
        """The flat image after an operation that wrote mats[written] and nothing else."""
        out = self.flat.copy()
        out[self.idx[written]] = np.asarray(mats, np.float64)[written]
        return out


class Out:
    """What an operation must leave in buf: want[written] (float64: exact check; bound
    given: longdouble reference and elementwise bound) and every other bit unchanged."""

    def __init__(self, buf, written, want, bound=None, checked=None):
        self.buf, self.written, self.want, self.bound = buf, written, want, bound
        # the written elements whose value is compared (a row sample where the longdouble
        # reference of the whole product would take seconds); default: all of them
        self.checked = written if checked is None else (checked & written)


class Case:
    def __init__(self, op, M, N, K, batch=1, A=None, B=None, C=None, D=None, alpha=1.0, beta=0.0, flags=0, p0=0,
                 p1=0, outs=(), ins=(), tag=""):
        self.op, self.M, self.N, self.K, self.batch = op, M, N, K, batch
        self.A, self.B, self.C, self.D = A, B, C, D
        self.alpha, self.beta, self.flags, self.p0, self.p1 = alpha, beta, flags, p0, p1
        self.outs, self.ins, self.tag = list(outs), list(ins), tag

    def bufs(self):
        seen = {}
        for d in (self.A, self.B, self.C, self.D):
            if d is not None:
                seen[id(d.buf)] = d.buf
        return list(seen.values())

    def verify(self, after):
        """after: {id(buf): flat array after the operation}.  Returns the list of
        violations (empty: pass)."""
        bad = []
        for o in self.outs:
            bad += check_untouched(o.buf, after[id(o.buf)], o.written, "output")
            bad += check_values(o.buf.get(after[id(o.buf)]), o.want, o.checked, o.bound)
        outs = {id(o.buf) for o in self.outs}
        for b in self.ins:
            assert id(b) not in outs
            bad += check_untouched(b, after[id(b)], None, "input")
        return [f"{self.tag}: {m}" for m in bad]


def check_untouched(buf, after, written, what):
    """Every element outside written (band, gaps, unwritten matrix elements) keeps its bits."""
    after = np.asarray(after, np.float64)
    if after.shape != buf.flat.shape:
        return [f"{what} buffer changed size"]
    keep = np.ones(buf.size, bool)
    if written is not None:
        keep[buf.idx[written]] = False
    diff = np.nonzero((bits(after) != bits(buf.flat)) & keep)[0]
    if diff.size == 0:
        return []
    i = int(diff[0])
    end = buf.offset + (buf.batch - 1) * buf.stride + buf.rows * buf.ld
    where = "band" if i < buf.offset or i >= end else "matrix region"
    return [f"{what}: {diff.size} element(s) that must stay unchanged were written, first at flat index {i} "
            f"({where}, offset {buf.offset}, ld {buf.ld}, stride {buf.stride})"]


def check_values(got, want, written, bound=None):
    got = np.asarray(got, np.float64)
    if not np.any(written):
        return []
    if bound is None:
        ok = (got == np.asarray(want, np.float64)) | ~written   # NaN != anything: fails
        n = int(np.count_nonzero(~ok))
        if n == 0:
            return []
        i = tuple(int(x) for x in np.argwhere(~ok)[0])
        return [f"exact: {n} element(s) differ, first at {i}: got {got[i]!r}, want {float(want[i])!r}"]
    err = np.abs(got.astype(LD) - want)
    ok = (err <= bound) | ~written                             # NaN compares false: fails
    n = int(np.count_nonzero(~ok))
    if n == 0:
        return []
    i = tuple(int(x) for x in np.argwhere(~ok)[0])
    return [f"real: {n} element(s) outside the bound, first at {i}: |err| {float(err[i]):.3e} > "
            f"{float(bound[i]):.3e}"]


def worst_ratio(got, want, written, bound):
    """max |err| / bound over the written elements (a figure for reports; 0 when empty)."""
    if not np.any(written):
        return 0.0
    err = np.abs(np.asarray(got, np.float64).astype(LD) - want)[written]
    return float(np.max(err / np.maximum(bound[written], np.finfo(np.float64).tiny)))


# ---- operand generation and references -------------------------------------------------
def gen(rng, shape, real):
    if real:
        return rng.standard_normal(shape)
    return rng.integers(-3, 4, size=shape).astype(np.float64)


def unit_lower(rng, batch, n, real):
    """Unit lower-triangular (the potrf's L_cc^-1 stand-in): integer entries in {-1, 0, 1}."""
    L = rng.standard_normal((batch, n, n)) / 8 if real else rng.integers(-1, 2, size=(batch, n, n)).astype(float)
    L = np.tril(L, -1)
    return L + np.eye(n)[None]


def matmul(a, b, dt):
    """a @ b over the batch in dtype dt (float64: BLAS-free exactness is not needed, the
    integer products are exact in any order; longdouble: numpy's own loops)."""
    return np.matmul(a.astype(dt), b.astype(dt))


def T(a):
    return np.swapaxes(a, -1, -2)


def dot_bound(K, absprod, alpha=1.0, beta=0.0, absC0=None):
    b = abs(alpha) * absprod
    if absC0 is not None and beta != 0.0:
        b = b + abs(beta) * absC0
    return (2 * K + 8) * U * b


def lower_mask(batch, M, N):
    r, c = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    return np.broadcast_to(c <= r, (batch, M, N)).copy()


def _layout(cols, rows, batch, variant):
    """(ld, stride, shift) of an operand for an alignment variant:
    even  -- even ld, 16-byte-aligned base (the vector-load path)
    odd   -- odd ld (scalar loads)
    shift -- even ld, base one double past a 16-byte boundary (scalar loads)
    flip  -- even ld, odd batch stride: alternate matrices flip between the two paths
    packed -- ld = cols (no gap), aligned"""
    if variant == "flip":
        ld = ld_for(cols, "even")
        return ld, rows * ld + 1, 0
    if variant == "shift":
        return ld_for(cols, "even"), None, 1
    return ld_for(cols, variant), None, 0


def case_product(op, M, N, K, batch=1, alpha=1.0, beta=0.0, form="nt", tri_a=False, lower_c=False, tri_b=False,
                 alias=False, p0=0, variant="even", real=False, seed=0, sample_rows=None):
    """C = alpha op(A) op(B) + beta C0 for the launchers that share these semantics:
    form nt (A M x K, B N x K; ops nt, rowblock, lat0), nn (B K x N), tn (A K x M, B K x N).
    alias: C is A's buffer (K == N; in-place row-block / latency forms).
    sample_rows (real only): compare that many rows of C -- the first and last three, the
    rows around every multiple of 128, and random ones -- against the longdouble reference."""
    rng = np.random.default_rng(seed)
    shp_a = (batch, K, M) if form == "tn" else (batch, M, K)
    shp_b = (batch, N, K) if form == "nt" else (batch, K, N)
    A, B = gen(rng, shp_a, real), gen(rng, shp_b, real)
    if tri_a:
        A = np.tril(A)
    if tri_b:
        B = np.tril(B)
    C0 = A.copy() if alias else gen(rng, (batch, M, N), real)
    if alias:
        assert form == "nt" and K == N
    dt = LD if real else np.float64
    opa = T(A) if form == "tn" else A
    opb = T(B) if form == "nt" else B
    checked = None
    if real and sample_rows and sample_rows < M:
        edge = [r for m in range(0, M + 1, 128) for r in (m - 1, m, m + 1)] + [0, 1, 2, M - 3, M - 2, M - 1]
        rows = sorted({r for r in edge if 0 <= r < M} | set(rng.choice(M, sample_rows, replace=False).tolist()))
        want = np.zeros((batch, M, N), dt)
        want[:, rows] = alpha * matmul(opa[:, rows], opb, dt)
        checked = np.zeros((batch, M, N), bool)
        checked[:, rows] = True
    else:
        want = alpha * matmul(opa, opb, dt)
    if beta != 0.0:
        want = want + beta * C0.astype(dt)
    bound = dot_bound(K, np.matmul(np.abs(opa), np.abs(opb)), alpha, beta, np.abs(C0)) if real else None
    la, sa, sha = _layout(shp_a[2], shp_a[1], batch, variant)
    lb, sb, shb = _layout(shp_b[2], shp_b[1], batch, variant)
    lc, sc, shc = _layout(N, M, batch, variant)
    bA, bB = Buf(A, la, sa, sha), Buf(B, lb, sb, shb)
    bC = bA if alias else Buf(C0, lc, sc, shc)
    written = lower_mask(batch, M, N) if lower_c else np.ones((batch, M, N), bool)
    flags = (1 if tri_a else 0) | (2 if lower_c else 0) | (4 if tri_b else 0)
    tag = (f"{op} {M}x{N}x{K} b{batch} alpha {alpha} beta {beta} flags {flags} p0 {p0} {variant}"
           f"{' alias' if alias else ''}{' real' if real else ''}")
    return Case(op, M, N, K, batch, bA.desc(), bB.desc(), bC.desc(), None, alpha, beta, flags, p0, 0,
                outs=[Out(bC, written, want, bound, checked)], ins=[bB] if alias else [bA, bB], tag=tag)


def case_lat1(M, K, batch=1, alpha=1.0, beta=0.0, variant="even", real=False, seed=0):
    """lower C = alpha A A^T + beta C0 (launch_gemm_lat mode 1)."""
    rng = np.random.default_rng(seed)
    A, C0 = gen(rng, (batch, M, K), real), gen(rng, (batch, M, M), real)
    dt = LD if real else np.float64
    want = alpha * matmul(A, T(A), dt)
    if beta != 0.0:
        want = want + beta * C0.astype(dt)
    bound = dot_bound(K, np.matmul(np.abs(A), np.abs(T(A))), alpha, beta, np.abs(C0)) if real else None
    bA, bC = Buf(A, *_layout(K, M, batch, variant)), Buf(C0, *_layout(M, M, batch, variant))
    tag = f"lat1 {M}x{M}x{K} b{batch} alpha {alpha} beta {beta} {variant}{' real' if real else ''}"
    return Case("lat1", M, M, K, batch, bA.desc(), None, bC.desc(), None, alpha, beta, 0, 0, 0,
                outs=[Out(bC, lower_mask(batch, M, M), want, bound)], ins=[bA], tag=tag)


def case_syrk_diag(w, K, ks, batch=3, variant="even", real=False, seed=0):
    """The potrf's diagonal-block update inside one matrix per batch member: rows of
    [A (w x K) | C (w x w)], lower C -= A A^T; C's strict upper triangle is poisoned."""
    rng = np.random.default_rng(seed)
    A, C0 = gen(rng, (batch, w, K), real), gen(rng, (batch, w, w), real)
    low = lower_mask(batch, w, w)
    mat = np.concatenate([A, np.where(low, C0, poison(C0.shape))], axis=2)
    dt = LD if real else np.float64
    want = np.concatenate([A.astype(dt), C0.astype(dt) - matmul(A, T(A), dt)], axis=2)
    bound = None
    if real:
        bound = np.concatenate([np.zeros(A.shape), dot_bound(K, np.matmul(np.abs(A), np.abs(T(A))), 1.0, 1.0,
                                                              np.abs(C0))], axis=2)
    buf = Buf(mat, *_layout(K + w, w, batch, variant))
    written = np.concatenate([np.zeros(A.shape, bool), low], axis=2)
    tag = f"syrk_diag w {w} K {K} ks {ks} b{batch} {variant}{' real' if real else ''}"
    return Case("syrk_diag", w, w, K, batch, buf.sub(0, 0, w, K), None, buf.sub(0, K, w, w), None, -1.0, 1.0, 0, ks,
                0, outs=[Out(buf, written, want, bound)], tag=tag)


def case_updsolve(M, K, wn, batch=8, variant="even", real=False, seed=0):
    """The potrf's fused update + panel solve, laid out as launch_potrf_batched128 lays it
    out inside one matrix per batch member (block column c = K, width 128):
        rows 0..127   : B = L[c:c+128, 0:K]            (the diagonal block's left columns)
        rows 128..    : A = L[c+128:, 0:K] | C (M x 128) | D (next diagonal block, wn x wn lower)
    X = (C - A B^T) Linv^T overwrites C; wn > 0: D -= [A | X][0:wn] [A | X][0:wn]^T (lower).
    Everything else in the matrix is poisoned.
    real bound: Y^ = fl(C - A B^T) has |dY| <= e_Y = (2K + 8) u (|C| + |A| |B|^T);
    X^ = fl(Y^ Linv^T) has |dX| <= e_X = (e_Y + (2 * 128 + 8) u (|Y| + e_Y)) |Linv|^T;
    with R = [A | X], D^ has |dD| <= e_X' |R|^T + |R| e_X'^T + e_X' e_X'^T
    + (2 (K + 128) + 8) u (|D| + (|R| + e_X') (|R| + e_X')^T), e_X' = [0 | e_X]."""
    rng = np.random.default_rng(seed)
    BT = 128
    A, B = gen(rng, (batch, M, K), real), gen(rng, (batch, BT, K), real)
    C0, D0 = gen(rng, (batch, M, BT), real), gen(rng, (batch, wn, wn), real)
    Li = unit_lower(rng, batch, BT, real)
    dt = LD if real else np.float64
    Y = C0.astype(dt) - matmul(A, T(B), dt)
    X = np.matmul(Y, T(Li).astype(dt))
    R = np.concatenate([A.astype(dt), X], axis=2)[:, :wn]
    D = D0.astype(dt) - np.matmul(R, T(R))
    ncol = K + BT + BT
    mat = poison((batch, BT + M, ncol))
    want = np.zeros(mat.shape, dt)
    written = np.zeros(mat.shape, bool)
    mat[:, :BT, :K] = B
    mat[:, BT:, :K] = A
    mat[:, BT:, K:K + BT] = C0
    low = lower_mask(batch, wn, wn)
    dview = mat[:, BT:BT + wn, K + BT:K + BT + wn]
    dview[low] = D0[low]
    want[:, BT:, K:K + BT] = X
    written[:, BT:, K:K + BT] = True
    want[:, BT:BT + wn, K + BT:K + BT + wn] = D
    written[:, BT:BT + wn, K + BT:K + BT + wn] = low
    bound = None
    if real:
        f = np.float64
        eY = (2 * K + 8) * U * (np.abs(C0) + np.matmul(np.abs(A), np.abs(T(B))))
        eX = np.matmul(eY + (2 * BT + 8) * U * (np.abs(Y).astype(f) + eY), np.abs(T(Li)))
        aR = np.abs(R).astype(f)
        eR = np.concatenate([np.zeros(A.shape), eX], axis=2)[:, :wn]
        eD = (np.matmul(eR, T(aR)) + np.matmul(aR, T(eR)) + np.matmul(eR, T(eR)) +
              (2 * (K + BT) + 8) * U * (np.abs(D0) + np.matmul(aR + eR, T(aR + eR))))
        bound = np.zeros(mat.shape)
        bound[:, BT:, K:K + BT] = eX
        bound[:, BT:BT + wn, K + BT:K + BT + wn] = eD
    buf = Buf(mat, *_layout(ncol, BT + M, batch, variant))
    bL = Buf(Li, BT, BT * BT, 0)
    tag = f"updsolve M {M} K {K} wn {wn} b{batch} {variant}{' real' if real else ''}"
    return Case("updsolve", M, BT, K, batch, buf.sub(BT, 0, M, K), buf.sub(0, 0, BT, K),
                buf.sub(BT, K, M, BT + wn), bL.desc(), 1.0, 1.0, 0, wn, 0,
                outs=[Out(buf, written, want, bound)], ins=[bL], tag=tag)


def sumsq_rows(kind, M):
    return (M + 127) // 128 if kind == 1 else (M + 63) // 64


def case_sumsq(n, P, kind, n_out=0, variant="packed", real=False, seed=0):
    """launch_gemm_sumsq (n_out = 0) / launch_gemm_sumsq_mean: v = [W; alpha^T] Ks^T with W
    (n x n) lower triangular and Ks (P x n), both packed (ld n);
    part[t][j] = sum of v[r][j]^2 over the rows r < n of row tile t (64 rows, 128 under
    kind 1), meanT = rows n.. of v.  part and meanT carry a poisoned ld gap.
    real bound: each computed v^ has |dv| <= e = (2n + 8) u (|A| |Ks|^T) (the product bound);
    a tile's sum of T <= 128 squares is a T-term fma dot product of v^ with itself, so
        |dpart| <= sum_r (2 |v| e + e^2) + (2 T + 8) u sum_r (|v| + e)^2."""
    assert variant in ("packed", "shift")
    rng = np.random.default_rng(seed)
    W = np.tril(gen(rng, (1, n, n), real))
    Wext = np.concatenate([W, gen(rng, (1, n_out, n), real)], axis=1)
    Ks = gen(rng, (1, P, n), real)
    dt = LD if real else np.float64
    v = matmul(Wext, T(Ks), dt)[0]
    tile = 128 if kind == 1 else 64
    rows = sumsq_rows(kind, n + n_out)
    part = np.zeros((1, rows, P), dt)
    for t in range(rows):
        part[0, t] = np.sum(v[t * tile:min((t + 1) * tile, n)] ** 2, axis=0)
    pb = mb = None
    if real:
        av = np.abs(v).astype(np.float64)
        e = (2 * n + 8) * U * np.matmul(np.abs(Wext), np.abs(T(Ks)))[0]
        pb = np.zeros((1, rows, P))
        for t in range(rows):
            sl = slice(t * tile, min((t + 1) * tile, n))
            pb[0, t] = np.sum(2 * av[sl] * e[sl] + e[sl] ** 2, axis=0) + \
                (2 * tile + 8) * U * np.sum((av[sl] + e[sl]) ** 2, axis=0)
        mb = e[None, n:]
    sh = 1 if variant == "shift" else 0
    bW, bK = Buf(Wext, n, None, sh), Buf(Ks, n, None, sh)
    bP = Buf(poison((1, rows, P)), ld_for(P, "even"), None, sh)
    outs = [Out(bP, np.ones((1, rows, P), bool), part, pb)]
    D = None
    if n_out:
        bM = Buf(poison((1, n_out, P)), ld_for(P, "odd"), None, 0)
        outs.append(Out(bM, np.ones((1, n_out, P), bool), v[None, n:], mb))
        D = bM.desc()
    tag = f"sumsq n {n} P {P} kind {kind} n_out {n_out} {variant}{' real' if real else ''}"
    return Case("sumsq_mean" if n_out else "sumsq", n, P, n, 1, bW.desc(), bK.desc(), bP.desc(), D, 1.0, 0.0, 0, kind,
                n_out, outs=outs, ins=[bW, bK], tag=tag)


def perfect_after(case):
    """The buffers after a correct operation (numpy float64 of the reference)."""
    after = {id(b): b.flat.copy() for b in case.bufs()}
    for o in case.outs:
        after[id(o.buf)] = o.buf.with_values(np.asarray(o.want, np.float64), o.written)
    return after
