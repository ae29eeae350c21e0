"""The GEMM checker (tests/gemm_check.py) rejects subtly wrong results and accepts
numpy's own float64 product -- the evidence that tests/test_gpu_gemm.py would fail for
a subtly wrong kernel.  No GPU: every "kernel result" here is built in numpy."""
import numpy as np
import pytest

import gemm_check as gc

real = pytest.mark.skipif(not gc.longdouble_ok(), reason="numpy longdouble is no finer than float64 here")


def after_with(case, got, out=0):
    """Buffers after an operation that wrote got (over the written mask) into output out
    and the reference everywhere else."""
    after = gc.perfect_after(case)
    o = case.outs[out]
    after[id(o.buf)] = o.buf.with_values(np.asarray(got, np.float64), o.written)
    return after


def f64_product(case, A=None, B=None, K=None):
    """alpha A B^T + beta C0 of an NT case in plain float64 (numpy's own product)."""
    A = case.A.buf.mats if A is None else A
    B = case.B.buf.mats if B is None else B
    p = case.alpha * np.matmul(A, gc.T(B))
    return p + case.beta * case.C.buf.mats if case.beta != 0.0 else p


def test_longdouble_reference_is_finer_than_fp64():
    if not gc.longdouble_ok():
        pytest.skip("numpy longdouble is no finer than float64 here")
    assert float(np.finfo(np.longdouble).eps) < 1e-18


def test_integer_reference_is_exact():
    """float64 numpy equals int64 arithmetic at the largest product of the GPU suite."""
    rng = np.random.default_rng(0)
    A, B = rng.integers(-3, 4, size=(770, 520)), rng.integers(-3, 4, size=(769, 520))
    assert np.array_equal(A.astype(np.float64) @ B.T.astype(np.float64), (A @ B.T).astype(np.float64))
    assert 9 * 1100 * 2 < 2 ** 53 and 128 * (9 * 1100) ** 2 < 2 ** 53


@pytest.mark.parametrize("builder", [
    lambda r: gc.case_product("nt", 63, 65, 17, batch=2, alpha=2.0, beta=0.5, real=r, variant="odd"),
    lambda r: gc.case_product("nt", 130, 130, 40, batch=3, alpha=-1.0, beta=1.0, lower_c=True, real=r,
                              variant="flip"),
    lambda r: gc.case_product("nn", 65, 63, 17, alpha=0.5, beta=-1.0, form="nn", real=r),
    lambda r: gc.case_product("tn", 65, 63, 17, alpha=-1.0, beta=1.0, form="tn", real=r, variant="shift"),
    lambda r: gc.case_product("lat0", 17, 128, 128, alias=True, tri_b=True, real=r),
    lambda r: gc.case_lat1(33, 127, batch=2, alpha=-1.0, beta=1.0, real=r),
    lambda r: gc.case_syrk_diag(17, 100, 3, real=r),
    lambda r: gc.case_updsolve(200, 128, 72, real=r),
    lambda r: gc.case_sumsq(130, 20, 1, n_out=3, real=r),
    lambda r: gc.case_sumsq(65, 65, 0, real=r, variant="shift"),
])
@pytest.mark.parametrize("is_real", [False, pytest.param(True, marks=real)])
def test_reference_result_is_accepted(builder, is_real):
    """Every builder's own reference, rounded to float64, passes its own check."""
    case = builder(is_real)
    assert case.verify(gc.perfect_after(case)) == []


@real
@pytest.mark.parametrize("shape", [(63, 65, 17), (300, 257, 260), (32, 33, 1100)])
def test_numpy_float64_product_is_accepted(shape):
    """numpy's own float64 product sits far inside the real-valued bound."""
    case = gc.case_product("nt", *shape, alpha=-1.0, beta=0.5, real=True)
    got = f64_product(case)
    assert case.verify(after_with(case, got)) == []
    o = case.outs[0]
    assert gc.worst_ratio(got, o.want, o.written, o.bound) < 0.1


@real
def test_numpy_float64_composites_are_accepted():
    """The composite bounds (SUMSQ, fused update + solve) hold for plain float64 numpy."""
    case = gc.case_sumsq(300, 20, 2, n_out=3, real=True)
    W, Ks = case.A.buf.mats[0], case.B.buf.mats[0]
    v = W @ Ks.T
    part = np.stack([np.sum(v[t * 64:min((t + 1) * 64, 300)] ** 2, axis=0) for t in range(5)])[None]
    after = after_with(case, part, 0)
    after[id(case.outs[1].buf)] = case.outs[1].buf.with_values(v[None, 300:], case.outs[1].written)
    assert case.verify(after) == []
    case = gc.case_updsolve(200, 128, 72, real=True)
    m, Li = case.A.buf.mats, case.D.buf.mats
    A, B, C0 = m[:, 128:, :128], m[:, :128, :128], m[:, 128:, 128:256]
    X = np.matmul(C0 - np.matmul(A, gc.T(B)), gc.T(Li))
    R = np.concatenate([A, X], axis=2)[:, :72]
    got = np.zeros(m.shape)
    got[:, 128:, 128:256] = X
    with np.errstate(invalid="ignore"):
        got[:, 128:200, 256:328] = m[:, 128:200, 256:328] - np.matmul(R, gc.T(R))
    assert case.verify(after_with(case, got)) == []


@pytest.mark.parametrize("is_real", [False, pytest.param(True, marks=real)])
def test_one_dropped_k_term_is_rejected(is_real):
    case = gc.case_product("nt", 63, 65, 17, alpha=2.0, beta=1.0, real=is_real)
    A, B = case.A.buf.mats, case.B.buf.mats
    got = f64_product(case)
    assert case.verify(after_with(case, got)) == []
    i, j = 40, 64
    k = int(np.argmax(np.abs(A[0, i] * B[0, j]) > 0)) if not is_real else 5
    assert A[0, i, k] * B[0, j, k] != 0
    got[0, i, j] -= case.alpha * A[0, i, k] * B[0, j, k]
    bad = case.verify(after_with(case, got))
    assert len(bad) == 1 and "1 element(s)" in bad[0] and "(0, 40, 64)" in bad[0]


@pytest.mark.parametrize("is_real", [False, pytest.param(True, marks=real)])
def test_ragged_last_column_from_the_neighbouring_tile_is_rejected(is_real):
    """N = 65: column 64 is the second tile's only live column; a mis-masked edge that
    serves it from the first tile's last column must fail."""
    case = gc.case_product("nt", 63, 65, 17, alpha=1.0, beta=0.0, real=is_real)
    got = f64_product(case)
    got[:, :, 64] = got[:, :, 63]
    bad = case.verify(after_with(case, got))
    assert len(bad) == 1 and ", 64)" in bad[0]


@pytest.mark.parametrize("tail", [1, 2, 7, 15])
@pytest.mark.parametrize("is_real", [False, pytest.param(True, marks=real)])
def test_omitted_last_k_step_is_rejected(tail, is_real):
    K = 32 + tail
    case = gc.case_product("nt", 65, 63, K, alpha=-1.0, beta=1.0, real=is_real)
    A, B = case.A.buf.mats, case.B.buf.mats
    got = f64_product(case, A[:, :, :32], B[:, :, :32])
    assert case.verify(after_with(case, got)) != []


@real
def test_fp32_accumulation_is_rejected_only_by_the_real_check():
    """The integer operands are exact in fp32 as well: an fp32-accumulated product passes
    the exact check and must fail the real-valued one (far outside: ~1e6 x the bound)."""
    ci = gc.case_product("nt", 65, 63, 300, alpha=1.0, beta=0.0)
    A, B = ci.A.buf.mats.astype(np.float32), ci.B.buf.mats.astype(np.float32)
    assert ci.verify(after_with(ci, np.matmul(A, gc.T(B)).astype(np.float64))) == []
    cr = gc.case_product("nt", 65, 63, 300, alpha=1.0, beta=0.0, real=True)
    A, B = cr.A.buf.mats.astype(np.float32), cr.B.buf.mats.astype(np.float32)
    got = np.matmul(A, gc.T(B)).astype(np.float64)
    assert cr.verify(after_with(cr, got)) != []
    o = cr.outs[0]
    assert gc.worst_ratio(got, o.want, o.written, o.bound) > 1e4


def test_element_above_the_diagonal_is_rejected():
    case = gc.case_product("nt", 130, 130, 40, batch=3, alpha=-1.0, beta=1.0, lower_c=True)
    after = gc.perfect_after(case)
    assert case.verify(after) == []
    buf = case.C.buf
    # the value a kernel without the col <= row test would have stored there
    full = f64_product(case)
    i = next(r for r in range(64, 129) if full[1, r, r + 1] != buf.mats[1, r, r + 1])
    after[id(buf)][buf.idx[1, i, i + 1]] = full[1, i, i + 1]
    bad = case.verify(after)
    assert len(bad) == 1 and "must stay unchanged" in bad[0] and "matrix region" in bad[0]


@pytest.mark.parametrize("where", ["before", "after", "gap", "row_past_m", "input_band"])
def test_guard_band_element_is_rejected(where):
    case = gc.case_product("nt", 63, 65, 17, batch=2, alpha=1.0, beta=0.0)
    after = gc.perfect_after(case)
    buf = case.C.buf if where != "input_band" else case.B.buf
    flat = after[id(buf)]
    i = {"before": buf.offset - 1, "after": buf.size - 1, "gap": buf.offset + buf.cols,
         "row_past_m": buf.offset + (buf.batch - 1) * buf.stride + buf.rows * buf.ld,
         "input_band": 0}[where]
    assert gc.bits(flat)[i] == gc.POISON
    flat[i] = 0.0
    bad = case.verify(after)
    assert len(bad) == 1 and "must stay unchanged" in bad[0]
    # a NaN of another bit pattern is a write too
    flat[i] = np.nan
    assert len(case.verify(after)) == 1


@pytest.mark.parametrize("is_real", [False, pytest.param(True, marks=real)])
def test_nan_from_a_poisoned_read_is_rejected(is_real):
    case = gc.case_product("nt", 63, 65, 17, alpha=1.0, beta=0.0, real=is_real)
    got = f64_product(case)
    got[0, 62, 64] = gc.poison(1)[0]
    assert len(case.verify(after_with(case, got))) == 1


def test_composite_mutations_are_rejected():
    """One wrong element in each composite output: a SUMSQ tile that sums one row of the
    next tile, a mean row taken from the wrong alpha row, a diagonal-block update that
    misses its last K split, a fused step whose look-ahead block is not updated."""
    case = gc.case_sumsq(130, 20, 0, n_out=3)
    v = case.A.buf.mats[0] @ case.B.buf.mats[0].T
    part = np.asarray(case.outs[0].want, np.float64).copy()
    part[0, 0] += v[64] ** 2
    assert len(case.verify(after_with(case, part, 0))) == 1
    mean = np.asarray(case.outs[1].want, np.float64).copy()
    mean[0, 1] = mean[0, 2]
    assert len(case.verify(after_with(case, mean, 1))) == 1
    case = gc.case_syrk_diag(17, 100, 3)
    A = case.A.buf.mats[:, :, :100]
    got = np.asarray(case.outs[0].want, np.float64).copy()
    got[:, :, 100:] += np.matmul(A[:, :, 96:], gc.T(A[:, :, 96:]))
    assert len(case.verify(after_with(case, got))) == 1
    case = gc.case_updsolve(200, 128, 72)
    got = np.asarray(case.outs[0].want, np.float64).copy()
    with np.errstate(invalid="ignore"):
        got[:, 128:200, 256:328] = case.C.buf.mats[:, 128:200, 256:328]
    assert len(case.verify(after_with(case, got))) == 1


def test_wrapper_extents_match_the_layouts():
    """_lib.GemmOperand computes the furthest element as the layouts here do, and the
    wrapper's table of touched extents covers every operand of every builder."""
    from gp_mpc_rocket_landing_amd import _lib
    cases = [gc.case_product("nt", 130, 70, 300, batch=3, variant="flip"),
             gc.case_product("tn", 65, 63, 17, form="tn"), gc.case_product("nn_batched", 65, 63, 17, batch=3, form="nn"),
             gc.case_lat1(33, 127, batch=2), gc.case_syrk_diag(17, 100, 3), gc.case_updsolve(200, 128, 72),
             gc.case_updsolve(128, 0, 0), gc.case_sumsq(130, 20, 1, n_out=3), gc.case_sumsq(65, 65, 2)]
    for c in cases:
        ext = _lib._gemm_extents(_lib.GEMM_OP[c.op], c.M, c.N, c.K, c.p0, c.p1)
        for name in "ABCD":
            d = getattr(c, name)
            if ext[name] is None:
                continue
            assert d is not None and d.rows >= ext[name][0] and d.cols >= ext[name][1], (c.tag, name)
            g = _lib.GemmOperand(None, d.offset, d.rows, d.cols, d.ld, d.stride, d.batch)
            assert g.last() == d.last() < d.buf.size
