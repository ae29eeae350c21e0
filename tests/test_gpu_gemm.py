"""Every kernel path of the FP64 MFMA GEMM family (csrc/gemm.hip, csrc/mma128.h) called
directly through gpmpc_gemm_diag and compared with an exact reference (tests/gemm_check.py:
integer operands, tolerance zero; one ragged case per path also with standard normal
operands against a longdouble reference, elementwise (2K + 8) u bound).  Every buffer
carries poisoned guard bands and ld gaps that must come back bit-unchanged, and every case
meant for a path asserts the path the launcher reports.

Argument combinations follow what the callers in csrc/ produce or csrc/gemm.h promises:
tri_a only with beta != 1 (nothing accumulates a triangular product, so it never meets
the K split), K split of the row-block form only with beta = 1, the SUMSQ operands
packed (ld n), the fused update + solve in the potrf's in-matrix layout.

Run as a script (``python tests/test_gpu_gemm.py NAME``) it is the child process of
test_switch_forced_paths: the environment switches are read once per process."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_check as gc  # noqa: E402

pytestmark = pytest.mark.gpu
S = gc.SCALARS
PLANNED = ("nt", "nn", "nn_batched", "tn", "rowblock", "sumsq", "sumsq_mean")   # the launchers with a decision


def ab(i):
    """A deterministic walk over the (alpha, beta) pairs of {0, 1, -1, 2, 0.5}^2."""
    return S[(3 * i + 1) % 5], S[(i + i // 5) % 5]


def run_case(ctx, case, path=None, split=None, grid=None, report=None):
    """Upload the case's buffers, launch, download, verify.  Returns the violations."""
    import torch
    from gp_mpc_rocket_landing_amd import _lib
    tens = {id(b): torch.from_numpy(b.flat.copy()).cuda() for b in case.bufs()}
    assert all(t.data_ptr() % 16 == 0 for t in tens.values())

    def op(d):
        if d is None:
            return None
        return _lib.GemmOperand(tens[id(d.buf)], d.offset, d.rows, d.cols, d.ld, d.stride, d.batch)

    torch.cuda.synchronize()
    got = _lib.gemm_diag(ctx, case.op, case.M, case.N, case.K, op(case.A), op(case.B), op(case.C), op(case.D),
                         case.alpha, case.beta, case.flags, case.p0, case.p1, case.batch)
    ctx.sync()
    after = {k: t.cpu().numpy() for k, t in tens.items()}
    bad = case.verify(after)
    for name, want, have in (("path", path, got[0]), ("split", split, got[1]), ("grid", grid, got[2])):
        if want is not None and want != have:
            bad.append(f"{case.tag}: {name} {have!r}, meant for {want!r}")
    if case.op in PLANNED:   # what ran is what the plan says, under this process's switches
        plan = _lib.gemm_plan(case.op, case.M, case.N, case.K, case.batch, case.beta, case.flags, case.p0, case.p1)
        if plan[:3] != got:
            bad.append(f"{case.tag}: ran {got!r}, the plan is {plan!r}")
    if report is not None:
        for o in case.outs:
            if o.bound is not None:
                report.append((case.tag, got[0], gc.worst_ratio(o.buf.get(after[id(o.buf)]), o.want, o.checked,
                                                                o.bound)))
    return bad


def run_all(ctx, specs):
    """specs: (case, path, split, grid) tuples (None: not asserted)."""
    bad, report = [], []
    for spec in specs:
        case, want = spec[0], (tuple(spec[1:]) + (None, None, None))[:3]
        if any(o.bound is not None for o in case.outs) and not gc.longdouble_ok():
            continue  # the real-valued check needs a longdouble finer than fp64
        bad += run_case(ctx, case, *want, report=report)
    for tag, path, ratio in report:
        print(f"real {tag} [{path}]: max |err| / bound = {ratio:.3g}")
    assert not bad, "\n".join(bad[:20])


def test_real_reference_available():
    if not gc.longdouble_ok():
        pytest.skip("numpy longdouble is no finer than float64: the real-valued cases are left out")
    assert gc.longdouble_ok()


# ---- general NT products ---------------------------------------------------------------
def P(*a, **k):
    return gc.case_product("nt", *a, **k)


def test_nt_64_tile(gpu_ctx):
    specs = []
    for i, shp in enumerate([(1, 1, 1), (63, 65, 17), (64, 64, 16), (65, 63, 15)]):
        for j in range(3):
            a, b = ab(5 * i + j)
            specs.append((P(*shp, alpha=a, beta=b, seed=i), "64", 1, "2d"))
    specs += [(P(100, 130, 0, alpha=2.0, beta=0.5), "64"), (P(100, 130, 0, alpha=2.0, beta=0.0), "64"),
              (P(100, 130, 0, alpha=1.0, beta=1.0, batch=3), "64"),
              (P(130, 70, 300, batch=3, alpha=-1.0, beta=0.5, variant="flip"), "64", 1, "2d"),
              (P(130, 70, 300, batch=3, alpha=2.0, beta=0.0, variant="odd"), "64", 1, "2d"),
              (P(63, 65, 17, alpha=-1.0, beta=0.5, real=True), "64"),
              (P(130, 70, 300, batch=3, alpha=2.0, beta=1.0, variant="flip", real=True), "64")]
    run_all(gpu_ctx, specs)


def test_nt_64_tile_lower(gpu_ctx):
    """M = N = 130, K = 40: the 1-D triangular grid (batch 3), the XCD-batched grid (batch
    8) and the XCD-batched grid with padding workgroups (batch 11)."""
    specs = []
    for batch, grid in ((3, "tri"), (8, "xcd_batch"), (11, "xcd_batch")):
        for j, (a, b) in enumerate(((-1.0, 1.0), (2.0, 0.0), (0.5, 0.5))):
            specs.append((P(130, 130, 40, batch=batch, alpha=a, beta=b, lower_c=True, seed=batch + j), "64", 1, grid))
    specs.append((P(130, 130, 40, batch=11, alpha=-1.0, beta=1.0, lower_c=True, real=True), "64", 1, "xcd_batch"))
    # M != N under lower_c (the potrf's panel update): the general 2-D grid
    specs.append((P(130, 64, 40, batch=3, alpha=-1.0, beta=1.0, lower_c=True), "64", 1, "2d"))
    run_all(gpu_ctx, specs)


def test_nt_128_tile(gpu_ctx):
    run_all(gpu_ctx, [
        (P(256, 256, 256, alpha=1.0, beta=0.0), "128", 1, "2d"),
        (P(300, 257, 260, alpha=-1.0, beta=0.5), "128", 1, "2d"),
        (P(300, 257, 260, alpha=2.0, beta=0.5, real=True), "128", 1, "2d"),
        (P(385, 383, 271, batch=2, alpha=0.5, beta=-1.0), "128", 1, "2d"),
        (P(385, 383, 271, batch=2, alpha=1.0, beta=2.0, variant="flip"), "128", 1, "2d"),
    ])


def test_nt_128_tile_k_split(gpu_ctx):
    """K = 1100, beta = 1: the cost model of launch_gemm_impl splits K in 4 (atomic adds)."""
    run_all(gpu_ctx, [
        (P(300, 300, 1100, alpha=-1.0, beta=1.0), "128_ksplit", 4, "2d"),
        (P(300, 300, 1100, alpha=2.0, beta=1.0, lower_c=True), "128_ksplit", 4, "tri"),
        (P(300, 300, 1100, alpha=-1.0, beta=1.0, lower_c=True, variant="odd"), "128_ksplit", 4, "tri"),
        (P(300, 300, 1100, alpha=-1.0, beta=1.0, real=True, sample_rows=24), "128_ksplit", 4, "2d"),
        # beta != 1 keeps one pass over K
        (P(300, 300, 1100, alpha=-1.0, beta=0.5), "128", 1, "2d"),
    ])


def test_nt_stream_k(gpu_ctx):
    run_all(gpu_ctx, [
        (P(770, 769, 520, alpha=-1.0, beta=1.0), "streamk", 512, "2d"),
        (P(770, 770, 520, batch=2, alpha=0.5, beta=1.0, lower_c=True), "streamk", 512, "tri"),
        (P(770, 769, 520, alpha=2.0, beta=1.0, variant="odd", real=True, sample_rows=24), "streamk", 512, "2d"),
    ])


def test_nt_skinny_split_k(gpu_ctx):
    specs = []
    for i, shp in enumerate([(3, 700, 1000), (700, 3, 1000), (32, 33, 257)]):
        for j, (a, b) in enumerate(((1.0, 0.0), (-1.0, 1.0), (2.0, 0.5))):
            specs.append((P(*shp, alpha=a, beta=b, seed=3 * i + j), "splitk"))
    specs += [(P(32, 33, 257, alpha=-1.0, beta=0.5, real=True), "splitk", 4),
              (P(3, 700, 1000, alpha=1.0, beta=0.0, variant="odd"), "splitk"),
              (P(700, 3, 1000, alpha=1.0, beta=1.0, variant="shift"), "splitk"),
              # not skinny enough, too short, batched: the one-pass kernel
              (P(33, 33, 257, alpha=1.0, beta=0.0), "64"), (P(32, 33, 255, alpha=1.0, beta=0.0), "64"),
              (P(32, 33, 257, batch=2, alpha=1.0, beta=0.0), "64")]
    run_all(gpu_ctx, specs)


def test_nt_triangular_a(gpu_ctx):
    """A square lower-triangular A with K == M (W = L^-1 as the left operand), below and
    above the 128-tile threshold; the entries above A's diagonal are zeros, its ld gap is
    poisoned."""
    run_all(gpu_ctx, [
        (P(130, 70, 130, alpha=1.0, beta=0.0, tri_a=True), "64"),
        (P(130, 70, 130, alpha=-1.0, beta=0.5, tri_a=True, variant="odd"), "64"),
        (P(300, 260, 300, alpha=1.0, beta=0.0, tri_a=True), "128"),
        (P(300, 260, 300, alpha=2.0, beta=0.5, tri_a=True, variant="shift"), "128"),
        (P(300, 260, 300, alpha=1.0, beta=0.0, tri_a=True, real=True), "128"),
        (P(130, 70, 130, alpha=1.0, beta=0.0, tri_a=True, real=True), "64"),
    ])


def test_nt_alignment(gpu_ctx):
    """The 16-byte vector loads against the scalar loads: even ld on an aligned base, odd
    ld, a base one double past a 16-byte boundary, and an odd batch stride over an even ld
    (alternate matrices flip between the two), for one ragged shape per NT kernel."""
    specs = []
    for variant in ("even", "odd", "shift", "flip"):
        specs += [(P(65, 63, 15, batch=3, alpha=-1.0, beta=0.5, variant=variant), "64", 1, "2d"),
                  (P(130, 130, 40, batch=3, alpha=-1.0, beta=1.0, lower_c=True, variant=variant), "64", 1, "tri"),
                  (P(130, 130, 40, batch=11, alpha=2.0, beta=1.0, lower_c=True, variant=variant), "64", 1,
                   "xcd_batch"),
                  (P(300, 257, 260, batch=2, alpha=2.0, beta=0.5, variant=variant), "128", 1, "2d")]
    for variant in ("odd", "shift"):
        specs += [(P(32, 33, 257, alpha=-1.0, beta=1.0, variant=variant), "splitk", 4),
                  (P(300, 300, 1100, alpha=-1.0, beta=1.0, variant=variant), "128_ksplit", 4, "2d")]
    specs.append((P(770, 770, 520, batch=2, alpha=-1.0, beta=1.0, lower_c=True, variant="flip"), "streamk", 512,
                  "tri"))
    run_all(gpu_ctx, specs)


# ---- NN, TN, batched NN ----------------------------------------------------------------
@pytest.mark.parametrize("form", ["nn", "nn_batched", "tn"])
def test_nn_tn(gpu_ctx, form):
    f = form[:2]
    batch = 3 if form == "nn_batched" else 1
    skinny = (130, 3, 520) if form == "tn" else (3, 130, 520)   # launch_splitk forms 2 and 1
    specs = []
    for i, shp in enumerate([(65, 63, 17), (129, 258, 128), skinny]):
        path = "splitk" if shp == skinny and batch == 1 else "64"
        for j in range(2):
            a, b = ab(7 * i + 3 * j + 1)
            specs.append((gc.case_product(form, *shp, batch=batch, alpha=a, beta=b, form=f, seed=i + j), path))
        for variant in ("odd", "shift") + (("flip",) if batch > 1 else ()):
            specs.append((gc.case_product(form, *shp, batch=batch, alpha=-1.0, beta=1.0, form=f, variant=variant),
                          path))
    specs.append((gc.case_product(form, 65, 63, 17, batch=batch, alpha=-1.0, beta=0.5, form=f, real=True), "64"))
    specs.append((gc.case_product(form, *skinny, batch=batch, alpha=1.0, beta=0.5, form=f, real=True), None))
    run_all(gpu_ctx, specs)


# ---- row block --------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [3, 8, 16])
def test_rowblock(gpu_ctx, batch):
    grid = "2d" if batch == 3 else "rowblock_xcd"
    specs = []
    for i, shp in enumerate([(129, 100, 37), (300, 128, 128), (300, 128, 384)]):
        for lower in (False, True):
            a, b = ab(4 * i + lower + batch)
            specs.append((gc.case_product("rowblock", *shp, batch=batch, alpha=a, beta=b, lower_c=lower, p0=1,
                                          seed=i), "128", 1, grid))
            specs.append((gc.case_product("rowblock", *shp, batch=batch, alpha=-1.0, beta=1.0, lower_c=lower, p0=3,
                                          seed=i + 9), "128_ksplit", 3, grid))
    # the potrf's in-place panel solve: C aliases A, alpha = 1, beta = 0, K = N = 128
    specs.append((gc.case_product("rowblock", 300, 128, 128, batch=batch, alpha=1.0, beta=0.0, alias=True, p0=1),
                  "128", 1, grid))
    if batch == 3:
        for variant in ("odd", "shift", "flip"):
            specs.append((gc.case_product("rowblock", 129, 100, 37, batch=3, alpha=-1.0, beta=1.0, lower_c=True,
                                          p0=3, variant=variant), "128_ksplit", 3, grid))
            specs.append((gc.case_product("rowblock", 300, 128, 128, batch=3, alpha=1.0, beta=0.0, alias=True,
                                          p0=1, variant=variant), "128", 1, grid))
        specs.append((gc.case_product("rowblock", 129, 100, 37, batch=3, alpha=-1.0, beta=1.0, lower_c=True, p0=3,
                                      real=True), "128_ksplit", 3, grid))
        specs.append((gc.case_product("rowblock", 129, 100, 37, batch=3, alpha=2.0, beta=0.5, p0=1, real=True),
                      "128", 1, grid))
    run_all(gpu_ctx, specs)


# ---- latency form -----------------------------------------------------------------------
def test_lat_mode0(gpu_ctx):
    specs, i = [], 0
    for M in (1, 16, 17, 100):
        for N in (1, 32, 33, 128):
            for K in (1, 7, 8, 127, 128):
                a, b = ab(i)
                i += 1
                specs.append((gc.case_product("lat0", M, N, K, batch=1 + i % 2, alpha=a, beta=b, seed=i), "lat"))
    for M in (1, 17, 100):
        # the potrf's panel solve: in place, B = L_cc^-1 lower triangular, batched
        specs.append((gc.case_product("lat0", M, 128, 128, batch=8, alpha=1.0, beta=0.0, tri_b=True, alias=True,
                                      seed=M), "lat"))
        specs.append((gc.case_product("lat0", M, 33, 33, batch=2, alpha=-1.0, beta=1.0, tri_b=True, seed=M), "lat"))
        specs.append((gc.case_product("lat0", M, 1, 1, alpha=2.0, beta=0.0, alias=True, seed=M), "lat"))
    for variant in ("odd", "shift", "flip"):
        specs.append((gc.case_product("lat0", 17, 33, 127, batch=3, alpha=-1.0, beta=0.5, variant=variant), "lat"))
        specs.append((gc.case_product("lat0", 17, 128, 128, batch=3, alpha=1.0, beta=0.0, tri_b=True, alias=True,
                                      variant=variant), "lat"))
    specs.append((gc.case_product("lat0", 17, 33, 127, batch=3, alpha=-1.0, beta=0.5, real=True), "lat"))
    specs.append((gc.case_product("lat0", 100, 128, 128, batch=2, alpha=1.0, beta=0.0, tri_b=True, alias=True,
                                  real=True), "lat"))
    run_all(gpu_ctx, specs)


def test_lat_mode1(gpu_ctx):
    specs, i = [], 0
    for M in (1, 16, 17, 33, 100):
        for K in (1, 7, 8, 127, 128):
            for beta in (0.0, 1.0):
                i += 1
                specs.append((gc.case_lat1(M, K, batch=1 + i % 3, alpha=S[1 + i % 4], beta=beta, seed=i), "lat", 1,
                              "tri"))
    for variant in ("odd", "shift", "flip"):
        specs.append((gc.case_lat1(33, 127, batch=3, alpha=-1.0, beta=1.0, variant=variant), "lat"))
    specs.append((gc.case_lat1(33, 127, batch=3, alpha=-1.0, beta=1.0, real=True), "lat"))
    run_all(gpu_ctx, specs)


# ---- the potrf's diagonal-block update and fused update + solve -------------------------
def test_syrk_diag(gpu_ctx):
    specs = []
    for w in (1, 16, 17, 127, 128):
        for K in (16, 100, 384):
            for ks in (1, 3):
                specs.append((gc.case_syrk_diag(w, K, ks, batch=3, seed=w + K + ks), "syrk_diag", ks))
    for variant in ("odd", "shift", "flip"):
        for ks in (1, 3):
            specs.append((gc.case_syrk_diag(127, 100, ks, batch=3, variant=variant), "syrk_diag", ks))
    specs.append((gc.case_syrk_diag(127, 100, 3, batch=3, real=True), "syrk_diag", 3))
    specs.append((gc.case_syrk_diag(17, 384, 1, batch=3, real=True), "syrk_diag", 1))
    run_all(gpu_ctx, specs)


@pytest.mark.parametrize("M", [128, 200, 300])
def test_updsolve(gpu_ctx, M):
    specs = []
    for K in (0, 128, 256):
        for wn in (0, 72, 128):
            specs.append((gc.case_updsolve(M, K, wn, batch=8, seed=M + K + wn), "updsolve"))
    if M == 200:
        for variant in ("odd", "shift", "flip"):
            specs.append((gc.case_updsolve(200, 128, 72, batch=8, variant=variant), "updsolve"))
            specs.append((gc.case_updsolve(200, 0, 0, batch=8, variant=variant), "updsolve"))
        specs.append((gc.case_updsolve(200, 128, 72, batch=8, real=True), "updsolve"))
    if M == 128:
        specs.append((gc.case_updsolve(128, 0, 72, batch=8, real=True), "updsolve"))
        specs.append((gc.case_updsolve(128, 128, 0, batch=16), "updsolve"))
    run_all(gpu_ctx, specs)


# ---- SUMSQ epilogues --------------------------------------------------------------------
def sumsq_path(kind, n, n_out, P):
    """The kernel a forced kind runs: the K split only where launch_splitk_sumsq takes the
    product (P <= 64, K = n >= 256, >= 2 chunks), else the 64-tile kernel."""
    if kind == 1:
        return "128"
    ty = (n + n_out + 63) // 64
    if kind == 2 and P <= 64 and n >= 256 and min(512 // ty, n // 64) >= 2:
        return "splitk"
    return "64"


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n_out", [0, 3])
def test_sumsq(gpu_ctx, kind, n_out):
    """launch_gemm_sumsq (n_out 0) and launch_gemm_sumsq_mean (3 alpha rows) under every
    forced kind, including the below-threshold sizes the fleet's shrinking prefix produces
    (kind 128 at n = 130, P = 20; the K split at n = 300, P <= 64)."""
    specs = []
    for n in (1, 64, 65, 130, 300):
        for Pq in (1, 20, 64, 65, 300):
            specs.append((gc.case_sumsq(n, Pq, kind, n_out, seed=n + Pq), sumsq_path(kind, n, n_out, Pq)))
    assert sumsq_path(2, 300, n_out, 20) == "splitk" and sumsq_path(2, 300, n_out, 65) == "64"
    for n, Pq in ((65, 20), (130, 20), (300, 20), (300, 65)):
        specs.append((gc.case_sumsq(n, Pq, kind, n_out, variant="shift"), sumsq_path(kind, n, n_out, Pq)))
        specs.append((gc.case_sumsq(n, Pq, kind, n_out, real=True), sumsq_path(kind, n, n_out, Pq)))
    run_all(gpu_ctx, specs)


# ---- refusals ---------------------------------------------------------------------------
def test_diag_refuses_what_the_launchers_do_not_promise(gpu_ctx):
    """-2 and nothing launched: the buffers come back bit-unchanged."""
    import torch
    from gp_mpc_rocket_landing_amd import _lib
    bad = [
        gc.case_product("rowblock", 64, 129, 16, p0=1),                       # N > 128
        gc.case_product("rowblock", 64, 64, 64, alpha=1.0, beta=0.5, p0=3),   # K split without beta = 1
        gc.case_product("lat0", 16, 129, 16), gc.case_product("lat0", 16, 16, 129),
        gc.case_lat1(16, 129),
        gc.case_product("nt", 64, 64, 64, alpha=1.0, beta=1.0, tri_a=True),   # accumulating a triangular A
        gc.case_updsolve(128, 128, 0, batch=3),                               # batch not a multiple of 8
    ]
    for case in bad:
        tens = {id(b): torch.from_numpy(b.flat.copy()).cuda() for b in case.bufs()}

        def op(d):
            return None if d is None else _lib.GemmOperand(tens[id(d.buf)], d.offset, d.rows, d.cols, d.ld,
                                                           d.stride, d.batch)
        with pytest.raises(_lib.HIPError) as e:
            _lib.gemm_diag(gpu_ctx, case.op, case.M, case.N, case.K, op(case.A), op(case.B), op(case.C), op(case.D),
                           case.alpha, case.beta, case.flags, case.p0, case.p1, case.batch)
        assert e.value.rc == -2, case.tag
        gpu_ctx.sync()
        for b in case.bufs():
            assert np.array_equal(gc.bits(tens[id(b)].cpu().numpy()), gc.bits(b.flat)), case.tag
    # the wrapper refuses a description that reaches past its tensor, or is smaller than
    # what the operation touches, before calling into the library
    case = gc.case_product("nt", 63, 65, 17)
    tens = {id(b): torch.from_numpy(b.flat.copy()).cuda() for b in case.bufs()}
    d = case.C
    ok = [_lib.GemmOperand(tens[id(x.buf)], x.offset, x.rows, x.cols, x.ld, x.stride, x.batch)
          for x in (case.A, case.B, case.C)]
    far = _lib.GemmOperand(tens[id(d.buf)], d.buf.size - 10, d.rows, d.cols, d.ld, d.stride, d.batch)
    small = _lib.GemmOperand(tens[id(d.buf)], d.offset, d.rows - 1, d.cols, d.ld, d.stride, d.batch)
    for c in (far, small):
        with pytest.raises(ValueError):
            _lib.gemm_diag(gpu_ctx, "nt", 63, 65, 17, ok[0], ok[1], c)
    with pytest.raises(ValueError):
        _lib.gemm_diag(gpu_ctx, "nt", 63, 65, 17, ok[0], None, ok[2])


# ---- switch-forced fallback branches (child processes) ----------------------------------
def child_specs(name):
    if name == "plain_grids":   # GPMPC_SPLITK=0 GPMPC_XCD_BATCH=0 GPMPC_ROWBLOCK_XCD=0
        return [(P(3, 700, 1000, alpha=-1.0, beta=1.0), "64", 1, "2d"),
                (P(32, 33, 257, alpha=2.0, beta=0.5), "64", 1, "2d"),
                (gc.case_product("tn", 130, 3, 520, alpha=1.0, beta=0.0, form="tn"), "64"),
                (gc.case_product("nn", 3, 130, 520, alpha=1.0, beta=0.5, form="nn"), "64"),
                (P(130, 130, 40, batch=11, alpha=-1.0, beta=1.0, lower_c=True), "64", 1, "tri"),
                (gc.case_product("rowblock", 129, 100, 37, batch=8, alpha=-1.0, beta=1.0, lower_c=True, p0=3),
                 "128_ksplit", 3, "2d"),
                (gc.case_sumsq(300, 20, 2, 3), "64"), (gc.case_sumsq(300, 20, -1, 3), "64")]
    if name == "small_tiles":   # GPMPC_GEMM128=0
        return [(P(300, 257, 260, alpha=-1.0, beta=0.5), "64", 1, "2d"),
                (P(300, 300, 1100, alpha=2.0, beta=1.0, lower_c=True), "64", 1, "tri"),
                (P(300, 260, 300, alpha=1.0, beta=0.0, tri_a=True), "64"),
                (gc.case_sumsq(300, 300, -1, 3), "64"), (gc.case_sumsq(300, 300, 1, 3), "128")]
    if name == "forced_k_split":   # GPMPC_STREAMK=0 GPMPC_KSPLIT=3 GPMPC_SYRK128=1
        return [(P(300, 257, 260, alpha=-1.0, beta=1.0), "128_ksplit", 3, "2d"),
                (P(300, 300, 260, batch=2, alpha=2.0, beta=1.0, lower_c=True), "128_ksplit", 3, "tri"),
                (P(300, 300, 260, batch=2, alpha=2.0, beta=0.5, lower_c=True), "128", 1, "tri"),
                (P(130, 130, 40, batch=3, alpha=-1.0, beta=1.0, lower_c=True), "64", 1, "tri")]
    raise KeyError(name)


CHILD_ENV = {"plain_grids": {"GPMPC_SPLITK": "0", "GPMPC_XCD_BATCH": "0", "GPMPC_ROWBLOCK_XCD": "0"},
             "small_tiles": {"GPMPC_GEMM128": "0"},
             "forced_k_split": {"GPMPC_STREAMK": "0", "GPMPC_KSPLIT": "3", "GPMPC_SYRK128": "1"}}


@pytest.mark.parametrize("name", sorted(CHILD_ENV))
def test_switch_forced_paths(gpu_ctx, name):
    """The fallback branches no shape reaches in the session process (the switches are read
    once per process): skinny products and SUMSQ without the K split, the plain grids
    behind the XCD-batched ones, large products on 64-tiles, a forced K split."""
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], cwd=repo,
                       env=dict(os.environ, **CHILD_ENV[name]), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gemm child ok" in r.stdout, (name, r.stdout[-2000:], r.stderr[-3000:])


if __name__ == "__main__":
    sys.path.insert(0, os.getcwd())
    from gp_mpc_rocket_landing_amd import _lib
    child_ctx = _lib.Context(0)
    run_all(child_ctx, child_specs(sys.argv[1]))
    child_ctx.sync()
    print("gemm child ok")
