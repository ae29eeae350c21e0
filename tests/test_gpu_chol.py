"""Every path of the batched Cholesky (csrc/chol.hip), the triangular solves and the solve
helpers of csrc/gp.hip, run through gpmpc_potrf_diag / gpmpc_tri_diag in this process (the
policy is an argument, not the environment) and held to the rules of tests/chol_check.py:
the factor's elementwise backward error against a longdouble residual on well- and
ill-conditioned families, the triangular operations' residuals, and an exact integer family
at tolerance zero.  Operands sit in poisoned flat buffers (ld packed / even / odd, a gap
behind every matrix, a base one double off a 16-byte boundary); everything an operation must
not write -- the strict upper triangle included -- must come back bit-unchanged.

test_factor_coverage reads the executed plans back through gpmpc_potrf_plan and asserts that
together they contain every form, step kind and diagonal mode, so a change of defaults
cannot silently drop a path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chol_check as cc  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


def policy(sw):
    """The default policy with sw's fields replaced, in full: nothing is left to the environment."""
    return dict(_lib().POTRF_POLICY, **sw)


def run_factor(ctx, case, sw):
    """Factor the case's buffer in place under the policy; returns (flat after, info, kind)."""
    import torch
    L = _lib()
    t = torch.from_numpy(case.buf.flat.copy()).cuda()
    assert t.data_ptr() % 16 == 0
    info = torch.full((case.batch,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.potrf_diag(ctx, t, case.n, case.batch, case.buf.offset, case.buf.ld, case.buf.stride, info, **policy(sw))
    ctx.sync()
    kind = cc.plan_kind(*L.potrf_plan(case.n, case.batch, **policy(sw)))
    return t.cpu().numpy(), info.cpu().numpy(), kind


@pytest.mark.parametrize("name,sw,sizes", cc.FACTOR_RUNS, ids=[r[0] for r in cc.FACTOR_RUNS])
def test_factor(gpu_ctx, name, sw, sizes):
    bad, report = [], []
    for i, (n, batch) in enumerate(sizes):
        case = cc.factor_case(name, i, n, batch)
        after, info, kind = run_factor(gpu_ctx, case, sw)
        bad += case.verify(after, info, kind, report)
    for tag, kind, ratio, plain in report:
        print(f"factor {tag} [{kind}]: max |A - L L^T| / bound = {ratio:.3g}, / (u |L| |L^T|) = {plain:.3g}")
    assert not bad, "\n".join(bad[:20])


def test_factor_coverage():
    """What the runs of test_factor execute, from their plans: all three forms, all nine step
    kinds, the diagonal modes with and without the packed layout, both K splits of both
    update kinds, the fused step with K = 0, K > 0 and the look-ahead, K = 256 trailing."""
    L = _lib()
    plans = [L.potrf_plan(n, batch, **policy(sw)) for _, sw, sizes in cc.FACTOR_RUNS for n, batch in sizes]
    have = cc.plan_coverage(plans)
    print("covered:", sorted(have))
    assert cc.COVERAGE <= have, sorted(cc.COVERAGE - have)
    assert {cc.plan_kind(*p) for p in plans} == set(cc.KINDS)


PIVOT_POLICIES = [{}, {"trsm": 0, "lat": 0}, {"sweep": 0}, {"pk": 1}, {"p128": 0}, {"persist": 1}]


@pytest.mark.parametrize("sw", PIVOT_POLICIES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()) or "default")
def test_factor_bad_pivots(gpu_ctx, sw):
    """-1 and nan on the diagonal at columns 1, 32, 33, 128, 129 and n, each in its own member
    of one batch of 17: each reports its column, and every other member's factor is
    bit-identical to the same batch with good matrices in those places."""
    n, cols = 300, (1, 32, 33, 128, 129, 300)
    A = cc.factor_mats("gp6", n, 17)
    mats, bad = [], {}
    for b in range(17):
        k = (b - 2) // 2
        if 2 <= b < 14:
            mats.append(cc.bad_matrix(A[b], cols[k], -1.0 if b % 2 == 0 else np.nan))
            bad[b] = cols[k]
        else:
            mats.append(A[b])
    case = cc.FactorCase(np.stack(mats), "odd", bad=bad, tag=f"pivots {sw}")
    after, info, kind = run_factor(gpu_ctx, case, sw)
    problems = case.verify(after, info, kind)
    clean = cc.FactorCase(A, "odd", tag=f"pivots {sw}, all good")
    after_clean, info_clean, _ = run_factor(gpu_ctx, clean, sw)
    problems += clean.verify(after_clean, info_clean, kind)
    got, ref = case.buf.get(after), clean.buf.get(after_clean)
    for b in range(17):
        if b not in bad and not np.array_equal(cc.bits(got[b]), cc.bits(ref[b])):
            problems.append(f"member {b}: its factor changed with its neighbours' bad pivots")
    assert not problems, "\n".join(problems[:20])


def test_potrf_diag_refuses(gpu_ctx):
    """A policy gpmpc_potrf_plan refuses, overlapping members, a matrix past its tensor:
    refused before anything is launched, the buffer untouched."""
    import torch
    L = _lib()
    ctx = gpu_ctx
    t = torch.from_numpy(cc.poison(64)).cuda()
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(L.HIPError) as e:
        L.potrf_diag(ctx, t, 4, 2, 0, 4, 16, info, ob=100)
    assert e.value.rc == -2
    with pytest.raises(L.HIPError) as e:
        L.potrf_diag(ctx, t, 4, 2, 0, 4, 16, info, ob=2048)
    assert e.value.rc == -2
    with pytest.raises(ValueError):
        L.potrf_diag(ctx, t, 4, 2, 0, 4, 15, info)
    with pytest.raises(ValueError):
        L.potrf_diag(ctx, t, 4, 2, 40, 4, 16, info)
    with pytest.raises(TypeError):
        L.potrf_diag(ctx, t, 4, 2, 0, 4, 16, info, obb=128)
    ctx.sync()
    assert np.array_equal(cc.bits(t.cpu().numpy()), cc.bits(cc.poison(64)))


# ---- the triangular launchers and the solve helpers ------------------------------------------
def run_tri(ctx, case, report=None):
    import torch
    L = _lib()
    tens = {id(b): torch.from_numpy(b.flat.copy()).cuda() for b in case.bufs()}

    def op(b):
        return None if b is None else (tens[id(b)], b.offset, b.ld)

    torch.cuda.synchronize()
    L.tri_diag(ctx, case.op, case.n, case.nrhs, op(case.bL), op(case.bX), op(case.bW), case.flags)
    ctx.sync()
    return case.verify({k: t.cpu().numpy() for k, t in tens.items()}, report)


def finish(bad, report):
    worst = {}
    for tag, r in report:
        key = " ".join(tag.split()[:1] + [w for w in tag.split() if w in cc.REAL_FAMILIES + ("bwd", "fwd")])
        worst[key] = max(worst.get(key, 0.0), r)
    for key, r in sorted(worst.items()):
        print(f"{key}: max residual / bound = {r:.3g}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n", cc.TRI_N)
def test_trsm(gpu_ctx, n):
    """Forward and backward at every nrhs: the exact family at tolerance zero and one real
    family (rotating) by the residual rule; a random lower-triangular right-hand side at
    nrhs = n under RHS_LOWER."""
    bad, report = [], []
    for i, nrhs in enumerate(cc.tri_nrhs(n)):
        for trans in (False, True):
            j = 2 * i + trans + n
            variant = cc.LAYOUTS[j % 4]
            bad += run_tri(gpu_ctx, cc.trsm_case(n, nrhs, trans, "integer", variant))
            bad += run_tri(gpu_ctx, cc.trsm_case(n, nrhs, trans, cc.REAL_FAMILIES[j % 4], cc.LAYOUTS[(j + 1) % 4]),
                           report)
    for k, family in enumerate(("integer", cc.REAL_FAMILIES[n % 4], "gp8")):
        bad += run_tri(gpu_ctx, cc.trsm_case(n, n, False, family, cc.LAYOUTS[(n + k) % 4], rhs_lower=True), report)
    finish(bad, report)


@pytest.mark.parametrize("n", [33, 128, 129, 256, 257, 300, 385, 517])
def test_tri_inverse(gpu_ctx, n):
    """The doubling inverse: one block (n <= 128), a ragged pair alone (129, 257), full pairs
    (256), full and ragged pairs at two levels (300, 385, 517)."""
    bad, report = [], []
    for k, family in enumerate(("integer",) + cc.REAL_FAMILIES):
        bad += run_tri(gpu_ctx, cc.tri_inverse_case(n, family, cc.LAYOUTS[(n + k) % 4]), report)
    finish(bad, report)


@pytest.mark.parametrize("op", ["cho_solve_inv", "potrs_cols"])
def test_cho_solve(gpu_ctx, op):
    """(L L^T)^-1 y through W = L^-1 with one refinement step, and by the per-column
    substitution kernel: one bound for both (gp.hip: "as accurate as the two substitutions")."""
    bad, report = [], []
    for i, n in enumerate(cc.TRI_N):
        for k, nc in enumerate((1, 3, 16)):
            j = 3 * i + k
            bad += run_tri(gpu_ctx, cc.cho_case(op, n, nc, "integer", cc.LAYOUTS[j % 4]))
            bad += run_tri(gpu_ctx, cc.cho_case(op, n, nc, cc.REAL_FAMILIES[j % 4], cc.LAYOUTS[(j + 1) % 4]), report)
        bad += run_tri(gpu_ctx, cc.cho_case(op, n, 3, "gp8", "shift"), report)
    finish(bad, report)


def test_tri_diag_refuses(gpu_ctx):
    """Arguments outside a launcher's contract: -2, nothing launched, the buffers untouched."""
    import torch
    L = _lib()
    n = 40
    Lm, _ = cc.integer_L(n)
    tl = torch.from_numpy(np.ascontiguousarray(Lm).ravel().copy()).cuda()
    tx = torch.from_numpy(cc.poison(n * 20)).cuda()
    before = tx.clone()
    refused = [("cho_solve_inv", n, 17, (tl, 0, n), (tx, 0, 17), (tl, 0, n), 0),    # nrhs > 16
               ("cho_solve_inv", n, 3, (tl, 0, n), (tx, 0, 3), None, 0),             # no W
               ("cho_solve_inv", n, 3, (tl, 0, n), (tx, 0, 4), (tl, 0, n), 0),       # Y not packed
               ("potrs_cols", n, 3, (tl, 0, n), (tx, 0, 4), None, 0),                # Y not packed
               ("trsm", n, 5, (tl, 0, n), (tx, 0, 5), None, L.TRI_TRANS | L.TRI_RHS_LOWER),
               ("trsm", n, 5, (tl, 0, n), (tx, 0, 5), None, 4),                      # unknown flag
               ("tri_inverse", n, 5, (tl, 0, n), (tx, 0, 5), None, 0),               # nrhs != n
               ("potrs_cols", n, 3, (tl, 0, n), (tx, 0, 3), None, L.TRI_TRANS),      # flags on another op
               (7, n, 3, (tl, 0, n), (tx, 0, 3), None, 0)]
    for op, nn, nrhs, Lo, Xo, Wo, flags in refused:
        with pytest.raises(L.HIPError) as e:
            L.tri_diag(gpu_ctx, op, nn, nrhs, Lo, Xo, Wo, flags)
        assert e.value.rc == -2, (op, nrhs, flags)
    with pytest.raises(ValueError):
        L.tri_diag(gpu_ctx, "trsm", n, 21, (tl, 0, n), (tx, 0, 21), None, 0)         # past its tensor
    gpu_ctx.sync()
    assert torch.equal(tx.view(torch.int64), before.view(torch.int64))
