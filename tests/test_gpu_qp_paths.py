"""Every KKT factor path of gpmpc_qp_solve_batched, its pattern edges and its refusals.

The patterns are qp_check.table(): test_qp_check proves on the CPU (gpmpc_qp_pattern_info)
that each takes the path named here.

* One KKT solve per path.  Under qp_check.ONE_ITER the solve returns x = -M^-1 q after one
  iteration: the factor and the triangular solves alone, with no ADMM iteration behind which
  a wrong multiplier could hide.  Bound: 64 cond_inf(M) 2^-53 max|x_ref| against the dense
  longdouble reference.  The C oracle's own error against that reference is at most 2.0 in
  these units (test_qp_check); 64 leaves room for the device's other elimination orders
  (right-looking LDL^T, block-tridiagonal with explicit inverse blocks), while a wrong or
  missing multiplier is an error of order 1e-3 max|x| or more, 1e7 and more in these units.
  Measured on the MI355X, worst ratio per class: mode 0 (banded) 0.099, mode 1 (blocks, not
  MPC) 3.3, MPC N = 1..19 0.10, MPC N = 20 generic 0.075, fleet wide 0.072, fleet narrow 0.072.
* Full solves (default settings, max_iter = 200), three in a row carrying rho, the scaled dual
  and x, against the C oracle on decision-stable problems: status and iterations exact, rho,
  x, y and the objective within 1e-6.
* Settings, infeasible variants, a failed factorisation (status -100), a mixed batch, the
  per-stream pattern cache, the refusals, QPWorkspace.

The N = 20 MPC runs on all three solvers: the fleet's wide build, its narrow build (taken
above one problem per CU: 300 problems, the four problems tiled) and the generic kernel
(GPMPC_QP_FLEET=0).  Every other call holds at most 8 problems.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import qp_check as Q
from conftest import close

pytestmark = pytest.mark.gpu

FULL = (("max_iter", 200),)
N20 = [("mpc_N20", "1", 4), ("mpc_N20", "1", 300), ("mpc_N20", "0", 4)]
CASES = [(p["name"], "1", Q.PER_PATTERN) for p in Q.fitting() if p["name"] != "mpc_N20"] + N20
MODE0, MODE1 = "band_n129_w11", "blk_n129_w4_sparse"     # the settings tests' two patterns


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _kkt_refs(name):
    st = Q.oracle_settings()
    out = []
    for P, q, A, l, u, xw in Q.problems(name):
        x, cond = Q.kkt_reference(P, A, l, u, q, st.rho, st.sigma)
        x.setflags(write=False)
        out.append((x, cond))
    return tuple(out)


def _kkt_ratio(x, ref):
    xr, cond = ref
    return float(np.abs(x - xr).max() / (cond * Q.U * np.abs(xr).max()))


@pytest.mark.parametrize("name,fleet,B", CASES)
def test_one_kkt_solve_per_path(gpu_ctx, monkeypatch, name, fleet, B):
    monkeypatch.setenv("GPMPC_QP_FLEET", fleet)
    pat, probs, refs = Q.by_name(name), Q.problems(name), _kkt_refs(name)
    rc, out = Q.device_solve(_lib(), gpu_ctx, pat, [probs[b % len(probs)] for b in range(B)], Q.ONE_ITER)
    assert rc == 0, _lib()._L.gpmpc_last_error()
    ratios = [_kkt_ratio(out["x"][b], refs[b % len(refs)]) for b in range(B)]
    print("KKT", name, pat["cls"], "fleet=" + fleet, "B=%d" % B, "cond %.3g" % max(c for _, c in refs),
          "worst ratio %.3g" % max(ratios))
    assert out["status"].tolist() == [-2] * B and out["iter"].tolist() == [1] * B
    assert max(ratios) <= 64.0, ratios


def _check_against_oracle(out, b, r, tag):
    """One problem's device outputs against the oracle's result r."""
    print(tag, int(out["status"][b]), int(out["iter"][b]), out["rho"][b], r["status"], r["iter"], r["rho"])
    assert (int(out["status"][b]), int(out["iter"][b])) == (r["status"], r["iter"]), tag
    assert abs(out["rho"][b] - r["rho"]) <= 1e-6 * r["rho"], tag
    if r["status"] in Q.HAS_SOLUTION:
        ok, e = close(out["x"][b], r["x"], np.abs(r["x"]).max()); assert ok, (tag, "x", e)
        ok, e = close(out["y"][b], r["y"], np.abs(r["y"]).max()); assert ok, (tag, "y", e)
        np.testing.assert_allclose(out["obj"][b], r["obj_val"], rtol=1e-6)
    else:
        assert np.isnan(out["x"][b]).all() and np.isnan(out["y"][b]).all() and np.isnan(out["obj"][b]), tag


@pytest.mark.parametrize("name,fleet,B", CASES)
def test_full_solves_vs_c_oracle(gpu_ctx, monkeypatch, name, fleet, B):
    monkeypatch.setenv("GPMPC_QP_FLEET", fleet)
    pat = Q.by_name(name)
    idx = Q.stable_problems(name, 3, FULL)
    assert len(idx) >= 2
    probs = [Q.problems(name)[idx[b % len(idx)]] for b in range(min(B, len(idx)) if B <= 8 else B)]
    refs = [Q.oracle_run(Q.problems(name)[i], 3, **dict(FULL)) for i in idx]
    rho = ysc = None
    xw = "given"
    for rep in range(3):
        rc, out = Q.device_solve(_lib(), gpu_ctx, pat, probs, dict(FULL), x_ws=xw, rho=rho, y_scaled=ysc)
        assert rc == 0, _lib()._L.gpmpc_last_error()
        for b in range(len(probs)):
            _check_against_oracle(out, b, refs[b % len(idx)][rep], (name, rep, b))
        rho, ysc, xw = out["rho"], out["y_scaled"], out["x"].copy()


VARIANTS = {  # name -> (settings on top of max_iter = 200, problem transform, device_solve arguments)
    "no_scaling": (dict(scaling=0), None, {}),
    "no_adaptive_rho": (dict(adaptive_rho=0), None, {}),
    "no_checks": (dict(check_termination=0), None, {}),
    "x_ws_null": ({}, None, dict(x_ws=None)),
    "cold": (dict(warm_start=0), None, dict(y0=True)),      # x_ws and y_scaled passed and ignored
    "primal_inf": ({}, Q.primal_infeasible, {}),
    "dual_inf": ({}, Q.dual_infeasible, {}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", [MODE0, MODE1])
def test_settings_and_infeasible_variants_vs_c_oracle(gpu_ctx, name, variant):
    kw, transform, how = VARIANTS[variant]
    kw = dict(FULL, **kw)
    pat = Q.by_name(name)
    probs = [transform(pat, p) if transform else p for p in Q.problems(name)]
    y0 = 0.1 * np.random.RandomState(5).randn(pat["m"]) if how.get("y0") else None
    okw = dict(x_ws=None) if "x_ws" in how else {}
    probs = [p for p in probs if Q.decision_stable(p, 1, y0=y0, **okw, **kw)]
    assert probs, "no decision-stable problem"
    refs = [Q.oracle_run(p, 1, y0=y0, **okw, **kw)[0] for p in probs]
    rc, out = Q.device_solve(_lib(), gpu_ctx, pat, probs, kw, x_ws=how.get("x_ws", "given"),
                             y_scaled=None if y0 is None else np.tile(y0, (len(probs), 1)))
    assert rc == 0, _lib()._L.gpmpc_last_error()
    want = {"primal_inf": {-3, 3}, "dual_inf": {-4, 4}}.get(variant)
    for b, r in enumerate(refs):
        assert want is None or r["status"] in want
        _check_against_oracle(out, b, r, (name, variant, b))


@pytest.mark.parametrize("name,fleet", [(MODE0, "1"), (MODE1, "1"), ("mpc_N20", "1"), ("mpc_N20", "0")])
def test_factor_failure_returns_nan_and_keeps_the_state(gpu_ctx, monkeypatch, name, fleet):
    """Status -100: iter 0, x, y and obj NaN (not what an earlier solve left in the staging
    buffer), rho and y_scaled as passed in; the problem beside it is solved as if alone.  On
    the band patterns the first factorisation fails; on the N = 20 MPC, whose equalities cover
    Pdiag = -1e3 at first (test_qp_check), the one after the rho adaptation at iteration 25."""
    monkeypatch.setenv("GPMPC_QP_FLEET", fleet)
    L, pat = _lib(), Q.by_name(name)
    good = Q.problems(name)[0]
    y0 = 0.01 * np.random.RandomState(3).randn(2, pat["m"]); y0[0] = 0.0
    bad = Q.not_convex(pat, good, first=name != "mpc_N20", y0=y0[1])
    rc, first = Q.device_solve(L, gpu_ctx, pat, [good, good])     # a plausible solution in every buffer
    assert rc == 0 and first["status"][1] in Q.HAS_SOLUTION
    rho0 = np.array([0.1, 0.1])
    rc, out = Q.device_solve(L, gpu_ctx, pat, [good, bad], rho=rho0, y_scaled=y0, fill=7.0)
    assert rc == 0, L._L.gpmpc_last_error()
    assert (int(out["status"][1]), int(out["iter"][1])) == (-100, 0)
    assert np.isnan(out["obj"][1]) and np.isnan(out["x"][1]).all() and np.isnan(out["y"][1]).all()
    assert out["rho"][1] == rho0[1] and np.array_equal(out["y_scaled"][1], y0[1])
    for k in ("x", "y", "obj", "iter", "status", "rho", "y_scaled"):
        assert out[k][0].tobytes() == first[k][0].tobytes(), k


@pytest.mark.parametrize("name", [MODE0, MODE1])
def test_mixed_batch_equals_single_solves(gpu_ctx, name):
    """One workgroup per problem: a failed factorisation or an infeasible neighbour changes nothing."""
    L, pat = _lib(), Q.by_name(name)
    ok = Q.problems(name)
    probs = [ok[0], Q.not_convex(pat, ok[0]), ok[1], Q.primal_infeasible(pat, ok[1]), ok[2],
             Q.dual_infeasible(pat, ok[2]), ok[3]]
    rc, out = Q.device_solve(L, gpu_ctx, pat, probs, dict(FULL))
    assert rc == 0, L._L.gpmpc_last_error()
    st = out["status"].tolist()
    print(name, st, out["iter"].tolist())
    assert st[1] == -100 and st[3] in (-3, 3) and st[5] in (-4, 4) and all(st[b] in Q.HAS_SOLUTION for b in (0, 2, 4, 6))
    for b, p in enumerate(probs):
        rc, one = Q.device_solve(L, gpu_ctx, pat, [p], dict(FULL))
        assert rc == 0
        for k in ("x", "y", "obj", "iter", "status", "rho", "y_scaled"):
            assert out[k][b].tobytes() == one[k][0].tobytes(), (b, k)


def _moved_column(pat):
    """The same n, m, nnz and rowptr; one interior entry of one coupling row in the next column."""
    rp, ci = pat["rowptr"], pat["colidx"].copy()
    cnt = np.bincount(ci, minlength=pat["n"])
    for r in range(pat["m"] - pat["n"]):
        row = ci[rp[r]:rp[r + 1]]
        for k in range(1, row.size - 1):
            if row[k] + 1 < row[k + 1] and cnt[row[k] + 1] < Q.COLMAX:
                ci[rp[r] + k] += 1
                return dict(pat, colidx=ci)
    raise AssertionError("no entry to move")


def test_pattern_cache_follows_the_pattern(gpu_ctx):
    """qp_pattern keeps one pattern per stream: a pattern with the same sizes and rowptr but
    other columns, and one that differs only in n, each get their own analysis, and the first
    pattern solves to the same bits afterwards."""
    L, pat = _lib(), Q.by_name("band_n65_w8")
    prob = Q.problems("band_n65_w8")[0]
    P, q, A, l, u, xw = prob
    moved = _moved_column(pat)
    assert not np.array_equal(moved["colidx"], pat["colidx"]) and np.array_equal(moved["rowptr"], pat["rowptr"])
    A2 = sp.csr_matrix((A.data, moved["colidx"], moved["rowptr"]), shape=A.shape)
    wider = dict(pat, n=pat["n"] + 1)                        # one more variable, in no row
    A3 = sp.csr_matrix((A.data, pat["colidx"], pat["rowptr"]), shape=(pat["m"], pat["n"] + 1))
    prob3 = (np.append(P, 0.7), np.append(q, -0.3), A3, l, u, np.append(xw, 0.0))
    st = Q.oracle_settings()
    outs = []
    for p, pr in ((pat, prob), (moved, (P, q, A2, l, u, xw)), (wider, prob3), (pat, prob)):
        rc, out = Q.device_solve(L, gpu_ctx, p, [pr], Q.ONE_ITER)
        assert rc == 0, L._L.gpmpc_last_error()
        ref = Q.kkt_reference(pr[0], pr[2], l, u, pr[1], st.rho, st.sigma)
        ratio = _kkt_ratio(out["x"][0], ref)
        print("cache", p["n"], "ratio %.3g" % ratio)
        assert (int(out["status"][0]), int(out["iter"][0])) == (-2, 1) and ratio <= 64.0
        outs.append(out)
    for k in ("x", "y", "obj", "iter", "status", "rho", "y_scaled"):
        assert outs[0][k].tobytes() == outs[3][k].tobytes(), k
    assert outs[0]["x"].tobytes() != outs[1]["x"].tobytes()


def _dummy_problem(pat):
    A = sp.csr_matrix((np.ones(pat["colidx"].size), pat["colidx"], pat["rowptr"]), shape=(pat["m"], pat["n"]))
    n, m = pat["n"], pat["m"]
    return np.ones(n), np.zeros(n), A, -np.ones(m), np.ones(m), np.zeros(n)


@pytest.mark.parametrize("name", [p["name"] for p in Q.table() if p["cls"] == "refused"] + ["nnz"])
def test_refusals_touch_nothing(gpu_ctx, name):
    L = _lib()
    valid = Q.by_name("band_n23_w9")
    pat = valid if name == "nnz" else Q.by_name(name)
    nnz = int(pat["rowptr"][-1]) + 1 if name == "nnz" else None
    rc, out = Q.device_solve(L, gpu_ctx, pat, [_dummy_problem(pat)] * 2, fill=-777.0, nnz=nnz,
                             rho=[0.25, 0.5], y_scaled=np.full((2, pat["m"]), 0.125))
    assert rc == -2 and L._L.gpmpc_last_error()
    print(name, L._L.gpmpc_last_error().decode())
    for k in ("x", "y", "obj", "iter", "status"):
        assert np.all(out[k] == -777), k
    assert out["rho"].tolist() == [0.25, 0.5] and np.all(out["y_scaled"] == 0.125)
    if name in ("w17", "row9", "col13"):       # refused by the pattern analysis: the message states the real caps
        msg = L._L.gpmpc_last_error().decode()
        assert "<=%d, m" % Q.NMAX in msg and "<=%d, half" % Q.MMAX in msg, msg
    # the next valid solve is still right
    rc, out = Q.device_solve(L, gpu_ctx, valid, list(Q.problems("band_n23_w9")), Q.ONE_ITER)
    assert rc == 0
    assert max(_kkt_ratio(out["x"][b], r) for b, r in enumerate(_kkt_refs("band_n23_w9"))) <= 64.0


def test_empty_batch_returns_zero(gpu_ctx):
    L, pat = _lib(), Q.by_name("band_n23_w9")
    one = np.zeros(max(pat["m"], int(pat["rowptr"][-1])))
    iz = np.zeros(1, np.int32)
    st = L.qp_default_settings()
    rc = L._L.gpmpc_qp_solve_batched(gpu_ctx.h, 0, pat["n"], pat["m"], int(pat["rowptr"][-1]), L._i(pat["rowptr"]),
                                     L._i(pat["colidx"]), L._d(one), L._d(one), L._d(one), L._d(one), L._d(one),
                                     ctypes.byref(st), None, L._d(one), L._d(one), L._d(one), L._d(one),
                                     L._i(iz), L._i(iz), L._d(one))
    assert rc == 0


def _filtered(probs):
    """The MPC problems with their smallest dynamics entries (the same ones in every problem) set
    to zero, and the value-filtered pattern (|a| >= 1e-12) of the result."""
    A0 = probs[0][2]
    mag = np.max([np.abs(p[2].data) for p in probs], axis=0)
    drop = np.argsort(mag)[:6]
    out = []
    for P, q, A, l, u, xw in probs:
        d = A.data.copy(); d[drop] = 0.0
        out.append((P, q, sp.csr_matrix((d, A.indices, A.indptr), shape=A.shape), l, u, xw))
    keep = np.ones(A0.nnz, bool); keep[drop] = False
    rows = np.repeat(np.arange(A0.shape[0]), np.diff(A0.indptr))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=A0.shape[0]))]).astype(np.int32)
    return out, keep, (rp, A0.indices[keep].astype(np.int32))


def test_qp_workspace_reset_and_filtered_pattern(gpu_ctx):
    """QPWorkspace: a solve, a second solve on a value-filtered pattern (fewer non-zeros, the
    rows and the carried dual the same) warm-started from the first, both against the oracle;
    reset() then gives the first solve's bits again."""
    L = _lib()
    name = "mpc_N8"
    pat = Q.by_name(name)
    allp = Q.problems(name)
    zeroed, keep, fpat = _filtered(list(allp))
    assert fpat[0][-1] == keep.sum() < pat["rowptr"][-1]
    assert Q.classify(pat["n"], pat["m"], *fpat)["mode"] == 1
    idx = [b for b in range(len(allp)) if Q.decision_stable([allp[b], zeroed[b]], 2, **dict(FULL))]
    assert len(idx) >= 2
    refs = [Q.oracle_run([allp[b], zeroed[b]], 2, **dict(FULL)) for b in idx]
    ws = L.QPWorkspace(gpu_ctx, pat["n"], pat["m"], pat["rowptr"], pat["colidx"], batch=len(idx),
                       settings=L.qp_default_settings(**dict(FULL)))
    stack = lambda probs, k: np.stack([probs[b][k] for b in idx])
    args = lambda probs: (stack(probs, 0), stack(probs, 1), stack(probs, 3), stack(probs, 4))
    Av = np.stack([allp[b][2].data for b in idx])
    o1 = ws.solve(Av, *args(allp), x_ws=stack(allp, 5))
    Af = np.stack([zeroed[b][2].data[keep] for b in idx])
    o2 = ws.solve(Af, *args(zeroed), x_ws=o1["x"], pattern=fpat)
    for o, rep in ((o1, 0), (o2, 1)):
        o = dict(o, obj=o["obj_val"])
        for k in range(len(idx)):
            _check_against_oracle(o, k, refs[k][rep], (name, "workspace", rep, k))
    assert not np.array_equal(ws.rho, np.full(len(idx), 0.1)) or np.any(ws.y_scaled != 0.0)
    ws.reset()
    assert np.all(ws.rho == ws.settings.rho) and not ws.y_scaled.any()
    o3 = ws.solve(Av, *args(allp), x_ws=stack(allp, 5))
    for k in ("x", "y", "obj_val", "iter", "status", "rho"):
        assert o3[k].tobytes() == o1[k].tobytes(), k
