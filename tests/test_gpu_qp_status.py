"""Every OSQP status of the batched ADMM, on all three device solvers, against the C oracle.

The N = 20 MPC problems of test_gpu_parity._qp_batch (n = 207, m = 354: rows 0-146
equalities, the bound row of variable j at 147 + j) in six variants whose oracle
answers cover the statuses 1, 2, -2, -3, 3 and -4:

  base        unchanged
  primal_inf  the box of variable 1 moved to [l + 5, l + 6]; dynamics row 1 pins it to l
  dual_inf    P = 0, every bound row +-1e30, q random: the cost is unbounded below
  max_iter    primal_inf stopped at 25 iterations, before its certificate holds
  no_scaling  base with scaling = 0
  no_checks   base with check_termination = 0, max_iter = 60: only the final check
              and the approximate check run

Each variant is one cold solve (rho = settings.rho, y = 0) per seed; the settings
differ per variant and the entry takes one settings struct, so one call per variant.
Status and iteration count are exact, x and the objective within test_gpu_parity's
tolerances where the oracle returns a solution, rho within 1e-6 relative.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import close
from test_gpu_parity import _qp_batch

SEEDS = (0, 1, 2, 3)
MD = 147  # dynamics rows; bound row of variable j is MD + j
VARIANTS = {  # name -> settings that differ from the defaults
    "base": {},
    "primal_inf": {},
    "dual_inf": {},
    "max_iter": {"max_iter": 25},
    "no_scaling": {"scaling": 0},
    "no_checks": {"check_termination": 0, "max_iter": 60},
}
HAS_SOLUTION = (1, 2, -2)


@functools.lru_cache(maxsize=None)
def _base():
    probs = _qp_batch(len(SEEDS))
    for p in probs:
        p[2].sort_indices()
    return probs


def _problem(name, b):
    """(Pdiag, q, A, l, u, x_ws) of variant `name` for seed b (fresh arrays)."""
    P, q, A, l, u, xw = _base()[b]
    P, q, l, u = P.copy(), q.copy(), l.copy(), u.copy()
    if name in ("primal_inf", "max_iter"):
        lo = l[1]  # dynamics row 1: x_1 = l[1]
        l[MD + 1], u[MD + 1] = lo + 5.0, lo + 6.0
    elif name == "dual_inf":
        P[:] = 0.0
        l[MD:], u[MD:] = -1e30, 1e30
        q = np.random.RandomState(b).randn(q.size)
    return P, q, A, l, u, xw


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The C oracle's answers for variant `name`, one per seed; computed once, read-only."""
    from oracle import admm_ref
    out = []
    for b in SEEDS:
        P, q, A, l, u, xw = _problem(name, b)
        r = admm_ref.RefQP(A.shape[0], admm_ref.default_settings(**VARIANTS[name])).solve(P, q, A, l, u, xw)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return tuple(out)


def test_oracle_statuses_cover_the_table():
    """The chosen inputs reach every status the certificates and the table can give."""
    seen = {r["status"] for name in VARIANTS for r in _oracle(name)}
    assert {1, 2, -2, -3, 3, -4} <= seen, sorted(seen)
    # each variant still does what its name says
    assert {r["status"] for r in _oracle("primal_inf")} <= {-3, 3}
    assert {r["status"] for r in _oracle("dual_inf")} <= {-4, 4}
    assert {(r["status"], r["iter"]) for r in _oracle("max_iter")} == {(-2, 25)}
    assert {r["iter"] for r in _oracle("no_checks")} == {60}


def solve_variant(L, ctx, name, B):
    """One gpmpc_qp_solve_batched call: B problems, the seeds tiled.  Raw outputs."""
    probs = [_problem(name, SEEDS[i % len(SEEDS)]) for i in range(B)]
    A0 = probs[0][2]
    rp = np.ascontiguousarray(A0.indptr, np.int32); ci = np.ascontiguousarray(A0.indices, np.int32)
    n, m, nnz = A0.shape[1], A0.shape[0], A0.nnz
    Av = np.stack([p[2].data for p in probs]); Pd = np.stack([p[0] for p in probs])
    qv = np.stack([p[1] for p in probs]); lv = np.stack([p[3] for p in probs]); uv = np.stack([p[4] for p in probs])
    xw = np.stack([p[5] for p in probs])
    st = L.qp_default_settings(**VARIANTS[name])
    rho = np.full(B, float(st.rho)); ysc = np.zeros((B, m))
    x = np.empty((B, n)); y = np.empty((B, m)); it = np.zeros(B, np.int32); stt = np.zeros(B, np.int32)
    obj = np.empty(B)
    rc = L._L.gpmpc_qp_solve_batched(ctx.h, B, n, m, nnz, L._i(rp), L._i(ci), L._d(Av), L._d(Pd),
                                     L._d(qv), L._d(lv), L._d(uv), ctypes.byref(st), L._d(xw),
                                     L._d(rho), L._d(ysc), L._d(x), L._d(y), L._i(it), L._i(stt), L._d(obj))
    assert rc == 0, L._L.gpmpc_last_error()
    return dict(x=x, y=y, iter=it, status=stt, obj=obj, rho=rho)


@pytest.mark.gpu
@pytest.mark.parametrize("fleet,B", [("1", 24), ("1", 300), ("0", 24)])
def test_qp_status_vs_c_oracle(gpu_ctx, monkeypatch, fleet, B):
    """The fleet solver's wide build (one problem per CU or fewer), its narrow build
    (300 problems, two items per thread) and the generic kernel (GPMPC_QP_FLEET=0)."""
    monkeypatch.setenv("GPMPC_QP_FLEET", fleet)
    from gp_mpc_rocket_landing_amd import _lib as L
    for name in VARIANTS:
        ref = _oracle(name)
        out = solve_variant(L, gpu_ctx, name, B)
        for b in range(B):
            r = ref[b % len(SEEDS)]
            print(name, b, int(out["status"][b]), int(out["iter"][b]), out["rho"][b], r["status"], r["iter"], r["rho"])
            assert (int(out["status"][b]), int(out["iter"][b])) == (r["status"], r["iter"]), (name, b)
            assert abs(out["rho"][b] - r["rho"]) <= 1e-6 * r["rho"], (name, b)
            if r["status"] in HAS_SOLUTION:
                ok, e = close(out["x"][b], r["x"], np.abs(r["x"]).max()); assert ok, (name, b, e)
                np.testing.assert_allclose(out["obj"][b], r["obj_val"], rtol=1e-6)
