"""The convex-hull terminal layer without a device: the names, signatures and defaults of the
reference's src/terminal/convex_hull.py written out, the plan and the argument refusals of the
C ABI (include/gpmpc.h), and the branches of the Python surface that make no device call."""
import ctypes
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_names_signatures_and_defaults_are_the_references():
    from gp_mpc_rocket_landing_amd import terminal
    from gp_mpc_rocket_landing_amd.terminal import ConvexHullConfig, ConvexHullConstraint, TerminalSetManager
    for name in ("ConvexHullConfig", "ConvexHullConstraint", "TerminalSetManager"):
        assert name in terminal.__all__
    assert not hasattr(terminal, "CasADiConvexHullConstraint")
    E = inspect.Parameter.empty
    fields = [(f.name, f.type, f.default) for f in dataclasses.fields(ConvexHullConfig)]
    assert fields == [("n_vertices", "int", 10), ("use_slack", "bool", True), ("slack_weight", "float", 1e4),
                      ("convex_tol", "float", 1e-6), ("lambda_min", "float", 0.0), ("lambda_max", "float", 1.0)]
    C = ConvexHullConstraint
    assert _params(C.__init__) == [("self", E), ("vertices", E), ("q_values", E), ("config", None)]
    assert _params(C.update_vertices) == [("self", E), ("vertices", E), ("q_values", E)]
    assert _params(C.check_feasibility) == [("self", E), ("x", E)]
    assert _params(C.project_onto_hull) == [("self", E), ("x", E)]
    assert _params(C.get_interpolated_q) == [("self", E), ("lambdas", E)]
    assert _params(C.project_batch) == [("self", E), ("X", E)]
    assert _params(C.contains_batch) == [("self", E), ("X", E)]
    T = TerminalSetManager
    assert _params(T.__init__) == [("self", E), ("safe_set", E), ("n_vertices", 10), ("use_fuel_aware", True)]
    assert _params(T.get_terminal_set) == [("self", E), ("x", E), ("available_fuel", None)]
    assert _params(T.is_in_terminal_set) == [("self", E), ("x", E), ("available_fuel", None)]
    assert _params(T.get_terminal_cost) == [("self", E), ("x", E)]
    assert _params(T.invalidate) == [("self", E)]
    assert _params(T.project_batch) == [("self", E), ("X", E), ("available_fuel", None)]
    assert _params(T.is_in_terminal_set_batch) == [("self", E), ("X", E), ("available_fuel", None)]


def test_shape_constants_match_the_kernel():
    L = _lib()
    src = open(os.path.join(REPO, "gp_mpc_rocket_landing_amd", "csrc", "hull.h")).read()
    caps = {k: int(v) for k, v in re.findall(r"#define (HULL_MAXD|HULL_MAXK|HULL_WAVES|HULL_MAX_ITER) (\d+)", src)}
    assert caps == {"HULL_MAXD": L.HULL_MAXD, "HULL_MAXK": L.HULL_MAXK, "HULL_WAVES": L.HULL_WAVES,
                    "HULL_MAX_ITER": L.HULL_MAX_ITER}
    from gp_mpc_rocket_landing_amd.terminal import convex_hull
    assert (convex_hull.HULL_MAXK, convex_hull.HULL_MAXD) == (L.HULL_MAXK, L.HULL_MAXD)
    assert L.abi_version() == 4
    for name in ("gpmpc_hull_project", "gpmpc_knn_set_points", "gpmpc_knn_hull", "gpmpc_hull_plan"):
        assert name in L.EXPORTED


def test_plan_answers_without_a_device():
    L = _lib()
    for d, k, B in ((1, 1, 0), (7, 10, 1), (14, 50, 1024), (32, 64, 70)):
        assert L.hull_plan(d, k, B) == L.HULL_WAVES
    for d, k, B in ((0, 10, 1), (33, 10, 1), (7, 0, 1), (7, 65, 1), (7, 10, -1)):
        with pytest.raises(L.HIPError) as e:
            L.hull_plan(d, k, B)
        assert e.value.rc == -2
    assert L._L.gpmpc_hull_plan(7, 10, 1, None) == -2


def _project_rc(ctx=None, B=2, kmax=3, d=2, tol=1e-12, max_iter=100, shared=0, nv=None, null=None):
    """gpmpc_hull_project's return code on well-shaped buffers with one thing wrong."""
    L = _lib()
    kk, dd, bb = max(kmax, 1), max(d, 1), max(B, 1)
    bufs = dict(V=np.zeros((bb, kk, dd)), X=np.zeros((bb, dd)), lam=np.zeros((bb, kk)), proj=np.zeros((bb, dd)),
                dist=np.zeros(bb), gap=np.zeros(bb), iters=np.zeros(bb, np.int32), status=np.zeros(bb, np.int32))
    p = {k: (L._i(v) if v.dtype == np.int32 else L._d(v)) for k, v in bufs.items()}
    if null:
        p[null] = None
    nvp = L._i(np.ascontiguousarray(nv, np.int32)) if nv is not None else None
    rc = L._L.gpmpc_hull_project(ctx, p["V"], None, nvp, shared, p["X"], B, kmax, d, tol, max_iter, p["lam"],
                                 p["proj"], p["dist"], p["gap"], None, p["iters"], p["status"])
    return rc, L._L.gpmpc_last_error().decode()


@pytest.mark.parametrize("kw,names", [
    (dict(d=0), "d >= 1"), (dict(d=33), "d <= HULL_MAXD"), (dict(kmax=0), "kmax >= 1"),
    (dict(kmax=65), "kmax <= HULL_MAXK"), (dict(tol=0.0), "tol > 0"), (dict(tol=-1e-9), "tol > 0"),
    (dict(tol=float("nan")), "tol > 0"), (dict(max_iter=0), "max_iter >= 1"),
    (dict(max_iter=4097), "max_iter <= HULL_MAX_ITER"), (dict(B=-1), "B >= 0"), (dict(shared=2), "shared"),
    (dict(nv=[0, 4]), "nv[b]"), (dict(nv=[-1, 3]), "nv[b]"), (dict(null="V"), "V &&"), (dict(null="status"), "status"),
    (dict(), "ctx"),
])
def test_hull_project_refuses_bad_arguments(kw, names):
    """-2 with the refused condition named, before anything touches a device (no context given)."""
    rc, msg = _project_rc(**kw)
    assert rc == -2 and names in msg, (kw, rc, msg)


def test_knn_calls_refuse_a_null_set():
    L = _lib()
    assert L._L.gpmpc_knn_set_points(None, None, 7) == -2
    z = np.zeros(8)
    zi = np.zeros(8, np.int32)
    assert L._L.gpmpc_knn_hull(None, 0, L._d(z), L._d(z), 1, 10, 4, 50, 1, 1.0, None, 1e-12, 100, L._i(zi), L._i(zi),
                               L._d(z), L._d(z), L._d(z), L._d(z), None, L._i(zi), L._i(zi)) == -2


def test_empty_set_and_thin_sets_make_no_device_call():
    """K = 0 and n_x >= K are answered on the host, as in the reference."""
    from gp_mpc_rocket_landing_amd.terminal import ConvexHullConfig, ConvexHullConstraint
    x = np.array([0.5, -1.0, 2.0])
    ch = ConvexHullConstraint(np.zeros((0, 3)), np.zeros(0))
    assert (ch.K, ch.n_x) == (0, 0)
    xp, lam = ch.project_onto_hull(x)
    assert xp is x and lam.shape == (0,)
    assert ch.check_feasibility(x) is False
    Xp, Lam = ch.project_batch(np.stack([x, x]))
    assert np.array_equal(Xp, np.stack([x, x])) and Lam.shape == (2, 0)
    assert np.array_equal(ch.contains_batch(np.stack([x, x])), [False, False])
    # n_x >= K: a vertex within convex_tol, nothing else (the mid-point of two vertices is "outside")
    V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    ch = ConvexHullConstraint(V, np.array([1.0, 2.0, 4.0]))
    assert (ch.K, ch.n_x) == (3, 3)
    assert ch.check_feasibility(V[1] + 5e-7) is True
    assert ch.check_feasibility(V[1] + 1e-5) is False
    assert ch.check_feasibility(0.5 * (V[0] + V[1])) is False
    assert np.array_equal(ch.contains_batch(np.stack([V[2], V[2] + 1.0])), [True, False])
    ch2 = ConvexHullConstraint(V, np.zeros(3), ConvexHullConfig(convex_tol=1e-3))
    assert ch2.check_feasibility(V[1] + 1e-5) is True
    assert ch.get_interpolated_q(np.array([0.5, 0.25, 0.25])) == 2.0
    # update_vertices follows the reference: K changes, n_x keeps the value of construction
    ch.update_vertices(np.zeros((5, 3)), np.zeros(5))
    assert (ch.K, ch.n_x) == (5, 3)


def test_sets_past_the_kernel_limits_are_refused():
    from gp_mpc_rocket_landing_amd.terminal import ConvexHullConstraint
    with pytest.raises(ValueError, match="64"):
        ConvexHullConstraint(np.zeros((65, 3)), np.zeros(65))
    with pytest.raises(ValueError, match="32"):
        ConvexHullConstraint(np.zeros((4, 33)), np.zeros(4))
    ch = ConvexHullConstraint(np.zeros((4, 3)), np.zeros(4))
    with pytest.raises(ValueError, match="64"):
        ch.update_vertices(np.zeros((65, 3)), np.zeros(65))


def test_manager_over_an_empty_safe_set():
    from gp_mpc_rocket_landing_amd.terminal import SampledSafeSet, TerminalSetManager
    tm = TerminalSetManager(SampledSafeSet(n_x=7, n_u=3))
    assert tm.n_vertices == 10 and tm.use_fuel_aware is True
    assert tm._local_ss.config.K == 10
    X = np.arange(14.0).reshape(2, 7)
    out = tm.project_batch(X)
    assert np.array_equal(out["status"], [2, 2]) and np.array_equal(out["k_used"], [0, 0])
    assert np.array_equal(out["proj"], X) and np.all(np.isinf(out["dist"])) and np.all(np.isinf(out["q"]))
    assert np.array_equal(tm.is_in_terminal_set_batch(X), [False, False])
    assert tm.is_in_terminal_set(X[0]) is False
    v, q = tm.get_terminal_set(X[0])
    assert v.shape == (0, 7) and q.shape == (0,)
