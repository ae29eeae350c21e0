"""Every fit, predict, likelihood and append path of csrc/gp.hip at its edges: the tables of
tests/gp_check.py through ExactGPHandle, FITCHandle, gp_lml_batched and append, held to that
module's rules against longdouble references computed here (tests/test_gp_check.py shows
without a GPU what the rules accept and reject, and that a case sits on each side of every
edge).  The exact cases run under both values of GPMPC_POST_CS (read at fit and predict),
the sparse predicts with GPMPC_FITC_SMALL unset and 0 (read per call), each against the
reference -- not against each other, so an error in the handle's state shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_check as g  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not g.longdouble_ok(), reason="numpy longdouble is no finer than float64")]


def _lib():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


def kind_arg(c):
    return _lib().KernelProgram(*g.prog_arrays(c.spec)) if c.kind == "prog" else c.code


def verdict(results):
    for name, r in results:
        print(f"{name}: {r:.3g}")
    bad = g.failures(results)
    assert not bad, "\n".join(bad)


def fit_exact(ctx, c, n=None):
    n = c.n if n is None else n
    return _lib().ExactGPHandle(ctx, kind_arg(c), c.X[:n], c.Y[:n], c.ls, c.sigma2, c.noise)


def state_of(h, Y):
    L, alpha = h.state()
    return g.NS(Y=Y, L=L, alpha=alpha, ymean=h.y_mean, ystd=h.y_std, lml=h.lml, steps=h.jitter_steps)


@pytest.mark.parametrize("cs", ["0", "1"])
@pytest.mark.parametrize("spec", g.EXACT_ALL, ids=g.case_id)
def test_exact(gpu_ctx, monkeypatch, spec, cs):
    """Fit (state, lml, normalisation, ladder step), predict and predict_cov."""
    monkeypatch.setenv("GPMPC_POST_CS", cs)
    c = g.exact_case(spec)
    h = fit_exact(gpu_ctx, c)
    mean, var = h.predict(c.Xq)
    res = g.check_exact_fit(c, state_of(h, c.Y)) + g.check_exact_predict(c, mean, var)
    if c.opt == "clamp":
        assert var[0, 0] == g.CLAMP * h.y_std[0] ** 2
    if c.pc:
        cm, cov = h.predict_cov(c.Xq[:c.pc])
        res += g.check_cov(c, cm, cov, var)
    verdict(res)


def test_exhausted_ladder_raises_and_the_context_stays_usable(gpu_ctx):
    c = g.exact_case(g.EXACT_EXHAUST)
    with pytest.raises(ValueError):
        fit_exact(gpu_ctx, c)
    ok = g.exact_case(g.EXACT_FIT[2])
    verdict(g.check_exact_fit(ok, state_of(fit_exact(gpu_ctx, ok), ok.Y)))


@pytest.mark.parametrize("spec", g.SPARSE_ALL, ids=g.case_id)
def test_sparse(gpu_ctx, monkeypatch, spec):
    """FITC / VFE fit (lam, alpha, lml, normalisation) and both forms of the posterior."""
    c = g.sparse_case(spec)
    L = _lib()
    ls = L.KernelProgram(*g.prog_arrays(c.spec)) if c.kind == "prog" else c.ls
    h = L.FITCHandle(gpu_ctx, c.Z, c.X, c.Y, ls, c.sigma2, c.noise, jitter=c.jitter, method=c.method)
    res = g.check_sparse_fit(c, g.NS(lam=h.lam, alpha=h.alpha(), lml=h.lml, ymean=h.y_mean, ystd=h.y_std))
    monkeypatch.delenv("GPMPC_FITC_SMALL", raising=False)
    mean, var = h.predict(c.Xq)
    res += g.check_sparse_predict(c, mean, var, " (default form)")
    monkeypatch.setenv("GPMPC_FITC_SMALL", "0")
    mean, var = h.predict(c.Xq)
    res += g.check_sparse_predict(c, mean, var, " (GEMM form)")
    verdict(res)


@pytest.mark.parametrize("spec", g.BATCH_ALL, ids=g.case_id)
def test_lml_batched(gpu_ctx, spec):
    c = g.batch_case(spec)
    lml, steps = _lib().gp_lml_batched(gpu_ctx, c.code, c.X, c.y, c.ls, c.sigma2, c.noise)
    verdict(g.check_batched(c, lml, steps))


def test_lml_batched_and_the_handle_meet_one_reference(gpu_ctx):
    c = g.batch_case(g.BATCH_ALL[2])
    L = _lib()
    lml, _ = L.gp_lml_batched(gpu_ctx, c.code, c.X, c.y, c.ls, c.sigma2, c.noise)
    h = L.ExactGPHandle(gpu_ctx, c.code, c.X, c.y, c.ls[0], c.sigma2[0], c.noise[0])
    bound = c.b[0] * abs(c.lml[0])
    verdict([("batched lml", g.ratio(lml[0], c.lml[0], bound)), ("handle lml", g.ratio(h.lml[0], c.lml[0], bound))])


@pytest.mark.parametrize("spec", g.APPEND_ALL, ids=g.case_id)
def test_append(gpu_ctx, spec):
    """State, lml, normalisation and predictions of the grown handle against the longdouble GP
    of the concatenated data, after every block."""
    c = g.append_case(spec)
    h = fit_exact(gpu_ctx, c, c.n0)
    n, res = c.n0, []
    for k, stage in zip(c.ks, c.stages):
        assert h.append(c.X[n:n + k], c.Y[:n + k]) is True
        n += k
        assert h.n == n == stage.n
        mean, var = h.predict(c.Xq)
        res += g.check_append(c, stage, state_of(h, c.Y[:n]), mean, var)
    verdict(res)


def test_refused_append_leaves_the_handle_alone(gpu_ctx):
    c = g.append_case(g.APPEND_REFUSE)
    h = fit_exact(gpu_ctx, c, c.n0)
    assert h.jitter_steps == 0
    before = [g.gk.bits(a).copy() for a in h.predict(c.Xq) + h.state()]
    assert h.append(c.X[c.n0:], c.Y) is False
    assert h.n == c.n0
    after = [g.gk.bits(a) for a in h.predict(c.Xq) + h.state()]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_argument_refusals(gpu_ctx):
    """n_out = 17, d = 33, m = 0 and VFE with noise <= 0 are refused, and the context fits on."""
    L = _lib()
    rng = np.random.default_rng(5)
    X, Z = rng.standard_normal((20, 3)), rng.standard_normal((4, 3))
    Y = rng.standard_normal((20, 2))
    ls = np.full(3, 1.5)
    refused = [lambda: L.ExactGPHandle(gpu_ctx, L.SE_ARD, X, rng.standard_normal((20, 17)), ls, 1.0, 1e-2),
               lambda: L.ExactGPHandle(gpu_ctx, L.SE_ARD, rng.standard_normal((20, 33)), Y, np.full(33, 8.0), 1.0,
                                       1e-2),
               lambda: L.FITCHandle(gpu_ctx, Z, X, rng.standard_normal((20, 17)), ls, 1.0, 1e-2),
               lambda: L.FITCHandle(gpu_ctx, rng.standard_normal((4, 33)), rng.standard_normal((20, 33)), Y,
                                    np.full(33, 8.0), 1.0, 1e-2),
               lambda: L.FITCHandle(gpu_ctx, np.zeros((0, 3)), X, Y, ls, 1.0, 1e-2),
               lambda: L.FITCHandle(gpu_ctx, Z, X, Y, ls, 1.0, 0.0, method="vfe"),
               lambda: L.FITCHandle(gpu_ctx, Z, X, Y, ls, 1.0, -1e-3, method="vfe")]
    for make in refused:
        with pytest.raises(L.HIPError) as e:
            make()
        assert e.value.rc == -2
        h = L.ExactGPHandle(gpu_ctx, L.SE_ARD, X, Y, ls, 1.0, 1e-2)
        assert np.all(np.isfinite(h.lml))
        f = L.FITCHandle(gpu_ctx, Z, X, Y, ls, 1.0, 1e-2)
        assert np.all(np.isfinite(f.lml))
    for handle in (h, f):
        mean, var = handle.predict(np.zeros((0, 3)))
        assert mean.shape == var.shape == (0, 2)
