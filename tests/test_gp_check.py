"""The rules of tests/gp_check.py, without a GPU: on every case of the tables that
tests/test_gpu_gp.py runs, the float64 restatement of csrc/gp.hip's GP layer and
oracle/gp_oracle.py (LAPACK) pass every rule with a ratio <= 1/4, and each wrong variant is
rejected by a rule (a finite ratio > 1, never a shape or finiteness check) on every case where
it is defined.  Also: the constants c are the smallest powers of two that allow that, the
conditions on the cases, and -- from the kernel constants read out of csrc and from
gpmpc_gemm_row_tiles (no device) -- that a case sits on either side of every edge."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_check as g  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not g.longdouble_ok(), reason="numpy longdouble is no finer than float64")


def plans(M, p, K):
    from gp_mpc_rocket_landing_amd import _lib
    return _lib.gemm_row_tiles(M, p, K)


def rejected(results):
    """Some rule gives a finite ratio > 1."""
    return any(1.0 < r < math.inf for _, r in results)


def accept(results, what):
    name, r = g.worst(results)
    assert r <= 0.25, f"{what}: {name}: ratio {r:.3g} > 1/4"
    return r


# ---- exact ---------------------------------------------------------------------------------------
def exact_results(c, st, mean, var, cov=None):
    res = g.check_exact_fit(c, st) + g.check_exact_predict(c, mean, var)
    if c.pc:
        res += g.check_cov(c, cov[0], cov[1], var)
    return res


def exact_oracle(c):
    o = g.oracle_exact(c)
    mean, var = g.go.exact_predict(o.st, c.Xq)
    cov = None
    if c.pc:
        cov = (g.go.exact_predict(o.st, c.Xq[:c.pc])[0], g.go.exact_predict_cov(o.st, c.Xq[:c.pc])[1] / o.ystd[0] ** 2)
    return exact_results(c, o, mean, var, cov)


def exact_restated(c, fit_mut=None, pred_mut=None):
    st = g.restate_exact(c, mut=fit_mut)
    pr = g.restate_predict(st, c.spec, c.ls, c.sigma2, c.Xq, mut=pred_mut, plans=plans)
    if pr is None:
        return None
    return exact_results(c, st, pr[0], pr[1], g.restate_cov(st, c) if c.pc else None)


def exact_defined(c, mut):
    """Where a wrong variant changes anything the data can show."""
    r = c.ref
    if mut == "sample_std":
        return c.n >= 2
    if mut == "no_jitter":
        return r.steps > 0
    if mut == "alpha_last":
        return bool(np.any(r.alpha[-1] != 0))
    if mut in ("std_next", "std_not_squared"):
        return bool(np.any(r.ystd != 1)) and (mut != "std_next" or bool(np.any(np.roll(r.ystd, -1) != r.ystd)))
    if mut == "stale_partial":   # 1e-9 sigma2 is above the rule's bound
        return c.b < 1e-9 / 2
    return True


@pytest.mark.parametrize("spec", g.EXACT_ALL, ids=g.case_id)
def test_exact_rules_accept_and_reject(spec):
    c = g.exact_case(spec)
    print(c.tag, f"kappa {c.ref.kappa:.3g}, c N u kappa {c.b:.3g}: oracle {accept(exact_oracle(c), 'gp_oracle'):.3g}, "
          f"restatement {accept(exact_restated(c), 'restatement'):.3g}")
    for mut in g.FIT_MUTANTS + g.PREDICT_MUTANTS:
        if not exact_defined(c, mut):
            continue
        fit = mut in g.FIT_MUTANTS
        res = exact_restated(c, fit_mut=mut if fit else None, pred_mut=None if fit else mut)
        if res is None:
            continue
        assert rejected(res), f"{c.tag}: the rules accept the wrong variant {mut} (worst {g.worst(res)})"


def test_every_exact_mutant_is_defined_somewhere():
    seen = {m: 0 for m in g.FIT_MUTANTS + g.PREDICT_MUTANTS}
    for spec in g.EXACT_ALL:
        c = g.exact_case(spec)
        st = g.restate_exact(c)
        for m in seen:
            if exact_defined(c, m) and (m in g.FIT_MUTANTS or g.restate_predict(st, c.spec, c.ls, c.sigma2, c.Xq, mut=m,
                                                                                  plans=plans) is not None):
                seen[m] += 1
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen
    assert seen["omit_partial"] >= 5 and seen["stale_partial"] >= 10


def test_exhausted_ladder_case():
    c = g.exact_case(g.EXACT_EXHAUST)
    assert c.ref is None
    with pytest.raises(ValueError):
        g.oracle_exact(c)
    with pytest.raises(ValueError):
        g.restate_exact(c)


def test_ladder_cases_need_exactly_one_and_five_steps():
    steps = {s[6]: g.exact_case(s).ref.steps for s in g.EXACT_FIT if s[6] in ("dup1", "dup5")}
    assert steps == {"dup1": 1, "dup5": 5}
    for s in g.EXACT_FIT:
        if s[6] in ("dup1", "dup5"):
            assert g.oracle_exact(g.exact_case(s)).steps == steps[s[6]]


def test_clamp_cases_sit_on_both_sides():
    lo = g.exact_case([s for s in g.EXACT_PREDICT if s[6] == "clamp"][0])
    hi = g.exact_case([s for s in g.EXACT_PREDICT if s[6] == "above"][0])
    assert 0 < float(lo.pred.lat[0]) < g.CLAMP < float(hi.pred.lat[0]) < 4 * g.CLAMP
    assert float(lo.pred.var[0, 0]) == g.CLAMP and lo.ref.kappa == 1.0
    const = g.exact_case([s for s in g.EXACT_FIT if s[6] == "const"][0])
    assert const.ref.degenerate.tolist() == [False, True, False] and const.ref.ystd[1] == 1


# ---- sparse --------------------------------------------------------------------------------------
def sparse_restated(c, mut=None):
    fit_mut = mut if mut in ("lam_no_noise", "trace_n1", "w2_upper", "sample_std") else None
    st = g.restate_sparse(c, mut=fit_mut)
    if st is None:
        return None
    pr = g.restate_sparse_predict(c, st, c.Xq, mut=None if fit_mut else mut)
    if pr is None:
        return None
    return g.check_sparse_fit(c, st) + g.check_sparse_predict(c, pr[0], pr[1])


def sparse_defined(c, mut):
    r = c.ref
    if mut == "alpha_last":
        return bool(np.any(r.alpha[-1] != 0))
    if mut == "w2_upper":   # 1e-9 above the diagonal moves |w|^2 by about 1e-9 m |w|: above the bound
        return c.m >= 2 and c.b < 1e-10
    return True


@pytest.mark.parametrize("spec", g.SPARSE_ALL, ids=g.case_id)
def test_sparse_rules_accept_and_reject(spec):
    c = g.sparse_case(spec)
    o = g.oracle_sparse(c)
    mean, var = g.go.fitc_predict(o.st, c.Xq)
    ro = accept(g.check_sparse_fit(c, o) + g.check_sparse_predict(c, mean, var), "gp_oracle")
    rr = accept(sparse_restated(c), "restatement")
    print(c.tag, f"kappa K_uu {c.ref.kappa_uu:.3g} B {c.ref.kappa_B:.3g}, c N u kappa {c.b:.3g}: oracle {ro:.3g}, "
          f"restatement {rr:.3g}")
    for mut in g.SPARSE_MUTANTS:
        res = sparse_restated(c, mut) if sparse_defined(c, mut) else None
        if res is not None:
            assert rejected(res), f"{c.tag}: the rules accept the wrong variant {mut} (worst {g.worst(res)})"


def test_every_sparse_mutant_is_defined_somewhere():
    seen = {m: 0 for m in g.SPARSE_MUTANTS}
    for spec in g.SPARSE_ALL:
        c = g.sparse_case(spec)
        for m in seen:
            seen[m] += sparse_defined(c, m) and sparse_restated(c, m) is not None
    print(seen)
    assert all(v >= 3 for v in seen.values()), seen


# ---- gp_lml_batched ------------------------------------------------------------------------------
def batched_results(c, f, **kw):
    r = [f(c, b, **kw) for b in range(c.B)]
    return g.check_batched(c, np.array([x[0] for x in r], float), [x[1] for x in r])


@pytest.mark.parametrize("spec", g.BATCH_ALL, ids=g.case_id)
def test_batched_rules_accept_and_reject(spec):
    c = g.batch_case(spec)
    print(c.tag, f"c N u kappa {c.b.max():.3g}: oracle {accept(batched_results(c, g.oracle_lml), 'gp_oracle'):.3g}, "
          f"restatement {accept(batched_results(c, g.restate_lml), 'restatement'):.3g}")
    for mut in ("lml_no_2pi", "lml_n1") + (("no_jitter",) if c.opt == "ladder" else ()):
        res = batched_results(c, g.restate_lml, mut=mut)
        assert rejected(res), f"{c.tag}: the rules accept the wrong variant {mut} (worst {g.worst(res)})"
    if c.opt == "ladder":
        assert c.steps.tolist() == [0, 1, 0, -1, 0]


def test_batched_and_handle_share_one_reference():
    """The parameter set the GPU test gives to both gp_lml_batched and ExactGPHandle: the two
    restatements are within the rule of the same longdouble value."""
    c = g.batch_case(g.BATCH_ALL[2])
    lml, _ = g.restate_lml(c, 0)
    e = g.NS(X=c.X, Y=c.y[:, None], spec=c.kind, ls=c.ls[0], sigma2=c.sigma2[0], noise=c.noise[0])
    for got in (lml, g.restate_exact(e).lml[0]):
        assert g.ratio(got, c.lml[0], c.b[0] * abs(c.lml[0])) <= 0.25


# ---- append --------------------------------------------------------------------------------------
def append_stages(c, mut=None):
    """[(results of the restated append, results of gp_oracle on the concatenated data)] per block."""
    st = g.restate_exact(c, XY=(c.X[:c.n0], c.Y[:c.n0]))
    out = []
    for k, stage in zip(c.ks, c.stages):
        grown = g.restate_append(c, st, k, mut=mut)
        mean, var = g.restate_predict(grown, c.kind, c.ls, c.sigma2, c.Xq, plans=plans)
        o = g.oracle_exact(c, XY=(c.X[:stage.n], c.Y[:stage.n]))
        om, ov = g.go.exact_predict(o.st, c.Xq)
        out.append((g.check_append(c, stage, grown, mean, var), g.check_append(c, stage, o, om, ov)))
        st = g.restate_append(c, st, k)
    return out


@pytest.mark.parametrize("spec", g.APPEND_ALL, ids=g.case_id)
def test_append_rules_accept_and_reject(spec):
    c = g.append_case(spec)
    for i, (rr, ro) in enumerate(append_stages(c)):
        print(c.tag, f"block {i}: c N u kappa {c.stages[i].b:.3g}: oracle {accept(ro, 'gp_oracle'):.3g}, "
              f"restatement {accept(rr, 'restatement'):.3g}")
    for mut in ("w_sign", "old_norm"):
        for rr, _ in append_stages(c, mut):
            assert rejected(rr), f"{c.tag}: the rules accept the wrong variant {mut} (worst {g.worst(rr)})"


def test_refused_append_is_not_positive_definite():
    """The concatenated matrix of the refused append fails the oracle's plain Cholesky (and
    the longdouble one), while the fit it grows from needs no jitter."""
    c = g.append_case(g.APPEND_REFUSE)
    n = c.n0 + sum(c.ks)
    K = g.go.gram(c.kind, c.X, None, c.sigma2, c.ls) + c.noise * np.eye(n)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(K)
    np.linalg.cholesky(K[:c.n0, :c.n0])
    assert g.ld_chol(g.ld_gram(c.kind, c.X, None, c.ls, c.sigma2) + g.LD(c.noise) * np.eye(n, dtype=g.LD)) is None
    assert g.ld_exact(c.kind, c.X[:c.n0], c.Y[:c.n0], c.ls, c.sigma2, c.noise).steps == 0


# ---- constants, conditions, coverage ---------------------------------------------------------------
def family_worst():
    w = {k: [0.0, 0.0] for k in g.C}

    def upd(fam, ro, rr):
        w[fam][0] = max(w[fam][0], g.worst(ro)[1])
        w[fam][1] = max(w[fam][1], g.worst(rr)[1])

    def type_b(res):
        return [x for x in res if not any(k in x[0] for k in ("y_mean", "y_std", "from the state", "steps"))]

    for spec in g.EXACT_ALL:
        c = g.exact_case(spec)
        upd("exact", type_b(exact_oracle(c)), type_b(exact_restated(c)))
    for spec in g.SPARSE_ALL:
        c = g.sparse_case(spec)
        o = g.oracle_sparse(c)
        mean, var = g.go.fitc_predict(o.st, c.Xq)
        upd(c.method, type_b(g.check_sparse_fit(c, o) + g.check_sparse_predict(c, mean, var)),
            type_b(sparse_restated(c)))
    for spec in g.BATCH_ALL:
        c = g.batch_case(spec)
        upd("batched", type_b(batched_results(c, g.oracle_lml)), type_b(batched_results(c, g.restate_lml)))
    for spec in g.APPEND_ALL:
        for rr, ro in append_stages(g.append_case(spec)):
            upd("append", type_b(ro), type_b(rr))
    return w


def test_constants_are_the_smallest_powers_of_two():
    w = family_worst()
    for fam, (ro, rr) in w.items():
        print(f"    {fam:8s} c {g.C[fam]:3d}   gp_oracle {ro:.3f}   restatement {rr:.3f}")
    for fam, (ro, rr) in w.items():
        c = g.C[fam]
        assert c == 2 ** round(math.log2(c)) and max(ro, rr) <= 0.25, (fam, ro, rr)
        assert c == 1 or 2 * max(ro, rr) > 0.25, f"{fam}: c / 2 would do ({ro:.3g}, {rr:.3g})"


def test_case_conditions():
    """The caps (asserted by the builders too), the near queries and what the tables must contain."""
    for spec in g.EXACT_ALL:
        c = g.exact_case(spec)
        assert c.b <= 1e-8
    for spec in g.SPARSE_ALL:
        c = g.sparse_case(spec)
        assert c.b <= (1e-8 if c.method == "fitc" else 1e-6)
    for spec in g.BATCH_ALL:
        assert g.batch_case(spec).b.max() <= 1e-8
    for spec in g.APPEND_ALL:
        assert max(s.b for s in g.append_case(spec).stages) <= 1e-8
    fit = g.EXACT_FIT
    assert {s[0] for s in fit} >= {1, 2, 31, 32, 33, 128, 129, 255, 256, 257, 300}
    assert {s[1] for s in fit} >= {1, 3, 8, 15, 16} and {s[2] for s in fit} >= {1, 11, 13, 32}
    assert {s[3] for s in fit} >= set(g.K4) | {"prog"}
    pred = g.EXACT_PREDICT
    assert {(s[0], s[1]) for s in pred} >= {(61, 3), (62, 3), (127, 1), (126, 3), (113, 16), (250, 6), (253, 3)}
    assert {s[4] for s in pred} >= {1, 63, 64, 65, 255, 256, 257}
    assert {s[7] for s in g.EXACT_COV} == {1, 33, 65} and {s[1] for s in g.EXACT_COV} == {1, 3}
    assert min(s[0] for s in g.EXACT_COV) <= 128 < max(s[0] for s in g.EXACT_COV)
    sp = g.SPARSE_SHAPES
    assert {s[0] for s in sp} >= {1, 16, 17, 128, 129, 255, 256, 257} and {s[1] for s in sp} == {33, 257, 300}
    assert (40, 33) in {(s[0], s[1]) for s in sp} and {s[2] for s in sp} >= {1, 8, 9, 16}
    assert {s[3] for s in sp} == {1, 11, 32} and {s[4] for s in sp} == {1, 37, 257}
    assert all(s[0] <= 16 for s in sp if s[3] == 1)
    assert {s[0] for s in g.BATCH_ALL} >= {1, 31, 32, 33, 256, 257} and {s[1] for s in g.BATCH_ALL} >= {1, 3, 17}
    assert {s[3] for s in g.BATCH_ALL} == set(g.K4)
    ap = g.APPEND_ALL
    assert {(s[0], s[1][0]) for s in ap} == {(1, 1), (31, 2), (120, 9), (128, 1), (129, 127), (250, 7), (40, 60)}
    assert {s[4] for s in ap} == {"se_ard", "se_iso", "matern52"} and {s[2] for s in ap} == {1, 16}
    assert {s[3] for s in ap} >= {1, 32} and any(len(s[1]) == 2 for s in ap)


def test_a_case_sits_on_each_side_of_every_edge():
    src = open(os.path.join(REPO, "gp_mpc_rocket_landing_amd", "csrc", "gp.hip")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (FITC_SMALL_M|FITC_SMALL_NO|TRMV_T_RB) (\d+)", src)}
    tri = {int(v) for v in re.findall(r"const bool inv = (?:tri_inv_env && )?\w+ > (\d+);", src)}
    assert tri == {128} and len(re.findall(r"const bool inv = ", src)) == 2   # exact_fit and sparse_fit
    stride = {int(v) for v in re.findall(r"i \+= (\d+)\)", src)}
    assert stride == {256}
    lml_rb = {int(v) for v in re.findall(r"r0 \+= (\d+)\)", src)}
    assert lml_rb == {32} and val["TRMV_T_RB"] == 32

    def both_sides(values, edge):
        return edge in values and edge + 1 in values

    ns = {s[0] for s in g.EXACT_ALL}
    ms = {s[1] for s in g.SPARSE_ALL}
    assert both_sides(ns, 128) and both_sides(ms, 128)                      # TRSM | doubling inverse
    assert both_sides(ns, 256) and both_sides(ms, 256)                      # the 256-thread strides
    assert both_sides({s[0] for s in g.BATCH_ALL}, 256) and both_sides({s[0] for s in g.BATCH_ALL}, 32)
    assert both_sides(ns, 32)                                               # k_trmv_t_part's row blocks
    assert both_sides({s[3] for s in g.SPARSE_ALL if s[1] <= val["FITC_SMALL_M"]}, val["FITC_SMALL_NO"])
    assert both_sides(ms, val["FITC_SMALL_M"])
    # an append carries a handle across 128 and across 256
    grown = [(s[0], s[0] + s[1][0]) for s in g.APPEND_ALL]
    assert any(a <= 128 < b for a, b in grown) and any(a <= 256 < b for a, b in grown)
    # M = n + n_out on both sides of a 64-row tile, read from the plans; every SUMSQ kind
    from gp_mpc_rocket_landing_amd import _lib
    tiles, kinds, paths = {}, set(), set()
    for s in g.EXACT_ALL:
        nrt, kind = plans(s[0] + s[1], s[4], s[0])
        tiles.setdefault(nrt, []).append(s[:2])
        kinds.add(kind)
        paths.add(_lib.gemm_plan("sumsq_mean", s[0], s[4], s[0], p0=-1, p1=s[1])[0])
    print({k: v[:3] for k, v in tiles.items()}, kinds, paths)
    assert kinds == {0, 1, 2} and paths == {"64", "128", "splitk"}, (kinds, paths)
    assert {1, 2} <= set(tiles) and any(t >= 4 for t in tiles)
    for a, b in (((61, 3), (62, 3)), ((127, 1), (126, 3))):
        assert plans(sum(a), 1, a[0])[0] + 1 == plans(sum(b), 1, b[0])[0]
    # the GEMM form of the sparse posterior sums two partial buffers: both tile counts change
    assert {plans(s[1], s[5], s[1])[0] for s in g.SPARSE_ALL} >= {1, 2, 3}
