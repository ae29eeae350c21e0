"""The rules of tests/chol_check.py, without a GPU: they accept float64 restatements of every
algorithm form of the batched Cholesky, the triangular solves and the solve helpers (and
LAPACK's results), on every family, and reject each of them made subtly wrong.  The exact
family's claim -- every order of the operations is exact -- is checked here too, and the
factor runs of tests/test_gpu_chol.py are read back through gpmpc_potrf_plan (no device) for
what they cover."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chol_check as cc  # noqa: E402
import gemm_check as gc  # noqa: E402

FORMS = [(kind, left) for kind in cc.KINDS for left in (False, True) if not (kind == "col32" and left)]
needs_ld = pytest.mark.skipif(not gc.longdouble_ok(), reason="numpy longdouble is no finer than float64")


@needs_ld
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_factor_rule_accepts_restatements_and_lapack(family):
    """Left- and right-looking, 128-inverse, 32-inverse TRSM form, the per-block inverse form
    and the 32-column form, and LAPACK: all inside the bound with a factor 2 to spare."""
    worst = {}
    for n in (1, 33, 129, 300):
        A = cc.factor_mats(family, n, 2)
        for b in range(2):
            for kind, left in FORMS:
                # longdouble at every size for one member, float64 (c1 doubled) for the other
                r = cc.factor_ratio(A[b], cc.restate_potrf(A[b], kind, left), kind, longdouble=b == 0)
                worst[kind] = max(worst.get(kind, 0.0), r)
                assert r <= 0.5, (family, n, kind, left, r)
            r = cc.factor_ratio(A[b], np.linalg.cholesky(A[b]), "inv128", longdouble=b == 0)
            worst["lapack"] = max(worst.get("lapack", 0.0), r)
            assert r <= 0.5, (family, n, "lapack", r)
    print(family, {k: f"{v:.3g}" for k, v in worst.items()})


def test_factor_rule_float64_evaluation_at_the_largest_size():
    for family in cc.FAMILIES:
        A = cc.factor_mats(family, 420, 1)[0]
        for kind, left in FORMS:
            assert cc.factor_ratio(A, cc.restate_potrf(A, kind, left), kind, longdouble=False) <= 0.5
        if gc.longdouble_ok():   # the figures DESIGN.md quotes beside the device's
            lap = cc.factor_ratios(A, np.linalg.cholesky(A), "inv128")[1]
            inv = cc.factor_ratios(A, cc.restate_potrf(A, "inv128"), "inv128")[1]
            print(f"{family} n 420: max |A - L L^T| / (u |L| |L^T|): LAPACK {lap:.3g}, 128-inverse restatement {inv:.3g}")


def test_explicit_inverse_term_is_needed_and_sufficient():
    """On the GP family the 128-inverse restatement misses c1 u |L| |L^T| alone by far (the
    panel solve is only conditionally backward stable) and LAPACK does not: the second term
    of the rule is what the inverse forms are entitled to, and nothing else is."""
    A = cc.factor_mats("gp8", 420, 1)[0]
    Lr = np.tril(cc.restate_potrf(A, "inv128"))
    low = np.tril(np.ones(A.shape, bool))

    def plain_ratio(L):
        return np.max((np.abs(A - L @ L.T) / (cc.U * (np.abs(L) @ np.abs(L).T)))[low])

    Ll = np.linalg.cholesky(A)
    plain, lap = plain_ratio(Lr), plain_ratio(Ll)
    print(f"gp8 n 420: max |A - L L^T| / (u |L| |L^T|): 128-inverse restatement {plain:.0f}, LAPACK {lap:.1f}")
    assert lap < 100 < plain
    # a LAPACK-grade factor is not granted the inverse term where no inverse was used
    assert cc.factor_ratio(A, Ll, "inv128", longdouble=False) <= 0.5


# ---- mutants of the factor ------------------------------------------------------------------
def factor_cases():
    out = []
    for i, (family, n, batch) in enumerate([("wishart", 300, 3), ("graded", 257, 2), ("gp8", 300, 2),
                                            ("gp6", 129, 2), ("wishart", 33, 3)]):
        out.append(cc.FactorCase(cc.factor_mats(family, n, batch), cc.LAYOUTS[i % 4], tag=f"{family} {n} b{batch}"))
    return out


def test_factor_rule_rejects_every_mutant():
    cc.restate_potrf.met.clear()
    info0 = lambda c: [0] * c.batch  # noqa: E731
    seen = {m: 0 for m in cc.MUTANTS}
    for case in factor_cases():
        for kind, left in FORMS:
            ld = (kind, left) in (("inv128", False), ("trsm32", True))   # elsewhere the float64 evaluation
            assert not case.verify(case.perfect_after(kind, left), info0(case), kind, longdouble=ld), (case.tag, kind)
            for m in cc.MUTANTS:
                before = cc.restate_potrf.met.get(m, 0)
                after = case.perfect_after(kind, left, (m, 1))
                if cc.restate_potrf.met.get(m, 0) == before:
                    continue   # the mutant does not apply to this case (no ragged block, one block, ...)
                seen[m] += 1
                assert case.verify(after, info0(case), kind, longdouble=ld), (case.tag, kind, left, m, "accepted")
    assert all(v >= 4 for v in seen.values()), seen
    print("mutants met and rejected:", seen)


def test_factor_case_checks_info_and_the_poisoned_surroundings():
    A = cc.factor_mats("wishart", 33, 3)
    case = cc.FactorCase(np.stack([A[0], cc.bad_matrix(A[1], 32, -1.0), A[2]]), "odd", bad={1: 32}, tag="t")
    after = case.perfect_after("col32")
    assert not case.verify(after, [0, 32, 0], "col32")
    assert case.verify(after, [0, 33, 0], "col32") and case.verify(after, [0, 0, 0], "col32")
    for i in (0, case.buf.offset - 1, case.buf.idx[0, 0, 5], case.buf.offset + case.buf.stride - 1, case.buf.size - 1):
        hit = after.copy()
        hit[i] = 1.0    # the band, the strict upper triangle, the stride gap
        assert case.verify(hit, [0, 32, 0], "col32"), i
    neg = after.copy()
    neg[case.buf.idx[2, 7, 7]] *= -1.0
    assert any("diag" in m for m in case.verify(neg, [0, 32, 0], "col32"))


# ---- the triangular rules ---------------------------------------------------------------------
@pytest.mark.parametrize("family", cc.REAL_FAMILIES)
def test_triangular_rules_accept_restatements(family):
    worst = {}
    for n in (31, 129, 300, 385):
        L = cc.family_L(family, n)
        rng = np.random.default_rng(n)
        for trans in (False, True):
            for nrhs in (3, 65):
                B = rng.standard_normal((n, nrhs))
                for name, X in (("blocked", cc.restate_trsm(L, B, trans)),
                                ("lapack", cc.sla.solve_triangular(L, B, lower=True, trans="T" if trans else "N"))):
                    r = cc.trsm_ratio(L, B, X, trans)
                    worst[name] = max(worst.get(name, 0.0), r)
                    assert r <= 0.5, (family, n, trans, nrhs, name, r)
        Bl = np.tril(rng.standard_normal((n, n)))
        assert cc.trsm_ratio(L, Bl, cc.restate_trsm(L, Bl, False), False) <= 0.5
        W = cc.restate_tri_inverse(L)
        r = cc.tri_inverse_ratio(L, W)
        worst["doubling"] = max(worst.get("doubling", 0.0), r)
        assert r <= 0.5, (family, n, "tri_inverse", r)
        y = rng.standard_normal((n, 3))
        for name, a in (("potrs", cc.restate_potrs(L, y)), ("inv_refined", cc.restate_cho_solve_inv(L, W, y))):
            r = cc.cho_ratio(L, y, a)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 0.5, (family, n, name, r)
    print(family, {k: f"{v:.3g}" for k, v in worst.items()})


def test_inverse_solve_with_refinement_meets_the_substitutions_bound():
    """gp.hip's claim on the worst-conditioned family, in float64: the explicit-inverse solve
    with its refinement step is inside the bound of the two substitutions.  (So is the
    unrefined one here, by less: the bound carries |a^|, which is large where L is
    ill-conditioned; its ratio is printed beside the refined one.)"""
    L = cc.family_L("gp8", 385)
    y = np.random.default_rng(5).standard_normal((385, 3))
    W = cc.restate_tri_inverse(L)
    r0 = cc.cho_ratio(L, y, cc.restate_cho_solve_inv(L, W, y, refine=False))
    r1 = cc.cho_ratio(L, y, cc.restate_cho_solve_inv(L, W, y))
    print(f"gp8 n 385: cho_solve through W, residual / bound: unrefined {r0:.3g}, refined {r1:.3g}")
    assert r1 <= 0.5 and r1 < r0


@pytest.mark.parametrize("n", [1, 31, 33, 129, 300, 517])
def test_exact_family_is_exact_in_every_order(n):
    L, Linv = cc.integer_L(n)
    for nrhs in (1, 5, n):
        B = cc.integer_rhs(n, nrhs)
        cc.assert_exact_range(L, Linv, B)
        for trans in (False, True):
            want = (Linv.T if trans else Linv) @ B
            assert np.array_equal(cc.restate_trsm(L, B, trans), want)
            assert np.array_equal(cc.sla.solve_triangular(L, B, lower=True, trans="T" if trans else "N"), want)
            if gc.longdouble_ok():
                assert np.array_equal(np.matmul((Linv.T if trans else Linv).astype(cc.LD), B.astype(cc.LD)), want)
    Bl = cc.integer_rhs(n, n, lower=True)
    assert np.array_equal(cc.restate_trsm(L, Bl, False), Linv @ Bl)
    assert np.array_equal(np.triu(Linv @ Bl, 1), np.zeros((n, n)))
    assert np.array_equal(cc.restate_tri_inverse(L), Linv)
    y = cc.integer_rhs(n, 3)
    want = Linv.T @ (Linv @ y)
    assert np.array_equal(cc.restate_potrs(L, y), want)
    assert np.array_equal(cc.restate_cho_solve_inv(L, Linv, y), want)
    assert np.array_equal(y - L @ (L.T @ want), np.zeros_like(y))   # the refinement residual: exactly zero


def test_triangular_rules_reject_mutants():
    seen = {}

    def hit(name, rejected, what):
        seen[name] = seen.get(name, 0) + 1
        assert rejected, (name, what, "accepted")

    for family in cc.REAL_FAMILIES + ("integer",):
        for n in (129, 300, 385):
            if family == "integer":
                L, Linv = cc.integer_L(n)
                B = cc.integer_rhs(n, 65)
            else:
                L, B = cc.family_L(family, n), np.random.default_rng(n).standard_normal((n, 65))
            for trans in (False, True):
                case = cc.TriCase("trsm", L, B, 1 if trans else 0, variant="odd", tag="t",
                                  want=((Linv.T if trans else Linv) @ B) if family == "integer" else None)
                good = cc.restate_trsm(L, B, trans)
                assert not case.verify(case.after_with(good)), (family, n, trans)
                for m in ("previnv", "skiplast", "kslice"):
                    met = []
                    X = cc.restate_trsm(L, B, trans, m, met)
                    if met and not np.array_equal(X, good):   # (an all-zero slice dropped is no mutant)
                        hit(m, case.verify(case.after_with(X)), (family, n, trans))
                X = good.copy()
                X[n // 2, 7] *= 1.0 + 1e-9
                if X[n // 2, 7] != 0.0:
                    hit("nudge", case.verify(case.after_with(X)), (family, n, trans))
                X = good.copy()
                X[n - 1, 0] = np.nan
                hit("poison", case.verify(case.after_with(X)), (family, n, trans))
                after = case.after_with(good)
                after[id(case.bX)][cc.gap_index(case.bX)] = 0.0
                hit("gapwrite", case.verify(after), (family, n, trans))
                after = case.after_with(good)
                after[id(case.bL)][case.bL.idx[0, 3, 2]] += 1.0
                hit("inputwrite", case.verify(after), (family, n, trans))
            case = cc.TriCase("tri_inverse", L, np.eye(n), variant="even", tag="t",
                              want=Linv if family == "integer" else None)
            assert not case.verify(case.after_with(cc.restate_tri_inverse(L)))
            for m in ("previnv", "skiplast", "kslice"):
                met = []
                W = cc.restate_tri_inverse(L, m, met)
                if met and not np.array_equal(W, cc.restate_tri_inverse(L)):
                    hit("inv_" + m, case.verify(case.after_with(W)), (family, n))
            W = cc.restate_tri_inverse(L)
            W[n - 1, n // 3] *= 1.0 + 1e-9
            if W[n - 1, n // 3] != 0.0 and family != "gp8":
                # (on the worst-conditioned family an inverse accurate to 1e-9 is within what the
                # doubling form is entitled to: its bound carries cond(L_CC))
                hit("inv_nudge", case.verify(case.after_with(W)), (family, n))
            after = case.after_with(cc.restate_tri_inverse(L))
            after[id(case.bX)][case.bX.idx[0, 2, 9]] = 1e-300     # above the diagonal
            hit("inv_upper", case.verify(after), (family, n))
            y = B[:, :3]
            case = cc.TriCase("potrs_cols", L, y, variant="shift", tag="t",
                              want=(Linv.T @ (Linv @ y)) if family == "integer" else None)
            a = cc.restate_potrs(L, y)
            assert not case.verify(case.after_with(a)), (family, n, "potrs")
            a[n // 2, 1] *= 1.0 + 1e-9
            if a[n // 2, 1] != 0.0:
                hit("cho_nudge", case.verify(case.after_with(a)), (family, n))
    assert all(v >= 8 for v in seen.values()) and len(seen) == 13, seen
    print("mutants met and rejected:", seen)


# ---- what the GPU file's factor runs cover ------------------------------------------------------
def test_factor_runs_cover_every_form_step_and_mode():
    from gp_mpc_rocket_landing_amd import _lib
    plans = [_lib.potrf_plan(n, batch, **sw) if sw else _lib.potrf_plan(n, batch, **_lib.POTRF_POLICY)
             for _, sw, sizes in cc.FACTOR_RUNS for n, batch in sizes]
    have = cc.plan_coverage(plans)
    assert cc.COVERAGE <= have, sorted(cc.COVERAGE - have)
    kinds = {cc.plan_kind(*p) for p in plans}
    assert kinds == set(cc.KINDS)
    sizes = {(n, b) for name, _, ss in cc.FACTOR_RUNS if name.startswith("default") for n, b in ss}
    assert {(n, b) for n in cc.SIZES for b in (1, 3, 8, 17)} <= sizes and (300, 72) in sizes
