"""The Gram checker (tests/gram_check.py) accepts a float64 restatement of the kernels'
arithmetic on every case tests/test_gpu_gram.py runs and rejects subtly wrong kernels built
in numpy -- the evidence that the GPU tests would fail for a subtly wrong kernel -- and the
launcher's path table (gpmpc_gram_path) is what the GPU tests assume.  No GPU."""
import numpy as np
import pytest

import gram_check as gc

pytestmark = pytest.mark.skipif(not gc.longdouble_ok(), reason="numpy longdouble is no finer than float64 here")

GROUPS = ([("k_gram", d) for d in gc.WIDTHS] + [("k_gram_rows", d) for d in (11, 12, 13)])


def group_cases(path, d):
    specs = gc.kgram_specs(d) if path == "k_gram" else gc.rows_specs(d)
    return [gc.make_case(*s) for s in specs]


def shifted_columns(case, K):
    return np.roll(K, 1, axis=1) if case.n2 >= 2 else None


def swapped_rows(case, K):
    if case.n1 < 2:
        return None
    out = K.copy()
    out[[0, case.n1 - 1]] = out[[case.n1 - 1, 0]]
    return out


def last_feature_dropped(case, K):
    if case.n1 == 1 and case.X2 is None:
        return None   # one entry, d2 = 0 whatever the width
    if case.n1 * case.n2 == 1 and case.X1[0, -1] == case.X2[0, -1]:
        return None   # one pair of rows that does not differ in the last feature (integer inputs)
    if case.d == 1:
        return np.full_like(K, case.sigma2)   # no feature left: d2 = 0 everywhere
    return gc.restate(case, nfeat=case.d - 1)


def lengthscale_off_by_one(case, K):
    if case.kind == "se_iso" or case.d < 2 or (case.n1 == 1 and case.X2 is None):
        return None   # one lengthscale; one entry, d2 = 0 whatever the lengthscales
    return gc.restate(case, ls=np.roll(case.ls, -1))


def second_tile_from_first(case, K, tile):
    if case.n1 <= tile:
        return None
    return gc.restate(case, a_rows=lambda a: gc.first_tile_rows(a, tile))


def one_entry_nudged(case, K):
    out = K.copy()
    out[case.n1 // 2, case.n2 // 2] += 1e-9 * case.sigma2
    return out


def aliased_lds(case, K):
    if case.d < 2:
        return None   # [r][0] is where it belongs
    return gc.restate(case, a_rows=gc.aliased_rows)


@pytest.mark.parametrize("path,d", GROUPS)
def test_restatement_accepted_and_wrong_kernels_rejected(path, d):
    tile = 64 if path == "k_gram" else 128
    mutants = {"shifted_columns": shifted_columns, "swapped_rows": swapped_rows,
               "last_feature_dropped": last_feature_dropped, "lengthscale_off_by_one": lengthscale_off_by_one,
               "second_tile_from_first": lambda c, K: second_tile_from_first(c, K, tile),
               "one_entry_nudged": one_entry_nudged, "aliased_lds": aliased_lds}
    applied = dict.fromkeys(mutants, 0)
    worst = 0.0
    for case in group_cases(path, d):
        K = gc.restate(case)
        assert gc.check_gram(case, K) == [], case.tag
        worst = max(worst, gc.worst_ratio(K, case.ref, case.bound))
        for name, f in mutants.items():
            bad = f(case, K)
            if bad is None:
                continue
            applied[name] += 1
            assert gc.check_gram(case, bad) != [], (case.tag, name)
    print(f"{path} d {d}: the restatement's max |err| / bound = {worst:.3g}")
    # every mutant met cases of this group (those the shape or the kind leaves out aside)
    assert applied["one_entry_nudged"] > 0 and applied["swapped_rows"] > 0 and applied["last_feature_dropped"] > 0
    assert applied["shifted_columns"] > 0 and applied["second_tile_from_first"] > 0
    assert (applied["aliased_lds"] > 0 and applied["lengthscale_off_by_one"] > 0) or d == 1


@pytest.mark.parametrize("kind", ["se_ard", "se_iso"])
def test_gradient_restatement_accepted_and_wrong_planes_rejected(kind):
    worst = 0.0
    for spec in gc.grad_specs(kind):
        case = gc.make_case(*spec, grad=True)
        K = gc.restate(case)
        G = gc.restate_grad(case, K)
        assert gc.check_gram(case, K) == [] and gc.check_grad(case, G) == [], case.tag
        worst = max(worst, gc.worst_ratio(G, case.gref, case.gbound))
        if G.shape[0] >= 2:   # plane i holding plane i - 1
            assert gc.check_grad(case, np.roll(G, 1, axis=0)) != [], case.tag
        nudged = G.copy()
        nudged[-1, case.n1 // 2, case.n2 // 2] += 1e-9 * case.sigma2
        assert gc.check_grad(case, nudged) != [], case.tag
        if case.d >= 2:       # planes formed from a K with the aliased a-rows
            assert gc.check_grad(case, gc.restate_grad(case, gc.restate(case, a_rows=gc.aliased_rows))) != [], case.tag
    print(f"k_gram_grad {kind}: the restatement's max |err| / bound = {worst:.3g}")


def test_exact_family_allows_only_the_relative_term():
    """Integer inputs, power-of-two lengthscales, sigma2 = 1: d2 is exact in fp64, so the
    bound is (8 + 4 s) u |K_ref| and the restatement's d2 equals the reference's."""
    for kind in gc.KINDS:
        case = gc.make_case(kind, 65, 63, 14, "integer")
        assert case.exact and not np.any(case.e_d2)
        assert np.array_equal(case.bound, (8 + 4 * case.s) * gc.U * np.abs(case.ref))
        a, na = gc.scale_rows(kind, case.X1, case.ls)
        b, nb = gc.scale_rows(kind, case.X2, case.ls)
        d2 = (na[:, None] + nb[None, :]) - 2.0 * (a @ b.T)
        ls = np.ones(case.d) if kind == "se_iso" else case.ls
        assert np.array_equal(d2.astype(gc.LD), gc.sqdist_planes(case.X1, case.X2, ls).sum(axis=0))


def test_badly_scaled_case_is_refused():
    """Unit lengthscales at d = 32: every entry is about e^-32 and an absolute bound would
    pass any kernel; the builder refuses the case."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((20, 32))
    with pytest.raises(AssertionError, match="badly scaled"):
        gc.Case("se_ard", X, None, np.ones(32), 1.0, "centred")


def test_poisoned_or_nan_entry_is_rejected():
    case = gc.make_case("se_ard", 63, 65, 3, "centred")
    K = gc.restate(case)
    K[62, 64] = gc.poison(1)[0]
    assert len(gc.check_gram(case, K)) == 1
    case = gc.make_case("matern32", 65, None, 3, "cluster")
    K = gc.restate(case)
    K[7, 7] = np.nextafter(case.sigma2, 0.0)   # one ulp under sigma2 on the diagonal
    assert gc.violations(K, case.ref, case.bound, case.tag) == [] and len(gc.check_gram(case, K)) == 1


def test_gp_case_needs_no_jitter():
    """The d = 3 GP of test_gpu_gram.py factors at jitter ladder step 0 in the oracle, for
    the fit and for every parameter set of the batched LML."""
    from oracle import gp_oracle
    X, Y, ls, s2, noise, _ = gc.gp_case()
    assert X.shape == (70, 3)
    K = gp_oracle.gram("se_ard", X, None, s2, ls)
    assert gp_oracle.chol_with_jitter(K + noise * np.eye(70))[1] == 0
    assert gp_oracle.exact_fit(X, Y, sigma2=s2, ls=ls, noise=noise)["jitter_steps"] == 0
    assert np.linalg.cond(K + noise * np.eye(70)) < 70 * s2 / noise


def test_path_table():
    """gpmpc_gram_path, the value launch_gram branches on: k_gram<11 / 12 / 13> for those
    widths and the runtime-width instantiation for every other one; k_gram_rows from 512
    rows at widths 11..13 only; a transposed output always k_gram.  Every case of
    test_gpu_gram.py lies on the path it is meant for."""
    from gp_mpc_rocket_landing_amd import _lib
    for d in range(1, 33):
        D = d if 11 <= d <= 13 else 0
        for n1 in (511, 512, 513):
            want = ("k_gram_rows", D) if n1 >= 512 and D else ("k_gram", D)
            assert _lib.gram_path(n1, d) == want, (n1, d)
            assert _lib.gram_path(n1, d, 1) == ("k_gram", D), (n1, d)
        for n1 in (0, 1, 64, 129):
            assert _lib.gram_path(n1, d) == ("k_gram", D)
    for d in gc.WIDTHS:
        assert all(_lib.gram_path(s[1], d)[0] == "k_gram" for s in gc.kgram_specs(d))
    for d in (11, 12, 13):
        assert all(_lib.gram_path(s[1], d) == ("k_gram_rows", d) for s in gc.rows_specs(d))
    for bad in ((10, 0), (10, 33), (-1, 11)):
        assert _lib._L.gpmpc_gram_path(bad[0], bad[1], 0) == -2
        with pytest.raises(_lib.HIPError):
            _lib.gram_path(*bad)
