"""The GEMM launchers' dispatch, read without a GPU through gpmpc_gemm_plan (the same
gemm_plan that the launchers of csrc/gemm.hip execute, csrc/gemm_plan.h): a differential test
against the rule as it stood before the plan existed (tests/gemm_plan_oracle.py) over a full
sweep of requests and switches; invariants of every plan over the same sweep; every
(path, split, grid) that tests/test_gpu_gemm.py asserts, pinned; the switch names and the
binding; and the one tile-height rule of the SUMSQ partial buffer (gemm_row_tiles = the
launcher's pick).

A plan is (path, split, grid, gx, gy, gz, tile height, kc) -- include/gpmpc.h."""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_plan_oracle as oracle  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gp_mpc_rocket_landing_amd", "csrc")
NO_SCRATCH = 8   # GPMPC_GEMM_NO_SCRATCH
DEFAULT = {"big": 1, "kmin": 256, "splitk": 1, "syrk128": -1, "streamk": -1, "ksplit": 0, "remap": 0, "xcd_batch": 1,
           "rowblock_xcd": 1, "post_xcd": 0}
# the default policy and each single switch moved off its default
MOVED = [("big", 0), ("kmin", 512), ("splitk", 0), ("syrk128", 0), ("syrk128", 1), ("streamk", 0), ("streamk", 1),
         ("ksplit", 3), ("remap", 1), ("xcd_batch", 0), ("rowblock_xcd", 0), ("post_xcd", 1)]
POLICIES = [{}] + [{k: v} for k, v in MOVED]
DIMS = [0, 1, 32, 33, 64, 65, 255, 256, 257, 511, 512, 767, 768, 1023, 1024, 1100, 4000]
BATCHES = [1, 2, 8, 11, 16]
BETAS = [0.0, 0.5, 1.0]
FIELDS = ("op", "M", "N", "K", "batch", "beta", "flags", "p0", "p1")


def pol_id(p):
    return "-".join(f"{k}{v}" for k, v in p.items()) or "default"


# ---- the sweep: every request the launchers' contracts allow over the grids above --------------

def _product(**axes):
    grids = np.meshgrid(*[np.asarray(v) for v in axes.values()], indexing="ij")
    return {k: g.ravel() for k, g in zip(axes, grids)}


@functools.lru_cache(maxsize=None)
def sweep():
    """The requests as the arguments of gpmpc_gemm_plan, pruned by the contracts
    gpmpc_gemm_diag enforces (include/gpmpc.h) and by nothing else."""
    O = oracle
    parts = []
    # NT: any batch; tri_a only with beta != 1 and K <= M; lower_c free
    r = _product(M=DIMS, N=DIMS, K=DIMS, batch=BATCHES, beta=BETAS, flags=[0, 1, 2, 3])
    keep = ((r["flags"] & 1) == 0) | ((r["beta"] != 1.0) & (r["K"] <= r["M"]))
    parts.append(dict({k: v[keep] for k, v in r.items()}, op=O.NT, p0=0, p1=0))
    # NN, TN: batch 1, no flags; NN_BATCHED: any batch
    for op, batches in ((O.NN, [1]), (O.TN, [1]), (O.NN_BATCHED, BATCHES)):
        parts.append(dict(_product(M=DIMS, N=DIMS, K=DIMS, batch=batches, beta=BETAS), op=op, flags=0, p0=0, p1=0))
    # ROWBLOCK: N <= 128, lower_c free, ksplit 3 only with beta = 1
    r = _product(M=DIMS, N=[n for n in DIMS if n <= 128], K=DIMS, batch=BATCHES, beta=BETAS, flags=[0, 2], p0=[1, 3])
    keep = (r["p0"] == 1) | (r["beta"] == 1.0)
    parts.append(dict({k: v[keep] for k, v in r.items()}, op=O.ROWBLOCK, p1=0))
    # SUMSQ / SUMSQ_MEAN: K == M, batch 1, no flags, every forced kind; 3 mean rows
    for op, n_out in ((O.SUMSQ, 0), (O.SUMSQ_MEAN, 3)):
        r = _product(M=DIMS, N=DIMS, beta=BETAS, p0=[-1, 0, 1, 2])
        parts.append(dict(r, K=r["M"], op=op, batch=1, flags=0, p1=n_out))
    n = [len(p["M"]) for p in parts]
    out = {k: np.concatenate([np.broadcast_to(np.asarray(p[k]), (m,)) for p, m in zip(parts, n)]) for k in FIELDS}
    return {k: v.astype(np.float64 if k == "beta" else np.int64) for k, v in out.items()}


def oracle_request(req, no_scratch=0):
    return dict(op=req["op"], M=req["M"], N=req["N"], K=req["K"], batch=req["batch"], beta1=req["beta"] == 1.0,
                tri_a=req["flags"] & 1, lower_c=(req["flags"] >> 1) & 1, p0=req["p0"], p1=req["p1"],
                no_scratch=np.full(len(req["op"]), no_scratch))


def c_plans(req, policy, extra_flags=0):
    """gpmpc_gemm_plan for every request (policy: a dict over the default policy, None: the
    process's switches): an (n, 8) array.  Every call must return 0."""
    from gp_mpc_rocket_landing_amd import _lib
    c = ctypes.c_int
    f = ctypes.CFUNCTYPE(c, c, c, c, c, c, ctypes.c_double, c, c, c, ctypes.c_void_p, ctypes.c_void_p)(
        ctypes.cast(_lib._L.gpmpc_gemm_plan, ctypes.c_void_p).value)
    n = len(req["op"])
    out = np.full((n, 8), -9, np.int32)
    pol = np.array(list(dict(_lib.GEMM_POLICY, **(policy or {})).values()), np.int32)
    pa = [pol.ctypes.data if policy is not None else None] * n
    cols = [req[k].tolist() for k in FIELDS]
    cols[6] = (req["flags"] | extra_flags).tolist()
    rcs = set(map(f, *cols, pa, range(out.ctypes.data, out.ctypes.data + 32 * n, 32))) if n else {0}
    assert rcs == {0}, rcs
    return out.astype(np.int64)


@pytest.fixture(scope="module", params=POLICIES, ids=pol_id)
def swept(request):
    """(policy, the plans of the whole sweep under it): computed once for the tests that read it."""
    return request.param, c_plans(sweep(), request.param)


def describe(req, i):
    return {k: req[k][i].item() for k in FIELDS}


# ---- 1. differential: the plan against the rule it replaced ------------------------------------

def test_the_sweep_is_whole():
    req = sweep()
    n = len(req["op"])
    d, b = len(DIMS), len(BATCHES)
    tri = sum(1 for M in DIMS for K in DIMS if K <= M)   # (M, K) pairs a triangular A allows
    want = (d ** 3 * b * 3 * 2 + d * tri * b * 2 * 2      # NT: lower_c free; tri_a with beta != 1, K <= M
            + 2 * d ** 3 * 3 + d ** 3 * b * 3             # NN, TN, NN_BATCHED
            + d * 6 * d * b * 2 * (3 + 1)                 # ROWBLOCK: ksplit 3 with beta = 1 only
            + 2 * d * d * 3 * 4)                          # SUMSQ, SUMSQ_MEAN
    print(f"requests per policy: {n}; compared in all: {n * (len(POLICIES) + 1)}")
    assert n == want and len(POLICIES) == 13


def test_plan_is_the_parents_decision(swept):
    policy, got = swept
    req = sweep()
    want = oracle.decide(oracle_request(req), dict(DEFAULT, **policy))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(bad), [(describe(req, i), got[i].tolist(), want[i].tolist()) for i in bad[:5]])


def test_plan_without_scratch_is_the_parents_fall_through():
    req = sweep()
    got, want = c_plans(req, {}, NO_SCRATCH), oracle.decide(oracle_request(req, 1), DEFAULT)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(bad), [(describe(req, i), got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    assert not (got[:, 0] == oracle.PATH_SPLITK).any()


# ---- 2. invariants over the same sweep -----------------------------------------------------------

def test_plan_invariants_over_the_sweep(swept):
    O = oracle
    policy, p = swept
    req = sweep()
    path, split, grid, gx, gy, gz, tile, kc = p.T
    op, M, N, K, beta1 = req["op"], req["M"], req["N"], req["K"], req["beta"] == 1.0
    tri_a, lower_c = req["flags"] & 1, (req["flags"] >> 1) & 1
    sumsq = (op == O.SUMSQ) | (op == O.SUMSQ_MEAN)

    def holds(name, ok):
        bad = np.flatnonzero(~ok)
        assert not len(bad), (name, len(bad), [(describe(req, i), p[i].tolist()) for i in bad[:5]])

    Mi = M + req["p1"]   # the SUMSQ_MEAN product's rows
    empty = (Mi == 0) | (N == 0)
    holds("empty products launch nothing", (path == O.PATH_NONE) == empty)
    holds("a non-empty product has a grid", empty | (gx * gy * gz >= 1))
    holds("tile heights", np.isin(tile, (64, 128)) & ((tile == 128) == np.isin(path, (1, 2, 3))))
    # a forced SUMSQ kind is the kernel's tile height, whatever the size and the switches
    # (an empty product writes no partial row)
    forced = sumsq & (req["p0"] >= 0) & ~empty
    holds("forced kinds", ~forced | (O.cdiv(Mi, tile) == np.where(req["p0"] == 1, O.cdiv(Mi, 128), O.cdiv(Mi, 64))))
    holds("forced 128", ~forced | ((req["p0"] == 1) == (path == O.PATH_128)))
    s = path == O.PATH_SPLITK
    holds("skinny splits", ~s | ((kc % 16 == 0) & (kc > 0) & ((split - 1) * kc < K) & (K <= split * kc) & (split >= 2)
                                 & (gz == split)))
    holds("kc only with a skinny split", s | (kc == 0))
    k = path == O.PATH_128_KSPLIT
    holds("a K split accumulates", ~k | (~sumsq & beta1 & (split > 1)))
    holds("one pass otherwise", k | s | (path == O.PATH_STREAMK) | empty | (split == 1))
    auto = k & (op == O.NT) & (dict(DEFAULT, **policy)["ksplit"] == 0)
    holds("the cost model's splits", ~auto | ((K // np.maximum(split, 1) >= 256) & (split <= 16)))
    holds("split <= 16", ~k | (split <= 16))
    sk = path == O.PATH_STREAMK
    holds("stream-K", ~sk | ((op == O.NT) & beta1 & (split >= 1) & (split <= 512) & (gx == split)))
    holds("the triangular grids", ~np.isin(grid, (O.GRID_TRI, O.GRID_XCD_BATCH))
          | ((op == O.NT) & (lower_c == 1) & (M == N) & (tri_a == 0)))
    holds("the row-block grid", (grid != O.GRID_ROWBLOCK_XCD) | (op == O.ROWBLOCK))


def test_sumsq_tile_height_is_what_the_consumers_count():
    """Under the process's switches: the plan's tile height for an automatic SUMSQ request is
    gemm_sumsq_rows of the kind gemm_row_tiles reports, its path that kind's kernel, and
    neither moves when the split-K scratch is not to be had."""
    from gp_mpc_rocket_landing_amd import _lib
    O = oracle
    req = sweep()
    sel = ((req["op"] == O.SUMSQ) | (req["op"] == O.SUMSQ_MEAN)) & (req["beta"] == 0.0)
    req = {k: v[sel] for k, v in req.items()}
    p, dry = c_plans(req, None), c_plans(req, None, NO_SCRATCH)
    assert len(p) == 2 * 17 * 17 * 4 and (p[:, 6] == dry[:, 6]).all()
    for i in range(len(p)):
        Mi, N, K, forced = int(req["M"][i] + req["p1"][i]), int(req["N"][i]), int(req["K"][i]), int(req["p0"][i])
        rows, auto = _lib.gemm_row_tiles(Mi, N, K) if Mi else (0, 0)
        kind = forced if forced >= 0 else auto
        if not (Mi and N):
            assert p[i, 0] == dry[i, 0] == O.PATH_NONE   # no partial row is written
            continue
        assert O.cdiv(Mi, int(p[i, 6])) == _lib.gemm_sumsq_rows(kind, Mi), describe(req, i)
        if forced < 0:
            assert rows == O.cdiv(Mi, int(p[i, 6])) and p[i, 0] == {0: 0, 1: 1, 2: 4}[auto], describe(req, i)


# ---- 3. every (path, split, grid) tests/test_gpu_gemm.py asserts -------------------------------------
# (arguments of _lib.gemm_plan, (path, split, grid)); None: not asserted there

def nt(M, N, K, batch=1, beta=0.0, tri_a=0, lower_c=0):
    return ("nt", M, N, K, batch, beta, tri_a | 2 * lower_c, 0, 0)


def rb(M, N, K, batch, beta, lower_c, p0):
    return ("rowblock", M, N, K, batch, beta, 2 * lower_c, p0, 0)


def sq(n, P, kind, n_out):
    return ("sumsq_mean" if n_out else "sumsq", n, P, n, 1, 0.0, 0, kind, n_out)


GPU_CASES = (
    # test_nt_64_tile
    [(nt(*shp, beta=b), ("64", 1, "2d")) for shp in [(1, 1, 1), (63, 65, 17), (64, 64, 16), (65, 63, 15)]
     for b in BETAS]
    + [(nt(100, 130, 0, beta=0.5), ("64", None, None)), (nt(100, 130, 0, beta=0.0), ("64", None, None)),
       (nt(100, 130, 0, batch=3, beta=1.0), ("64", None, None))]
    + [(nt(130, 70, 300, batch=3, beta=b), ("64", 1, "2d")) for b in BETAS]
    # test_nt_64_tile_lower
    + [(nt(130, 130, 40, batch=batch, beta=b, lower_c=1), ("64", 1, grid))
       for batch, grid in ((3, "tri"), (8, "xcd_batch"), (11, "xcd_batch")) for b in (1.0, 0.0, 0.5)]
    + [(nt(130, 64, 40, batch=3, beta=1.0, lower_c=1), ("64", 1, "2d"))]
    # test_nt_128_tile
    + [(nt(256, 256, 256), ("128", 1, "2d")), (nt(300, 257, 260, beta=0.5), ("128", 1, "2d")),
       (nt(385, 383, 271, batch=2, beta=-1.0), ("128", 1, "2d")), (nt(385, 383, 271, batch=2, beta=2.0), ("128", 1, "2d"))]
    # test_nt_128_tile_k_split
    + [(nt(300, 300, 1100, beta=1.0), ("128_ksplit", 4, "2d")),
       (nt(300, 300, 1100, beta=1.0, lower_c=1), ("128_ksplit", 4, "tri")),
       (nt(300, 300, 1100, beta=0.5), ("128", 1, "2d"))]
    # test_nt_stream_k
    + [(nt(770, 769, 520, beta=1.0), ("streamk", 512, "2d")),
       (nt(770, 770, 520, batch=2, beta=1.0, lower_c=1), ("streamk", 512, "tri"))]
    # test_nt_skinny_split_k
    + [(nt(*shp, beta=b), ("splitk", None, None)) for shp in [(3, 700, 1000), (700, 3, 1000), (32, 33, 257)]
       for b in BETAS]
    + [(nt(32, 33, 257, beta=0.5), ("splitk", 4, None)), (nt(33, 33, 257), ("64", None, None)),
       (nt(32, 33, 255), ("64", None, None)), (nt(32, 33, 257, batch=2), ("64", None, None))]
    # test_nt_triangular_a
    + [(nt(130, 70, 130, beta=b, tri_a=1), ("64", None, None)) for b in (0.0, 0.5)]
    + [(nt(300, 260, 300, beta=b, tri_a=1), ("128", None, None)) for b in (0.0, 0.5)]
    # test_nt_alignment
    + [(nt(65, 63, 15, batch=3, beta=0.5), ("64", 1, "2d")),
       (nt(130, 130, 40, batch=11, beta=1.0, lower_c=1), ("64", 1, "xcd_batch")),
       (nt(300, 257, 260, batch=2, beta=0.5), ("128", 1, "2d")), (nt(32, 33, 257, beta=1.0), ("splitk", 4, None))]
    # test_nn_tn
    + [((form, *shp, batch, b, 0, 0, 0), (path, None, None))
       for form, batch, skinny in (("nn", 1, (3, 130, 520)), ("nn_batched", 3, (3, 130, 520)), ("tn", 1, (130, 3, 520)))
       for shp, path in (((65, 63, 17), "64"), ((129, 258, 128), "64"), (skinny, "splitk" if batch == 1 else "64"))
       for b in BETAS]
    # test_rowblock
    + [(rb(*shp, batch, b, lower, p0), ("128_ksplit" if p0 == 3 else "128", p0, grid))
       for batch, grid in ((3, "2d"), (8, "rowblock_xcd"), (16, "rowblock_xcd"))
       for shp in [(129, 100, 37), (300, 128, 128), (300, 128, 384)] for lower in (0, 1)
       for b, p0 in ((0.0, 1), (0.5, 1), (1.0, 1), (1.0, 3))]
    # test_sumsq: sumsq_path spelled out (the K split takes n = 300 with P <= 64 only)
    + [(sq(n, Pq, kind, n_out),
        ("128" if kind == 1 else "splitk" if kind == 2 and n == 300 and Pq <= 64 else "64", None, None))
       for kind in (0, 1, 2) for n_out in (0, 3) for n in (1, 64, 65, 130, 300) for Pq in (1, 20, 64, 65, 300)]
)
# test_switch_forced_paths: CHILD_ENV as explicit policies
GPU_CHILD_CASES = {
    "plain_grids": ({"splitk": 0, "xcd_batch": 0, "rowblock_xcd": 0}, [
        (nt(3, 700, 1000, beta=1.0), ("64", 1, "2d")), (nt(32, 33, 257, beta=0.5), ("64", 1, "2d")),
        (("tn", 130, 3, 520, 1, 0.0, 0, 0, 0), ("64", None, None)),
        (("nn", 3, 130, 520, 1, 0.5, 0, 0, 0), ("64", None, None)),
        (nt(130, 130, 40, batch=11, beta=1.0, lower_c=1), ("64", 1, "tri")),
        (rb(129, 100, 37, 8, 1.0, 1, 3), ("128_ksplit", 3, "2d")),
        (sq(300, 20, 2, 3), ("64", None, None)), (sq(300, 20, -1, 3), ("64", None, None))]),
    "small_tiles": ({"big": 0}, [
        (nt(300, 257, 260, beta=0.5), ("64", 1, "2d")), (nt(300, 300, 1100, beta=1.0, lower_c=1), ("64", 1, "tri")),
        (nt(300, 260, 300, tri_a=1), ("64", None, None)),
        (sq(300, 300, -1, 3), ("64", None, None)), (sq(300, 300, 1, 3), ("128", None, None))]),
    "forced_k_split": ({"streamk": 0, "ksplit": 3, "syrk128": 1}, [
        (nt(300, 257, 260, beta=1.0), ("128_ksplit", 3, "2d")),
        (nt(300, 300, 260, batch=2, beta=1.0, lower_c=1), ("128_ksplit", 3, "tri")),
        (nt(300, 300, 260, batch=2, beta=0.5, lower_c=1), ("128", 1, "tri")),
        (nt(130, 130, 40, batch=3, beta=1.0, lower_c=1), ("64", 1, "tri"))]),
}


def check_cases(cases, policy):
    from gp_mpc_rocket_landing_amd import _lib
    bad = []
    for args, want in cases:
        got = _lib.gemm_plan(*args, **dict(DEFAULT, **policy))[:3]
        if any(w is not None and w != g for w, g in zip(want, got)):
            bad.append((args, got, want))
    assert not bad, bad[:10]


def test_gpu_cases_take_the_paths_their_tests_claim():
    assert len(GPU_CASES) > 250
    check_cases(GPU_CASES, {})


@pytest.mark.parametrize("name", sorted(GPU_CHILD_CASES))
def test_gpu_switch_cases_take_the_paths_their_tests_claim(name):
    import test_gpu_gemm
    policy, cases = GPU_CHILD_CASES[name]
    env_of = {v: k for k, v in ENV_OF.items()}
    assert {env_of[k]: int(v) for k, v in test_gpu_gemm.CHILD_ENV[name].items()} == policy
    check_cases(cases, policy)


# ---- 4. the binding, the switches' names, one reader -------------------------------------------------

ENV_OF = {"big": "GPMPC_GEMM128", "kmin": "GPMPC_GEMM128_KMIN", "splitk": "GPMPC_SPLITK", "syrk128": "GPMPC_SYRK128",
          "streamk": "GPMPC_STREAMK", "ksplit": "GPMPC_KSPLIT", "remap": "GPMPC_GEMM_REMAP",
          "xcd_batch": "GPMPC_XCD_BATCH", "rowblock_xcd": "GPMPC_ROWBLOCK_XCD", "post_xcd": "GPMPC_POST_XCD"}


def test_binding_matches_the_headers():
    from gp_mpc_rocket_landing_amd import _lib
    src = open(os.path.join(CSRC, "gemm_plan.h")).read()
    body = re.search(r"struct GemmPolicy \{(.*?)\n\};", src, re.S).group(1)
    fields = [(k, int(v)) for k, v in re.findall(r"^\s*int (\w+) = (-?\d+);", body, re.M)]
    assert fields == list(_lib.GEMM_POLICY.items()) == list(DEFAULT.items())
    # each field's comment names its switch, and gemm_policy_env reads that name into it
    assert dict(re.findall(r"^\s*int (\w+) = -?\d+;\s*// (GPMPC_\w+):", body, re.M)) == ENV_OF
    reads = re.findall(r'p\.(\w+) = gpmpc_env_int\("(GPMPC_\w+)", ([^)]+)\);', src)
    assert [(f, e) for f, e, _ in reads] == list(ENV_OF.items())
    assert [int(eval(d, {"GEMM_BT": 128})) for _, _, d in reads] == list(DEFAULT.values())
    hdr = open(os.path.join(REPO, "include", "gpmpc.h")).read()
    assert int(re.search(r"#define GPMPC_GEMM_POLICY_N (\d+)", hdr).group(1)) == len(fields)
    assert int(re.search(r"#define GPMPC_GEMM_PLAN_INTS (\d+)", hdr).group(1)) == 8
    assert int(re.search(r"GPMPC_GEMM_NO_SCRATCH = (\d+)", hdr).group(1)) == NO_SCRATCH == _lib.GEMM_NO_SCRATCH
    assert "gpmpc_gemm_plan" in _lib.EXPORTED
    assert (oracle.NT, oracle.NN, oracle.NN_BATCHED, oracle.TN, oracle.ROWBLOCK, oracle.SUMSQ, oracle.SUMSQ_MEAN) == \
        tuple(_lib.GEMM_OP[k] for k in ("nt", "nn", "nn_batched", "tn", "rowblock", "sumsq", "sumsq_mean"))


# one request per switch whose plan the switch moves (post_xcd moves only the 128-tile SUMSQ
# kernel's mapping argument, which the eight reported ints do not carry: its reader is pinned
# by test_binding_matches_the_headers alone)
PROBES = [nt(300, 257, 260), nt(32, 33, 257), nt(300, 300, 260, batch=2, beta=0.5, lower_c=1),
          nt(300, 300, 1100, beta=0.5, lower_c=1),
          nt(770, 769, 520, beta=1.0), nt(300, 300, 300, beta=1.0), nt(300, 257, 260, beta=1.0), nt(130, 512, 40),
          nt(130, 130, 40, batch=8, lower_c=1), rb(129, 100, 37, 8, 0.0, 0, 1), sq(1024, 1024, -1, 0)]
_ENV_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd())
from gp_mpc_rocket_landing_amd import _lib as L
print(json.dumps([L.gemm_plan(*a) for a in json.loads(sys.argv[1])]))
"""


def _child(code, env, *argv):
    base = {k: v for k, v in os.environ.items() if not k.startswith("GPMPC_") or k in ("GPMPC_LIB", "GPMPC_HIP_RUNTIME")}
    r = subprocess.run([sys.executable, "-c", code, *argv], cwd=REPO, env=dict(base, **env), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (env, r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("field,value,want", [(None, None, {})] + [(k, str(v), {k: v}) for k, v in MOVED]
                         + [("splitk", "", {"splitk": 0}), ("xcd_batch", "x", {"xcd_batch": 0})])
def test_process_policy_reads_the_documented_switches(field, value, want):
    """policy = NULL follows the process's environment: each GPMPC_* name reaches its field,
    an empty or non-numeric value reads as 0."""
    from gp_mpc_rocket_landing_amd import _lib
    got = _child(_ENV_CHILD, {ENV_OF[field]: value} if field else {}, json.dumps(PROBES))
    exp = [_lib.gemm_plan(*a, **dict(DEFAULT, **want)) for a in PROBES]
    assert [(*g[:3], tuple(g[3]), *g[4:]) for g in got] == exp
    if field and field != "post_xcd":   # the probes do show the switch
        assert exp != [_lib.gemm_plan(*a, **DEFAULT) for a in PROBES]


def test_one_home_for_the_gemm_switches():
    """The plan header has no launch and no HIP type in it and includes standard headers and
    gpmpc.h only; the ten switch names appear in csrc nowhere else."""
    src = open(os.path.join(CSRC, "gemm_plan.h")).read()
    assert not re.search(r"hipLaunch|hipError_t|hipStream_t|<hip/|<<<", src)
    assert re.findall(r'#include ["<]([^">]+)[">]', src) == ["cstdint", "../../include/gpmpc.h"]
    names = re.compile(r"\b(" + "|".join(ENV_OF.values()) + r")\b")
    hits = [(name, m) for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))
            for m in names.findall(open(os.path.join(CSRC, name)).read())]
    assert {n for n, _ in hits} == {"gemm_plan.h"} and {m for _, m in hits} == set(ENV_OF.values())


def test_plan_arguments():
    from gp_mpc_rocket_landing_amd import _lib
    f = _lib._L.gpmpc_gemm_plan
    out = np.full(8, -5, np.int32)
    pol = np.array(list(_lib.GEMM_POLICY.values()), np.int32)
    assert f(0, 300, 300, 1100, 1, 1.0, 0, 0, 0, _lib._i(pol), _lib._i(out)) == 0
    assert out.tolist() == [2, 4, 0, 3, 3, 4, 128, 0]
    assert _lib.gemm_plan("nt", 300, 300, 1100, beta=1.0, **DEFAULT) == ("128_ksplit", 4, "2d", (3, 3, 4), 128, 0)
    assert _lib.gemm_plan("nt", 32, 33, 257, **DEFAULT) == ("splitk", 4, "2d", (1, 1, 4), 64, 80)
    assert _lib.gemm_plan("nt", 0, 33, 257, **DEFAULT) == ("none", 0, "2d", (0, 0, 0), 64, 0)
    assert _lib.gemm_plan("sumsq", 300, 0, 300, p0=1, **DEFAULT)[0] == "none"
    for op in (5, 6, 7, 8, 11, -1):   # the fixed-path launchers have no decision
        assert f(op, 64, 64, 64, 1, 0.0, 0, 1, 0, _lib._i(pol), _lib._i(out)) == -2
    for M, N, K, batch in ((-1, 64, 64, 1), (64, -1, 64, 1), (64, 64, -1, 1), (64, 64, 64, 0), (64, 64, 64, -3)):
        assert f(0, M, N, K, batch, 0.0, 0, 0, 0, _lib._i(pol), _lib._i(out)) == -2
    assert f(0, 64, 64, 64, 1, 0.0, 0, 0, 0, _lib._i(pol), None) == -2
    with pytest.raises(_lib.HIPError):
        _lib.gemm_plan("lat0", 16, 16, 16)
    with pytest.raises(TypeError):
        _lib.gemm_plan("nt", 300, 300, 300, gemm128=0)


# ---- 5. one tile-height rule for the SUMSQ partial buffer ------------------------------------------

_TILES_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd())
from gp_mpc_rocket_landing_amd import _lib as L
g = [255, 256, 257, 300, 511, 512, 513]
print(json.dumps([[M, N, K, *L.gemm_row_tiles(M, N, K)] for M in g for N in [20, 64] + g for K in g]))
"""


@pytest.mark.parametrize("env,kmin,big", [({}, 256, True), ({"GPMPC_GEMM128_KMIN": "512"}, 512, True),
                                          ({"GPMPC_GEMM128": "0"}, 256, False)])
def test_gemm_row_tiles_is_the_launchers_tile_height(env, kmin, big):
    """The partial buffer's rows as its consumers count them (gemm_row_tiles) against the
    kernel the launcher picks (gemm_sumsq_kind): 128-row tiles exactly when GPMPC_GEMM128 is on
    and M, N >= 256, K >= GPMPC_GEMM128_KMIN (launch_gemm_impl's rule), 64-row tiles otherwise --
    also under GPMPC_GEMM128_KMIN = 512 with 256 <= K < 512, where the two used to differ."""
    rows = _child(_TILES_CHILD, env)
    assert len(rows) == 7 * 9 * 7
    for M, N, K, tiles, kind in rows:
        want128 = big and M >= 256 and N >= 256 and K >= kmin
        assert (kind == 1) == want128, (M, N, K, kind)
        assert kind in (0, 1, 2) and (kind != 2 or (N <= 64 and K >= 256))
        assert tiles == ((M + 127) // 128 if kind == 1 else (M + 63) // 64), (M, N, K, tiles, kind)
