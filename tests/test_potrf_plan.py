"""The batched Cholesky's launch plan, read without a GPU through gpmpc_potrf_plan (the same
potrf_plan that launch_potrf_batched executes, csrc/potrf_plan.h): the regimes that
test_gpu_parity.test_potrf_batched_dev and test_potrf_switch_paths say they cover, pinned;
invariants of every plan over a sweep of shapes and switches; and the switch names.

A step is (kind, c, K0, a0, a1, a2, a3) -- include/gpmpc.h lists the operands per kind."""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gp_mpc_rocket_landing_amd", "csrc")
DB = 128
UPDATES = ("upd_syrk_diag", "upd_rowblock")
SOLVES = ("updsolve", "psolve_trsm", "psolve_lat", "psolve_rowblock")
TRAILS = ("trail_lat", "trail_syrk")
# the switch cases of test_potrf_switch_paths
SWITCH_CASES = [{}, {"la": 1}, {"syrk_diag": 0}, {"fuse": 0}, {"pk": 1}]


def plan(n, batch, **sw):
    """The plan under the default policy with the given switches (an explicit policy
    always: the process's own environment plays no part)."""
    from gp_mpc_rocket_landing_amd import _lib
    return _lib.potrf_plan(n, batch, **dict({"p128": 1}, **sw))


def steps128(n, batch, **sw):
    form, steps = plan(n, batch, **sw)
    assert form == "128"
    return steps


def kinds(steps):
    return [s[0] for s in steps]


def K_of(s):
    """K of an update, fused step or trailing update."""
    return s[5] if s[0] == "upd_rowblock" else s[4]


def ks_of(s):
    return s[6] if s[0] == "upd_rowblock" else s[5]


# ---- 1. the shapes of test_potrf_batched_dev -------------------------------------------------

def gpu_test_shapes():
    import test_gpu_parity
    mark = [m for m in test_gpu_parity.test_potrf_batched_dev.pytestmark if m.name == "parametrize"][0]
    return [tuple(p) for p in mark.args[1]]


def regime(batch):
    """The batch regimes of test_potrf_batched_dev's docstring."""
    if batch >= 256 or (batch >= 128 and batch % 8 == 0):
        return "left"
    return "lat" if batch <= 16 else "trsm" if batch <= 64 else "inverse"


@pytest.mark.parametrize("n,batch", gpu_test_shapes())
def test_gpu_test_shapes_take_the_regime_their_test_claims(n, batch):
    steps = steps128(n, batch)
    ks, reg = kinds(steps), regime(batch)
    diags = [s for s in steps if s[0] == "diag"]
    nblk = (n + DB - 1) // DB
    assert len(diags) == nblk
    # the column-sweep diagonal kernel everywhere; its 32 x 32 inverted blocks feed the TRSM-form solve
    assert {s[5] for s in diags} == {3 if reg in ("lat", "trsm") else 1}
    # the packed lower LDS layout exactly where there are more matrices than CUs
    assert {s[4] for s in diags} == {int(batch > 256)}
    solves = [k for k in ks if k in SOLVES]
    assert len(solves) == nblk - 1
    if reg == "left":
        # left-looking block columns in ONE outer panel: no trailing SYRK
        assert not set(ks) & set(TRAILS) and {s[2] for s in steps} == {0}
        # each block column but the first takes one update by all earlier columns (K = c)
        assert [(s[1], K_of(s)) for s in steps if s[0] in UPDATES] == [(c, c) for c in range(DB, n, DB)]
        assert set(solves) <= {"updsolve", "psolve_rowblock"}
        if batch % 8:
            assert "updsolve" not in ks
    else:
        # right-looking: no update launches, one trailing SYRK per block column but the last
        assert not set(ks) & set(UPDATES) and "updsolve" not in ks
        trail = {"lat": "trail_lat", "trsm": "trail_syrk", "inverse": "trail_syrk"}[reg]
        assert [k for k in ks if k in TRAILS] == [trail] * (nblk - 1)
        assert set(solves) <= {"psolve_rowblock" if reg == "inverse" else "psolve_trsm"}
        assert all(s[4] == DB for s in steps if s[0] in TRAILS)   # K = 128 SYRKs


def test_pinned_plans_300():
    """Derived from the parent's driver (its launches, in order) before the plan existed."""
    right = [("diag", 0, 0, 128, 0, 3, 1), ("psolve_trsm", 0, 0, 172, 0, 0, 0), ("trail", 128, 0, 172, 128, 0, 0),
             ("diag", 128, 128, 128, 0, 3, 1), ("psolve_trsm", 128, 128, 44, 0, 0, 0),
             ("trail", 256, 128, 44, 128, 0, 0), ("diag", 256, 256, 44, 0, 3, 0)]

    def with_trail(kind):
        return [(kind,) + s[1:] if s[0] == "trail" else s for s in right]
    assert steps128(300, 16) == with_trail("trail_lat")
    assert steps128(300, 64) == with_trail("trail_syrk")
    assert steps128(300, 256) == [
        ("diag", 0, 0, 128, 0, 1, 1), ("updsolve", 0, 0, 172, 0, 0, 0),
        ("upd_rowblock", 128, 0, 172, 128, 128, 1), ("diag", 128, 0, 128, 0, 1, 1),
        ("psolve_rowblock", 128, 0, 44, 0, 0, 0),
        ("upd_syrk_diag", 256, 0, 44, 256, 2, 0), ("diag", 256, 0, 44, 0, 1, 0)]


def test_520_256_has_every_left_looking_step():
    """The comment on (520, 256): the solve-only first column, K > 0 update + solve, balanced
    diagonal SYRK with K split, an unfused column, a ragged 8-wide last block."""
    steps = steps128(520, 256)
    assert steps[:2] == [("diag", 0, 0, 128, 0, 1, 1), ("updsolve", 0, 0, 392, 0, 0, 0)]
    assert any(s[0] == "updsolve" and s[4] > 0 for s in steps)
    assert any(s[0] == "upd_syrk_diag" and s[5] > 1 for s in steps)
    fused = {s[1] for s in steps if s[0] == "updsolve"}
    unfused = {s[1] for s in steps if s[0] == "psolve_rowblock"}
    assert fused == {0, 128, 256} and unfused == {384}
    assert ("upd_rowblock", 384, 0, 136, 128, 384, 1) in steps
    assert steps[-2:] == [("upd_syrk_diag", 512, 0, 8, 512, 2, 0), ("diag", 512, 0, 8, 0, 1, 0)]


def test_other_commented_shapes():
    ks = kinds(steps128(300, 136))    # left-looking from batch 128, too few workgroups to fuse
    assert "updsolve" not in ks and not set(ks) & set(TRAILS) and "upd_rowblock" in ks
    assert all(s[4] == 1 for s in steps128(300, 520) if s[0] == "diag")   # packed diagonal kernel
    assert [s for s in steps128(257, 64) if s[0] == "diag"][-1][3] == 1   # a 1-wide last block
    assert [s for s in steps128(257, 260) if s[0] == "diag"][-1][3:5] == (1, 1)


# ---- 2. the switch cases of test_potrf_switch_paths at (520, 256) ------------------------------

def test_switch_look_ahead():
    steps = steps128(520, 256, la=1)
    ahead = [i for i, s in enumerate(steps) if s[0] == "updsolve" and s[5] > 0]
    assert [steps[i][1] for i in ahead] == [0, 128] and all(steps[i][5] == DB for i in ahead)
    for i in ahead:   # the next block's diagonal update came with this step: its factor follows at once
        assert steps[i + 1][:2] == ("diag", steps[i][1] + DB)
    assert [s[1] for s in steps if s[0] in UPDATES] == [384, 512]
    assert len(steps) == len(steps128(520, 256)) - len(ahead)


def test_switch_syrk_diag_off():
    steps, base = steps128(520, 256, syrk_diag=0), steps128(520, 256)
    assert "upd_syrk_diag" not in kinds(steps)
    # the same updates by the 128-tile kernel: rows = w for a fused column's diagonal block
    assert [s for s in steps if s[0] == "upd_rowblock"] == [
        ("upd_rowblock", s[1], s[2], s[3], s[3], s[4], s[5]) if s[0] == "upd_syrk_diag" else s
        for s in base if s[0] in UPDATES]


def test_switch_fuse_off():
    steps = steps128(520, 256, fuse=0)
    assert "updsolve" not in kinds(steps)
    assert [s[1] for s in steps if s[0] == "psolve_rowblock"] == [0, 128, 256, 384]
    assert [s[3] for s in steps if s[0] == "upd_rowblock"] == [392, 264, 136]   # whole block columns


def test_switch_packed_diag():
    for sw in ({"pk": 1}, {"pk": 1, "fuse": 0}):
        assert all(s[4] == 1 for s in steps128(520, 256, **sw) if s[0] == "diag")
    assert all(s[4] == 0 for s in steps128(520, 256, pk=1, sweep=0) if s[0] == "diag")   # only with the sweep
    assert all(s[4] == 0 for s in steps128(300, 520, pk=0) if s[0] == "diag")


# ---- 3. invariants over a sweep --------------------------------------------------------------

SWEEP_N = [1, 100, 128, 129, 256, 300, 520, 1000, 1025]
SWEEP_B = [1, 16, 17, 64, 65, 128, 136, 255, 256, 257, 520, 1024]


def check_plan(n, batch, steps):
    cols = list(range(0, n, DB))
    at = {}
    for i, s in enumerate(steps):
        at.setdefault((s[0] if s[0] == "diag" else "solve" if s[0] in SOLVES else "other", s[1]), []).append(i)
    assert [s[1] for s in steps if s[0] == "diag"] == cols   # every block once, in order
    for c in cols:
        d = steps[at[("diag", c)][0]]
        assert d[3] == min(DB, n - c) and d[6] == int(c + DB < n)   # Linv written iff rows follow
        solves = at.get(("solve", c), [])
        assert len(solves) == int(c + DB < n)
        if solves:
            assert solves[0] > at[("diag", c)][0] and steps[solves[0]][3] == n - c - DB
    for s in steps:
        if s[0] in UPDATES + TRAILS + ("updsolve",):
            assert K_of(s) == s[1] - s[2] and 0 <= s[2] <= s[1]
        if s[0] in UPDATES:
            assert K_of(s) > 0 and 1 <= ks_of(s) <= max(1, K_of(s) // DB)
            assert s[3] in (min(DB, n - s[1]), n - s[1]) and 0 < min(DB, n - s[1]) == (s[3] if s[0] == "upd_syrk_diag" else s[4])
        if s[0] == "updsolve":
            assert batch % 8 == 0 and 0 <= s[5] <= min(DB, s[3])
        if s[0] in TRAILS:   # only where the outer panel ends before n
            assert s[2] < s[1] < n and s[1] % DB == 0 and s[3] == n - s[1]
        assert s[1] < n and s[1] % DB == 0 and s[2] % DB == 0 and s[2] <= s[1]


@pytest.mark.parametrize("sw", SWITCH_CASES, ids=lambda sw: "-".join(f"{k}{v}" for k, v in sw.items()) or "default")
def test_plan_invariants_over_the_sweep(sw):
    for n in SWEEP_N:
        for batch in SWEEP_B:
            form, steps = plan(n, batch, **sw)
            assert form == "128", (n, batch)
            try:
                check_plan(n, batch, steps)
            except AssertionError as e:
                raise AssertionError(f"n = {n}, batch = {batch}, {sw}: {steps}") from e


def test_form_follows_p128_and_persist():
    for n, batch in [(1, 1), (300, 16), (520, 256), (1025, 1024)]:
        for sw in SWITCH_CASES:
            assert plan(n, batch, **sw)[0] == "128"
            assert plan(n, batch, **dict(sw, p128=0)) == ("32", [])
            assert plan(n, batch, **dict(sw, p128=0, persist=1)) == ("32", [])
            assert plan(n, batch, **dict(sw, persist=1)) == ("persist", [])
            assert plan(n, batch, **dict(sw, persist=-1))[0] == "128"


def test_plan_arguments():
    from gp_mpc_rocket_landing_amd import _lib
    import ctypes
    import numpy as np
    form = ctypes.c_int(-9)
    buf = np.full((3, 7), -5, np.int32)
    f = _lib._L.gpmpc_potrf_plan
    pol = np.array(list(_lib.POTRF_POLICY.values()), np.int32)
    assert f(300, 16, _lib._i(pol), ctypes.byref(form), _lib._i(buf), 3) == 7   # the count, past cap
    assert form.value == 2 and buf[2].tolist() == [7, 128, 0, 172, 128, 0, 0]
    assert f(300, 16, _lib._i(pol), ctypes.byref(form), None, 0) == 7
    assert f(0, 16, _lib._i(pol), ctypes.byref(form), None, 0) == 0
    assert f(300, 16, _lib._i(pol), None, _lib._i(buf), 3) == -2
    assert f(-1, 16, _lib._i(pol), ctypes.byref(form), _lib._i(buf), 3) == -2
    pol[list(_lib.POTRF_POLICY).index("ob")] = 100   # not a multiple of 128
    assert f(300, 16, _lib._i(pol), ctypes.byref(form), _lib._i(buf), 3) == -2
    with pytest.raises(TypeError):
        _lib.potrf_plan(300, 16, fused=0)
    assert _lib.potrf_plan(300, 300, ob=256)[1][-1][:3] == ("diag", 256, 256)


# ---- the switches: names, order, one reader ---------------------------------------------------

def test_binding_matches_the_headers():
    from gp_mpc_rocket_landing_amd import _lib
    src = open(os.path.join(CSRC, "potrf_plan.h")).read()
    body = re.search(r"struct PotrfPolicy \{(.*?)\n\};", src, re.S).group(1)
    fields = [(k, int(v)) for k, v in re.findall(r"^\s*int (\w+) = (-?\d+);", body, re.M)]
    assert fields == list(_lib.POTRF_POLICY.items())
    hdr = open(os.path.join(REPO, "include", "gpmpc.h")).read()
    assert int(re.search(r"#define GPMPC_POTRF_POLICY_N (\d+)", hdr).group(1)) == len(fields)
    assert int(re.search(r"#define GPMPC_POTRF_STEP_INTS (\d+)", hdr).group(1)) == 7
    codes = {k.lower(): int(v) for k, v in re.findall(r"GPMPC_POTRF_([A-Z_]+[A-Z]) = (\d+)", hdr)}
    assert codes == {k: i for i, k in enumerate(_lib.POTRF_STEP)}


ENV_OF = {"p128": "GPMPC_POTRF128", "persist": "GPMPC_POTRF_PERSIST", "lat": "GPMPC_POTRF_LAT",
          "sweep": "GPMPC_DIAG_SWEEP", "trsm": "GPMPC_POTRF_TRSM", "pk": "GPMPC_DIAG_PK", "ob": "GPMPC_POTRF_OB",
          "ksplit": "GPMPC_POTRF_KSPLIT", "fuse": "GPMPC_POTRF_FUSE", "la": "GPMPC_POTRF_LA",
          "syrk_diag": "GPMPC_SYRK_DIAG", "fuse_min": "GPMPC_POTRF_FUSE_MIN"}
_ENV_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd())
from gp_mpc_rocket_landing_amd import _lib as L
print(json.dumps([L.potrf_plan(n, b) for n, b in [(520, 256), (300, 16), (1000, 64)]]))
"""


def _child(code, env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("GPMPC_") or k in ("GPMPC_LIB", "GPMPC_HIP_RUNTIME")}
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=dict(base, **env), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (env, r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("field,value,want", [
    (None, None, {}), ("p128", "0", {"p128": 0}), ("persist", "1", {"persist": 1}), ("lat", "1", {"lat": 1}),
    ("sweep", "0", {"sweep": 0}), ("trsm", "0", {"trsm": 0}), ("pk", "1", {"pk": 1}), ("ob", "300", {"ob": 256}),
    ("ob", "0", {"ob": 128}), ("ob", "9999", {"ob": 1024}), ("ksplit", "1", {"ksplit": 1}), ("fuse", "0", {"fuse": 0}),
    ("fuse", "", {"fuse": 0}), ("la", "1", {"la": 1}), ("syrk_diag", "0", {"syrk_diag": 0}),
    ("fuse_min", "1", {"fuse_min": 1}), ("lat", "x", {"lat": 0})])
def test_process_policy_reads_the_documented_switches(field, value, want):
    """policy = NULL follows the process's environment: each GPMPC_* name reaches its field,
    an empty or non-numeric value reads as 0, GPMPC_POTRF_OB is cut to 128..1024 in 128s."""
    got = _child(_ENV_CHILD, {ENV_OF[field]: value} if field else {})
    exp = [plan(n, b, **want) for n, b in [(520, 256), (300, 16), (1000, 64)]]
    assert [(f, [tuple(s) for s in st]) for f, st in got] == exp


def test_one_switch_reader():
    """getenv appears in csrc only in gpmpc_env_int and for GPMPC_POOL_CAP_MB (a byte count
    read with strtoull); the plan header has no launch and no HIP type in it."""
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            for i, line in enumerate(open(os.path.join(CSRC, name)), 1):
                if "getenv(" in line:
                    hits.append((name, line.strip()))
    assert hits == [("ctx.hip", "const char *e = getenv(name);"),
                    ("ctx.hip", 'const char *e = getenv("GPMPC_POOL_CAP_MB");')]
    src = open(os.path.join(CSRC, "potrf_plan.h")).read()
    assert not re.search(r"hipLaunch|hipError_t|hipStream_t|<hip/|<<<", src)
    assert re.findall(r'#include ["<]([^">]+)[">]', src) == ["climits", "../../include/gpmpc.h"]
