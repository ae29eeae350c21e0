"""The fleet step's front end folded into fewer launches leaves every bit alone.

GPMPC_GRAM_FEAT (the row-tiled Gram kernel forms the query rows itself, no k_fleet_queries
launch) is read once per process, so every configuration flies in a child process of its
own and the parent compares what they saved.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import close

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("GPMPC_GRAM_FEAT",)

# The smallest fleet on the flagship's kernels: 32 landings x N = 20 = 640 query rows (the
# row-tiled Gram starts at 512, launch_gram) against a GP of 300 rows (the 128-tile posterior
# needs M, P, K >= 256, gemm_sumsq_kind): three row tiles of [W; alpha^T], the last partial
# and holding the alpha rows, K = 300 no multiple of 16.  Six steps; landings 5 and 17 start
# below the touchdown altitude and terminate at step 1; landings 3..9 are reset after step 2.
_FLEET_CHILD = r"""
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from gp_mpc_rocket_landing_amd import _lib
from gp_mpc_rocket_landing_amd.fleet import Fleet, fit_gp, initial_conditions
out, mc = sys.argv[1], sys.argv[2] == "mc"
ctx = _lib.Context(0)
gp = fit_gp(ctx, n_train=300)
B = 32
x0 = initial_conditions(B, seed0=42)
for b in (5, 17):
    x0[b, 1] = 0.4
    x0[b, 4:7] = 0.0
f = Fleet(ctx, gp, B, horizon=20)
f.reset(x0)
if mc:
    f.attach_mc(log=True)
keep = {}
for k in range(6):
    f.step(1)
    st = f.state()
    for name, v in st.items():
        keep["%s_%d" % (name, k)] = v
    keep["mean_%d" % k], keep["var_%d" % k] = f.posterior()
    if k == 1:
        f.reset(initial_conditions(7, seed0=4242), first=3)
if mc:
    keep["log_states"], keep["log_controls"], keep["log_nsteps"] = f.read_log()
keep["query_launches"] = np.array(_lib._L.gpmpc_fleet_query_launches(f.h))
f.close()
np.savez(out, **keep)
print("frontend child ok")
"""

def _child(script, out, env, *args):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", script, str(out), *args], cwd=REPO, env=e, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "frontend child ok" in r.stdout, (env, r.stdout[-1000:], r.stderr[-3000:])
    return dict(np.load(str(out)))


OFF = {k: "0" for k in SWITCHES}


def _same_flight(on, off):
    """The two children took the two paths at every one of the six steps (the running
    count never fell below the row-tiled Gram's 512 rows): no k_fleet_queries launch
    with the switch on, one a step with it off; everything they saved is equal."""
    assert sorted(on) == sorted(off)
    assert int(on["query_launches"]) == 0 and int(off["query_launches"]) == 6
    for name in sorted(on):
        if name != "query_launches":
            np.testing.assert_array_equal(on[name], off[name], err_msg=name)


@pytest.mark.parametrize("build", [{}, {"GPMPC_FLEET_WIDE": "0"}], ids=["wide", "narrow"])
def test_fleet_frontend_switches_keep_every_bit(tmp_path, build):
    """Records, x, state() (Xw, Uw, y, rho) and posterior() mean and variance after each of
    six steps, every new switch on against all off: array_equal.  On the control build 32
    landings take by default (wide) and on the flagship's (narrow, forced in both runs: the
    two builds' bits differ, which is why a fleet keeps one for life)."""
    off = _child(_FLEET_CHILD, tmp_path / "off.npz", dict(OFF, **build), "plain")
    on = _child(_FLEET_CHILD, tmp_path / "on.npz", build, "plain")
    # the scenario is the one described: two landings gone at step 1, seven flying again after the reset
    assert np.all(off["rec_0"][[5, 17], 0] != 0) and np.sum(off["rec_0"][:, 0] != 0) == 2
    assert np.all(off["rec_2"][3:10, 0] == 0) and np.all(off["rec_2"][3:10, 1] == 1)
    assert np.all(np.isfinite(off["mean_5"][off["rec_4"][:, 0] == 0]))
    _same_flight(on, off)


def test_fleet_frontend_with_the_protocol_attached(tmp_path):
    """The same flight with the Monte-Carlo attachment (k_fleet_mc after the control kernel):
    switches on against off, the log and everything else equal."""
    off = _child(_FLEET_CHILD, tmp_path / "off.npz", OFF, "mc")
    on = _child(_FLEET_CHILD, tmp_path / "on.npz", {}, "mc")
    assert "log_states" in on and int(on["log_nsteps"].max()) >= 4
    _same_flight(on, off)


def test_predict_edge_rows_match_the_oracle(gpu_ctx):
    """Exact-GP posteriors at n in {253, 254, 300} ([W; alpha^T] of 256, 257 and 303 rows:
    full tiles, the alpha rows across a tile boundary, a partial last tile) and P in
    {256, 640}, within test_gpu_parity.py's tolerance (|a - b| <= 1e-6 max(|b|, y_std),
    y_std^2 for the variance) of gp_oracle.exact_predict.  A predict passes no plans, so this
    guards k_gram_rows' staging from a / na (P = 640) beside the path the fleet now takes;
    no switch of this file changes it."""
    from gp_mpc_rocket_landing_amd import _lib
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from oracle import gp_oracle
    for n in (253, 254, 300):
        X, U, D = synthetic_training_data(n, seed=n)
        Z = gp_oracle.features_3dof(X, U)
        gp = _lib.ExactGPHandle(gpu_ctx, _lib.SE_ARD, Z, D, np.ones(11), 1.0, 1e-4)
        st = gp_oracle.exact_fit(Z, D)
        for P in (256, 640):
            Xq, Uq, _ = synthetic_training_data(P, seed=1000 + n + P)
            Zq = gp_oracle.features_3dof(Xq, Uq)
            m, v = gp.predict(Zq)
            mo, vo = gp_oracle.exact_predict(st, Zq)
            ok, e = close(m, mo, st["y_std"]); assert ok, (n, P, e)
            ok, e = close(v, vo, st["y_std"] ** 2); assert ok, (n, P, e)
