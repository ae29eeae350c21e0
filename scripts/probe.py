"""Measurement probes for the GPU box, one subcommand each (run from the repo root,
through gpurun, alone or under scripts/profile.sh for a kernel trace / PMC pass):

  single                    the single-landing step (configs[2]: the fleet at B = 1), 100 steps x 3
  step [B] [steps]          the bench's control step alone (B landings, N = 20, GP n = 1000)
  stamps [B] [steps]        landing 0's control-kernel phase cycles (gpmpc_fleet_set_stamps)
  placement [B]             where the control kernel's waves land (HW_ID) and per-landing spans
  streams                   the fleet as 1 / 2 / 4 shards on as many streams: free-running, and
                            pipelined (shard posteriors serialised, controls beside them)
  fit                       Simple3DoFGP.fit through the surface and the bare C-ABI fit, x 8
  append [k]                gpmpc_gp_append of k rows into the n = 1000 GP against a refit
  chol                      bench.py's Cholesky leg (JSON)
  potrf [NxB,...]           batched potrf ms / TFLOP/s / error per shape
  potrf_streams             batched potrf split over 1 / 2 / 4 streams
  syrk_fitc                 the config-5 FITC SYRK (2000 x 4000), 30 launches (JSON)
  gemm_loop [n]             the 128-tile MFMA loop's steady state: lower SYRK n = k (JSON)
  trsm                      trsm_lower / potrs at n = 128 and 1000, for a kernel trace
  rollouts6 [64,512]        bench.py's configs[4] rollouts leg (JSON)
  qp_sweep [B] [mi:eps,..]  configs[4] ADMM settings: status histogram and timing per setting
  surface [reps] [prof]     bench.py's 3-DoF drop-in surface leg (JSON); prof: under cProfile
  surface6 [reps] [prof]    bench.py's 14-state drop-in surface leg (JSON); prof: under cProfile
                            (GPMPC_QP_STAMPS=1 beside either: k_qp_batched phase cycles on stderr,
                            summarised by scripts/pmc.py qpstamps)
  novelty [reps]            gpmpc_select_diverse, both paths, over n at d = 5, n_select = 100 (the
                            crossover of the automatic path); NoveltySelector.select_diverse at
                            n = 2000 / 6000 / 300000 against the numpy restatement of the reference's
                            loop; gpmpc_nn_dist at n = 300000, r = 1000 (JSON lines)
  unscented [reps]          UncertaintyPropagator.propagate_unscented_batch, the one device call
                            against the per-step host loop (use_device = False), back to back, at
                            B = 1 / 64, N = 20: the 3-DoF model (exact n = 1000, default FITC) and the
                            14-state model (exact n = 1000, FITC M = 50 and M = 2000) (JSON lines)
  mc [reps]                 UncertaintyPropagator.propagate_monte_carlo_batch, the whole call (host draws
                            and the one device call) against the per-step host loop (use_device = False)
                            in the same process, at B = 1 / 64, N = 20, S = 100 / 4096 particles (host
                            loop at S = 100 only): the 3-DoF model (exact n = 1000, default FITC) and the
                            14-state model (FITC M = 50, exact n = 1000) (JSON lines)
  knn [reps]                gpmpc_knn_query (k = 64) and gpmpc_knn_interp (K_max = 50) over a resident
                            set of n = 131072, d = 7 and n = 65536, d = 14 at B = 1 / 64 / 1024, whole
                            calls, against the scipy loop the reference runs on the same box (one
                            KDTree.query and one query_ball_point per state; the tree build apart); the
                            plan of every shape and the whole-call fp64 rate; before them the query
                            alone over small sets (n = 512 / 4096 / 16384, B = 1 ... 64) for the
                            crossover between the two (JSON lines)
  hull [reps] [device_only] TerminalSetManager.project_batch (gpmpc_knn_hull, one device call) for 1024
                            states over safe sets of 4096 rows, 7 and 14 states, K = 10 and K = 50,
                            against the numpy restatement of the contract (tests/hull_check.py) looped
                            over the same vertex sets; with a second argument the device calls alone,
                            for a kernel trace (JSON lines)
"""
import json
import os
import sys
import time
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from gp_mpc_rocket_landing_amd import _lib  # noqa: E402

FP64_PEAK = 78.6e12


def _torch():
    import torch
    return torch


def _fleet():
    from gp_mpc_rocket_landing_amd import fleet
    return fleet


def _events(torch, stream, fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    return e0, e1


# ---- the 3-DoF fleet -------------------------------------------------------------------
def single():
    F = _fleet()
    ctx = _lib.Context(0)
    f = F.Fleet(ctx, F.fit_gp(ctx, n_train=1000), 1)
    for _ in range(3):
        f.reset(F.initial_conditions(1))
        ctx.sync()
        t0 = time.perf_counter()
        f.step(100)
        ctx.sync()
        print(f"{(time.perf_counter() - t0) / 100 * 1e6:.1f} us per step", flush=True)
    f.close()


def step(B="1024", steps="10"):
    F = _fleet()
    B, steps = int(B), int(steps)
    ctx = _lib.Context(0)
    fl = F.Fleet(ctx, F.fit_gp(ctx, n_train=1000), B)
    fl.reset(F.initial_conditions(B))
    fl.step(3)
    ctx.sync()
    t0 = time.perf_counter()
    fl.step(steps)
    ctx.sync()
    dt = (time.perf_counter() - t0) / steps
    print(f"{B} landings: {dt * 1e3:.3f} ms per step, {B / dt / 1e6:.3f} M steps/s", flush=True)
    fl.close()


def stamps(B="1024", steps="4"):
    """Slots: 0 assembly, 1 scaling, 2 factor, 3 rhs, 4 KKT block solve (rest), 5 x/z/y
    update, 6 checks + adaptive rho, 7 plant + tail, 8-10 the KKT solve's forward chain /
    diagonal blocks / backward chain, 11/12 the rhs and update compute before their
    barriers, 14 realtime (100 MHz), 15 total shader cycles."""
    torch, F = _torch(), _fleet()
    B, steps = int(B), int(steps)
    ctx = _lib.Context(0)
    fl = F.Fleet(ctx, F.fit_gp(ctx, n_train=1000), B, horizon=20)
    fl.reset(F.initial_conditions(B))
    fl.step(3)
    st = torch.zeros(16, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _lib._chk(_lib._L.gpmpc_fleet_set_stamps(fl.h, st.data_ptr()), "stamps")
    rec0, _ = fl.read()
    fl.step(steps)
    ctx.sync()
    rec1, _ = fl.read()
    s = st.cpu().numpy().astype(np.float64)
    it = rec1[0, 11] - rec0[0, 11]
    names = ["assembly", "scaling", "factor", "rhs", "kkt_solve(rest)", "update", "checks", "tail",
             "kkt_forward", "kkt_diagonal", "kkt_backward", "rhs_compute", "update_compute", "unused"]
    tot = s[15]
    print(f"B={B} landing 0: {steps} steps, {it:.0f} ADMM iterations, {tot:.0f} shader cycles "
          f"({s[14] / 100e6 * 1e6:.1f} us realtime)")
    for i, nm in enumerate(names):
        print(f"  {nm:10s} {s[i]:10.0f} cycles  {s[i] / tot * 100:5.1f}%  {s[i] / max(it, 1):8.0f} per iteration")
    fl.close()


def placement(B="1024"):
    """HW_ID (SIMD, CU, SE, XCC) of each landing's two waves and its start / end realtime
    over one control step; chain-wave sharing per SIMD and span by ADMM iterations.
    (GPMPC_FLEET_SIMD=0 for the chain-sharing lines: by default each workgroup claims
    its chain SIMD at run time.)"""
    torch, F = _torch(), _fleet()
    B = int(B)
    ctx = _lib.Context(0)
    fl = F.Fleet(ctx, F.fit_gp(ctx, n_train=1000), B, horizon=20)
    fl.reset(F.initial_conditions(B))
    fl.step(3)
    tr = torch.zeros(B * 4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _lib._chk(_lib._L.gpmpc_fleet_set_trace(fl.h, tr.data_ptr()), "trace")
    rec0, _ = fl.read()
    fl.step(1)
    ctx.sync()
    rec1, _ = fl.read()
    t = tr.cpu().numpy().reshape(B, 4).view(np.uint64)
    its = rec1[:, 11] - rec0[:, 11]
    span = (t[:, 1].astype(np.float64) - t[:, 0].astype(np.float64)) / 100.0

    def decode(v):
        v = int(v)
        hw = v & 0xFFFFFFFF
        return (((v >> 32) & 15), (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15), (hw >> 4) & 3

    w = [decode(v) for v in t[:, 2]]
    w1 = [decode(v) for v in t[:, 3]]
    per_cu = Counter(c for c, _ in w)
    print(f"{len(per_cu)} CUs used, landings per CU {Counter(per_cu.values())}")
    print(f"both waves on one CU: {sum(a[0] == b[0] for a, b in zip(w, w1))}/{B}")
    print(f"chain waves per SIMD: {Counter(Counter(w).values())}; all waves per SIMD: "
          f"{Counter(Counter(w + w1).values())}")
    for k in sorted(set(its.astype(int))):
        m = its == k
        print(f"  it={k:3d}: {m.sum():4d} landings, span {span[m].mean():7.1f} us "
              f"(min {span[m].min():.1f}, max {span[m].max():.1f})")
    fl.close()


def streams(steps="20", warm="3"):
    """The 1024-landing fleet as S shards (fleet_batch 1024: every landing's bits are the
    whole fleet's) on S streams.  Free-running: each shard steps on its own stream.
    Pipelined: the shards' posterior phases (mask 13) serialised in shard order through
    events, each shard's control kernel (mask 2) beside the next shard's posterior.
    Checks the pipelined records against the whole fleet's."""
    torch, F = _torch(), _fleet()
    steps, warm, B = int(steps), int(warm), 1024
    ctx0 = _lib.Context(0)
    gp = F.fit_gp(ctx0, n_train=1000)
    x0 = F.initial_conditions(B)

    def timed(ctxs, fn):
        for c in ctxs:
            c.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        for c in ctxs:
            c.sync()
        return round((time.perf_counter() - t0) / steps * 1e3, 4)

    out = {}
    whole = F.Fleet(ctx0, gp, B, horizon=20)
    whole.reset(x0)
    whole.step(warm)
    out["whole_step_ms"] = timed([ctx0], lambda: whole.step(1))
    out["whole_post_ms"] = timed([ctx0], lambda: whole.phases(13))
    out["whole_ctl_ms"] = timed([ctx0], lambda: whole.phases(2))
    whole.close()
    for S in (2, 4):
        n = B // S
        ctxs = [ctx0] + [_lib.Context(0) for _ in range(S - 1)]
        strm = [torch.cuda.ExternalStream(c.stream) for c in ctxs]

        def shards():
            sh = []
            for s in range(S):
                f = F.Fleet(ctxs[s], gp, n, fleet_batch=B, horizon=20)
                f.reset(x0[s * n:(s + 1) * n])
                sh.append(f)
            for c in ctxs:
                c.sync()
            return sh

        sh = shards()
        for f in sh:
            f.step(warm)
        out[f"S{S}_free_step_ms"] = timed(ctxs, lambda: [f.step(1) for f in sh])
        out[f"S{S}_post_one_shard_ms"] = timed(ctxs, lambda: sh[0].phases(13))
        out[f"S{S}_ctl_one_shard_ms"] = timed(ctxs, lambda: sh[0].phases(2))
        for f in sh:
            f.close()
        sh = shards()
        evs = [torch.cuda.Event() for _ in range(S)]
        prev = [None]

        def pipelined():
            for s in range(S):
                if prev[0] is not None:
                    strm[s].wait_event(prev[0])
                sh[s].phases(13)
                evs[s].record(strm[s])
                prev[0] = evs[s]
                sh[s].phases(2)

        for _ in range(warm):
            pipelined()
        out[f"S{S}_pipelined_step_ms"] = timed(ctxs, pipelined)
        rec_p = np.concatenate([f.read()[0] for f in sh])
        w = F.Fleet(ctx0, gp, B, horizon=20)
        w.reset(x0)
        w.step(warm + steps)
        out[f"S{S}_pipelined_bits_equal"] = bool(np.array_equal(rec_p, w.read()[0], equal_nan=True))
        w.close()
        for f in sh:
            f.close()
    print(json.dumps(out), flush=True)


# ---- GP fit / append ---------------------------------------------------------------------
def fit():
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.gp.features import Simple3DoFFeatureExtractor
    X, U, D = synthetic_training_data(1000, seed=0)
    Z = Simple3DoFFeatureExtractor().extract_batch(X, U)
    ctx = _lib.default_context()
    for rep in range(8):
        gp = Simple3DoFGP(use_sparse=False)
        gp.add_data(X, U, D)
        t0 = time.perf_counter(); gp.fit(); t1 = time.perf_counter()
        h = _lib.ExactGPHandle(ctx, _lib.SE_ARD, Z, D, np.ones(Z.shape[1]), 1.0, 1e-4)
        t2 = time.perf_counter()
        del h
        print(f"rep {rep}: surface fit {1e3 * (t1 - t0):.3f} ms, C-ABI fit {1e3 * (t2 - t1):.3f} ms", flush=True)


def append(k="10"):
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from gp_mpc_rocket_landing_amd.gp.features import Simple3DoFFeatureExtractor
    n, k = 1000, int(k)
    ctx = _lib.Context(0)
    X, U, D = synthetic_training_data(n + k, seed=0)
    Z = Simple3DoFFeatureExtractor().extract_batch(X, U)
    ta, tf = [], []
    for _ in range(6):
        h = _lib.ExactGPHandle(ctx, _lib.SE_ARD, Z[:n], D[:n], np.ones(11), 1.0, 1e-4)
        t0 = time.perf_counter()
        assert h.append(Z[n:], D)
        ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h2 = _lib.ExactGPHandle(ctx, _lib.SE_ARD, Z, D, np.ones(11), 1.0, 1e-4)
        tf.append(time.perf_counter() - t0)
        del h, h2
    print(json.dumps({"append_ms": [round(t * 1e3, 3) for t in ta], "refit_ms": [round(t * 1e3, 3) for t in tf]}))


# ---- Cholesky / SYRK / GEMM / TRSM -------------------------------------------------------
def chol():
    import bench
    print(json.dumps(bench.cholesky_bench(_lib.Context(0), _torch())), flush=True)


def potrf(shapes="1000x1,1000x14,1000x64,1000x256,2000x1,2000x8"):
    torch = _torch()
    ctx = _lib.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    for n, batch in (tuple(int(v) for v in t.split("x")) for t in shapes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(0)
        G = torch.randn(batch, n, n, dtype=torch.float64, device="cuda", generator=g) / n ** 0.5
        base = torch.baddbmm(torch.eye(n, dtype=torch.float64, device="cuda").expand(batch, n, n), G,
                             G.transpose(1, 2))
        del G
        A = base.clone()
        info = torch.zeros(batch, dtype=torch.int32, device="cuda")
        ts = []
        for _ in range(4):
            A.copy_(base)
            torch.cuda.synchronize()
            e0, e1 = _events(torch, stream, lambda: _lib._chk(_lib._L.gpmpc_potrf_batched_dev(
                ctx.h, n, batch, A.data_ptr(), n, n * n, info.data_ptr()), "potrf"))
            ctx.sync()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        assert int(info.abs().sum()) == 0
        pick = [0, batch - 1]
        err = float((torch.tril(A[pick]) - torch.linalg.cholesky(base[pick])).abs().max())
        t = min(ts[1:])
        fl = batch * (n ** 3 / 3 + n ** 2 / 2 + n / 6)
        print(f"n={n} batch={batch}: {t * 1e3:.3f} ms  {fl / t / 1e12:.2f} TFLOP/s  "
              f"{fl / t / FP64_PEAK * 100:.1f}% fp64 peak  maxerr {err:.2e}", flush=True)
        del A, base


def potrf_streams():
    torch = _torch()
    n = 1000
    for total, groups in [(64, 1), (64, 2), (64, 4), (256, 1), (256, 2), (256, 4), (1024, 1), (1024, 4)]:
        ctxs = [_lib.Context(0) for _ in range(groups)]
        g = torch.Generator(device="cuda").manual_seed(0)
        G = torch.randn(total, n, n, dtype=torch.float64, device="cuda", generator=g) / n ** 0.5
        base = torch.baddbmm(torch.eye(n, dtype=torch.float64, device="cuda").expand(total, n, n), G,
                             G.transpose(1, 2))
        del G
        A = base.clone()
        info = torch.zeros(total, dtype=torch.int32, device="cuda")
        per, best = total // groups, None
        for _ in range(4):
            A.copy_(base)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, c in enumerate(ctxs):
                _lib._chk(_lib._L.gpmpc_potrf_batched_dev(c.h, n, per, A[i * per].data_ptr(), n, n * n,
                                                           info[i * per:].data_ptr()), "potrf")
            for c in ctxs:
                c.sync()
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
        assert int(info.abs().sum()) == 0
        print(f"total={total} groups={groups}: {best * 1e3:.3f} ms  "
              f"{total * n ** 3 / 3 / best / FP64_PEAK * 100:.1f}% peak", flush=True)
        del A, base
        for c in ctxs:
            c.close()


def _syrk_timed(n, k, beta, seed, reps):
    torch = _torch()
    ctx = _lib.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(n, k, dtype=torch.float64, device="cuda", generator=g) / k ** 0.5
    C = torch.eye(n, dtype=torch.float64, device="cuda") if beta else torch.zeros(n, n, dtype=torch.float64,
                                                                                   device="cuda")
    ts = []
    for it in range(reps + 3):
        e0, e1 = _events(torch, stream, lambda: _lib._chk(_lib._L.gpmpc_syrk_batched_dev(
            ctx.h, n, k, 1, A.data_ptr(), k, 0, C.data_ptr(), n, 0, 1.0, beta), "syrk"))
        ctx.sync()
        if it >= 3:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    fl = n * (n + 1) * k  # lower triangle incl. diagonal, 2 flop per multiply-add
    return A, C, dict(n=n, k=k, min_ms=round(min(ts) * 1e3, 4), median_ms=round(float(np.median(ts)) * 1e3, 4),
                      frac_min=round(fl / min(ts) / FP64_PEAK, 4),
                      frac_median=round(fl / float(np.median(ts)) / FP64_PEAK, 4))


def syrk_fitc():
    print(json.dumps(_syrk_timed(2000, 4000, 1.0, 3, 30)[2]))


def gemm_loop(n="3968"):
    """n = k = 3968: 31 row tiles, 496 lower tiles, one round of 512 resident workgroups,
    248 K steps each (STORE epilogue, beta = 0: no split-K / stream-K)."""
    torch = _torch()
    A, C, r = _syrk_timed(int(n), int(n), 0.0, 5, 10)
    r["maxerr"] = float((torch.tril(C[:256, :256]) - torch.tril(A[:256] @ A[:256].T)).abs().max())
    print(json.dumps(r))


def trsm():
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    for n, nrhs in ((128, 64), (128, 3), (1000, 3), (1000, 1000)):
        A = rs.randn(n, n)
        L = np.linalg.cholesky(A @ A.T / n + np.eye(n))
        B = rs.randn(n, nrhs)
        for _ in range(5):
            _lib.trsm_lower(ctx, L, B)
            _lib.potrs(ctx, L, B)
    print("done", flush=True)


# ---- configs[4] ----------------------------------------------------------------------------
def rollouts6(batches="64,512"):
    import bench
    bs = tuple(int(v) for v in batches.split(","))
    print(json.dumps(bench.rollouts6_bench(_lib.Context(0), _torch(), batches=bs)), flush=True)


def qp_sweep(B="64", settings="50:1e-4,100:1e-4,200:1e-4,400:1e-4,1000:1e-4,4000:1e-4"):
    """At which ADMM settings does the configs[4] controller return "solved" for >= 90% of
    its QPs?  Per (max_iter, eps): the status histogram and the to-termination timing."""
    import bench
    from gp_mpc_rocket_landing_amd.rollouts6 import Rollouts6, fit_structured_fitc, initial_conditions_6dof
    ctx = _lib.Context(0)
    gv, gw = fit_structured_fitc(ctx, n_train=4000, n_inducing=2000)
    B = int(B)
    for mi, eps in (tuple(float(x) for x in t.split(":")) for t in settings.split(",")):
        qp = dict(max_iter=int(mi), eps_abs=eps, eps_rel=eps)
        st = bench.rollouts6_qp_status(ctx, gv, gw, B, **qp)
        ro = Rollouts6(ctx, gv, gw, B, **qp)
        ro.reset(initial_conditions_6dof(B)); ro.step(1); ctx.sync()
        ro.reset(initial_conditions_6dof(B)); ctx.sync()
        t0 = time.perf_counter(); steps = 0
        while steps < 301:
            ro.step(10); steps += 10
            if np.all(ro.read()[0][:, 0] != 0):
                break
        el = time.perf_counter() - t0
        ro.close()
        print(json.dumps({"max_iter": int(mi), "eps": eps, "ms_per_step": round(el / steps * 1e3, 3),
                          "rollouts_per_s": round(B / el, 1), **st}), flush=True)


def _surface(leg, reps, prof):
    import bench
    ctx = _lib.default_context()
    fn = getattr(bench, leg)
    if prof != "prof":
        print(json.dumps(fn(ctx, reps=int(reps))), flush=True)
        return
    import cProfile
    import pstats
    fn(ctx, reps=1)  # warm
    pr = cProfile.Profile()
    pr.enable()
    print(json.dumps(fn(ctx, reps=1)), flush=True)
    pr.disable()
    pstats.Stats(pr).sort_stats("tottime").print_stats(30)
    pstats.Stats(pr).sort_stats("cumulative").print_stats(40)


def surface(reps="2", prof=""):
    _surface("surface_single_landing_bench", reps, prof)


def surface6(reps="2", prof=""):
    _surface("surface_gpmpc6_bench", reps, prof)


# ---- novelty selection --------------------------------------------------------------------
def _greedy_numpy(X, scores, n_select, w=0.5):
    """The reference's select_diverse loop restated with a running minimum: O(n_select) numpy
    calls where the reference makes O(n_select^2 n), so the stricter CPU baseline."""
    mind = np.full(len(X), np.inf); free = np.ones(len(X), bool); idx = []
    for t in range(n_select):
        v = scores.copy() if t == 0 else scores + w * mind
        v[~free] = -np.inf
        p = int(np.argmax(v))
        idx.append(p); free[p] = False
        mind = np.minimum(mind, np.linalg.norm(X - X[p], axis=1))
    return np.array(idx)


def _median_ms(fn, reps):
    fn()   # warm-up: code objects, pool blocks
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()   # every timed call ends in a stream synchronise
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def novelty(reps="7"):
    from gp_mpc_rocket_landing_amd.learning import NoveltyConfig, NoveltySelector
    reps = int(reps)
    ctx = _lib.default_context()
    rng = np.random.default_rng(0)
    d = 5
    # 1. the two paths over n (whole call: copies in, kernels, copies out)
    for n in (256, 1024, 2048, 4096, 8192, 16384, 65536):
        X = rng.standard_normal((n, d)); sc = rng.uniform(0, 1, n)
        row = dict(probe="select_paths", n=n, d=d, n_select=100)
        picks = {}
        for path in (1, 2):
            if path == 1 and n > _lib.SELECT_ONE_MAXN:
                continue
            picks[path] = _lib.select_diverse(ctx, X, sc, 100, path=path)[0]
            row[f"path{path}_ms"] = _median_ms(lambda: _lib.select_diverse(ctx, X, sc, 100, path=path), reps)
        row["paths_agree"] = bool(all(np.array_equal(v, picks[2]) for v in picks.values()))
        print(json.dumps(row), flush=True)
    # 2. the surface against the numpy restatement
    R = rng.standard_normal((1000, d))
    for n, n_select, cpu in ((2000, 200, True), (6000, 5000, True), (300000, 100, False)):
        X = rng.standard_normal((n, d))
        sel = NoveltySelector(NoveltyConfig(distance_threshold=3.0))
        sel.set_reference_data(R)
        sc = sel.compute_novelty_scores(X)
        row = dict(probe="select_diverse", n=n, d=d, n_select=n_select, r=1000)
        got = sel.select_diverse(X, n_select=n_select)
        row["surface_ms"] = _median_ms(lambda: sel.select_diverse(X, n_select=n_select), reps)
        row["scores_ms"] = _median_ms(lambda: sel.compute_novelty_scores(X), reps)   # nn_dist + host numpy
        row["nn_dist_ms"] = _median_ms(lambda: _lib.nn_dist(ctx, X, R), reps)
        for path in (1, 2):
            if path == 1 and n > _lib.SELECT_ONE_MAXN:
                continue
            row[f"path{path}_ms"] = _median_ms(lambda: _lib.select_diverse(ctx, X, sc, n_select, path=path), reps)
        if cpu:
            t0 = time.perf_counter()
            want = _greedy_numpy(X, sc, n_select)
            row["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
            row["picks_equal_numpy"] = bool(np.array_equal(got, want))
        print(json.dumps(row), flush=True)
    # 3. the distance kernel
    X = rng.standard_normal((300000, d))
    row = dict(probe="nn_dist", n=300000, r=1000, d=d)
    row["call_ms"] = _median_ms(lambda: _lib.nn_dist(ctx, X, R), reps)
    sub = _lib.nn_dist(ctx, X[:2000], R)
    row["equal_numpy_2000"] = bool(np.array_equal(sub, np.min(np.linalg.norm(X[:2000, None] - R, axis=2), axis=1)))
    print(json.dumps(row), flush=True)


def unscented(reps="5"):
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from gp_mpc_rocket_landing_amd.dynamics import Rocket6DoFConfig, Rocket6DoFDynamics, create_normalized_rocket
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    from gp_mpc_rocket_landing_amd.rollouts6 import fit_structured_gp, initial_conditions_6dof
    reps = int(reps)
    N = 20
    X, U, D = synthetic_training_data(1000, seed=0)

    def gp3(sparse):
        np.random.seed(0)
        g = Simple3DoFGP(use_sparse=sparse)
        g.add_data(X, U, D); g.fit()
        return g

    legs = [("3dof", "exact n=1000", lambda: gp3(False)), ("3dof", "fitc M=50", lambda: gp3(True)),
            ("6dof", "exact n=1000", lambda: fit_structured_gp(1000, 50, use_sparse=False)),
            ("6dof", "fitc M=50", lambda: fit_structured_gp(1000, 50)),
            ("6dof", "fitc M=2000", lambda: fit_structured_gp(4000, 2000))]
    for model, name, make in legs:
        gp = make()
        for B in (1, 64):
            rs = np.random.RandomState(B)
            if model == "3dof":
                dyn = create_normalized_rocket()
                X0 = _fleet().initial_conditions(B)
                Uh = np.tile((-X0[:, 0:1] * np.array([-1.0, 0, 0]))[:, None, :], (1, N, 1)) * (1 + 0.1 * rs.randn(B, N, 1))
            else:
                dyn = Rocket6DoFDynamics(Rocket6DoFConfig())
                X0 = initial_conditions_6dof(B)
                Uh = np.zeros((B, N, 3))
                Uh[:, :, 2] = 0.9 * X0[:, 0:1] * Rocket6DoFConfig().g0
                Uh[:, :, :2] = 0.05 * rs.randn(B, N, 2)
            p = UncertaintyPropagator(dyn, gp, method="unscented")
            row = dict(probe="unscented", model=model, gp=name, B=B, N=N, ut=list(p.ut_params))

            # At the reference's alpha = 1e-3 the centre weight is ~ -1e6, and over a GP whose mean
            # coefficients are large the recursion's own rounding can leave a covariance indefinite:
            # either path then raises LinAlgError.  Each trajectory is kept or dropped on its own.
            def device():
                return p._device_unscented(X0, Uh, None, 0.1)   # the one call the surface makes

            def host():
                out = []
                for b in range(B):
                    try:
                        out.append(p.propagate_unscented_batch(X0[b:b + 1], Uh[b:b + 1], None, 0.1))
                    except np.linalg.LinAlgError:
                        out.append(None)
                return out

            md, cd, info = device()
            row["device_ms"] = _median_ms(device, reps)
            p.use_device = False
            hl = host()
            row["host_loop_ms"] = _median_ms(host, max(2, reps // 2))
            both = [b for b in range(B) if info[b] == 0 and hl[b] is not None]
            row["device_stopped"] = int(np.count_nonzero(info)); row["host_stopped"] = sum(h is None for h in hl)
            row["means_maxdiff"] = max(float(np.abs(md[b] - hl[b][0][0]).max()) for b in both)
            row["covs_maxdiff"] = max(float(np.abs(cd[b] - hl[b][1][0]).max()) for b in both)
            print(json.dumps(row), flush=True)


def mc(reps="3"):
    from gp_mpc_rocket_landing_amd.data import synthetic_training_data
    from gp_mpc_rocket_landing_amd.dynamics import Rocket6DoFConfig, Rocket6DoFDynamics, create_normalized_rocket
    from gp_mpc_rocket_landing_amd.gp import Simple3DoFGP
    from gp_mpc_rocket_landing_amd.mpc import UncertaintyPropagator
    from gp_mpc_rocket_landing_amd.rollouts6 import fit_structured_gp, initial_conditions_6dof
    reps = int(reps)
    N = 20
    X, U, D = synthetic_training_data(1000, seed=0)

    def gp3(sparse):
        np.random.seed(0)
        g = Simple3DoFGP(use_sparse=sparse)
        g.add_data(X, U, D); g.fit()
        return g

    legs = [("3dof", "exact n=1000", lambda: gp3(False)), ("3dof", "fitc M=50", lambda: gp3(True)),
            ("6dof", "fitc M=50", lambda: fit_structured_gp(1000, 50)),
            ("6dof", "exact n=1000", lambda: fit_structured_gp(1000, 50, use_sparse=False))]
    for model, name, make in legs:
        gp = make()
        for B in (1, 64):
            rs = np.random.RandomState(B)
            if model == "3dof":
                dyn = create_normalized_rocket()
                X0 = _fleet().initial_conditions(B)
                Uh = np.tile((-X0[:, 0:1] * np.array([-1.0, 0, 0]))[:, None, :], (1, N, 1)) * (1 + 0.1 * rs.randn(B, N, 1))
            else:
                dyn = Rocket6DoFDynamics(Rocket6DoFConfig())
                X0 = initial_conditions_6dof(B)
                Uh = np.zeros((B, N, 3))
                Uh[:, :, 2] = 0.9 * X0[:, 0:1] * Rocket6DoFConfig().g0
                Uh[:, :, :2] = 0.05 * rs.randn(B, N, 2)
            p = UncertaintyPropagator(dyn, gp, method="monte_carlo")
            for S in (100, 4096):
                row = dict(probe="mc", model=model, gp=name, B=B, N=N, S=S)

                def surface():   # the whole call: the draws on the host, then one device call (or the host loop)
                    np.random.seed(1)
                    return p.propagate_monte_carlo_batch(X0, Uh, None, 0.1, n_samples=S)

                def draws():
                    np.random.seed(1)
                    return p._monte_carlo_draw(X0, None, N, S)

                p.use_device = True
                md, cd = surface()
                row["device_ms"] = _median_ms(surface, reps)
                row["draws_ms"] = _median_ms(draws, reps)   # the part of device_ms that is numpy's RNG
                if S == 100:
                    p.use_device = False
                    t0 = time.perf_counter()
                    mh, ch = surface()
                    row["host_loop_ms"] = (time.perf_counter() - t0) * 1e3   # one run, no warm-up needed: numpy
                    row["means_maxdiff"] = float(np.abs(md - mh).max())
                    row["covs_maxdiff"] = float(np.abs(cd - ch).max())
                print(json.dumps(row), flush=True)


def knn(reps="7"):
    from scipy.spatial import KDTree
    reps = int(reps)
    ctx = _lib.default_context()
    rng = np.random.default_rng(0)
    # small sets, for the crossover of terminal/local_safe_set.py: the KD-tree answers them in
    # microseconds, a device call never costs less than its launches and copies
    for n, d in ((512, 7), (4096, 7), (16384, 7)):
        S = np.cumsum(rng.standard_normal((n // 64, 64, d)) * 0.2, axis=1).reshape(n, d)
        Xall = S[rng.choice(n, 64, replace=False)] + 0.05 * rng.standard_normal((64, d))
        ks = _lib.KnnSet(ctx, S, rng.random(n))
        tree = KDTree(S)
        for B in (1, 2, 4, 8, 64):
            X = Xall[:B]
            parts, qw = _lib.knn_plan(n, d, B)
            row = dict(probe="knn_small", n=n, d=d, B=B, parts=parts, q_per_wave=qw)
            row["query_ms"] = _median_ms(lambda: ks.query(X, 64, 1.0), reps)

            def scipy_small():
                for x in X:
                    tree.query(x, k=50)
                    tree.query_ball_point(x, 1.0)
            row["scipy_loop_ms"] = _median_ms(scipy_small, reps)
            print(json.dumps(row), flush=True)
        ks.close()
    for n, d in ((131072, 7), (65536, 14)):
        # a trajectory log in the small: correlated rows, the queries near stored rows
        S = np.cumsum(rng.standard_normal((n // 64, 64, d)) * 0.2, axis=1).reshape(n, d)
        q = rng.random(n)
        Xall = S[rng.choice(n, 1024, replace=False)] + 0.05 * rng.standard_normal((1024, d))
        t0 = time.perf_counter()
        ks = _lib.KnnSet(ctx, S, q)
        create_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        tree = KDTree(S)
        build_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(probe="knn_set", n=n, d=d, knn_create_ms=create_ms, kdtree_build_ms=build_ms)),
              flush=True)
        flops_row = 3 * d   # a difference, a square and an addition per feature and (query, row)
        for B in (1, 64, 1024):
            X = Xall[:B]
            parts, qw = _lib.knn_plan(n, d, B)
            row = dict(probe="knn", n=n, d=d, B=B, parts=parts, q_per_wave=qw)
            row["query_ms"] = _median_ms(lambda: ks.query(X, 64, 1.0), reps)
            row["interp_ms"] = _median_ms(lambda: ks.interp(X, 10, 4, 50, True, 1.0), reps)
            row["query_gflops_whole_call"] = flops_row * n * B / (row["query_ms"][0] * 1e-3) / 1e9

            def scipy_loop():
                for x in X:
                    tree.query(x, k=50)
                    tree.query_ball_point(x, 1.0)
            row["scipy_loop_ms"] = _median_ms(scipy_loop, reps)
            idx, dist, nb, _ = ks.query(X[:16], 50, 1.0)
            same = True
            for b, x in enumerate(X[:16]):
                dd, ii = tree.query(x, k=50)
                same = same and np.array_equal(ii, idx[b]) and np.array_equal(dd, dist[b]) and \
                    len(tree.query_ball_point(x, 1.0)) == nb[b]
            row["equal_scipy_16"] = bool(same)
            print(json.dumps(row), flush=True)
        ks.close()


def hull(reps="7", device_only=""):
    """TerminalSetManager.project_batch for 1024 states over safe sets of 4096 rows (7 and 14
    states, K = 10 and K = 50), the fused device call against the numpy restatement of the
    contract (tests/hull_check.py) looped over the same vertex sets.  device_only: the device
    calls alone, for a kernel trace."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import hull_check as hc
    from gp_mpc_rocket_landing_amd.terminal import SampledSafeSet, TerminalSetManager
    reps = int(reps)
    os.environ["GPMPC_KNN"] = "device"
    rng = np.random.default_rng(0)
    for n_x in (7, 14):
        ss = SampledSafeSet(n_x=n_x, n_u=3)
        for _ in range(64):   # a trajectory log in the small: 64 walks of 64 states
            ss.add_trajectory(np.cumsum(rng.standard_normal((64, n_x)) * 0.2, axis=0), np.zeros((63, 3)), np.ones(63))
        S = ss.get_all_states()
        X = S[rng.choice(len(S), 1024, replace=False)] + 0.05 * rng.standard_normal((1024, n_x))
        for K in (10, 50):
            tm = TerminalSetManager(ss, n_vertices=K)
            row = dict(probe="hull", n=len(S), n_x=n_x, B=len(X), K=K)
            row["project_batch_ms"] = _median_ms(lambda: tm.project_batch(X), reps)
            out = tm.project_batch(X)
            row["status_counts"] = {int(k): int(v) for k, v in Counter(out["status"].tolist()).items()}
            row["k_used"] = [int(out["k_used"].min()), int(out["k_used"].max())]
            row["inside"] = int(np.sum(out["dist"] <= 1e-6))
            if not device_only:
                sets = [(S[out["idx"][b, :out["k_used"][b]]], X[b]) for b in range(len(X))]
                res = []

                def numpy_loop():
                    res[:] = [hc.wolfe(V, x) for V, x in sets]
                row["numpy_loop_ms"] = _median_ms(numpy_loop, min(reps, 3))
                row["numpy_status_counts"] = {int(k): int(v) for k, v in Counter(r["status"] for r in res).items()}
                row["max_cycles_numpy"] = int(max(r["iters"] for r in res))
                row["max_rel_err_vs_numpy"] = float(max(hc.rel_err(out["proj"][b], res[b]["proj"], *sets[b])
                                                        for b in range(len(X))))
            print(json.dumps(row), flush=True)


COMMANDS = dict(hull=hull, knn=knn, mc=mc, unscented=unscented, novelty=novelty, single=single, step=step, stamps=stamps, placement=placement, streams=streams, fit=fit,
                append=append, chol=chol, potrf=potrf, potrf_streams=potrf_streams, syrk_fitc=syrk_fitc,
                gemm_loop=gemm_loop, trsm=trsm, rollouts6=rollouts6, qp_sweep=qp_sweep, surface=surface,
                surface6=surface6)

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in COMMANDS:
        sys.exit(__doc__)
    COMMANDS[sys.argv[1]](*sys.argv[2:])
