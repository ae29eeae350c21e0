"""The GEMM launchers' dispatch as it stood before csrc/gemm_plan.h existed: a transcription
of commit d721b0c's gemm.hip:947-1213 (launch_splitk, launch_splitk_sumsq, gemm_sumsq_kind,
launch_gemm_impl, launch_gemm_nn, launch_gemm_nn_batched, launch_gemm_tn,
launch_gemm_nt_rowblock), statement by statement, over numpy arrays of requests.  It is the
oracle of tests/test_gemm_plan.py: whoever changes a rule in gemm_plan.h changes it here
in the same commit, on purpose.

A request is a dict of equally long integer arrays: op (GEMM_OP code), M, N, K, batch, beta1
(beta == 1.0), tri_a, lower_c, p0 (row-block: ksplit; SUMSQ: the forced kind), p1 (SUMSQ_MEAN:
n_out), no_scratch (gpmpc_scratch would return null).  M, N, K are the arguments of
gpmpc_gemm_diag: the SUMSQ launchers multiply an (M + p1) x K matrix.  The answer is an
(n, 8) array: path, split, grid, gx, gy, gz, tile height, kc."""
import numpy as np

GT, GK, BT = 64, 16, 128
NT, NN, NN_BATCHED, TN, ROWBLOCK, SUMSQ, SUMSQ_MEAN = 0, 1, 2, 3, 4, 9, 10
PATH_NONE, PATH_64, PATH_128, PATH_128_KSPLIT, PATH_STREAMK, PATH_SPLITK = -1, 0, 1, 2, 3, 4
GRID_2D, GRID_TRI, GRID_XCD_BATCH, GRID_ROWBLOCK_XCD = 0, 1, 2, 3
SUMSQ_64, SUMSQ_128, SUMSQ_SPLITK = 0, 1, 2


def cdiv(a, b):
    return (a + b - 1) // b


def _chunks(K, tiles):
    """S = max(1, min(512 / tiles, K / 64)); kc = roundup(ceil(K / S), GK); S = ceil(K / kc)."""
    S0 = np.maximum(1, np.minimum(512 // np.maximum(tiles, 1), K // 64))
    kc = cdiv(cdiv(K, S0), GK) * GK
    return S0, cdiv(K, np.maximum(kc, 1)), kc


def _splitk(pol, M, N, K, no_scratch):
    """launch_splitk (954-962): taken, S, kc."""
    S0, S, kc = _chunks(K, cdiv(M, GT) * cdiv(N, GT))
    return (pol["splitk"] != 0) & ((M <= 32) | (N <= 32)) & (K >= 256) & (S0 >= 2) & (no_scratch == 0), S, kc


def _splitk_sumsq(pol, M, N, K, no_scratch):
    """launch_splitk_sumsq (1021-1029): taken, S, kc."""
    S0, S, kc = _chunks(K, cdiv(M, GT))
    return (pol["splitk"] != 0) & (N <= GT) & (K >= 256) & (S0 >= 2) & (no_scratch == 0), S, kc


def sumsq_kind(pol, M, N, K):
    """gemm_sumsq_kind (1047-1052)."""
    S0, _, _ = _chunks(K, cdiv(M, GT))
    big = (pol["big"] != 0) & (M >= 2 * BT) & (N >= 2 * BT) & (K >= pol["kmin"])
    split = (pol["splitk"] != 0) & (N <= GT) & (K >= 256) & (S0 >= 2)
    return np.where(big, SUMSQ_128, np.where(split, SUMSQ_SPLITK, SUMSQ_64))


class _Out:
    """Rows are decided once, by the first rule that takes them (the launchers return there)."""

    def __init__(self, n):
        self.a = np.zeros((n, 8), np.int64)
        self.a[:, 0], self.a[:, 6] = PATH_NONE, GT
        self.open = np.ones(n, bool)

    def take(self, mask, path, split, grid, gx, gy, gz, tile, kc=0):
        m = self.open & mask
        for j, v in enumerate((path, split, grid, gx, gy, gz, tile, kc)):
            self.a[m, j] = np.broadcast_to(v, m.shape)[m]
        self.open &= ~m


def _impl(pol, out, sel, sumsq, M, N, K, batch, beta1, tri_a, lower_c, kind, no_scratch):
    """launch_gemm_impl (1054-1150) for the rows of sel."""
    store = ~sumsq
    out.take(sel & ((M <= 0) | (N <= 0)), PATH_NONE, 0, 0, 0, 0, 0, GT)
    kind = np.where(store | (batch != 1), -1, kind)
    tg = (lower_c != 0) & (M == N) & (tri_a == 0)
    t128 = cdiv(M, BT) * (cdiv(M, BT) + 1) // 2 * batch
    s128 = pol["syrk128"]
    tri_ok = ~tg | ((s128 != 0) if s128 >= 0 else ((t128 >= 1024) | (K >= 1024)))
    sk_ok = store & beta1 & (tri_a == 0) & (M >= 2 * BT) & (N >= 2 * BT) & (K >= 2 * BT)
    sk_auto = (M >= 768) & (N >= 768) & (K >= 512)
    tx, ty = cdiv(N, BT), cdiv(M, BT)
    T = np.where(tg, ty * (ty + 1) // 2, tx * ty)
    total = T * batch * cdiv(K, GK)
    nwg = np.minimum(512, total)
    grid = np.where(tg, GRID_TRI, GRID_2D)
    out.take(sel & sk_ok & ((pol["streamk"] > 0) if pol["streamk"] >= 0 else sk_auto), PATH_STREAMK, nwg, grid,
             nwg, 1, 1, BT)
    use128 = np.where(kind >= 0, kind == SUMSQ_128,
                      (pol["big"] != 0) & tri_ok & (M >= 2 * BT) & (N >= 2 * BT) & (K >= pol["kmin"]))
    tiles = np.where(lower_c != 0, ty * (ty + 1) // 2, tx * ty) * batch
    ksplit = np.ones_like(M)
    model = store & beta1 & (K >= 1024)
    best = np.full(M.shape, 1e30)
    for ks in range(1, 17):
        c = ((tiles * ks + 511) // 512).astype(np.float64) * (K.astype(np.float64) / ks + 256.0)
        better = model & (ks <= K // 256) & (c < best * 0.98)
        best = np.where(better, c, best)
        ksplit = np.where(better, ks, ksplit)
    if pol["ksplit"] > 0:
        ksplit = np.where(store & beta1, pol["ksplit"], ksplit)
    out.take(sel & use128, np.where(ksplit > 1, PATH_128_KSPLIT, PATH_128), ksplit, grid,
             np.where(tg, ty * (ty + 1) // 2, tx), np.where(tg, 1, ty), batch * ksplit, BT)
    ok, S, kc = _splitk(pol, M, N, K, no_scratch)
    out.take(sel & store & (batch == 1) & (tri_a == 0) & (lower_c == 0) & ok, PATH_SPLITK, S, GRID_2D,
             cdiv(N, GT), cdiv(M, GT), S, GT, kc)
    ok, S, kc = _splitk_sumsq(pol, M, N, K, no_scratch)
    wants = np.where(kind >= 0, kind == SUMSQ_SPLITK, sumsq_kind(pol, M, N, K) != SUMSQ_128)
    out.take(sel & sumsq & (batch == 1) & wants & ok, PATH_SPLITK, S, GRID_2D, 1, cdiv(M, GT), S, GT, kc)
    tx, ty = cdiv(N, GT), cdiv(M, GT)
    remap = (pol["remap"] != 0) & (batch == 1) & (ty > 1) & (tx % 8 == 0)
    T = ty * (ty + 1) // 2
    xb = np.where(tg & (pol["xcd_batch"] != 0) & (batch >= 8), batch, 0)
    gx = np.where(xb != 0, T * cdiv(batch, 8) * 8, np.where(tg, T, np.where(remap, tx * ty, tx)))
    gy = np.where((xb != 0) | tg | remap, 1, ty)
    gz = np.where((xb != 0) | (~tg & remap), 1, batch)
    out.take(sel, PATH_64, 1, np.where(xb != 0, GRID_XCD_BATCH, grid), gx, gy, gz, GT)


def decide(req, pol):
    r = {k: np.asarray(v, np.int64) for k, v in req.items()}
    op, M, N, K, batch, p0 = r["op"], r["M"], r["N"], r["K"], r["batch"], r["p0"]
    beta1, no_scratch = r["beta1"] != 0, r["no_scratch"]
    out = _Out(len(op))
    # launch_gemm_nt (1215-1221); launch_gemm_sumsq / _mean (1223-1234): M = n + n_out, tri_a = 1, batch 1
    sumsq = (op == SUMSQ) | (op == SUMSQ_MEAN)
    Mi = M + np.where(op == SUMSQ_MEAN, r["p1"], 0)
    _impl(pol, out, (op == NT) | sumsq, sumsq, Mi, N, K, batch, beta1, np.where(sumsq, 1, r["tri_a"]),
          np.where(sumsq, 0, r["lower_c"]), np.where(sumsq, p0, -1), no_scratch)
    # launch_gemm_nn (1153-1165), launch_gemm_tn (1180-1192), launch_gemm_nn_batched (1168-1177)
    flat = (op == NN) | (op == TN) | (op == NN_BATCHED)
    out.take(flat & ((M <= 0) | (N <= 0) | ((op == NN_BATCHED) & (batch <= 0))), PATH_NONE, 0, 0, 0, 0, 0, GT)
    ok, S, kc = _splitk(pol, M, N, K, no_scratch)
    out.take(flat & (op != NN_BATCHED) & ok, PATH_SPLITK, S, GRID_2D, cdiv(N, GT), cdiv(M, GT), S, GT, kc)
    out.take(flat, PATH_64, 1, GRID_2D, cdiv(N, GT), cdiv(M, GT), np.where(op == NN_BATCHED, batch, 1), GT)
    # launch_gemm_nt_rowblock (1197-1213)
    rb = op == ROWBLOCK
    out.take(rb & ((M <= 0) | (N <= 0)), PATH_NONE, 0, 0, 0, 0, 0, GT)
    ks = np.where((p0 < 1) | ~beta1, 1, p0)
    xcd = (pol["rowblock_xcd"] != 0) & (batch >= 8) & (batch % 8 == 0)
    out.take(rb, np.where(ks > 1, PATH_128_KSPLIT, PATH_128), ks, np.where(xcd, GRID_ROWBLOCK_XCD, GRID_2D), 1,
             cdiv(M, BT), batch * ks, BT)
    assert not out.open.any()
    return out.a
