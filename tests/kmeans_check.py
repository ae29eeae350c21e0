"""The oracle of the k-means tests (a helper, not a test): scipy's kmeans2 iteration restated
in numpy with the three choices csrc/kmeans.hip makes -- the distance in its direct form
summed left to right, the lowest index on equal distances, and the update in ascending
observation order with one division by the count, a cluster without members keeping its row.
test_kmeans_host.py pins it to the installed scipy bit for bit."""
import warnings

import numpy as np

# (n, d, k, seed): the shapes the restatement was compared with scipy on
TABLE = [(300, 11, 50, 0), (1000, 11, 50, 1), (200, 3, 20, 2), (97, 4, 13, 4), (130, 5, 17, 5), (64, 13, 63, 6)]
PRODUCTION = (4000, 13, 2000, 3)
ROWS = 128           # observations per block of lloyd's distance pass
MIN_MARGIN = 1e-9   # below this a test input is too close to a tie to expect the device path


def make_data(n, d, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    return X * rng.uniform(0.5, 3, d)


def sqdist(X, C):
    """|x_i - c_j|^2 (n, k), each sum taken left to right over the features."""
    d2 = np.zeros((X.shape[0], C.shape[0]))
    for f in range(X.shape[1]):
        df = X[:, f:f + 1] - C[None, :, f]
        d2 = d2 + df * df
    return d2


def lloyd(X, C0, iters=10):
    """-> (code book, labels of the last assignment, empties per iteration, min margin), the
    margin (second smallest - smallest squared distance) / (|x|^2 + max_j |c_j|^2) over every
    decision; inf with a single centre, 0 where the scale is 0."""
    X = np.ascontiguousarray(X, np.float64)
    C = np.array(C0, np.float64)
    n, d = X.shape
    k = C.shape[0]
    xx = np.zeros(n)
    for f in range(d):
        xx = xx + X[:, f] * X[:, f]
    empties, margin = [], np.inf
    label = np.zeros(n, np.int64)
    for _ in range(iters):
        cc = np.zeros(k)
        for f in range(d):
            cc = cc + C[:, f] * C[:, f]
        for r0 in range(0, n, ROWS):    # row blocks: the (rows, k) distances stay in cache
            d2 = sqdist(X[r0:r0 + ROWS], C)
            label[r0:r0 + ROWS] = np.argmin(d2, axis=1)   # the first index of the minimum
            if k > 1:
                part = np.partition(d2, 1, axis=1)[:, :2]
            else:
                part = np.concatenate([d2, np.full_like(d2, np.inf)], axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                scale = xx[r0:r0 + ROWS] + cc.max()
                m = (part[:, 1] - part[:, 0]) / scale
            margin = min(margin, float(np.min(np.where((m >= 0) & (scale > 0), m, 0.0))))
        new = np.zeros_like(C)
        count = np.zeros(k, np.int64)
        for i in range(n):              # ascending observation order, plain rounded adds
            new[label[i]] += X[i]
            count[label[i]] += 1
        has = count > 0
        new[has] /= count[has][:, None]
        new[~has] = C[~has]
        empties.append(int(np.sum(~has)))
        C = new
    return C, label, np.array(empties), margin


def margin_expanded(X, C0, iters=10):
    """lloyd's min margin at a size where lloyd itself takes seconds: the same quantity from
    |x|^2 + |c|^2 - 2 x.c through one matrix product per iteration, the code books being
    scipy's own (kmeans2 one iteration at a time).  The two forms differ by the distance
    rounding, some 1e-15 of the scale: nothing against the 1e-9 this is compared with."""
    from scipy.cluster.vq import kmeans2
    X = np.ascontiguousarray(X, np.float64)
    C = np.array(C0, np.float64)
    xx = np.sum(X * X, axis=1)
    margin = np.inf
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(iters):
            cc = np.sum(C * C, axis=1)
            d2 = xx[:, None] + cc[None, :] - 2.0 * (X @ C.T)
            part = np.partition(d2, 1, axis=1)[:, :2]
            margin = min(margin, float(np.min((part[:, 1] - part[:, 0]) / (xx + cc.max()))))
            C, _ = kmeans2(X, C, iter=1, minit="matrix")
    return margin


def scipy_points(X, k, seed, iters=10):
    """kmeans2(X, k, minit="points") under np.random.seed(seed): (code book, labels, idx drawn)."""
    from scipy.cluster.vq import kmeans2
    np.random.seed(seed)
    idx = np.random.choice(X.shape[0], size=k, replace=False)
    np.random.seed(seed)
    C, label = kmeans2(X, k, iter=iters, minit="points")
    return C, label, idx
