"""k-means for the sparse GP's inducing points: scipy's kmeans2(X, k, minit="points") with
Lloyd's iteration on the device (csrc/kmeans.hip).

The draw is scipy's own (the same ``choice`` call on the same global RandomState), so the
global RNG advances exactly as under kmeans2.  The iteration then runs on the device from
X[idx]; when the device reports a nearest-centre decision too close to call (``unsafe > 0``,
the guard of DESIGN §15) its result is discarded and scipy iterates from the same draw.
"""
from __future__ import annotations

import os
import warnings

import numpy as np
from scipy._lib._util import check_random_state
from scipy.cluster.vq import kmeans2

from .. import _lib

EMPTY_WARNING = "One of the clusters is empty. Re-run kmeans with a different initialization."


def mode() -> str:
    """GPMPC_KMEANS: ``device`` (default) or ``host`` (scipy's kmeans2 alone)."""
    m = os.environ.get("GPMPC_KMEANS", "device")
    if m not in ("device", "host"):
        raise ValueError(f"GPMPC_KMEANS must be 'device' or 'host', got {m!r}")
    return m


def device_eligible(X, k) -> bool:
    """The device path takes a finite float64 (n, d <= 32) array and an integer k >= 1."""
    return (isinstance(X, np.ndarray) and X.dtype == np.float64 and X.ndim == 2 and X.shape[0] >= 1
            and 1 <= X.shape[1] <= _lib.KMEANS_MAXD and isinstance(k, (int, np.integer)) and k >= 1
            and bool(np.all(np.isfinite(X))))


def draw_points(n, k) -> np.ndarray:
    """The indices kmeans2's minit="points" draws (vq._kpoints on check_random_state(None))."""
    return check_random_state(None).choice(n, size=int(k), replace=False)


def kmeans2_points(X, k, iter=10):
    """``kmeans2(X, k, iter=iter, minit="points")``: (code book (k, d), label (n,)), the same
    bits, warnings and use of the global RNG.  ``kmeans2_points.last_path`` tells where the
    iteration ran: "device", or "host" after the guard fired."""
    if int(iter) < 1:
        raise ValueError(f"Invalid iter ({iter}), must be a positive integer.")
    if not device_eligible(X, k):
        raise ValueError("kmeans2_points: X must be a finite float64 (n, d <= 32) array and k an integer >= 1")
    idx = draw_points(X.shape[0], k)
    C0 = np.take(X, idx, axis=0)
    C, label, empties, _, unsafe = _lib.kmeans_lloyd(_lib.default_context(), X, C0, iters=int(iter))
    if unsafe > 0:
        kmeans2_points.last_path = "host"
        return kmeans2(X, C0, iter=iter, minit="matrix")
    kmeans2_points.last_path = "device"
    for _ in range(int(np.count_nonzero(empties))):
        warnings.warn(EMPTY_WARNING, stacklevel=2)
    return C, label.astype(np.int32)


kmeans2_points.last_path = None
