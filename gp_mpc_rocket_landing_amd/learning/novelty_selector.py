"""Novelty-based choice of GP training data (reference src/learning/novelty_selector.py):
NoveltyConfig, NoveltySelector, ActiveDataSelector, DataBuffer with the reference's names,
signatures, defaults and return values.

The two loops of the reference that scale with the data run on the device through the
C-ABI: the nearest-reference distance (gpmpc_nn_dist, instead of the KD-tree / brute-force
numpy query) and the greedy farthest-point loop of select_diverse (gpmpc_select_diverse,
instead of the Python double loop).  Both sum in numpy's order, so
select_diverse returns the reference's indices for the same scores.  The GP terms go
through the model's own predict, which is on the device already.  There is no CPU
fallback for the device calls.

One difference from the reference: a model whose predict returns a GPPrediction (ExactGP)
is read through its mean / variance fields; the reference unpacks a tuple, which only the
multi-output models return.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .. import _lib


@dataclass
class NoveltyConfig:
    """novelty_selector.py:34-57."""
    method: str = "combined"          # "distance", "uncertainty", "residual", "combined"
    distance_threshold: float = 0.1
    distance_weight: float = 1.0
    uncertainty_threshold: float = 0.5
    uncertainty_weight: float = 1.0
    residual_threshold: float = 0.1
    residual_weight: float = 0.5
    score_threshold: float = 0.3
    max_points: int = 5000


def _mean_var(pred):
    """(mean, variance) of a model's predict result: a GPPrediction or a pair."""
    if hasattr(pred, "variance"):
        return pred.mean, pred.variance
    mean, var = pred
    return mean, var


class NoveltySelector:
    """novelty_selector.py:60-296."""

    def __init__(self, config: Optional[NoveltyConfig] = None):
        self.config = config or NoveltyConfig()
        self._reference_data: Optional[np.ndarray] = None
        self._gp_model = None

    def set_reference_data(self, X) -> None:
        self._reference_data = X.copy()

    def set_gp_model(self, gp_model) -> None:
        self._gp_model = gp_model

    def compute_novelty_scores(self, X, Y=None) -> np.ndarray:
        """The weighted sum of the method's terms over its maximum (:110-152)."""
        n = len(X)
        if n == 0:
            return np.array([])
        cfg = self.config
        scores = np.zeros(n)
        if cfg.method in ("distance", "combined"):
            scores += cfg.distance_weight * self._compute_distance_novelty(X)
        if cfg.method in ("uncertainty", "combined") and self._gp_model is not None:
            scores += cfg.uncertainty_weight * self._compute_uncertainty_novelty(X)
        if cfg.method in ("residual", "combined") and Y is not None:
            scores += cfg.residual_weight * self._compute_residual_novelty(Y)
        top = np.max(scores)
        if top > 0:
            scores = scores / top
        return scores

    def _compute_distance_novelty(self, X) -> np.ndarray:
        """1 - exp(-dist / distance_threshold), dist to the nearest reference row on the
        device (:154-170); ones without reference data."""
        ref = self._reference_data
        if ref is None or len(ref) == 0:
            return np.ones(len(X))
        distances = _lib.nn_dist(_lib.default_context(), X, ref)
        return 1.0 - np.exp(-distances / self.config.distance_threshold)

    def _compute_uncertainty_novelty(self, X) -> np.ndarray:
        """The model's predictive variance (summed over outputs) over the threshold, capped
        at 1; ones when the model's predict fails (:172-191)."""
        if self._gp_model is None:
            return np.ones(len(X))
        try:
            _, var = _mean_var(self._gp_model.predict(X))
            if var.ndim > 1:
                var = np.sum(var, axis=1)
            scores = np.minimum(var / self.config.uncertainty_threshold, 1.0)
        except Exception:
            scores = np.ones(len(X))
        return scores

    def _compute_residual_novelty(self, Y) -> np.ndarray:
        """|residual| over the threshold, capped at 1 (:193-202)."""
        mag = np.linalg.norm(Y, axis=1) if Y.ndim > 1 else np.abs(Y)
        return np.minimum(mag / self.config.residual_threshold, 1.0)

    def select(self, X, Y=None, n_select: Optional[int] = None, return_scores: bool = False):
        """The n_select highest scores, or everything at or above score_threshold
        (:204-235)."""
        scores = self.compute_novelty_scores(X, Y)
        if n_select is None:
            indices = np.where(scores >= self.config.score_threshold)[0]
        elif n_select >= len(scores):
            indices = np.arange(len(scores))
        else:
            indices = np.argsort(scores)[-n_select:]
        if return_scores:
            return indices, scores
        return indices

    def select_diverse(self, X, Y=None, n_select: int = 100) -> np.ndarray:
        """Greedy farthest-point picks by novelty + 0.5 * distance to the picked set
        (:237-296), on the device."""
        n = len(X)
        if n_select >= n:
            return np.arange(n)
        scores = self.compute_novelty_scores(X, Y)
        idx, _ = _lib.select_diverse(_lib.default_context(), X, scores, n_select, 0.5)
        return idx


class ActiveDataSelector:
    """novelty_selector.py:299-372."""

    def __init__(self, gp_model, acquisition: str = "uncertainty"):
        self.gp_model = gp_model
        self.acquisition = acquisition

    def compute_acquisition(self, X) -> np.ndarray:
        """"expected_improvement" (:339-356); "uncertainty" and any other name: the
        predictive variance, summed over outputs."""
        mean, var = _mean_var(self.gp_model.predict(X))
        if self.acquisition == "expected_improvement":
            y_best = np.min(self.gp_model._Y) if hasattr(self.gp_model, "_Y") else 0
            std = np.sqrt(var)
            z = (y_best - mean) / (std + 1e-10)
            from scipy.stats import norm  # noqa: PLC0415
            values = (y_best - mean) * norm.cdf(z) + std * norm.pdf(z)
        else:
            values = var
        if values.ndim > 1:
            return np.sum(values, axis=1)
        return values

    def select(self, X, n_select: int) -> np.ndarray:
        values = self.compute_acquisition(X)
        if n_select >= len(values):
            return np.arange(len(values))
        return np.argsort(values)[-n_select:]


class DataBuffer:
    """A bounded store of (X, Y) rows that prunes by select_diverse when it overflows
    (novelty_selector.py:375-447)."""

    def __init__(self, max_size: int = 5000, novelty_selector: Optional[NoveltySelector] = None):
        self.max_size = max_size
        self.selector = novelty_selector or NoveltySelector()
        self._X: Optional[np.ndarray] = None
        self._Y: Optional[np.ndarray] = None

    def add(self, X_new, Y_new) -> int:
        """Returns the number of rows added; after a prune, the reference's count of kept new
        rows as it is written there (:433-436): against the buffer's length after the prune."""
        if self._X is None:
            self._X = X_new.copy()
            self._Y = Y_new.copy()
            return len(X_new)
        X_all = np.vstack([self._X, X_new])
        Y_all = np.vstack([self._Y, Y_new])
        if len(X_all) <= self.max_size:
            self._X, self._Y = X_all, Y_all
            return len(X_new)
        self.selector.set_reference_data(X_all)
        keep = self.selector.select_diverse(X_all, Y_all, n_select=self.max_size)
        self._X = X_all[keep]
        self._Y = Y_all[keep]
        return np.sum(keep >= len(self._X) - len(X_new))

    def get_data(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._X is None:
            return np.array([]), np.array([])
        return self._X.copy(), self._Y.copy()

    @property
    def size(self) -> int:
        return len(self._X) if self._X is not None else 0
