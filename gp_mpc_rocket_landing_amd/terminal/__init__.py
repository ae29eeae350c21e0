"""Terminal ingredients of learning MPC (reference src/terminal): the sampled safe set of flown
landings, the local safe set of K nearest safe states and the cost-to-go approximators.  The
neighbour searches run on the device (csrc/knn.hip).  Not restated: the CasADi
convex hull (convex_hull.py) and memory_safe_set.py."""
from .local_safe_set import LocalSafeSet, LocalSafeSetConfig, MultiResolutionLocalSafeSet
from .q_function import (GPQFunction, InverseDistanceQFunction, IterativeQFunction, LocalLinearQFunction,
                         QFunctionApproximator, QFunctionConfig, QFunctionManager)
from .safe_set import FuelAwareSafeSet, SampledSafeSet, TrajectoryData

__all__ = ["LocalSafeSet", "LocalSafeSetConfig", "MultiResolutionLocalSafeSet", "GPQFunction",
           "InverseDistanceQFunction", "IterativeQFunction", "LocalLinearQFunction", "QFunctionApproximator",
           "QFunctionConfig", "QFunctionManager", "FuelAwareSafeSet", "SampledSafeSet", "TrajectoryData"]
