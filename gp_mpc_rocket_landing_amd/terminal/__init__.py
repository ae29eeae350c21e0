"""Terminal ingredients of learning MPC (reference src/terminal): the sampled safe set of flown
landings, the local safe set of K nearest safe states, the cost-to-go approximators and the
convex-hull terminal constraint.  The neighbour searches and the hull projections run on the
device (csrc/knn.hip; csrc/hull.hip).  Not restated: the CasADi form of
the hull constraint and memory_safe_set.py."""
from .convex_hull import ConvexHullConfig, ConvexHullConstraint, TerminalSetManager
from .local_safe_set import LocalSafeSet, LocalSafeSetConfig, MultiResolutionLocalSafeSet
from .q_function import (GPQFunction, InverseDistanceQFunction, IterativeQFunction, LocalLinearQFunction,
                         QFunctionApproximator, QFunctionConfig, QFunctionManager)
from .safe_set import FuelAwareSafeSet, SampledSafeSet, TrajectoryData

__all__ = ["ConvexHullConfig", "ConvexHullConstraint", "TerminalSetManager", "LocalSafeSet", "LocalSafeSetConfig",
           "MultiResolutionLocalSafeSet", "GPQFunction",
           "InverseDistanceQFunction", "IterativeQFunction", "LocalLinearQFunction", "QFunctionApproximator",
           "QFunctionConfig", "QFunctionManager", "FuelAwareSafeSet", "SampledSafeSet", "TrajectoryData"]
