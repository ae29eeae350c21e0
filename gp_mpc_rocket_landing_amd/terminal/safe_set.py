"""The sampled safe set of learning MPC: the states of every successful landing with their
cost-to-go (mirror of the reference's src/terminal/safe_set.py by name, signature, default
and return value; all of it runs on the host).

SS^j = SS^(j-1) united with the states of landing j; Q(x_k) = sum_{i >= k} l(x_i, u_i) along
the landing that visited x_k (Rosolia & Borrelli 2017).

One addition: ``SampledSafeSet.add_monte_carlo_results`` turns a fleet run
(experiments.monte_carlo.MonteCarloResults) into a safe set.
"""
from __future__ import annotations

import pickle
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np


@dataclass
class TrajectoryData:
    """One successful landing: states (T+1, n_x), controls (T, n_u), stage costs (T,),
    cost-to-go (T+1,), their total, and free-form metadata."""

    iteration: int
    states: np.ndarray
    controls: np.ndarray
    costs: np.ndarray
    cost_to_go: np.ndarray
    total_cost: float
    metadata: Dict[str, Any] = field(default_factory=dict)

    def __post_init__(self):
        steps = len(self.controls)
        assert len(self.states) == steps + 1, "States should have T+1 points"
        assert len(self.costs) == steps, "Costs should have T points"
        assert len(self.cost_to_go) == steps + 1, "Cost-to-go should have T+1 points"

    @property
    def T(self) -> int:
        return len(self.controls)

    @property
    def n_x(self) -> int:
        return self.states.shape[1]

    @property
    def n_u(self) -> int:
        return self.controls.shape[1]


def cost_to_go(stage_costs) -> np.ndarray:
    """Q_k = l_k + Q_(k+1) from Q_T = 0, accumulated backwards one addition a step (the
    reference's loop, safe_set.py:155-160: these are its bits)."""
    steps = len(stage_costs)
    q = np.zeros(steps + 1)
    for k in reversed(range(steps)):
        q[k] = stage_costs[k] + q[k + 1]
    return q


class SampledSafeSet:
    """States of successful landings with their cost-to-go; grows one landing at a time.

    The flat views (``get_all_states`` and friends) stack the landings in the order they were
    added, terminal states included (their Q is 0); the control of a terminal state is a row
    of zeros."""

    def __init__(self, n_x: int, n_u: int, target_state: Optional[np.ndarray] = None, fuel_index: int = 0):
        self.n_x = n_x
        self.n_u = n_u
        self.target_state = target_state
        self.fuel_index = fuel_index
        self._trajectories: List[TrajectoryData] = []
        self._iteration_count = 0
        self._all_states: Optional[np.ndarray] = None
        self._all_q_values: Optional[np.ndarray] = None
        self._all_controls: Optional[np.ndarray] = None
        self._state_iterations: Optional[np.ndarray] = None
        self._cache_valid = False

    def add_trajectory(self, states, controls, stage_costs, iteration: Optional[int] = None,
                       metadata: Optional[Dict] = None) -> None:
        """Add a landing: states (T+1, n_x), controls (T, n_u), stage_costs (T,).  Without
        ``iteration`` it takes the next one."""
        if iteration is None:
            iteration = self._iteration_count
        q = cost_to_go(stage_costs)
        self._trajectories.append(TrajectoryData(iteration=iteration, states=states.copy(), controls=controls.copy(),
                                                 costs=stage_costs.copy(), cost_to_go=q, total_cost=q[0],
                                                 metadata=metadata or {}))
        self._iteration_count = max(self._iteration_count, iteration + 1)
        self._cache_valid = False

    def add_monte_carlo_results(self, results, stage_cost: Callable[[np.ndarray, np.ndarray], float]) -> int:
        """Add every successful landing of a ``MonteCarloResults`` (its ``results``: states
        (T+1, n_x), controls (T, n_u), ``success``) with the stage cost ``stage_cost(x_k, u_k)``
        of each step; failed landings and landings without a step are skipped.  Every landing
        takes the next iteration number.  Returns how many were added."""
        added = 0
        for r in getattr(results, "results", results):
            if not r.success or len(r.controls) == 0:
                continue
            costs = np.array([float(stage_cost(x, u)) for x, u in zip(r.states[:-1], r.controls)])
            self.add_trajectory(np.asarray(r.states, float), np.asarray(r.controls, float), costs,
                                metadata={"run_id": getattr(r, "run_id", None)})
            added += 1
        return added

    def _rebuild_cache(self) -> None:
        if self._cache_valid:
            return
        if not self._trajectories:
            self._all_states = np.zeros((0, self.n_x))
            self._all_q_values = np.zeros(0)
            self._all_controls = np.zeros((0, self.n_u))
            self._state_iterations = np.zeros(0, dtype=int)
        else:
            ts = self._trajectories
            self._all_states = np.vstack([t.states for t in ts])
            self._all_q_values = np.concatenate([t.cost_to_go for t in ts])
            self._all_controls = np.vstack([np.vstack([t.controls, np.zeros((1, self.n_u))]) for t in ts])
            self._state_iterations = np.concatenate([np.full(len(t.states), t.iteration) for t in ts])
        self._cache_valid = True

    def get_all_states(self) -> np.ndarray:
        self._rebuild_cache()
        return self._all_states

    def get_all_q_values(self) -> np.ndarray:
        self._rebuild_cache()
        return self._all_q_values

    def get_all_controls(self) -> np.ndarray:
        self._rebuild_cache()
        return self._all_controls

    def get_states_with_min_fuel(self, min_fuel: float) -> Tuple[np.ndarray, np.ndarray]:
        """States whose fuel / mass entry is at least ``min_fuel``, and their Q."""
        self._rebuild_cache()
        keep = self._all_states[:, self.fuel_index] >= min_fuel
        return self._all_states[keep], self._all_q_values[keep]

    def get_states_from_iteration(self, iteration: int) -> Tuple[np.ndarray, np.ndarray]:
        self._rebuild_cache()
        keep = self._state_iterations == iteration
        return self._all_states[keep], self._all_q_values[keep]

    def get_best_trajectory(self) -> Optional[TrajectoryData]:
        if not self._trajectories:
            return None
        return self._trajectories[int(np.argmin([t.total_cost for t in self._trajectories]))]

    def get_trajectory(self, iteration: int) -> Optional[TrajectoryData]:
        for t in self._trajectories:
            if t.iteration == iteration:
                return t
        return None

    @property
    def num_trajectories(self) -> int:
        return len(self._trajectories)

    @property
    def num_states(self) -> int:
        self._rebuild_cache()
        return len(self._all_states)

    @property
    def num_iterations(self) -> int:
        return self._iteration_count

    def get_statistics(self) -> Dict[str, Any]:
        self._rebuild_cache()
        if not self._trajectories:
            return {"num_trajectories": 0, "num_states": 0, "num_iterations": 0}
        costs = [t.total_cost for t in self._trajectories]
        return {
            "num_trajectories": len(self._trajectories),
            "num_states": len(self._all_states),
            "num_iterations": self._iteration_count,
            "best_cost": min(costs),
            "worst_cost": max(costs),
            "mean_cost": np.mean(costs),
            "cost_improvement": costs[0] - min(costs) if len(costs) > 1 else 0,
        }

    def save(self, filepath: str) -> None:
        """Pickle the landings and the set's parameters."""
        with open(filepath, "wb") as f:
            pickle.dump({"n_x": self.n_x, "n_u": self.n_u, "target_state": self.target_state,
                         "fuel_index": self.fuel_index, "trajectories": self._trajectories,
                         "iteration_count": self._iteration_count}, f)

    @classmethod
    def load(cls, filepath: str) -> "SampledSafeSet":
        with open(filepath, "rb") as f:
            data = pickle.load(f)
        ss = cls(n_x=data["n_x"], n_u=data["n_u"], target_state=data["target_state"], fuel_index=data["fuel_index"])
        ss._trajectories = data["trajectories"]
        ss._iteration_count = data["iteration_count"]
        return ss

    def clear(self) -> None:
        self._trajectories = []
        self._iteration_count = 0
        self._cache_valid = False


class FuelAwareSafeSet(SampledSafeSet):
    """A safe set that also knows the fuel each state needed to reach the end of its landing
    (its mass minus the landing's last mass, plus ``fuel_margin``): a state is offered only to
    a query that has that much."""

    def __init__(self, n_x: int, n_u: int, target_state: Optional[np.ndarray] = None, fuel_index: int = 0,
                 fuel_margin: float = 0.1):
        super().__init__(n_x, n_u, target_state, fuel_index)
        self.fuel_margin = fuel_margin
        self._fuel_required: Optional[np.ndarray] = None

    def add_trajectory(self, states, controls, stage_costs, iteration: Optional[int] = None,
                       metadata: Optional[Dict] = None) -> None:
        super().add_trajectory(states, controls, stage_costs, iteration, metadata)
        self._fuel_required = None

    def clear(self) -> None:
        super().clear()
        self._fuel_required = None

    def _compute_fuel_required(self) -> None:
        if self._fuel_required is not None:
            return
        self._rebuild_cache()
        if len(self._all_states) == 0:
            self._fuel_required = np.zeros(0)
            return
        fi = self.fuel_index
        self._fuel_required = np.concatenate([t.states[:, fi] - t.states[-1, fi] + self.fuel_margin
                                              for t in self._trajectories])

    def get_feasible_states(self, available_fuel: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> (states, q_values, indices into the full set) of the states whose required fuel
        is at most ``available_fuel``."""
        self._rebuild_cache()
        self._compute_fuel_required()
        keep = self._fuel_required <= available_fuel
        return self._all_states[keep], self._all_q_values[keep], np.where(keep)[0]

    def get_fuel_required(self) -> np.ndarray:
        self._compute_fuel_required()
        return self._fuel_required
