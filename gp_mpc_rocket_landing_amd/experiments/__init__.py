"""Monte-Carlo landing driver (reference src/experiments/monte_carlo.py)."""
from .monte_carlo import (LandingConstraints, LandingOutcome, MonteCarloResults, MonteCarloSimulator,
                          SimulationConfig, SimulationResult, compare_controllers, mc_noise_table,
                          sample_initial_condition)

__all__ = ["LandingConstraints", "LandingOutcome", "MonteCarloResults", "MonteCarloSimulator",
           "SimulationConfig", "SimulationResult", "compare_controllers", "mc_noise_table",
           "sample_initial_condition"]
