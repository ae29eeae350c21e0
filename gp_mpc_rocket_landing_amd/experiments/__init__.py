"""Monte-Carlo landing driver, baseline controllers and dispersion analysis (reference
src/experiments/monte_carlo.py, baselines.py, dispersion.py)."""
from .baselines import (BaselineComparison, LQRConfig, LQRController, LQRSolution, NominalMPCWrapper,
                        OpenLoopController, PIDConfig, PIDController, PIDSolution, TubeMPCWrapper,
                        create_baseline_controllers)
from .dispersion import (AeroDispersionConfig, DispersedDynamics, DispersionAnalysis, DispersionAnalysisResults,
                         DispersionConfig, InitialConditionDispersion, ThrustDispersionConfig, WindConfig, WindModel)
from .monte_carlo import (LandingConstraints, LandingOutcome, MonteCarloResults, MonteCarloSimulator,
                          SimulationConfig, SimulationResult, compare_controllers, mc_noise_table,
                          sample_initial_condition)

__all__ = ["LandingConstraints", "LandingOutcome", "MonteCarloResults", "MonteCarloSimulator",
           "SimulationConfig", "SimulationResult", "compare_controllers", "mc_noise_table",
           "sample_initial_condition",
           "BaselineComparison", "LQRConfig", "LQRController", "LQRSolution", "NominalMPCWrapper",
           "OpenLoopController", "PIDConfig", "PIDController", "PIDSolution", "TubeMPCWrapper",
           "create_baseline_controllers",
           "AeroDispersionConfig", "DispersedDynamics", "DispersionAnalysis", "DispersionAnalysisResults",
           "DispersionConfig", "InitialConditionDispersion", "ThrustDispersionConfig", "WindConfig", "WindModel"]
