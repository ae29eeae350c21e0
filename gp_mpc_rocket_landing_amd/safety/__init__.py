"""The safety layer of the control step (reference src/safety): the LQR / PD backup
controllers, the ellipsoidal invariant set and the predictive safety filter.  The filter's
rollouts and gradient loop run on the device (csrc/safety.hip), and so do the
uncertainty tubes of tube MPC (tube_mpc.py, csrc/tube.hip).  Not restated: the
CasADi / IPOPT path of the filter's QP."""
from .backup_controller import (BackupControllerConfig, EmergencyBrakingController, LQRBackupController,
                                PDBackupController, create_backup_controller)
from .invariant_sets import (EllipsoidalInvariantSet, InvariantSetConfig, PolytopeInvariantSet, TubeController,
                             compute_lmi_invariant_set)
from .safety_filter import (PredictiveSafetyFilter, SafetyFilterBatch, SafetyFilterConfig, SafetyFilterResult,
                            SafetySimulationBatch, SimpleSafetyFilter)
from .tube_mpc import RobustTubeMPC, TubeConstraintTightener, TubeMPCConfig, TubePropagator

__all__ = ["BackupControllerConfig", "EmergencyBrakingController", "LQRBackupController", "PDBackupController",
           "create_backup_controller", "EllipsoidalInvariantSet", "InvariantSetConfig", "PolytopeInvariantSet",
           "TubeController", "compute_lmi_invariant_set", "PredictiveSafetyFilter", "SafetyFilterBatch",
           "SafetyFilterConfig", "SafetyFilterResult", "SafetySimulationBatch", "SimpleSafetyFilter", "RobustTubeMPC",
           "TubeConstraintTightener", "TubeMPCConfig", "TubePropagator"]
