"""ctypes binding of libgpmpc_hip.so (include/gpmpc.h).

The product path has no CPU fallback: importing this module without the built
HIP library raises, and every call goes through the C-ABI.  Build with
``python -c "import __graft_entry__ as g; g.build()"`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPMPC_LIB") or os.path.join(_HERE, "libgpmpc_hip.so")  # GPMPC_LIB: A/B builds

SE_ARD, SE_ISO, MATERN32, MATERN52 = 0, 1, 2, 3
ERR_NOT_PD = -100
REC_LEN = 16
COMM_ID_BYTES = 128   # GPMPC_COMM_ID_BYTES (sizeof ncclUniqueId)
# caps of the generic device QP (csrc/qp.h QP_NMAX, QP_MMAX, QP_NNZMAX)
QP_NMAX, QP_MMAX, QP_NNZMAX = 216, 360, 896
# ... and of its KKT factor: half-bandwidth, entries per row / column of A (QP_W, QP_RMAX, QP_CMAX)
QP_WMAX, QP_ROWMAX, QP_COLMAX = 16, 8, 12
# gpmpc_qp_pattern_info's answer, in order (include/gpmpc.h)
QP_PATTERN_INFO = ("mode", "w", "nblk", "fac_len", "maxrow", "maxcol", "n_offd", "fits", "is_fleet_pattern")

QP_STATUS = {1: "solved", 2: "solved inaccurate", -2: "maximum iterations reached",
             -3: "primal infeasible", 3: "primal infeasible inaccurate", -4: "dual infeasible",
             4: "dual infeasible inaccurate", -7: "problem non convex", -10: "unsolved"}

if not os.path.exists(LIB_PATH):
    raise ImportError(f"HIP library missing: {LIB_PATH} (build it with __graft_entry__.build(); "
                      "there is no CPU fallback)")


def _share_torch_hip_runtime():
    """Make this process use ONE HIP runtime.  torch bundles its own
    libamdhip64 (SONAME libamdhip64.so.7, loaded by the unversioned name from
    torch/lib).  If our library pulled /opt/rocm's copy in first, torch would
    later load a second runtime, and whichever initialises second sees no
    device.  Preloading torch's copy globally lets our NEEDED libamdhip64.so.7
    resolve to it (GPMPC_HIP_RUNTIME=system keeps /opt/rocm's instead)."""
    if os.environ.get("GPMPC_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    tlib = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        p = os.path.join(tlib, name)
        if os.path.exists(p):
            ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)


_share_torch_hip_runtime()
_L = ctypes.CDLL(LIB_PATH)
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p


class QPSettings(ctypes.Structure):
    _fields_ = [("rho", ctypes.c_double), ("sigma", ctypes.c_double), ("alpha", ctypes.c_double),
                ("eps_abs", ctypes.c_double), ("eps_rel", ctypes.c_double),
                ("eps_prim_inf", ctypes.c_double), ("eps_dual_inf", ctypes.c_double),
                ("max_iter", ctypes.c_int), ("check_termination", ctypes.c_int),
                ("adaptive_rho", ctypes.c_int), ("adaptive_rho_interval", ctypes.c_int),
                ("adaptive_rho_tolerance", ctypes.c_double), ("scaling", ctypes.c_int),
                ("warm_start", ctypes.c_int)]


class Rollout6Config(ctypes.Structure):
    _fields_ = [("horizon", ctypes.c_int), ("dt", ctypes.c_double), ("max_steps", ctypes.c_int),
                ("qp", QPSettings), ("fitc_mean_as_written", ctypes.c_int),
                ("q_diag", ctypes.c_double * 14), ("p_diag", ctypes.c_double * 14),
                ("r_diag", ctypes.c_double * 3), ("t_min", ctypes.c_double), ("t_max", ctypes.c_double),
                ("tan_gamma_gs", ctypes.c_double), ("trust_x2", ctypes.c_double),
                ("trust_u2", ctypes.c_double), ("use_gp_mean", ctypes.c_int), ("upright_target", ctypes.c_int),
                ("rocket_j", ctypes.c_double * 3), ("rocket_r_t", ctypes.c_double * 3),
                ("rocket_g_i", ctypes.c_double * 3), ("rocket_alpha", ctypes.c_double),
                ("rocket_g0", ctypes.c_double), ("rocket_J", ctypes.c_double * 9)]


class FleetConfig(ctypes.Structure):
    _fields_ = [("horizon", ctypes.c_int), ("dt", ctypes.c_double), ("target_mode", ctypes.c_int),
                ("use_gp", ctypes.c_int), ("residual_model", ctypes.c_int),
                ("max_steps", ctypes.c_int), ("qp", QPSettings),
                ("sqp_iters", ctypes.c_int), ("sqp_tol", ctypes.c_double), ("sqp_qp", QPSettings)]


class FleetMCConfig(ctypes.Structure):
    """gpmpc_fleet_mc_config: the Monte-Carlo protocol attachment of a fleet."""
    _fields_ = [("thrust_dispersion", ctypes.c_double), ("aero_dispersion", ctypes.c_double),
                ("log_steps", ctypes.c_int)]


class SafetyConfig(ctypes.Structure):
    """gpmpc_safety_config: the predictive safety filter's backup law, ellipsoid and loop."""
    _fields_ = [("horizon", ctypes.c_int), ("dt", ctypes.c_double), ("K", ctypes.c_double * 42),
                ("P", ctypes.c_double * 196), ("x_eq", ctypes.c_double * 14), ("u_eq", ctypes.c_double * 3),
                ("u_min", ctypes.c_double * 3), ("u_max", ctypes.c_double * 3), ("alpha", ctypes.c_double),
                ("backup_margin", ctypes.c_double), ("have_constraints", ctypes.c_int), ("T_min", ctypes.c_double),
                ("T_max", ctypes.c_double), ("cos_theta_max", ctypes.c_double), ("tan2_gamma", ctypes.c_double),
                ("n_iters", ctypes.c_int), ("lr", ctypes.c_double), ("fd_eps", ctypes.c_double)]


class BaselineConfig(ctypes.Structure):
    """gpmpc_baseline_config: controller kind, batch, the plant's scalars, clips, PID gains and
    the dispersed plant's switches."""
    _fields_ = [("kind", ctypes.c_int), ("batch", ctypes.c_int), ("max_steps", ctypes.c_int), ("dt", ctypes.c_double),
                ("alpha", ctypes.c_double), ("g", ctypes.c_double * 3), ("T_lo", ctypes.c_double),
                ("T_hi", ctypes.c_double), ("gimbal_max", ctypes.c_double), ("Kp_z", ctypes.c_double),
                ("Ki_z", ctypes.c_double), ("Kd_z", ctypes.c_double), ("Kp_xy", ctypes.c_double),
                ("Ki_xy", ctypes.c_double), ("Kd_xy", ctypes.c_double), ("max_integral", ctypes.c_double),
                ("thrust_min", ctypes.c_double), ("thrust_max", ctypes.c_double), ("pid_dt", ctypes.c_double),
                ("pid_g", ctypes.c_double), ("n_ref", ctypes.c_int), ("thrust_rows", ctypes.c_int),
                ("wind_kind", ctypes.c_int), ("wind_rows", ctypes.c_int), ("drag", ctypes.c_int),
                ("sim_thrust", ctypes.c_double), ("sim_aero", ctypes.c_double), ("log", ctypes.c_int)]


def _sig(name, res, *args):
    f = getattr(_L, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_c = ctypes.c_int
_sig("gpmpc_abi_version", _c)
ABI_VERSION = 4   # include/gpmpc.h GPMPC_ABI_VERSION this binding's structures follow
if _L.gpmpc_abi_version() != ABI_VERSION:
    raise ImportError(f"{LIB_PATH} has C-ABI {_L.gpmpc_abi_version()}, this binding needs {ABI_VERSION}: "
                      "rebuild it (__graft_entry__.build())")
_sig("gpmpc_last_error", ctypes.c_char_p)
_sig("gpmpc_ctx_create", _c, _c, ctypes.POINTER(_vp))
_sig("gpmpc_ctx_destroy", _c, _vp)
_sig("gpmpc_ctx_sync", _c, _vp)
_sig("gpmpc_ctx_stream", _vp, _vp)
_sig("gpmpc_gram", _c, _vp, _c, _dp, _c, _dp, _c, _c, _dp, ctypes.c_double, _dp, _c)
_sig("gpmpc_potrf", _c, _vp, _c, _dp, _c, _ip)
_sig("gpmpc_potrf_batched_dev", _c, _vp, _c, _c, _vp, _c, ctypes.c_int64, _vp)
_sig("gpmpc_trsm_lower", _c, _vp, _c, _c, _dp, _c, _dp, _c)
_sig("gpmpc_potrs", _c, _vp, _c, _c, _dp, _c, _dp, _c)
_sig("gpmpc_gp_fit_exact", _c, _vp, _c, _dp, _c, _c, _dp, _c, _dp, ctypes.c_double,
     ctypes.c_double, ctypes.POINTER(_vp), _dp, _dp, _dp, _ip)
_sig("gpmpc_gp_fit_exact_prog", _c, _vp, _ip, _c, _dp, _c, _dp, _c, _c, _dp, _c, ctypes.c_double,
     ctypes.POINTER(_vp), _dp, _dp, _dp, _ip)
_sig("gpmpc_sparse_fit_prog", _c, _vp, _c, _ip, _c, _dp, _c, _dp, _c, _dp, _c, _c, _dp, _c, ctypes.c_double,
     ctypes.c_double, ctypes.POINTER(_vp), _dp, _dp, _dp, _dp)
_sig("gpmpc_gp_predict", _c, _vp, _vp, _dp, _c, _dp, _dp)
_sig("gpmpc_gp_predict_cov", _c, _vp, _vp, _dp, _c, _dp, _dp)
_sig("gpmpc_gp_get_state", _c, _vp, _vp, _dp, _dp)
_sig("gpmpc_gp_destroy", _c, _vp)
_sig("gpmpc_gp_append", _c, _vp, _vp, _dp, _c, _dp, _dp, _dp, _dp)
_sig("gpmpc_gp_lml_batched", _c, _vp, _c, _dp, _c, _c, _dp, _c, _dp, _dp, _dp, _dp, _ip)
_sig("gpmpc_fitc_fit", _c, _vp, _dp, _c, _dp, _c, _c, _dp, _c, _dp, ctypes.c_double,
     ctypes.c_double, ctypes.c_double, ctypes.POINTER(_vp), _dp, _dp, _dp, _dp)
_sig("gpmpc_vfe_fit", _c, _vp, _dp, _c, _dp, _c, _c, _dp, _c, _dp, ctypes.c_double,
     ctypes.c_double, ctypes.c_double, ctypes.POINTER(_vp), _dp, _dp, _dp)
_sig("gpmpc_fitc_predict", _c, _vp, _vp, _dp, _c, _dp, _dp)
_sig("gpmpc_fitc_destroy", _c, _vp)
_sig("gpmpc_fitc_get_state", _c, _vp, _vp, _dp)
_sig("gpmpc_qp_default_settings", None, ctypes.POINTER(QPSettings))
_sig("gpmpc_qp_solve_batched", _c, _vp, _c, _c, _c, _c, _ip, _ip, _dp, _dp, _dp, _dp, _dp,
     ctypes.POINTER(QPSettings), _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp)
_sig("gpmpc_qp_pattern_info", _c, _c, _c, _ip, _ip, _ip)
_sig("gpmpc_fleet_default_config", None, ctypes.POINTER(FleetConfig))
_sig("gpmpc_fleet_create", _c, _vp, _vp, ctypes.POINTER(FleetConfig), _c, ctypes.POINTER(_vp))
_sig("gpmpc_fleet_create_shard", _c, _vp, _vp, ctypes.POINTER(FleetConfig), _c, _c, ctypes.POINTER(_vp))
_sig("gpmpc_fleet_create_fitc", _c, _vp, _vp, ctypes.POINTER(FleetConfig), _c, _c, ctypes.POINTER(_vp))
_sig("gpmpc_fleet_reset", _c, _vp, _c, _c, _dp)
_sig("gpmpc_fleet_step", _c, _vp, _c)
_sig("gpmpc_fleet_step_phases", _c, _vp, _c)
_sig("gpmpc_fleet_set_stamps", _c, _vp, _vp)
_sig("gpmpc_fleet_set_trace", _c, _vp, _vp)
_sig("gpmpc_syrk_batched_dev", _c, _vp, _c, _c, _c, _vp, _c, ctypes.c_int64, _vp, _c, ctypes.c_int64,
     ctypes.c_double, ctypes.c_double)
_sig("gpmpc_cov_propagate", _c, _vp, _c, _c, _c, _dp, _dp, _vp, ctypes.c_double, _dp)
_sig("gpmpc_cov_propagate_dev", _c, _vp, _c, _c, _c, _vp, _vp, _vp, ctypes.c_double, _vp)
_sig("gpmpc_uprop3_linear", _c, _vp, _vp, _c, _c, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _vp,
     ctypes.c_double, _dp, _dp)
_sig("gpmpc_uprop6_linear", _c, _vp, _vp, _vp, _c, _dp, _c, _c, ctypes.c_double, _dp, _dp, _vp,
     ctypes.c_double, _dp, _dp)
_sig("gpmpc_uprop3_unscented", _c, _vp, _vp, _c, _c, _c, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _dp,
     _vp, ctypes.c_double, _dp, _dp, _ip)
_sig("gpmpc_uprop6_unscented", _c, _vp, _vp, _vp, _c, _dp, _dp, _c, _c, ctypes.c_double, _dp, _dp, _vp,
     ctypes.c_double, _dp, _dp, _ip)
_sig("gpmpc_uprop3_mc", _c, _vp, _vp, _c, _c, _c, _c, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _vp,
     ctypes.c_double, _dp, _dp, _dp, _dp, _vp)
_sig("gpmpc_uprop6_mc", _c, _vp, _vp, _vp, _c, _dp, _c, _c, _c, ctypes.c_double, _dp, _dp, _vp,
     ctypes.c_double, _dp, _dp, _dp, _dp, _vp)
_sig("gpmpc_fleet_read", _c, _vp, _dp, _dp)
_sig("gpmpc_gram_grad", _c, _vp, _c, _dp, _c, _dp, _c, _c, _dp, ctypes.c_double, _dp, _dp)
_sig("gpmpc_fleet_get_state", _c, _vp, _dp, _dp, _dp, _dp)
_sig("gpmpc_fleet_get_posterior", _c, _vp, _dp, _dp)
_sig("gpmpc_fleet_records_dev", _vp, _vp)
_sig("gpmpc_fleet_query_launches", _c, _vp)
_sig("gpmpc_fleet_destroy", _c, _vp)
_i64 = ctypes.c_int64
_sig("gpmpc_gemm_diag", _c, _vp, _c, _c, _c, _c, _c, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64,
     ctypes.c_double, ctypes.c_double, _c, _c, _c, _ip)
_sig("gpmpc_gemm_row_tiles", _c, _c, _c, _c, _ip)
_sig("gpmpc_potrf_plan", _c, _c, _c, _ip, _ip, _ip, _c)
_sig("gpmpc_potrf_diag", _c, _vp, _c, _c, _vp, _c, _i64, _vp, _ip)
_sig("gpmpc_tri_diag", _c, _vp, _c, _c, _c, _vp, _i64, _vp, _i64, _vp, _c)
_sig("gpmpc_gemm_plan", _c, _c, _c, _c, _c, _c, ctypes.c_double, _c, _c, _c, _ip, _ip)
_sig("gpmpc_gram_path", _c, _c, _c, _c)
_sig("gpmpc_fleet_mc_attach", _c, _vp, ctypes.POINTER(FleetMCConfig), _dp)
_sig("gpmpc_fleet_mc_read_log", _c, _vp, _c, _c, _dp, _dp, _ip)
_sig("gpmpc_fleet_mc_detach", _c, _vp)
_sig("gpmpc_nn_dist", _c, _vp, _dp, _c, _dp, _c, _c, _dp)
_sig("gpmpc_select_diverse", _c, _vp, _dp, _c, _c, _dp, _c, ctypes.c_double, _c, _ip, _dp)
_sig("gpmpc_kmeans_lloyd", _c, _vp, _dp, _c, _c, _dp, _c, _c, _dp, _ip, _ip, _dp, _ip)
_sig("gpmpc_kmeans_tau", ctypes.c_double, _c)
_sig("gpmpc_knn_create", _c, _vp, _dp, _c, _c, _dp, _dp, ctypes.POINTER(_vp))
_sig("gpmpc_knn_destroy", _c, _vp)
_sig("gpmpc_knn_query", _c, _vp, _c, _dp, _c, _c, ctypes.c_double, _dp, _ip, _dp, _ip, _ip)
_sig("gpmpc_knn_interp", _c, _vp, _c, _dp, _c, _c, _c, _c, _c, ctypes.c_double, _dp, _dp, _ip)
_sig("gpmpc_knn_plan", _c, _c, _c, _c, _c, _ip, _ip)
_sig("gpmpc_hull_project", _c, _vp, _dp, _dp, _ip, _c, _dp, _c, _c, _c, ctypes.c_double, _c, _dp, _dp, _dp, _dp, _dp,
     _ip, _ip)
_sig("gpmpc_knn_set_points", _c, _vp, _dp, _c)
_sig("gpmpc_knn_hull", _c, _vp, _c, _dp, _dp, _c, _c, _c, _c, _c, ctypes.c_double, _dp, ctypes.c_double, _c, _ip, _ip,
     _dp, _dp, _dp, _dp, _dp, _ip, _ip)
_sig("gpmpc_hull_plan", _c, _c, _c, _c, _ip)
_sig("gpmpc_safety_default_config", None, ctypes.POINTER(SafetyConfig))
_sig("gpmpc_safety_filter", _c, _vp, _dp, ctypes.POINTER(SafetyConfig), _c, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip)
_sig("gpmpc_safety_simulate", _c, _vp, _dp, ctypes.POINTER(SafetyConfig), _c, _c, _dp, _dp, _dp, _dp, _dp, _ip, _ip)
_sig("gpmpc_tube_linear", _c, _vp, _dp, _c, _c, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _c, ctypes.c_double, _dp,
     _dp, _dp, _dp)
_sig("gpmpc_tube_mc", _c, _vp, _dp, _c, _c, _c, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _dp)
_sig("gpmpc_tube_plan", _c, _c, _c, _ip, _ip)
_sig("gpmpc_baseline_default_config", None, ctypes.POINTER(BaselineConfig))
_sig("gpmpc_baseline_fly", _c, _vp, ctypes.POINTER(BaselineConfig), _dp, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _dp, _ip,
     _dp, _dp)
_sig("gpmpc_rollout6_default_config", None, ctypes.POINTER(Rollout6Config))
_sig("gpmpc_rollout6_create", _c, _vp, _vp, _vp, ctypes.POINTER(Rollout6Config), _c, ctypes.POINTER(_vp))
_sig("gpmpc_rollout6_create_exact", _c, _vp, _vp, _vp, ctypes.POINTER(Rollout6Config), _c, ctypes.POINTER(_vp))
_sig("gpmpc_rollout6_solve", _c, _vp, _dp, _dp, _c, _c, ctypes.c_double, _dp, _dp, _ip, _ip, _ip, _ip)
_sig("gpmpc_rollout6_solve_ref", _c, _vp, _dp, _dp, _dp, _dp, _c, _c, ctypes.c_double, _dp, _dp, _ip, _ip, _ip,
     _ip)
_sig("gpmpc_rollout6_set_state", _c, _vp, _dp, _dp, _dp)
_sig("gpmpc_rollout6_records_dev", _vp, _vp)
_sig("gpmpc_comm_unique_id", _c, ctypes.c_char_p)
_sig("gpmpc_comm_init", _c, _vp, ctypes.c_char_p, _c, _c, ctypes.POINTER(_vp))
_sig("gpmpc_comm_destroy", _c, _vp)
_sig("gpmpc_comm_count", _c, _vp, _ip)
_sig("gpmpc_gather_results", _c, _vp, _vp, _vp, _ip, _c, _dp)
_sig("gpmpc_gather_prepare", _c, _vp, _vp, _vp, _ip, _c)
_sig("gpmpc_gather_collective", _c, _vp, _vp, _ip, _c, _dp)
_sig("gpmpc_rollout6_reset", _c, _vp, _c, _c, _dp)
_sig("gpmpc_rollout6_step", _c, _vp, _c)
_sig("gpmpc_rollout6_step_phases", _c, _vp, _c)
_sig("gpmpc_rollout6_read", _c, _vp, _dp, _dp)
_sig("gpmpc_rollout6_get_state", _c, _vp, _dp, _dp, _dp, _dp, _dp, _dp)
_sig("gpmpc_rollout6_destroy", _c, _vp)

EXPORTED = ["gpmpc_abi_version", "gpmpc_last_error", "gpmpc_ctx_create", "gpmpc_ctx_destroy",
            "gpmpc_ctx_sync", "gpmpc_ctx_stream", "gpmpc_gram", "gpmpc_gram_grad", "gpmpc_potrf",
            "gpmpc_potrf_batched_dev", "gpmpc_trsm_lower", "gpmpc_potrs", "gpmpc_gp_fit_exact",
            "gpmpc_gp_predict", "gpmpc_gp_predict_cov", "gpmpc_gp_fit_exact_prog", "gpmpc_sparse_fit_prog", "gpmpc_gp_get_state", "gpmpc_gp_destroy",
            "gpmpc_gp_lml_batched", "gpmpc_gp_append",
            "gpmpc_fitc_fit", "gpmpc_fitc_predict", "gpmpc_fitc_destroy",
            "gpmpc_qp_default_settings", "gpmpc_qp_solve_batched", "gpmpc_fleet_default_config",
            "gpmpc_fleet_create", "gpmpc_fleet_create_shard", "gpmpc_fleet_create_fitc", "gpmpc_fleet_reset", "gpmpc_fleet_step", "gpmpc_fleet_read",
            "gpmpc_fleet_step_phases", "gpmpc_fleet_get_state", "gpmpc_fleet_get_posterior", "gpmpc_fleet_set_stamps", "gpmpc_fleet_set_trace",
            "gpmpc_syrk_batched_dev", "gpmpc_cov_propagate", "gpmpc_cov_propagate_dev", "gpmpc_uprop3_linear", "gpmpc_uprop6_linear",
            "gpmpc_fleet_records_dev", "gpmpc_fleet_destroy", "gpmpc_rollout6_default_config",
            "gpmpc_rollout6_create", "gpmpc_rollout6_reset", "gpmpc_rollout6_step", "gpmpc_rollout6_read",
            "gpmpc_rollout6_get_state", "gpmpc_rollout6_destroy", "gpmpc_rollout6_create_exact",
            "gpmpc_rollout6_solve", "gpmpc_rollout6_solve_ref", "gpmpc_rollout6_set_state", "gpmpc_fitc_get_state",
            "gpmpc_rollout6_records_dev", "gpmpc_comm_unique_id", "gpmpc_comm_init", "gpmpc_comm_destroy",
            "gpmpc_comm_count", "gpmpc_gather_results", "gpmpc_gather_prepare", "gpmpc_gather_collective", "gpmpc_rollout6_step_phases", "gpmpc_vfe_fit",
            "gpmpc_fleet_mc_attach", "gpmpc_fleet_mc_read_log", "gpmpc_fleet_mc_detach",
            "gpmpc_fleet_query_launches", "gpmpc_gemm_diag", "gpmpc_nn_dist", "gpmpc_select_diverse",
            "gpmpc_gemm_row_tiles", "gpmpc_potrf_plan", "gpmpc_gram_path", "gpmpc_gemm_plan", "gpmpc_potrf_diag",
            "gpmpc_tri_diag", "gpmpc_uprop3_unscented", "gpmpc_uprop6_unscented", "gpmpc_kmeans_lloyd",
            "gpmpc_kmeans_tau", "gpmpc_qp_pattern_info", "gpmpc_uprop3_mc", "gpmpc_uprop6_mc", "gpmpc_knn_create",
            "gpmpc_knn_destroy", "gpmpc_knn_query", "gpmpc_knn_interp", "gpmpc_knn_plan",
            "gpmpc_hull_project", "gpmpc_knn_set_points", "gpmpc_knn_hull", "gpmpc_hull_plan",
            "gpmpc_safety_default_config", "gpmpc_safety_filter", "gpmpc_safety_simulate",
            "gpmpc_tube_linear", "gpmpc_tube_mc", "gpmpc_tube_plan",
            "gpmpc_baseline_default_config", "gpmpc_baseline_fly"]


class HIPError(RuntimeError):
    """A C-ABI call returned non-zero; ``rc`` is its return code (-2: the arguments
    were refused, e.g. a malformed composite-kernel program)."""

    def __init__(self, msg, rc=None):
        super().__init__(msg)
        self.rc = rc


def _err(rc, what):
    msg = _L.gpmpc_last_error().decode(errors="replace")
    raise HIPError(f"{what} failed ({rc}): {msg}", rc)


def _chk(rc, what):
    if rc != 0:
        _err(rc, what)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def abi_version():
    return _L.gpmpc_abi_version()


class Context:
    """One HIP device + stream (gpmpc_ctx)."""

    def __init__(self, device=0):
        h = _vp()
        _chk(_L.gpmpc_ctx_create(int(device), ctypes.byref(h)), "gpmpc_ctx_create")
        self.h = h
        self.device = device

    @property
    def stream(self):
        return _L.gpmpc_ctx_stream(self.h)

    def sync(self):
        _chk(_L.gpmpc_ctx_sync(self.h), "gpmpc_ctx_sync")

    def close(self):
        if self.h:
            _L.gpmpc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("GPMPC_DEVICE", "0")))
    return _default_ctx


# ---- thin wrappers -----------------------------------------------------------
def gram(ctx, kind, X1, X2, ls, sigma2):
    X1 = f64(np.atleast_2d(X1)); n1, d = X1.shape
    ls = f64(np.atleast_1d(ls))
    if ls.size == 1 and kind != SE_ISO:
        ls = np.full(d, float(ls[0]))
    if X2 is None:
        K = np.empty((n1, n1))
        _chk(_L.gpmpc_gram(ctx.h, kind, _d(X1), n1, None, n1, d, _d(ls), float(sigma2), _d(K), n1), "gram")
        return K
    X2 = f64(np.atleast_2d(X2)); n2 = X2.shape[0]
    K = np.empty((n1, n2))
    _chk(_L.gpmpc_gram(ctx.h, kind, _d(X1), n1, _d(X2), n2, d, _d(ls), float(sigma2), _d(K), n2), "gram")
    return K


def gram_grad(ctx, kind, X1, X2, ls, sigma2):
    """(K, G): the Gram and its log-hyperparameter gradients (gpmpc_gram_grad):
    G (d, n1, n2) for SE_ARD, (1, n1, n2) for SE_ISO."""
    X1 = f64(np.atleast_2d(X1)); n1, d = X1.shape
    ls = f64(np.atleast_1d(ls))
    if ls.size == 1 and kind != SE_ISO:
        ls = np.full(d, float(ls[0]))
    X2a = None if X2 is None else f64(np.atleast_2d(X2))
    n2 = n1 if X2a is None else X2a.shape[0]
    K = np.empty((n1, n2)); G = np.empty((1 if kind == SE_ISO else d, n1, n2))
    _chk(_L.gpmpc_gram_grad(ctx.h, kind, _d(X1), n1, None if X2a is None else _d(X2a), n2, d, _d(ls),
                            float(sigma2), _d(K), _d(G)), "gram_grad")
    return K, G


def potrf(ctx, A):
    """Lower Cholesky of A (returns L with a zero upper triangle) and LAPACK info."""
    A = f64(A).copy(); n = A.shape[0]
    info = np.zeros(1, np.int32)
    rc = _L.gpmpc_potrf(ctx.h, n, _d(A), n, _i(info))
    if rc < 0:
        _err(rc, "potrf")
    return np.tril(A), int(info[0])


def trsm_lower(ctx, L, B):
    L = f64(L); B = f64(B).copy()
    vec = B.ndim == 1
    if vec:
        B = B[:, None].copy()
    _chk(_L.gpmpc_trsm_lower(ctx.h, L.shape[0], B.shape[1], _d(L), L.shape[0], _d(B), B.shape[1]), "trsm")
    return B[:, 0] if vec else B


def potrs(ctx, L, B):
    L = f64(L); B = f64(B).copy()
    vec = B.ndim == 1
    if vec:
        B = B[:, None].copy()
    _chk(_L.gpmpc_potrs(ctx.h, L.shape[0], B.shape[1], _d(L), L.shape[0], _d(B), B.shape[1]), "potrs")
    return B[:, 0] if vec else B


def gp_lml_batched(ctx, kind, X, y, ls, sigma2, noise):
    """Log marginal likelihood of the exact GP at B parameter sets (rows of ls
    (B x d; SE_ISO: B x 1), sigma2 (B,), noise (B,)): returns (lml (B,),
    jitter_steps (B,)); -inf / -1 where the jitter ladder is exhausted."""
    X = f64(np.atleast_2d(X)); n, d = X.shape
    y = f64(np.asarray(y).reshape(-1))
    assert y.size == n, "X and y must have same number of samples"
    sigma2 = f64(np.atleast_1d(sigma2)); B = sigma2.size
    noise = f64(np.broadcast_to(np.atleast_1d(noise), (B,)))
    ls = np.atleast_2d(np.asarray(ls, dtype=np.float64))
    L = np.empty((B, d))
    L[:] = ls[:, :1] if ls.shape[1] == 1 else ls
    L = f64(L)
    lml = np.empty(B); steps = np.empty(B, np.int32)
    _chk(_L.gpmpc_gp_lml_batched(ctx.h, kind, _d(X), n, d, _d(y), B, _d(L), _d(sigma2), _d(noise),
                                 _d(lml), _i(steps)), "gp_lml_batched")
    return lml, steps


KP_WHITE, KP_SUM, KP_PROD = 4, 10, 11   # gpmpc.h GPMPC_KP_*


class KernelProgram:
    """A composite kernel (SumKernel / ProductKernel / WhiteNoise over the stationary
    kernels, kernels.py:676-844) as the device's postfix program: ``ops`` (code,
    parameter offset) pairs and ``par`` (gpmpc.h GPMPC_KP_*).  Passed as ``kind`` to
    ExactGPHandle / FITCHandle, which then ignore ``ls`` / ``sigma2``."""

    def __init__(self, ops, par):
        self.ops = np.ascontiguousarray(np.asarray(ops, np.int32).reshape(-1, 2))
        self.par = f64(np.asarray(par, float).reshape(-1))

    def __eq__(self, other):
        return (isinstance(other, KernelProgram) and np.array_equal(self.ops, other.ops)
                and np.array_equal(self.par, other.par))

    def __repr__(self):
        return f"KernelProgram(ops={self.ops.tolist()}, par={self.par.tolist()})"


class ExactGPHandle:
    """Device-resident exact GP (shared factor across outputs).  ``kind``: one of the
    four kernel kinds, or a KernelProgram (a composite kernel)."""

    def __init__(self, ctx, kind, X, Y, ls, sigma2, noise):
        X = f64(np.atleast_2d(X)); Y = f64(Y)
        if Y.ndim == 1:
            Y = Y[:, None]
        n, d = X.shape; no = Y.shape[1]
        self.ctx = ctx; self.n = n; self.d = d; self.n_out = no
        self.y_mean = np.empty(no); self.y_std = np.empty(no); self.lml = np.empty(no)
        js = np.zeros(1, np.int32)
        h = _vp()
        if isinstance(kind, KernelProgram):
            rc = _L.gpmpc_gp_fit_exact_prog(ctx.h, _i(kind.ops), kind.ops.shape[0], _d(kind.par), kind.par.size,
                                            _d(X), n, d, _d(Y), no, float(noise), ctypes.byref(h),
                                            _d(self.y_mean), _d(self.y_std), _d(self.lml), _i(js))
        else:
            ls = f64(np.atleast_1d(ls))
            if ls.size == 1 and kind != SE_ISO:
                ls = np.full(d, float(ls[0]))
            rc = _L.gpmpc_gp_fit_exact(ctx.h, kind, _d(X), n, d, _d(Y), no, _d(ls), float(sigma2),
                                       float(noise), ctypes.byref(h), _d(self.y_mean), _d(self.y_std),
                                       _d(self.lml), _i(js))
        if rc == ERR_NOT_PD:
            raise ValueError("Kernel matrix is not positive definite even with jitter")
        _chk(rc, "gp_fit_exact")
        self.h = h
        self.jitter_steps = int(js[0])

    def append(self, Xnew, Yall):
        """Grow the GP by the rows Xnew (k x d) in O(n^2 k) (gpmpc_gp_append);
        Yall = the targets of all n + k rows.  False (handle unchanged) when the
        caller must refit instead (jitter-fitted GP / indefinite Schur complement)."""
        Xnew = f64(np.atleast_2d(Xnew)); k = Xnew.shape[0]
        Yall = f64(Yall)
        if Yall.ndim == 1:
            Yall = Yall[:, None]
        assert Xnew.shape[1] == self.d and Yall.shape == (self.n + k, self.n_out)
        ym = np.empty(self.n_out); ys = np.empty(self.n_out); lml = np.empty(self.n_out)
        rc = _L.gpmpc_gp_append(self.ctx.h, self.h, _d(Xnew), k, _d(Yall), _d(ym), _d(ys), _d(lml))
        if rc == ERR_NOT_PD:
            return False
        _chk(rc, "gp_append")
        self.n += k
        self.y_mean, self.y_std, self.lml = ym, ys, lml
        return True

    def predict(self, Xq):
        Xq = f64(np.atleast_2d(Xq)); p = Xq.shape[0]
        mean = np.empty((p, self.n_out)); var = np.empty((p, self.n_out))
        _chk(_L.gpmpc_gp_predict(self.ctx.h, self.h, _d(Xq), p, _d(mean), _d(var)), "gp_predict")
        return mean, var

    def predict_cov(self, Xq):
        Xq = f64(np.atleast_2d(Xq)); p = Xq.shape[0]
        mean = np.empty((p, self.n_out)); cov = np.empty((p, p))
        _chk(_L.gpmpc_gp_predict_cov(self.ctx.h, self.h, _d(Xq), p, _d(mean), _d(cov)), "gp_predict_cov")
        return mean, cov

    def state(self):
        L = np.empty((self.n, self.n)); a = np.empty((self.n, self.n_out))
        _chk(_L.gpmpc_gp_get_state(self.ctx.h, self.h, _d(L), _d(a)), "gp_get_state")
        return L, a

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _L.gpmpc_gp_destroy(self.h)
                self.h = None
        except Exception:
            pass


class FITCHandle:
    """A fitted sparse GP on the device: FITC (gpmpc_fitc_fit) or, with
    ``method="vfe"``, VFE (gpmpc_vfe_fit; ``lam`` is then None)."""

    def __init__(self, ctx, Z, X, Y, ls, sigma2, noise, jitter=1e-6, method="fitc"):
        Z = f64(np.atleast_2d(Z)); X = f64(np.atleast_2d(X)); Y = f64(Y)
        if Y.ndim == 1:
            Y = Y[:, None]
        m, d = Z.shape; n = X.shape[0]; no = Y.shape[1]
        self.ctx = ctx; self.n_out = no; self.m = m
        self.y_mean = np.empty(no); self.y_std = np.empty(no); self.lml = np.empty(no)
        h = _vp()
        prog = ls if isinstance(ls, KernelProgram) else None
        if prog is None:
            ls = f64(np.atleast_1d(ls))
            if ls.size == 1:
                ls = np.full(d, float(ls[0]))
        if prog is not None and method in ("fitc", "vfe"):
            # a composite kernel (``ls`` is its KernelProgram): gpmpc_sparse_fit_prog
            self.lam = np.empty(n) if method == "fitc" else None
            rc = _L.gpmpc_sparse_fit_prog(ctx.h, 0 if method == "fitc" else 1, _i(prog.ops), prog.ops.shape[0],
                                          _d(prog.par), prog.par.size, _d(Z), m, _d(X), n, d, _d(Y), no,
                                          float(noise), float(jitter), ctypes.byref(h), _d(self.y_mean),
                                          _d(self.y_std), _d(self.lml),
                                          _d(self.lam) if self.lam is not None else None)
        elif method == "vfe":
            self.lam = None
            rc = _L.gpmpc_vfe_fit(ctx.h, _d(Z), m, _d(X), n, d, _d(Y), no, _d(ls), float(sigma2),
                                  float(noise), float(jitter), ctypes.byref(h), _d(self.y_mean),
                                  _d(self.y_std), _d(self.lml))
        elif method == "fitc":
            self.lam = np.empty(n)
            rc = _L.gpmpc_fitc_fit(ctx.h, _d(Z), m, _d(X), n, d, _d(Y), no, _d(ls), float(sigma2),
                                   float(noise), float(jitter), ctypes.byref(h), _d(self.y_mean),
                                   _d(self.y_std), _d(self.lml), _d(self.lam))
        else:
            raise ValueError(f"method must be 'fitc' or 'vfe', got {method!r}")
        if rc > 0:
            raise np.linalg.LinAlgError(_L.gpmpc_last_error().decode())
        _chk(rc, "fitc_fit")
        self.h = h

    def predict(self, Xq):
        Xq = f64(np.atleast_2d(Xq)); p = Xq.shape[0]
        mean = np.empty((p, self.n_out)); var = np.empty((p, self.n_out))
        _chk(_L.gpmpc_fitc_predict(self.ctx.h, self.h, _d(Xq), p, _d(mean), _d(var)), "fitc_predict")
        return mean, var

    def alpha(self):
        """The fitted alpha (m x n_out), gpmpc_fitc_get_state."""
        a = np.empty((self.m, self.n_out))
        _chk(_L.gpmpc_fitc_get_state(self.ctx.h, self.h, _d(a)), "fitc_get_state")
        return a

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _L.gpmpc_fitc_destroy(self.h)
                self.h = None
        except Exception:
            pass


def _field_names(struct):
    return {f[0] for f in struct._fields_}


def set_fields(struct, kw, nested=None):
    """Assign keyword settings to a ctypes struct, refusing names it does not
    have (ctypes would silently accept a typo such as ``max_iters``).  Keys
    unknown to ``struct`` go to the ``nested`` member struct when given."""
    own = _field_names(type(struct))
    sub = getattr(struct, nested) if nested else None
    subn = _field_names(type(sub)) if sub is not None else set()
    for k, v in kw.items():
        if k in own and k != nested:
            cur = getattr(struct, k)
            if isinstance(cur, ctypes.Structure) and isinstance(v, dict):  # a nested settings struct
                set_fields(cur, v)
                continue
            if isinstance(cur, ctypes.Array):  # fixed-size array fields take a sequence
                v = np.ravel(np.asarray(v, dtype=np.float64))
                if v.size != len(cur):
                    raise ValueError(f"{k} needs {len(cur)} values, got {v.size}")
                v = type(cur)(*v.tolist())
            setattr(struct, k, v)
        elif k in subn:
            setattr(sub, k, v)
        else:
            raise TypeError(f"unknown setting {k!r} for {type(struct).__name__}")
    return struct


def qp_default_settings(**kw):
    s = QPSettings()
    _L.gpmpc_qp_default_settings(ctypes.byref(s))
    return set_fields(s, kw)


def qp_pattern_info(n, m, rowptr, colidx):
    """gpmpc_qp_pattern_info: which KKT factor path the batched QP takes for the CSR pattern
    (rowptr, colidx) of an m x n A, as a dict over QP_PATTERN_INFO.  Host only: no context."""
    rp = np.ascontiguousarray(rowptr, np.int32); ci = np.ascontiguousarray(colidx, np.int32)
    if rp.size != int(m) + 1 or ci.size < int(rp[-1]):
        raise ValueError(f"rowptr needs m + 1 = {int(m) + 1} entries and colidx rowptr[m], got {rp.size}, {ci.size}")
    info = np.zeros(len(QP_PATTERN_INFO), np.int32)
    _chk(_L.gpmpc_qp_pattern_info(int(n), int(m), _i(rp), _i(ci), _i(info)), "qp_pattern_info")
    return dict(zip(QP_PATTERN_INFO, (int(v) for v in info)))


def rollout6_default_config(**kw):
    """6-DoF rollout config; QP settings may be given flat (``max_iter=...``)."""
    c = Rollout6Config()
    _L.gpmpc_rollout6_default_config(ctypes.byref(c))
    return set_fields(c, kw, nested="qp")


def fleet_default_config(**kw):
    """Fleet config; QP settings may be given flat (``max_iter=...``); the SQP
    passes' settings as ``sqp_qp=dict(...)`` on top of the (final) ``qp``."""
    c = FleetConfig()
    _L.gpmpc_fleet_default_config(ctypes.byref(c))
    sq = kw.pop("sqp_qp", None)
    set_fields(c, kw, nested="qp")
    if sq:   # explicit pass settings on top of qp; otherwise max_iter 0 = "the same as qp"
        c.sqp_qp = c.qp
        set_fields(c.sqp_qp, sq)
    return c


def fleet_mc_attach(h, max_steps, batch, thrust_dispersion=0.0, aero_dispersion=0.0, log=True, noise=None):
    """gpmpc_fleet_mc_attach on the fleet handle ``h``: ``noise`` (batch, max_steps, 4)
    standard normals or None; ``log``: keep the trajectories."""
    cfg = FleetMCConfig(float(thrust_dispersion), float(aero_dispersion), int(max_steps) if log else 0)
    nz = None
    if noise is not None:
        nz = f64(noise)
        if nz.shape != (int(batch), int(max_steps), 4):
            raise ValueError(f"noise must be (batch, max_steps, 4) = {(int(batch), int(max_steps), 4)}, got {nz.shape}")
    _chk(_L.gpmpc_fleet_mc_attach(h, ctypes.byref(cfg), None if nz is None else _d(nz)), "fleet_mc_attach")


def fleet_mc_read_log(h, max_steps, first, count):
    """gpmpc_fleet_mc_read_log: (states (count, max_steps+1, 7), controls (count, max_steps, 3),
    nsteps (count,)); rows past a landing's count are NaN."""
    states = np.empty((count, max_steps + 1, 7)); controls = np.empty((count, max_steps, 3))
    ns = np.zeros(count, np.int32)
    _chk(_L.gpmpc_fleet_mc_read_log(h, int(first), int(count), _d(states), _d(controls), _i(ns)), "fleet_mc_read_log")
    return states, controls, ns


def fleet_mc_detach(h):
    _chk(_L.gpmpc_fleet_mc_detach(h), "fleet_mc_detach")


class QPWorkspace:
    """OSQP-workspace equivalent over gpmpc_qp_solve_batched: a fixed CSR
    pattern of A shared by ``batch`` problems, diagonal P, and the state OSQP
    keeps between solves (rho, scaled y).  Mirrors osqp.OSQP().setup/update/
    warm_start/solve as osqp_rti.py:454-567 drives it."""

    def __init__(self, ctx, n, m, rowptr, colidx, batch=1, settings=None):
        self.ctx = ctx; self.n = int(n); self.m = int(m); self.batch = int(batch)
        self.rowptr = np.ascontiguousarray(rowptr, np.int32)
        self.colidx = np.ascontiguousarray(colidx, np.int32)
        self.nnz = int(self.rowptr[-1])
        self.settings = settings if settings is not None else qp_default_settings()
        self.reset()

    def reset(self):
        """Fresh workspace: rho back to settings.rho, y = 0 (osqp.OSQP().setup)."""
        self.rho = np.full(self.batch, float(self.settings.rho))
        self.y_scaled = np.zeros((self.batch, self.m))

    def solve(self, Aval, Pdiag, q, l, u, x_ws=None, pattern=None):
        """``pattern`` = (rowptr, colidx) replaces the workspace's pattern for this
        solve (a value-filtered A whose non-zeros move); the rows, and
        with them OSQP's persistent y, stay the same."""
        B, n, m = self.batch, self.n, self.m
        rowptr, colidx = self.rowptr, self.colidx
        if pattern is not None:
            rowptr = np.ascontiguousarray(pattern[0], np.int32)
            colidx = np.ascontiguousarray(pattern[1], np.int32)
            assert rowptr.size == m + 1
        nnz = int(rowptr[-1])
        Av = f64(np.reshape(Aval, (B, nnz))); Pd = f64(np.reshape(Pdiag, (B, n)))
        qv = f64(np.reshape(q, (B, n))); lv = f64(np.reshape(l, (B, m))); uv = f64(np.reshape(u, (B, m)))
        xw = None if x_ws is None else f64(np.reshape(x_ws, (B, n)))
        x = np.empty((B, n)); y = np.empty((B, m)); obj = np.empty(B)
        it = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
        rc = _L.gpmpc_qp_solve_batched(self.ctx.h, B, n, m, nnz, _i(rowptr), _i(colidx),
                                       _d(Av), _d(Pd), _d(qv), _d(lv), _d(uv), ctypes.byref(self.settings),
                                       None if xw is None else _d(xw), _d(self.rho), _d(self.y_scaled),
                                       _d(x), _d(y), _i(it), _i(st), _d(obj))
        _chk(rc, "qp_solve_batched")
        return dict(x=x, y=y, iter=it, status=st, obj_val=obj, rho=self.rho.copy())


QP_STATUS_TEXT = {1: "solved", 2: "solved_inaccurate", -2: "maximum iterations reached",
                  -3: "primal infeasible", 3: "primal infeasible inaccurate",
                  -4: "dual infeasible", 4: "dual infeasible inaccurate", -7: "problem non convex",
                  -10: "unsolved", -100: "kkt factorisation failed"}


def _uprop_buffers(what, nx, X0, U, S0):
    """What every propagation wrapper takes and returns: X0 (B, nx), U (B, N, 3) and S0 (None
    or (B, nx, nx)) as contiguous float64, their shapes checked; S0's pointer (or None); the
    means (B, N+1, nx) and covariances (B, N+1, nx, nx) to fill."""
    X0 = f64(np.atleast_2d(X0)); U = f64(U)
    B, N = U.shape[0], U.shape[1]
    if X0.shape != (B, nx) or U.shape != (B, N, 3):
        raise ValueError(f"{what}: shapes X0 {X0.shape}, U {U.shape}")
    s0 = None
    if S0 is not None:
        S0 = f64(S0)
        if S0.shape != (B, nx, nx):
            raise ValueError(f"{what}: S0 shape {S0.shape}")
        s0 = S0.ctypes.data_as(_vp)
    return X0, U, S0, s0, np.empty((B, N + 1, nx)), np.empty((B, N + 1, nx, nx))


def uprop3_linear(ctx, gp, X0, U, S0=None, dt=0.1, alpha=1.0 / 30.0, g=(-1.0, 0.0, 0.0), s0_diag=1e-6):
    """gpmpc_uprop3_linear: the 3-DoF linear uncertainty propagation of B trajectories on the
    device.  gp: an ExactGPHandle of the 3-DoF GP; X0 (B, 7), U (B, N, 3), S0 None or
    (B, 7, 7) -> means (B, N+1, 7), covariances (B, N+1, 7, 7)."""
    X0, U, S0, s0, means, covs = _uprop_buffers("uprop3_linear", 7, X0, U, S0)
    g3 = f64(np.asarray(g, float).reshape(3))
    _chk(_L.gpmpc_uprop3_linear(ctx.h, gp.h, U.shape[0], U.shape[1], float(dt), float(alpha), _d(g3), _d(X0), _d(U), s0,
                                float(s0_diag), _d(means), _d(covs)), "uprop3_linear")
    return means, covs


def uprop6_linear(ctx, hv, hw, exact, rocket, X0, U, S0=None, dt=0.1, s0_diag=1e-6):
    """gpmpc_uprop6_linear: the 14-state linear uncertainty propagation of B trajectories on
    the device.  hv, hw: the StructuredRocketGP's device pair (ExactGPHandle with exact=True,
    else FITCHandle); rocket: 17 doubles (J_B row-major, r_T_B, g_I, alpha, g0); X0 (B, 14),
    U (B, N, 3), S0 None or (B, 14, 14) -> means (B, N+1, 14), covariances (B, N+1, 14, 14)."""
    X0, U, S0, s0, means, covs = _uprop_buffers("uprop6_linear", 14, X0, U, S0)
    rk = f64(np.asarray(rocket, float).reshape(17))
    _chk(_L.gpmpc_uprop6_linear(ctx.h, hv.h, hw.h, int(bool(exact)), _d(rk), U.shape[0], U.shape[1], float(dt), _d(X0), _d(U), s0,
                                float(s0_diag), _d(means), _d(covs)), "uprop6_linear")
    return means, covs


def _ut_buffers(what, nx, X0, U, S0, ut):
    X0, U, S0, s0, means, covs = _uprop_buffers(what, nx, X0, U, S0)
    ut3 = f64(np.asarray(ut, float).reshape(3))
    return X0, U, S0, s0, ut3, means, covs, np.zeros(U.shape[0], np.int32)


def uprop3_unscented(ctx, gp, exact, X0, U, S0=None, dt=0.1, alpha=1.0 / 30.0, g=(-1.0, 0.0, 0.0),
                     ut=(1e-3, 2.0, 0.0), s0_diag=1e-6):
    """gpmpc_uprop3_unscented: the 3-DoF unscented uncertainty propagation of B trajectories
    on the device.  gp: the 3-DoF GP's ExactGPHandle (exact=True) or FITCHandle; ut: the
    transform's (alpha, beta, kappa); X0 (B, 7), U (B, N, 3), S0 None or (B, 7, 7) -> means
    (B, N+1, 7), covariances (B, N+1, 7, 7), info (B,): 0, or k+1 when the Cholesky factor of
    step k failed (that trajectory's later rows are NaN)."""
    X0, U, S0, s0, ut3, means, covs, info = _ut_buffers("uprop3_unscented", 7, X0, U, S0, ut)
    g3 = f64(np.asarray(g, float).reshape(3))
    _chk(_L.gpmpc_uprop3_unscented(ctx.h, gp.h, int(bool(exact)), U.shape[0], U.shape[1], float(dt), float(alpha),
                                   _d(g3), _d(ut3), _d(X0), _d(U), s0, float(s0_diag), _d(means), _d(covs),
                                   _i(info)), "uprop3_unscented")
    return means, covs, info


def uprop6_unscented(ctx, hv, hw, exact, rocket, X0, U, S0=None, dt=0.1, ut=(1e-3, 2.0, 0.0), s0_diag=1e-6):
    """gpmpc_uprop6_unscented: the 14-state unscented uncertainty propagation of B
    trajectories on the device.  hv, hw, exact, rocket as uprop6_linear; ut: the transform's
    (alpha, beta, kappa); X0 (B, 14), U (B, N, 3), S0 None or (B, 14, 14) -> means
    (B, N+1, 14), covariances (B, N+1, 14, 14), info (B,) as uprop3_unscented."""
    X0, U, S0, s0, ut3, means, covs, info = _ut_buffers("uprop6_unscented", 14, X0, U, S0, ut)
    rk = f64(np.asarray(rocket, float).reshape(17))
    _chk(_L.gpmpc_uprop6_unscented(ctx.h, hv.h, hw.h, int(bool(exact)), _d(rk), _d(ut3), U.shape[0], U.shape[1],
                                   float(dt), _d(X0), _d(U), s0, float(s0_diag), _d(means), _d(covs), _i(info)),
         "uprop6_unscented")
    return means, covs, info


def _mc_buffers(what, nx, groups, X0, U, S0, particles0, normals, return_particles):
    U = f64(U); particles0 = f64(particles0); normals = f64(normals)
    if U.ndim != 3 or particles0.ndim != 3:
        raise ValueError(f"{what}: shapes U {U.shape}, particles0 {particles0.shape}")
    X0, U, S0, s0, means, covs = _uprop_buffers(what, nx, X0, U, S0)
    B, N, S = U.shape[0], U.shape[1], particles0.shape[1]
    if particles0.shape != (B, S, nx):
        raise ValueError(f"{what}: particles0 shape {particles0.shape}, expected {(B, S, nx)}")
    if normals.shape != (B, N, S, groups, 3):
        raise ValueError(f"{what}: normals shape {normals.shape}, expected {(B, N, S, groups, 3)}")
    paths = np.empty((B, N + 1, S, nx)) if return_particles else None
    pp = None if paths is None else paths.ctypes.data_as(_vp)
    return X0, U, S0, s0, particles0, normals, means, covs, paths, pp


def uprop3_mc(ctx, gp, exact, X0, U, S0, particles0, normals, dt=0.1, alpha=1.0 / 30.0, g=(-1.0, 0.0, 0.0),
              return_particles=False, s0_diag=1e-6):
    """gpmpc_uprop3_mc: the 3-DoF Monte-Carlo uncertainty propagation of B trajectories on the
    device.  gp, exact as uprop3_unscented; the draws are the caller's: particles0 (B, S, 7)
    and the standard normals (B, N, S, 1, 3); X0 (B, 7), U (B, N, 3), S0 None or (B, 7, 7) ->
    means (B, N+1, 7), covariances (B, N+1, 7, 7), and the particles (B, N+1, S, 7) or None."""
    X0, U, S0, s0, particles0, normals, means, covs, paths, pp = _mc_buffers(
        "uprop3_mc", 7, 1, X0, U, S0, particles0, normals, return_particles)
    g3 = f64(np.asarray(g, float).reshape(3))
    _chk(_L.gpmpc_uprop3_mc(ctx.h, gp.h, int(bool(exact)), U.shape[0], U.shape[1], particles0.shape[1], float(dt),
                            float(alpha), _d(g3), _d(X0), _d(U), s0, float(s0_diag), _d(particles0), _d(normals),
                            _d(means), _d(covs), pp), "uprop3_mc")
    return means, covs, paths


def uprop6_mc(ctx, hv, hw, exact, rocket, X0, U, S0, particles0, normals, dt=0.1, return_particles=False,
              s0_diag=1e-6):
    """gpmpc_uprop6_mc: the 14-state Monte-Carlo uncertainty propagation of B trajectories on
    the device.  hv, hw, exact, rocket as uprop6_linear; particles0 (B, S, 14), normals
    (B, N, S, 2, 3) (per particle the d_v normals, then the d_omega ones); X0 (B, 14), U
    (B, N, 3), S0 None or (B, 14, 14) -> means (B, N+1, 14), covariances (B, N+1, 14, 14), and
    the particles (B, N+1, S, 14) or None."""
    X0, U, S0, s0, particles0, normals, means, covs, paths, pp = _mc_buffers(
        "uprop6_mc", 14, 2, X0, U, S0, particles0, normals, return_particles)
    rk = f64(np.asarray(rocket, float).reshape(17))
    _chk(_L.gpmpc_uprop6_mc(ctx.h, hv.h, hw.h, int(bool(exact)), _d(rk), U.shape[0], U.shape[1],
                            particles0.shape[1], float(dt), _d(X0), _d(U), s0, float(s0_diag), _d(particles0),
                            _d(normals), _d(means), _d(covs), pp), "uprop6_mc")
    return means, covs, paths


def cov_propagate(ctx, A, q, S0=None, s0_diag=1e-6):
    """Batched Sigma_{k+1} = A_k Sigma_k A_k^T + diag(q_k) on the device.
    A (B, N, nx, nx), q (B, N, nx), S0 (B, nx, nx) or None -> (B, N+1, nx, nx)."""
    A = f64(A); q = f64(q)
    B, N, nx = A.shape[0], A.shape[1], A.shape[-1]
    if A.shape != (B, N, nx, nx) or q.shape != (B, N, nx):
        raise ValueError(f"cov_propagate: shapes A {A.shape}, q {q.shape}")
    out = np.empty((B, N + 1, nx, nx))
    s0 = None
    if S0 is not None:
        S0 = f64(S0)
        if S0.shape != (B, nx, nx):
            raise ValueError(f"cov_propagate: S0 shape {S0.shape}")
        s0 = S0.ctypes.data_as(_vp)
    _chk(_L.gpmpc_cov_propagate(ctx.h, B, N, nx, _d(A), _d(q), s0, float(s0_diag), _d(out)),
         "cov_propagate")
    return out


# ---- novelty / diverse-subset selection (csrc/select.hip) ------------------------
# the kernels' shape constants (csrc/select.hip; tests/test_select_host.py keeps them equal)
NN_TILE = 128              # reference rows per LDS tile of gpmpc_nn_dist
SELECT_ONE_THREADS = 512   # path 1's one workgroup
SELECT_ONE_MAXN = 8192     # the most candidates path 1 takes
SELECT_GRID_SLICE = 1024   # candidates per workgroup of path 2
SELECT_CROSSOVER = 6144    # path 0: path 1 up to this n, path 2 above
SELECT_MAXD = 32


def _finite(a, what):
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what} must be finite")


def nn_dist(ctx, X, R):
    """gpmpc_nn_dist: the distance of every row of X (n, d) to its nearest row of R (r, d),
    bit-equal to ``np.min(np.linalg.norm(X[:, None] - R, axis=2), axis=1)``."""
    X = f64(np.atleast_2d(X)); R = f64(np.atleast_2d(R))
    n, d = X.shape
    if R.shape[1] != d:
        raise ValueError(f"nn_dist: X has {d} features, R {R.shape[1]}")
    _finite(X, "nn_dist: X"); _finite(R, "nn_dist: R")
    dist = np.empty(n)
    _chk(_L.gpmpc_nn_dist(ctx.h, _d(X), n, _d(R), R.shape[0], d, _d(dist)), "nn_dist")
    return dist


def select_diverse(ctx, X, scores, n_select, diversity_weight=0.5, path=0):
    """gpmpc_select_diverse: greedy farthest-point picking of n_select of the n rows of X
    (n, d) by scores (n,) -> (indices (n_select,) in pick order, combined (n_select,) each
    pick's winning value).  ``path``: 0 automatic, 1 / 2 force a kernel path."""
    X = f64(np.atleast_2d(X)); n, d = X.shape
    scores = f64(np.asarray(scores).reshape(-1))
    if scores.size != n:
        raise ValueError(f"select_diverse: {n} candidates, {scores.size} scores")
    _finite(X, "select_diverse: X"); _finite(scores, "select_diverse: scores")
    n_select = int(n_select)
    m = max(n_select, 0)
    idx = np.zeros(m, np.int32); comb = np.empty(m)
    _chk(_L.gpmpc_select_diverse(ctx.h, _d(X), n, d, _d(scores), n_select, float(diversity_weight), int(path),
                                 _i(idx), _d(comb)), "select_diverse")
    return idx.astype(np.int64), comb


# ---- k-means for the inducing points (csrc/kmeans.hip) ---------------------------
# the kernels' shape constants (csrc/kmeans.hip; tests/test_kmeans_host.py keeps them equal)
KMEANS_TILE = 128      # centres per LDS tile of the assign kernel
KMEANS_OBS = 64        # observations per workgroup of the assign kernel
KMEANS_WAVES = 8       # its waves: each scans every eighth centre of a tile
KMEANS_MAXD = 32


def kmeans_tau(d):
    """gpmpc_kmeans_tau: the margin at or below which a nearest-centre decision is unsafe."""
    return float(_L.gpmpc_kmeans_tau(int(d)))


def kmeans_lloyd(ctx, X, C0, iters=10):
    """gpmpc_kmeans_lloyd: ``iters`` Lloyd iterations over X (n, d) from the code book C0
    (k, d) -> (C (k, d), labels (n,) int64 of the last assignment, empties (iters,) centres
    without observations per iteration, min_margin, unsafe).  With unsafe == 0, C and labels
    are the bits of ``scipy.cluster.vq.kmeans2(X, C0, iter=iters, minit="matrix")``."""
    X = f64(np.atleast_2d(X)); C0 = f64(np.atleast_2d(C0))
    n, d = X.shape; k = C0.shape[0]
    if C0.shape[1] != d:
        raise ValueError(f"kmeans_lloyd: X has {d} features, C0 {C0.shape[1]}")
    _finite(X, "kmeans_lloyd: X"); _finite(C0, "kmeans_lloyd: C0")
    iters = int(iters)
    C = np.empty((k, d)); labels = np.zeros(n, np.int32); empties = np.zeros(max(iters, 0), np.int32)
    margin = np.zeros(1); unsafe = np.zeros(1, np.int32)
    _chk(_L.gpmpc_kmeans_lloyd(ctx.h, _d(X), n, d, _d(C0), k, iters, _d(C), _i(labels), _i(empties), _d(margin),
                               _i(unsafe)), "kmeans_lloyd")
    return C, labels.astype(np.int64), empties.astype(np.int64), float(margin[0]), int(unsafe[0])


# ---- k-nearest-neighbour search over a resident set (csrc/knn.hip) -----------------
# the kernels' shape constants (csrc/knn.hip; tests/test_knn_plan.py keeps them equal)
KNN_MAXD = 32
KNN_MAXK = 64          # the list a query keeps: one entry a lane
KNN_Q = 2              # queries a wave serves at once (1 for a single query)
KNN_PART_ROWS = 1024   # the least rows of a part of the split
KNN_MAX_PARTS = 64
KNN_TARGET_WG = 512    # the scan's grid is split up to this many workgroups
KNN_KD, KNN_NUMPY = 0, 1   # the summation order of s^2: scipy's KD-tree, np.linalg.norm


def knn_plan(n, d, B, k=KNN_MAXK):
    """gpmpc_knn_plan (no device): (parts, q_per_wave) of a call of B queries over n rows."""
    parts = np.zeros(1, np.int32); q = np.zeros(1, np.int32)
    rc = _L.gpmpc_knn_plan(int(n), int(d), int(B), int(k), _i(parts), _i(q))
    if rc:
        _err(rc, "knn_plan")
    return int(parts[0]), int(q[0])


# ---- projection onto a convex hull (csrc/hull.hip) ----------------------------------
# the kernel's shape constants (csrc/hull.h; tests/test_hull_host.py keeps them equal)
HULL_MAXD = 32
HULL_MAXK = 64
HULL_WAVES = 4         # queries a workgroup serves: one a wave
HULL_MAX_ITER = 4096   # the most cycles a call may ask for, and the wrappers' default
HULL_TOL = 1e-12       # the wrappers' default stop tolerance on the relative gap
HULL_STATUS = {0: "certified", 1: "not certified", 2: "empty vertex set", 3: "non-finite input"}


def hull_plan(d, kmax, B):
    """gpmpc_hull_plan (no device): the queries one workgroup serves."""
    q = np.zeros(1, np.int32)
    rc = _L.gpmpc_hull_plan(int(d), int(kmax), int(B), _i(q))
    if rc:
        _err(rc, "hull_plan")
    return int(q[0])


def _hull_outputs(B, kmax, d):
    return {"lam": np.zeros((B, kmax)), "proj": np.empty((B, d)), "dist": np.empty(B), "gap": np.empty(B),
            "iters": np.zeros(B, np.int32), "status": np.zeros(B, np.int32)}


def _hull_finish(out):
    out["iters"] = out["iters"].astype(np.int64); out["status"] = out["status"].astype(np.int64)
    return out


def hull_project(ctx, V, X, q=None, nv=None, tol=HULL_TOL, max_iter=HULL_MAX_ITER):
    """gpmpc_hull_project: every row of X (B, d) projected onto the hull of its vertex set ->
    dict(lam (B, kmax), proj (B, d), dist, gap, qhull (None without q), iters, status).  V
    (kmax, d): one set for all queries; V (B, kmax, d): a set a query, of which query b uses its
    first nv[b] rows (nv None: all).  q: the vertices' values, shaped as V without its last axis."""
    V = f64(V); X = f64(np.atleast_2d(X))
    B, d = X.shape
    shared = V.ndim == 2
    if V.ndim not in (2, 3) or V.shape[-1] != d or (not shared and V.shape[0] != B):
        raise ValueError(f"hull_project: V is {V.shape}, X {X.shape}")
    kmax = V.shape[-2]
    if q is not None:
        q = f64(q)
        if q.shape != V.shape[:-1]:
            raise ValueError(f"hull_project: q is {q.shape}, expected {V.shape[:-1]}")
    if nv is not None:
        nv = np.ascontiguousarray(np.broadcast_to(np.asarray(nv), (B,)), dtype=np.int32)
    out = _hull_outputs(B, kmax, d)
    qh = np.empty(B)
    _chk(_L.gpmpc_hull_project(ctx.h, _d(V), _d(q) if q is not None else None, _i(nv) if nv is not None else None,
                               int(shared), _d(X), B, kmax, d, float(tol), int(max_iter), _d(out["lam"]),
                               _d(out["proj"]), _d(out["dist"]), _d(out["gap"]), _d(qh) if q is not None else None,
                               _i(out["iters"]), _i(out["status"])), "hull_project")
    out["qhull"] = qh if q is not None else None
    return _hull_finish(out)


class KnnSet:
    """A set of n rows resident on the device (gpmpc_knn): S (n, d) stored as given, q (n,)
    the rows' cost-to-go and fuel_req (n,) the fuel a row needs, either may be None."""

    def __init__(self, ctx, S, q=None, fuel_req=None):
        S = f64(np.atleast_2d(S)); n, d = S.shape
        _finite(S, "KnnSet: S")
        bufs = []
        for name, a in (("q", q), ("fuel_req", fuel_req)):
            if a is not None:
                a = f64(np.asarray(a).reshape(-1))
                if a.size != n:
                    raise ValueError(f"KnnSet: {n} rows, {a.size} {name}")
                _finite(a, f"KnnSet: {name}")
            bufs.append(a)
        h = _vp()
        _chk(_L.gpmpc_knn_create(ctx.h, _d(S), n, d, _d(bufs[0]) if q is not None else None,
                                 _d(bufs[1]) if fuel_req is not None else None, ctypes.byref(h)), "knn_create")
        self.h, self.ctx, self.n, self.d = h, ctx, n, d
        self.has_q, self.has_fuel = q is not None, fuel_req is not None
        self.dp = 0   # features of the payload rows (set_points), 0 without them

    def _queries(self, what, Xq, avail_fuel):
        Xq = f64(np.atleast_2d(Xq))
        if Xq.shape[1] != self.d:
            raise ValueError(f"{what}: the set has {self.d} features, the queries {Xq.shape[1]}")
        _finite(Xq, f"{what}: Xq")
        if avail_fuel is not None:
            avail_fuel = f64(np.broadcast_to(np.asarray(avail_fuel, np.float64), (Xq.shape[0],)))
            _finite(avail_fuel, f"{what}: avail_fuel")
        return Xq, avail_fuel

    def query(self, Xq, k, radius=0.0, avail_fuel=None, order=KNN_KD):
        """gpmpc_knn_query -> idx (B, k) int64 (n where fewer than k rows qualify), dist (B, k),
        n_ball (B,), n_feasible (B,)."""
        Xq, av = self._queries("knn_query", Xq, avail_fuel)
        if not np.isfinite(radius):
            raise ValueError("knn_query: radius must be finite")
        B, k = Xq.shape[0], int(k)
        m = max(k, 0)
        idx = np.zeros((B, m), np.int32); dist = np.empty((B, m))
        nb = np.zeros(B, np.int32); nf = np.zeros(B, np.int32)
        _chk(_L.gpmpc_knn_query(self.h, int(order), _d(Xq), B, k, float(radius), _d(av) if av is not None else None,
                                _i(idx), _d(dist), _i(nb), _i(nf)), "knn_query")
        return idx.astype(np.int64), dist, nb.astype(np.int64), nf.astype(np.int64)

    def interp(self, Xq, k_base, k_min, k_max, adaptive, radius, avail_fuel=None, order=KNN_KD):
        """gpmpc_knn_interp -> q_out (B,), k_used (B,) int64: LocalSafeSet.interpolate_q with
        inverse-distance weights, the K rule included (k_used -1: fewer rows than K)."""
        Xq, av = self._queries("knn_interp", Xq, avail_fuel)
        if not np.isfinite(radius):
            raise ValueError("knn_interp: radius must be finite")
        B = Xq.shape[0]
        out = np.empty(B); used = np.zeros(B, np.int32)
        _chk(_L.gpmpc_knn_interp(self.h, int(order), _d(Xq), B, int(k_base), int(k_min), int(k_max), int(bool(adaptive)),
                                 float(radius), _d(av) if av is not None else None, _d(out), _i(used)), "knn_interp")
        return out, used.astype(np.int64)

    def set_points(self, P):
        """gpmpc_knn_set_points: the payload rows P (n, dp) that ``hull`` takes its vertices from."""
        P = f64(np.atleast_2d(P))
        if P.shape[0] != self.n:
            raise ValueError(f"knn_set_points: {self.n} rows, {P.shape[0]} payload rows")
        _finite(P, "knn_set_points: P")
        _chk(_L.gpmpc_knn_set_points(self.h, _d(P), P.shape[1]), "knn_set_points")
        self.dp = P.shape[1]

    def hull(self, Xq, Xp, k_base, k_min, k_max, adaptive, radius, avail_fuel=None, order=KNN_KD, tol=HULL_TOL,
             max_iter=HULL_MAX_ITER):
        """gpmpc_knn_hull -> the dict of ``hull_project`` plus k_used (B,) and idx (B, k_max) int64:
        the search for Xq, the K rule, and the projection of Xp (B, dp) onto the hull of the K
        nearest payload rows in one call."""
        Xq, av = self._queries("knn_hull", Xq, avail_fuel)
        if not np.isfinite(radius):
            raise ValueError("knn_hull: radius must be finite")
        B, km, dp = Xq.shape[0], max(int(k_max), 0), self.dp
        Xp = f64(np.atleast_2d(Xp))
        if dp and Xp.shape != (B, dp):
            raise ValueError(f"knn_hull: Xp is {Xp.shape}, expected {(B, dp)}")
        out = _hull_outputs(B, km, max(dp, 1))
        used = np.zeros(B, np.int32); idx = np.zeros((B, km), np.int32)
        qh = np.full(B, np.nan)
        _chk(_L.gpmpc_knn_hull(self.h, int(order), _d(Xq), _d(Xp), B, int(k_base), int(k_min), int(k_max),
                               int(bool(adaptive)), float(radius), _d(av) if av is not None else None, float(tol),
                               int(max_iter), _i(used), _i(idx), _d(out["lam"]), _d(out["proj"]), _d(out["dist"]),
                               _d(out["gap"]), _d(qh) if self.has_q else None, _i(out["iters"]), _i(out["status"])),
             "knn_hull")
        out["qhull"] = qh if self.has_q else None
        out["k_used"] = used.astype(np.int64); out["idx"] = idx.astype(np.int64)
        return _hull_finish(out)

    def close(self):
        if self.h:
            _L.gpmpc_knn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- diagnostic: the internal GEMM launchers (gpmpc_gemm_diag) -----------------
GEMM_OP = {"nt": 0, "nn": 1, "nn_batched": 2, "tn": 3, "rowblock": 4, "lat0": 5, "lat1": 6, "syrk_diag": 7,
           "updsolve": 8, "sumsq": 9, "sumsq_mean": 10}
GEMM_TRI_A, GEMM_LOWER_C, GEMM_TRI_B = 1, 2, 4
GEMM_NO_SCRATCH = 8   # gemm_plan only: the plan when the split-K partial buffer is not to be had
GEMM_PATH = {-1: "none", 0: "64", 1: "128", 2: "128_ksplit", 3: "streamk", 4: "splitk", 5: "lat", 6: "syrk_diag",
             7: "updsolve"}
GEMM_GRID = {0: "2d", 1: "tri", 2: "xcd_batch", 3: "rowblock_xcd"}
GEMM_SUMSQ_64, GEMM_SUMSQ_128, GEMM_SUMSQ_SPLITK = 0, 1, 2


class GemmOperand:
    """Where an operand of gemm_diag lies inside a flat float64 device tensor: ``batch``
    matrices of ``rows`` x ``cols`` elements, leading dimension ``ld``, ``stride`` elements
    apart, the first at element ``offset``."""

    def __init__(self, tensor, offset, rows, cols, ld, stride=0, batch=1):
        self.tensor, self.offset, self.rows, self.cols = tensor, int(offset), int(rows), int(cols)
        self.ld, self.stride, self.batch = int(ld), int(stride), int(batch)

    def last(self):
        """The furthest element the description reaches (offset - 1 when it is empty)."""
        if self.rows <= 0 or self.cols <= 0 or self.batch <= 0:
            return self.offset - 1
        return self.offset + (self.batch - 1) * self.stride + (self.rows - 1) * self.ld + self.cols - 1

    def check(self, name, rows, cols, batch):
        import torch
        t = self.tensor
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 1
                and t.is_contiguous()):
            raise ValueError(f"gemm_diag: operand {name} needs a flat contiguous float64 device tensor")
        if self.rows < rows or self.cols < cols or self.batch != batch:
            raise ValueError(f"gemm_diag: operand {name} is described as {self.batch} x {self.rows} x {self.cols}, "
                             f"the operation touches {batch} x {rows} x {cols}")
        if self.ld < self.cols or self.stride < 0 or self.offset < 0:
            raise ValueError(f"gemm_diag: operand {name}: ld {self.ld} < cols {self.cols}, or a negative "
                             "stride / offset")
        if self.last() >= t.numel():
            raise ValueError(f"gemm_diag: operand {name} reaches element {self.last()} of a tensor of {t.numel()}")

    def ptr(self):
        return self.tensor.data_ptr() + 8 * self.offset


def gemm_sumsq_rows(kind, M):
    """Rows of the SUMSQ partial buffer under a forced kind (csrc/gemm.h gemm_sumsq_rows)."""
    return (M + 127) // 128 if kind == GEMM_SUMSQ_128 else (M + 63) // 64


def _gemm_extents(op, M, N, K, p0, p1):
    """(rows, cols) every operand of the operation touches (None: unused)."""
    o = GEMM_OP
    if op in (o["nt"], o["rowblock"], o["lat0"]):
        return {"A": (M, K), "B": (N, K), "C": (M, N), "D": None}
    if op in (o["nn"], o["nn_batched"]):
        return {"A": (M, K), "B": (K, N), "C": (M, N), "D": None}
    if op == o["tn"]:
        return {"A": (K, M), "B": (K, N), "C": (M, N), "D": None}
    if op in (o["lat1"], o["syrk_diag"]):
        return {"A": (M, K), "B": None, "C": (M, M), "D": None}
    if op == o["updsolve"]:
        return {"A": (M, K) if (K > 0 or p0 > 0) else None, "B": (128, K) if K > 0 else None,
                "C": (M, 128 + p0), "D": (128, 128)}
    if op in (o["sumsq"], o["sumsq_mean"]):
        n_out = p1 if op == o["sumsq_mean"] else 0
        rows = gemm_sumsq_rows(p0, M + n_out) if p0 >= 0 else (M + n_out + 63) // 64
        return {"A": (M + n_out, M), "B": (N, M), "C": (rows, N), "D": (n_out, N) if n_out else None}
    raise ValueError(f"gemm_diag: unknown op {op}")


def gemm_diag(ctx, op, M, N, K, A=None, B=None, C=None, D=None, alpha=1.0, beta=0.0, flags=0, p0=0, p1=0,
              batch=1):
    """One internal GEMM launcher on device tensors (gpmpc_gemm_diag; tests only).  ``op`` is
    a GEMM_OP name; A, B, C, D are GemmOperand descriptions (None where the operation takes
    no such operand).  Raises ValueError, before anything is launched, when a description
    is smaller than what the operation touches or reaches past its tensor; HIPError (rc -2)
    when the library refuses the combination.  Returns (path, split, grid) as the names of
    GEMM_PATH / GEMM_GRID and the split count.  The launch is asynchronous on ctx's stream."""
    opc = GEMM_OP[op] if isinstance(op, str) else int(op)
    M, N, K, batch, p0, p1 = int(M), int(N), int(K), int(batch), int(p0), int(p1)
    if min(M, N, K) < 0 or batch < 1:
        raise ValueError("gemm_diag: negative dimension or batch < 1")
    ext = _gemm_extents(opc, M, N, K, p0, p1)
    ops = {"A": A, "B": B, "C": C, "D": D}
    for name, d in ops.items():
        if ext[name] is None:
            continue
        if d is None:
            raise ValueError(f"gemm_diag: operand {name} missing")
        d.check(name, ext[name][0], ext[name][1], batch)

    def g(d, f):
        return f(d) if d is not None else 0

    if opc == GEMM_OP["updsolve"]:
        # Linv is 128 x 128 at ld 128; its batch stride travels as ldd.  B shares A's stride.
        if D.ld != 128:
            raise ValueError("gemm_diag: updsolve's Linv has ld 128")
        if A is not None and B is not None and (B.ld != A.ld or B.stride != A.stride):
            raise ValueError("gemm_diag: updsolve's B shares A's ld and stride")
        if C.ld != (A.ld if A is not None else C.ld):
            raise ValueError("gemm_diag: updsolve's C shares A's ld")
        ldd = D.stride
        lda = C.ld
    else:
        ldd = g(D, lambda d: d.ld)
        lda = g(A, lambda d: d.ld)
    if opc in (GEMM_OP["sumsq"], GEMM_OP["sumsq_mean"]) and (A.ld != M or B.ld != M):
        raise ValueError("gemm_diag: the SUMSQ operands are packed (ld n)")
    if opc == GEMM_OP["syrk_diag"] and (C.ld != A.ld or C.stride != A.stride):
        raise ValueError("gemm_diag: syrk_diag's C shares A's ld and stride")
    path = np.full(3, -9, np.int32)
    rc = _L.gpmpc_gemm_diag(ctx.h, opc, M, N, K, batch, g(A, GemmOperand.ptr) or None, lda,
                            g(A, lambda d: d.stride), g(B, GemmOperand.ptr) or None, g(B, lambda d: d.ld),
                            g(B, lambda d: d.stride), g(C, GemmOperand.ptr) or None, g(C, lambda d: d.ld),
                            g(C, lambda d: d.stride), g(D, GemmOperand.ptr) or None, ldd, float(alpha),
                            float(beta), int(flags), p0, p1, _i(path))
    _chk(rc, "gemm_diag")
    return GEMM_PATH[int(path[0])], int(path[1]), GEMM_GRID[int(path[2])]


def gemm_row_tiles(M, N, K):
    """(rows of the SUMSQ partial buffer its consumers sum, kind the launcher picks) for an
    M x N x K product under this process's switches (gpmpc_gemm_row_tiles; no device)."""
    kind = ctypes.c_int(-9)
    return _L.gpmpc_gemm_row_tiles(int(M), int(N), int(K), ctypes.byref(kind)), kind.value


# csrc/gemm_plan.h: GemmPolicy's fields with their defaults ("auto" for the three-state ones)
GEMM_POLICY = {"big": 1, "kmin": 256, "splitk": 1, "syrk128": -1, "streamk": -1, "ksplit": 0, "remap": 0,
               "xcd_batch": 1, "rowblock_xcd": 1, "post_xcd": 0}


def gemm_plan(op, M, N, K, batch=1, beta=0.0, flags=0, p0=0, p1=0, **switches):
    """What the launcher of ``op`` (a GEMM_OP name with a decision: nt, nn, nn_batched, tn,
    rowblock, sumsq, sumsq_mean) does for the product (gpmpc_gemm_plan; no device):
    (path, split, grid) as gemm_diag reports them, then the launch grid (gx, gy, gz), the tile
    height and the skinny splits' chunk length kc.  Without keywords the plan follows this
    process's GPMPC_* switches; with any, the default policy with those fields of GEMM_POLICY
    replaced."""
    unknown = set(switches) - set(GEMM_POLICY)
    if unknown:
        raise TypeError(f"gemm_plan: unknown switches {sorted(unknown)}")
    pol = np.array(list(dict(GEMM_POLICY, **switches).values()), np.int32)
    out = np.full(8, -9, np.int32)
    opc = GEMM_OP[op] if isinstance(op, str) else int(op)
    _chk(_L.gpmpc_gemm_plan(opc, int(M), int(N), int(K), int(batch), float(beta), int(flags), int(p0), int(p1),
                            _i(pol) if switches else None, _i(out)), "gemm_plan")
    return (GEMM_PATH[int(out[0])], int(out[1]), GEMM_GRID[int(out[2])], (int(out[3]), int(out[4]), int(out[5])),
            int(out[6]), int(out[7]))


GRAM_PATH_ROWS = 64   # gpmpc.h GPMPC_GRAM_PATH_ROWS


def gram_path(n1, d, transpose_out=0):
    """(kernel, D) the Gram launcher takes for n1 rows of d features under this process's
    switches (gpmpc_gram_path; no device): ("k_gram", D) or ("k_gram_rows", D), D = the
    width the kernel is instantiated for (0: the one that reads the width at run time)."""
    p = _L.gpmpc_gram_path(int(n1), int(d), int(transpose_out))
    if p < 0:
        _err(p, "gram_path")
    return ("k_gram_rows" if p & GRAM_PATH_ROWS else "k_gram"), p & ~GRAM_PATH_ROWS


# ---- diagnostic: the batched Cholesky's launch plan (gpmpc_potrf_plan; no device) ----
# csrc/potrf_plan.h: PotrfPolicy's fields with their defaults ("auto" for the three-state ones)
POTRF_POLICY = {"p128": 1, "persist": 0, "lat": -1, "sweep": 1, "trsm": -1, "pk": -1, "ob": 0, "ksplit": 0,
                "fuse": 1, "la": 0, "syrk_diag": 1, "fuse_min": 0, "stamps": 0}
POTRF_STEP = ["diag", "upd_syrk_diag", "upd_rowblock", "updsolve", "psolve_trsm", "psolve_lat", "psolve_rowblock",
              "trail_lat", "trail_syrk"]
POTRF_FORM = ["32", "persist", "128"]


def potrf_plan(n, batch, **switches):
    """The launches gpmpc_potrf_batched_dev makes for (n, batch): (form, steps), form a
    POTRF_FORM name, each step (kind name, c, K0, four operands -- include/gpmpc.h).
    Without keywords the plan follows this process's GPMPC_* switches; with any, it follows
    the default policy with those fields of POTRF_POLICY replaced."""
    unknown = set(switches) - set(POTRF_POLICY)
    if unknown:
        raise TypeError(f"potrf_plan: unknown switches {sorted(unknown)}")
    pol = np.array(list(dict(POTRF_POLICY, **switches).values()), np.int32)
    form = ctypes.c_int(-9)
    cap = 4 * ((int(n) + 127) // 128) + 4   # at most an update, the factor, a solve and a trailing update per block
    buf = np.zeros((cap, 7), np.int32)
    cnt = _L.gpmpc_potrf_plan(int(n), int(batch), _i(pol) if switches else None, ctypes.byref(form), _i(buf), cap)
    if cnt < 0 or cnt > cap:
        _err(cnt, "potrf_plan")
    return POTRF_FORM[form.value], [(POTRF_STEP[r[0]], *map(int, r[1:])) for r in buf[:cnt]]


def _potrf_policy(switches):
    unknown = set(switches) - set(POTRF_POLICY)
    if unknown:
        raise TypeError(f"unknown potrf switches {sorted(unknown)}")
    return np.array(list(dict(POTRF_POLICY, **switches).values()), np.int32)


# ---- diagnostics: the batched Cholesky under an explicit policy, the triangular launchers ----
def potrf_diag(ctx, A, n, batch, offset, ld, stride, info, **switches):
    """gpmpc_potrf_batched_dev under an explicit policy (gpmpc_potrf_diag; tests only) on
    ``batch`` matrices of order n inside the flat float64 device tensor A: the first at
    element ``offset``, leading dimension ``ld``, ``stride`` elements apart.  info: an int32
    device tensor of batch elements.  Without keywords the policy is this process's; with
    any, the default policy with those fields of POTRF_POLICY replaced (as potrf_plan).
    Raises ValueError before anything is launched when the description reaches past A."""
    pol = _potrf_policy(switches)
    n, batch, offset, ld, stride = int(n), int(batch), int(offset), int(ld), int(stride)
    if A.dim() != 1 or A.dtype.itemsize != 8 or not A.is_contiguous() or not A.is_cuda:
        raise ValueError("potrf_diag: A must be a flat contiguous float64 device tensor")
    if n < 0 or batch < 0 or offset < 0 or ld < n or (batch > 1 and stride < (n - 1) * ld + n):
        raise ValueError("potrf_diag: negative size, ld < n, or overlapping batch members")
    if n and batch and offset + (batch - 1) * stride + (n - 1) * ld + n > A.numel():
        raise ValueError("potrf_diag: the matrices reach past the tensor")
    if info.numel() < batch or info.dtype.itemsize != 4 or not info.is_cuda:
        raise ValueError("potrf_diag: info must be an int32 device tensor of batch elements")
    _chk(_L.gpmpc_potrf_diag(ctx.h, n, batch, A.data_ptr() + 8 * offset, ld, stride, info.data_ptr(),
                             _i(pol) if switches else None), "potrf_diag")


TRI_OP = {"trsm": 0, "tri_inverse": 1, "cho_solve_inv": 2, "potrs_cols": 3}
TRI_TRANS, TRI_RHS_LOWER = 1, 2


def tri_diag(ctx, op, n, nrhs, L, X, W=None, flags=0):
    """One triangular launcher or solve helper on device tensors (gpmpc_tri_diag; tests
    only).  L, X, W are (flat float64 device tensor, offset, ld) triples: L n x n, X n x nrhs
    (overwritten), W n x n (cho_solve_inv only).  Raises ValueError before anything is
    launched when a description reaches past its tensor; HIPError (rc -2) when the arguments
    are outside the launcher's contract."""
    opc = TRI_OP[op] if isinstance(op, str) else int(op)
    n, nrhs = int(n), int(nrhs)
    if n < 1 or nrhs < 1:
        raise ValueError("tri_diag: n and nrhs must be positive")

    def ptr(name, d, rows, cols):
        t, off, ld = d
        off, ld = int(off), int(ld)
        if t.dim() != 1 or t.dtype.itemsize != 8 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"tri_diag: operand {name} needs a flat contiguous float64 device tensor")
        if off < 0 or ld < cols or off + (rows - 1) * ld + cols > t.numel():
            raise ValueError(f"tri_diag: operand {name} has ld {ld} < {cols} or reaches past its tensor")
        return t.data_ptr() + 8 * off, ld

    pl, ldl = ptr("L", L, n, n)
    px, ldx = ptr("X", X, n, nrhs)
    pw = None
    if W is not None:
        pw, ldw = ptr("W", W, n, n)
        if ldw != n:
            raise ValueError("tri_diag: W is packed (ld n)")
    _chk(_L.gpmpc_tri_diag(ctx.h, opc, n, nrhs, pl, ldl, px, ldx, pw, int(flags)), "tri_diag")


# ---- predictive safety filter (csrc/safety.hip) ----------------------------------------------
def safety_default_config(**kw):
    """gpmpc_safety_config at the library defaults with the keyword fields replaced (array
    fields take any sequence of the right size)."""
    c = SafetyConfig()
    _L.gpmpc_safety_default_config(ctypes.byref(c))
    return set_fields(c, kw)


def safety_filter(ctx, rocket, cfg, X, U_nom):
    """gpmpc_safety_filter: the predictive safety filter at B states X (B, 14) with nominal
    controls U_nom (B, 3) in one device call.  rocket: 17 doubles as uprop6_linear; cfg: a
    SafetyConfig -> u_safe (B, 3), margin (B,), backup_value (B,), flags (B,; bit 0 modified,
    bit 1 safe), viol_mask (B,; bit 0 immediate, bit 1 + k path_k), iters (B,)."""
    X = f64(np.atleast_2d(X)); U_nom = f64(np.atleast_2d(U_nom))
    B = X.shape[0]
    if B and (X.shape != (B, 14) or U_nom.shape != (B, 3)):
        raise ValueError(f"safety_filter: shapes X {X.shape}, U_nom {U_nom.shape}")
    rk = f64(np.asarray(rocket, float).reshape(17))
    u_safe = np.empty((B, 3)); margin = np.empty(B); value = np.empty(B)
    flags = np.zeros(B, np.int32); mask = np.zeros(B, np.int32); iters = np.zeros(B, np.int32)
    _chk(_L.gpmpc_safety_filter(ctx.h, _d(rk), ctypes.byref(cfg), B, _d(X), _d(U_nom), _d(u_safe), _d(margin),
                                _d(value), _i(flags), _i(mask), _i(iters)), "safety_filter")
    return u_safe, margin, value, flags, mask, iters


def safety_simulate(ctx, rocket, cfg, X0, U_nom):
    """gpmpc_safety_simulate: the closed loop filter -> plant step of B starts X0 (B, 14) over
    the nominal controls U_nom (B, T, 3) in one device call -> X (B, T+1, 14), U (B, T, 3),
    margin, flags, iters (each (B, T))."""
    X0 = f64(np.atleast_2d(X0)); U_nom = f64(U_nom)
    B = X0.shape[0]
    if U_nom.ndim != 3 or (B and (X0.shape != (B, 14) or U_nom.shape[::2] != (B, 3))):
        raise ValueError(f"safety_simulate: shapes X0 {X0.shape}, U_nom {U_nom.shape}")
    T = U_nom.shape[1]
    rk = f64(np.asarray(rocket, float).reshape(17))
    X = np.empty((B, T + 1, 14)); U = np.empty((B, T, 3)); margin = np.empty((B, T))
    flags = np.zeros((B, T), np.int32); iters = np.zeros((B, T), np.int32)
    _chk(_L.gpmpc_safety_simulate(ctx.h, _d(rk), ctypes.byref(cfg), B, T, _d(X0), _d(U_nom), _d(X), _d(U),
                                  _d(margin), _i(flags), _i(iters)), "safety_simulate")
    return X, U, margin, flags, iters


# ---- tube MPC: uncertainty tubes (csrc/tube.hip) ------------------------------------------------
def tube_plan(N=0, n_samples=0):
    """gpmpc_tube_plan (no device): (k_tile, mc_cap): the horizon steps one pass of the linear
    kernel takes and the largest n_samples tube_mc accepts."""
    kt = np.zeros(1, np.int32); cap = np.zeros(1, np.int32)
    rc = _L.gpmpc_tube_plan(int(N), int(n_samples), _i(kt), _i(cap))
    if rc:
        _err(rc, "tube_plan")
    return int(kt[0]), int(cap[0])


def _tube_traj(what, X_nom, U_nom):
    X_nom = f64(X_nom); U_nom = f64(U_nom)
    if X_nom.ndim != 3 or U_nom.ndim != 3 or X_nom.shape[2] != 14 or U_nom.shape[2] != 3 or (
            X_nom.shape[0] != U_nom.shape[0] or X_nom.shape[1] != U_nom.shape[1] + 1):
        raise ValueError(f"{what}: shapes X_nom {X_nom.shape}, U_nom {U_nom.shape}")
    return X_nom, U_nom, X_nom.shape[0], U_nom.shape[1]


def tube_linear(ctx, rocket, X_nom, U_nom, dt, eps=1e-6, w=None, w_max=0.1, K=None, return_AB=False):
    """gpmpc_tube_linear: the linear tubes of B nominal trajectories X_nom (B, N+1, 14), U_nom
    (B, N, 3) in one device call.  w: None (w_max on every row), (14,) or (B, N, 14); K: None or
    (3, 14) -> tubes (B, N+1, 14), and with return_AB the linearisations A (B, N, 14, 14) and
    B (B, N, 14, 3)."""
    X_nom, U_nom, B, N = _tube_traj("tube_linear", X_nom, U_nom)
    rk = f64(np.asarray(rocket, float).reshape(17))
    mode, wp = 0, None
    if w is not None:
        w = f64(w)
        if w.shape not in ((14,), (B, N, 14)):
            raise ValueError(f"tube_linear: w shape {w.shape}, expected (14,) or {(B, N, 14)}")
        mode, wp = (1 if w.ndim == 1 else 2), _d(w)
    Kp = None
    if K is not None:
        K = f64(K)
        if K.shape != (3, 14):
            raise ValueError(f"tube_linear: K shape {K.shape}, expected (3, 14)")
        Kp = _d(K)
    tubes = np.empty((B, N + 1, 14))
    A = np.empty((B, N, 14, 14)) if return_AB else None
    Bm = np.empty((B, N, 14, 3)) if return_AB else None
    _chk(_L.gpmpc_tube_linear(ctx.h, _d(rk), B, N, float(dt), float(eps), _d(X_nom), _d(U_nom), wp, mode, float(w_max),
                              Kp, _d(tubes), _d(A) if return_AB else None, _d(Bm) if return_AB else None),
         "tube_linear")
    return (tubes, A, Bm) if return_AB else tubes


def tube_mc(ctx, rocket, X_nom, U_nom, noise, dt, quantile=0.95):
    """gpmpc_tube_mc: the Monte-Carlo quantile tubes of B nominal trajectories over the
    caller's draws noise (B, N, n_samples, 14) in one device call -> tubes (B, N+1, 14)."""
    X_nom, U_nom, B, N = _tube_traj("tube_mc", X_nom, U_nom)
    noise = f64(noise)
    if noise.ndim != 4 or noise.shape[:2] != (B, N) or noise.shape[3] != 14:
        raise ValueError(f"tube_mc: noise shape {noise.shape}, expected {(B, N)} x n_samples x 14")
    rk = f64(np.asarray(rocket, float).reshape(17))
    tubes = np.empty((B, N + 1, 14))
    _chk(_L.gpmpc_tube_mc(ctx.h, _d(rk), B, N, noise.shape[2], float(dt), float(quantile), _d(X_nom), _d(U_nom),
                          _d(noise), _d(tubes)), "tube_mc")
    return tubes


# ---- baseline controllers and dispersed plants (csrc/baseline.hip) ------------------------------
def baseline_default_config(**kw):
    """gpmpc_baseline_config at the library defaults with the keyword fields replaced."""
    c = BaselineConfig()
    _L.gpmpc_baseline_default_config(ctypes.byref(c))
    return set_fields(c, kw)


def baseline_fly(ctx, x0, kind, max_steps, dt, alpha=1.0 / 30.0, g=(-1.0, 0.0, 0.0), K=None, u_hover=None,
                 T_lo=0.0, T_hi=6.5, gimbal_max=0.5, pid=None, U_ref=None, thrust_table=None, wind_table=None,
                 wind_rows=None, wind_altitude_factor=False, drag_cda=None, sim_thrust=0.0, sim_aero=0.0, noise=None,
                 log=True, timing=None):
    """gpmpc_baseline_fly: B landings from x0 (B, 7) under one baseline controller in one device
    call.  kind 0 LQR (K (B, 3, 7), u_hover (B, 3), the clips), 1 PID (pid: the
    gpmpc_baseline_config gain fields by name), 2 open loop (U_ref (n, 3)).  The dispersed plant:
    thrust_table (>= B + max_steps, 4), wind_table (rows, 3) with wind_rows (max_steps,) and
    wind_altitude_factor, drag_cda (B,); the simulator's own dispersions: sim_thrust, sim_aero
    over noise (B, max_steps, 4).  -> records (B, 16), nsteps (B,), log (max_steps, B, 10) or
    None (rows past nsteps.max() are not written).  timing: a dict that receives "kernel_ms"."""
    x0 = f64(np.atleast_2d(x0))
    B, T = x0.shape[0], int(max_steps)
    if x0.shape != (B, 7):
        raise ValueError(f"baseline_fly: x0 shape {x0.shape}, expected (B, 7)")
    cfg = baseline_default_config(kind=int(kind), batch=B, max_steps=T, dt=float(dt), alpha=float(alpha), g=g,
                                  T_lo=float(T_lo), T_hi=float(T_hi), gimbal_max=float(gimbal_max),
                                  sim_thrust=float(sim_thrust), sim_aero=float(sim_aero), log=int(bool(log)))
    if pid:
        set_fields(cfg, {k: float(v) for k, v in pid.items()})

    def arr(a, shape, what, dtype=np.float64):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if any(s is not None and s != t for s, t in zip(shape, a.shape)) or a.ndim != len(shape):
            raise ValueError(f"baseline_fly: {what} shape {a.shape}, expected {shape}")
        return a

    K = arr(K, (B, 3, 7), "K")
    u_hover = arr(u_hover, (B, 3), "u_hover")
    U_ref = arr(U_ref, (None, 3), "U_ref")
    thrust_table = arr(thrust_table, (None, 4), "thrust_table")
    wind_table = arr(wind_table, (None, 3), "wind_table")
    wind_rows = arr(wind_rows, (T,), "wind_rows", np.int32)
    drag_cda = arr(drag_cda, (B,), "drag_cda")
    noise = arr(noise, (B, T, 4), "noise")
    cfg.n_ref = 0 if U_ref is None else len(U_ref)
    cfg.thrust_rows = 0 if thrust_table is None else len(thrust_table)
    if wind_table is not None:
        cfg.wind_kind, cfg.wind_rows = (2 if wind_altitude_factor else 1), len(wind_table)
    cfg.drag = int(drag_cda is not None)
    rec = np.zeros((B, 16)); ns = np.zeros(B, np.int32)
    logbuf = np.empty((T, B, 10)) if log and B * T > 0 else None
    ms = np.zeros(1)
    p = lambda a, f=_d: None if a is None else f(a)   # noqa: E731
    _chk(_L.gpmpc_baseline_fly(ctx.h, ctypes.byref(cfg), _d(x0), p(K), p(u_hover), p(U_ref), p(thrust_table),
                               p(wind_table), p(wind_rows, _i), p(drag_cda), p(noise), _d(rec), _i(ns), p(logbuf),
                               _d(ms) if timing is not None else None), "baseline_fly")
    if timing is not None:
        timing["kernel_ms"] = float(ms[0])
    return rec, ns, logbuf
