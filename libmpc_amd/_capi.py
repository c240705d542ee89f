"""ctypes binding of the mpcx C ABI (include/mpcx.h).  Product code: loads
libmpc_amd/libmpcx.so and fails loudly when it is missing -- there is no fallback."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPCX_LIBRARY", os.path.join(_HERE, "libmpcx.so"))   # override: testing aid for build variants

OK = 0
E_INVALID, E_UNSUPPORTED, E_DEVICE, E_NUMERIC, E_STATE = -1, -2, -3, -4, -5
STATUS_SUCCESS, STATUS_MAX_ITERATION, STATUS_INFEASIBLE, STATUS_ERROR, STATUS_UNKNOWN = range(5)
REF_SHARED, REF_PER_INSTANCE, REF_PER_STEP = 0, 1, 2
DARE_CONTROL, DARE_ESTIMATOR = 0, 1
REF_PREVIEW = 3          # loops only: [B x (ticks + ph) x n], a window of ph rows per tick


class Dims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nx", "nu", "ndu", "ny", "ph", "ch")]


class LParams(C.Structure):
    """POD mirror of mpc::LParameters (reference include/mpc/Types.hpp:99-161)."""
    _fields_ = [("maximum_iteration", C.c_int), ("time_limit", C.c_double), ("enable_warm_start", C.c_int),
                ("alpha", C.c_double), ("rho", C.c_double), ("eps_rel", C.c_double), ("eps_abs", C.c_double),
                ("eps_prim_inf", C.c_double), ("eps_dual_inf", C.c_double),
                ("verbose", C.c_int), ("adaptive_rho", C.c_int), ("polish", C.c_int)]


class Batch(C.Structure):
    _fields_ = [("batch", C.c_int),
                ("x0", C.c_void_p), ("u0", C.c_void_p),
                ("yref", C.c_void_p), ("yref_mode", C.c_int),
                ("uref", C.c_void_p), ("uref_mode", C.c_int),
                ("duref", C.c_void_p), ("duref_mode", C.c_int),
                ("dmeas", C.c_void_p), ("dmeas_mode", C.c_int),
                ("cmd", C.c_void_p), ("cost", C.c_void_p),
                ("status", C.c_void_p), ("solver_status", C.c_void_p), ("is_feasible", C.c_void_p),
                ("iterations", C.c_void_p),
                ("active_lower", C.c_void_p), ("active_upper", C.c_void_p),
                ("seq_state", C.c_void_p), ("seq_output", C.c_void_p), ("seq_input", C.c_void_p),
                ("polish_rounds", C.c_void_p), ("active_count", C.c_void_p),
                ("warm_active_lower", C.c_void_p), ("warm_active_upper", C.c_void_p), ("warm_shift", C.c_int)]


class LoopDesc(C.Structure):
    """mpcx_lmpc_loop_desc: a closed-loop run on the device (plant_A / _B / _Bd are host pointers, everything else device pointers)"""
    _fields_ = [("batch", C.c_int), ("ticks", C.c_int),
                ("plant_A", C.c_void_p), ("plant_B", C.c_void_p), ("plant_Bd", C.c_void_p),
                ("x0", C.c_void_p), ("u0", C.c_void_p),
                ("yref", C.c_void_p), ("yref_mode", C.c_int),
                ("uref", C.c_void_p), ("uref_mode", C.c_int),
                ("duref", C.c_void_p), ("duref_mode", C.c_int),
                ("dmeas", C.c_void_p), ("dmeas_mode", C.c_int),
                ("noise", C.c_void_p), ("carry_working_set", C.c_int),
                ("traj_x", C.c_void_p), ("traj_u", C.c_void_p), ("traj_cost", C.c_void_p),
                ("traj_status", C.c_void_p), ("traj_solver_status", C.c_void_p), ("traj_iterations", C.c_void_p),
                ("traj_polish_rounds", C.c_void_p), ("traj_active_count", C.c_void_p),
                ("plant_batch", C.c_void_p)]


class LoopGradDesc(C.Structure):
    """mpcx_lmpc_loop_grad_desc: the backward pass of a plain closed loop (device pointers throughout)"""
    _fields_ = ([("seed_x", C.c_void_p), ("seed_u", C.c_void_p), ("reduce", C.c_int)] +
                [("d_" + n, C.c_void_p) for n in ("x0", "u0", "yref", "noise", "plant", "oweight", "uweight", "duweight", "A", "B", "C", "Bd", "Dd")] +
                [("flags", C.c_void_p), ("n_used", C.c_void_p)])


class ObserverDesc(C.Structure):
    """mpcx_lmpc_observer_desc: the observer of an observed loop (gain is a host pointer, everything else device pointers)"""
    _fields_ = [("gain", C.c_void_p), ("gain_batch", C.c_void_p), ("xhat0", C.c_void_p), ("meas_noise", C.c_void_p),
                ("traj_xhat", C.c_void_p), ("traj_y", C.c_void_p)]


class DisturbanceObserverDesc(C.Structure):
    """mpcx_lmpc_disturbance_observer_desc: the observer of an offset-free loop (gain is a host pointer, everything else device pointers)"""
    _fields_ = [("gain", C.c_void_p), ("gain_batch", C.c_void_p), ("xhat0", C.c_void_p), ("dhat0", C.c_void_p), ("meas_noise", C.c_void_p),
                ("traj_xhat", C.c_void_p), ("traj_dhat", C.c_void_p), ("traj_y", C.c_void_p)]


class TargetDesc(C.Structure):
    """mpcx_lmpc_target_desc: the steady-state targets of an offset-free loop (map is a host pointer, everything else device pointers)"""
    _fields_ = [("map", C.c_void_p), ("map_batch", C.c_void_p), ("traj_us", C.c_void_p)]


class Sens(C.Structure):
    """mpcx_lmpc_sens: sensitivities of a solved batch (device pointers throughout)"""
    _fields_ = [("batch", C.c_int), ("active_lower", C.c_void_p), ("active_upper", C.c_void_p), ("status", C.c_void_p),
                ("mode", C.c_int), ("seed_cmd", C.c_void_p), ("seed_input", C.c_void_p),
                ("d_x0", C.c_void_p), ("d_u0", C.c_void_p), ("d_yref", C.c_void_p), ("flags", C.c_void_p)]


SENS_JACOBIAN, SENS_VJP = 0, 1


class ParamSens(C.Structure):
    """mpcx_lmpc_param_sens: parameter sensitivities of a solved batch (device pointers; `solved` points to a Batch)"""
    _fields_ = [("solved", C.c_void_p), ("seed_cmd", C.c_void_p), ("seed_input", C.c_void_p), ("reduce", C.c_int),
                ("d_oweight", C.c_void_p), ("d_uweight", C.c_void_p), ("d_duweight", C.c_void_p),
                ("d_lower", C.c_void_p), ("d_upper", C.c_void_p), ("flags", C.c_void_p), ("n_used", C.c_void_p)]


class ModelSens(C.Structure):
    """mpcx_lmpc_model_sens: model sensitivities of a solved batch (device pointers; `solved` points to a Batch)"""
    _fields_ = [("solved", C.c_void_p), ("seed_cmd", C.c_void_p), ("seed_input", C.c_void_p), ("reduce", C.c_int),
                ("d_A", C.c_void_p), ("d_B", C.c_void_p), ("d_C", C.c_void_p), ("d_Bd", C.c_void_p), ("d_Dd", C.c_void_p),
                ("flags", C.c_void_p), ("n_used", C.c_void_p)]


class BankGrad(C.Structure):
    """mpcx_lmpc_bank_grad: gradients of a bank's solved batch on weights, bounds and models (device pointers; `solved` points to a Batch)"""
    _fields_ = ([("solved", C.c_void_p), ("seed_cmd", C.c_void_p), ("seed_input", C.c_void_p)] +
                [("d_" + n, C.c_void_p) for n in ("oweight", "uweight", "duweight", "lower", "upper", "A", "B", "C", "Bd", "Dd")] +
                [("flags", C.c_void_p), ("group_order", C.c_void_p), ("group_offsets", C.c_void_p)] +
                [("c_" + n, C.c_void_p) for n in ("oweight", "uweight", "duweight", "lower", "upper", "A", "B", "C", "Bd", "Dd")] +
                [("n_used", C.c_void_p)])


class Info(C.Structure):
    _fields_ = [("n_ref", C.c_int), ("m_ref", C.c_int), ("neq_ref", C.c_int), ("nz", C.c_int), ("mg", C.c_int),
                ("active_words", C.c_int), ("kernel_variant", C.c_int),
                ("flops_setup", C.c_double), ("flops_per_admm_iter", C.c_double),
                ("flops_fixed_per_solve", C.c_double), ("bytes_per_solve", C.c_double)]


EXPORTS = [
    "mpcx_lmpc_create", "mpcx_lmpc_destroy", "mpcx_lparams_default", "mpcx_last_error",
    "mpcx_lmpc_set_state_space_model", "mpcx_lmpc_set_disturbances",
    "mpcx_lmpc_set_objective_weights", "mpcx_lmpc_set_objective_weights_slice",
    "mpcx_lmpc_set_state_bounds", "mpcx_lmpc_set_state_bounds_slice",
    "mpcx_lmpc_set_input_bounds", "mpcx_lmpc_set_input_bounds_slice",
    "mpcx_lmpc_set_output_bounds", "mpcx_lmpc_set_output_bounds_slice",
    "mpcx_lmpc_set_input_rate_bounds", "mpcx_lmpc_set_input_rate_bounds_slice",
    "mpcx_lmpc_set_soft_constraint_weights", "mpcx_lmpc_set_soft_constraint_weights_slice",
    "mpcx_lmpc_set_terminal_cost",
    "mpcx_lmpc_set_linear_constraints", "mpcx_lmpc_set_linear_constraints_slice",
    "mpcx_lmpc_set_linear_constraint_weights", "mpcx_lmpc_set_linear_constraint_weights_slice",
    "mpcx_lmpc_set_scalar_constraint_slice", "mpcx_lmpc_set_scalar_constraint_index",
    "mpcx_lmpc_set_references", "mpcx_lmpc_set_references_slice",
    "mpcx_lmpc_set_exogenous_inputs", "mpcx_lmpc_set_exogenous_inputs_slice",
    "mpcx_lmpc_set_optimizer_parameters", "mpcx_lmpc_set_strict_infeasibility", "mpcx_lmpc_setup", "mpcx_lmpc_solve_batch",
    "mpcx_lmpc_time_solve_batch", "mpcx_lmpc_sensitivity_batch", "mpcx_lmpc_sens_size", "mpcx_lmpc_sensitivity_host",
    "mpcx_lmpc_param_sensitivity_batch", "mpcx_lmpc_param_sens_size", "mpcx_lmpc_param_sens_reserve", "mpcx_lmpc_param_sensitivity_host",
    "mpcx_lmpc_model_sensitivity_batch", "mpcx_lmpc_model_sens_size", "mpcx_lmpc_model_sens_reserve", "mpcx_lmpc_model_sensitivity_host", "mpcx_lmpc_solve_host", "mpcx_lmpc_get_info", "mpcx_version",
    "mpcx_lmpc_graph_create", "mpcx_lmpc_graph_launch", "mpcx_lmpc_graph_destroy",
    "mpcx_lmpc_loop_create", "mpcx_lmpc_loop_run", "mpcx_lmpc_loop_destroy", "mpcx_lmpc_loop_desc_size",
    "mpcx_lmpc_loop_grad_create", "mpcx_lmpc_loop_grad_run", "mpcx_lmpc_loop_grad_destroy", "mpcx_lmpc_loop_grad_desc_size",
    "mpcx_lmpc_loop_create_observed", "mpcx_lmpc_hetero_loop_create_observed", "mpcx_lmpc_observer_desc_size", "mpcx_lmpc_kalman_gain",
    "mpcx_lmpc_loop_create_offset_free", "mpcx_lmpc_hetero_loop_create_offset_free", "mpcx_lmpc_disturbance_observer_desc_size",
    "mpcx_lmpc_loop_create_offset_free_target", "mpcx_lmpc_hetero_loop_create_offset_free_target", "mpcx_lmpc_target_desc_size",
    "mpcx_target_map_batch", "mpcx_target_apply_batch",
    "mpcx_nlmpc_create", "mpcx_nlmpc_destroy", "mpcx_nlmpc_get_dims", "mpcx_nlmpc_evaluate_batch",
    "mpcx_nlparams_default", "mpcx_nlmpc_set_optimizer_parameters", "mpcx_nlmpc_solve_batch", "mpcx_nlmpc_time_solve_batch", "mpcx_discretize_batch", "mpcx_dare_batch",
    "mpcx_nlmpc_set_state_bounds_slice", "mpcx_nlmpc_set_input_bounds_slice", "mpcx_nlmpc_solve_host",
    "mpcx_nlmpc_create_custom", "mpcx_nlmpc_create_from_source", "mpcx_nlmpc_set_input_scale", "mpcx_nlmpc_set_state_scale",
    "mpcx_nlmpc_loop_create", "mpcx_nlmpc_loop_run", "mpcx_nlmpc_loop_destroy", "mpcx_nlmpc_loop_desc_size", "mpcx_nlmpc_plant_step_batch",
    "mpcx_nlmpc_loop_create_observed", "mpcx_nlmpc_ekf_desc_size", "mpcx_nlmpc_ekf_step_batch",
    "mpcx_comm_get_unique_id", "mpcx_comm_create", "mpcx_comm_destroy", "mpcx_comm_rank", "mpcx_comm_world", "mpcx_allgather_u",
    "mpcx_lmpc_hetero_create", "mpcx_lmpc_hetero_destroy", "mpcx_lmpc_hetero_get_info", "mpcx_lmpc_hetero_solve_batch",
    "mpcx_lmpc_hetero_time_solve_batch", "mpcx_lmpc_hetero_create_ex", "mpcx_lmpc_hetero_debug_get", "mpcx_lmpc_hetero_loop_create",
    "mpcx_lmpc_hetero_sensitivity_batch", "mpcx_lmpc_hetero_gradient_batch", "mpcx_lmpc_bank_grad_size",
    # profiling and testing aids (declared in include/mpcx.h under that heading)
    "mpcx_lmpc_set_total_batch", "mpcx_lmpc_debug_time_kernels", "mpcx_lmpc_debug_get", "mpcx_lmpc_debug_setup_counts", "mpcx_lmpc_debug_use_fused",
    "mpcx_lmpc_debug_force_generic", "mpcx_lmpc_debug_set_rounds", "mpcx_lmpc_debug_set_cycle_buffer", "mpcx_lmpc_debug_wave_reduce", "mpcx_lmpc_debug_ws_solve",
    "mpcx_lmpc_loop_debug_replay", "mpcx_lmpc_loop_debug_tick", "mpcx_nlmpc_loop_debug_replay", "mpcx_nlmpc_loop_debug_tick",
    "mpcx_dare_debug_product", "mpcx_nlmpc_debug_set_tolerances", "mpcx_nlmpc_debug_last_form", "mpcx_nlmpc_last_form", "mpcx_nlmpc_debug_get_ws", "mpcx_nlmpc_debug_generated_source", "mpcx_nlmpc_debug_compile_source",
]


class NLParams(C.Structure):
    """mpcx_nlparams == mpc::NLParameters (Types.hpp:99-144)"""
    _fields_ = [("maximum_iteration", C.c_int), ("time_limit", C.c_double), ("enable_warm_start", C.c_int),
                ("relative_ftol", C.c_double), ("relative_xtol", C.c_double), ("absolute_ftol", C.c_double),
                ("absolute_xtol", C.c_double), ("hard_constraints", C.c_int)]


class NlmpcBatch(C.Structure):
    _fields_ = [("batch", C.c_int), ("x0", C.c_void_p), ("u0", C.c_void_p), ("z_warm", C.c_void_p), ("cmd", C.c_void_p),
                ("cost", C.c_void_p), ("status", C.c_void_p), ("solver_status", C.c_void_p), ("is_feasible", C.c_void_p),
                ("iterations", C.c_void_p), ("z", C.c_void_p), ("seq_state", C.c_void_p), ("seq_input", C.c_void_p),
                ("seq_output", C.c_void_p), ("warm_curvature", C.c_int), ("multipliers", C.c_void_p), ("params", C.c_void_p)]


class NlmpcLoopDesc(C.Structure):
    """mpcx_nlmpc_loop_desc: an NLMPC closed-loop run on the device (device pointers throughout)"""
    _fields_ = [("batch", C.c_int), ("ticks", C.c_int), ("x0", C.c_void_p), ("u0", C.c_void_p),
                ("params", C.c_void_p), ("plant_params", C.c_void_p), ("noise", C.c_void_p),
                ("substeps", C.c_int), ("warm", C.c_int),
                ("traj_x", C.c_void_p), ("traj_u", C.c_void_p), ("traj_cost", C.c_void_p),
                ("traj_status", C.c_void_p), ("traj_solver_status", C.c_void_p), ("traj_is_feasible", C.c_void_p),
                ("traj_iterations", C.c_void_p)]


class NlmpcEkfDesc(C.Structure):
    """mpcx_nlmpc_ekf_desc: the extended Kalman filter of an observed NLMPC loop (Cm, Q, R, P0 are host pointers, everything else device pointers)"""
    _fields_ = [("ny", C.c_int), ("Cm", C.c_void_p), ("Q", C.c_void_p), ("R", C.c_void_p), ("P0", C.c_void_p),
                ("xhat0", C.c_void_p), ("meas_noise", C.c_void_p), ("traj_xhat", C.c_void_p), ("traj_y", C.c_void_p),
                ("traj_P", C.c_void_p), ("ekf_flags", C.c_void_p)]


class NlmpcDims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nx", "nu", "ph", "ch", "nz", "neq", "nineq", "jeq_w", "neq_user", "ny", "nbnd", "n_params")]


class NlmpcSource(C.Structure):
    """mpcx_nlmpc_source: user hooks as C++ text (the bodies of the reference's lambdas), compiled at run time"""
    _fields_ = ([(n, C.c_int) for n in ("nx", "nu", "ny", "ph", "ch", "nineq", "neq_user")] +
                [(n, C.c_char_p) for n in ("preamble", "state_fn", "objective_fn", "ineq_fn", "eq_fn", "output_fn")])

_lib = None


class MpcxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mpcx error {code}: {msg}")
        self.code = code


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  libmpc_amd has no CPU fallback.")
        # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be in the process first so
        # that libmpcx.so binds to the same HIP runtime instead of loading a second one.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.mpcx_last_error.restype = C.c_char_p
        _lib.mpcx_version.restype = C.c_char_p
        _lib.mpcx_lmpc_set_scalar_constraint_slice.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _lib.mpcx_lmpc_set_scalar_constraint_index.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_set_soft_constraint_weights.argtypes = [C.c_void_p] * 4
        _lib.mpcx_lmpc_set_soft_constraint_weights_slice.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int]
        _lib.mpcx_lmpc_set_terminal_cost.argtypes = [C.c_void_p] * 4
        _lib.mpcx_lmpc_set_linear_constraints.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _lib.mpcx_lmpc_set_linear_constraints_slice.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int]
        _lib.mpcx_lmpc_set_linear_constraint_weights.argtypes = [C.c_void_p] * 2
        _lib.mpcx_lmpc_set_linear_constraint_weights_slice.argtypes = [C.c_void_p] * 2 + [C.c_int, C.c_int]
        _lib.mpcx_nlmpc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.mpcx_nlmpc_destroy.argtypes = [C.c_void_p]
        _lib.mpcx_lmpc_sensitivity_batch.argtypes = [C.c_void_p] * 3
        _lib.mpcx_lmpc_sensitivity_host.argtypes = [C.c_void_p] * 5
        _lib.mpcx_lmpc_hetero_sensitivity_batch.argtypes = [C.c_void_p] * 4
        _lib.mpcx_lmpc_hetero_gradient_batch.argtypes = [C.c_void_p] * 4
        _lib.mpcx_lmpc_param_sensitivity_batch.argtypes = [C.c_void_p] * 3
        _lib.mpcx_lmpc_param_sens_reserve.argtypes = [C.c_void_p, C.c_int]
        _lib.mpcx_lmpc_param_sensitivity_host.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 7
        _lib.mpcx_lmpc_model_sensitivity_batch.argtypes = [C.c_void_p] * 3
        _lib.mpcx_lmpc_model_sens_reserve.argtypes = [C.c_void_p, C.c_int]
        _lib.mpcx_lmpc_model_sensitivity_host.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 7
        _lib.mpcx_lmpc_graph_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_graph_destroy.argtypes = [C.c_void_p]
        _lib.mpcx_lmpc_loop_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_hetero_loop_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_loop_create_observed.argtypes = [C.c_void_p] * 5
        _lib.mpcx_lmpc_hetero_loop_create_observed.argtypes = [C.c_void_p] * 6
        _lib.mpcx_lmpc_loop_create_offset_free.argtypes = [C.c_void_p] * 5
        _lib.mpcx_lmpc_hetero_loop_create_offset_free.argtypes = [C.c_void_p] * 6
        _lib.mpcx_lmpc_loop_create_offset_free_target.argtypes = [C.c_void_p] * 6
        _lib.mpcx_lmpc_hetero_loop_create_offset_free_target.argtypes = [C.c_void_p] * 7
        _lib.mpcx_target_map_batch.argtypes = [C.c_int] * 6 + [C.c_void_p] * 9
        _lib.mpcx_target_apply_batch.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.mpcx_lmpc_kalman_gain.argtypes = [C.c_void_p] * 6
        _lib.mpcx_lmpc_loop_run.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_loop_destroy.argtypes = [C.c_void_p]
        _lib.mpcx_lmpc_loop_grad_create.argtypes = [C.c_void_p] * 4
        _lib.mpcx_lmpc_loop_grad_run.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_loop_grad_destroy.argtypes = [C.c_void_p]
        _lib.mpcx_lmpc_loop_debug_replay.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_lmpc_loop_debug_tick.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_get_dims.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_evaluate_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
        _lib.mpcx_nlparams_default.restype = None
        for _n in ("mpcx_nlmpc_set_state_bounds_slice", "mpcx_nlmpc_set_input_bounds_slice"):
            getattr(_lib, _n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _lib.mpcx_discretize_batch.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
        _lib.mpcx_dare_batch.argtypes = [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 5
        _lib.mpcx_dare_debug_product.argtypes = [C.c_int]
        _lib.mpcx_lmpc_debug_wave_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.mpcx_lmpc_debug_ws_solve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.mpcx_nlmpc_set_optimizer_parameters.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_solve_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_time_solve_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.mpcx_nlmpc_create_from_source.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        _lib.mpcx_nlmpc_set_input_scale.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_set_state_scale.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_loop_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_loop_run.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_loop_destroy.argtypes = [C.c_void_p]
        _lib.mpcx_nlmpc_loop_debug_replay.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_loop_debug_tick.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_plant_step_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
        _lib.mpcx_nlmpc_loop_create_observed.argtypes = [C.c_void_p] * 5
        _lib.mpcx_nlmpc_ekf_step_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int] + [C.c_void_p] * 4
        _lib.mpcx_comm_get_unique_id.argtypes = [C.c_void_p]
        _lib.mpcx_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.mpcx_comm_destroy.argtypes = [C.c_void_p]
        _lib.mpcx_comm_rank.argtypes = [C.c_void_p]
        _lib.mpcx_comm_world.argtypes = [C.c_void_p]
        _lib.mpcx_allgather_u.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return _lib


def check(rc):
    if rc < 0:
        raise MpcxError(rc, lib().mpcx_last_error().decode())
    return rc
