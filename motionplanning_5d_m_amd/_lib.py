"""ctypes binding of libcfs_hip.so (the C ABI of include/cfs_hip.h).

There is no CPU fallback: if the HIP library is missing this module raises at import of the
symbols, and without a GPU every compute entry point returns CFS_ERR_NO_DEVICE, which
``check()`` turns into ``CfsError``.

``torch`` (when importable) is imported BEFORE the library is loaded so that the process holds
one HIP runtime (both resolve the SONAME libamdhip64.so.7; see DESIGN.md "Process layout").
"""
from __future__ import annotations

import ctypes as C
import os

try:  # plumbing only: device memory, streams, torch.distributed
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the host-pointer entry points
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcfs_hip.so")

CFS_MAX_LINKS = 8
CFS_MAX_OBS = 32
CFS_MAX_H = 64

CFS_SUCCESS = 0
ERRORS = {-1: "CFS_ERR_INVALID_ARG", -2: "CFS_ERR_NO_DEVICE", -3: "CFS_ERR_HIP", -4: "CFS_ERR_NOT_SPD",
          -5: "CFS_ERR_DYNAMICS", -6: "CFS_ERR_ALLOC"}
STATUS = {0: "OK_CONVERGED", 1: "OK_MAXITER", 2: "QP_INFEASIBLE", 3: "NUMERIC", 4: "SOFT_ENDED"}
ROBOT_KIND = {"M16iB": 0, "M200i": 1, "2L": 2}
MODE = {"CFS": 0, "PSGCFS": 1}
JACOBIAN = {"fd_literal": 0, "analytic": 1}   # cfs_jacobian_mode
INFEASIBLE = {"stop": 0, "soften": 1}          # cfs_infeasible_policy
OBSTACLES = {"static": 0, "per_waypoint": 1}    # cfs_obstacle_motion
IK_STATUS = {0: "SOLVED", 1: "NOT_CONVERGED", 2: "IN_COLLISION"}                       # cfs_ik_out.status
IK_CAND_STATUS = {0: "CONVERGED", 1: "MAX_ITER", 2: "IN_COLLISION", 3: "NUMERIC"}      # cfs_ik_out.cand_status
CART_STATUS = {0: "SOLVED", 1: "NO_COMPLETE_LINE", 2: "NO_START"}                      # cfs_cart_out.status
CART_CAND_STATUS = {0: "COMPLETE", 1: "MAX_ITER", 2: "IN_COLLISION", 3: "NUMERIC", 4: "JOINT_JUMP", 5: "NO_START"}   # cfs_cart_out.cand_status
TIME_STATUS = {0: "TIMED", 1: "NOT_TIMED", 2: "NUMERIC", 3: "STALLED", 4: "REPEATED_ROW"}                            # cfs_time_out.status
PATH_AUDIT_STATUS = {0: "AUDITED", 1: "NOT_AUDITED", 2: "NUMERIC"}                                                    # cfs_audit_out.status
# cfs_audit_out.state_out: cfs_cart_out.cand_status, then what the audit adds
PATH_AUDIT_STATE = {**CART_CAND_STATUS, 6: "CLEARANCE_NOT_CERTIFIED", 7: "CHORD_NOT_CERTIFIED"}


class CfsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class cfs_robot(C.Structure):
    _fields_ = [
        ("kind", C.c_int),
        ("nlink", C.c_int),
        ("DH", C.c_double * (CFS_MAX_LINKS * 4)),
        ("base", C.c_double * 3),
        ("cap", C.c_double * (CFS_MAX_LINKS * 6)),
        ("T", C.c_double * 9),
        ("delta_t", C.c_double),
    ]


class cfs_problem_desc(C.Structure):
    _fields_ = [
        ("robot", cfs_robot),
        ("mode", C.c_int),
        ("H", C.c_int),
        ("njoint", C.c_int),
        ("nobs", C.c_int),
        ("QQ", C.c_void_p),
        ("Aaug", C.c_void_p),
        ("Baug", C.c_void_p),
        ("lim", C.c_void_p),
        ("MAX_input", C.c_void_p),
        ("margin", C.c_void_p),
        ("epsilon_O", C.c_double),
        ("MAX_O_ITER", C.c_int),
        ("alpha", C.c_double),
        ("max_batch", C.c_int),
    ]


class cfs_cost_weights(C.Structure):
    _fields_ = [
        ("Qp", C.c_void_p),
        ("Qv", C.c_void_p),
        ("q_cross", C.c_double),
        ("w_stage", C.c_double),
        ("w_terminal", C.c_double),
        ("Rblk", C.c_void_p),
        ("cR", C.c_double),
    ]


class cfs_batch_in(C.Structure):
    _fields_ = [
        ("B", C.c_int),
        ("x_init", C.c_void_p),
        ("xR1", C.c_void_p),
        ("ff", C.c_void_p),
        ("caug", C.c_void_p),
        ("obs", C.c_void_p),
        ("noise", C.c_void_p),
        ("noise_rows", C.c_int),
    ]


class cfs_batch_out(C.Structure):
    _fields_ = [
        ("u", C.c_void_p),
        ("x_", C.c_void_p),
        ("cost_all", C.c_void_p),
        ("e_cost_all", C.c_void_p),
        ("e_u_all", C.c_void_p),
        ("iter_O", C.c_void_p),
        ("total_iter", C.c_void_p),
        ("status", C.c_void_p),
    ]


class cfs_rrt_desc(C.Structure):
    _fields_ = [
        ("robot", cfs_robot),
        ("nstate", C.c_int),
        ("solver", C.c_int),
        ("max_iter", C.c_int),
        ("bi", C.c_double),
        ("rewire", C.c_double),
        ("per_tree", C.c_int),
        ("x0", C.c_void_p),
        ("goal", C.c_void_p),
        ("goal_th", C.c_void_p),
        ("region_g", C.c_void_p),
        ("region_s", C.c_void_p),
        ("sample_off", C.c_void_p),
        ("ratial", C.c_void_p),
        ("nobs", C.c_int),
        ("obs", C.c_void_p),
        ("D", C.c_void_p),
        ("uniforms", C.c_void_p),
        ("ndraw", C.c_int),
        ("seed", C.c_ulonglong),
        ("max_draws", C.c_longlong),
    ]


class cfs_rrt_out(C.Structure):
    _fields_ = [
        ("node_num", C.c_void_p),
        ("fail", C.c_void_p),
        ("parent", C.c_void_p),
        ("nodes", C.c_void_p),
        ("total_dis", C.c_void_p),
        ("all_ee", C.c_void_p),
        ("route_len", C.c_void_p),
        ("route", C.c_void_p),
        ("draws_used", C.c_void_p),
        ("proposals", C.c_void_p),
    ]


class cfs_ik_desc(C.Structure):
    _fields_ = [
        ("robot", cfs_robot),
        ("njoint", C.c_int),
        ("tool", C.c_double * 3),
        ("tool_axis", C.c_double * 3),
        ("use_axis", C.c_int),
        ("lo", C.c_void_p),
        ("hi", C.c_void_p),
        ("weight", C.c_void_p),
        ("restarts", C.c_int),
        ("max_iter", C.c_int),
        ("tol_pos", C.c_double),
        ("tol_axis", C.c_double),
        ("nobs", C.c_int),
        ("obs", C.c_void_p),
        ("D", C.c_void_p),
        ("seed", C.c_ulonglong),
    ]


class cfs_ik_out(C.Structure):
    _fields_ = [
        ("theta", C.c_void_p),
        ("status", C.c_void_p),
        ("selected", C.c_void_p),
        ("n_ok", C.c_void_p),
        ("err_pos", C.c_void_p),
        ("err_axis", C.c_void_p),
        ("clearance", C.c_void_p),
        ("cand_theta", C.c_void_p),
        ("cand_status", C.c_void_p),
        ("cand_iter", C.c_void_p),
    ]


class cfs_cart_desc(C.Structure):
    _fields_ = [
        ("robot", cfs_robot),
        ("njoint", C.c_int),
        ("tool", C.c_double * 3),
        ("tool_axis", C.c_double * 3),
        ("use_axis", C.c_int),
        ("lo", C.c_void_p),
        ("hi", C.c_void_p),
        ("weight", C.c_void_p),
        ("candidates", C.c_int),
        ("steps", C.c_int),
        ("max_iter", C.c_int),
        ("max_joint_step", C.c_double),
        ("tol_pos", C.c_double),
        ("tol_axis", C.c_double),
        ("nobs", C.c_int),
        ("obs", C.c_void_p),
        ("D", C.c_void_p),
    ]


class cfs_cart_out(C.Structure):
    _fields_ = [
        ("theta", C.c_void_p),
        ("status", C.c_void_p),
        ("path", C.c_void_p),
        ("selected", C.c_void_p),
        ("n_ok", C.c_void_p),
        ("n_done", C.c_void_p),
        ("clearance", C.c_void_p),
        ("cand_status", C.c_void_p),
        ("cand_done", C.c_void_p),
        ("cand_iter", C.c_void_p),
        ("cand_end", C.c_void_p),
        ("cand_path", C.c_void_p),
    ]


class cfs_time_desc(C.Structure):
    _fields_ = [
        ("robot", cfs_robot),
        ("njoint", C.c_int),
        ("tool", C.c_double * 3),
        ("vmax", C.c_void_p),
        ("amax", C.c_void_p),
        ("feed", C.c_double),
        ("curve_share", C.c_double),
        ("stop_every", C.c_int),
    ]


class cfs_time_out(C.Structure):
    _fields_ = [
        ("time", C.c_void_p),
        ("sdot", C.c_void_p),
        ("duration", C.c_void_p),
        ("status", C.c_void_p),
        ("selected", C.c_void_p),
        ("group_status", C.c_void_p),
    ]


class cfs_audit_desc(C.Structure):
    _fields_ = [
        ("robot", cfs_robot),
        ("njoint", C.c_int),
        ("tool", C.c_double * 3),
        ("nobs", C.c_int),
        ("obs", C.c_void_p),
        ("D", C.c_void_p),
        ("substeps", C.c_int),
        ("min_clearance", C.c_double),
        ("max_chord", C.c_double),
    ]


class cfs_audit_out(C.Structure):
    _fields_ = [
        ("clear_rows", C.c_void_p),
        ("clear_path", C.c_void_p),
        ("s_path", C.c_void_p),
        ("clear_lower", C.c_void_p),
        ("chord_err", C.c_void_p),
        ("chord_upper", C.c_void_p),
        ("link_path", C.c_void_p),
        ("obs_path", C.c_void_p),
        ("status", C.c_void_p),
        ("state_out", C.c_void_p),
    ]


# every symbol include/cfs_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("cfs_abi_version", C.c_int, []),
    ("cfs_last_error", C.c_char_p, []),
    ("cfs_device_count", C.c_int, []),
    ("cfs_set_device", C.c_int, [C.c_int]),
    ("cfs_problem_create", C.c_int, [C.POINTER(cfs_problem_desc), C.POINTER(_P)]),
    ("cfs_problem_destroy", None, [_P]),
    ("cfs_problem_create_from_weights", C.c_int, [C.POINTER(cfs_problem_desc), C.POINTER(cfs_cost_weights), C.POINTER(_P)]),
    ("cfs_problem_family", C.c_int, [_P, _P, C.POINTER(C.c_double)]),
    ("cfs_set_launch_order", C.c_int, [_P, _P, C.c_int]),
    ("cfs_solve_batch", C.c_int, [_P, C.POINTER(cfs_batch_in), C.POINTER(cfs_batch_out)]),
    ("cfs_solve_batch_device", C.c_int, [_P, C.POINTER(cfs_batch_in), C.POINTER(cfs_batch_out), _P]),
    ("cfs_set_state_cost", C.c_int, [_P, _P]),
    ("cfs_build_terms_device", C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_build_terms_from_routes_device", C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P]),
    ("cfs_profile_enable", C.c_int, [_P, C.c_int]),
    ("cfs_profile_read", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("cfs_dist_arm", C.c_int, [C.POINTER(cfs_robot), C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    ("cfs_linearize", C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    ("cfs_get_con", C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("cfs_qp", C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_mesh_create", C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(_P)]),
    ("cfs_mesh_load_stl", C.c_int, [C.c_char_p, C.c_double, C.c_int, C.POINTER(_P)]),
    ("cfs_mesh_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("cfs_mesh_destroy", None, [_P]),
    ("cfs_mesh_segment_distance", C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    ("cfs_dist_arm_mesh", C.c_int, [C.POINTER(cfs_robot), C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    ("cfs_problem_set_meshes", C.c_int, [_P, C.c_int, _P]),
    ("cfs_problem_set_mesh_motion", C.c_int, [_P, _P]),
    ("cfs_chomp_batch", C.c_int, [_P, C.POINTER(cfs_batch_in), _P, _P, _P, C.POINTER(cfs_batch_out)]),
    ("cfs_build_terms_from_ragged_routes_device", C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("cfs_rrt_grow", C.c_int, [C.POINTER(cfs_rrt_desc), C.c_int, C.POINTER(cfs_rrt_out)]),
    ("cfs_rrt_grow_device", C.c_int, [C.POINTER(cfs_rrt_desc), C.c_int, C.POINTER(cfs_rrt_out), _P]),
    ("cfs_rrt_grow_mesh", C.c_int, [C.POINTER(cfs_rrt_desc), C.c_int, _P, _P, C.c_int, C.c_int, C.POINTER(cfs_rrt_out)]),
    ("cfs_rrt_grow_mesh_device", C.c_int, [C.POINTER(cfs_rrt_desc), C.c_int, _P, _P, C.c_int, C.c_int, C.POINTER(cfs_rrt_out), _P]),
    ("cfs_cost_b", C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    ("cfs_get_cost", C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    ("cfs_debug_set_options", C.c_int, [_P, C.c_int, C.c_int, C.c_double]),
    ("cfs_debug_fused_tier", C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_int)]),
    ("cfs_debug_stamps", C.c_int, [_P, C.c_int, _P]),
    ("cfs_debug_trace_begin", C.c_int, [_P, C.c_int, C.c_int]),
    ("cfs_debug_trace_read", C.c_int, [_P, _P]),
    ("cfs_debug_launch_order", C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    ("cfs_debug_log_u", C.c_int, [_P, C.c_int]),
    ("cfs_debug_read_u_log", C.c_int, [_P, C.c_int, _P]),
    ("cfs_debug_rrt_frontier_overflows", C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    ("cfs_problem_set_jacobian", C.c_int, [_P, C.c_int]),
    ("cfs_problem_get_jacobian", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("cfs_problem_set_infeasible_policy", C.c_int, [_P, C.c_int, C.c_double]),
    ("cfs_problem_get_infeasible_policy", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("cfs_soft_results", C.c_int, [_P, C.c_int, _P, _P]),
    ("cfs_dist_arm_grad", C.c_int, [C.POINTER(cfs_robot), C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    ("cfs_select_best_device", C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(cfs_batch_out), _P, C.POINTER(cfs_batch_out), _P, _P, _P, _P]),
    ("cfs_problem_set_obstacle_motion", C.c_int, [_P, C.c_int]),
    ("cfs_problem_get_obstacle_motion", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("cfs_problem_set_joint_limits", C.c_int, [_P, _P, _P]),
    ("cfs_problem_get_joint_limits", C.c_int, [_P, C.POINTER(C.c_int), _P, _P]),
    ("cfs_clearance_device", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_clearance", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_clearance_mesh_device", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_clearance_mesh", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_clearance_mesh_motion_device", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_clearance_mesh_motion", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("cfs_ik_solve", C.c_int, [C.POINTER(cfs_ik_desc), C.c_int, _P, _P, _P, C.POINTER(cfs_ik_out)]),
    ("cfs_ik_solve_device", C.c_int, [C.POINTER(cfs_ik_desc), C.c_int, _P, _P, _P, C.POINTER(cfs_ik_out), _P]),
    ("cfs_tool_pose", C.c_int, [C.POINTER(cfs_robot), C.c_int, _P, _P, C.c_int, _P, _P, _P, _P]),
    ("cfs_ik_solve_mesh", C.c_int, [C.POINTER(cfs_ik_desc), C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(cfs_ik_out)]),
    ("cfs_ik_solve_mesh_device", C.c_int, [C.POINTER(cfs_ik_desc), C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(cfs_ik_out), _P]),
    ("cfs_debug_ik_frontier_overflows", C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    ("cfs_cart_path", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, _P, _P, _P, _P, _P, C.POINTER(cfs_cart_out)]),
    ("cfs_cart_path_device", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, _P, _P, _P, _P, _P, C.POINTER(cfs_cart_out), _P]),
    ("cfs_cart_path_mesh", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(cfs_cart_out)]),
    ("cfs_cart_path_mesh_device", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(cfs_cart_out),
                                            _P]),
    ("cfs_debug_cart_frontier_overflows", C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    ("cfs_debug_mesh_segment_distance_contracted", C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    ("cfs_cart_follow", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(cfs_cart_out)]),
    ("cfs_cart_follow_device", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(cfs_cart_out), _P]),
    ("cfs_cart_follow_mesh", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P,
                                       C.POINTER(cfs_cart_out)]),
    ("cfs_cart_follow_mesh_device", C.c_int, [C.POINTER(cfs_cart_desc), C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P,
                                              C.POINTER(cfs_cart_out), _P]),
    ("cfs_path_time", C.c_int, [C.POINTER(cfs_time_desc), C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(cfs_time_out)]),
    ("cfs_path_time_device", C.c_int, [C.POINTER(cfs_time_desc), C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(cfs_time_out), _P]),
    ("cfs_path_audit", C.c_int, [C.POINTER(cfs_audit_desc), C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(cfs_audit_out)]),
    ("cfs_path_audit_device", C.c_int, [C.POINTER(cfs_audit_desc), C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(cfs_audit_out), _P]),
]

# cfs_debug_set_options mask bits (include/cfs_hip.h)
DBG = {"no_refine": 2, "no_warm_start": 8, "no_certificate": 16, "no_prune": 32, "no_auto_order": 64, "tier_w1": 128,
       "clear_no_bound": 256, "clear_seed": 512}

# cfs_rrt_grow_mesh* flags (include/cfs_hip.h): developer switches, bit-identical trees under every value
RRT_MESH = {"per_lane": 1, "wave": 2, "small_frontier": 4}
# cfs_ik_solve_mesh* flags: the same switches with the same values (IKSolver's mesh_variant)
IK_MESH = {"per_lane": 1, "wave": 2, "small_frontier": 4}

_lib = None


def lib():
    """Load libcfs_hip.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C motionplanning_5d_m_amd/csrc)")
        h = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(h, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc: int) -> None:
    if rc != CFS_SUCCESS:
        raise CfsError(rc, lib().cfs_last_error().decode(errors="replace"))


def device_count() -> int:
    return int(lib().cfs_device_count())
