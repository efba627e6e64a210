"""ctypes binding of libkmanip_hip.so (C ABI: include/kmanip.h).

The north star names cffi for this layer; cffi is not installed in the build image
(`import cffi` -> ModuleNotFoundError), so the stdlib `ctypes` loader is used.
There is NO CPU fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from .model import KModelDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KMANIP_LIB") or os.path.join(_HERE, "libkmanip_hip.so")   # KMANIP_LIB: diagnostic builds only
_lib = None

# every symbol include/kmanip.h declares (tests check the library exports all of them)
EXPORTS = [
    "kmanip_model_desc_size", "kmanip_create", "kmanip_reset", "kmanip_step", "kmanip_step_chunk", "kmanip_get_state",
    "kmanip_set_state", "kmanip_get_episode", "kmanip_set_episode", "kmanip_get_counters", "kmanip_bind_sim_time", "kmanip_bind_applied_force", "kmanip_bind_reward_done_record", "kmanip_select_reward_done_record", "kmanip_observe", "kmanip_forces", "kmanip_kinematics", "kmanip_inverse", "kmanip_forward", "kmanip_kinematics_rows", "kmanip_site_cost", "kmanip_rollout", "kmanip_feedback", "kmanip_feedback_box", "kmanip_transition_fd", "kmanip_param_fd", "kmanip_lqr_backward", "kmanip_lqr_backward_box", "kmanip_adjoint", "kmanip_set_seed", "kmanip_get_diag", "kmanip_timing_summary", "kmanip_enable_timing", "kmanip_ik", "kmanip_ik_eval",
    "kmanip_render_depth", "kmanip_render_rgb", "kmanip_render_rgb_multi", "kmanip_render_labels_multi", "kmanip_render_seg", "kmanip_set_render_links", "kmanip_get_render_links", "kmanip_set_depth_links", "kmanip_get_depth_links", "kmanip_get_camera_poses", "kmanip_render_points", "kmanip_snapshot_render_state", "kmanip_set_render_source", "kmanip_bind_step_depth", "kmanip_scripted_action", "kmanip_sample_action", "kmanip_set_env_params", "kmanip_get_env_params", "kmanip_set_env_param_ranges", "kmanip_set_visual_params", "kmanip_get_visual_params", "kmanip_set_visual_param_ranges",
    "kmanip_get_state_dev", "kmanip_set_state_dev", "kmanip_copy_envs", "kmanip_state_index_errors", "kmanip_num_envs", "kmanip_last_error", "kmanip_version", "kmanip_destroy",
]


# include/kmanip_debug.h: diagnostics, not part of the boundary (product build; the -DKM_PROFILE build adds kmanip_dbg_prof*)
DEBUG_EXPORTS = ["kmanip_dbg_wave_clocks", "kmanip_dbg_math"]

# include/kmanip_debug.h KM_MATH_*: name -> (fn, arguments per row, results per row) of kmanip_dbg_math
MATH_FNS = {"km_sincos": (0, 1, 2), "km_atan2": (1, 2, 1), "km_sqrt": (2, 1, 1), "km_rcp": (3, 1, 1), "frcp": (4, 1, 1), "rsqrt_nr": (5, 1, 1),
            "normalize3_fast": (6, 3, 4), "normalize4_fast": (7, 4, 4), "axis_angle2quat": (8, 4, 4), "mat2quat": (9, 9, 4),
            "sub_quat": (10, 8, 3), "sub_quat_sc": (11, 8, 5), "quat_log_diff": (12, 8, 3)}


class KManipError(RuntimeError):
    pass


class KLinkCapsule(C.Structure):
    """include/kmanip.h KLinkCapsule: one link capsule of kmanip_set_render_links."""
    _fields_ = [("link", C.c_int32), ("label", C.c_int32), ("cam_mask", C.c_uint32), ("pad_", C.c_int32),
                ("p0", C.c_double * 3), ("seg", C.c_double * 3), ("radius", C.c_double)]


class KStateDev(C.Structure):
    """include/kmanip.h KStateDev: DEVICE pointers of kmanip_get_state_dev / kmanip_set_state_dev, NULL = that field is skipped."""
    _fields_ = [("qpos", C.c_void_p), ("qvel", C.c_void_p), ("ctrl", C.c_void_p), ("qacc_warm", C.c_void_p),
                ("step_idx", C.c_void_p), ("episode", C.c_void_p)]


class KForcesDev(C.Structure):
    """include/kmanip.h KForcesDev: DEVICE pointers of kmanip_forces, NULL = that field is skipped."""
    _fields_ = [("qacc", C.c_void_p), ("qfrc_constraint", C.c_void_p), ("qfrc_actuator", C.c_void_p), ("contact_force", C.c_void_p),
                ("contact_bit", C.c_void_p), ("contact_frame", C.c_void_p), ("contact_pos", C.c_void_p), ("contact_dist", C.c_void_p),
                ("contact_mask", C.c_void_p), ("status", C.c_void_p)]


class KKinDev(C.Structure):
    """include/kmanip.h KKinDev: DEVICE pointers of kmanip_kinematics, NULL = that field is skipped."""
    _fields_ = [("link_xpos", C.c_void_p), ("link_xmat", C.c_void_p), ("site_xpos", C.c_void_p), ("site_xmat", C.c_void_p),
                ("site_jacp", C.c_void_p), ("site_jacr", C.c_void_p), ("site_vel", C.c_void_p), ("qM", C.c_void_p),
                ("qfrc_bias", C.c_void_p), ("status", C.c_void_p)]


class KInverseIn(C.Structure):
    """include/kmanip.h KInverseIn: DEVICE pointers of kmanip_inverse's inputs; qpos / qvel NULL = the handle's state."""
    _fields_ = [("qacc", C.c_void_p), ("qpos", C.c_void_p), ("qvel", C.c_void_p)]


class KInverseDev(C.Structure):
    """include/kmanip.h KInverseDev: DEVICE pointers of kmanip_inverse's outputs, NULL = that field is skipped."""
    _fields_ = [("qfrc_inverse", C.c_void_p), ("qfrc_constraint", C.c_void_p), ("contact_force", C.c_void_p),
                ("contact_bit", C.c_void_p), ("contact_mask", C.c_void_p), ("status", C.c_void_p)]


class KForwardIn(C.Structure):
    """include/kmanip.h KForwardIn: DEVICE pointers of kmanip_forward's inputs; env_index NULL = row r is env r, any other field
    NULL = what the named env stores."""
    _fields_ = [("env_index", C.c_void_p), ("qpos", C.c_void_p), ("qvel", C.c_void_p), ("ctrl", C.c_void_p), ("qacc_warm", C.c_void_p),
                ("qfrc_applied", C.c_void_p)]


class KKinRowsIn(C.Structure):
    """include/kmanip.h KKinRowsIn: DEVICE pointers of kmanip_kinematics_rows' inputs (KForwardIn's NULL semantics)."""
    _fields_ = [("env_index", C.c_void_p), ("qpos", C.c_void_p), ("qvel", C.c_void_p)]


class KSiteCostIn(C.Structure):
    """include/kmanip.h KSiteCostIn: DEVICE pointers of kmanip_site_cost's inputs (env_index / qpos: KForwardIn's NULL semantics;
    target_quat NULL: no rotation term) and, per arm, whether its target position rides on the cube."""
    _fields_ = [("env_index", C.c_void_p), ("qpos", C.c_void_p), ("target_pos", C.c_void_p), ("target_quat", C.c_void_p),
                ("weight", C.c_void_p), ("follow_cube", C.c_int32 * 2)]


class KSiteCostDev(C.Structure):
    """include/kmanip.h KSiteCostDev: DEVICE pointers of kmanip_site_cost's outputs, any of them NULL."""
    _fields_ = [("cost", C.c_void_p), ("lx", C.c_void_p), ("lxx", C.c_void_p), ("site_xpos", C.c_void_p), ("resid", C.c_void_p),
                ("status", C.c_void_p)]


class KRolloutIn(C.Structure):
    """include/kmanip.h KRolloutIn: DEVICE pointers of kmanip_rollout's inputs (KForwardIn's NULL semantics) and the two flags that
    say whether ctrl / qfrc_applied are [n, nstep, ..] rows, one per step, or [n, ..] rows held for all steps."""
    _fields_ = [("env_index", C.c_void_p), ("qpos", C.c_void_p), ("qvel", C.c_void_p), ("qacc_warm", C.c_void_p), ("ctrl", C.c_void_p),
                ("qfrc_applied", C.c_void_p), ("ctrl_per_step", C.c_int32), ("frc_per_step", C.c_int32)]


class KRolloutDev(C.Structure):
    """include/kmanip.h KRolloutDev: DEVICE pointers of kmanip_rollout's outputs, any of them NULL."""
    _fields_ = [("qpos", C.c_void_p), ("qvel", C.c_void_p), ("qacc_warm", C.c_void_p), ("contact_mask", C.c_void_p), ("reward", C.c_void_p),
                ("status", C.c_void_p), ("steps_done", C.c_void_p)]


class KFeedbackIn(C.Structure):
    """include/kmanip.h KFeedbackIn: KRolloutIn's fields, then the DEVICE pointers and counts of kmanip_feedback's policy -- the gain
    trajectory of each row, the reference states and the TRANSPOSED gains [ng, T, 2 nv, nu] (T = nstep if gain_per_step else 1)."""
    _fields_ = KRolloutIn._fields_ + [("gain_index", C.c_void_p), ("qpos_ref", C.c_void_p), ("qvel_ref", C.c_void_p), ("gain_t", C.c_void_p),
                                      ("ng", C.c_int32), ("gain_per_step", C.c_int32)]


class KFeedbackDev(C.Structure):
    """include/kmanip.h KFeedbackDev: KRolloutDev's fields, then ctrl [n, nstep, nu], the control that acted during each step."""
    _fields_ = KRolloutDev._fields_ + [("ctrl", C.c_void_p)]


class KFeedbackBoxIn(C.Structure):
    """include/kmanip.h KFeedbackBoxIn: KFeedbackIn's fields, then the DEVICE pointers of the box [ng or 1, nu] that clamps the
    policy's output and the flag that says whether every gain trajectory has its own."""
    _fields_ = KFeedbackIn._fields_ + [("lo", C.c_void_p), ("hi", C.c_void_p), ("box_per_traj", C.c_int32)]


class KTransFdIn(C.Structure):
    """include/kmanip.h KTransFdIn: the DEVICE pointers of KRolloutIn's rows (one step, everything held), the KM_WRT_* mask of the
    differentiated inputs, eps and the offset of the perturbed rows' warm start."""
    _fields_ = KRolloutIn._fields_[:6] + [("wrt", C.c_int32), ("eps", C.c_double), ("warm_offset", C.c_double)]


class KTransFdDev(C.Structure):
    """include/kmanip.h KTransFdDev: DEVICE pointers of kmanip_transition_fd's outputs -- the nominal rows one step on, the transposed
    derivative [n, ncol, 2 nv], the status of every column and the contact masks of its +eps / -eps rows."""
    _fields_ = [("qpos", C.c_void_p), ("qvel", C.c_void_p), ("qacc_warm", C.c_void_p), ("contact_mask", C.c_void_p), ("status", C.c_void_p),
                ("deriv_t", C.c_void_p), ("status_cols", C.c_void_p), ("contact_mask_fd", C.c_void_p)]


class KParamFdIn(C.Structure):
    """include/kmanip.h KParamFdIn: the DEVICE pointers of KRolloutIn's rows, the rows' parameters [n, KM_EP_N] (NULL: the named env's),
    the mask of the differentiated KM_EP_* parameters, their perturbations and the offset of the perturbed rows' warm start."""
    _fields_ = KRolloutIn._fields_[:6] + [("params", C.c_void_p), ("wrt", C.c_int32), ("eps", C.c_double * 4), ("eps_relative", C.c_int32),
                                          ("warm_offset", C.c_double)]


class KParamFdDev(C.Structure):
    """include/kmanip.h KParamFdDev: DEVICE pointers of kmanip_param_fd's outputs -- the transposed derivative [n, npar, 2 nv], the status
    of every column and the contact masks of its + / - rows."""
    _fields_ = [("deriv_t", C.c_void_p), ("status_cols", C.c_void_p), ("contact_mask_fd", C.c_void_p)]


class KLqrIn(C.Structure):
    """include/kmanip.h KLqrIn: DEVICE pointers of kmanip_lqr_backward's inputs -- the transposed step Jacobians with their block
    strides in doubles (0 = dense), the cost's derivatives, shared by the problems or one set each, and the regularisation."""
    _fields_ = [("a_t", C.c_void_p), ("b_t", C.c_void_p), ("a_stride", C.c_int64), ("b_stride", C.c_int64), ("lx", C.c_void_p),
                ("lu", C.c_void_p), ("lxx", C.c_void_p), ("luu", C.c_void_p), ("lxx_per_env", C.c_int32), ("luu_per_env", C.c_int32),
                ("reg", C.c_void_p)]


class KLqrDev(C.Structure):
    """include/kmanip.h KLqrDev: DEVICE pointers of kmanip_lqr_backward's outputs, any of them NULL."""
    _fields_ = [("k", C.c_void_p), ("gain_t", C.c_void_p), ("dv", C.c_void_p), ("status", C.c_void_p), ("fail_step", C.c_void_p)]


class KLqrBoxIn(C.Structure):
    """include/kmanip.h KLqrBoxIn: KLqrIn, then the DEVICE pointers of the nominal controls [n, T, nu] and of the box [n or 1, nu]."""
    _fields_ = [("lqr", KLqrIn), ("u", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p), ("box_per_env", C.c_int32)]


class KLqrBoxDev(C.Structure):
    """include/kmanip.h KLqrBoxDev: KLqrDev, then the clamped-set masks [n, T] uint32 and the QP's step counts [n, T] int32."""
    _fields_ = [("lqr", KLqrDev), ("clamped", C.c_void_p), ("qp_iters", C.c_void_p)]


class KAdjointIn(C.Structure):
    """include/kmanip.h KAdjointIn: DEVICE pointers of kmanip_adjoint's inputs -- KLqrIn's transposed step Jacobians and strides, the
    loss's direct partials gx [n m, T + 1, nx] and gu [n m, T, nu] (NULL: zeros), and the transposed gains [n, T, nx, nu] (NULL: open loop)."""
    _fields_ = [("a_t", C.c_void_p), ("b_t", C.c_void_p), ("a_stride", C.c_int64), ("b_stride", C.c_int64), ("gx", C.c_void_p),
                ("gu", C.c_void_p), ("gain_t", C.c_void_p)]


class KAdjointDev(C.Structure):
    """include/kmanip.h KAdjointDev: DEVICE pointers of kmanip_adjoint's outputs lam [n m, T + 1, nx] and mu [n m, T, nu], either NULL."""
    _fields_ = [("lam", C.c_void_p), ("mu", C.c_void_p)]


KM_WRT = {"qpos": 1, "qvel": 2, "ctrl": 4, "qfrc_applied": 8}     # include/kmanip.h KM_WRT_*: the columns always run in this order
KM_MAX_LINK_CAPSULES = 24
KM_COPY_EPISODE, KM_COPY_ENV_PARAMS = 1, 2       # include/kmanip.h: flags of kmanip_copy_envs
KM_POINTS_FRAMES = {"camera": 0, "world": 1}     # include/kmanip.h KM_POINTS_CAMERA / KM_POINTS_WORLD


def build(force: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", src_dir, "-s", "-j4"] + (["-B"] if force else [])
    subprocess.check_call(cmd)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KManipError(
            "libkmanip_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'`; "
            "there is no CPU fallback for the simulation path." % LIB_PATH)
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so); this library links against the same SONAME.  Whichever is
    # loaded FIRST serves the whole process, and a process that loaded /opt/rocm's copy first and torch's afterwards ends up with
    # two runtimes, the second of which sees no device ("no ROCm-capable device is detected" from kmanip_create after
    # `build(); smoke()` in one process).  The host side of this package is torch-based anyway: load torch's runtime first.
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001  (a torch-less C caller binds the ABI directly)
        pass
    lib = C.CDLL(LIB_PATH)
    vp, i32p, u8p, f64p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_float)
    lib.kmanip_model_desc_size.restype = C.c_int
    lib.kmanip_create.argtypes = [C.POINTER(KModelDesc), C.c_int, C.c_int, C.c_uint64, C.c_int64, C.POINTER(vp)]
    lib.kmanip_reset.argtypes = [vp, vp, vp, vp]
    lib.kmanip_step.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.kmanip_step_chunk.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.kmanip_get_state.argtypes = [vp, f64p, f64p, f64p, f64p, i32p]
    lib.kmanip_set_state.argtypes = [vp, f64p, f64p, f64p, f64p, i32p]
    lib.kmanip_get_episode.argtypes = [vp, i32p]
    lib.kmanip_set_episode.argtypes = [vp, i32p]
    lib.kmanip_get_counters.argtypes = [vp, vp, vp, vp]
    lib.kmanip_bind_sim_time.argtypes = [vp, vp]
    lib.kmanip_bind_applied_force.argtypes = [vp, vp]
    lib.kmanip_bind_reward_done_record.argtypes = [vp, vp, vp]
    lib.kmanip_select_reward_done_record.argtypes = [vp, C.c_int]
    lib.kmanip_observe.argtypes = [vp, vp, vp, vp]
    lib.kmanip_forces.argtypes = [vp, C.POINTER(KForcesDev), vp]
    lib.kmanip_kinematics.argtypes = [vp, C.POINTER(KKinDev), vp]
    lib.kmanip_inverse.argtypes = [vp, C.POINTER(KInverseIn), C.POINTER(KInverseDev), vp]
    lib.kmanip_forward.argtypes = [vp, C.POINTER(KForwardIn), C.c_int, C.POINTER(KForcesDev), vp]
    lib.kmanip_kinematics_rows.argtypes = [vp, C.POINTER(KKinRowsIn), C.c_int, C.POINTER(KKinDev), vp]
    lib.kmanip_site_cost.argtypes = [vp, C.POINTER(KSiteCostIn), C.c_int, C.POINTER(KSiteCostDev), vp]
    lib.kmanip_rollout.argtypes = [vp, C.POINTER(KRolloutIn), C.c_int, C.c_int, C.c_int, C.POINTER(KRolloutDev), vp]
    lib.kmanip_feedback.argtypes = [vp, C.POINTER(KFeedbackIn), C.c_int, C.c_int, C.c_int, C.POINTER(KFeedbackDev), vp]
    lib.kmanip_feedback_box.argtypes = [vp, C.POINTER(KFeedbackBoxIn), C.c_int, C.c_int, C.c_int, C.POINTER(KFeedbackDev), vp]
    lib.kmanip_transition_fd.argtypes = [vp, C.POINTER(KTransFdIn), C.c_int, C.c_int, C.POINTER(KTransFdDev), vp]
    lib.kmanip_param_fd.argtypes = [vp, C.POINTER(KParamFdIn), C.c_int, C.c_int, C.POINTER(KParamFdDev), vp]
    lib.kmanip_lqr_backward.argtypes = [vp, C.POINTER(KLqrIn), C.c_int, C.c_int, C.POINTER(KLqrDev), vp]
    lib.kmanip_lqr_backward_box.argtypes = [vp, C.POINTER(KLqrBoxIn), C.c_int, C.c_int, C.POINTER(KLqrBoxDev), vp]
    lib.kmanip_adjoint.argtypes = [vp, C.POINTER(KAdjointIn), C.c_int, C.c_int, C.c_int, C.POINTER(KAdjointDev), vp]
    lib.kmanip_set_seed.argtypes = [vp, C.c_uint64, C.c_int]
    lib.kmanip_get_diag.argtypes = [vp, C.POINTER(C.c_uint32), i32p, i32p]
    lib.kmanip_timing_summary.argtypes = [vp, f64p, f64p, f64p, i32p]
    lib.kmanip_enable_timing.argtypes = [vp, C.c_int]
    lib.kmanip_ik.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, f64p, f64p, i32p, i32p]
    lib.kmanip_ik_eval.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, f64p, f64p, f64p]
    lib.kmanip_render_depth.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.kmanip_render_rgb.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.kmanip_render_rgb_multi.argtypes = [vp, C.c_int, i32p, i32p, i32p, C.POINTER(vp), vp]
    lib.kmanip_render_labels_multi.argtypes = [vp, C.c_int, i32p, i32p, i32p, C.POINTER(vp), C.POINTER(vp), vp]
    lib.kmanip_render_seg.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.kmanip_set_render_links.argtypes = [vp, C.c_int, C.POINTER(KLinkCapsule)]
    lib.kmanip_get_render_links.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(KLinkCapsule)]
    lib.kmanip_set_depth_links.argtypes = [vp, C.c_int]
    lib.kmanip_get_depth_links.argtypes = [vp, C.POINTER(C.c_int)]
    lib.kmanip_get_camera_poses.argtypes = [vp, C.c_int, vp, vp]
    lib.kmanip_render_points.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.kmanip_snapshot_render_state.argtypes = [vp, C.c_int, vp]
    lib.kmanip_set_render_source.argtypes = [vp, C.c_int]
    lib.kmanip_bind_step_depth.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.kmanip_scripted_action.argtypes = [vp, vp, vp]
    lib.kmanip_sample_action.argtypes = [vp, vp, C.c_int, vp]
    lib.kmanip_set_env_params.argtypes = [vp, vp, vp]
    lib.kmanip_get_env_params.argtypes = [vp, vp, vp]
    lib.kmanip_set_env_param_ranges.argtypes = [vp, f64p, f64p]
    lib.kmanip_set_visual_params.argtypes = [vp, vp, vp]
    lib.kmanip_get_visual_params.argtypes = [vp, vp, vp]
    lib.kmanip_set_visual_param_ranges.argtypes = [vp, f64p, f64p]
    lib.kmanip_get_state_dev.argtypes = [vp, vp, C.c_int, C.POINTER(KStateDev), vp]
    lib.kmanip_set_state_dev.argtypes = [vp, vp, C.c_int, C.POINTER(KStateDev), vp]
    lib.kmanip_copy_envs.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint, vp]
    lib.kmanip_state_index_errors.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.kmanip_num_envs.argtypes = [vp]
    lib.kmanip_last_error.argtypes = [vp]
    lib.kmanip_last_error.restype = C.c_char_p
    lib.kmanip_version.restype = C.c_char_p
    lib.kmanip_destroy.argtypes = [vp]
    lib.kmanip_destroy.restype = None
    lib.kmanip_dbg_wave_clocks.argtypes = [vp, C.POINTER(C.c_ulonglong), i32p, i32p]
    lib.kmanip_dbg_math.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp]
    if lib.kmanip_model_desc_size() != C.sizeof(KModelDesc):
        raise KManipError("KModelDesc layout mismatch: lib %d vs python %d"
                          % (lib.kmanip_model_desc_size(), C.sizeof(KModelDesc)))
    _lib = lib
    return lib
