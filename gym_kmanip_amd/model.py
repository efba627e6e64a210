"""Host-side model compiler: asset JSON + env config -> KModelDesc (include/kmanip.h).

Mirrors what `env_sim.new(gym_env)` reads from the gym env (reference env_sim.py:26-27,45,
50-51,76-77,112,140,154,208-209: mjcf_filename, q_len, q_pos_home, q_id_r_mask, q_id_l_mask,
ctrl_id_r_grip, ctrl_id_l_grip, obs_list, act_list) and the module constants of
gym_kmanip/__init__.py:28-41,164-208.  No reference file is read at run time: the tree comes
from the build-owned JSON written by tools/mjcf_extract.py.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

ASSETS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")

KM_MAX_LINKS = 20
KM_MAX_ARMS = 2
KM_MAX_IK = 7
KM_MAX_SPHERES = 12
KM_MAX_CAMS = 4
KM_CAM_INDEX = {"grip_r": 0, "grip_l": 1, "top": 2, "head": 3}


class Cam:
    """gym_kmanip/__init__.py:143-161: image size / channels / value range of one camera (fl, pp are logging metadata there)."""

    def __init__(self, w, h, name, fl=0, pp=(0, 0)):
        self.w, self.h, self.c, self.name, self.log_name = w, h, 3, name, "camera/" + name
        self.fl, self.pp = fl, tuple(pp)
        self.low, self.high, self.dtype = 0, 255, np.uint8

    def __repr__(self):
        return "Cam(%s %dx%d)" % (self.name, self.w, self.h)


CAMERAS = {"head": Cam(640, 480, "head", 448, (320, 240)), "top": Cam(640, 480, "top", 448, (320, 240)),
           "grip_r": Cam(60, 40, "grip_r", 45, (30, 20)), "grip_l": Cam(60, 40, "grip_l", 45, (30, 20))}
KM_ACT_KEYS = ["eel_pos", "eel_orn", "eer_pos", "eer_orn", "grip_l", "grip_r", "q_pos_r", "q_pos_l"]
KM_DONE_TRUNCATED = 1
KM_DONE_DIVERGED = 2

# ---- constants of gym_kmanip/__init__.py (values restated; line numbers cite the reference)
MAX_EPISODE_STEPS = 64          # :28
CONTROL_TIMESTEP = 0.02         # :30
MAX_Q_VEL = math.pi             # :31
CTRL_ALPHA = 1.0                # :34 (identity filter; folded away)
IK_RES_RAD = 0.02               # :37
IK_RES_REG_PREV = 6e-3          # :38
IK_RES_REG_HOME = 2e-6          # :39
IK_JAC_RAD = 0.02               # :40
IK_JAC_REG = 9e-3               # :41
CUBE_SPAWN_RANGE = np.array([[0.1, 0.3], [0.5, 0.7], [0.6, 0.7]])  # :164-170
EE_POS_DELTA = [0.01, 0.01, 0.01]   # :174-180
EE_ORN_DELTA = [0.1, 0.1, 0.1]      # :181-187
EPSILON = 1e-6                  # :192
Q_POS_DELTA = 0.1               # :196
EE_S_MIN = -0.029               # :199
EE_S_MAX = 0.005                # :200
EE_S_DELTA = 0.0001             # :201
REWARD_SUCCESS_THRESHOLD = 2.0  # :204
REWARD_VEL_PENALTY = 0.01       # :205
REWARD_GRIP_DIST = 0.01         # :206
REWARD_TOUCH_CUBE = 1.0         # :207
REWARD_LIFT_CUBE = 1.0          # :208

# MuJoCo defaults (no <option>/<default> element exists in any reference XML)
MJ_TIMESTEP = 0.002
MJ_DEFAULT_SOLREF = [0.02, 1.0]
MJ_DEFAULT_SOLIMP = [0.9, 0.95, 0.001, 0.5, 2.0]
MJ_DEFAULT_FRICTION = [1.0, 0.005, 0.0001]

# ---- home poses, __init__.py:53-122 (float32 like ACT_DTYPE there)
Q_SOLO_ARM_HOME = np.array([0.0, 0.75, 1.0, 1.0, 2.0, -2.0, 0.0, 0.0, 0.005, 0.005], dtype=np.float32)
Q_DUAL_ARM_HOME = np.array([0.0, 0.75, 1.0, 1.0, 2.0, -2.7, 0.0, 0.0, 0.005, 0.005,
                            0.0, -0.75, -1.0, -1.0, 2.0, 0.0, 0.0, 0.0, 0.005, 0.005], dtype=np.float32)
Q_TORSO_HOME = np.array([-1.0, 0.0, 1.7, 1.6, 0.34, 1.6, 1.4, -0.26, 0.0, 0.0, 0.0,
                         -1.7, -1.6, -0.34, -1.6, -1.4, -1.7, 0.0, 0.0, 0.0], dtype=np.float32)

OBS_STATE = ["q_pos", "q_vel", "cube_pos", "cube_orn"]


@dataclass
class EnvSpec:
    """kwargs of one `gym.register` call, gym_kmanip/__init__.py:244-483."""
    env_id: str
    asset: str
    obs_list: List[str]
    act_list: List[str]
    q_pos_home: np.ndarray
    q_id_r_mask: Optional[List[int]] = None
    q_id_l_mask: Optional[List[int]] = None
    ctrl_id_r_grip: Optional[List[int]] = None
    ctrl_id_l_grip: Optional[List[int]] = None
    max_episode_steps: int = MAX_EPISODE_STEPS


_SOLO = dict(asset="solo_arm", q_pos_home=Q_SOLO_ARM_HOME, q_id_r_mask=[0, 1, 2, 3, 4, 5, 6],
             ctrl_id_r_grip=[8, 9])
_DUAL = dict(asset="dual_arm", q_pos_home=Q_DUAL_ARM_HOME, q_id_r_mask=[0, 1, 2, 3, 4, 5, 6],
             q_id_l_mask=[10, 11, 12, 13, 14, 15, 16], ctrl_id_r_grip=[8, 9], ctrl_id_l_grip=[18, 19])
_TORSO = dict(asset="torso", q_pos_home=Q_TORSO_HOME, q_id_r_mask=[2, 3, 4, 5, 6, 7],
              q_id_l_mask=[11, 12, 13, 14, 15, 16], ctrl_id_r_grip=[8, 9], ctrl_id_l_grip=[17, 18])
_ACT_SOLO = ["eer_pos", "eer_orn", "grip_r"]
_ACT_BOTH = ["eel_pos", "eel_orn", "eer_pos", "eer_orn", "grip_l", "grip_r"]

ENV_SPECS: Dict[str, EnvSpec] = {
    "KManipSoloArm": EnvSpec("KManipSoloArm", obs_list=OBS_STATE, act_list=_ACT_SOLO, **_SOLO),
    "KManipSoloArmQPos": EnvSpec("KManipSoloArmQPos", obs_list=OBS_STATE, act_list=["q_pos_r", "grip_r"], **_SOLO),
    "KManipSoloArmVision": EnvSpec("KManipSoloArmVision", obs_list=["q_pos", "q_vel", "camera/head", "camera/grip_r"],
                                   act_list=_ACT_SOLO, **_SOLO),
    "KManipDualArm": EnvSpec("KManipDualArm", obs_list=OBS_STATE, act_list=_ACT_BOTH, **_DUAL),
    "KManipDualArmQPos": EnvSpec("KManipDualArmQPos", obs_list=OBS_STATE,
                                 act_list=["q_pos_r", "q_pos_l", "grip_l", "grip_r"], **_DUAL),
    "KManipDualArmVision": EnvSpec("KManipDualArmVision",
                                   obs_list=["q_pos", "q_vel", "camera/head", "camera/grip_l", "camera/grip_r"],
                                   act_list=_ACT_BOTH, **_DUAL),
    "KManipTorso": EnvSpec("KManipTorso", obs_list=OBS_STATE, act_list=_ACT_BOTH, **_TORSO),
    "KManipTorsoVision": EnvSpec("KManipTorsoVision",
                                 obs_list=["q_pos", "q_vel", "camera/head", "camera/grip_l", "camera/grip_r"],
                                 act_list=_ACT_BOTH, **_TORSO),
}


class KModelDesc(C.Structure):
    """ctypes mirror of `struct KModelDesc` in include/kmanip.h (field order matters)."""
    _fields_ = [
        ("nlink", C.c_int32), ("narm", C.c_int32), ("nsphere", C.c_int32), ("act_dim", C.c_int32),
        ("obs_dim", C.c_int32), ("max_episode_steps", C.c_int32), ("n_sub_steps", C.c_int32),
        ("solver_iterations", C.c_int32), ("touch_reward_enabled", C.c_int32), ("auto_reset", C.c_int32),
        ("act_col", C.c_int32 * len(KM_ACT_KEYS)), ("solver", C.c_int32), ("ik_max_nfev", C.c_int32), ("pad0_", C.c_int32),
        ("link_parent", C.c_int32 * KM_MAX_LINKS), ("jnt_type", C.c_int32 * KM_MAX_LINKS),
        ("forcelimited", C.c_int32 * KM_MAX_LINKS), ("pad1_", C.c_int32 * KM_MAX_LINKS),
        ("link_pos", (C.c_double * 3) * KM_MAX_LINKS), ("link_quat", (C.c_double * 4) * KM_MAX_LINKS),
        ("jnt_axis", (C.c_double * 3) * KM_MAX_LINKS), ("jnt_range", (C.c_double * 2) * KM_MAX_LINKS),
        ("frictionloss", C.c_double * KM_MAX_LINKS), ("kp", C.c_double * KM_MAX_LINKS),
        ("ctrlrange", (C.c_double * 2) * KM_MAX_LINKS), ("forcerange", (C.c_double * 2) * KM_MAX_LINKS),
        ("mass", C.c_double * KM_MAX_LINKS), ("com", (C.c_double * 3) * KM_MAX_LINKS),
        ("inertia", (C.c_double * 3) * KM_MAX_LINKS), ("q_home", C.c_double * KM_MAX_LINKS),
        ("arm_present", C.c_int32 * KM_MAX_ARMS), ("arm_nq", C.c_int32 * KM_MAX_ARMS),
        ("arm_q_id", (C.c_int32 * (KM_MAX_IK + 1)) * KM_MAX_ARMS), ("arm_grip_id", (C.c_int32 * 2) * KM_MAX_ARMS),
        ("arm_site_link", C.c_int32 * KM_MAX_ARMS), ("arm_mode", C.c_int32 * KM_MAX_ARMS),
        ("arm_has_grip", C.c_int32 * KM_MAX_ARMS), ("pad2_", C.c_int32 * 2),
        ("arm_site_pos", (C.c_double * 3) * KM_MAX_ARMS), ("arm_site_quat", (C.c_double * 4) * KM_MAX_ARMS),
        ("sphere_link", C.c_int32 * KM_MAX_SPHERES), ("sphere_visible", C.c_int32 * KM_MAX_SPHERES), ("sphere_pos", (C.c_double * 3) * KM_MAX_SPHERES),
        ("sphere_radius", C.c_double * KM_MAX_SPHERES), ("sphere_seg", (C.c_double * 3) * KM_MAX_SPHERES), ("table_z", C.c_double), ("table_rect", C.c_double * 4),
        ("cube_mass", C.c_double), ("cube_inertia", C.c_double * 3), ("cube_half", C.c_double * 3),
        ("cube_frictionloss", C.c_double), ("cube_quat0", C.c_double * 4),
        ("cube_spawn_lo", C.c_double * 3), ("cube_spawn_hi", C.c_double * 3),
        ("con_cube_solref", C.c_double * 2), ("con_cube_solimp", C.c_double * 5),
        ("con_cube_friction", C.c_double * 3), ("con_def_solref", C.c_double * 2),
        ("con_def_solimp", C.c_double * 5), ("con_def_friction", C.c_double * 3),
        ("timestep", C.c_double), ("gravity", C.c_double * 3), ("solver_tolerance", C.c_double),
        ("ik_res_rad", C.c_double), ("ik_res_reg_prev", C.c_double), ("ik_res_reg_home", C.c_double),
        ("ik_jac_rad", C.c_double), ("ik_jac_reg", C.c_double),
        ("ee_pos_delta", C.c_double * 3), ("ee_orn_delta", C.c_double * 3), ("q_pos_delta", C.c_double),
        ("ee_s_min", C.c_double), ("ee_s_max", C.c_double), ("ee_s_delta", C.c_double),
        ("max_q_vel", C.c_double), ("epsilon", C.c_double),
        ("reward_vel_penalty", C.c_double), ("reward_grip_dist", C.c_double),
        ("reward_touch_cube", C.c_double), ("reward_lift_cube", C.c_double),
        ("cam_present", C.c_int32 * KM_MAX_CAMS), ("cam_link", C.c_int32 * KM_MAX_CAMS),
        ("cam_target_link", C.c_int32 * KM_MAX_CAMS),
        ("cam_pos", (C.c_double * 3) * KM_MAX_CAMS), ("cam_target_pos", (C.c_double * 3) * KM_MAX_CAMS),
        ("cam_fovy", C.c_double * KM_MAX_CAMS), ("cam_znear", C.c_double), ("cam_zfar", C.c_double),
        ("dof_invweight0", C.c_double * KM_MAX_LINKS), ("body_invweight0", (C.c_double * 2) * KM_MAX_LINKS),
        ("cube_invweight0", C.c_double * 2), ("meaninertia", C.c_double),
    ]


def load_asset(name: str) -> dict:
    with open(os.path.join(ASSETS_DIR, name + ".json")) as f:
        return json.load(f)


def _mix(a, b, n):
    """MuJoCo contact parameter mixing with equal solmix (mix = 0.5)."""
    a = list(a) + list(MJ_DEFAULT_SOLIMP[len(a):n]) if len(a) < n else list(a)
    return [0.5 * x + 0.5 * y for x, y in zip(a[:n], b[:n])]


@dataclass
class CompiledModel:
    spec: EnvSpec
    asset: dict
    desc: KModelDesc
    nlink: int
    nq: int
    nv: int
    nu: int
    act_dim: int
    obs_dim: int
    act_slices: Dict[str, slice] = field(default_factory=dict)
    obs_slices: Dict[str, slice] = field(default_factory=dict)
    cameras: List[str] = field(default_factory=list)


SOLVERS = {"pgs": 0, "newton": 1}


def _quat2mat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def invweight0(d: "KModelDesc"):
    """What MuJoCo's mj_setConst computes at qpos0 (every joint at 0; no `ref`/`springref` in any reference XML) and the
    constraint code then uses for efc_diagApprox and the solver scale -- from the model's own (surrogate) inertias:
      dof_invweight0[i]   = (M^-1)_ii
      body_invweight0[b]  = (mean of the translational, mean of the rotational) diagonal of J_b M^-1 J_b^T, J_b = the
                            6 x nv Jacobian of body b at its centre of mass
      cube (free body)    = (1/m, mean_k 1/I_k); free-joint dof_invweight0 is averaged per 3-dof block the same way
      meaninertia         = trace(M) / nv over all nv = nlink + 6 dofs
    Returns (dofw[nl], bodyw[nl][2], cubew[2], meaninertia)."""
    nl = d.nlink
    xpos = np.zeros((nl, 3)); xmat = np.zeros((nl, 3, 3)); axis = np.zeros((nl, 3)); cpos = np.zeros((nl, 3))
    for i in range(nl):
        p = d.link_parent[i]
        R0 = _quat2mat(list(d.link_quat[i]))
        lp = np.array(list(d.link_pos[i]))
        if p < 0:
            xpos[i], xmat[i] = lp, R0
        else:
            xpos[i], xmat[i] = xpos[p] + xmat[p] @ lp, xmat[p] @ R0          # joint value 0: no joint motion
        axis[i] = xmat[i] @ np.array(list(d.jnt_axis[i]))
        cpos[i] = xpos[i] + xmat[i] @ np.array(list(d.com[i]))
    anc = []
    for i in range(nl):
        a, j = [], i
        while j >= 0:
            a.append(j); j = d.link_parent[j]
        anc.append(a)

    def jac(b, pt):
        J = np.zeros((6, nl))
        for j in anc[b]:
            if d.jnt_type[j] == 1:
                J[:3, j] = axis[j]
            else:
                J[:3, j] = np.cross(axis[j], pt - xpos[j]); J[3:, j] = axis[j]
        return J

    M = np.zeros((nl, nl))
    Js = []
    for b in range(nl):
        J = jac(b, cpos[b]); Js.append(J)
        Iw = xmat[b] @ np.diag(list(d.inertia[b])) @ xmat[b].T
        M += d.mass[b] * J[:3].T @ J[:3] + J[3:].T @ Iw @ J[3:]
    Minv = np.linalg.inv(M)
    dofw = np.diag(Minv).copy()
    bodyw = np.zeros((nl, 2))
    for b in range(nl):
        A = Js[b] @ Minv @ Js[b].T
        bodyw[b] = [np.trace(A[:3, :3]) / 3.0, np.trace(A[3:, 3:]) / 3.0]
    cubew = (1.0 / d.cube_mass, float(np.mean([1.0 / d.cube_inertia[k] for k in range(3)])))
    trace = np.trace(M) + 3 * d.cube_mass + sum(d.cube_inertia[k] for k in range(3))
    return dofw, bodyw, cubew, float(trace / (nl + 6))


def compile_model(env_id_or_spec, *, auto_reset: bool = True, touch_reward: bool = False,
                  solver: str = "newton", solver_iterations: int = 100, solver_tolerance: float = 1e-8,
                  ik_max_nfev: int = 0) -> CompiledModel:
    spec = ENV_SPECS[env_id_or_spec] if isinstance(env_id_or_spec, str) else env_id_or_spec
    asset = load_asset(spec.asset)
    links = asset["links"]
    nl = len(links)
    assert nl <= KM_MAX_LINKS and nl == len(spec.q_pos_home)
    d = KModelDesc()
    d.nlink = nl
    d.max_episode_steps = spec.max_episode_steps
    d.n_sub_steps = int(round(CONTROL_TIMESTEP / MJ_TIMESTEP))
    d.solver = SOLVERS[solver]
    d.solver_iterations = solver_iterations
    d.ik_max_nfev = int(ik_max_nfev)      # 0 = the reference's least_squares default (100 n); > 0: opt-in cap (include/kmanip.h)
    d.solver_tolerance = solver_tolerance
    d.touch_reward_enabled = int(touch_reward)
    d.auto_reset = int(auto_reset)
    for i, l in enumerate(links):
        assert l["parent"] < i
        d.link_parent[i] = l["parent"]
        j = l["joint"]
        d.jnt_type[i] = 1 if j["type"] == "slide" else 0
        assert j["limited"]
        for k in range(3):
            d.link_pos[i][k] = l["pos"][k]
            d.jnt_axis[i][k] = j["axis"][k]
            d.com[i][k] = l["inertial"]["com"][k]
            d.inertia[i][k] = l["inertial"]["diaginertia"][k]
        for k in range(4):
            d.link_quat[i][k] = l["quat"][k]
        d.jnt_range[i][0], d.jnt_range[i][1] = j["range"]
        d.frictionloss[i] = j["frictionloss"]
        a = l["actuator"]
        d.kp[i] = a["kp"]
        d.ctrlrange[i][0], d.ctrlrange[i][1] = a["ctrlrange"]
        if a["forcerange"] is not None:
            d.forcelimited[i] = 1
            d.forcerange[i][0], d.forcerange[i][1] = a["forcerange"]
        d.mass[i] = l["inertial"]["mass"]
        d.q_home[i] = float(np.float32(spec.q_pos_home[i]))

    # ---- action layout: Dict-space insertion order, env_base.py:151-188
    col = 0
    act_slices = {}
    masks = {"q_pos_r": spec.q_id_r_mask, "q_pos_l": spec.q_id_l_mask}
    for k, key in enumerate(KM_ACT_KEYS):
        if key in spec.act_list:
            width = {"grip_l": 1, "grip_r": 1}.get(key, 3)
            if key in masks:
                width = len(masks[key])
            d.act_col[k] = col
            act_slices[key] = slice(col, col + width)
            col += width
        else:
            d.act_col[k] = -1
    d.act_dim = col
    d.obs_dim = 2 * nl + 7

    # ---- arms
    narm = 0
    for arm, (side, mask, grip, site) in enumerate([
            ("r", spec.q_id_r_mask, spec.ctrl_id_r_grip, "eer_site_pos"),
            ("l", spec.q_id_l_mask, spec.ctrl_id_l_grip, "eel_site_pos")]):
        if mask is None:
            continue
        d.arm_present[arm] = 1
        d.arm_nq[arm] = len(mask)
        assert len(mask) <= KM_MAX_IK
        for k, q in enumerate(mask):
            d.arm_q_id[arm][k] = q
        s = asset["sites"][site]
        d.arm_site_link[arm] = s["link"]
        for k in range(3):
            d.arm_site_pos[arm][k] = s["pos"][k]
        for k in range(4):
            d.arm_site_quat[arm][k] = s["quat"][k]
        if ("ee%s_pos" % side) in spec.act_list:
            assert ("ee%s_orn" % side) in spec.act_list
            d.arm_mode[arm] = 1
        elif ("q_pos_%s" % side) in spec.act_list:
            d.arm_mode[arm] = 2
        if ("grip_%s" % side) in spec.act_list:
            d.arm_has_grip[arm] = 1
            d.arm_grip_id[arm][0], d.arm_grip_id[arm][1] = grip
        narm += 1
    d.narm = narm

    # ---- colliders
    sph = asset["spheres"]
    assert len(sph) <= KM_MAX_SPHERES
    d.nsphere = len(sph)
    for i, s in enumerate(sph):
        d.sphere_link[i] = s["link"]
        d.sphere_visible[i] = s.get("visible", 1)
        d.sphere_radius[i] = s["radius"]
        for k in range(3):
            d.sphere_pos[i][k] = s["pos"][k]
            d.sphere_seg[i][k] = s.get("seg", (0.0, 0.0, 0.0))[k]
    d.table_z = asset["table"]["plane_z"]
    for k, v in enumerate(asset["table"].get("rect", (-np.inf, np.inf, -np.inf, np.inf))):    # x_lo, x_hi, y_lo, y_hi of the table top
        d.table_rect[k] = v
    cube = asset["cube"]
    d.cube_mass = cube["mass"]
    d.cube_frictionloss = cube["frictionloss"]
    for k in range(3):
        d.cube_inertia[k] = cube["diaginertia"][k]
        d.cube_half[k] = cube["half_size"][k]
        d.cube_spawn_lo[k] = CUBE_SPAWN_RANGE[k, 0]
        d.cube_spawn_hi[k] = CUBE_SPAWN_RANGE[k, 1]
    for k in range(4):
        d.cube_quat0[k] = cube["quat0"][k]
    assert cube["condim"] == 4
    # pair parameters: condim = max, friction = element-wise max, solref/solimp = equal-weight mix
    for k, v in enumerate(_mix(cube["solref"], MJ_DEFAULT_SOLREF, 2)):
        d.con_cube_solref[k] = v
    for k, v in enumerate(_mix(cube["solimp"], MJ_DEFAULT_SOLIMP, 5)):
        d.con_cube_solimp[k] = v
    for k in range(3):
        d.con_cube_friction[k] = max(cube["friction"][k], MJ_DEFAULT_FRICTION[k])
        d.con_def_friction[k] = MJ_DEFAULT_FRICTION[k]
    for k in range(2):
        d.con_def_solref[k] = MJ_DEFAULT_SOLREF[k]
    for k in range(5):
        d.con_def_solimp[k] = MJ_DEFAULT_SOLIMP[k]

    # ---- options / constants
    d.timestep = asset["option"]["timestep"]
    for k in range(3):
        d.gravity[k] = asset["option"]["gravity"][k]
        d.ee_pos_delta[k] = EE_POS_DELTA[k]
        d.ee_orn_delta[k] = EE_ORN_DELTA[k]
    d.ik_res_rad, d.ik_res_reg_prev, d.ik_res_reg_home = IK_RES_RAD, IK_RES_REG_PREV, IK_RES_REG_HOME
    d.ik_jac_rad, d.ik_jac_reg = IK_JAC_RAD, IK_JAC_REG
    d.q_pos_delta = Q_POS_DELTA
    d.ee_s_min, d.ee_s_max, d.ee_s_delta = EE_S_MIN, EE_S_MAX, EE_S_DELTA
    d.max_q_vel = MAX_Q_VEL
    d.epsilon = EPSILON
    d.reward_vel_penalty, d.reward_grip_dist = REWARD_VEL_PENALTY, REWARD_GRIP_DIST
    d.reward_touch_cube, d.reward_lift_cube = REWARD_TOUCH_CUBE, REWARD_LIFT_CUBE

    # ---- gripper cameras (targetbody mode); znear from scene.xml:5 (<map znear="0.1"/> x extent ~1 m)
    for cname, ci in KM_CAM_INDEX.items():
        cams = [c for c in asset["cameras"] if c["name"] == cname]
        if not cams:
            continue
        cam = cams[0]
        tgt = asset["targets"][cam["target"]]
        d.cam_present[ci] = 1
        d.cam_link[ci] = cam["link"]
        d.cam_target_link[ci] = tgt["link"]
        d.cam_fovy[ci] = cam["fovy"]
        for k in range(3):
            d.cam_pos[ci][k] = cam["pos"][k]
            d.cam_target_pos[ci][k] = tgt["pos"][k]
    d.cam_znear, d.cam_zfar = 0.01, 5.0

    # ---- qpos0-time constants (MuJoCo mj_setConst)
    dofw, bodyw, cubew, meaninertia = invweight0(d)
    for i in range(nl):
        d.dof_invweight0[i] = dofw[i]
        d.body_invweight0[i][0], d.body_invweight0[i][1] = bodyw[i]
    d.cube_invweight0[0], d.cube_invweight0[1] = cubew
    d.meaninertia = meaninertia

    obs_slices = {"q_pos": slice(0, nl), "q_vel": slice(nl, 2 * nl),
                  "cube_pos": slice(2 * nl, 2 * nl + 3), "cube_orn": slice(2 * nl + 3, 2 * nl + 7)}
    cams = [o.split("/")[-1] for o in spec.obs_list if o.startswith("camera/")]
    return CompiledModel(spec=spec, asset=asset, desc=d, nlink=nl, nq=nl + 7, nv=nl + 6, nu=nl,
                         act_dim=col, obs_dim=2 * nl + 7, act_slices=act_slices,
                         obs_slices=obs_slices, cameras=cams)


# ---- per-env physics parameters (include/kmanip.h KM_EP_*), in KM_EP_* order
ENV_PARAMS = ("cube_mass", "cube_friction", "cube_frictionloss", "kp_scale")


def env_param_defaults(cm: CompiledModel) -> Dict[str, float]:
    """The compiled model's own value of every per-env parameter."""
    d = cm.desc
    return {"cube_mass": d.cube_mass, "cube_friction": d.con_cube_friction[0], "cube_frictionloss": d.cube_frictionloss,
            "kp_scale": 1.0}


def check_env_param(name: str, v) -> float:
    """ValueError unless v is a finite value within the parameter's limits (mass and kp scale > 0, friction terms >= 0)."""
    if name not in ENV_PARAMS:
        raise ValueError("unknown env parameter %r (known: %s)" % (name, ", ".join(ENV_PARAMS)))
    v = float(v)
    positive = name in ("cube_mass", "kp_scale")
    if not math.isfinite(v) or (v <= 0 if positive else v < 0):
        raise ValueError("%s = %r: must be finite and %s 0" % (name, v, ">" if positive else ">="))
    return v


def trace_robot(d: "KModelDesc") -> float:
    """Robot part of trace(M(qpos0)) as the library derives it at create (kmanip_api.hip trace_robot_of), same order."""
    return d.meaninertia * float(d.nlink + 6) - (3.0 * d.cube_mass + ((d.cube_inertia[0] + d.cube_inertia[1]) + d.cube_inertia[2]))


def with_env_params(cm: CompiledModel, cube_mass=None, cube_friction=None, cube_frictionloss=None,
                    kp_scale=None) -> CompiledModel:
    """The host definition of the per-env parameters: a copy of `cm` whose desc has the named fields and the constants derived
    from them replaced, in the evaluation order the kernels use (kmanip_dyn.hip ep_derive) -- an env of a handle with
    parameters p behaves exactly like a handle created from with_env_params(cm, **p).desc.
      cube_mass          uniform-density box of unchanged size: cube_inertia[k] * (m / m0); cube_invweight0 = (1/m, mean 1/I_k);
                         meaninertia = (trace_robot + 3 m + (I_0 + I_1 + I_2)) / nv (the compiled value while m == m0)
      cube_friction      con_cube_friction[0] (torsional / rolling unchanged)
      cube_frictionloss  the cube free joint's friction loss
      kp_scale           every position servo's kp times the scale
    Unnamed (None) fields keep the model's values; bad values raise ValueError."""
    d0 = cm.desc
    d = KModelDesc.from_buffer_copy(d0)
    if cube_mass is not None:
        m0, m = d0.cube_mass, check_env_param("cube_mass", cube_mass)
        inertia = [d0.cube_inertia[k] * (m / m0) for k in range(3)]
        d.cube_mass = m
        for k in range(3):
            d.cube_inertia[k] = inertia[k]
        d.cube_invweight0[0] = 1.0 / m
        d.cube_invweight0[1] = ((1.0 / inertia[0] + 1.0 / inertia[1]) + 1.0 / inertia[2]) / 3.0
        if m != m0:
            nv = d0.nlink + 6
            d.meaninertia = ((trace_robot(d0) + 3.0 * m) + ((inertia[0] + inertia[1]) + inertia[2])) / nv
    if cube_friction is not None:
        d.con_cube_friction[0] = check_env_param("cube_friction", cube_friction)
    if cube_frictionloss is not None:
        d.cube_frictionloss = check_env_param("cube_frictionloss", cube_frictionloss)
    if kp_scale is not None:
        s = check_env_param("kp_scale", kp_scale)
        for i in range(d0.nlink):
            d.kp[i] = d0.kp[i] * s
    return dataclasses.replace(cm, desc=d)


def _philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011) on uint32 words, as kmanip_device.hpp philox4x32_10 evaluates it."""
    c0, c1, c2, c3 = (int(x) & 0xFFFFFFFF for x in ctr)
    k0, k1 = (int(x) & 0xFFFFFFFF for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c3 ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.array([c0, c1, c2, c3], dtype=np.uint32)


def _u53(hi, lo):
    return (float(int(hi) >> 5) * 67108864.0 + float(int(lo) >> 6)) / 9007199254740992.0


KM_EP_CTR3 = 2      # include/kmanip.h: counter word 3 of the ranges-mode draw (words 2 and 3; the cube spawn uses 0 and 1)


def draw_env_params(seed: int, genv: int, episode: int, lo, hi) -> np.ndarray:
    """The values ranges mode draws at the reset that starts `episode` of global env `genv` (include/kmanip.h
    kmanip_set_env_param_ranges): p_k = lo_k + (hi_k - lo_k) * u_k, product rounded before the sum, u_k from Philox4x32-10 with
    key = seed and counter (genv lo, genv hi, episode, KM_EP_CTR3 + k // 2), words (0, 1) for even k and (2, 3) for odd k."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    g = int(genv) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros(len(ENV_PARAMS))
    for blk in range(2):
        o = _philox4x32_10((g & 0xFFFFFFFF, g >> 32, int(episode) & 0xFFFFFFFF, KM_EP_CTR3 + blk), key)
        for j in range(2):
            k = 2 * blk + j
            u = _u53(o[2 * j], o[2 * j + 1])
            out[k] = float(lo[k]) + (float(hi[k]) - float(lo[k])) * u
    return out


# ---- per-env visual parameters of the camera renders (include/kmanip.h KM_VP_*)
# name -> (first index in the KM_VP_N values, number of components)
VISUAL_PARAMS = {"cube_rgb": (0, 3), "table_rgb": (3, 3), "robot_rgb": (6, 3), "background_rgb": (9, 3), "ambient": (12, 1),
                 "headlight": (13, 1), "directional": (14, 1), "camera_offset": (15, 3)}
KM_VP_N = 18
KM_VP_CTR3 = 0x100  # include/kmanip.h: counter word 3 of the visual draw is KM_VP_CTR3 + k // 2 (disjoint from spawn, KM_EP_CTR3, actions)
VP_MAX_CAM_OFFSET = 0.25


def visual_param_defaults() -> Dict[str, object]:
    """The values every env renders with when none are set (the default kernels' constants)."""
    return {"cube_rgb": (1.0, 0.0, 0.0), "table_rgb": (0.2, 0.2, 0.2), "robot_rgb": (0.647059, 0.647059, 0.647059),
            "background_rgb": (0.0, 0.0, 0.0), "ambient": 0.4, "headlight": 0.4, "directional": 1.0,
            "camera_offset": (0.0, 0.0, 0.0)}


def visual_param_vector(values: Dict[str, object]) -> np.ndarray:
    """float64[KM_VP_N] of named per-env values (unnamed ones at their defaults), in KM_VP_* order."""
    out = np.zeros(KM_VP_N)
    full = dict(visual_param_defaults())
    full.update(values)
    for name, (k, n) in VISUAL_PARAMS.items():
        out[k:k + n] = np.broadcast_to(np.asarray(full[name], dtype=np.float64), (n,)) if n > 1 else float(full[name])
    return out


def check_visual_param(name: str, v) -> np.ndarray:
    """ValueError unless every component of v is finite and within the parameter's limits: colours in [0, 1], light terms >= 0,
    |camera offset| <= 0.25 m.  Returns v as a float64 array."""
    if name not in VISUAL_PARAMS:
        raise ValueError("unknown visual parameter %r (known: %s)" % (name, ", ".join(VISUAL_PARAMS)))
    a = np.asarray(v, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError("%s: values must be finite" % name)
    if name.endswith("_rgb"):
        ok, what = ((a >= 0) & (a <= 1)).all(), "in [0, 1]"
    elif name == "camera_offset":
        ok, what = (np.abs(a) <= VP_MAX_CAM_OFFSET).all(), "within +-%g m" % VP_MAX_CAM_OFFSET
    else:
        ok, what = (a >= 0).all(), ">= 0"
    if not ok:
        raise ValueError("%s: values must be %s" % (name, what))
    return a


def with_visual_params(cm: CompiledModel, camera_offset=None, **others) -> CompiledModel:
    """The host definition of the per-env camera offset: a copy of `cm` whose desc has cam_pos[c] + camera_offset for every
    present camera c (in cam_link's frame; world frame for top / head).  An env with offset o renders what a handle of
    with_visual_params(cm, camera_offset=o).desc renders.  Colours and light terms are not part of KModelDesc: they may be named
    (and are validated) but change nothing here."""
    for name, v in others.items():
        check_visual_param(name, v)
    d = KModelDesc.from_buffer_copy(cm.desc)
    if camera_offset is not None:
        o = check_visual_param("camera_offset", camera_offset)
        if o.shape != (3,):
            raise ValueError("camera_offset: expected 3 components, got shape %s" % (o.shape,))
        for c in range(KM_MAX_CAMS):
            if d.cam_present[c]:
                for k in range(3):
                    d.cam_pos[c][k] = d.cam_pos[c][k] + float(o[k])
    return dataclasses.replace(cm, desc=d)


def draw_visual_params(seed: int, genv: int, episode: int, lo, hi) -> np.ndarray:
    """The values ranges mode gives global env `genv` in `episode` (include/kmanip.h kmanip_set_visual_param_ranges): value k is
    lo_k + (hi_k - lo_k) * u_k, product rounded before the sum, u_k from Philox4x32-10 with key = seed and counter
    (genv lo, genv hi, episode, KM_VP_CTR3 + k // 2), words (0, 1) for even k and (2, 3) for odd k."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    g = int(genv) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros(KM_VP_N)
    for blk in range((KM_VP_N + 1) // 2):
        o = _philox4x32_10((g & 0xFFFFFFFF, g >> 32, int(episode) & 0xFFFFFFFF, KM_VP_CTR3 + blk), key)
        for j in range(2):
            k = 2 * blk + j
            if k < KM_VP_N:
                u = _u53(o[2 * j], o[2 * j + 1])
                out[k] = float(lo[k]) + (float(hi[k]) - float(lo[k])) * u
    return out


def ctrl_range(cm: CompiledModel, device=None):
    """(lo, hi): the compiled model's ctrlrange as float64 torch tensors [nu], actuator i's in entry i -- the box that
    KManipEnvHip.lqr_backward_box, rollout_feedback(ctrl_lo=, ctrl_hi=) and ilqr.ilqr(ctrl_lo=, ctrl_hi=) take."""
    import torch
    r = torch.tensor([[cm.desc.ctrlrange[i][0], cm.desc.ctrlrange[i][1]] for i in range(cm.nu)], dtype=torch.float64, device=device)
    return r[:, 0].contiguous(), r[:, 1].contiguous()


def contact_slots(nlink: int) -> int:
    """include/kmanip.h KM_CONTACT_SLOTS: 4 cube corners + KM_SPHERE_SLOTS sphere-cube + KM_SPHERE_TABLE_SLOTS sphere-table (8 / 14)."""
    return 4 + 2 * (nlink // 10) + (6 if nlink >= 20 else 2)


# ---- segmentation labels of the camera renders (include/kmanip.h KM_SEG_*)
KM_SEG_BACKGROUND, KM_SEG_TABLE, KM_SEG_CUBE, KM_SEG_ROBOT_R, KM_SEG_ROBOT_L, KM_SEG_N = 0, 1, 2, 3, 4, 5
SEG_CLASSES = ("background", "table", "cube", "robot_r", "robot_l")


def sphere_arm(cm: CompiledModel, strict: bool = False) -> list:
    """The arm (0 right, 1 left) of every collision sphere, as kmanip_create computes it for the label render: sphere s belongs to
    arm a when sphere_link[s] is an ancestor-or-self of arm_site_link[a] or of one of arm_grip_id[a][*], walking link_parent.
    That names exactly one arm for every sphere of the reference models.  For any other desc kmanip_create refuses nothing: a
    sphere on several chains gets the lowest of those arms and one on none gets arm 0, and so does this function; strict=True
    raises ValueError for such a sphere instead."""
    d = cm.desc
    out = []
    for s in range(d.nsphere):
        arms = []
        for a in range(KM_MAX_ARMS):
            if not d.arm_present[a]:
                continue
            chain = set()
            for leaf in (d.arm_site_link[a], d.arm_grip_id[a][0], d.arm_grip_id[a][1]):
                j = leaf
                while 0 <= j < d.nlink:
                    chain.add(j)
                    j = d.link_parent[j]
            if d.sphere_link[s] in chain:
                arms.append(a)
        if strict and len(arms) != 1:
            raise ValueError("sphere %d lies on the chains of arms %s, expected exactly one" % (s, arms))
        out.append(arms[0] if arms else 0)
    return out


# ---- link capsules of the RGB / label renders (include/kmanip.h KLinkCapsule)
KM_MAX_LINK_CAPSULES = 24


def link_arm(cm: CompiledModel) -> Dict[int, int]:
    """{link: arm} for every link on an arm's chain -- sphere_arm's rule: an ancestor-or-self of arm_site_link[a] or of one of
    arm_grip_id[a][*]; a link on several chains belongs to the lowest of those arms.  Links on no chain are absent."""
    d = cm.desc
    out: Dict[int, int] = {}
    for a in range(KM_MAX_ARMS):
        if not d.arm_present[a]:
            continue
        for leaf in (d.arm_site_link[a], d.arm_grip_id[a][0], d.arm_grip_id[a][1]):
            j = leaf
            while 0 <= j < d.nlink:
                out.setdefault(j, a)
                j = d.link_parent[j]
    return out


def camera_intrinsics(cm: CompiledModel, cam, height=None, width=None) -> dict:
    """Pinhole intrinsics of a height x width image of camera `cam` (a name or a Cam; default size: the camera's reference
    resolution): {"f", "cx", "cy", "fovy"} with f = (height / 2) / tan(fovy / 2) in pixels (square pixels), cx = width / 2,
    cy = height / 2, fovy in degrees.  Pixel convention of every render of the library: pixel (r, c) is the ray through the pixel's
    centre, dx = (c + 0.5 - cx) / f to the right and dy = -(r + 0.5 - cy) / f upwards (rows run down, the camera's y axis up), with
    direction x dx + y dy - z in the camera's axes; a depth D (metres along the optical axis) is the camera-frame point
    (D dx, D dy, -D)."""
    name = getattr(cam, "name", cam)
    if name not in KM_CAM_INDEX or not cm.desc.cam_present[KM_CAM_INDEX[name]]:
        raise ValueError("no camera %r in this model" % (name,))
    height = CAMERAS[name].h if height is None else int(height)
    width = CAMERAS[name].w if width is None else int(width)
    if height < 1 or width < 1:
        raise ValueError("camera_intrinsics: height and width must be positive")
    fovy = float(cm.desc.cam_fovy[KM_CAM_INDEX[name]])
    return {"f": 0.5 * height / math.tan(0.5 * fovy * (math.pi / 180.0)), "cx": 0.5 * width, "cy": 0.5 * height, "fovy": fovy}


def link_capsules(cm: CompiledModel, radius: float = 0.03) -> list:
    """The default capsule list of kmanip_set_render_links, as dicts with the fields of KLinkCapsule (link, label, cam_mask, p0,
    seg, radius), in this order:
      joint-to-joint capsules -- for every link j whose parent p >= 0, both on an arm's chain (link_arm): one capsule on p from
        its origin to link_pos[j], of `radius` (0.03 m: the collision housings already in the model);
      finger capsules -- for every visible sphere s: one capsule on sphere_link[s] from its origin to sphere_pos[s], of
        sphere_radius[s].
    label = KM_SEG_ROBOT_R + the chain's arm.  cam_mask = every present camera, minus camera c for capsules whose link is
    cam_link[c] or link_parent[cam_link[c]]: a gripper camera sits 5 cm from its link's joint origin and looks through it."""
    d = cm.desc
    la = link_arm(cm)
    present = 0
    for c in range(KM_MAX_CAMS):
        if d.cam_present[c]:
            present |= 1 << c

    def mask(link):
        m = present
        for c in range(KM_MAX_CAMS):
            cl = d.cam_link[c]
            if d.cam_present[c] and cl >= 0 and link in (cl, d.link_parent[cl]):
                m &= ~(1 << c)
        return m

    def cap(link, seg, rad):
        return {"link": int(link), "label": KM_SEG_ROBOT_R + la[link], "cam_mask": mask(link), "p0": (0.0, 0.0, 0.0),
                "seg": tuple(float(x) for x in seg), "radius": float(rad)}
    caps = []
    for j in range(d.nlink):
        p = d.link_parent[j]
        if p >= 0 and p in la and j in la:
            caps.append(cap(p, d.link_pos[j], radius))
    for s in range(d.nsphere):
        if d.sphere_visible[s] and d.sphere_link[s] in la:
            caps.append(cap(d.sphere_link[s], d.sphere_pos[s], d.sphere_radius[s]))
    if len(caps) > KM_MAX_LINK_CAPSULES:
        raise ValueError("%d capsules: kmanip_set_render_links takes at most %d" % (len(caps), KM_MAX_LINK_CAPSULES))
    return caps


def check_link_capsules(cm: CompiledModel, caps) -> list:
    """kmanip_set_render_links' validation on the host: a list of dicts (or (link, label, cam_mask, p0, seg, radius) tuples) ->
    a list of dicts; ValueError for more than KM_MAX_LINK_CAPSULES entries, a link out of range, a label other than the two robot
    classes, a radius that is not finite and > 0, or a p0 / seg that is not finite."""
    keys = ("link", "label", "cam_mask", "p0", "seg", "radius")
    out = []
    caps = list(caps)
    if len(caps) > KM_MAX_LINK_CAPSULES:
        raise ValueError("%d capsules: at most %d" % (len(caps), KM_MAX_LINK_CAPSULES))
    for k, c in enumerate(caps):
        c = dict(c) if isinstance(c, dict) else dict(zip(keys, c))
        if set(c) != set(keys):
            raise ValueError("capsule %d: expected the fields %s" % (k, ", ".join(keys)))
        p0, seg = np.asarray(c["p0"], dtype=np.float64), np.asarray(c["seg"], dtype=np.float64)
        if not 0 <= int(c["link"]) < cm.desc.nlink:
            raise ValueError("capsule %d: link out of range" % k)
        if int(c["label"]) not in (KM_SEG_ROBOT_R, KM_SEG_ROBOT_L):
            raise ValueError("capsule %d: label must be KM_SEG_ROBOT_R or KM_SEG_ROBOT_L" % k)
        if not (np.isfinite(c["radius"]) and c["radius"] > 0):
            raise ValueError("capsule %d: radius must be finite and > 0" % k)
        if p0.shape != (3,) or seg.shape != (3,) or not (np.isfinite(p0).all() and np.isfinite(seg).all()):
            raise ValueError("capsule %d: p0 and seg must be 3 finite numbers" % k)
        out.append({"link": int(c["link"]), "label": int(c["label"]), "cam_mask": int(c["cam_mask"]) & 0xFFFFFFFF,
                    "p0": tuple(float(x) for x in p0), "seg": tuple(float(x) for x in seg), "radius": float(c["radius"])})
    return out
