"""Link and site poses, site Jacobians, M and bias forces of a state from the CPU oracle, in NumPy: the reference of kmanip_kinematics.

Oracle.fk gives the link origins and quaternions and the site poses; xmat is the rotation matrix of the (normalised) quaternion.
Oracle.dynamics gives the dense joint-space inertia M (cube block diag(m, m, m, I)) and the bias forces; neither depends on ctrl.
The site Jacobian is the geometric one, built from fk alone: the world axis of joint j is xmat_j @ jnt_axis[j], and walking
link_parent from arm_site_link[a] visits the dofs that move the site -- hinge j: axis_j x (site - xpos_j) in jacp and axis_j in jacr;
slide j: axis_j in jacp, 0 in jacr; every other column, the cube's six included, 0.  site_vel = [jacp qvel, jacr qvel]."""
import numpy as np

from regime_states import quat2mat

FIELDS = ("link_xpos", "link_xmat", "site_xpos", "site_xmat", "site_jacp", "site_jacr", "site_vel", "qM", "qfrc_bias")
GEOMETRY = ("link_xpos", "link_xmat", "site_xpos", "site_xmat", "site_jacp", "site_jacr", "site_vel")


def site_chain(cm, arm):
    """The dofs that move arm's site: arm_site_link and its ancestors."""
    d = cm.desc
    out = []
    j = d.arm_site_link[arm]
    while j >= 0:
        out.append(j)
        j = d.link_parent[j]
    return out[::-1]


def geometry(cm, orc, qpos, qvel=None):
    """The fk part of decode: poses, Jacobians and (with qvel) the site velocity of one state."""
    d = cm.desc
    nl, nv = cm.nlink, cm.nv
    qpos = np.asarray(qpos, dtype=np.float64)
    xpos, xquat, sp, sm = orc.fk(qpos)
    xmat = np.stack([quat2mat(q) for q in xquat])
    axis = np.stack([xmat[j] @ np.array(d.jnt_axis[j]) for j in range(nl)])
    jacp, jacr = np.zeros((2, 3, nv)), np.zeros((2, 3, nv))
    for a in range(2):
        if not d.arm_present[a]:
            assert not sp[a].any() and not sm[a].any()
            continue
        for j in site_chain(cm, a):
            if d.jnt_type[j] == 1:
                jacp[a, :, j] = axis[j]
            else:
                jacp[a, :, j] = np.cross(axis[j], sp[a] - xpos[j])
                jacr[a, :, j] = axis[j]
    out = dict(link_xpos=xpos, link_xmat=xmat.reshape(nl, 9), site_xpos=sp, site_xmat=sm.reshape(2, 9), site_jacp=jacp, site_jacr=jacr)
    if qvel is not None:
        qvel = np.asarray(qvel, dtype=np.float64)
        out["site_vel"] = np.concatenate([jacp @ qvel, jacr @ qvel], axis=1)
    return out


def decode(cm, orc, qpos, qvel):
    """Everything kmanip_kinematics reports for one state, from a one-env oracle (shapes: the KKinDev fields without the env axis)."""
    qpos = np.asarray(qpos, dtype=np.float64); qvel = np.asarray(qvel, dtype=np.float64)
    out = geometry(cm, orc, qpos, qvel)
    dyn = orc.dynamics(qpos, qvel, qpos[:cm.nlink])
    out["qM"], out["qfrc_bias"] = dyn["M"], dyn["bias"]
    return out


def twin(cm, orc, qpos, qvel):
    """M and bias with the joint positions and qvel multiplied by (1 + 1e-15): the distance to decode is the reference's own error."""
    q = np.array(qpos, dtype=np.float64)
    q[:cm.nlink] *= 1.0 + 1e-15
    dyn = orc.dynamics(q, np.asarray(qvel, dtype=np.float64) * (1.0 + 1e-15), q[:cm.nlink])
    return dict(qM=dyn["M"], qfrc_bias=dyn["bias"])


def scales(o, qvel):
    """Per-env normalisers: (site_vel, qM, qfrc_bias) = max(1, max|qvel|), max(1, max|M|), max(1, max|bias|)."""
    return (max(1.0, float(np.abs(qvel).max())), max(1.0, float(np.abs(o["qM"]).max())), max(1.0, float(np.abs(o["qfrc_bias"]).max())))


def differences(got, o, qvel):
    """{field: max |got - o|, normalised as the bars are stated} for the fields present in `got` (arrays of one env)."""
    sv, sm, sb = scales(o, np.asarray(qvel))
    norm = dict(site_vel=sv, qM=sm, qfrc_bias=sb)
    return {k: float(np.abs(np.asarray(got[k]).reshape(-1) - np.asarray(o[k]).reshape(-1)).max()) / norm.get(k, 1.0) for k in FIELDS if k in got}


_CELL_DECODES = {}


def cell_decodes(asset):
    """(cm, decode of every regime cell's copy (regime_states.cells), its twin), computed once per asset and shared by the tests."""
    import regime_states as R
    from oracle.oracle import Oracle
    if asset not in _CELL_DECODES:
        cm = R.model(asset)
        qpos, qvel, _, labels = R.cells(asset)
        orc = Oracle(cm, 1)
        dec = [decode(cm, orc, qpos[e], qvel[e]) for e in range(len(labels))]
        tw = [twin(cm, orc, qpos[e], qvel[e]) for e in range(len(labels))]
        _CELL_DECODES[asset] = (cm, dec, tw)
    return _CELL_DECODES[asset]


# ---------------------------------------------------------------------------------------------- the resolved-rate reach, in NumPy
def arm_columns(cm):
    """[(arm, action slice, dof ids)] of the arms a *QPos id drives."""
    out = []
    for a, (key, ids) in enumerate((("q_pos_r", cm.spec.q_id_r_mask), ("q_pos_l", cm.spec.q_id_l_mask))):
        if key in cm.act_slices:
            out.append((a, cm.act_slices[key], list(ids)))
    return out


def resolved_rate_action(cm, site_xpos, site_jacp, goal, damping=1e-4):
    """The action of gym_kmanip_amd/examples/resolved_rate_reach.py for a batch: per arm dq = Jp^T (Jp Jp^T + damping I)^-1 (goal -
    site_xpos) on the arm's arm_q_id columns, action = clip(dq / q_pos_delta, -1, 1), grip 0.  site_xpos, goal [n, 2, 3];
    site_jacp [n, 2, 3, nv]."""
    n = len(site_xpos)
    act = np.zeros((n, cm.act_dim), dtype=np.float32)
    for a, sl, ids in arm_columns(cm):
        Jp = site_jacp[:, a][:, :, ids]
        A = Jp @ Jp.transpose(0, 2, 1) + damping * np.eye(3)
        dq = (Jp.transpose(0, 2, 1) @ np.linalg.solve(A, (goal[:, a] - site_xpos[:, a])[:, :, None]))[:, :, 0]
        act[:, sl] = np.clip(dq / cm.desc.q_pos_delta, -1.0, 1.0)
    return act


def reach_goals(cm, site_xpos, seed):
    """Each site's position plus an offset drawn uniformly in +-5 cm per axis."""
    return site_xpos + np.random.default_rng(seed).uniform(-0.05, 0.05, site_xpos.shape)


def median_distance(cm, site_xpos, goal):
    arms = [a for a, _, _ in arm_columns(cm)]
    return float(np.median(np.linalg.norm(site_xpos[:, arms] - goal[:, arms], axis=-1)))
