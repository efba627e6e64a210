"""The CPU side of kmanip_kinematics_rows and kmanip_site_cost: a stand-in env, an extended-precision restatement and the input family.

KinematicsAt        a mixin that gives feedback_oracle.OracleFeedback a kinematics_at of the device's shapes and status rules, from
                    kin_oracle.geometry (poses, Jacobians, site velocity; qM and qfrc_bias through kin_oracle.decode where asked for).
                    OracleSite is OracleFeedback with it: ilqr.SiteCost(device=False) and ilqr.ilqr run on it unchanged.
restate(...)        cost, lx, lxx, e_pos and e_rot of include/kmanip.h KSiteCostIn from a geometry dict, in np.longdouble (or, with
                    dtype=np.float64, the same text in double).  Independent of the kernel's route: the rotation error comes from the
                    matrix R_site R_target^T (angle = atan2(|skew part|, (trace - 1) / 2)), not from quaternions.
family(asset, ...)  THE INPUT FAMILY: the states are regime_states.cells(asset) (47 / 72: not a multiple of the 4 / 2 rows of a wave); the
                    targets are the site's own pose displaced by 0.05 N(0, 1) m and by a rotation of angle U(0.1, 2.5) rad about a
                    random axis (default_rng(seed)); a draw is kept only if every |e_rot| restate computes is below 2.8 rad, away from
                    the cut at pi.  Weights: per row and arm, position and rotation weight drawn from {0, 0.5, 20} -- the nine
                    patterns are dealt in turn, then shuffled, so every pattern occurs.  With follow_cube the target position is stored
                    as an offset from the cube's."""
import numpy as np

import feedback_oracle as FO
import kin_oracle as KO

WEIGHTS = (0.0, 0.5, 20.0)
MAX_EROT = 2.8
KIN_SHAPES = {"link_xpos": ("nl", 3), "link_xmat": ("nl", 9), "site_xpos": (2, 3), "site_xmat": (2, 9), "site_jacp": (2, 3, "nv"),
              "site_jacr": (2, 3, "nv"), "site_vel": (2, 6), "qM": ("nv", "nv"), "qfrc_bias": ("nv",)}


class KinematicsAt:
    """kinematics_at(envs, qpos, qvel, out, fields) of KManipEnvHip on the oracle: row r takes env envs[r]'s model and stored state
    (self.state) where no row is given.  Torch in, torch out; NumPy otherwise."""

    def kinematics_at(self, envs=None, qpos=None, qvel=None, out=None, fields=None):
        import torch
        is_t = lambda t: isinstance(t, torch.Tensor)
        as_torch = any(is_t(t) for t in (envs, qpos, qvel))
        np_ = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if is_t(t) else t)
        cm = self.cm
        q, v = np_(qpos), np_(qvel)
        idx = None if envs is None else np.asarray(np_(envs), dtype=np.int64).reshape(-1)
        n = len(idx) if idx is not None else next((len(t) for t in (q, v) if t is not None), self.num_envs)
        names = list(fields) if fields is not None else list(KO.FIELDS) + ["status"]
        assert not set(names) - set(KO.FIELDS) - {"status"}, names
        dims = {"nl": cm.nlink, "nv": cm.nv}
        res = {k: np.zeros((n,) + tuple(dims.get(d, d) for d in KIN_SHAPES[k])) for k in names if k != "status"}
        status = np.zeros(n, dtype=np.uint8)
        heavy = "qM" in names or "qfrc_bias" in names
        for r in range(n):
            e = r if idx is None else int(idx[r])
            if not 0 <= e < self.num_envs:
                status[r] = 2
                continue
            qr = q[r] if q is not None else self.state["qpos"][e]
            vr = v[r] if v is not None else self.state["qvel"][e]
            if not (np.isfinite(qr).all() and np.isfinite(vr).all()):
                status[r] = 1
                continue
            m = self.models[e]
            orc = self._orc[id(m)]
            o = KO.decode(m, orc, qr, vr) if heavy else KO.geometry(m, orc, qr, vr)
            for k in res:
                res[k][r] = np.asarray(o[k]).reshape(res[k][r].shape)
        if "status" in names:
            res["status"] = status
        return {k: (torch.from_numpy(res[k]) if as_torch else res[k]) for k in names}


class OracleSite(KinematicsAt, FO.OracleFeedback):
    pass


def boxed_stand_in(cm, num_envs):
    """OracleSite on boxqp_reference.OracleLqrBox: rollout_feedback takes ctrl_lo / ctrl_hi (one box shared by the rows)."""
    import boxqp_reference as BQ

    class OracleSiteBox(KinematicsAt, BQ.OracleLqrBox):
        pass
    return OracleSiteBox(cm, num_envs)


# ------------------------------------------------------------------------------------------------------------------- restatement
def _quat2mat(q, dtype):
    q = np.asarray(q, dtype=dtype)
    w, x, y, z = q / np.sqrt((q * q).sum())
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dtype)


def rotation_vector(Rm, dtype=np.longdouble):
    """The world-frame rotation vector of a rotation matrix with angle in (0, pi): axis from the skew part, angle from atan2."""
    Rm = np.asarray(Rm, dtype=dtype)
    v = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]], dtype=dtype) / dtype(2)
    s = np.sqrt((v * v).sum())
    c = (Rm[0, 0] + Rm[1, 1] + Rm[2, 2] - dtype(1)) / dtype(2)
    if s == 0:
        return np.zeros(3, dtype=dtype)
    return v / s * np.arctan2(s, c)


def restate(cm, geo, qpos, target_pos, target_quat, weight, follow, dtype=np.longdouble):
    """dict(cost, lx [2 nv], lxx [2 nv, 2 nv], resid [2, 6]) of one state from its geometry dict (kin_oracle.geometry / decode),
    target_pos [2, 3], target_quat [2, 4] or None, weight [2, 2], follow (two bools), every operation in `dtype`."""
    d = cm.desc
    nl, nv = cm.nlink, cm.nv
    cube = np.asarray(qpos[nl:nl + 3], dtype=dtype)
    cost = dtype(0)
    lx, lxx, resid = np.zeros(2 * nv, dtype=dtype), np.zeros((2 * nv, 2 * nv), dtype=dtype), np.zeros((2, 6), dtype=dtype)
    for a in range(2):
        if not d.arm_present[a]:
            continue
        w0, w1 = dtype(weight[a][0]), dtype(weight[a][1]) if target_quat is not None else dtype(0)
        Jp, Jr = np.asarray(geo["site_jacp"][a], dtype=dtype).copy(), np.asarray(geo["site_jacr"][a], dtype=dtype)
        pstar = np.asarray(target_pos[a], dtype=dtype)
        if follow[a]:
            pstar = pstar + cube
            Jp[:, nl:nl + 3] = -np.eye(3, dtype=dtype)
        e_pos = np.asarray(geo["site_xpos"][a], dtype=dtype) - pstar
        e_rot = np.zeros(3, dtype=dtype)
        if w1 != 0:
            Rs = np.asarray(geo["site_xmat"][a], dtype=dtype).reshape(3, 3)
            e_rot = rotation_vector(Rs @ _quat2mat(target_quat[a], dtype).T, dtype)
        resid[a, :3], resid[a, 3:] = e_pos, e_rot
        cost = cost + (w0 * (e_pos * e_pos).sum() + w1 * (e_rot * e_rot).sum()) / dtype(2)
        lx[:nv] += w0 * (Jp.T @ e_pos) + w1 * (Jr.T @ e_rot)
        lxx[:nv, :nv] += w0 * (Jp.T @ Jp) + w1 * (Jr.T @ Jr)
    return dict(cost=cost, lx=lx, lxx=lxx, resid=resid)


# -------------------------------------------------------------------------------------------------------------------- the family
def _rot(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


_FAMILY = {}


def family(asset, follow=False, seed=0):
    """The module header's family for one asset, built once per argument set: dict(cm, geo (kin_oracle.cell_decodes' decodes), qpos,
    qvel, target_pos [n, 2, 3], target_quat [n, 2, 4], weight [n, 2, 2], follow (two bools), kept [n] bool: the draw passed the
    |e_rot| < MAX_EROT test, ref: restate per state in longdouble)."""
    import regime_states as R
    key = (asset, bool(follow), seed)
    if key in _FAMILY:
        return _FAMILY[key]
    cm, dec, _ = KO.cell_decodes(asset)
    qpos, qvel, _, labels = R.cells(asset)
    n, nl = len(labels), cm.nlink
    rng = np.random.default_rng(seed)
    fol = (bool(follow), bool(follow))
    tp, tq = np.zeros((n, 2, 3)), np.zeros((n, 2, 4))
    tq[:, :, 0] = 1.0
    patterns = [(p, r) for p in WEIGHTS for r in WEIGHTS]
    w = np.zeros((n, 2, 2))
    for a in range(2):
        w[:, a] = np.array([patterns[i % 9] for i in range(n)])[rng.permutation(n)]
    for e, o in enumerate(dec):
        for a in range(2):
            if not cm.desc.arm_present[a]:
                continue
            tp[e, a] = o["site_xpos"][a] + 0.05 * rng.standard_normal(3) - (qpos[e, nl:nl + 3] if follow else 0.0)
            Rt = _rot(rng.standard_normal(3), rng.uniform(0.1, 2.5)) @ o["site_xmat"][a].reshape(3, 3)
            tq[e, a] = R.mat2quat(Rt)
    # the test on |e_rot| ignores the weights: a rotation weight of zero would hide the angle
    ones = np.ones((2, 2))
    kept = np.array([all(float(np.linalg.norm(restate(cm, dec[e], qpos[e], tp[e], tq[e], ones, fol)["resid"][a, 3:])) < MAX_EROT
                         for a in range(2)) for e in range(n)])
    ref = [restate(cm, dec[e], qpos[e], tp[e], tq[e], w[e], fol) for e in range(n)]
    _FAMILY[key] = dict(cm=cm, geo=dec, qpos=qpos, qvel=qvel, labels=labels, target_pos=tp, target_quat=tq, weight=w, follow=fol, kept=kept,
                        ref=ref)
    return _FAMILY[key]


def relative(got, ref):
    """max |got - ref| relative to the largest entry of ref (1 where ref is all zeros): how the bar is stated, per output and row."""
    ref = np.asarray(ref, dtype=np.longdouble)
    scale = np.abs(ref).max() if ref.size else 0
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max() / (scale if scale > 0 else 1))
