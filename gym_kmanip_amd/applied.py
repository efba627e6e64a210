"""Rows of an applied-force tensor (KManipEnvHip.bind_applied_force: MuJoCo's data.qfrc_applied) from Cartesian wrenches.

Plain tensor arithmetic: it runs wherever its inputs live (device tensors stay on the device, CPU tensors work too) and never calls
the library.  A row has nv = nlink + 6 columns in the dof order of kinematics()' qM / qfrc_bias:
  0 .. nlink-1          joint torque (hinge) or force (slide)
  nlink .. nlink+2      force on the cube at its centre of mass, world frame
  nlink+3 .. nlink+5    torque on the cube in the cube's BODY frame (free-joint convention)
cube_wrench and site_wrench ACCUMULATE into `out` ([n, nv], allocated as zeros when None) and return it, so several wrenches add up
in one row:

    tau = env.new_applied_force()                              # zeros, bound
    tau.zero_()
    applied.cube_wrench(cm, env.state_tensors()["qpos"], force=push, out=tau)
    applied.site_wrench(cm, env.kinematics(), 0, force=f_hand, out=tau)

from_inverse and fwdinv_residual work on the results of KManipEnvHip.inverse (MuJoCo's mj_inverse) and forces:

    inv = env.inverse(qacc_wanted)                             # the total force behind qacc_wanted
    tau.copy_(applied.from_inverse(inv, env.forces()))         # ... minus what the servos already give: forces()["qacc"] == qacc_wanted
"""
from __future__ import annotations


def _torch():
    import torch
    return torch


def _out(cm, like, n, out):
    torch = _torch()
    if out is None:
        return torch.zeros((n, cm.nv), dtype=like.dtype, device=like.device)
    if tuple(out.shape) != (n, cm.nv):
        raise ValueError("out must have shape (%d, %d), got %s" % (n, cm.nv, tuple(out.shape)))
    return out


def _vec3(v, like, n, what):
    torch = _torch()
    v = torch.as_tensor(v, dtype=like.dtype, device=like.device)
    if v.shape not in ((3,), (n, 3)):
        raise ValueError("%s must have shape (3,) or (%d, 3), got %s" % (what, n, tuple(v.shape)))
    return v.expand(n, 3)


def _pad_actuator(inv, f):
    """qfrc_actuator [n, nu] of a forces() result as [n, nv] rows (the cube's six columns zero)."""
    torch = _torch()
    qi, fa = inv["qfrc_inverse"], f["qfrc_actuator"]
    return torch.cat((fa, torch.zeros((fa.shape[0], qi.shape[1] - fa.shape[1]), dtype=fa.dtype, device=fa.device)), dim=1)


def from_inverse(inv, f):
    """Rows for bind_applied_force from an inverse() result `inv` (it needs qfrc_inverse) and a forces() result `f` of the same state
    (it needs qfrc_actuator): qfrc_inverse - pad(qfrc_actuator), the force that ON TOP OF THE SERVOS produces the acceleration
    `inv` was evaluated at.  A new [n, nv] tensor."""
    return inv["qfrc_inverse"] - _pad_actuator(inv, f)


def fwdinv_residual(f, inv, applied=None):
    """[n]: per-env max |qfrc_inverse - pad(qfrc_actuator) - applied|, where `inv` is inverse() evaluated at f["qacc"] and `applied`
    the applied-force rows that were bound when `f` was computed (None: none).  At the exact forward solution it is zero: the figure
    measures how far the solver stopped from it (the comparison of MuJoCo's mj_compareFwdInv)."""
    r = from_inverse(inv, f)
    if applied is not None:
        r = r - applied
    return r.abs().amax(dim=1)


def quat_to_mat(q):
    """[n, 3, 3] rotation matrices of [n, 4] wxyz quaternions, normalised first."""
    torch = _torch()
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def cube_wrench(cm, qpos, force=None, torque=None, out=None):
    """A WORLD-frame force at the cube's centre of mass and a WORLD-frame torque on the cube, added to `out`.  qpos: [n, nq]
    (state_tensors()["qpos"]); force / torque: (3,) or [n, 3], None = zero.  The force goes to columns nlink .. nlink+2 as it is;
    the torque is rotated into the cube's frame, R(q)^T tau with q the normalised cube quaternion of qpos, and goes to columns
    nlink+3 .. nlink+5."""
    torch = _torch()
    nl = cm.nlink
    n = qpos.shape[0]
    out = _out(cm, qpos, n, out)
    if force is not None:
        out[:, nl:nl + 3] += _vec3(force, qpos, n, "force")
    if torque is not None:
        R = quat_to_mat(qpos[:, nl + 3:nl + 7])
        out[:, nl + 3:nl + 6] += torch.einsum("nij,ni->nj", R, _vec3(torque, qpos, n, "torque"))
    return out


def site_wrench(cm, kin, arm, force=None, torque=None, out=None):
    """A WORLD-frame force at the end-effector site of `arm` (0 = right) and a world-frame torque on its link, as joint forces
    jacp^T f + jacr^T tau, added to `out`.  kin: a kinematics() result with site_jacp / site_jacr ([n, 2, 3, nv]); force / torque:
    (3,) or [n, 3], None = zero."""
    torch = _torch()
    jp = kin["site_jacp"][:, arm]
    n = jp.shape[0]
    out = _out(cm, jp, n, out)
    if force is not None:
        out += torch.einsum("nij,ni->nj", jp, _vec3(force, jp, n, "force"))
    if torque is not None:
        out += torch.einsum("nij,ni->nj", kin["site_jacr"][:, arm], _vec3(torque, jp, n, "torque"))
    return out
