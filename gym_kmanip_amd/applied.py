"""Rows of an applied-force tensor (KManipEnvHip.bind_applied_force: MuJoCo's data.qfrc_applied) from Cartesian wrenches.

Plain tensor arithmetic: it runs wherever its inputs live (device tensors stay on the device, CPU tensors work too) and never calls
the library.  A row has nv = nlink + 6 columns in the dof order of kinematics()' qM / qfrc_bias:
  0 .. nlink-1          joint torque (hinge) or force (slide)
  nlink .. nlink+2      force on the cube at its centre of mass, world frame
  nlink+3 .. nlink+5    torque on the cube in the cube's BODY frame (free-joint convention)
Both helpers ACCUMULATE into `out` ([n, nv], allocated as zeros when None) and return it, so several wrenches add up in one row:

    tau = env.new_applied_force()                              # zeros, bound
    tau.zero_()
    applied.cube_wrench(cm, env.state_tensors()["qpos"], force=push, out=tau)
    applied.site_wrench(cm, env.kinematics(), 0, force=f_hand, out=tau)
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
