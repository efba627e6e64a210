"""Gradients through rollouts: the first-order use of the step Jacobians that ilqr.trajectory_fd returns.

rollout_grad      the gradient of a cost on a rollout with respect to the controls, the initial state and, closed loop, the gains
rollout_jacobian  d x_T / d u_0..T-1 and d x_T / d x_0, nx cotangent vectors per problem through one adjoint
diff_rollout      env.rollout as a torch.autograd.Function: loss.backward() passes through it

The state is (qpos in the tangent space, qvel), 2 nv wide, as transition_fd defines it.  The sweep itself is
derivatives.adjoint_pass (a torch loop over the steps) or, with device=True, env.adjoint (kmanip_adjoint: one launch).  With
device=False everything needs only env.rollout, env.rollout_feedback and env.cm, so a CPU stand-in
(tests/tools/feedback_oracle.py OracleFeedback) runs the same code, as it runs ilqr."""
import functools

from .derivatives import adjoint_pass, tangent_diff
from .ilqr import trajectory_fd


def _sweep(env, fd, gx, gu, gains, gains_t, m, device):
    """(lam, mu) of derivatives.adjoint_pass on trajectory_fd's result, or of env.adjoint on deriv_t where fused gave it."""
    if not device:
        if gains is None and gains_t is not None:
            gains = gains_t.transpose(2, 3)
        return adjoint_pass(fd["A"], fd["B"], gx, gu, gains, m)
    dyn = dict(deriv_t=fd["deriv_t"]) if "deriv_t" in fd else dict(A=fd["A"], B=fd["B"])
    r = env.adjoint(gx, gu, gains=gains if gains_t is None else None, gains_t=gains_t, m=m, **dyn)
    return r["lam"], r["mu"]


def rollout_grad(env, envs, qpos0, qvel0, warm0, ctrl, cost, gains=None, gains_t=None, qpos_ref=None, qvel_ref=None, qfrc_applied=None,
                 nsub=None, eps=1e-6, fused=False, device=False):
    """The gradient of cost.total over the rollout of ctrl [n, T, nu] from (qpos0, qvel0, warm0) [n, ..]: ONE ilqr.trajectory_fd call
    (its one rollout launch is the nominal trajectory, its transition_fd call the Jacobians of every step), one cost.derivatives call
    (lx and lu only: a first-order method) and one adjoint sweep.
    CLOSED LOOP (gains [n, T, nu, nx] or gains_t [n, T, nx, nu], with qpos_ref [n, T, nq] and qvel_ref [n, T, nv]): one
    rollout_feedback call of the policy u_t = ctrl_t + K_t dx_t comes first, and everything continues with the controls it recorded
    -- replayed open loop they give the same trajectory -- while the sweep carries K_t' mu_t.
    Returns a dict:
      cost [n]; grad_ctrl [n, T, nu], the gradient with respect to ctrl (closed loop: the open-loop term); grad_x0 [n, 2 nv], with
      respect to the initial tangent state; lam [n, T + 1, 2 nv]; ctrl [n, T, nu] the controls that acted; qpos [n, T + 1, nq],
      qvel [n, T + 1, nv]; A [n, T, 2 nv, 2 nv] and B [n, T, 2 nv, nu], the step Jacobians the sweep used; status [n] and status_fd
      [n], trajectory_fd's (closed loop: status is the larger of the feedback launch's and the replay's).  A row with a nonzero
      status has no gradient worth the name.
      closed loop also grad_gains [n, T, nu, nx] = mu_t (x) dx_t, dx_t = [tangent_diff(qpos_t, qpos_ref_t) ; qvel_t - qvel_ref_t].
    With gains dx is taken as linear in the state (derivatives.adjoint_pass's one approximation).
    fused: trajectory_fd's.  device: the sweep is env.adjoint (kmanip_adjoint, one launch) on deriv_t where fused gives it, else on
    A and B; False: derivatives.adjoint_pass."""
    import torch
    cm = env.cm
    n, T = int(ctrl.shape[0]), int(ctrl.shape[1])
    closed = gains is not None or gains_t is not None
    status_fb = None
    if closed:
        if qpos_ref is None or qvel_ref is None:
            raise ValueError("rollout_grad: a closed-loop rollout needs qpos_ref and qvel_ref")
        idx = torch.arange(n, dtype=torch.int32, device=ctrl.device) if envs is None else torch.as_tensor(envs).to(device=ctrl.device, dtype=torch.int32)
        fb = env.rollout_feedback(envs=idx, qpos=qpos0, qvel=qvel0, warm=warm0, ctrl=ctrl, qfrc_applied=qfrc_applied,
                                  **(dict(gains=gains) if gains_t is None else dict(gains_t=gains_t)),
                                  qpos_ref=qpos_ref.contiguous(), qvel_ref=qvel_ref.contiguous(), nsub=nsub, fields=("ctrl", "status"))
        ctrl, status_fb = fb["ctrl"], fb["status"]
    fd = trajectory_fd(env, envs, qpos0, qvel0, warm0, ctrl, qfrc_applied=qfrc_applied, nsub=nsub, eps=eps, fused=fused)
    lx, lu = cost.derivatives(fd["qpos"], fd["qvel"], ctrl)[:2]
    lam, mu = _sweep(env, fd, lx, lu, gains, gains_t, 1, device)
    out = {"cost": cost.total(fd["qpos"], fd["qvel"], ctrl), "grad_ctrl": mu, "grad_x0": lam[:, 0], "lam": lam, "ctrl": ctrl,
           "qpos": fd["qpos"], "qvel": fd["qvel"], "status": fd["status"] if status_fb is None else torch.maximum(fd["status"], status_fb),
           "status_fd": fd["status_fd"], "A": fd["A"], "B": fd["B"]}
    if closed:
        q, v = fd["qpos"][:, :-1], fd["qvel"][:, :-1]
        dq = tangent_diff(cm, q.reshape(n * T, -1), qpos_ref.reshape(n * T, -1)).reshape(n, T, -1)
        dx = torch.cat([dq, v - qvel_ref], dim=2)
        out["grad_gains"] = mu[:, :, :, None] * dx[:, :, None, :]
    return out


def rollout_jacobian(env, envs, qpos0, qvel0, warm0, ctrl, qfrc_applied=None, nsub=None, eps=1e-6, fused=False, device=False):
    """The sensitivity of the final state of an open-loop rollout: one trajectory_fd call and ONE adjoint sweep of m = nx = 2 nv
    cotangent vectors per problem, gx the identity at T -- every step's Jacobians are read once for all nx vectors.  Returns a dict:
      dxT_du [n, nx, T, nu]: entry (e, j, t, i) = d x_T[j] / d u_t[i];  dxT_dx0 [n, nx, nx]: entry (e, j, k) = d x_T[j] / d x_0[k]
      qpos [n, T + 1, nq], qvel [n, T + 1, nv], status [n], status_fd [n]: trajectory_fd's.
    A site's sensitivity d site_pose / d u is its Jacobian at x_T (kinematics_at: site_jacp, site_jacr) times dxT_du's position
    rows.  fused, device: rollout_grad's."""
    import torch
    n, T = int(ctrl.shape[0]), int(ctrl.shape[1])
    nx = 2 * env.cm.nv
    fd = trajectory_fd(env, envs, qpos0, qvel0, warm0, ctrl, qfrc_applied=qfrc_applied, nsub=nsub, eps=eps, fused=fused)
    gx = torch.zeros((n, nx, T + 1, nx), dtype=ctrl.dtype, device=ctrl.device)
    gx[:, :, T] = torch.eye(nx, dtype=ctrl.dtype, device=ctrl.device)
    lam, mu = _sweep(env, fd, gx.reshape(n * nx, T + 1, nx), None, None, None, nx, device)
    return {"dxT_du": mu.reshape(n, nx, T, -1), "dxT_dx0": lam[:, 0].reshape(n, nx, nx), "qpos": fd["qpos"], "qvel": fd["qvel"],
            "status": fd["status"], "status_fd": fd["status_fd"]}


def quat_tangent_basis(quat):
    """[.., 4, 3]: column k is quat (x) [0, e_k] (wxyz) -- twice the derivative of the quaternion along tangent column k, the
    body-frame convention of qvel's angular part (derivatives.tangent_perturb, KTransFdIn::eps).  For a unit quaternion the three
    columns are orthonormal and orthogonal to quat."""
    import torch
    w, x, y, z = quat.unbind(dim=-1)
    return torch.stack([torch.stack([-x, -y, -z], dim=-1), torch.stack([w, -z, y], dim=-1), torch.stack([z, w, -x], dim=-1),
                        torch.stack([-y, x, w], dim=-1)], dim=-2)


def ambient_to_tangent(cm, qpos, g_qpos):
    """[.., nv]: a gradient with respect to qpos [.., nq] as a gradient with respect to its tangent.  Joint and cube-position
    entries map as they are; for the cube's quaternion q, g_tan_k = g_q . (0.5 q (x) [0, e_k])."""
    import torch
    nl = cm.nlink
    rot = 0.5 * (g_qpos[..., None, nl + 3:nl + 7] @ quat_tangent_basis(qpos[..., nl + 3:nl + 7]))[..., 0, :]
    return torch.cat([g_qpos[..., :nl + 3], rot], dim=-1)


def tangent_to_ambient(cm, qpos, g_tan):
    """[.., nq]: the MINIMAL ambient gradient of a tangent gradient [.., nv] at qpos (a unit cube quaternion q): the one with no
    component along q itself, 2 q (x) [0, g_rot].  ambient_to_tangent maps it back to g_tan."""
    import torch
    nl = cm.nlink
    quat = 2.0 * (quat_tangent_basis(qpos[..., nl + 3:nl + 7]) @ g_tan[..., nl + 3:nl + 6, None])[..., 0]
    return torch.cat([g_tan[..., :nl + 3], quat], dim=-1)


@functools.lru_cache(maxsize=None)
def _rollout_function():
    import torch

    class _DiffRollout(torch.autograd.Function):
        @staticmethod
        def forward(ctx, qpos0, qvel0, ctrl, env, envs, warm0, opts):
            fd = trajectory_fd(env, envs, qpos0.detach(), qvel0.detach(), warm0, ctrl.detach(), qfrc_applied=opts["qfrc_applied"],
                               nsub=opts["nsub"], eps=opts["eps"], fused=opts["fused"])
            ctx.env, ctx.fd, ctx.device = env, fd, opts["device"]
            if opts.get("info") is not None:
                opts["info"].update(status=fd["status"], status_fd=fd["status_fd"])
            return fd["qpos"][:, 1:].clone(), fd["qvel"][:, 1:].clone()

        @staticmethod
        def backward(ctx, g_qpos, g_qvel):
            env, fd = ctx.env, ctx.fd
            cm = env.cm
            n, T = int(g_qpos.shape[0]), int(g_qpos.shape[1])
            gx = torch.zeros((n, T + 1, 2 * cm.nv), dtype=g_qpos.dtype, device=g_qpos.device)
            gx[:, 1:, :cm.nv] = ambient_to_tangent(cm, fd["qpos"][:, 1:], g_qpos)
            gx[:, 1:, cm.nv:] = g_qvel
            lam, mu = _sweep(env, fd, gx, None, None, None, 1, ctx.device)
            g_q0 = tangent_to_ambient(cm, fd["qpos"][:, 0], lam[:, 0, :cm.nv])
            return g_q0, lam[:, 0, cm.nv:].clone(), mu, None, None, None, None

    return _DiffRollout


def diff_rollout(env, envs, qpos0, qvel0, warm0, ctrl, qfrc_applied=None, nsub=None, eps=1e-6, fused=False, device=False, info=None):
    """env.rollout that autograd differentiates: returns (qpos [n, T, nq], qvel [n, T, nv]), the state after each step of the
    open-loop rollout of ctrl [n, T, nu] from (qpos0, qvel0, warm0), and loss.backward() on any function of the two reaches ctrl,
    qvel0 and qpos0.  Forward is one ilqr.trajectory_fd call (the rollout and the Jacobians of every step, kept for backward);
    backward is one adjoint sweep (device: env.adjoint, else derivatives.adjoint_pass).
    Backward maps the gradients it is handed, which are with respect to qpos's nq coordinates, to the tangent space
    (ambient_to_tangent: joints, cube position and velocities as they are, the quaternion through 0.5 q (x) [0, e_k], the
    body-frame convention of transition_fd's columns), and hands qpos0 the minimal ambient gradient 2 q (x) [0, lam_rot] (q taken as
    a unit quaternion).  Only first-order terms: the Jacobians are constants of the graph.
    warm0 gets no gradient (None): the solver's warm start is where its iteration begins, not a state of the system -- the
    converged step does not depend on it beyond the solver's tolerance.  qfrc_applied [n, nv] is held and not differentiated.
    info: a dict that receives status [n] and status_fd [n] of the forward call."""
    opts = dict(qfrc_applied=qfrc_applied, nsub=nsub, eps=eps, fused=fused, device=device, info=info)
    return _rollout_function().apply(qpos0, qvel0, ctrl, env, envs, warm0, opts)
