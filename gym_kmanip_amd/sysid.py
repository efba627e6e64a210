"""System identification on the step derivatives in the per-env physics parameters: what KManipEnvHip.param_fd
adds to the stack of ilqr.trajectory_fd (A_t = d x_{t+1} / d x_t), the adjoint sweep (the costates lam_t) and set_env_params.

trajectory_param_fd   P_t = d x_{t+1} / d p at every step of a trajectory, one param_fd call
param_grad            the gradient of a rollout loss in the parameters, sum_t P_t' lam_{t+1}
param_sensitivity     S_t = d x_t / d p, the forward recursion S_{t+1} = (A_t + B_t K_t) S_t + P_t
TrackingCost          1/2 sum_t dx_t' Q dx_t against an observed trajectory, with its residual
rollout_param_grad    cost, its gradient in the parameters (and controls, and initial state) in four calls
identify              Gauss-Newton with Levenberg-Marquardt damping on the parameters of n envs, one trajectory each

The state is (qpos in the tangent space, qvel), 2 nv wide, as transition_fd defines it; the parameters are model.ENV_PARAMS, the
columns always in that order.  Everything is torch arithmetic on the device of the caller's tensors.  With device=False it needs only
env.rollout, env.param_fd and env.cm (identify: also env.set_env_params and env.get_env_params), so a CPU stand-in
(tests/tools/paramfd_oracle.py OracleParamFd) runs the same code."""
from .derivatives import tangent_diff
from .grad import _sweep
from .ilqr import trajectory_fd
from .model import ENV_PARAMS


def _wrt(wrt):
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    unknown = set(wrt) - set(ENV_PARAMS)
    if unknown:
        raise ValueError("unknown env parameter(s) %s (known: %s)" % (sorted(unknown), ", ".join(ENV_PARAMS)))
    return tuple(name for name in ENV_PARAMS if name in wrt)


def trajectory_param_fd(env, fd, envs, ctrl, qfrc_applied=None, params=None, nsub=None, eps=1e-4, relative=True, wrt=ENV_PARAMS,
                        warm_offset=1.0, info=None):
    """P [n, T, 2 nv, npar]: d x_{t+1} / d p at every step of the trajectory `fd` (an ilqr.trajectory_fd result for ctrl [n, T, nu] and
    the same envs, qfrc_applied and nsub), ONE env.param_fd call over the n T start-of-step rows -- fd's qpos, qvel and warm, the rows
    trajectory_fd handed transition_fd.  params None: the values in force for the envs; else param_fd's, one row per problem
    ({name: [n]} or [n, KM_EP_N]).  info: a dict that receives status_cols [n, T, npar], status_fd [n] (the largest over the problem's
    steps and columns) and wrt, the columns' names."""
    import torch
    n, T = int(ctrl.shape[0]), int(ctrl.shape[1])
    dev = ctrl.device
    idx = torch.arange(n, dtype=torch.int32, device=dev) if envs is None else torch.as_tensor(envs).to(device=dev, dtype=torch.int32)
    flat = lambda t: t.reshape(n * T, t.shape[-1]).contiguous()
    rep = lambda t: torch.as_tensor(t, dtype=torch.float64).to(dev).expand(n).repeat_interleave(T)
    if isinstance(params, dict):
        params = {name: None if v is None else rep(v) for name, v in params.items()}
    elif params is not None:
        params = params.repeat_interleave(T, dim=0).contiguous()
    d = env.param_fd(envs=idx.repeat_interleave(T), qpos=flat(fd["qpos"][:, :-1]), qvel=flat(fd["qvel"][:, :-1]), ctrl=flat(ctrl),
                     warm=flat(fd["warm"]), qfrc_applied=None if qfrc_applied is None else qfrc_applied.repeat_interleave(T, dim=0),
                     params=params, nsub=nsub, eps=eps, relative=relative, wrt=wrt, warm_offset=warm_offset)
    npar = len(d["wrt"])
    if info is not None:
        info.update(status_cols=d["status_cols"].reshape(n, T, npar), status_fd=d["status_fd"].reshape(n, T).max(dim=1).values, wrt=d["wrt"])
    return d["P"].reshape(n, T, d["P"].shape[1], npar)


def param_grad(lam, P):
    """[n, npar]: sum_t P_t' lam_{t+1}, the gradient in the parameters of the loss whose costates are lam [n, T + 1, 2 nv] (the adjoint
    sweep's), P [n, T, 2 nv, npar].  The same lam is right open loop and under rollout_feedback's gains: the closed-loop sweep already
    carries the feedback."""
    import torch
    return torch.einsum("ntxp,ntx->np", P, lam[:, 1:])


def param_sensitivity(A, P, B=None, gains=None):
    """S [n, T + 1, 2 nv, npar]: d x_t / d p with x_0 held, S_0 = 0 and S_{t+1} = (A_t + B_t K_t) S_t + P_t (gains [n, T, nu, 2 nv] with
    B [n, T, 2 nv, nu]: the policy of rollout_feedback; without them the open-loop recursion).  A torch loop over the steps."""
    import torch
    if (B is None) != (gains is None):
        raise ValueError("param_sensitivity: give B and gains together")
    n, T, nx, npar = (int(s) for s in P.shape)
    S = torch.zeros((n, T + 1, nx, npar), dtype=P.dtype, device=P.device)
    for t in range(T):
        At = A[:, t] if gains is None else A[:, t] + B[:, t] @ gains[:, t]
        S[:, t + 1] = At @ S[:, t] + P[:, t]
    return S


class TrackingCost:
    """1/2 sum_{t <= T} dx_t' Q dx_t with dx_t = [tangent_diff(qpos_t, qpos_obs_t) ; qvel_t - qvel_obs_t]: the distance of a rollout to an
    observed trajectory qpos_obs [n, T + 1, nq], qvel_obs [n, T + 1, nv] (x_0 .. x_T).  Q [2 nv, 2 nv] or its diagonal [2 nv].
    ilqr.QuadraticCost's interface (total, derivatives; no control term: lu and luu are zeros) and its Gauss-Newton habit -- dx is
    taken as linear in the state's tangent -- plus residual, the dx itself."""

    def __init__(self, cm, qpos_obs, qvel_obs, Q):
        import torch
        self.cm, self.qpos_obs, self.qvel_obs = cm, qpos_obs, qvel_obs
        self.Q = torch.diag(Q) if Q.dim() == 1 else Q

    def residual(self, qpos, qvel):
        """dx [n, T + 1, 2 nv] of states qpos [n, T + 1, nq], qvel [n, T + 1, nv]."""
        import torch
        n, L = int(qpos.shape[0]), int(qpos.shape[1])
        dq = tangent_diff(self.cm, qpos.reshape(n * L, -1), self.qpos_obs.reshape(n * L, -1)).reshape(n, L, -1)
        return torch.cat([dq, qvel - self.qvel_obs], dim=2)

    def total(self, qpos, qvel, ctrl=None):
        d = self.residual(qpos, qvel)
        return 0.5 * ((d @ self.Q) * d).sum(dim=(1, 2))

    def derivatives(self, qpos, qvel, ctrl):
        """(lx [n, T + 1, 2 nv], lu [n, T, nu] zeros, lxx [T + 1, 2 nv, 2 nv], luu [T, nu, nu] zeros)."""
        import torch
        d = self.residual(qpos, qvel)
        T, nu = int(ctrl.shape[1]), int(ctrl.shape[2])
        sym = 0.5 * (self.Q + self.Q.transpose(0, 1))
        return (d @ sym, torch.zeros_like(ctrl), sym[None].expand(T + 1, -1, -1),
                torch.zeros((T, nu, nu), dtype=ctrl.dtype, device=ctrl.device))


def rollout_param_grad(env, envs, qpos0, qvel0, warm0, ctrl, cost, wrt=ENV_PARAMS, qfrc_applied=None, nsub=None, eps=1e-6, eps_param=1e-4,
                       relative=True, fused=False, device=False):
    """The gradient of cost.total over the rollout of ctrl [n, T, nu] from (qpos0, qvel0, warm0) in the parameters of the envs: ONE
    ilqr.trajectory_fd call, one cost.derivatives call, one adjoint sweep (grad.py's: device=True is env.adjoint) and ONE env.param_fd
    call.  Returns a dict: cost [n]; grad_params [n, npar] (columns: the entry wrt); grad_ctrl [n, T, nu]; grad_x0 [n, 2 nv]; P [n, T, 2
    nv, npar]; A and B, the step Jacobians the sweep used; lam [n, T + 1, 2 nv]; qpos, qvel; status and status_fd [n] (trajectory_fd's) and status_param [n] (param_fd's largest
    column status over the problem's steps).  A row with a nonzero status has no gradient worth the name.  eps is transition_fd's,
    eps_param / relative param_fd's."""
    fd = trajectory_fd(env, envs, qpos0, qvel0, warm0, ctrl, qfrc_applied=qfrc_applied, nsub=nsub, eps=eps, fused=fused)
    lx, lu = cost.derivatives(fd["qpos"], fd["qvel"], ctrl)[:2]
    lam, mu = _sweep(env, fd, lx, lu, None, None, 1, device)
    info = {}
    P = trajectory_param_fd(env, fd, envs, ctrl, qfrc_applied=qfrc_applied, nsub=nsub, eps=eps_param, relative=relative, wrt=wrt, info=info)
    return {"cost": cost.total(fd["qpos"], fd["qvel"], ctrl), "grad_params": param_grad(lam, P), "grad_ctrl": mu, "grad_x0": lam[:, 0],
            "P": P, "A": fd["A"], "B": fd["B"], "lam": lam, "qpos": fd["qpos"], "qvel": fd["qvel"], "status": fd["status"], "status_fd": fd["status_fd"],
            "status_param": info["status_fd"], "wrt": info["wrt"]}


def _scaled_jacobian(cost, S, scale):
    """J [n, (T + 1) 2 nv, npar] = W^(1/2) S with column j times scale[:, j], and W^(1/2) [2 nv, 2 nv] (W = cost.Q = L L', W^(1/2) = L')."""
    import torch
    Q = 0.5 * (cost.Q + cost.Q.transpose(0, 1))
    d = torch.diagonal(Q)
    if torch.equal(Q, torch.diag(d)):
        half = torch.diag(torch.sqrt(d))
    else:
        half = torch.linalg.cholesky(Q).transpose(0, 1)
    n, L, nx, npar = (int(s) for s in S.shape)
    J = (half @ S) * scale[:, None, None, :]
    return J.reshape(n, L * nx, npar), half


def identify(env, envs, qpos0, qvel0, warm0, ctrl, qpos_obs, qvel_obs, wrt=ENV_PARAMS, iters=8, Q=None, qfrc_applied=None, nsub=None,
             eps=1e-6, eps_param=1e-4, fused=False, damping=0.1, damping_up=10.0, damping_down=0.1, min_factor=0.5, max_factor=2.0, callback=None):
    """Estimates the parameters `wrt` of envs [n] (no entry repeated) from one observed trajectory each: qpos_obs [n, T + 1, nq],
    qvel_obs [n, T + 1, nv], the states x_0 .. x_T that ctrl [n, T, nu] produced from (qpos0, qvel0, warm0).  Each problem estimates
    the parameters of its own env, starting from the values the handle has in force.
    THE HANDLE'S PARAMETERS ARE CHANGED: every candidate is written with env.set_env_params, and on return the envs hold the estimate.
    A handle in ranges mode is refused (a reset would redraw what is being estimated).
    Per iteration: one trajectory_fd call (fused: its switch), one param_fd call, the sensitivity recursion, then the step
      d = -(J'J + mu diag(J'J))^-1 J' r,   J = W^(1/2) S with column j scaled by p_j,   r = W^(1/2) dx   (W = Q, default the identity)
    so that d is a RELATIVE change, p <- p (1 + d), held within [min_factor, max_factor] p: no iterate moves a parameter by more than a
    factor of two, and every value stays inside its domain (mass and kp scale > 0; friction and friction loss start above 0 and stay there -- the derivative AT 0 does not exist).  The candidate is
    evaluated by one env.rollout; a problem accepts it only if its loss falls (mu <- mu damping_down), else it keeps its values and
    mu <- mu damping_up.  The start is damped (mu = 0.1): from the model's defaults an undamped first step overshoots in the grasp cell
    and the rejections that follow use up the iterations.
    Returns a dict: params {name: [n]} the estimate (all of ENV_PARAMS); wrt; loss [iters + 1, n] the loss before every iteration and
    after the last; accepted [iters, n] bool; singular_values [n, npar] of the scaled J at the last iterate, descending -- a ratio
    near zero says that a direction in parameter space is not observable from this trajectory (a cube in flight shows only a combination of its mass
    and friction loss); status [n] the largest rollout / linearisation / param_fd status met.
    callback(iteration, params [n, npar], loss [n], singular_values [n, npar]) is called with every linearisation."""
    import torch
    cm = env.cm
    order = _wrt(wrt)
    if getattr(env, "_ep_ranges", None) is not None:
        raise ValueError("identify: the handle is in ranges mode (a reset would redraw the parameters): call set_env_param_ranges() first")
    n, T = int(ctrl.shape[0]), int(ctrl.shape[1])
    dev = ctrl.device
    idx = torch.as_tensor(envs).to(device=dev, dtype=torch.int64).reshape(-1)
    if int(idx.shape[0]) != n or len(set(idx.tolist())) != n:
        raise ValueError("identify: envs must name %d different envs, one per problem" % n)
    cols = [ENV_PARAMS.index(name) for name in order]
    Qm = torch.ones(2 * cm.nv, dtype=ctrl.dtype, device=dev) if Q is None else Q
    cost = TrackingCost(cm, qpos_obs, qvel_obs, Qm)
    full = torch.stack([v.to(dev) for v in env.get_env_params().values()], dim=1).clone()        # [num_envs, KM_EP_N]

    def write(p_rows):
        full[idx] = p_rows
        env.set_env_params(**{name: full[:, k].contiguous() for k, name in enumerate(ENV_PARAMS)})

    def linearise():
        fd = trajectory_fd(env, idx.to(torch.int32), qpos0, qvel0, warm0, ctrl, qfrc_applied=qfrc_applied, nsub=nsub, eps=eps, fused=fused)
        info = {}
        P = trajectory_param_fd(env, fd, idx.to(torch.int32), ctrl, qfrc_applied=qfrc_applied, nsub=nsub, eps=eps_param, wrt=order, info=info)
        S = param_sensitivity(fd["A"], P)
        J, half = _scaled_jacobian(cost, S, p[:, cols])
        r = (cost.residual(fd["qpos"], fd["qvel"]) @ half.transpose(0, 1)).reshape(n, -1)
        st = torch.maximum(torch.maximum(fd["status"], fd["status_fd"]), info["status_fd"])
        return J, r, 0.5 * (r * r).sum(dim=1), st

    p = full[idx].clone()                                # [n, KM_EP_N]
    mu = torch.full((n,), float(damping), dtype=ctrl.dtype, device=dev)
    losses, accepted = [], []
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    for it in range(iters):
        J, r, loss, st = linearise()
        status = torch.maximum(status, st)
        sv = torch.linalg.svdvals(J)
        if callback is not None:
            callback(it, p[:, cols].clone(), loss.clone(), sv)
        losses.append(loss)
        H = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[:, :, None])[:, :, 0]
        dg = torch.diagonal(H, dim1=1, dim2=2)
        dg = torch.where(dg > 0, dg, torch.ones_like(dg))
        d = -torch.linalg.solve(H + torch.diag_embed(mu[:, None] * dg), g)
        d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
        cand = p.clone()
        cand[:, cols] = p[:, cols] * torch.clamp(1.0 + d, min=min_factor, max=max_factor)
        write(cand)
        roll = env.rollout(envs=idx.to(torch.int32), qpos=qpos0, qvel=qvel0, warm=warm0, ctrl=ctrl, qfrc_applied=qfrc_applied, nsub=nsub,
                           fields=("qpos", "qvel", "status"))
        new = cost.total(torch.cat([qpos0[:, None], roll["qpos"]], dim=1), torch.cat([qvel0[:, None], roll["qvel"]], dim=1))
        ok = (roll["status"] == 0) & (new < loss)
        accepted.append(ok)
        p = torch.where(ok[:, None], cand, p)
        mu = torch.where(ok, mu * damping_down, mu * damping_up)
        if not bool(ok.all()):
            write(p)                                     # the problems that refused their candidate keep their values
    J, r, loss, st = linearise()
    status = torch.maximum(status, st)
    sv = torch.linalg.svdvals(J)
    if callback is not None:
        callback(iters, p[:, cols].clone(), loss.clone(), sv)
    losses.append(loss)
    return {"params": {name: p[:, k].clone() for k, name in enumerate(ENV_PARAMS)}, "wrt": order, "loss": torch.stack(losses),
            "accepted": torch.stack(accepted) if accepted else torch.zeros((0, n), dtype=torch.bool, device=dev),
            "singular_values": sv, "status": status}
