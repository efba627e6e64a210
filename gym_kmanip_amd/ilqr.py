"""iLQR in ctrl space over KManipEnvHip.rollout, derivatives.transition_fd and KManipEnvHip.rollout_feedback.

One iteration is three device calls whatever the horizon T: the nominal trajectory (one rollout launch), its linearisation
(transition_fd over all n T start-of-step states as rows: two launches), and the line search -- the backward pass's policy
u_t = u_t + alpha k_t + K_t (x_t - x_t_nominal) rolled out CLOSED LOOP for every step size alpha at once, one rollout_feedback launch
of n len(alphas) rows that share the n gain trajectories through gain_index.

The state is (qpos in the tangent space, qvel), 2 nv wide, as transition_fd defines it; differences of states are
derivatives.tangent_diff's.  The cost is an object with total() and derivatives(): QuadraticCost (a goal state in joint space), SiteCost (a
goal pose of the end-effector sites in task space) or a SumCost of such.  Everything is torch arithmetic on the device of the caller's tensors and needs only env.rollout,
env.rollout_feedback, env.cm and that device, so a CPU stand-in (tests/tools/feedback_oracle.py OracleFeedback) runs the same code."""
import functools

from .derivatives import tangent_diff, transition_fd


def _start_states(first, records):
    """[n, T, w]: the state BEFORE each step -- the initial row, then records 0 .. T-2 (record t is the state after step t)."""
    import torch
    return torch.cat([first[:, None], records[:, :-1]], dim=1)


def trajectory_fd(env, envs, qpos0, qvel0, warm0, ctrl, qfrc_applied=None, nsub=None, eps=1e-6, fused=False):
    """The nominal trajectory of ctrl [n, T, nu] from (qpos0, qvel0, warm0) and its linearisation at every step.  One rollout launch,
    then ONE transition_fd call over the n T start-of-step states as rows (row e T + t names env envs[e]; its warm start is the
    trajectory's qacc_warm before that step).  envs None: row e is env e.  qfrc_applied [n, nv], held, or None.  Returns a dict:
      A [n, T, 2 nv, 2 nv], B [n, T, 2 nv, nu]       d x_{t+1} / d x_t, d x_{t+1} / d u_t
      qpos [n, T + 1, nq], qvel [n, T + 1, nv]       x_0 .. x_T (x_t: the state before step t)
      warm [n, T, nv]                                 the warm start of every step
      status [n] uint8                                the nominal rollout's; status_fd [n]: the largest over the row's steps
    fused=True: the linearisation is env.transition_fd (kmanip_transition_fd: the rows perturbed and differenced inside the kernel,
    DESIGN.md section 31) in place of derivatives.transition_fd over env.rollout; the same rows, the same arithmetic per row.  Where
    that call returns its buffer, the dict also has deriv_t [n, T, 2 nv + nu, 2 nv], a view of it: what A and B are transposed views
    of, and what env.lqr_backward reads without a copy."""
    import torch
    cm = env.cm
    n, T = int(ctrl.shape[0]), int(ctrl.shape[1])
    dev = ctrl.device
    idx = torch.arange(n, dtype=torch.int32, device=dev) if envs is None else torch.as_tensor(envs).to(device=dev, dtype=torch.int32)
    roll = env.rollout(envs=idx, qpos=qpos0, qvel=qvel0, warm=warm0, ctrl=ctrl, qfrc_applied=qfrc_applied, nsub=nsub,
                       fields=("qpos", "qvel", "qacc_warm", "status"))
    qs, vs, ws = _start_states(qpos0, roll["qpos"]), _start_states(qvel0, roll["qvel"]), _start_states(warm0, roll["qacc_warm"])
    flat = lambda t: t.reshape(n * T, t.shape[-1]).contiguous()
    linearise = env.transition_fd if fused else functools.partial(transition_fd, env)
    d = linearise(envs=idx.repeat_interleave(T), qpos=flat(qs), qvel=flat(vs), ctrl=flat(ctrl), warm=flat(ws),
                  qfrc_applied=None if qfrc_applied is None else qfrc_applied.repeat_interleave(T, dim=0), nsub=nsub, eps=eps)
    nx = 2 * cm.nv
    out = {"A": d["A"].reshape(n, T, nx, nx), "B": d["B"].reshape(n, T, nx, cm.nu),
           "qpos": torch.cat([qpos0[:, None], roll["qpos"]], dim=1), "qvel": torch.cat([qvel0[:, None], roll["qvel"]], dim=1), "warm": ws,
           "status": roll["status"], "status_fd": torch.maximum(d["status"], d["status_fd"]).reshape(n, T).max(dim=1).values}
    if fused and "deriv_t" in d:
        out["deriv_t"] = d["deriv_t"].reshape(n, T, nx + cm.nu, nx)
    return out


class QuadraticCost:
    """sum_{t < T} 1/2 (dx_t' Q dx_t + u_t' R u_t) + 1/2 dx_T' Qf dx_T with dx = [tangent_diff(qpos, goal_qpos) ; qvel - goal_qvel]:
    the distance to a goal state measured in the tangent space.  goal_qpos [n, nq] (or [nq]), goal_qvel [n, nv] (or [nv]); Q, Qf
    [2 nv, 2 nv] or their diagonals [2 nv]; R [nu, nu] or [nu].  The derivatives treat dx as linear in the state's tangent (exact
    for joints, cube position and velocities; for the cube's rotation the log map's Jacobian is taken as the identity, the
    Gauss-Newton habit -- weigh the rotation columns with zeros for a joint-space goal and nothing is approximated)."""

    def __init__(self, cm, goal_qpos, goal_qvel, Q, R, Qf):
        import torch
        self.cm = cm
        mat = lambda m: torch.diag(m) if m.dim() == 1 else m
        self.goal_qpos, self.goal_qvel = goal_qpos.reshape(-1, cm.nq), goal_qvel.reshape(-1, cm.nv)
        self.Q, self.R, self.Qf = mat(Q), mat(R), mat(Qf)

    def dx(self, qpos, qvel):
        """[n, L, 2 nv] of states [n, L, nq] / [n, L, nv] (n rows against the goal's n, or its one row)."""
        import torch
        n, L = int(qpos.shape[0]), int(qpos.shape[1])
        reps = n // int(self.goal_qpos.shape[0])
        gq = self.goal_qpos.repeat(reps, 1)[:, None].expand(n, L, -1).reshape(n * L, -1)
        dq = tangent_diff(self.cm, qpos.reshape(n * L, -1), gq).reshape(n, L, -1)
        return torch.cat([dq, qvel - self.goal_qvel.repeat(reps, 1)[:, None]], dim=2)

    def total(self, qpos, qvel, ctrl):
        """[n]: the cost of trajectories qpos [n, T + 1, nq], qvel [n, T + 1, nv] (x_0 .. x_T) under ctrl [n, T, nu]."""
        d = self.dx(qpos, qvel)
        run = 0.5 * ((d[:, :-1] @ self.Q) * d[:, :-1]).sum(dim=(1, 2)) + 0.5 * ((ctrl @ self.R) * ctrl).sum(dim=(1, 2))
        return run + 0.5 * ((d[:, -1] @ self.Qf) * d[:, -1]).sum(dim=1)

    def derivatives(self, qpos, qvel, ctrl):
        """(lx [n, T + 1, 2 nv], lu [n, T, nu], lxx [T + 1, 2 nv, 2 nv], luu [T, nu, nu]) along a trajectory; entry T of lx / lxx is
        the final cost's."""
        import torch
        d = self.dx(qpos, qvel)
        T = int(ctrl.shape[1])
        lxx = torch.cat([self.Q[None].expand(T, -1, -1), self.Qf[None]], dim=0)
        lx = torch.einsum("tij,ntj->nti", lxx, d)
        return lx, ctrl @ self.R.transpose(0, 1), lxx, self.R[None].expand(T, -1, -1)


def _mat2quat(m):
    """wxyz [.., 4] of rotation matrices [.., 9] (row-major), normalised: mju_mat2Quat's four cases, chosen as the kernels' mat2quat
    chooses them (the trace if positive, else the largest diagonal entry)."""
    import torch
    m0, m1, m2, m3, m4, m5, m6, m7, m8 = m.unbind(dim=-1)
    tr = m0 + m4 + m8
    case = torch.where(tr > 0, 0, torch.where((m0 > m4) & (m0 > m8), 1, torch.where(m4 > m8, 2, 3)))
    arg = torch.stack([1 + tr, 1 + m0 - m4 - m8, 1 - m0 + m4 - m8, 1 - m0 - m4 + m8], dim=-1).gather(-1, case[..., None])[..., 0]
    r = 0.5 * torch.sqrt(arg)
    s = 0.25 / r
    d75, d26, d31, s13, s26, s57 = s * (m7 - m5), s * (m2 - m6), s * (m3 - m1), s * (m1 + m3), s * (m2 + m6), s * (m5 + m7)
    cands = torch.stack([torch.stack([r, d75, d26, d31], dim=-1), torch.stack([d75, r, s13, s26], dim=-1),
                         torch.stack([d26, s13, r, s57], dim=-1), torch.stack([d31, s26, s57, r], dim=-1)], dim=-2)
    q = cands.gather(-2, case[..., None, None].expand(case.shape + (1, 4)))[..., 0, :]
    return q / q.norm(dim=-1, keepdim=True)


def _rotation_error(qs, qt):
    """[.., 3]: the world-frame rotation vector (angle in (-pi, pi]) of qs (x) conj(qt), unit quaternions wxyz -- the rotation that
    takes the frame qt to the frame qs.  derivatives.tangent_diff's atan2 form (no division by zero at the identity) on a = conj(qs),
    b = conj(qt): conj(a) (x) b is that product."""
    import math
    import torch
    wa, xa, ya, za = qs[..., 0], -qs[..., 1], -qs[..., 2], -qs[..., 3]
    wb, xb, yb, zb = qt[..., 0], -qt[..., 1], -qt[..., 2], -qt[..., 3]
    w = wa * wb + xa * xb + ya * yb + za * zb
    x = (wa * xb - xa * wb) + (za * yb - ya * zb)
    y = (wa * yb - ya * wb) + (xa * zb - za * xb)
    z = (wa * zb - za * wb) + (ya * xb - xa * yb)
    sn = torch.sqrt(x * x + y * y + z * z)
    ang = 2.0 * torch.atan2(sn, w)
    ang = torch.where(ang > math.pi, ang - 2.0 * math.pi, ang)
    k = torch.where(sn > 0, ang / torch.where(sn > 0, sn, torch.ones_like(sn)), 2.0 / torch.where(w != 0, w, torch.ones_like(w)))
    return torch.stack([k * x, k * y, k * z], dim=-1)


def site_cost_rows(env, envs, qpos, qvel, target_pos, target_quat, weight, follow_cube, want_derivatives=True):
    """THE DEFINITION kmanip_site_cost is held to (include/kmanip.h KSiteCostIn states the formulas): one
    env.kinematics_at call over the N rows (envs [N] int32, qpos [N, nq], qvel [N, nv]) and torch arithmetic on target_pos [N, 2, 3],
    target_quat [N, 2, 4] or None, weight [N, 2, 2] and follow_cube (two bools).  Returns dict(cost [N], status [N] and, if wanted, lx
    [N, 2 nv], lxx [N, 2 nv, 2 nv]); a row with status != 0 is zeros."""
    import torch
    cm = env.cm
    nl, nv = cm.nlink, cm.nv
    q, tp, tq, w = qpos, target_pos, target_quat, weight
    N = int(q.shape[0])
    present = torch.tensor([bool(cm.desc.arm_present[a]) for a in range(2)], device=q.device)
    k = env.kinematics_at(envs=envs, qpos=q, qvel=qvel, fields=SiteCost.FIELDS)
    ok = (k["status"] == 0)
    f = torch.tensor([float(bool(x)) for x in follow_cube], dtype=q.dtype, device=q.device)
    zero = torch.zeros((), dtype=q.dtype, device=q.device)
    w0 = torch.where(present[None], w[:, :, 0], zero)
    w1 = torch.where(present[None], w[:, :, 1], zero) if tq is not None else torch.zeros_like(w0)
    e_pos = torch.where(present[None, :, None], k["site_xpos"] - (tp + f[None, :, None] * q[:, None, nl:nl + 3]), zero)
    if tq is None:
        e_rot = torch.zeros_like(e_pos)
    else:
        eye = torch.eye(3, dtype=q.dtype, device=q.device).reshape(1, 1, 9)
        use = ok[:, None] & (w1 != 0)
        unit = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=q.dtype, device=q.device)
        qt = torch.where(use[:, :, None], tq, unit)
        e_rot = _rotation_error(_mat2quat(torch.where(use[:, :, None], k["site_xmat"], eye)), qt / qt.norm(dim=-1, keepdim=True))
        e_rot = torch.where(use[:, :, None], e_rot, zero)
    cost = 0.5 * (w0 * (e_pos * e_pos).sum(dim=-1) + w1 * (e_rot * e_rot).sum(dim=-1)).sum(dim=1)
    bad = ~(torch.isfinite(cost))
    status = torch.where(ok & bad, torch.ones_like(k["status"]), k["status"])      # (a non-finite target or weight of a present arm)
    ok = status == 0
    out = {"cost": torch.where(ok, cost, zero), "status": status}
    if want_derivatives:
        Jp, Jr = k["site_jacp"].clone(), k["site_jacr"]
        for c in range(3):
            Jp[:, :, c, nl + c] = -f * present.to(q.dtype)
        lx = torch.zeros((N, 2 * nv), dtype=q.dtype, device=q.device)
        lxx = torch.zeros((N, 2 * nv, 2 * nv), dtype=q.dtype, device=q.device)
        lx[:, :nv] = torch.einsum("ra,rac,racj->rj", w0, e_pos, Jp) + torch.einsum("ra,rac,racj->rj", w1, e_rot, Jr)
        lxx[:, :nv, :nv] = torch.einsum("ra,raci,racj->rij", w0, Jp, Jp) + torch.einsum("ra,raci,racj->rij", w1, Jr, Jr)
        out.update(lx=torch.where(ok[:, None], lx, zero), lxx=torch.where(ok[:, None, None], lxx, zero))
    return out


class SiteCost:
    """sum_{t <= T} 1/2 sum_a (w_pos[a] |e_pos_a(x_t)|^2 + w_rot[a] |e_rot_a(x_t)|^2) over the present arms a, the final state with
    wf_pos / wf_rot: the distance of the end-effector sites to a target pose, in task space (DESIGN.md section 40;
    include/kmanip.h KSiteCostIn states e_pos, e_rot, the gradient and the Gauss-Newton Hessian).
    target_pos [n0, arms, 3], or [n0, T + 1, arms, 3] for a trajectory to track; target_quat likewise with 4 (wxyz), or None: no
    rotation term.  arms: the present arms in order, or 2 (the slots of an absent arm are ignored).  Problem e is env e (n0 <=
    num_envs); rows beyond n0 repeat the targets as QuadraticCost.dx repeats its goal: row a n0 + e uses entry e.  w_pos, w_rot: a
    number or one per arm; wf_pos, wf_rot: the final state's, default the running ones.  follow_cube (a bool or one per arm): the
    target position is an offset from the cube's position, and the cost then also pulls on the cube's position columns.
    device=False: env.kinematics_at and torch arithmetic -- the definition kmanip_site_cost is held to; it needs only
    env.kinematics_at and env.cm, so a CPU stand-in serves it.  device=True: one env.site_cost launch per call."""

    FIELDS = ("site_xpos", "site_xmat", "site_jacp", "site_jacr", "status")

    def __init__(self, env, target_pos, target_quat=None, w_pos=1.0, w_rot=0.0, wf_pos=None, wf_rot=None, follow_cube=False, device=False):
        import torch
        self.env, self.cm, self.device = env, env.cm, bool(device)
        present = [a for a in range(2) if self.cm.desc.arm_present[a]]
        dt, dev = target_pos.dtype, target_pos.device

        def slots(t, width):                      # [n0, (T + 1,) arms, width] -> [n0, T + 1 or 1, 2, width]
            if t.dim() == 3:
                t = t[:, None]
            if t.shape[2] == 2:
                return t
            assert t.shape[2] == len(present), "one target per present arm, or two"
            out = torch.zeros(t.shape[:2] + (2, width), dtype=dt, device=dev)
            out[:, :, present] = t
            if width == 4:
                out[..., 0] = torch.where(out.abs().sum(dim=-1) == 0, torch.ones_like(out[..., 0]), out[..., 0])
            return out

        def per_arm(v):                           # a number or [arms] -> [2], zeros at an absent arm
            v = torch.as_tensor(v, dtype=dt, device=dev).reshape(-1)
            out = torch.zeros(2, dtype=dt, device=dev)
            out[present] = v.expand(len(present)) if v.numel() == 1 else (v if v.numel() == len(present) else v[present])
            return out
        self.target_pos = slots(target_pos, 3)
        self.target_quat = None if target_quat is None else slots(target_quat, 4)
        wr = per_arm(w_rot) if target_quat is not None else torch.zeros(2, dtype=dt, device=dev)
        wfr = wr if wf_rot is None or target_quat is None else per_arm(wf_rot)
        wp = per_arm(w_pos)
        self.w_run, self.w_final = torch.stack([wp, wr], dim=1), torch.stack([wp if wf_pos is None else per_arm(wf_pos), wfr], dim=1)
        fc = (follow_cube, follow_cube) if isinstance(follow_cube, (bool, int)) else tuple(follow_cube)
        self.follow_cube = tuple(bool(f) and a in present for a, f in zip(range(2), fc))

    def _rows(self, n, L):
        """(env index [n L] int32, target_pos [n L, 2, 3], target_quat [n L, 2, 4] or None, weight [n L, 2, 2]) of n trajectories of
        L states, the last one the final state."""
        import torch
        n0 = int(self.target_pos.shape[0])
        reps = n // n0
        assert reps * n0 == n, "the rows are a multiple of the targets"
        spread = lambda t: t.repeat(reps, 1, 1, 1).expand(n, L, 2, t.shape[-1]).reshape(n * L, 2, t.shape[-1]).contiguous()
        w = torch.cat([self.w_run[None].expand(L - 1, 2, 2), self.w_final[None]], dim=0)
        idx = torch.arange(n0, dtype=torch.int32, device=self.target_pos.device).repeat(reps).repeat_interleave(L)
        return idx, spread(self.target_pos), None if self.target_quat is None else spread(self.target_quat), \
            w[None].expand(n, L, 2, 2).reshape(n * L, 2, 2).contiguous()

    def _evaluate(self, qpos, qvel, want_derivatives):
        """dict(cost [n, L], status [n, L] and, if wanted, lx [n, L, nx], lxx [n, L, nx, nx]) of states qpos [n, L, nq], qvel [n, L, nv]."""
        n, L = int(qpos.shape[0]), int(qpos.shape[1])
        idx, tp, tq, w = self._rows(n, L)
        q = qpos.reshape(n * L, -1).contiguous()
        if self.device:
            r = self.env.site_cost(tp, w, envs=idx, qpos=q, target_quat=tq, follow_cube=self.follow_cube,
                                   fields=("cost", "lx", "lxx", "status") if want_derivatives else ("cost", "status"))
            return {k: v.reshape((n, L) + tuple(v.shape[1:])) for k, v in r.items()}
        r = site_cost_rows(self.env, idx, q, qvel.reshape(n * L, -1).contiguous(), tp, tq, w, self.follow_cube, want_derivatives)
        return {k: v.reshape((n, L) + tuple(v.shape[1:])) for k, v in r.items()}

    def total(self, qpos, qvel, ctrl):
        """[n]: the cost of trajectories qpos [n, T + 1, nq], qvel [n, T + 1, nv]; inf where any state of the trajectory has status != 0."""
        import torch
        r = self._evaluate(qpos, qvel, False)
        c = r["cost"].sum(dim=1)
        return torch.where((r["status"] == 0).all(dim=1), c, torch.full_like(c, float("inf")))

    def derivatives(self, qpos, qvel, ctrl):
        """(lx [n, T + 1, 2 nv], lu zeros [n, T, nu], lxx [n, T + 1, 2 nv, 2 nv] per problem, luu zeros [T, nu, nu])."""
        import torch
        r = self._evaluate(qpos, qvel, True)
        T, nu = int(ctrl.shape[1]), int(ctrl.shape[2])
        return r["lx"], torch.zeros_like(ctrl), r["lxx"], torch.zeros((T, nu, nu), dtype=ctrl.dtype, device=ctrl.device)


class SumCost:
    """The sum of costs with QuadraticCost's two methods: totals and derivatives added, a shared lxx [T + 1, nx, nx] / luu [T, nu, nu]
    broadcast against a per-problem [n, T + 1, nx, nx] / [n, T, nu, nu]."""

    def __init__(self, *costs):
        assert costs, "at least one cost"
        self.costs = costs

    def total(self, qpos, qvel, ctrl):
        out = self.costs[0].total(qpos, qvel, ctrl)
        for c in self.costs[1:]:
            out = out + c.total(qpos, qvel, ctrl)
        return out

    def derivatives(self, qpos, qvel, ctrl):
        out = self.costs[0].derivatives(qpos, qvel, ctrl)
        for c in self.costs[1:]:
            out = tuple(a + b for a, b in zip(out, c.derivatives(qpos, qvel, ctrl)))
        return out


def backward_pass(A, B, lx, lu, lxx, luu, reg=0.0):
    """The batched Riccati recursion of iLQR.  A [n, T, nx, nx], B [n, T, nx, nu]; lx [n, T + 1, nx], lu [n, T, nu], lxx
    [n or 1 .., T + 1, nx, nx] and luu [.., T, nu, nu] (a leading batch dimension is optional), entry T of lx / lxx the final cost's;
    no cross term.  reg: Levenberg regularisation added to the diagonal of Quu, a number or [n].  Returns (k [n, T, nu],
    K [n, T, nu, nx], dV [n, 2]): the policy du_t = alpha k_t + K_t dx_t and the expected reduction of the cost for a step alpha,
    -(alpha dV[:, 0] + alpha^2 dV[:, 1])."""
    import torch
    n, T, nx, nu = B.shape
    if lxx.dim() == 3:
        lxx = lxx[None]
    if luu.dim() == 3:
        luu = luu[None]
    reg = torch.as_tensor(reg, dtype=A.dtype, device=A.device).reshape(-1, 1, 1)
    eye = torch.eye(nu, dtype=A.dtype, device=A.device)
    Vx, Vxx = lx[:, T], lxx[:, T].expand(n, nx, nx)
    k, K = torch.zeros_like(lu), torch.zeros((n, T, nu, nx), dtype=A.dtype, device=A.device)
    dV = torch.zeros((n, 2), dtype=A.dtype, device=A.device)
    for t in range(T - 1, -1, -1):
        At, Bt = A[:, t], B[:, t]
        AtT, BtT = At.transpose(1, 2), Bt.transpose(1, 2)
        Qx = lx[:, t] + (AtT @ Vx[:, :, None])[:, :, 0]
        Qu = lu[:, t] + (BtT @ Vx[:, :, None])[:, :, 0]
        Qxx = lxx[:, t] + AtT @ Vxx @ At
        Quu = luu[:, t] + BtT @ Vxx @ Bt
        Qux = BtT @ Vxx @ At
        sol = torch.linalg.solve(Quu + reg * eye, torch.cat([Qu[:, :, None], Qux], dim=2))
        kt, Kt = -sol[:, :, 0], -sol[:, :, 1:]
        KtT = Kt.transpose(1, 2)
        Vx = Qx + (KtT @ (Quu @ kt[:, :, None] + Qu[:, :, None]) + Qux.transpose(1, 2) @ kt[:, :, None])[:, :, 0]
        Vxx = Qxx + KtT @ Quu @ Kt + KtT @ Qux + Qux.transpose(1, 2) @ Kt
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
        dV[:, 0] += (kt * Qu).sum(dim=1)
        dV[:, 1] += 0.5 * (kt * (Quu @ kt[:, :, None])[:, :, 0]).sum(dim=1)
        k[:, t], K[:, t] = kt, Kt
    return k, K, dV


# the constants of the box QP (Tassa, Mansard, Todorov, "Control-limited differential dynamic programming", ICRA 2014): parameters of the
# published algorithm, the same in kmanip_lqr_box.hip
BOXQP_ITERS, BOXQP_TRIALS, BOXQP_ARMIJO, BOXQP_STEP = 100, 100, 0.1, 0.6


def box_qp(H, q, bl, bh):
    """min_d 0.5 d'H d + q'd subject to bl <= d <= bh for n problems at once, H [n, nu, nu], the rest [n, nu]: the projected-Newton
    box QP of control-limited DDP, the iteration include/kmanip.h KLqrBoxIn states -- from d = clip(0, bl, bh): the gradient, the
    clamped set c, the Cholesky factor of H with the unit row and column at c, the Newton step on the free coordinates, a projected
    Armijo line search.  A problem has converged when its last step was a full one that the clip left alone and c is the set that
    step was factorised for, when every coordinate is clamped, or when the step is no descent direction (s . g >= 0: the face's exact
    minimiser).  No gradient threshold enters.  A Python loop over the iterations, every problem masked once it is done.
    Returns (d [n, nu], c [n, nu] bool, L [n, nu, nu] the factor for the final c, iters [n], status [n]: 0, 1 a pivot that is
    not > 0 or not finite / a box with bl <= bh false / a step that is not finite, 3 the iteration or line-search cap)."""
    import torch
    n, nu = q.shape
    eye = torch.eye(nu, dtype=q.dtype, device=q.device).expand(n, nu, nu)
    value = lambda x: (x * (0.5 * (H @ x[:, :, None])[:, :, 0] + q)).sum(dim=1)
    clip = lambda x: torch.where(x < bl, bl, torch.where(x > bh, bh, x))
    status = torch.where((bl <= bh).all(dim=1), 0, 1).to(torch.uint8)
    done = status != 0
    d = clip(torch.zeros_like(q))
    v = value(d)
    moved = torch.ones(n, dtype=torch.bool, device=q.device)
    have = torch.zeros_like(moved)                       # a factor exists, for the set cf
    c = cf = torch.zeros_like(q, dtype=torch.bool)
    L = eye.clone()
    iters = torch.zeros(n, dtype=torch.int32, device=q.device)
    for it in range(BOXQP_ITERS + 1):
        g = q + (H @ d[:, :, None])[:, :, 0]
        c = torch.where(done[:, None], c, ((d == bl) & (g > 0)) | ((d == bh) & (g < 0)))
        done = done | (~done & ~moved & have & (c == cf).all(dim=1))
        if bool(done.all()):
            break
        if it == BOXQP_ITERS:
            status[~done] = 3
            break
        unit = c[:, :, None] | c[:, None, :]
        Lnew, info = torch.linalg.cholesky_ex(torch.where(unit, eye, torch.where(done[:, None, None], eye, H)))
        bad = ~done & ((info != 0) | ~torch.isfinite(Lnew).all(dim=2).all(dim=1))
        status[bad] = 1
        done = done | bad
        L = torch.where(done[:, None, None], L, Lnew)
        cf, have = torch.where(done[:, None], cf, c), have | ~done
        done = done | (~done & c.all(dim=1))
        s = torch.cholesky_solve(torch.where(c, torch.zeros_like(g), -g)[:, :, None], L)[:, :, 0]
        s = torch.where(c, torch.zeros_like(s), s)
        sg = (s * g).sum(dim=1)
        bad = ~done & ~torch.isfinite(sg)
        status[bad] = 1
        done = done | bad | (~done & ~(sg < 0))
        if bool(done.all()):
            break
        a = torch.ones_like(v)
        found = done.clone()
        xc, vc, clipped = d, v, torch.zeros_like(done)
        for _ in range(BOXQP_TRIALS):
            y = d + a[:, None] * s
            xt = clip(y)
            vt = value(xt)
            ok = ~found & ((vt - v) / (a * sg) >= BOXQP_ARMIJO)
            xc, vc = torch.where(ok[:, None], xt, xc), torch.where(ok, vt, vc)
            clipped = torch.where(ok, (xt != y).any(dim=1), clipped)
            found = found | ok
            if bool(found.all()):
                break
            a = torch.where(found, a, a * BOXQP_STEP)
        status[~found] = 3
        done = done | ~found
        run = ~done
        moved = torch.where(run, clipped | (a != 1.0), moved)
        d, v = torch.where(run[:, None], xc, d), torch.where(run, vc, v)
        iters = iters + run.to(iters.dtype)
    bad = (status == 0) & ~torch.isfinite(d).all(dim=1)
    status[bad] = 1
    return d, c, L, iters, status


def backward_pass_box(A, B, lx, lu, lxx, luu, u, lo, hi, reg=0.0, info=None):
    """The backward pass of control-limited DDP: backward_pass with the box lo <= u_t + du <= hi on the controls -- THE DEFINITION
    kmanip_lqr_backward_box is held to.  backward_pass's arguments, u [n, T, nu] the nominal controls, lo and
    hi [nu] or [n, nu] (-inf / +inf: unbounded on that side).  Per step, with H = Quu + reg I: k = box_qp(H, Qu, lo - u_t, hi - u_t);
    on the free set K_f = -H_ff^-1 Qux_f, the rows of K at the clamped actuators zeros; Vx, Vxx and dV by backward_pass's formulas
    with these k and K (Quu without reg).  A problem whose QP fails at step t (box_qp's status) stops there: all its k, K, dV and
    masks are zeros.  Returns (k [n, T, nu], K [n, T, nu, nx], dV [n, 2], clamped [n, T] int32: bit i set where actuator i ended
    step t on a bound); a dict given as `info` receives status [n] uint8, fail_step [n] int32 (-1: none) and qp_iters [n, T] int32."""
    import torch
    n, T, nx, nu = B.shape
    if lxx.dim() == 3:
        lxx = lxx[None]
    if luu.dim() == 3:
        luu = luu[None]
    dev, dt = A.device, A.dtype
    reg = torch.as_tensor(reg, dtype=dt, device=dev).reshape(-1, 1, 1)
    lo = torch.as_tensor(lo, dtype=dt, device=dev).reshape(-1, nu).expand(n, nu)
    hi = torch.as_tensor(hi, dtype=dt, device=dev).reshape(-1, nu).expand(n, nu)
    eye = torch.eye(nu, dtype=dt, device=dev)
    bits = (2 ** torch.arange(nu, device=dev)).to(torch.int64)
    Vx, Vxx = lx[:, T], lxx[:, T].expand(n, nx, nx)
    k, K = torch.zeros_like(lu), torch.zeros((n, T, nu, nx), dtype=dt, device=dev)
    dV = torch.zeros((n, 2), dtype=dt, device=dev)
    clamped = torch.zeros((n, T), dtype=torch.int32, device=dev)
    qp_iters = torch.zeros((n, T), dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    fail_step = torch.full((n,), -1, dtype=torch.int32, device=dev)
    for t in range(T - 1, -1, -1):
        At, Bt = A[:, t], B[:, t]
        AtT, BtT = At.transpose(1, 2), Bt.transpose(1, 2)
        Qx = lx[:, t] + (AtT @ Vx[:, :, None])[:, :, 0]
        Qu = lu[:, t] + (BtT @ Vx[:, :, None])[:, :, 0]
        Qxx = lxx[:, t] + AtT @ Vxx @ At
        Quu = luu[:, t] + BtT @ Vxx @ Bt
        Qux = BtT @ Vxx @ At
        kt, c, L, its, st = box_qp(Quu + reg * eye, Qu, lo - u[:, t], hi - u[:, t])
        Kt = -torch.cholesky_solve(torch.where(c[:, :, None], torch.zeros_like(Qux), Qux), L)
        Kt = torch.where(c[:, :, None], torch.zeros_like(Kt), Kt)
        st = torch.where((st == 0) & ~torch.isfinite(Kt).all(dim=2).all(dim=1), torch.ones_like(st), st)
        new = (status == 0) & (st != 0)
        status, fail_step = torch.where(new, st, status), torch.where(new, torch.full_like(fail_step, t), fail_step)
        KtT = Kt.transpose(1, 2)
        Vx = Qx + (KtT @ (Quu @ kt[:, :, None] + Qu[:, :, None]) + Qux.transpose(1, 2) @ kt[:, :, None])[:, :, 0]
        Vxx = Qxx + KtT @ Quu @ Kt + KtT @ Qux + Qux.transpose(1, 2) @ Kt
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
        dV[:, 0] += (kt * Qu).sum(dim=1)
        dV[:, 1] += 0.5 * (kt * (Quu @ kt[:, :, None])[:, :, 0]).sum(dim=1)
        k[:, t], K[:, t] = kt, Kt
        clamped[:, t], qp_iters[:, t] = (c.to(torch.int64) * bits).sum(dim=1).to(torch.int32), its
    ok = status == 0
    zero = lambda x: torch.where(ok.reshape((n,) + (1,) * (x.dim() - 1)), x, torch.zeros_like(x))
    if info is not None:
        info.update(status=status, fail_step=fail_step, qp_iters=zero(qp_iters))
    return zero(k), zero(K), zero(dV), zero(clamped)


def forward_pass(env, envs, qpos0, qvel0, warm0, ctrl, k, K, qpos_ref, qvel_ref, cost, alphas, qfrc_applied=None, nsub=None, K_t=None,
                 ctrl_lo=None, ctrl_hi=None):
    """The line search in ONE rollout_feedback launch of n len(alphas) rows: row a n + e starts at env e's initial state, carries the
    open-loop term ctrl[e] + alphas[a] k[e] and follows gain trajectory e (gain_index), i.e. K[e] about the nominal states
    qpos_ref / qvel_ref [n, T, ..] before each step.  Returns a dict: cost [len(alphas), n] (inf where the row stopped early),
    best [n] the index of the cheapest alpha per env, best_cost [n], ctrl [n, T, nu] the controls the best row applied, rows: the
    launch's result.  K_t [n, T, 2 nv, nu]: the gains transposed (env.lqr_backward's gains_t), handed to the launch as they are in
    place of K, which then is not read.  ctrl_lo / ctrl_hi [nu] or [n, nu]: the launch clamps the policy's output to the box
    (rollout_feedback's ctrl_lo / ctrl_hi), and `ctrl` is the clamped controls; both None: today's call."""
    import torch
    n, T, nu = ctrl.shape
    dev = ctrl.device
    al = torch.as_tensor(alphas, dtype=ctrl.dtype, device=dev)
    na = int(al.numel())
    idx = torch.arange(n, dtype=torch.int32, device=dev) if envs is None else torch.as_tensor(envs).to(device=dev, dtype=torch.int32)
    open_loop = (ctrl[None] + al[:, None, None, None] * k[None]).reshape(na * n, T, nu).contiguous()
    rows = env.rollout_feedback(envs=idx.repeat(na), qpos=qpos0.repeat(na, 1), qvel=qvel0.repeat(na, 1), warm=warm0.repeat(na, 1),
                                ctrl=open_loop, qfrc_applied=None if qfrc_applied is None else qfrc_applied.repeat(na, 1),
                                **(dict(gains=K) if K_t is None else dict(gains_t=K_t)),
                                qpos_ref=qpos_ref.contiguous(), qvel_ref=qvel_ref.contiguous(),
                                gain_index=torch.arange(n, dtype=torch.int32, device=dev).repeat(na), nsub=nsub,
                                fields=("qpos", "qvel", "ctrl", "status"),
                                **({} if ctrl_lo is None and ctrl_hi is None else dict(ctrl_lo=ctrl_lo, ctrl_hi=ctrl_hi)))
    q = torch.cat([qpos0.repeat(na, 1)[:, None], rows["qpos"]], dim=1)
    v = torch.cat([qvel0.repeat(na, 1)[:, None], rows["qvel"]], dim=1)
    c = cost.total(q, v, rows["ctrl"])
    c = torch.where(rows["status"] == 0, c, torch.full_like(c, float("inf"))).reshape(na, n)
    best_cost, best = c.min(dim=0)
    pick = best * n + torch.arange(n, device=dev)
    return {"cost": c, "best": best, "best_cost": best_cost, "ctrl": rows["ctrl"][pick], "rows": rows}


def ilqr(env, envs, qpos0, qvel0, warm0, ctrl, cost, iters=10, alphas=(1.0, 0.5, 0.25), reg=1e-6, reg_factor=10.0, qfrc_applied=None,
         nsub=None, eps=1e-6, fused=False, device_backward=False, ctrl_lo=None, ctrl_hi=None):
    """iLQR from the initial rows (qpos0, qvel0, warm0) [n, ..] and the control guess ctrl [n, T, nu]: per iteration trajectory_fd,
    cost.derivatives, backward_pass and forward_pass.  An env accepts the cheapest of its line-search rows if it is cheaper than its
    nominal trajectory, and divides its regularisation by reg_factor; otherwise it keeps its controls and multiplies it.  Returns a
    dict: ctrl [n, T, nu]; cost [iters + 1, n], the accepted cost after every iteration (entry 0: the guess's), never increasing;
    accepted [iters, n] bool; k, K of the last backward pass; reg [n].  fused: trajectory_fd's.
    device_backward: the backward pass is env.lqr_backward (kmanip_lqr_backward, one launch) on deriv_t where
    fused gives it, else on A and B, and the line search takes its transposed gains as they are.  It factorises Quu + reg I by
    Cholesky: an env whose factorisation fails (status != 0; its k and K are zeros) counts as not accepted -- it keeps its controls and
    its reg is multiplied by reg_factor.  The dict then also has backward_status [iters, n] uint8.
    ctrl_lo / ctrl_hi [nu] or [n, nu] (one of them None: that side unbounded): CONTROL-LIMITED iLQR -- the guess
    is clipped into the box, the backward pass is backward_pass_box or, with device_backward, env.lqr_backward_box, and the line search
    clamps the policy's output, so every control applied lies in the box.  An env whose backward pass has status 1 or 3 counts as
    not accepted, as above; backward_status is returned on either path, clamped [n, T] (the last pass's masks) with it.  Both None:
    today's code path."""
    import torch
    n = int(ctrl.shape[0])
    ctrl = ctrl.clone()
    boxed = ctrl_lo is not None or ctrl_hi is not None
    if boxed:
        inf = torch.full((ctrl.shape[2],), float("inf"), dtype=ctrl.dtype, device=ctrl.device)
        ctrl_lo = -inf if ctrl_lo is None else torch.as_tensor(ctrl_lo, dtype=ctrl.dtype, device=ctrl.device)
        ctrl_hi = inf if ctrl_hi is None else torch.as_tensor(ctrl_hi, dtype=ctrl.dtype, device=ctrl.device)
        ctrl = torch.minimum(torch.maximum(ctrl, ctrl_lo.reshape(-1, 1, ctrl.shape[2])), ctrl_hi.reshape(-1, 1, ctrl.shape[2]))
    clamped = None
    reg = torch.full((n,), float(reg), dtype=ctrl.dtype, device=ctrl.device)
    history, accepted = [], []
    k = K = None
    statuses = []
    for _ in range(iters):
        fd = trajectory_fd(env, envs, qpos0, qvel0, warm0, ctrl, qfrc_applied=qfrc_applied, nsub=nsub, eps=eps, fused=fused)
        if not history:
            history.append(cost.total(fd["qpos"], fd["qvel"], ctrl))
        K_t = solved = None
        if boxed:
            derivs = cost.derivatives(fd["qpos"], fd["qvel"], ctrl)
            if device_backward:
                dyn = dict(deriv_t=fd["deriv_t"]) if "deriv_t" in fd else dict(A=fd["A"], B=fd["B"])
                bp = env.lqr_backward_box(*derivs, ctrl, ctrl_lo, ctrl_hi, reg=reg, **dyn)
                k, K, K_t, clamped, status = bp["k"], bp["K"], bp["gains_t"], bp["clamped"], bp["status"]
            else:
                bp = {}
                k, K, _, clamped = backward_pass_box(fd["A"], fd["B"], *derivs, ctrl, ctrl_lo, ctrl_hi, reg=reg, info=bp)
                status = bp["status"]
            solved = status == 0
            statuses.append(status)
        elif device_backward:
            dyn = dict(deriv_t=fd["deriv_t"]) if "deriv_t" in fd else dict(A=fd["A"], B=fd["B"])
            bp = env.lqr_backward(*cost.derivatives(fd["qpos"], fd["qvel"], ctrl), reg=reg, **dyn)
            k, K, K_t, solved = bp["k"], bp["K"], bp["gains_t"], bp["status"] == 0
            statuses.append(bp["status"])
        else:
            k, K, _ = backward_pass(fd["A"], fd["B"], *cost.derivatives(fd["qpos"], fd["qvel"], ctrl), reg=reg)
        fp = forward_pass(env, envs, qpos0, qvel0, warm0, ctrl, k, K, fd["qpos"][:, :-1], fd["qvel"][:, :-1], cost, alphas,
                          qfrc_applied=qfrc_applied, nsub=nsub, K_t=K_t, ctrl_lo=ctrl_lo, ctrl_hi=ctrl_hi)
        ok = fp["best_cost"] < history[-1]
        if solved is not None:
            ok = ok & solved
        ctrl = torch.where(ok[:, None, None], fp["ctrl"], ctrl)
        reg = torch.where(ok, reg / reg_factor, reg * reg_factor)
        history.append(torch.where(ok, fp["best_cost"], history[-1]))
        accepted.append(ok)
    res = {"ctrl": ctrl, "cost": torch.stack(history), "accepted": torch.stack(accepted), "k": k, "K": K, "reg": reg}
    if device_backward or boxed:
        res["backward_status"] = torch.stack(statuses)
    if boxed:
        res["clamped"] = clamped
    return res
