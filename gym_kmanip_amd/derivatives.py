"""Finite-difference derivatives of the forward dynamics, assembled from two KManipEnvHip.forward launches (forward_fd: d qacc / d
input), and of one step of the simulator, assembled from two KManipEnvHip.rollout launches (transition_fd:
MuJoCo's mjd_transitionFD, A = d s' / d s and B = d s' / d ctrl).

Positions are perturbed in the TANGENT space, whose columns are qvel's: nv = nlink + 6 columns for nq = nlink + 7 coordinates.
Joint and cube-position columns add eps; cube-rotation column k multiplies the cube's quaternion on the right by
exp(eps e_k / 2) -- the body-frame convention of qvel's angular part, MuJoCo's mj_integratePos.

Everything here is torch arithmetic on whatever device the caller's tensors live on, one operation per kernel, so a CPU stand-in
with a .forward of the same shape (tests/tools/forward_oracle.py OracleForward) is driven through the same code and is handed
bit-equal rows."""
import math

WRT = ("qpos", "qvel", "ctrl", "qfrc_applied")
_BLOCK = {"qpos": "dqpos", "qvel": "dqvel", "ctrl": "dctrl", "qfrc_applied": "dfrc"}


def tangent_perturb(cm, qpos, col, eps):
    """A copy of qpos [n, nq] moved by eps along tangent column `col` (0 .. nv-1).  Columns below nlink + 3 (joints, cube position):
    that coordinate += eps.  Column nlink + 3 + k: quat <- quat (x) [cos(eps / 2), sin(eps / 2) e_k], the rotation by eps about the
    cube's own axis k.  The product is not re-normalised (its norm is the input's up to rounding; the kinematics normalise the
    quaternion as they do in a step)."""
    nl = cm.nlink
    if not 0 <= col < nl + 6:
        raise ValueError("tangent column %d outside 0 .. %d" % (col, nl + 5))
    out = qpos.clone()
    if col < nl + 3:
        out[:, col] += eps
        return out
    v1 = [0.0, 0.0, 0.0]
    v1[col - nl - 3] = math.sin(0.5 * eps)
    w1, (x1, y1, z1) = math.cos(0.5 * eps), v1
    w0, x0, y0, z0 = (qpos[:, nl + 3 + k] for k in range(4))
    out[:, nl + 3] = w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1
    out[:, nl + 4] = w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1
    out[:, nl + 5] = w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1
    out[:, nl + 6] = w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1
    return out


def tangent_diff(cm, qpos_b, qpos_a):
    """[n, nv]: the tangent vector from qpos_a to qpos_b, MuJoCo's mj_differentiatePos -- the inverse of tangent_perturb to first
    order.  Joints and cube position are subtracted.  The rotation part is the body-frame log of quat_a^-1 (x) quat_b: the rotation
    vector, about the cube's own axes at qpos_a, that takes a's orientation to b's (angle in (-pi, pi]).  The quaternions need not be
    normalised: axis and atan2 do not see a common positive factor."""
    import torch
    nl = cm.nlink
    out = qpos_b[:, :nl + 6] - qpos_a[:, :nl + 6]
    wa, xa, ya, za = (qpos_a[:, nl + 3 + k] for k in range(4))
    wb, xb, yb, zb = (qpos_b[:, nl + 3 + k] for k in range(4))
    # conj(a) (x) b, the vector part as two differences of products each: equal quaternions give exactly zero
    w = wa * wb + xa * xb + ya * yb + za * zb
    x = (wa * xb - xa * wb) + (za * yb - ya * zb)
    y = (wa * yb - ya * wb) + (xa * zb - za * xb)
    z = (wa * zb - za * wb) + (ya * xb - xa * yb)
    s = torch.sqrt(x * x + y * y + z * z)
    ang = 2.0 * torch.atan2(s, w)
    ang = torch.where(ang > math.pi, ang - 2.0 * math.pi, ang)
    # angle / sin(angle / 2) -> 2 / w as the vector part vanishes (no division by zero at the identity)
    k = torch.where(s > 0, ang / torch.where(s > 0, s, torch.ones_like(s)), 2.0 / torch.where(w != 0, w, torch.ones_like(w)))
    out[:, nl + 3] = k * x
    out[:, nl + 4] = k * y
    out[:, nl + 5] = k * z
    return out


def transition_fd(env, envs=None, qpos=None, qvel=None, ctrl=None, qfrc_applied=None, warm=None, nsub=None, eps=1e-6,
                  wrt=("qpos", "qvel", "ctrl"), warm_offset=1.0):
    """MuJoCo's mjd_transitionFD on env.rollout: centred finite differences of ONE step (nstep = 1, nsub sub-steps; None = the
    model's n_sub_steps, a control step; 1 = mj_step) with respect to the inputs named in `wrt`, at the rows (envs, qpos, qvel, ctrl,
    qfrc_applied, warm) as rollout() takes them.  Two launches: the nominal rows, then all 2 ncol n perturbed rows at once.
    The state is (qpos in the tangent space, qvel), 2 nv wide: perturbed along tangent_perturb's columns, differenced with
    tangent_diff.  Returns a dict of tensors on the inputs' device:
      qpos [n, nq], qvel [n, nv], qacc_warm [n, nv], contact_mask [n], status [n] uint8      the nominal rows one step on
      A [n, 2 nv, 2 nv] = d s' / d s (wrt holds qpos and qvel), B [n, 2 nv, nu] = d s' / d ctrl (wrt holds ctrl),
      dnext_dfrc [n, 2 nv, nv] (wrt holds qfrc_applied); dnext_dqpos / dnext_dqvel [n, 2 nv, nv] for a wrt with one of the two
      status_fd [n] uint8          the largest status over the row's perturbed copies (nonzero: the row's blocks are not derivatives)
      contact_mask_fd [ncol, 2, n] int32      the contact mask after the step of every perturbed row, + then -, columns in `wrt` order
    qpos, qvel and ctrl must be given as rows where they are differentiated (state_tensors(envs) returns the stored ones);
    qfrc_applied=None in `wrt` means rows of zeros, given explicitly to both launches.
    THE WARM START.  The perturbed rows start their first sub-step from the nominal rows' warm start -- `warm` if given, else the
    nominal rows' qacc_warm after the step -- plus warm_offset on every dof, forward_fd's mechanism and for its reason: started at a
    point where the scaled gradient is below the model's solver_tolerance the Newton solver returns that point untouched, and a row
    moved by eps is that close to the nominal solution, so the quotient would carry tolerance / eps.  Sub-steps after the first
    warm-start from their own previous qacc, as they do in a step, and nothing can offset those: with nsub > 1 the solver's
    tolerance does enter the quotient as tolerance / eps.  A caller who wants derivatives tighter than that compiles the model with a
    smaller solver_tolerance (compile_model(..., solver_tolerance=...)); warm_offset = 0 gives the plain warm start.
    THE DYNAMICS ARE PIECEWISE SMOOTH: where +eps and -eps fall on different sides of a change of the active set the quotient is a
    secant, not a derivative (forward_fd's note); contact_mask_fd shows the contact part of that.  It needs only env.rollout, env.cm
    and the tensors' device, so a CPU stand-in (tests/tools/rollout_oracle.py OracleRollout) is driven through the same code and
    is handed bit-equal rows."""
    import torch
    cm = env.cm
    nv, nu = cm.nv, cm.nu
    wrt = tuple(wrt)
    unknown = set(wrt) - set(WRT)
    if unknown:
        raise ValueError("unknown wrt name(s) %s" % sorted(unknown))
    given = {"qpos": qpos, "qvel": qvel, "ctrl": ctrl, "qfrc_applied": qfrc_applied}
    for name in ("qpos", "qvel", "ctrl"):
        if given[name] is None and name in wrt:
            raise ValueError("transition_fd: %s is differentiated and must be given as rows" % name)
        if given[name] is not None and given[name].dim() != 2:
            raise ValueError("transition_fd: %s must be [n, width] rows of one step" % name)
    ref = next((t for t in (qpos, qvel, ctrl, qfrc_applied, warm) if t is not None), None)
    if "qfrc_applied" in wrt and qfrc_applied is None:
        if ref is None:
            raise ValueError("transition_fd: with nothing given as rows there is nothing to size the force rows by")
        given["qfrc_applied"] = torch.zeros((ref.shape[0], nv), dtype=torch.float64, device=ref.device)
    fields = ("qpos", "qvel", "qacc_warm", "contact_mask", "status")
    nominal = env.rollout(envs=envs, qpos=given["qpos"], qvel=given["qvel"], ctrl=given["ctrl"], warm=warm,
                          qfrc_applied=given["qfrc_applied"], nstep=1, nsub=nsub, fields=fields)
    out = {k: nominal[k][:, 0] for k in ("qpos", "qvel", "qacc_warm", "contact_mask")}
    out["status"] = nominal["status"]
    n, dev = int(out["qpos"].shape[0]), out["qpos"].device
    width = {"qpos": nv, "qvel": nv, "ctrl": nu, "qfrc_applied": nv}
    ncol = sum(width[name] for name in wrt)
    if ncol == 0 or n == 0:
        return out
    reps = 2 * ncol
    idx = torch.arange(n, dtype=torch.int32, device=dev) if envs is None else torch.as_tensor(envs).to(device=dev, dtype=torch.int32)
    big = {name: (None if t is None else t.repeat(reps, 1)) for name, t in given.items()}
    c = 0
    for name in wrt:
        for j in range(width[name]):
            for s, sign in enumerate((1.0, -1.0)):
                lo = (2 * c + s) * n
                if name == "qpos":
                    big[name][lo:lo + n] = tangent_perturb(cm, given[name], j, sign * eps)
                else:
                    big[name][lo:lo + n, j] += sign * eps
            c += 1
    base = warm if warm is not None else out["qacc_warm"]
    pert = env.rollout(envs=idx.repeat(reps), qpos=big["qpos"], qvel=big["qvel"], ctrl=big["ctrl"], warm=(base + warm_offset).repeat(reps, 1),
                       qfrc_applied=big["qfrc_applied"], nstep=1, nsub=nsub, fields=fields)
    out["status_fd"] = pert["status"].reshape(reps, n).max(dim=0).values
    out["contact_mask_fd"] = pert["contact_mask"].reshape(ncol, 2, n)
    q = pert["qpos"][:, 0]
    v = pert["qvel"][:, 0].reshape(ncol, 2, n, nv)
    dq = torch.stack([tangent_diff(cm, q[(2 * k) * n:(2 * k + 1) * n], q[(2 * k + 1) * n:(2 * k + 2) * n]) for k in range(ncol)])      # [ncol, n, nv]
    d = (torch.cat([dq, v[:, 0] - v[:, 1]], dim=2) / (2.0 * eps)).permute(1, 2, 0)          # [n, 2 nv, ncol]
    c = 0
    blocks = {}
    for name in wrt:
        blocks[name] = d[:, :, c:c + width[name]].contiguous()
        c += width[name]
    if "qpos" in blocks and "qvel" in blocks:
        out["A"] = torch.cat([blocks["qpos"], blocks["qvel"]], dim=2)
    else:
        for name in ("qpos", "qvel"):
            if name in blocks:
                out["dnext_d" + name] = blocks[name]
    if "ctrl" in blocks:
        out["B"] = blocks["ctrl"]
    if "qfrc_applied" in blocks:
        out["dnext_dfrc"] = blocks["qfrc_applied"]
    return out


def adjoint_pass(A, B, gx, gu=None, gains=None, m=1):
    """The adjoint sweep of a rollout: THE DEFINITION kmanip_adjoint is held to (include/kmanip.h KAdjointIn).
    A [n, T, nx, nx], B [n, T, nx, nu] the step Jacobians (trajectory_fd's); m >= 1 cotangent vectors per problem, row e m + j
    carrying vector j through the dynamics of problem e; gx [n m, T + 1, nx] the loss's direct partials with respect to the tangent
    state x_t (entry 0: x_0, entry T: the final state), gu [n m, T, nu] those with respect to u_t or None (zeros); gains
    [n, T, nu, nx] the feedback K_t of a closed-loop rollout u_t = ctrl_t + K_t dx_t, or None (open loop).  lam[T] = gx[T]; for
    t = T-1 .. 0
        mu[t]  = gu[t] + B_t' lam[t+1]
        lam[t] = gx[t] + A_t' lam[t+1] + K_t' mu[t]
    the direct term added last.  Returns (lam [n m, T + 1, nx], mu [n m, T, nu]): lam[:, 0] is the gradient with respect to the
    initial tangent state, mu the gradient with respect to the control that acted (the open-loop term); the gradient with respect to
    K_t is the outer product mu[t] (x) dx_t.  With gains, dx_t is taken as linear in the state (QuadraticCost's Gauss-Newton
    habit): exact when the cube-rotation columns of K are zero.  A torch loop over the T steps, on the device of the tensors."""
    import torch
    n, T, nx, nu = B.shape
    m = int(m)
    if tuple(gx.shape) != (n * m, T + 1, nx):
        raise ValueError("adjoint_pass: gx must be [n m, T + 1, nx] = %s, not %s" % ((n * m, T + 1, nx), tuple(gx.shape)))
    g = gx.reshape(n, m, T + 1, nx)
    h = None if gu is None else gu.reshape(n, m, T, nu)
    lam = torch.empty((n, m, T + 1, nx), dtype=A.dtype, device=A.device)
    mu = torch.empty((n, m, T, nu), dtype=A.dtype, device=A.device)
    nxt = g[:, :, T]
    lam[:, :, T] = nxt
    for t in range(T - 1, -1, -1):
        u = nxt @ B[:, t]                                 # rows of lam[t+1]' B_t = (B_t' lam[t+1])'
        if h is not None:
            u = u + h[:, :, t]
        s = nxt @ A[:, t]
        if gains is not None:
            s = s + u @ gains[:, t]
        nxt = s + g[:, :, t]
        mu[:, :, t], lam[:, :, t] = u, nxt
    return lam.reshape(n * m, T + 1, nx), mu.reshape(n * m, T, nu)


def forward_fd(env, envs=None, qpos=None, qvel=None, ctrl=None, qfrc_applied=None, eps=1e-6,
               wrt=("qpos", "qvel", "ctrl", "qfrc_applied"), warm_offset=1.0):
    """Centred finite differences of env.forward's qacc and qfrc_constraint with respect to the inputs named in `wrt`, at the rows
    (envs, qpos, qvel, ctrl, qfrc_applied) as forward() takes them.  Two launches: the nominal rows, then all 2 ncol n perturbed
    rows at once, each with the nominal qacc + warm_offset (on every dof) as its warm start.
    WHY NOT THE NOMINAL qacc ITSELF: the Newton solver returns its starting point untouched when the gradient there, scaled by
    1 / (meaninertia nv), is below the model's solver_tolerance (MuJoCo's rule), and it stops iterating by the same test.  A row
    moved by eps starts that close to its own solution whenever the input's effect on the forces is small -- measured on an
    MI355X with warm_offset = 0: the dqvel blocks were off by 8.5e-9 x normaliser / eps (0.18 in an entry), the solver's tolerance
    divided by eps, while dqpos / dctrl / dfrc met the bar.  Started one unit of acceleration away, the solver iterates, and its
    last full Newton step lands on the row's solution to rounding (what the parity tests measure from a zero start; a zero start
    would fail the same way at an equilibrium, where qacc = 0 is the solution).  warm_offset = 0 gives the plain warm start.
    Returns a dict of tensors on the inputs' device:
      qacc, qfrc_constraint [n, nv], status [n] uint8     the nominal rows
      dqacc_dqpos [n, nv, nv] (tangent columns: tangent_perturb), dqacc_dqvel [n, nv, nv], dqacc_dctrl [n, nv, nu],
      dqacc_dfrc [n, nv, nv]; dqfrc_constraint_dqpos / _dqvel / _dctrl / _dfrc likewise      the blocks of `wrt` only
      status_fd [n] uint8          the largest status over the row's perturbed copies (nonzero: the row's blocks are not derivatives)
      contact_mask_fd [ncol, 2, n] int32      the contact mask of every perturbed row, + then -, columns in `wrt` order
    An input that is differentiated must be given as rows (state_tensors(envs) returns the stored ones); qfrc_applied=None in `wrt`
    means rows of zeros, given explicitly to both launches (a bound force is then not read: pass its rows to differentiate about
    it).  Inputs not in `wrt` may stay None: every row then uses what its env stores.
    THE DYNAMICS ARE PIECEWISE SMOOTH.  Across a change of the active set -- a contact opening or closing, a friction-loss row
    saturating, a servo reaching its force or control clamp -- qacc has a kink, and where +eps and -eps fall on different sides
    of one the quotient is a SECANT across it, not a derivative; contact_mask_fd shows the contact part of that.  No smoothing is
    applied."""
    import torch
    cm = env.cm
    nv, nu = cm.nv, cm.nu
    wrt = tuple(wrt)
    unknown = set(wrt) - set(WRT)
    if unknown:
        raise ValueError("unknown wrt name(s) %s" % sorted(unknown))
    given = {"qpos": qpos, "qvel": qvel, "ctrl": ctrl, "qfrc_applied": qfrc_applied}
    for name in wrt:
        if given[name] is None and name != "qfrc_applied":
            raise ValueError("forward_fd: %s is differentiated and must be given as rows" % name)
    nominal = None
    if "qfrc_applied" in wrt and qfrc_applied is None:
        ref = next((t for t in (qpos, qvel, ctrl) if t is not None), None)
        if ref is None:          # nothing given at all: the row count and the device come from a first nominal launch
            nominal = env.forward(envs=envs, fields=("qacc",))
            ref = nominal["qacc"]
        given["qfrc_applied"] = torch.zeros((ref.shape[0], nv), dtype=torch.float64, device=ref.device)
    fields = ("qacc", "qfrc_constraint", "contact_mask", "status")
    nominal = env.forward(envs=envs, qpos=given["qpos"], qvel=given["qvel"], ctrl=given["ctrl"], qfrc_applied=given["qfrc_applied"],
                          fields=fields)
    a0 = nominal["qacc"]
    n, dev = int(a0.shape[0]), a0.device
    out = {"qacc": a0, "qfrc_constraint": nominal["qfrc_constraint"], "status": nominal["status"]}
    width = {"qpos": nv, "qvel": nv, "ctrl": nu, "qfrc_applied": nv}
    ncol = sum(width[name] for name in wrt)
    if ncol == 0 or n == 0:
        return out
    reps = 2 * ncol
    idx = torch.arange(n, dtype=torch.int32, device=dev) if envs is None else torch.as_tensor(envs).to(device=dev, dtype=torch.int32)
    big = {name: (None if t is None else t.repeat(reps, 1)) for name, t in given.items()}
    c = 0
    for name in wrt:
        for j in range(width[name]):
            for s, sign in enumerate((1.0, -1.0)):
                lo = (2 * c + s) * n
                if name == "qpos":
                    big[name][lo:lo + n] = tangent_perturb(cm, given[name], j, sign * eps)
                else:
                    big[name][lo:lo + n, j] += sign * eps
            c += 1
    pert = env.forward(envs=idx.repeat(reps), qpos=big["qpos"], qvel=big["qvel"], ctrl=big["ctrl"], warm=(a0 + warm_offset).repeat(reps, 1),
                       qfrc_applied=big["qfrc_applied"], fields=fields)
    out["status_fd"] = pert["status"].reshape(reps, n).max(dim=0).values
    out["contact_mask_fd"] = pert["contact_mask"].reshape(ncol, 2, n)
    for key in ("qacc", "qfrc_constraint"):
        v = pert[key].reshape(ncol, 2, n, nv)
        d = ((v[:, 0] - v[:, 1]) / (2.0 * eps)).permute(1, 2, 0)          # [n, nv, ncol]
        c = 0
        for name in wrt:
            out["d%s_%s" % (key, _BLOCK[name])] = d[:, :, c:c + width[name]].contiguous()
            c += width[name]
    return out
