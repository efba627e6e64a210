"""The physics step with an applied force (MuJoCo's data.qfrc_applied), restated in NumPy from what oracle.Oracle returns: the
reference of kmanip_bind_applied_force.  The oracle's control step knows no applied force; Oracle.physics_step_applied (the physics
sub-steps alone, for sweep caps this module cannot reach in a test's time) is held to this restatement by
tests/test_pgs_fixed_point_cpu.py.

Per sub-step: dyn = Oracle.dynamics(qpos, qvel, ctrl) gives M, bias, qacc_smooth and the constraint rows J, aref, R of the state,
Oracle.constraint_rows their types and friction-loss bounds.  The force enters in one place,
    a_s = qacc_smooth + M^-1 tau,
and the constrained acceleration a follows from a_s as the handle's solver defines it:
  Newton   the exact minimiser of 1/2 (a - a_s)^T M (a - a_s) + sum_i s_i(J_i a - aref_i), s_i the row cost of
           force_oracle.row_forces (one-sided quadratic rows; Huber with bound floss on the friction-loss rows), by Newton's method
           with an exact line search from a = a_s.  The minimiser is unique (M is positive definite): no warm start is needed.
  PGS      the oracle's sweep (step2_accel of oracle/kmanip_oracle.c) row for row: B = M^-1 J^T, Adiag_i = J_i B_i, warm-start
           forces from the carried qacc_warm kept only if the dual cost is <= 0, row updates f_i - res / den clipped per type, stop
           when improvement / (meaninertia nv) < solver_tolerance or at solver_iterations.
Then the oracle's euler: qvel += dt a, joints and cube position advance with the new qvel, the cube quaternion is normalised,
multiplied on the right by the axis-angle quaternion of dt * w_body and normalised again.

Row layout of tau: the dof order of qM / qfrc_bias -- nlink joints, the force on the cube (world frame), the torque on it (cube frame)."""
import numpy as np

MJ_MINVAL = 1e-15
KM_SOLVER_NEWTON = 1


def draw_test_forces(cm, n, seed=11):
    """The "test forces" of the applied-force tests: default_rng(seed); +-2 on every joint, +-2 m g on the cube's three force
    components, +-1e-3 on its torque components."""
    nl = cm.nlink
    mg = cm.desc.cube_mass * abs(cm.desc.gravity[2])
    scale = np.array([2.0] * nl + [2.0 * mg] * 3 + [1e-3] * 3)
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, cm.nv)) * scale


# ------------------------------------------------------------------------------------------------------------------ row costs
def _rows(x, R, types, floss):
    """(cost, force, second derivative) of every row at x = J a - aref."""
    D = 1.0 / R
    one = x < 0
    cost = np.where(one, 0.5 * D * x * x, 0.0)
    f = np.where(one, -D * x, 0.0)
    h = np.where(one, D, 0.0)
    fl = types == 0
    if fl.any():
        xf, Rf, Df, b = x[fl], R[fl], D[fl], floss[fl]
        lo, hi = xf <= -Rf * b, xf >= Rf * b
        cost[fl] = np.where(lo, b * (-0.5 * Rf * b - xf), np.where(hi, b * (-0.5 * Rf * b + xf), 0.5 * Df * xf * xf))
        f[fl] = np.where(lo, b, np.where(hi, -b, -Df * xf))
        h[fl] = np.where(lo | hi, 0.0, Df)
    return cost, f, h


def newton_exact(M, J, aref, R, types, floss, a_s, max_iter=200):
    """argmin_a 1/2 (a - a_s)^T M (a - a_s) + sum_i s_i(J_i a - aref_i): Newton with the exact Hessian and an exact line search."""
    a = a_s.copy()
    if len(aref) == 0:
        return a

    def total(a):
        d = a - a_s
        c, f, h = _rows(J @ a - aref, R, types, floss)
        return 0.5 * d @ (M @ d) + c.sum(), f, h
    cost, f, h = total(a)
    for _ in range(max_iter):
        grad = M @ (a - a_s) - J.T @ f
        H = M + J.T @ (h[:, None] * J)
        p = -np.linalg.solve(H, grad)
        gp = grad @ p
        if not gp < 0:
            break
        x, y, pMp = J @ a - aref, J @ p, p @ (M @ p)
        g0 = M @ (a - a_s)

        def dphi(al):
            _, fr, hr = _rows(x + al * y, R, types, floss)
            return g0 @ p + al * pMp - fr @ y, pMp + hr @ (y * y)
        lo, hi = 0.0, 1.0
        while dphi(hi)[0] < 0:
            lo, hi = hi, 2.0 * hi
        al = hi
        for _ in range(100):                                # safeguarded Newton on the piecewise-linear, increasing phi'
            d1, d2 = dphi(al)
            if d1 == 0:
                break
            if d1 < 0:
                lo = al
            else:
                hi = al
            nxt = al - d1 / d2
            if not (lo < nxt < hi):
                nxt = 0.5 * (lo + hi)
            if nxt == al or hi - lo <= 4e-16 * hi:
                break
            al = nxt
        a_new = a + al * p
        c_new, f_new, h_new = total(a_new)
        if not c_new < cost:
            break
        a, cost, f, h = a_new, c_new, f_new, h_new
    return a


def pgs_sweep(cm, M, J, aref, R, types, floss, a_s, warm):
    """step2_accel's PGS branch of oracle/kmanip_oracle.c, row for row.  Returns qacc."""
    d = cm.desc
    ne, nv = len(aref), cm.nv
    if ne == 0:
        return a_s.copy()
    B = np.linalg.solve(M, J.T).T                                  # rows B_i = M^-1 J_i^T
    Adiag = np.einsum("ij,ij->i", J, B)
    b = J @ a_s - aref
    jar = J @ warm - aref
    Dn = 1.0 / R
    f = np.where(jar < 0, -Dn * jar, 0.0)
    fl = types == 0
    f[fl] = np.where(jar[fl] <= -R[fl] * floss[fl], floss[fl], np.where(jar[fl] >= R[fl] * floss[fl], -floss[fl], -Dn[fl] * jar[fl]))
    y = J.T @ f
    z = np.linalg.solve(M, y)
    cost = 0.5 * y @ z + (0.5 * R * f * f + f * b).sum()
    if cost > 0:
        f = np.zeros(ne)
        a = a_s.copy()
    else:
        a = a_s + z
    scale = 1.0 / (d.meaninertia * nv)
    for _ in range(d.solver_iterations):
        improvement = 0.0
        for i in range(ne):
            den = Adiag[i] + R[i]
            res = J[i] @ a - aref[i] + R[i] * f[i]
            fn = f[i] - res / den
            fn = min(max(fn, -floss[i]), floss[i]) if types[i] == 0 else max(fn, 0.0)
            dlt = fn - f[i]
            if dlt != 0:
                f[i] = fn
                a = a + B[i] * dlt
                improvement -= dlt * (res + 0.5 * den * dlt)
        if improvement * scale < d.solver_tolerance:
            break
    return a


def accel(cm, orc, qpos, qvel, ctrl, warm, tau):
    """(qacc, dyn, types, floss, a_s) of one state under the force tau, by the solver of cm."""
    dyn = orc.dynamics(qpos, qvel, ctrl)
    types, floss = orc.constraint_rows(qpos, qvel)
    assert len(types) == dyn["nefc"]
    a_s = dyn["qacc_smooth"] + np.linalg.solve(dyn["M"], np.asarray(tau, dtype=np.float64))
    if cm.desc.solver == KM_SOLVER_NEWTON:
        a = newton_exact(dyn["M"], dyn["J"], dyn["aref"], dyn["R"], types, floss, a_s)
    else:
        a = pgs_sweep(cm, dyn["M"], dyn["J"], dyn["aref"], dyn["R"], types, floss, a_s, np.asarray(warm, dtype=np.float64))
    return a, dyn, types, floss, a_s


def euler(cm, qpos, qvel, a):
    """The oracle's euler (mj_Euler)."""
    nl, dt = cm.nlink, cm.desc.timestep
    qvel = qvel + dt * a
    qpos = qpos.copy()
    qpos[:nl + 3] += dt * qvel[:nl + 3]
    ax = qvel[nl + 3:nl + 6].copy()
    n = np.sqrt(ax @ ax)
    ax = np.array([1.0, 0.0, 0.0]) if n < MJ_MINVAL else ax / n
    ang = dt * n
    qr = np.array([1.0, 0.0, 0.0, 0.0]) if ang == 0 else np.concatenate([[np.cos(0.5 * ang)], ax * np.sin(0.5 * ang)])
    q = qpos[nl + 3:nl + 7]
    nq = np.sqrt(q @ q)
    q = np.array([1.0, 0.0, 0.0, 0.0]) if nq < MJ_MINVAL else q / nq
    w0, x0, y0, z0 = q
    w1, x1, y1, z1 = qr
    qn = np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                   w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])
    nn = np.sqrt(qn @ qn)
    qpos[nl + 3:nl + 7] = np.array([1.0, 0.0, 0.0, 0.0]) if nn < MJ_MINVAL else qn / nn
    return qpos, qvel


def physics_step(cm, orc, qpos, qvel, ctrl, warm, tau, nsub=None):
    """nsub sub-steps (default: the model's n_sub_steps) of one env under the constant force tau; ctrl is the one before_step left
    (it does not depend on the force: take it from the unchanged oracle's own step).  In the joint-delta models of the regime
    cells before_step does not move qpos, so the first sub-step's products are those of qpos itself.  Returns (qpos, qvel, warm)."""
    qpos = np.asarray(qpos, dtype=np.float64).copy(); qvel = np.asarray(qvel, dtype=np.float64).copy()
    warm = np.asarray(warm, dtype=np.float64).copy()
    for _ in range(cm.desc.n_sub_steps if nsub is None else nsub):
        a = accel(cm, orc, qpos, qvel, ctrl, warm, tau)[0]
        warm = a.copy()
        qpos, qvel = euler(cm, qpos, qvel, a)
    return qpos, qvel, warm


def forces_decode(cm, orc, qpos, qvel, ctrl, warm, tau, geometry=True):
    """force_oracle.decode of a state under the force tau: decode evaluated with a_s shifted by M^-1 tau and qacc the restatement's.
    qfrc_actuator stays the servo's (M qacc_smooth + bias of the unforced dynamics)."""
    import force_oracle as F

    a, dyn, types, floss, a_s = accel(cm, orc, qpos, qvel, ctrl, warm, tau)
    nl = cm.nlink
    fa = (dyn["M"] @ dyn["qacc_smooth"] + dyn["bias"])[:nl]

    class Shifted:
        """The oracle with dynamics() reporting the forced qacc_smooth and qacc."""
        def __getattr__(self, name):
            return getattr(orc, name)

        def dynamics(self, qp, qv, ct):
            return dict(dyn, qacc_smooth=a_s, qacc=a)
    out = F.decode(cm, Shifted(), qpos, qvel, ctrl, geometry=geometry)
    out["qfrc_actuator"] = fa
    out["M"] = dyn["M"]
    return out


# ------------------------------------------------------------------------------------------------ the regime cells under the test forces
_CELL_RUNS = {}


def control_step(cm, qpos, qvel, ctrl, warm, tau, act=None, models=None):
    """One control step of every env of a batch under the forces tau ([n, nv]), zero action unless `act` is given.  ctrl after
    before_step, done byte and step counter come from the unchanged oracle's own step of the same states (they do not depend on
    the force); qpos, qvel and the warm start from physics_step above; the contact mask is Oracle.contact_mask of the restated qpos.
    models: one compiled model per env (model.with_env_params) where the envs differ in their physics parameters."""
    import regime_states as R
    from oracle.oracle import Oracle
    n = len(qpos)
    act = np.zeros((n, cm.act_dim), dtype=np.float32) if act is None else act
    out = dict(qpos=np.zeros_like(qpos), qvel=np.zeros_like(qvel), warm=np.zeros_like(warm), ctrl=np.zeros_like(ctrl),
               done=np.zeros(n, dtype=np.uint8), step=np.zeros(n, dtype=np.int32), mask=np.zeros(n, dtype=np.uint32))
    shared = Oracle(cm, 1) if models is None else None
    for e in range(n):
        cme = cm if models is None else models[e]
        one = shared if models is None else Oracle(cme, 1)
        stepper = Oracle(cme, 1)
        stepper.set_state(qpos[e:e + 1], qvel[e:e + 1], ctrl[e:e + 1], warm[e:e + 1], np.zeros(1, dtype=np.int32))
        _, _, done = stepper.step(act[e:e + 1])
        _, _, c1, _, s1 = stepper.get_state()
        out["ctrl"][e], out["done"][e], out["step"][e] = c1[0], done[0], s1[0]
        out["qpos"][e], out["qvel"][e], out["warm"][e] = physics_step(cme, one, qpos[e], qvel[e], c1[0], warm[e], tau[e])
        out["mask"][e] = int(one.contact_mask(out["qpos"][e])[0])
    return out


def cell_runs(asset, solver):
    """The regime cells of the asset (regime_states.cells) one control step on, zero action, under the test forces: computed once per
    (asset, solver) and shared by the tests.  dict(cm, qpos, qvel, ctrl, warm, labels, tau, ref, twin): ref / twin are control_step
    results, twin from qvel * (1 + 1e-15) -- the distance between the two is the reference's own error in the cell."""
    import regime_states as R
    from oracle.oracle import Oracle
    key = (asset, solver)
    if key not in _CELL_RUNS:
        cm = R.model(asset, solver)
        qpos, qvel, ctrl, labels = R.cells(asset)
        warm = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
        tau = draw_test_forces(cm, len(labels))
        _CELL_RUNS[key] = dict(cm=cm, qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, labels=labels, tau=tau,
                               ref=control_step(cm, qpos, qvel, ctrl, warm, tau),
                               twin=control_step(cm, qpos, qvel * (1.0 + 1e-15), ctrl, warm, tau))
    return _CELL_RUNS[key]


def hover_state(cm, height=0.3):
    """(qpos, qvel, ctrl) of the home pose with the cube `height` metres above the table top, at rest."""
    import regime_states as R
    from oracle.oracle import Oracle
    qpos, qvel, ctrl = R.home_state(cm, Oracle(cm, 1))
    qpos[cm.nlink + 2] = cm.desc.table_z + height
    return qpos, qvel, ctrl
