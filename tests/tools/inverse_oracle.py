"""Inverse dynamics of a given acceleration (MuJoCo's mj_inverse / data.qfrc_inverse) from the CPU oracle, in NumPy: the reference of
kmanip_inverse.  oracle/ itself knows no inverse and stays as it is.

Oracle.dynamics gives M, bias and the constraint rows J, aref, R of a state, Oracle.constraint_rows their types and friction-loss
bounds.  At an acceleration a the rows' forces are applied_oracle._rows at x = J a - aref (friction-loss rows saturating at +-floss,
limit and contact rows one-sided), and
    qfrc_constraint = J^T f(a),      qfrc_inverse = M a + bias - qfrc_constraint.
The contacts are decoded from the edge forces in force_oracle.decode's row order (friction loss, limits, then the contacts in the
order of the mask's bits; six edges for a pair with the cube, four for a sphere on the table).

The test accelerations of a cell (cell_accels) are the forward solution a*, zero, and a* + s z for s in SCALES with DRAWS standard
normal z each from a fixed seed; `branches` counts which branch of every row type they visit."""
import numpy as np

import applied_oracle as AO
import force_oracle as FO

SCALES = (1.0, 30.0, 1000.0)
DRAWS = 3
N_ACCELS = 2 + len(SCALES) * DRAWS
SEED = 29


def rows_of(orc, qpos, qvel, ctrl):
    """(dyn, types, floss) of one state."""
    dyn = orc.dynamics(qpos, qvel, ctrl)
    types, floss = orc.constraint_rows(qpos, qvel)
    assert len(types) == dyn["nefc"]
    return dyn, types, floss


def inverse(cm, orc, qpos, qvel, ctrl, qacc, rows=None):
    """Everything kmanip_inverse reports for one state and one acceleration: qfrc_inverse, qfrc_constraint [nv], mask, contacts
    {bit: force[4]}, and the row forces f with x = J qacc - aref."""
    d = cm.desc
    nl = cm.nlink
    qpos = np.asarray(qpos, dtype=np.float64); qvel = np.asarray(qvel, dtype=np.float64); qacc = np.asarray(qacc, dtype=np.float64)
    dyn, types, floss = rows_of(orc, qpos, qvel, ctrl) if rows is None else rows
    x = dyn["J"] @ qacc - dyn["aref"]
    f = AO._rows(x, dyn["R"], types, floss)[1] if len(x) else np.zeros(0)
    fc = dyn["J"].T @ f
    mask = int(orc.contact_mask(qpos)[0])
    out = dict(qfrc_inverse=dyn["M"] @ qacc + dyn["bias"] - fc, qfrc_constraint=fc, mask=mask, contacts={}, f=f, x=x, types=types,
               floss=floss, R=dyn["R"])
    row = int((types == 0).sum()) + sum(qpos[j] < d.jnt_range[j][0] or qpos[j] > d.jnt_range[j][1] for j in range(nl))
    for b in FO.mask_bits(mask):
        cube_pair = b < 20
        fr = d.con_cube_friction if cube_pair else d.con_def_friction
        mu, mu3 = float(fr[0]), float(fr[1])
        ne = 6 if cube_pair else 4
        fe = f[row:row + ne]
        out["contacts"][b] = np.array([fe.sum(), mu * (fe[0] - fe[1]), mu * (fe[2] - fe[3]), mu3 * (fe[4] - fe[5]) if cube_pair else 0.0])
        row += ne
    assert row == dyn["nefc"], (row, dyn["nefc"], hex(mask))
    return out


def forward(cm, orc, qpos, qvel, ctrl, tau=None, rows=None):
    """(a*, a_smooth) of one state: the exact minimiser of the forward problem (applied_oracle.newton_exact) under the applied force
    tau (None: none), and the smooth acceleration it starts from."""
    dyn, types, floss = rows_of(orc, qpos, qvel, ctrl) if rows is None else rows
    a_s = dyn["qacc_smooth"] if tau is None else dyn["qacc_smooth"] + np.linalg.solve(dyn["M"], np.asarray(tau, dtype=np.float64))
    return AO.newton_exact(dyn["M"], dyn["J"], dyn["aref"], dyn["R"], types, floss, a_s), a_s


def cell_accels(a_star, env):
    """[N_ACCELS, nv]: a*, 0, a* + s z (s in SCALES, DRAWS draws each); z from default_rng([SEED, env])."""
    rng = np.random.default_rng([SEED, env])
    out = [a_star, np.zeros_like(a_star)]
    for s in SCALES:
        for _ in range(DRAWS):
            out.append(a_star + s * rng.standard_normal(len(a_star)))
    return np.stack(out)


def branches(o):
    """Counts of the branches the rows of one inverse() result are in: friction loss (low, quadratic, high), one-sided (active,
    inactive)."""
    fl = o["types"] == 0
    xf, Rb = o["x"][fl], o["R"][fl] * o["floss"][fl]
    lo, hi = xf <= -Rb, xf >= Rb
    xo = o["x"][~fl]
    return np.array([lo.sum(), (~lo & ~hi).sum(), hi.sum(), (xo < 0).sum(), (xo >= 0).sum()])


def scales(o):
    """Per-env normalisers: (qfrc_inverse, constraint forces) = max(1, max|qfrc_inverse|), max(1, max|qfrc_constraint|)."""
    return max(1.0, float(np.abs(o["qfrc_inverse"]).max())), max(1.0, float(np.abs(o["qfrc_constraint"]).max()))


def spreads(a, b):
    """(qfrc_inverse, qfrc_constraint, contact force) differences between two inverse() results, normalised by scales(a)."""
    si, sf = scales(a)
    assert a["mask"] == b["mask"]
    dc = max([float(np.abs(a["contacts"][k] - b["contacts"][k]).max()) for k in a["contacts"]], default=0.0)
    return (float(np.abs(a["qfrc_inverse"] - b["qfrc_inverse"]).max()) / si,
            float(np.abs(a["qfrc_constraint"] - b["qfrc_constraint"]).max()) / sf, dc / sf)


_CELL_INVERSES = {}


def cell_inverses(asset, params=None):
    """The regime cells of the asset (regime_states.cells) at every test acceleration, computed once per (asset, params) and shared
    by the tests.  params: keyword arguments of model.with_env_params, or None.  dict(cm, qpos, qvel, ctrl, labels, rows, a_star,
    a_smooth, qacc [n, N_ACCELS, nv], ref, twin): ref[e][k] / twin[e][k] are inverse() results, the twin at qvel * (1 + 1e-15) -- the
    distance between the two is the reference's own error."""
    import regime_states as R
    from gym_kmanip_amd.model import with_env_params
    from oracle.oracle import Oracle
    key = (asset, None if params is None else tuple(sorted(params.items())))
    if key not in _CELL_INVERSES:
        cm = R.model(asset)
        if params is not None:
            cm = with_env_params(cm, **params)
        qpos, qvel, ctrl, labels = R.cells(asset)
        orc = Oracle(cm, 1)
        n = len(labels)
        rows, a_star, a_smooth, qacc, ref, twin = [], [], [], [], [], []
        for e in range(n):
            r = rows_of(orc, qpos[e], qvel[e], ctrl[e])
            rt = rows_of(orc, qpos[e], qvel[e] * (1.0 + 1e-15), ctrl[e])
            a, a_s = forward(cm, orc, qpos[e], qvel[e], ctrl[e], rows=r)
            acc = cell_accels(a, e)
            rows.append(r); a_star.append(a); a_smooth.append(a_s); qacc.append(acc)
            ref.append([inverse(cm, orc, qpos[e], qvel[e], ctrl[e], q, rows=r) for q in acc])
            twin.append([inverse(cm, orc, qpos[e], qvel[e] * (1.0 + 1e-15), ctrl[e], q, rows=rt) for q in acc])
        _CELL_INVERSES[key] = dict(cm=cm, qpos=qpos, qvel=qvel, ctrl=ctrl, labels=labels, rows=rows, a_star=np.stack(a_star),
                                   a_smooth=np.stack(a_smooth), qacc=np.stack(qacc), ref=ref, twin=twin)
    return _CELL_INVERSES[key]
