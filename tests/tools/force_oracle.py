"""Contact forces, qfrc_constraint and qfrc_actuator of a state from the CPU oracle, in NumPy: the reference of kmanip_forces.

Oracle.dynamics gives M, bias, qacc_smooth, qacc (Newton from a zero warm start) and the constraint rows J, aref, R of a state;
Oracle.constraint_rows their types and friction-loss bounds; Oracle.contact_mask the KM_CON_* bits.  The row order is
make_constraints' (oracle/kmanip_oracle.c): friction-loss rows, limit rows, then the contacts in collide order -- cube corners by
corner index, sphere-cube by sphere index, sphere-table by sphere index -- which is the order of the mask's bits.  A contact's rows
are its pyramid edges J_0 +- mu_k J_k, ordered (+mu, -mu) for tangent 1, tangent 2, then torsion: 6 rows for a pair with the cube
(condim 4), 4 for a sphere on the table (condim 3).  With f_e the edge forces, MuJoCo's mj_contactForce decode is
    normal = sum_e f_e,   tangent_k = mu (f_k+ - f_k-),   torsion = mu_torsion (f_3+ - f_3-)
and J^T f over ALL rows is qfrc_constraint = M (qacc - qacc_smooth).  qfrc_actuator = M qacc_smooth + bias.

The geometry of a contact (point, frame, distance) is not an output of the oracle's Python interface: contact_geometry restates
collide in NumPy from Oracle.fk, and the frame's first two rows are cross-checked against the rows of J in decode."""
import numpy as np

from regime_states import quat2mat


def row_forces(dyn, types, floss):
    """Force of every constraint row at the oracle's qacc (row_cost of the oracle: saturating friction loss, one-sided rows)."""
    x = dyn["J"] @ dyn["qacc"] - dyn["aref"]
    R = dyn["R"]
    f = np.where(x < 0, -x / R, 0.0)
    fl = types == 0
    f[fl] = np.clip(-x[fl] / R[fl], -floss[fl], floss[fl])
    return f


def mask_bits(mask):
    return [b for b in range(32) if mask >> b & 1]


def make_frame(n):
    """mju_makeFrame: rows normal, t1, t2."""
    n = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    y = np.array([0.0, 1.0, 0.0]) if -0.5 < n[1] < 0.5 else np.array([0.0, 0.0, 1.0])
    y = y - (n @ y) * n
    y /= np.linalg.norm(y)
    return np.concatenate([n, y, np.cross(n, y)])


def contact_geometry(cm, orc, qpos):
    """{mask bit: (pos[3], frame[9], dist)} of every contact the collision keeps at qpos (collide of the oracle, in NumPy)."""
    d = cm.desc
    nl = cm.nlink
    qpos = np.asarray(qpos, dtype=np.float64)
    mask = int(orc.contact_mask(qpos)[0])
    xpos, xquat, _, _ = orc.fk(qpos)
    cpos = qpos[nl:nl + 3]
    cmat = quat2mat(qpos[nl + 3:nl + 7] / np.linalg.norm(qpos[nl + 3:nl + 7]))
    half = np.array(d.cube_half)
    up = make_frame([0.0, 0.0, 1.0])
    out = {}
    for b in mask_bits(mask):
        if b < 8:
            c = cpos + cmat @ (half * [(1 if b & 1 else -1), (1 if b & 2 else -1), (1 if b & 4 else -1)])
            dist = c[2] - d.table_z
            out[b] = (c - [0.0, 0.0, 0.5 * dist], up, dist)
            continue
        s = b - 8 if b < 20 else b - 20
        l = d.sphere_link[s]
        lmat = quat2mat(xquat[l])
        ctr = xpos[l] + lmat @ np.array(d.sphere_pos[s])
        rad = d.sphere_radius[s]
        if b >= 20:
            dist = ctr[2] - d.table_z - rad
            out[b] = (ctr - [0.0, 0.0, rad + 0.5 * dist], up, dist)
            continue
        seg = lmat @ np.array(d.sphere_seg[s])
        if seg @ seg > 0:
            ctr = ctr + min(max((cpos - ctr) @ seg / (seg @ seg), 0.0), 1.0) * seg
        loc = cmat.T @ (ctr - cpos)
        cl = np.clip(loc, -half, half)
        if (cl != loc).any():
            nloc = cl - loc
            dist = np.linalg.norm(nloc) - rad
        else:
            dd = half - np.abs(loc)
            best = int(np.argmin(dd))
            nloc = np.zeros(3)
            nloc[best] = -1.0 if loc[best] >= 0 else 1.0
            dist = -dd[best] - rad
        fr = make_frame(cmat @ nloc)
        out[b] = (ctr + fr[:3] * (rad + 0.5 * dist), fr, dist)
    return out


def decode(cm, orc, qpos, qvel, ctrl, geometry=True):
    """Everything kmanip_forces reports for one state, from a one-env oracle:
      qacc, qfrc_constraint, qfrc_actuator   [nv], [nv], [nu]
      jtf                                    J^T f over all rows [nv] (equals qfrc_constraint up to the oracle's solver tolerance)
      mask                                   the KM_CON_* bits
      contacts                               {bit: dict(force[4], normal[3] (from J, None for a sphere-table pair), mu, mu3,
                                             and with geometry: pos[3], frame[9], dist)}; empty for a state without contacts"""
    d = cm.desc
    nl = cm.nlink
    qpos = np.asarray(qpos, dtype=np.float64); qvel = np.asarray(qvel, dtype=np.float64); ctrl = np.asarray(ctrl, dtype=np.float64)
    dyn = orc.dynamics(qpos, qvel, ctrl)
    types, floss = orc.constraint_rows(qpos, qvel)
    assert len(types) == dyn["nefc"]
    mask = int(orc.contact_mask(qpos)[0])
    f = row_forces(dyn, types, floss)
    M = dyn["M"]
    out = dict(qacc=dyn["qacc"], qfrc_constraint=M @ (dyn["qacc"] - dyn["qacc_smooth"]), jtf=dyn["J"].T @ f,
               qfrc_actuator=(M @ dyn["qacc_smooth"] + dyn["bias"])[:nl], bias=dyn["bias"], mask=mask, contacts={})
    row = int((types == 0).sum()) + sum(qpos[j] < d.jnt_range[j][0] or qpos[j] > d.jnt_range[j][1] for j in range(nl))
    geo = contact_geometry(cm, orc, qpos) if geometry else {}
    for b in mask_bits(mask):
        cube_pair = b < 20
        fr = d.con_cube_friction if cube_pair else d.con_def_friction
        mu, mu3 = float(fr[0]), float(fr[1])
        ne = 6 if cube_pair else 4
        fe, Je = f[row:row + ne], dyn["J"][row:row + ne]
        force = np.array([fe.sum(), mu * (fe[0] - fe[1]), mu * (fe[2] - fe[3]), mu3 * (fe[4] - fe[5]) if cube_pair else 0.0])
        c = dict(force=force, mu=mu, mu3=mu3 if cube_pair else 0.0, normal=None)
        if cube_pair:                                        # the cube is the pair's second body: its linear columns of J_0 are the normal
            c["normal"] = 0.5 * (Je[0] + Je[1])[nl:nl + 3]
            if mu > 0:
                c["tangent1"] = (Je[0] - Je[1])[nl:nl + 3] / (2 * mu)
        if geometry:
            c["pos"], c["frame"], c["dist"] = geo[b]
        out["contacts"][b] = c
        row += ne
    assert row == dyn["nefc"], (row, dyn["nefc"], hex(mask))
    return out


def twin(cm, orc, qpos, qvel, ctrl):
    """decode at qvel * (1 + 1e-15): the distance between the two evaluations is the reference's own error at the state (the
    yardstick of tests/test_regimes_gpu.py)."""
    return decode(cm, orc, qpos, np.asarray(qvel, dtype=np.float64) * (1.0 + 1e-15), ctrl, geometry=False)


def scales(o):
    """Per-env normalisers of the bars: (qacc, forces, qfrc_actuator) = max(1, max|qacc|), max(1, max|qfrc_constraint|), and the
    servo forces' own maximum -- but never less than the largest arm bias force.  The oracle forms a servo force as the sum
    M qacc_smooth + bias of two terms of the bias's size, so that size is what its rounding error scales with: where every servo sits
    on its target (ctrl == qpos exactly: the home pose, whose values are float32 numbers) the true force is 0, the oracle's is
    1e-14 of rounding noise, and a normaliser of "its own maximum" alone would divide noise by noise (a spread of 4.0, measured)."""
    nl = len(o["qfrc_actuator"])
    fa = max(float(np.abs(o["qfrc_actuator"]).max()), float(np.abs(o["bias"][:nl]).max()))
    return max(1.0, float(np.abs(o["qacc"]).max())), max(1.0, float(np.abs(o["qfrc_constraint"]).max())), fa


def spreads(a, b):
    """(qacc, qfrc_constraint, contact force, qfrc_actuator) differences between two decodes of one state, normalised by scales(a)."""
    sq, sf, sa = scales(a)
    assert a["mask"] == b["mask"]
    dc = max([float(np.abs(a["contacts"][k]["force"] - b["contacts"][k]["force"]).max()) for k in a["contacts"]], default=0.0)
    return (float(np.abs(a["qacc"] - b["qacc"]).max()) / sq, float(np.abs(a["qfrc_constraint"] - b["qfrc_constraint"]).max()) / sf,
            dc / sf, float(np.abs(a["qfrc_actuator"] - b["qfrc_actuator"]).max()) / sa)


_CELL_DECODES = {}


def cell_decodes(asset):
    """(cm, decode of every regime cell's copy (regime_states.cells), its twin), computed once per asset and shared by the tests."""
    import regime_states as R
    from oracle.oracle import Oracle
    if asset not in _CELL_DECODES:
        cm = R.model(asset)
        qpos, qvel, ctrl, labels = R.cells(asset)
        orc = Oracle(cm, 1)
        dec = [decode(cm, orc, qpos[e], qvel[e], ctrl[e]) for e in range(len(labels))]
        tw = [twin(cm, orc, qpos[e], qvel[e], ctrl[e]) for e in range(len(labels))]
        _CELL_DECODES[asset] = (cm, dec, tw)
    return _CELL_DECODES[asset]
