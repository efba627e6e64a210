"""States of the step that random rollouts (almost) never reach, built on the CPU oracle alone (oracle + NumPy; no GPU).

Every parity test of k_step draws its states from a reset followed by uniform random actions.  Such rollouts hardly ever hold the
cube between two fingers, never between two arms, and rarely push a whole inertia block beyond its joint ranges -- the states the
task exists for and the ones in which kmanip_dyn_newton.hpp branches most (the joint problem KM_SUB_ALL against the split ones, the
hand-over out of the joint loop, the Woodbury shortcut at two / three quadratic rows per block, the per-block solves of the two-arm
models).  This module builds those states ("cells") directly and classifies any state into them:

  regime(cm, orc, qpos, qvel, ctrl)   what a state contains (contacts per arm, cube corners, joints beyond range per inertia block,
                                      servos at their force limit, ...)
  BUILDERS[cell](cm, orc, rng)        (qpos, qvel, ctrl) of J jittered copies of the cell, or None where the model cannot reach it
  IN_CELL[cell](regime dict)          the cell's own membership test
  census(...)                         how many samples of each cell the random-rollout recipe of the step matrix reaches

Poses that need the hand somewhere else are reached with Oracle.ik in a loop (move_site); no joint value is typed in by hand.
Models are the three assets in the joint-delta action mode (tests/tools/mujoco_pin.qpos_spec: no IK between action and ctrl) or the
registered EE-delta ids; a builder only reads the descriptor, so it serves both.

What before_step does with a built state's ctrl (env_sim.py:38-108, oracle before_step): the entries of the joints an action key
drives are overwritten at the first control step -- the arm joints with float32(qpos + 0.1 a) in the joint-delta mode, BOTH finger
servos of an arm with clip(float32(qpos[first slider] + 1e-4 a), ee_s_min, ee_s_max).  A squeeze written into ctrl therefore does
not survive the first before_step; the builders put it into the state instead: the second slider of a grasping hand is left
SQUEEZE further open than the first, so that every before_step commands it inward by kp * SQUEEZE again (squeeze_of)."""
import numpy as np

from gym_kmanip_amd.model import sphere_arm

J_COPIES = 6
CUBE_CLEAR = 1e-3            # "clear of the table": lowest cube corner more than 1 mm above it
PEN_JITTER = 1e-3            # +-1 mm of penetration
VEL_JITTER = 0.5             # +-0.5 in qvel


# ------------------------------------------------------------------------------------------------------------------ geometry
def quat2mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def mat2quat(m):
    """wxyz of a rotation matrix (largest-pivot branch), normalised, w >= 0."""
    t = np.trace(m)
    cands = [np.array([1 + t, m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]]),
             np.array([m[2, 1] - m[1, 2], 1 + 2 * m[0, 0] - t, m[0, 1] + m[1, 0], m[0, 2] + m[2, 0]]),
             np.array([m[0, 2] - m[2, 0], m[0, 1] + m[1, 0], 1 + 2 * m[1, 1] - t, m[1, 2] + m[2, 1]]),
             np.array([m[1, 0] - m[0, 1], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], 1 + 2 * m[2, 2] - t])]
    q = max(cands, key=lambda c: abs(c[int(np.argmax(np.abs(c)))]))
    q = q / np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def frame_along(axis, angle):
    """A rotation matrix whose first column is `axis` (normalised), turned by `angle` about it."""
    x = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    h = np.array([0.0, 0.0, 1.0]) if abs(x[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    y0 = np.cross(h, x); y0 /= np.linalg.norm(y0)
    z0 = np.cross(x, y0)
    y = np.cos(angle) * y0 + np.sin(angle) * z0
    return np.stack([x, y, np.cross(x, y)], axis=1)


def sphere_centres(cm, orc, qpos):
    """World centres of the collision spheres (sphere_pos in sphere_link's frame; the capsule sections are not applied)."""
    d = cm.desc
    xpos, xquat, _, _ = orc.fk(qpos)
    return np.stack([xpos[d.sphere_link[s]] + quat2mat(xquat[d.sphere_link[s]]) @ np.array(d.sphere_pos[s]) for s in range(d.nsphere)])


def cube_corners_z(cm, qpos):
    """Height of the 8 cube corners over the table top."""
    d = cm.desc
    nl = cm.nlink
    R = quat2mat(qpos[nl + 3:nl + 7] / np.linalg.norm(qpos[nl + 3:nl + 7]))
    h = np.array(d.cube_half)
    return np.array([(qpos[nl:nl + 3] + R @ (h * [(1 if i & 1 else -1), (1 if i & 2 else -1), (1 if i & 4 else -1)]))[2] - d.table_z
                     for i in range(8)])


def blocks(cm):
    """The inertia blocks of the joint-space matrix as kmanip_create splits them (kmanip_api.hip: the most balanced s in {10, 11}
    such that no link >= s has an ancestor < s): [(0, 10)] for the single arm, DualArm 10 + 10, Torso 11 + 9."""
    d = cm.desc
    nl = cm.nlink
    best = None
    for s in (10, 11):
        if nl == 20 and all(d.link_parent[i] < 0 or d.link_parent[i] >= s for i in range(s, nl)):
            if best is None or max(s, nl - s) < max(best, nl - best):
                best = s
    return [(0, nl)] if best is None else [(0, best), (best, nl)]


def n_arms(cm):
    return cm.nlink // 10


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- classifier
def regime(cm, orc, qpos, qvel, ctrl):
    """What one state contains.  From Oracle.contact_mask (the KM_CON_* bits of the collision at qpos), Oracle.constraint_rows
    (the rows the solver gets: their count must be the one the bits and the limits imply), Oracle.fk (cube clearance),
    model.sphere_arm and the descriptor (ranges, kp, forcerange)."""
    d = cm.desc
    nl = cm.nlink
    qpos = np.asarray(qpos, dtype=np.float64); qvel = np.asarray(qvel, dtype=np.float64); ctrl = np.asarray(ctrl, dtype=np.float64)
    mask = int(orc.contact_mask(qpos)[0])
    arms = sphere_arm(cm)
    nf = 2 * n_arms(cm)
    na = n_arms(cm)
    corners = bin(mask & 0xFF).count("1")
    finger_cube = [0] * na; link_cube = [0] * na; sphere_table = [0] * na
    for s in range(d.nsphere):
        if mask >> (8 + s) & 1:
            (finger_cube if s < nf else link_cube)[arms[s]] += 1
        if mask >> (20 + s) & 1:
            sphere_table[arms[s]] += 1
    blk = blocks(cm)
    beyond = [j for j in range(nl) if qpos[j] < d.jnt_range[j][0] or qpos[j] > d.jnt_range[j][1]]
    limits = [sum(lo <= j < hi for j in beyond) for lo, hi in blk]
    outward = all((qvel[j] < 0) == (qpos[j] < d.jnt_range[j][0]) and qvel[j] != 0 for j in beyond)
    # the rows the solver sees: friction loss (type 0), then one-sided rows = limits + 6 per cube contact + 4 per sphere-table one
    t, _ = orc.constraint_rows(qpos, qvel)
    n_sc = bin(mask >> 8 & 0xFFF).count("1"); n_st = bin(mask >> 20 & 0xFFF).count("1")
    assert int((t == 1).sum()) == len(beyond) + 6 * (corners + n_sc) + 4 * n_st, (hex(mask), beyond, int((t == 1).sum()))
    sat = []
    for j in range(nl):
        if d.forcelimited[j] and d.kp[j] > 0:
            c = min(max(ctrl[j], d.ctrlrange[j][0]), d.ctrlrange[j][1])
            f = d.kp[j] * (c - qpos[j])
            if f < d.forcerange[j][0] or f > d.forcerange[j][1]:
                sat.append(j)
    return dict(mask=mask, corners=corners, corners_bin="0" if corners == 0 else ("4" if corners == 4 else "1-3"),
                finger_cube=finger_cube, link_cube=link_cube, sphere_cube=n_sc, sphere_table=sphere_table, n_sphere_table=n_st,
                limits=limits, limits_outward=outward, saturated=sat,
                cube_clear=bool(cube_corners_z(cm, qpos).min() > CUBE_CLEAR), cube_low=float(cube_corners_z(cm, qpos).min()),
                cube_speed=float(np.linalg.norm(qvel[nl:nl + 3])), cube_spin=float(np.linalg.norm(qvel[nl + 3:nl + 6])),
                squeeze=[squeeze_of(cm, qpos, a) for a in range(na)], coupled=bool(mask & 0x000FFF00))


def squeeze_of(cm, qpos, arm):
    """The inward command every before_step renews on arm's second finger: both finger servos get clip(qpos[first slider]
    (+ 1e-4 a)), so the second slider is commanded by qpos[second] - clip(qpos[first]) metres towards closing (lower = closed)."""
    d = cm.desc
    g0, g1 = d.arm_grip_id[arm]
    return float(qpos[g1] - min(max(qpos[g0], d.ee_s_min), d.ee_s_max))


# ------------------------------------------------------------------------------------------------------------------- helpers
def home_state(cm, orc):
    """(qpos, qvel, ctrl) of the reset pose with the cube parked at rest on a far corner of the table (4 corners down, clear of
    both arms): cells about the arm alone keep the cube's own rows in the problem, in a sub-problem of their own."""
    d = cm.desc
    nl = cm.nlink
    qpos = np.zeros(cm.nq)
    qpos[:nl] = np.array(d.q_home[:nl])
    qpos[nl:nl + 3] = [d.table_rect[1] - 0.06, d.table_rect[3] - 0.04, d.table_z + d.cube_half[2] - 2e-4]
    qpos[nl + 3] = 1.0
    return qpos, np.zeros(cm.nv), f32(qpos[:nl])


def arm_joints(cm, arm):
    d = cm.desc
    return [d.arm_q_id[arm][i] for i in range(d.arm_nq[arm])]


def move_site(cm, orc, qpos, arm, delta=None, until=None, step=0.01, max_iter=80):
    """Repeated Oracle.ik(arm, ...) calls that carry the arm's site along `delta` (metres, world) in steps of at most `step`, the
    site's orientation kept, or -- with `until` -- by `step` along delta's direction until until(qpos) is true.  Returns the new
    qpos (the cube's entries untouched); raises if the IK stalls (the site moved by less than a tenth of the step asked for)."""
    qpos = np.array(qpos, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    ids = arm_joints(cm, arm)
    if until is None:
        if np.linalg.norm(delta) < 2e-5:                 # below what the IK resolves
            return qpos
        n = max(1, int(np.ceil(np.linalg.norm(delta) / step)))
        inc = delta / n
    else:
        n = max_iter
        inc = delta / np.linalg.norm(delta) * step
    for _ in range(n):
        if until is not None and until(qpos):
            return qpos
        _, _, sp, sm = orc.fk(qpos)
        q, _, _, st = orc.ik(arm, qpos, sp[arm] + inc, mat2quat(sm[arm]))
        if st == -2:                                     # x0 infeasible (a float32 home value a hair outside its range): start inside
            d = cm.desc
            qpos[ids] = np.clip(qpos[ids], [d.jnt_range[j][0] + 1e-6 for j in ids], [d.jnt_range[j][1] - 1e-6 for j in ids])
            q, _, _, st = orc.ik(arm, qpos, sp[arm] + inc, mat2quat(sm[arm]))
        qpos[ids] = q
        moved = orc.fk(qpos)[2][arm] - sp[arm]
        if np.linalg.norm(inc) > 5e-4 and np.linalg.norm(moved) < 0.1 * np.linalg.norm(inc):
            raise RuntimeError("IK stalled (status %d) moving arm %d" % (st, arm))
    if until is not None and not until(qpos):
        raise RuntimeError("move_site: condition not reached in %d IK steps" % max_iter)
    return qpos


def set_finger_gap(cm, orc, qpos, arm, gap, first_only=False):
    """Both sliders of `arm` (first_only: its first slider alone) set so that its finger-sphere centres are `gap` apart: the
    distance is linear in the slider values, measured at the two ends of the range."""
    d = cm.desc
    g0, g1 = d.arm_grip_id[arm]
    lo, hi = d.jnt_range[g0]

    def put(s):
        q = qpos.copy()
        q[g0] = s
        if not first_only:
            q[g1] = s
        return q

    def dist(s):
        c = sphere_centres(cm, orc, put(s))
        return np.linalg.norm(c[2 * arm] - c[2 * arm + 1])
    s = lo + (gap - dist(lo)) / (dist(hi) - dist(lo)) * (hi - lo)
    assert lo <= s <= hi, (s, lo, hi)
    return put(s)


def jitter_qvel(cm, rng, n=1, cube_free=False):
    """+-0.5 rad/s on the hinges and the cube's rotation; a tenth of it (m/s) on the slides -- 0.5 m/s would carry a finger across
    its whole 34 mm of travel inside one control step -- and on the translation of a cube that fingers hold or push (0.5 m/s would
    take it 1 cm out of a 2 mm contact).  cube_free: nothing touches the cube but the table: the full +-0.5 m/s."""
    d = cm.desc
    nl = cm.nlink
    lin = VEL_JITTER if cube_free else 0.1 * VEL_JITTER
    scale = np.array([VEL_JITTER if d.jnt_type[j] == 0 else 0.1 * VEL_JITTER for j in range(nl)] + [lin] * 3 + [VEL_JITTER] * 3)
    return rng.uniform(-1, 1, (n, cm.nv)) * scale


def _stack(states):
    return tuple(np.stack([s[k] for s in states]) for k in range(3))


SQUEEZE = 0.004              # the second finger of a grasp is commanded 4 mm further in


def grasp(cm, orc, qpos, arm, rng, pen=0.002, angle=None, squeeze=SQUEEZE):
    """The cube between arm's two finger spheres at the hand's current pose: finger centres 0.06 m - 2 pen apart (cube 0.04 m,
    finger radius 0.01 m: each finger `pen` inside), the cube at their midpoint with its x axis along the finger axis, turned by
    `angle` about it.  The second slider is left `squeeze` further open than the first (squeeze_of): it is opened by half of it
    and the first closed by as much, so the gap and both penetrations stay what they were."""
    d = cm.desc
    nl = cm.nlink
    g0, g1 = d.arm_grip_id[arm]
    q = set_finger_gap(cm, orc, qpos, arm, 2 * (d.cube_half[0] + d.sphere_radius[2 * arm] - pen))
    lo, hi = d.jnt_range[g1]
    q[g1] = min(q[g1] + 0.5 * squeeze, hi)
    # opening the second finger by half the squeeze widened the gap: close the first by as much
    q = set_finger_gap(cm, orc, q, arm, 2 * (d.cube_half[0] + d.sphere_radius[2 * arm] - pen), first_only=True)
    c = sphere_centres(cm, orc, q)
    a, b = c[2 * arm], c[2 * arm + 1]
    q[nl:nl + 3] = 0.5 * (a + b)
    q[nl + 3:nl + 7] = mat2quat(frame_along(b - a, rng.uniform(0, 2 * np.pi) if angle is None else angle))
    return q


def _ctrl_of(cm, qpos):
    """float32(qpos) for every actuator: what before_step leaves for a zero action (the grasping fingers' entries are renewed by
    it anyway)."""
    return f32(qpos[:cm.nlink])


# ------------------------------------------------------------------------------------------------------------------ builders
def pen_centre(cm):
    """Penetration of a grasping finger, the centre of the +-1 mm jitter: 2 mm where the finger slides have friction loss (SoloArm,
    DualArm: 30 N), 4 mm on the Torso, whose slides have none and a servo of kp 100 -- the contact opens its fingers by 1-2 mm
    within a control step, and at 2 mm only 7 of 18 G2 copies still held the cube after one (16 of 18 at 4 mm)."""
    g = cm.desc.arm_grip_id[0][0]
    return 0.002 if cm.desc.frictionloss[g] > 0 else 0.004


def _pens(rng, n, centre=0.002):
    return centre + rng.uniform(-PEN_JITTER, PEN_JITTER, n)


def build_G1(cm, orc, rng):
    """Two-finger grasp in the air at the home pose, arm 0 and (two-arm models) arm 1 in alternate copies: mask = the arm's two
    finger bits, no corner on the table.  Retention on the oracle (copies still holding both finger bits after one control step,
    zero action, newton and pgs): SoloArm 6/6, DualArm 6/6, Torso 6/6.  With a zero action every servo is re-targeted at the
    joint's current position, so the arm sinks and the contact opens the fingers: the grasp is gone after 2-3 steps (held_cube
    shows the grasp that lasts)."""
    d = cm.desc
    q0, _, _ = home_state(cm, orc)
    raised = {}
    out = []
    for i, pen in enumerate(_pens(rng, J_COPIES, pen_centre(cm))):
        arm = i % n_arms(cm)
        if arm not in raised:                                # (the Torso's left hand starts 2.6 cm over the table: lift it to 8 cm)
            c = sphere_centres(cm, orc, q0)
            low = 0.5 * (c[2 * arm] + c[2 * arm + 1])[2] - d.table_z < 0.07
            raised[arm] = _lower_hand(cm, orc, q0, arm, 0.08) if low else q0
        q = grasp(cm, orc, raised[arm], arm, rng, pen=pen)
        out.append((q, jitter_qvel(cm, rng)[0], _ctrl_of(cm, q)))
    return _stack(out)


def _lower_hand(cm, orc, q0, arm, height, inward=0.0):
    """The hand of `arm` brought (Oracle.ik loop) to where the midpoint of its finger spheres is `height` over the table top and,
    for hands that start over the table's edge, at least `inward` metres inside the table rectangle in y."""
    d = cm.desc

    def mid(q):
        c = sphere_centres(cm, orc, q)
        return 0.5 * (c[2 * arm] + c[2 * arm + 1])
    q = q0
    dy = d.table_rect[2] + inward - mid(q)[1]
    if dy > 0:
        q = move_site(cm, orc, q, arm, [0.0, dy, 0.0])
    for _ in range(3):                                       # the hand turns a little on its way: correct the remainder
        q = move_site(cm, orc, q, arm, [0.0, 0.0, d.table_z + height - mid(q)[2]])
    assert abs(mid(q)[2] - d.table_z - height) < 5e-4, mid(q)
    return q


def build_G2(cm, orc, rng):
    """The grasp with the cube resting on the table on 4 corners: the hand is lowered by IK until the finger midpoint is a cube
    half-height over the table; the cube lies flat, its x axis along the horizontal part of the finger axis, 0.1-0.3 mm into the
    table.  The arm's problem holds the coupling and the cube's corner rows at once (and, where a finger sphere of radius 1 cm at
    2 cm height tilts down, a sphere-table row).  Built 1 mm deeper than G1.  Retention: SoloArm 6/6, DualArm 6/6, Torso 4/6."""
    d = cm.desc
    nl = cm.nlink
    q0, _, _ = home_state(cm, orc)
    lowered = {arm: _lower_hand(cm, orc, q0, arm, d.cube_half[2], inward=0.08) for arm in range(n_arms(cm))}
    out = []
    for i, pen in enumerate(_pens(rng, J_COPIES, pen_centre(cm) + 0.001)):
        arm = i % n_arms(cm)
        q = grasp(cm, orc, lowered[arm], arm, rng, pen=pen, angle=0.0)
        c = sphere_centres(cm, orc, q)
        ax = c[2 * arm + 1] - c[2 * arm]
        yaw = np.arctan2(ax[1], ax[0])
        q[nl + 2] = d.table_z + d.cube_half[2] - rng.uniform(1e-4, 3e-4)
        q[nl + 3:nl + 7] = [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]
        out.append((q, jitter_qvel(cm, rng)[0], _ctrl_of(cm, q)))
    return _stack(out)


def build_G3(cm, orc, rng):
    """One finger only on the cube, pushing it along the table: the hand as in G2 with the gripper wide open, the cube flat on 4
    corners against the first finger (2-4 mm inside) and sliding away from it at 5-10 cm/s with the hand following at that speed -- the friction rows of the
    four corners work on the pyramid's edges."""
    d = cm.desc
    nl = cm.nlink
    q0, _, _ = home_state(cm, orc)
    out = []
    lowered = {}
    for i, pen in enumerate(_pens(rng, J_COPIES, 0.003)):
        arm = i % n_arms(cm)
        if arm not in lowered:
            g0, g1 = d.arm_grip_id[arm]
            q = _lower_hand(cm, orc, q0, arm, d.cube_half[2], inward=0.08)
            q[g0] = q[g1] = d.jnt_range[g0][1]
            lowered[arm] = q
        q = lowered[arm].copy()
        c = sphere_centres(cm, orc, q)
        ax = c[2 * arm + 1] - c[2 * arm]
        ax[2] = 0.0
        ax /= np.linalg.norm(ax)
        yaw = np.arctan2(ax[1], ax[0])
        q[nl:nl + 3] = c[2 * arm] + ax * (d.sphere_radius[2 * arm] + d.cube_half[0] - pen)
        q[nl + 2] = d.table_z + d.cube_half[2] - rng.uniform(1e-4, 3e-4)
        q[nl + 3:nl + 7] = [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]
        speed = rng.uniform(0.05, 0.1)
        v = jitter_qvel(cm, rng)[0]
        v[nl:nl + 3] = ax * speed
        ids = arm_joints(cm, arm)                            # the hand follows at the same speed (a finite difference of the IK)
        v[ids] = (move_site(cm, orc, q, arm, 0.002 * ax)[ids] - q[ids]) / 0.002 * speed
        out.append((q, v, _ctrl_of(cm, q)))
    return _stack(out)


def sphere_box_depth(cm, centre, radius, qpos):
    """Penetration (> 0: inside) of a sphere into the cube of qpos, the oracle's sphere-box test for a centre outside the box."""
    nl = cm.nlink
    R = quat2mat(qpos[nl + 3:nl + 7] / np.linalg.norm(qpos[nl + 3:nl + 7]))
    loc = R.T @ (centre - qpos[nl:nl + 3])
    h = np.array(cm.desc.cube_half)
    return radius - np.linalg.norm(loc - np.clip(loc, -h, h))


_PINCH_CACHE = {}


def pinch_approach(cm, orc):
    """Both hands brought together (alternating Oracle.ik steps of each arm's site towards the other's, orientation kept) until
    the sites are less than 6 cm apart.  Returns (qpos, site distance); the distance stays large where the arms cannot meet.
    Measured: Torso 0.050 m after 16 IK steps; DualArm 0.052 m after 20 -- when only ONE arm moves the DualArm's sites stay 0.24 m
    (left arm moving, IK status 2) or 0.20 m (right arm moving) apart, so its pinch exists only with both arms reaching in."""
    key = (cm.spec.asset, cm.spec.env_id)
    if key not in _PINCH_CACHE:
        q, _, _ = home_state(cm, orc)
        stalled = [False, False]
        for it in range(120):
            sp = orc.fk(q)[2]
            n = np.linalg.norm(sp[0] - sp[1])
            if n < 0.06 or all(stalled):
                break
            mover = it % 2
            if stalled[mover]:
                continue
            try:
                q = move_site(cm, orc, q, mover, (sp[1 - mover] - sp[mover]) / n * min(0.02, n - 0.05))
            except RuntimeError:
                stalled[mover] = True
        sp = orc.fk(q)[2]
        _PINCH_CACHE[key] = (q, float(np.linalg.norm(sp[0] - sp[1])))
    q, n = _PINCH_CACHE[key]
    return q.copy(), n


def pinch(cm, orc, rng, pen, angle, close=()):
    """A finger of each arm on the cube (the closest pair of the approach pose, brought to 0.06 m - 2 pen apart by moving the left
    hand along their line), the cube between them, its x axis along the pair, turned by `angle` about it.  close: arms whose OTHER
    finger is then slid in until it is `pen` inside the cube as well (None if its travel does not reach the cube at this angle)."""
    d = cm.desc
    nl = cm.nlink
    q, n = pinch_approach(cm, orc)
    if n >= 0.06:
        return None
    c = sphere_centres(cm, orc, q)
    i, j = min(((i, j) for i in (0, 1) for j in (2, 3)), key=lambda p: np.linalg.norm(c[p[0]] - c[p[1]]))
    target = 2 * (d.cube_half[0] + d.sphere_radius[0] - pen)
    for _ in range(4):
        c = sphere_centres(cm, orc, q)
        v = c[i] - c[j]
        dist = np.linalg.norm(v)
        if abs(dist - target) < 1e-5:
            break
        q = move_site(cm, orc, q, 1, v / dist * (dist - target), step=0.005)
    c = sphere_centres(cm, orc, q)
    assert abs(np.linalg.norm(c[i] - c[j]) - target) < 2e-4, (np.linalg.norm(c[i] - c[j]), target)
    q[nl:nl + 3] = 0.5 * (c[i] + c[j])
    q[nl + 3:nl + 7] = mat2quat(frame_along(c[j] - c[i], angle))
    for arm in close:
        k = 2 * arm + (1 - (i if arm == 0 else j) % 2)        # the arm's other finger
        q = _close_finger(cm, orc, q, k, pen)
        if q is None:
            return None
    return q


def _close_finger(cm, orc, q, k, pen):
    """Slide finger sphere k's own slider from the open end until the sphere is `pen` inside the cube; None if its travel never
    brings it that deep."""
    d = cm.desc
    arm = sphere_arm(cm)[k]
    g = d.arm_grip_id[arm][k % 2]
    lo, hi = d.jnt_range[g]
    ss = np.linspace(hi, lo, 137)
    prev = None
    for s in ss:
        qq = q.copy(); qq[g] = s
        dep = sphere_box_depth(cm, sphere_centres(cm, orc, qq)[k], d.sphere_radius[k], qq)
        if dep >= pen:
            if prev is not None and dep > prev[1]:
                s = prev[0] + (s - prev[0]) * (pen - prev[1]) / (dep - prev[1])
            qq[g] = s
            return qq
        prev = (s, dep)
    return None


def both_hands_on_cube(cm, orc, pen, angle):
    """Arm 0 grasps the cube as in G1 (at the pinch approach pose, cube turned by `angle` about its finger axis); arm 1's hand is
    then carried (Oracle.ik) to where the midpoint of ITS fingers is the cube's centre and its two fingers are slid in until each
    is `pen` inside a face: four finger spheres on the cube, all KM_SPHERE_SLOTS of the 20-link kernels in use.  (The model has no
    hand-hand collision, so the hands may overlap.)  None where a finger's travel does not reach."""
    d = cm.desc
    nl = cm.nlink
    q, n = pinch_approach(cm, orc)
    if n >= 0.06:
        return None
    g0, g1 = d.arm_grip_id[1]
    q[g0] = q[g1] = d.jnt_range[g0][1]
    for _ in range(6):                                       # the two finger midpoints brought together, whichever arm can move
        c = sphere_centres(cm, orc, q)
        delta = 0.5 * (c[0] + c[1]) - 0.5 * (c[2] + c[3])
        if np.linalg.norm(delta) < 1e-4:
            break
        try:
            q = move_site(cm, orc, q, 1, delta, step=0.005)
        except RuntimeError:
            try:
                q = move_site(cm, orc, q, 0, -delta, step=0.005)
            except RuntimeError:
                return None
    q = grasp(cm, orc, q, 0, None, pen=pen, angle=angle, squeeze=0.0)
    for k in (2, 3):
        q = _close_finger(cm, orc, q, k, pen)
        if q is None:
            return None
    return q


def build_P1(cm, orc, rng):
    """Two-arm pinch: one finger of each arm on the cube (mask 0x900: fingers 0 and 3), both arms' inertia blocks tied together
    through the cube.  Torso and -- with both arms reaching in (pinch_approach) -- DualArm; None for the single arm."""
    if n_arms(cm) < 2:
        return None
    out = []
    for pen in _pens(rng, J_COPIES, pen_centre(cm)):
        q = pinch(cm, orc, rng, pen, rng.uniform(0, 2 * np.pi))
        if q is None:
            return None
        out.append((q, jitter_qvel(cm, rng)[0], _ctrl_of(cm, q)))
    return _stack(out)


def build_P2(cm, orc, rng):
    """Three and four sphere-cube slots in use (KM_SPHERE_SLOTS = 4 on the 20-link kernels): arm 0 holds the cube between its two
    fingers, arm 1's hand is carried over it and closes one finger (odd copies: 3 slots) or both (even copies: 4 slots)
    (both_hands_on_cube).  None for the single arm, whose 2 slots G1 fills."""
    if n_arms(cm) < 2:
        return None
    d = cm.desc
    out = []
    for i, pen in enumerate(_pens(rng, J_COPIES, pen_centre(cm) + 0.001)):
        q = both_hands_on_cube(cm, orc, pen, rng.uniform(0, 2 * np.pi))
        if q is None:
            return None
        if i % 2:                                            # three slots: the left hand's second finger opened again
            g = d.arm_grip_id[1][1]
            q[g] = d.jnt_range[g][1]
        out.append((q, jitter_qvel(cm, rng)[0], _ctrl_of(cm, q)))
    return _stack(out)


def build_P3(cm, orc, rng):
    """A fifth penetrating sphere, so that device and oracle must drop the same one: NOT REACHABLE.  After the four fingers the
    next spheres in slot order are the palms (radius 3 cm).  With four fingers on the cube (P2, 8 angles about the grasp axis) the
    nearer palm stays 42.3 mm clear of the cube on the Torso and 22.3 mm on the DualArm: the palm sits behind the finger tips by
    more than a cube width, and the hand is rigid but for the finger slides.  Nothing is built; test_sphere_slot_overflow_parity
    (a rigged model) stays the only overflow test."""
    return None


def _place_on_corners(cm, R, k, pen, rng):
    """Cube centre height at which exactly the k lowest corners of orientation R are under the table top, the k-th by `pen`;
    None unless the (k+1)-th then stays at least 0.5 mm clear."""
    h = np.array(cm.desc.cube_half)
    z = np.sort([(R @ (h * [(1 if i & 1 else -1), (1 if i & 2 else -1), (1 if i & 4 else -1)]))[2] for i in range(8)])
    if z[k] - z[k - 1] < pen + 5e-4:
        return None
    return cm.desc.table_z - z[k - 1] - pen


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def build_C1(cm, orc, rng):
    """The free cube tilted onto exactly 1, 2 and 3 corners (two copies each), 0.1-0.5 mm into the table, with 2-5 rad/s of
    angular velocity about a random axis; the arm rests at home.  1: a corner down (the body diagonal near the vertical);
    2: an edge down (45 degrees about a face axis, the edge level to 0.3 mm); 3: a face tilted 2-4 degrees about its diagonal,
    lowered until three of its corners are under."""
    d = cm.desc
    nl = cm.nlink
    q0, _, _ = home_state(cm, orc)
    out = []
    for i in range(J_COPIES):
        k = 1 + i % 3
        while True:
            yaw = _rot([0, 0, 1], rng.uniform(0, 2 * np.pi))
            if k == 1:
                R = yaw @ _rot([1, 0, 0], np.arctan(np.sqrt(2)) + rng.uniform(-0.1, 0.1)) @ _rot([0, 0, 1], np.pi / 4 + rng.uniform(-0.1, 0.1))
            elif k == 2:
                R = yaw @ _rot([0, 1, 0], rng.uniform(-0.005, 0.005)) @ _rot([1, 0, 0], np.pi / 4 + rng.uniform(-0.2, 0.2))
            else:
                R = yaw @ _rot([1, 1, 0], np.deg2rad(rng.uniform(2, 4)))
            pen = rng.uniform(1e-4, 5e-4)
            z = _place_on_corners(cm, R, k, pen, rng)
            if z is not None:
                break
        q = q0.copy()
        q[nl + 2] = z
        q[nl + 3:nl + 7] = mat2quat(R)
        v = jitter_qvel(cm, rng, cube_free=True)[0]
        w = rng.normal(size=3)
        v[nl + 3:nl + 6] = w / np.linalg.norm(w) * rng.uniform(2, 5)
        out.append((q, v, _ctrl_of(cm, q)))
    return _stack(out)


def build_C2(cm, orc, rng):
    """The free cube 1-3 mm over the table (lowest corner), at a random orientation, moving at 3 m/s (1-2 m/s of it downwards)
    and spinning at 30 rad/s: the quaternion integration at a rotation of 0.06 rad per sub-step and the first impact, inside the
    first control step."""
    d = cm.desc
    nl = cm.nlink
    q0, _, _ = home_state(cm, orc)
    out = []
    for i in range(J_COPIES):
        qq = rng.normal(size=4)
        qq /= np.linalg.norm(qq)
        q = q0.copy()
        q[nl + 3:nl + 7] = qq if qq[0] >= 0 else -qq
        q[nl:nl + 2] = [0.5 * (d.table_rect[0] + d.table_rect[1]) + 0.2, 0.5 * (d.table_rect[2] + d.table_rect[3]) + 0.1]
        q[nl + 2] += rng.uniform(1e-3, 3e-3) - cube_corners_z(cm, q).min()
        v = jitter_qvel(cm, rng, cube_free=True)[0]
        vz = -rng.uniform(1, 2)
        phi = rng.uniform(0, 2 * np.pi)
        vh = np.sqrt(9.0 - vz * vz)
        v[nl:nl + 3] = [vh * np.cos(phi), vh * np.sin(phi), vz]
        w = rng.normal(size=3)
        v[nl + 3:nl + 6] = w / np.linalg.norm(w) * 30.0
        out.append((q, v, _ctrl_of(cm, q)))
    return _stack(out)


def _in_range_home(cm, orc):
    """home_state with every joint strictly inside its range (the Torso's home pose itself has three joints beyond theirs:
    5, 11 and 14 sit at +-1.6 / -1.7 rad against a range of +-1.5708)."""
    d = cm.desc
    q, v, _ = home_state(cm, orc)
    for j in range(cm.nlink):
        lo, hi = d.jnt_range[j]
        q[j] = min(max(q[j], lo + 1e-3 * (hi - lo)), hi - 1e-3 * (hi - lo))
    return q, v, _ctrl_of(cm, q)


def _push_beyond(cm, orc, q, v, joints, rng):
    """Each of `joints` put 0.01-0.03 rad (slides: 0.3-1 mm) beyond the nearer end of its range, moving further out at
    0.2-0.5 rad/s (a tenth of it in m/s for slides)."""
    d = cm.desc
    for j in joints:
        lo, hi = d.jnt_range[j]
        slide = d.jnt_type[j] == 1
        over = rng.uniform(0.01, 0.03) * (1.0 / 30 if slide else 1.0)
        speed = rng.uniform(0.2, 0.5) * (0.1 if slide else 1.0)
        up = abs(hi - q[j]) <= abs(q[j] - lo)
        q[j] = hi + over if up else lo - over
        v[j] = speed if up else -speed


def _limit_candidates(cm, orc, blk):
    """Joints of block `blk` that can sit beyond the nearer end of their range with no sphere touching anything: tried one at a
    time from the in-range home pose, nearest-to-its-limit first."""
    d = cm.desc
    q0, _, _ = _in_range_home(cm, orc)
    lo, hi = blocks(cm)[blk]
    cand = []
    for j in range(lo, hi):
        a, b = d.jnt_range[j]
        q = q0.copy()
        q[j] = b + 0.03 if abs(b - q[j]) <= abs(q[j] - a) else a - 0.03
        if not int(orc.contact_mask(q)[0]) & 0xFFFFFF00:
            cand.append((min(abs(b - q0[j]), abs(q0[j] - a)) / (b - a), j))
    return [j for _, j in sorted(cand)]


def build_L1(cm, orc, rng):
    """Exactly 1, 2, 3 and 4 joints of one inertia block beyond their range and moving further out -- the limit rows are
    quadratic rows of the arm problem, and 2 / 3 is where the Woodbury shortcut ends, per block.  Single arm: k = 1..4 (4 copies).
    Two-arm models, for each block as the primary one: k = 1..4 with the other block inside its ranges, then with 3 joints of the
    other block beyond theirs too (16 copies).  The joints are those nearest to an end of their range at home; the cube rests on
    the table out of reach."""
    nb = len(blocks(cm))
    cands = [_limit_candidates(cm, orc, b) for b in range(nb)]
    assert all(len(c) >= 4 for c in cands), cands
    out = []
    for prim in range(nb):
        for other in ((0,) if nb == 1 else (0, 3)):
            for k in (1, 2, 3, 4):
                q, v, _ = _in_range_home(cm, orc)
                v = jitter_qvel(cm, rng, cube_free=True)[0]
                joints = list(cands[prim][:k]) + (list(cands[1 - prim][:other]) if nb == 2 else [])
                _push_beyond(cm, orc, q, v, joints, rng)
                out.append((q, v, _ctrl_of(cm, q)))
    return _stack(out)


def build_F1(cm, orc, rng):
    """A position servo at its force limit: kp |clip(ctrl) - q| > forcerange.  forcelimited per model: SoloArm / DualArm every arm
    joint (kp 1000, +-100 N m; the finger slides are not limited), Torso all 20 (kp 100, +-100).  In the joint-delta action mode
    before_step renews an arm joint's ctrl as float32(q + 0.1 a), |a| <= 1: kp * 0.1 = 100 (SoloArm / DualArm) or 10 (Torso) can
    never pass the limit by the action alone.  Two ways remain and both are built, in alternate copies where the model has both:
      (a) a joint more than forcerange / kp beyond its range: ctrlrange clips the target to the range's end -- 0.11-0.14 rad
          beyond on SoloArm / DualArm (also one limit row); on the Torso that would take 1 rad and is not built;
      (b) an actuated joint no action key drives keeps the state's ctrl: the Torso's head joints 0, 1 and its hand joints 10, 19
          (kp 100): ctrl 1.1-1.4 rad away from q, inside ctrlrange.  SoloArm / DualArm have only joint 7 / 17 of that kind, with
          kp 0."""
    d = cm.desc
    nl = cm.nlink
    driven = set()
    for a in range(n_arms(cm)):
        driven |= set(arm_joints(cm, a)) | set(d.arm_grip_id[a])
    free = [j for j in range(nl) if j not in driven and d.forcelimited[j] and d.kp[j] > 0]
    lim = [j for b in range(len(blocks(cm))) for j in _limit_candidates(cm, orc, b)
           if j in driven and d.forcelimited[j] and d.jnt_type[j] == 0 and d.forcerange[j][1] / d.kp[j] < 0.2]
    out = []
    for i in range(J_COPIES):
        q, v, _ = _in_range_home(cm, orc)
        v = jitter_qvel(cm, rng, cube_free=True)[0]
        c = _ctrl_of(cm, q)
        if free and (i % 2 == 0 or not lim):
            j = free[(i // 2 if lim else i) % len(free)]
            need = d.forcerange[j][1] / d.kp[j]
            lo, hi = d.ctrlrange[j]
            t = q[j] + rng.uniform(1.1, 1.4) * need
            if t > hi:
                t = q[j] - rng.uniform(1.1, 1.4) * need
            assert lo <= t <= hi, (j, t)
            c[j] = f32(t)
        else:
            j = lim[(i // 2) % len(lim)]
            lo, hi = d.jnt_range[j]
            over = d.forcerange[j][1] / d.kp[j] * rng.uniform(1.1, 1.4)
            up = abs(hi - q[j]) <= abs(q[j] - lo)
            q[j] = hi + over if up else lo - over
            v[j] = rng.uniform(0.2, 0.5) * (1 if up else -1)
            c = _ctrl_of(cm, q)
        out.append((q, v, c))
    return _stack(out)


T1_MAX_DEPTH = 6e-3
_T1_CACHE = {}


def table_poses(cm, orc, arm):
    """{n: qpos} for n = 1, 2, 3: the arm lowered (Oracle.ik, 0.5 mm a step, from 3 cm up, gripper closed so that both fingers
    are level to a few mm) to the first pose with n of ITS spheres on the table (fingers first, then the palm), 0.3 mm past it;
    only poses whose deepest sphere is less than T1_MAX_DEPTH inside the table."""
    key = (cm.spec.asset, cm.spec.env_id, arm)
    if key in _T1_CACHE:
        return _T1_CACHE[key]
    d = cm.desc
    q0, _, _ = home_state(cm, orc)
    g0, g1 = d.arm_grip_id[arm]
    q0[g0] = q0[g1] = d.jnt_range[g0][0] + 1e-4
    q = _lower_hand(cm, orc, q0, arm, 0.03, inward=0.08)
    mine = [s for s in range(d.nsphere) if sphere_arm(cm)[s] == arm]
    poses = {}

    def count(qq):
        m = int(orc.contact_mask(qq)[0]) >> 20
        return sum(m >> s & 1 for s in mine)
    for _ in range(120):
        q = move_site(cm, orc, q, arm, [0.0, 0.0, -5e-4])
        c = sphere_centres(cm, orc, q)
        depth = max(d.table_z + d.sphere_radius[s] - c[s][2] for s in mine)
        if depth > T1_MAX_DEPTH:
            break
        n = count(q)
        if n and n not in poses:
            poses[n] = q.copy()
            for _ in range(3):                               # up to 0.3 mm deeper while the count holds
                qq = move_site(cm, orc, poses[n], arm, [0.0, 0.0, -1e-4])
                if count(qq) != n:
                    break
                poses[n] = qq
    _T1_CACHE[key] = poses
    return poses


def build_T1(cm, orc, rng):
    """The arm lying on the table: 1 and 2 sphere-table contacts (single arm: both of its KM_SPHERE_TABLE_SLOTS), on the two-arm
    models also 3 to 6 over both arms where the hands reach that many within T1_MAX_DEPTH (table_poses).  The copies cycle through
    the reachable totals; the cube rests out of reach.  Reached: SoloArm 1, 2; DualArm and Torso 1-4 -- a hand's third
    sphere, its palm, is still clear of the table when a finger is 12 mm inside it, so 5 and 6 are not reachable."""
    d = cm.desc
    na = n_arms(cm)
    poses = [table_poses(cm, orc, a) for a in range(na)]
    if na == 1:
        combos = [(n,) for n in sorted(poses[0])]
    else:
        combos = {}
        for a in [0] + sorted(poses[0]):
            for b in [0] + sorted(poses[1]):
                if a + b and (a + b not in combos or abs(a - b) < abs(combos[a + b][0] - combos[a + b][1])):
                    combos[a + b] = (a, b)
        combos = [combos[t] for t in sorted(combos)]
    out = []
    for i in range(max(J_COPIES, len(combos))):
        combo = combos[i % len(combos)]
        q, _, _ = home_state(cm, orc)
        for a, n in enumerate(combo):
            if n:
                ids = arm_joints(cm, a) + list(d.arm_grip_id[a])
                q[ids] = poses[a][n][ids]
        out.append((q, jitter_qvel(cm, rng, cube_free=True)[0], _ctrl_of(cm, q)))
    return _stack(out)


def build_T1G2(cm, orc, rng):
    """T1 together with G2, once: the hand is lowered as in G2 and then on until one of its spheres is on the table, and grasps the
    cube resting on 4 corners there -- contact rows of the arm against the table, of the cube against the table and the coupling
    in one problem."""
    d = cm.desc
    nl = cm.nlink
    q0, _, _ = home_state(cm, orc)
    q = _lower_hand(cm, orc, q0, 0, d.cube_half[2], inward=0.08)
    q = grasp(cm, orc, q, 0, rng, pen=0.002, angle=0.0)      # (the finger slides first: they move the finger spheres)
    q = move_site(cm, orc, q, 0, [0.0, 0.0, -1.0], until=lambda qq: int(orc.contact_mask(qq)[0]) >> 20 != 0, step=5e-4)
    q = move_site(cm, orc, q, 0, [0.0, 0.0, -3e-4])
    q = grasp(cm, orc, q, 0, rng, pen=0.002, angle=0.0)
    c = sphere_centres(cm, orc, q)
    ax = c[1] - c[0]
    yaw = np.arctan2(ax[1], ax[0])
    q[nl + 2] = d.table_z + d.cube_half[2] - 2e-4
    q[nl + 3:nl + 7] = [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]
    return _stack([(q, jitter_qvel(cm, rng)[0], _ctrl_of(cm, q))])


def build_X1(cm, orc, rng):
    """One env with G1 + L1(3) + T1 at once, on the two-arm models: arm 0 holds the cube in the air (G1); arm 1 lies on the table
    (table_poses, its largest count) with three of its joints beyond their ranges and moving out -- its two finger slides past
    their open end and its last hand joint, a leaf link that carries no collider, so the pose on the table is not disturbed.
    None for the single arm: its only joint that moves no collider is joint 7, and any other joint put beyond its range moves the
    hand away from the cube or the table, which Oracle.ik (it clips to the ranges) cannot restore."""
    if n_arms(cm) < 2:
        return None
    d = cm.desc
    nl = cm.nlink
    poses = table_poses(cm, orc, 1)
    q, _, _ = home_state(cm, orc)
    ids = arm_joints(cm, 1) + list(d.arm_grip_id[1])
    q[ids] = poses[max(poses)][ids]
    c = sphere_centres(cm, orc, q)
    if 0.5 * (c[0] + c[1])[2] - d.table_z < 0.07:
        q = _lower_hand(cm, orc, q, 0, 0.08)
    q = grasp(cm, orc, q, 0, rng, pen=0.002)
    v = jitter_qvel(cm, rng)[0]
    lo, hi = blocks(cm)[1]
    leaf = [j for j in range(lo, hi) if j not in ids and all(d.link_parent[k] != j for k in range(nl))
            and all(d.sphere_link[s] != j for s in range(d.nsphere))]
    assert leaf, "no collider-free leaf joint in arm 1's block"
    for j in list(d.arm_grip_id[1]) + leaf[:1]:
        q[j] = d.jnt_range[j][1] - 1e-9                      # at the open end: _push_beyond then takes the upper side
    _push_beyond(cm, orc, q, v, list(d.arm_grip_id[1]) + leaf[:1], rng)
    return _stack([(q, v, _ctrl_of(cm, q))])


BUILDERS = {"G1": build_G1, "G2": build_G2, "G3": build_G3, "P1": build_P1, "P2": build_P2, "P3": build_P3, "C1": build_C1,
            "C2": build_C2, "L1": build_L1, "F1": build_F1, "T1": build_T1, "T1G2": build_T1G2, "X1": build_X1}


# ---------------------------------------------------------------------------------------------------------- cell membership
def _one_arm_holds(r, n=2):
    return [a for a in range(len(r["finger_cube"])) if r["finger_cube"][a] == n and sum(r["finger_cube"]) == n]


IN_CELL = {
    "G1": lambda r: bool(_one_arm_holds(r)) and r["corners"] == 0 and r["cube_clear"] and r["squeeze"][_one_arm_holds(r)[0]] > 0,
    "G2": lambda r: bool(_one_arm_holds(r)) and r["corners"] == 4,
    "G3": lambda r: bool(_one_arm_holds(r, 1)) and r["sphere_cube"] == 1 and r["corners"] == 4,
    "P1": lambda r: r["finger_cube"] == [1, 1],
    "P2": lambda r: len(r["finger_cube"]) == 2 and min(r["finger_cube"]) >= 1 and sum(r["finger_cube"]) >= 3,
    "C1": lambda r: r["corners_bin"] == "1-3" and not r["coupled"] and r["cube_spin"] > 1.0,
    "C2": lambda r: r["corners"] == 0 and not r["coupled"] and r["cube_low"] < 5e-3 and r["cube_speed"] > 2.5 and r["cube_spin"] > 25.0,
    "L1": lambda r: max(r["limits"]) >= 1 and r["limits_outward"] and not r["coupled"] and r["n_sphere_table"] == 0,
    "F1": lambda r: len(r["saturated"]) >= 1,
    "T1": lambda r: r["n_sphere_table"] >= 1 and not r["coupled"],
    "T1G2": lambda r: bool(_one_arm_holds(r)) and r["corners"] == 4 and r["n_sphere_table"] >= 1,
    "X1": lambda r: len(r["finger_cube"]) == 2 and r["finger_cube"] == [2, 0] and r["cube_clear"] and r["limits"][1] == 3
    and r["limits_outward"] and r["sphere_table"][1] >= 1,
}
# what a G / P copy must still show after a control step to count as retained: the cell's sphere-cube contacts
RETAINED = {
    "G1": lambda r: bool(_one_arm_holds(r)), "G2": lambda r: bool(_one_arm_holds(r)), "T1G2": lambda r: bool(_one_arm_holds(r)),
    "G3": lambda r: bool(_one_arm_holds(r, 1)), "P1": IN_CELL["P1"], "P2": IN_CELL["P2"],
}
UNREACHABLE = {"solo_arm": ("P1", "P2", "P3", "X1"), "dual_arm": ("P3",), "torso": ("P3",)}


def all_cells(cm, orc, seed=0):
    """Every reachable cell's copies in one batch, cell-major: (qpos, qvel, ctrl, labels) with labels[e] the cell of env e."""
    rng = np.random.default_rng(seed)
    parts, labels = [], []
    for cell, build in BUILDERS.items():
        st = build(cm, orc, rng)
        if st is None:
            assert cell in UNREACHABLE[cm.spec.asset], (cell, cm.spec.asset)
            continue
        parts.append(st)
        labels += [cell] * len(st[0])
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3)) + (labels,)


def model(asset, solver="newton"):
    """The asset in the joint-delta action mode (mujoco_pin.qpos_spec), no auto-reset."""
    import mujoco_pin
    from gym_kmanip_amd.model import compile_model
    return compile_model(mujoco_pin.qpos_spec(asset), auto_reset=False, solver=solver)


_CELLS = {}


def cells(asset):
    """all_cells of the asset, built once (the builders read geometry only: the same states serve both solvers)."""
    from oracle.oracle import Oracle
    if asset not in _CELLS:
        cm = model(asset)
        _CELLS[asset] = all_cells(cm, Oracle(cm, 1), seed=0)
    return _CELLS[asset]


def loaded_oracle(cm, qpos, qvel, ctrl):
    """A batched oracle set to the states, warm start from Oracle.after_reset, step 0."""
    from oracle.oracle import Oracle
    n = len(qpos)
    orc = Oracle(cm, n)
    orc.set_state(qpos, qvel, ctrl, warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl), np.zeros(n, dtype=np.int32))
    return orc


def warm_start(cm, orc, qpos, qvel, ctrl):
    """qacc_warmstart of every env as Oracle.after_reset gives it (mj_forward with actuation disabled)."""
    return np.stack([orc.after_reset(qpos[e], qvel[e], ctrl[e]) for e in range(len(qpos))])


# ------------------------------------------------------------------------------------------------------------------- census
CENSUS_CELLS = ("G1", "G2", "G3", "P1", "P2", "C1", "C2", "L1(3+)", "F1", "T1(2+)", "T1G2", "X1")
_CENSUS_TEST = dict(IN_CELL)
# L1 and T1 are counted at the depth the builders add: three or more joints of one block beyond their range (the Woodbury
# boundary; the Torso's home pose alone has one and two), two or more spheres on the table
_CENSUS_TEST["L1(3+)"] = lambda r: max(r["limits"]) >= 3
_CENSUS_TEST["T1(2+)"] = lambda r: r["n_sphere_table"] >= 2 and not r["coupled"]


def census(cm, n=256, steps=66, seed=2, off=5, check=None, nthreads=4):
    """The random-rollout recipe of the step matrix (test_kernel_paths_gpu._step_parity: reset, actions uniform in [-1, 1) from
    default_rng(seed), auto-reset at step 64; the states compared are those BEFORE step k for k % 9 == 8, k = 63 and the last
    step, of the envs in `check`) run on the oracle; returns ({cell: number of compared states in it}, number compared)."""
    from oracle.oracle import Oracle
    check = list(range(0, n, 5)) if check is None else check
    orc = Oracle(cm, n, seed=seed, env_id_offset=off)
    one = Oracle(cm, 1)
    orc.reset()
    rng = np.random.default_rng(seed)
    counts = {c: 0 for c in CENSUS_CELLS}
    total = 0
    for k in range(steps):
        act = rng.uniform(-1, 1, (n, cm.act_dim)).astype(np.float32)
        if k % 9 == 8 or k in (63, steps - 1):
            qpos, qvel, ctrl = orc.get_state()[:3]
            for e in check:
                r = regime(cm, one, qpos[e], qvel[e], ctrl[e])
                total += 1
                for c in CENSUS_CELLS:
                    counts[c] += bool(_CENSUS_TEST[c](r))
        orc.step(act, nthreads)
    return counts, total


# --------------------------------------------------------------------------------------------- the Coulomb check of the grasp
HOLD_SQUEEZE = 0.01          # metres each finger servo is commanded past the cube's face
HOLD_STEPS = 32


def hold_spec(asset):
    """The asset's joint-delta spec WITHOUT the grip keys: before_step then leaves the finger servos' ctrl alone, so a squeeze
    written into the state persists (with the keys it is renewed from qpos at every control step; module docstring)."""
    import dataclasses
    import mujoco_pin
    s = mujoco_pin.qpos_spec(asset)
    return dataclasses.replace(s, env_id=s.env_id + "-nogrip", act_list=[k for k in s.act_list if not k.startswith("grip")])


def hold_action(cm, qpos, target):
    """The joint-delta action that renews every arm servo's target as `target` (before_step: ctrl = float32(q + 0.1 a)): without it
    a zero action re-targets each servo at the joint's current position and the arm sinks under its own weight."""
    act = np.zeros((len(qpos), cm.act_dim), dtype=np.float32)
    for key, ids in (("q_pos_r", cm.spec.q_id_r_mask), ("q_pos_l", cm.spec.q_id_l_mask)):
        if key in cm.act_slices:
            act[:, cm.act_slices[key]] = np.clip((target[ids] - qpos[:, ids]) / cm.desc.q_pos_delta, -1.0, 1.0)
    return act


def held_cube(asset, solver="newton"):
    """The cube held at rest in a G1 grasp, for the Coulomb check.  Arm 0's hand 8 cm over the table, the cube between its fingers
    (2 mm inside each), both finger servos commanded HOLD_SQUEEZE past that (hold_spec keeps the command).  The state is then
    settled on the oracle with a friction of 2 and every servo aimed at the built pose: 1200 times three sub-steps with every
    velocity zeroed after them, which ends in the static equilibrium (|qacc| < 0.1; the servos have no damping: the arm would
    swing for seconds otherwise, and zeroing once per control step can fall in step with that swing).  N is taken as the
    mean of the two finger servos' forces kp (q - ctrl) there: 1.20 N on the Torso (kp 100), 2.40 N on the SoloArm and the DualArm
    (kp 200).  The SoloArm's and the DualArm's slides also have 30 N of friction loss, which could carry part of the load; at
    this equilibrium it carries none: the normal force of each finger's contact in the oracle's own constraint rows (the sum of
    its six pyramid-edge forces, -(J qacc - aref) / R) is 2.34 / 2.46 N there and 1.19 / 1.21 N on the Torso, and held_cube asserts
    that both lie within 10 % of N.  Returns (cm, (qpos, qvel, ctrl, warm), target, N)."""
    import mujoco_pin
    from gym_kmanip_amd.model import compile_model, with_env_params
    from oracle.oracle import Oracle
    cmg = compile_model(mujoco_pin.qpos_spec(asset), auto_reset=False, solver=solver)
    og = Oracle(cmg, 1)
    cm = compile_model(hold_spec(asset), auto_reset=False, solver=solver)
    d = cmg.desc
    nl = cm.nlink
    g0, g1 = d.arm_grip_id[0]
    q, _, _ = home_state(cmg, og)
    q = _lower_hand(cmg, og, q, 0, 0.08)
    q = grasp(cmg, og, q, 0, None, pen=0.002, angle=0.0, squeeze=0.0)
    ctrl = f32(q[:nl])
    for g in (g0, g1):
        ctrl[g] = f32(max(q[g] - HOLD_SQUEEZE, d.jnt_range[g][0]))
    target = q[:nl].copy()
    orc = Oracle(with_env_params(cm, cube_friction=2.0), 1)
    ctrl[:nl] = np.where(np.isin(np.arange(nl), (g0, g1)), ctrl, f32(target))
    qq, warm = q.copy(), orc.after_reset(q, np.zeros(cm.nv), ctrl)
    for _ in range(1200):                                    # 3 sub-steps, then every velocity zeroed: a damped descent to rest
        qq, _, warm, bad, _, _, _ = orc.physics_step(qq, np.zeros(cm.nv), ctrl, warm, qq, 3)
        assert not bad
    acc = orc.dynamics(qq, np.zeros(cm.nv), ctrl)["qacc"]
    assert np.abs(acc).max() < 0.1, np.abs(acc).max()        # at rest: what is left would move nothing by 1e-5 m in 32 steps
    qpos, qvel, ctrl, warm = qq[None], np.zeros((1, cm.nv)), ctrl[None], warm[None]
    assert int(orc.contact_mask(qpos[0])[0]) == 0x300
    N = 0.5 * sum(d.kp[g] * (qpos[0, g] - ctrl[0, g]) for g in (g0, g1))
    dyn = orc.dynamics(qpos[0], qvel[0], ctrl[0])
    t, _ = orc.constraint_rows(qpos[0], qvel[0])
    first = int((t == 0).sum()) + sum(qpos[0, j] < d.jnt_range[j][0] or qpos[0, j] > d.jnt_range[j][1] for j in range(nl))
    f = np.maximum(0.0, -(dyn["J"] @ dyn["qacc"] - dyn["aref"]) / dyn["R"])[first:]      # the two sphere-cube contacts: 6 edges each
    assert len(f) == 12 and abs(f[:6].sum() - N) < 0.1 * N and abs(f[6:].sum() - N) < 0.1 * N, (N, f[:6].sum(), f[6:].sum())
    return cm, (qpos, qvel, ctrl, warm), target, float(N)


def coulomb_frictions(cm, N):
    """(hold, slip): twice and half the Coulomb threshold m g / (2 N) of a cube held between two fingers pressing with N each."""
    thr = cm.desc.cube_mass * abs(cm.desc.gravity[2]) / (2.0 * N)
    return 2.0 * thr, 0.5 * thr
