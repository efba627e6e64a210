"""States that reach every branch of the collision narrow phase, built WITHOUT IK: the arm stays at regime_states._in_range_home
(or a seeded in-range pose) and the free cube is placed at the arm's colliders.  (One state per two-arm asset is the exception:
"overflow" takes its arm pose from regime_states.both_hands_on_cube.)

A sphere collider gets the box put around it: a point of the box frame is chosen for the collider centre -- over a face, an edge or
a vertex of the box (outside, 0.1 .. 4 mm of penetration) or 1 .. 3 mm inside under a chosen face -- together with a seeded
direction; the cube pose follows.  For a capsule collider the cube CENTRE is chosen first, at the wanted segment parameter t (below
0, interior, above 1) plus an offset across the segment, then a rotation that carries the wanted box-frame point onto that offset.
Every placement is checked with contact_reference.geometry (the wanted collider, region and feature, and the branch margins) and
redrawn until it fits: the margins hold by construction, no state is left out.  Plane states put more than four corners under the
table, a cube across each table_rect bound, and -- on models with a raised table (contact_model.with_contact) -- more spheres under the
table than there are slots and a rectangle bound between two penetrating spheres."""
import numpy as np

import contact_model as CM
import contact_reference as CR
import regime_states as R

MARGIN = dict(loc=1e-4, faces=1e-4, ny=0.05, t=1e-3, rect=1e-4, dist=1e-5)
PEN = (1e-4, 4e-3)              # outside penetrations, metres
DEPTH = (1e-3, 3e-3)            # inside states: the centre this far under the nearest face
N_POSES = 3                     # arm poses: _in_range_home and two seeded in-range ones


def margins_ok(info):
    return all(info["margin"][k] >= v for k, v in MARGIN.items())


def arm_poses(cm, orc, seed=0):
    """[qpos]: _in_range_home, then seeded poses with every hinge within 0.25 rad (slides 3 mm) of it, kept 1 % inside the range."""
    d = cm.desc
    nl = cm.nlink
    q0, _, _ = R._in_range_home(cm, orc)
    rng = np.random.default_rng(seed)
    out = [q0]
    for _ in range(N_POSES - 1):
        q = q0.copy()
        for j in range(nl):
            lo, hi = d.jnt_range[j]
            q[j] += rng.uniform(-0.25, 0.25) * (0.012 if d.jnt_type[j] == 1 else 1.0)
            q[j] = min(max(q[j], lo + 0.01 * (hi - lo)), hi - 0.01 * (hi - lo))
        out.append(q)
    return out


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def wanted_loc(half, rad, region, fixed, rng, odd=False):
    """A point of the box frame for the collider centre.  fixed = {axis: sign} of the feature (one entry: face, two: edge, three:
    vertex).  odd (inside only): the nearest face is not the axis of largest |loc|."""
    loc = np.zeros(3)
    free = [a for a in range(3) if a not in fixed]
    if region == "inside":
        (a, s), = fixed.items()
        depth = rng.uniform(*DEPTH)
        loc[a] = s * (half[a] - depth)
        for b in free:
            room = half[b] - depth - 2e-3
            loc[b] = rng.uniform(-room, room)
        if odd:
            b = max(free, key=lambda x: half[x])
            lo, hi = abs(loc[a]) + 5e-4, half[b] - depth - 2e-3
            assert lo < hi, "no such point: the face's own axis is the longest"
            loc[b] = rng.choice([-1.0, 1.0]) * rng.uniform(lo, hi)
        return loc
    pen = rng.uniform(*PEN)
    u = np.zeros(3)
    w = rng.uniform(0.3, 1.0, 3)
    for a, s in fixed.items():
        u[a] = s * w[a]
        loc[a] = s * half[a]
    loc += (rad - pen) * _unit(u)
    for b in free:
        loc[b] = rng.uniform(-0.8, 0.8) * (half[b] - 1e-3)
    return loc


def place(cm, orc, q_arm, s, loc, rng, t_want=None, normal=None):
    """qpos with the cube posed so that collider s's centre sits at `loc` of the box frame.  Plain sphere: along a seeded direction
    (or so that the contact normal of a face-centre point is `normal`).  Capsule: the cube centre at segment parameter t_want
    (< 0, in (0, 1), > 1) plus an offset across the segment."""
    d = cm.desc
    nl = cm.nlink
    pos, mat = CR.body_poses(cm, orc, q_arm)
    l = d.sphere_link[s]
    p0 = pos[l] + mat[l] @ np.array(d.sphere_pos[s])
    seg = mat[l] @ np.array(d.sphere_seg[s])
    L = np.linalg.norm(loc)
    if seg @ seg > 0:
        along = 0.0 if 0 < t_want < 1 else (t_want if t_want < 0 else t_want - 1.0) * np.linalg.norm(seg)   # signed, metres, beyond the end
        assert abs(along) < L
        e = _unit(seg)
        x = np.cross(e, _unit(rng.normal(size=3)))
        off = np.sqrt(L * L - along * along) * _unit(x)
        ctr = p0 + min(max(t_want, 0.0), 1.0) * seg
        cpos = ctr + along * e + off
        w = ctr - cpos
    else:
        # a face-centre point has the contact normal -cmat loc / L: w = cmat loc = -L normal
        w = L * (_unit(rng.normal(size=3)) if normal is None else -_unit(normal))
        cpos = p0 - w
    Rm = R.frame_along(w, rng.uniform(0, 2 * np.pi)) @ R.frame_along(loc, 0.0).T            # carries loc onto w
    q = q_arm.copy()
    q[nl:nl + 3] = cpos
    q[nl + 3:nl + 7] = R.mat2quat(Rm)
    return q


def _sphere_state(cm, orc, poses, s, region, fixed, rng, t_want=None, odd=False, normal=None, pose=None):
    """One checked placement (redrawn until the reference sees the wanted contact with the margins kept)."""
    d = cm.desc
    half = np.array(d.cube_half)
    want_kind = "inside" if region == "inside" else ("face", "edge", "vertex")[len(fixed) - 1]
    for attempt in range(400):
        q_arm = poses[(attempt if pose is None else pose) % len(poses)]
        loc = wanted_loc(half, d.sphere_radius[s], region, fixed, rng, odd)
        if normal is not None:
            loc[[a for a in range(3) if a not in fixed]] = 0.0
        q = place(cm, orc, q_arm, s, loc, rng, t_want, normal)
        g = CR.geometry(cm, orc, q)
        c = [c for c in g["contacts"] if c["bit"] == 8 + s]
        if not c or not margins_ok(g["info"]):
            continue
        c = c[0]
        if c["region"] != want_kind or not all((c["loc"][a] > 0) == (sg > 0) for a, sg in fixed.items()):
            continue
        if np.abs(c["loc"] - loc).max() > 1e-9:
            continue
        return q
    raise AssertionError(("no placement", s, region, fixed, t_want))


def _features():
    """[(region, fixed)] of the 6 faces, 12 edges, 8 vertices and 6 inside faces."""
    out = [("face" if kind == "face" else kind, fixed) for kind, _, fixed in CR.box_features(np.ones(3))]
    return out + [("inside", fixed) for kind, _, fixed in CR.box_features(np.ones(3)) if kind == "face"]


def _corner_states(cm, orc, q_arm, rng):
    """5, 6, 7 and 8 corners under the table (the slots keep the first four), the cube clear of the arm, and a cube lying across each
    of the four table_rect bounds with corners under the table on both sides."""
    d = cm.desc
    nl = cm.nlink
    half = np.array(d.cube_half)
    rect = list(d.table_rect)
    signs = np.array([[(1 if i & 1 else -1), (1 if i & 2 else -1), (1 if i & 4 else -1)] for i in range(8)])
    out, labels = [], []
    spot = np.array([rect[1] - 0.1, rect[3] - 0.1])
    for k in (5, 6, 7, 8):
        for attempt in range(400):
            Rm = R._rot(_unit(rng.normal(size=3)), rng.uniform(0.1, 0.5)) @ R._rot([0, 0, 1.0], rng.uniform(0, 2 * np.pi))
            o = np.sort((signs * half) @ Rm[2])
            if k < 8 and o[k] - o[k - 1] < 4e-4:
                continue
            zs = (signs * half) @ Rm[2]
            under = [i for i in range(8) if zs[i] <= o[k - 1]]
            if sorted(under[:4]) == sorted(sorted(under, key=lambda i: zs[i])[:4]):
                continue                                    # the first four by index must not be the four deepest: the rule has to show
            z = d.table_z - (0.5 * (o[k - 1] + o[k]) if k < 8 else o[7] + 1e-3)
            q = q_arm.copy()
            q[nl:nl + 3] = [spot[0], spot[1], z]
            q[nl + 3:nl + 7] = R.mat2quat(Rm)
            g = CR.geometry(cm, orc, q)
            if g["info"]["n_corners"] == k and g["mask"] < 256 and margins_ok(g["info"]):
                out.append(q); labels.append("corners%d" % k)
                break
        else:
            raise AssertionError(("no corner state", k))
    mid_x, mid_y = 0.0, 0.5 * (rect[2] + rect[3]) + 0.1
    for name, xy in (("x_lo", (rect[0], mid_y)), ("x_hi", (rect[1], mid_y)), ("y_lo", (mid_x, rect[2])), ("y_hi", (mid_x, rect[3]))):
        for attempt in range(400):
            Rm = R._rot([0, 0, 1.0], rng.uniform(0.1, 1.4)) @ R._rot(_unit(rng.normal(size=3)), rng.uniform(0.0, 0.01))
            q = q_arm.copy()
            q[nl:nl + 3] = [xy[0] + rng.uniform(-3e-3, 3e-3), xy[1] + rng.uniform(-3e-3, 3e-3), d.table_z + half[2] - 1e-3]
            q[nl + 3:nl + 7] = R.mat2quat(Rm)
            g = CR.geometry(cm, orc, q)
            below = [(signs[i] * half) @ Rm[2] + q[nl + 2] < d.table_z for i in range(8)]
            if sum(below) == 4 and 0 < g["info"]["n_corners"] < 4 and g["mask"] < 256 and margins_ok(g["info"]):
                out.append(q); labels.append("rect_" + name)
                break
        else:
            raise AssertionError(("no rectangle state", name))
    return out, labels


def overflow_search(cm, orc, poses, rng, budget=3000):
    """One more penetrating sphere than KM_SPHERE_SLOTS on the shipped sphere list: the long box reaches the palm and both fingers
    of a hand.  A seeded hill climb over the cube pose and the finger slides (kept inside their ranges), from each of `poses`.
    It maximises the (slots + 1)-th largest penetration while the largest stays near 3 mm and the kept contacts' frames stay off
    the |n_y| = 0.5 boundary.  Returns (qpos or None, best value); a negative best value is the clearance left, in metres."""
    d = cm.desc
    nl = cm.nlink
    need = CR.sphere_slots(nl) + 1
    half = np.array(d.cube_half)

    def score(q):
        pos, mat = CR.body_poses(cm, orc, q)
        pens, ny = [], []
        for s in range(d.nsphere):
            l = d.sphere_link[s]
            ctr = pos[l] + mat[l] @ np.array(d.sphere_pos[s])
            seg = mat[l] @ np.array(d.sphere_seg[s])
            if seg @ seg > 0:
                ctr = ctr + min(max((pos[nl] - ctr) @ seg / (seg @ seg), 0.0), 1.0) * seg
            loc = mat[nl].T @ (ctr - pos[nl])
            sd, surf, _, _ = CR.closest_on_box(half, loc)
            pens.append(d.sphere_radius[s] - sd)
            if pens[-1] > 0 and len(ny) < CR.sphere_slots(nl):          # a kept contact: how far its frame is from the |n_y| = 0.5 boundary
                n = mat[nl] @ _unit(surf - loc)
                ny.append(abs(abs(n[1]) - 0.5))
        p = np.sort(pens)
        return float(p[-need] - 2.0 * max(0.0, p[-1] - 3e-3) - 0.1 * max(0.0, 2 * MARGIN["ny"] - min(ny, default=1.0)))

    slides = [j for j in range(nl) if d.jnt_type[j] == 1]
    best_q, best = None, -np.inf
    for q_arm in poses:
        c = R.sphere_centres(cm, orc, q_arm)
        q = q_arm.copy()
        q[nl:nl + 3] = (c[0] + c[1] + c[2 * R.n_arms(cm)]) / 3.0
        q[nl + 3:nl + 7] = R.mat2quat(R.frame_along(c[1] - c[0], 0.0))
        cur = score(q)
        step = 0.02
        for it in range(budget // len(poses)):
            cand = q.copy()
            cand[nl:nl + 3] += rng.normal(size=3) * step
            for j in slides:                                # the finger slides may close, inside their range
                lo, hi = d.jnt_range[j]
                cand[j] = min(max(cand[j] + rng.normal() * step, lo + 0.01 * (hi - lo)), hi - 0.01 * (hi - lo))
            Rm = R._rot(_unit(rng.normal(size=3)), rng.normal() * step * 20) @ R.quat2mat(q[nl + 3:nl + 7])
            cand[nl + 3:nl + 7] = R.mat2quat(Rm)
            sc = score(cand)
            if sc > cur:
                q, cur, step = cand, sc, min(1.3 * step, 0.02)
            else:
                step = max(0.97 * step, 2e-4)
        if cur > best:
            best_q, best = q, cur
    if best < 2e-4:
        return None, best
    for attempt in range(300):                              # the climb ends anywhere: nudge it until the branch margins hold
        cand = best_q.copy()
        if attempt:
            cand[nl:nl + 3] += rng.normal(size=3) * 3e-4
            cand[nl + 3:nl + 7] = R.mat2quat(R._rot(_unit(rng.normal(size=3)), rng.normal() * 0.01) @ R.quat2mat(best_q[nl + 3:nl + 7]))
        g = CR.geometry(cm, orc, cand)
        if g["info"]["n_sphere_cube"] >= need and margins_ok(g["info"]):
            return cand, best
    return None, best


T_REGIMES = ((-0.03, "0"), (0.5, "i"), (1.03, "1"))         # segment parameter of the cube centre: clamped to 0, interior, clamped to 1


def _t_plan(capsule, all_three, rng):
    """[(t_want, label)] a planned state is built at: (None, None) for a plain sphere; for a capsule section one seeded draw among
    below 0, two interior values and above 1 -- or, with all_three, one state in each regime."""
    if not capsule:
        return ((None, None),)
    return T_REGIMES if all_three else ((rng.choice([-0.03, 0.3, 0.7, 1.03]), None),)


FRAME_NORMALS = ((0.3, 0.9, 0.3), (0.3, -0.9, 0.3), (0.8, 0.2, 0.56), (0.8, -0.2, 0.56))       # |n_y| >= 0.5 and < 0.5, both signs

_STATES = {}


def states(asset):
    """dict(cm (box), cm0 (box0), qpos, qvel, ctrl, labels, overflow_best) of the asset, built once.  Labels:
    "s<sphere>:<region><feature>[:t<0|i|1|.05>][:odd]", "frame<k>", "corners<k>", "rect_<bound>", "overflow"."""
    from oracle.oracle import Oracle
    if asset in _STATES:
        return _STATES[asset]
    base = R.model(asset)
    cm, cm0 = CM.box(base), CM.box0(base)
    orc = Oracle(cm, 1)
    d = cm.desc
    rng = np.random.default_rng(11)
    poses = arm_poses(cm, orc)
    qs, labels = [], []
    feats = _features()
    ids = {(kind, tuple(sorted(fixed.items()))): fid for kind, fid, fixed in CR.box_features(np.ones(3))}
    # every feature of the box and every inside face, the colliders taken in turn; then every collider in every region class
    plan = [(s % d.nsphere, region, fixed) for s, (region, fixed) in enumerate(feats)]
    seen = {(s, region) for s, region, _ in plan}
    for s in range(d.nsphere):
        for k, region in enumerate(("face", "edge", "vertex", "inside")):
            if (s, region) not in seen:
                cands = [f for f in feats if f[0] == region]
                plan.append((s, region, cands[(3 * s + k) % len(cands)][1]))
    for s, region, fixed in plan:
        capsule = any(x != 0 for x in d.sphere_seg[s])
        fid = ids[("face" if region == "inside" else region, tuple(sorted(fixed.items())))]
        for tw, tl in _t_plan(capsule, region == "face" and len(labels) % 2 == 0, rng):
            q = _sphere_state(cm, orc, poses, s, region, fixed, rng, t_want=tw)
            qs.append(q)
            labels.append("s%d:%s%d" % (s, region, fid) + (":t" + tl if tl else ""))
    # capsule colliders at t clamped to 0, interior and clamped to 1 (whatever the plan above drew)
    for s in range(d.nsphere):
        if any(x != 0 for x in d.sphere_seg[s]):
            for tw, tl in T_REGIMES:
                fixed = feats[(s + int(tw * 10)) % 26][1]
                region = ("face", "edge", "vertex")[len(fixed) - 1]
                qs.append(_sphere_state(cm, orc, poses, s, region, fixed, rng, t_want=tw))
                labels.append("s%d:%s%d:t%s" % (s, region, ids[(region, tuple(sorted(fixed.items())))], tl))
    # inside, the nearest face not the axis of largest |loc|: y and z (impossible for x, the longest axis: |loc_x| > 0.027 there)
    for a in (1, 2):
        for sg in (-1, 1):
            qs.append(_sphere_state(cm, orc, poses, (a + (sg > 0)) % d.nsphere, "inside", {a: sg}, rng, odd=True,
                                    t_want=0.5 if any(x != 0 for x in d.sphere_seg[(a + (sg > 0)) % d.nsphere]) else None))
            labels.append("s%d:inside%d:odd" % ((a + (sg > 0)) % d.nsphere, 2 * a + (sg > 0)))
    # the frame's two branches, both signs of n_y: a finger sphere over a face centre with a chosen normal
    for k, n in enumerate(FRAME_NORMALS):
        qs.append(_sphere_state(cm, orc, poses, 0, "face", {k % 3: 1 if k < 2 else -1}, rng, normal=n, pose=0))
        labels.append("frame%d" % k)
    q2, l2 = _corner_states(cm, orc, poses[0], rng)
    qs += q2; labels += l2
    # one sphere more on the box than slots.  One hand does it on the single arm.  The two-arm models need four fingers and a palm:
    # the arm pose is regime_states.both_hands_on_cube's (cell P2; the one pose here that an IK built), the cube is placed by the search
    if cm.nlink == 20:
        over_poses = [R.both_hands_on_cube(base, Oracle(base, 1), 0.002, 0.0)]
        assert over_poses[0] is not None
    else:
        over_poses = poses
    qo, best = overflow_search(cm, orc, over_poses, np.random.default_rng(5))
    if qo is not None:
        qs.append(qo); labels.append("overflow")
    # every capsule section once more at a small interior t, over the box's largest face: the collider sits 6 mm from the segment's
    # start, so a collider wrongly left AT the start (t = 0) still touches the box, elsewhere -- the wrong t shows inside a contact
    rng_t = np.random.default_rng(14)
    for s in range(d.nsphere):
        if any(x != 0 for x in d.sphere_seg[s]):
            qs.append(_sphere_state(cm, orc, poses, s, "face", {2: 1 if s % 2 else -1}, rng_t, t_want=0.05))
            labels.append("s%d:face%d:t.05" % (s, 4 + s % 2))
    qpos = np.stack(qs)
    qvel = R.jitter_qvel(cm, np.random.default_rng(12), len(qs))
    ctrl = np.stack([R._ctrl_of(cm, q) for q in qs])
    _STATES[asset] = dict(cm=cm, cm0=cm0, qpos=qpos, qvel=qvel, ctrl=ctrl, labels=labels, overflow_best=best)
    return _STATES[asset]


_TABLE = {}


def table_states(asset):
    """[(name, cm, qpos[1, nq], qvel, ctrl)] on box models with a RAISED table (with_contact(table_z=..., table_rect=...)), the arm
    resting at _in_range_home and the cube in free fall 0.3 m above:
      table_overflow   one more sphere under the table than KM_SPHERE_TABLE_SLOTS
      table_rect       a rectangle bound passing between the two lowest penetrating spheres"""
    from oracle.oracle import Oracle
    if asset in _TABLE:
        return _TABLE[asset]
    base = CM.box(R.model(asset))
    d = base.desc
    nl = base.nlink
    orc = Oracle(base, 1)
    q0, v0, c0 = R._in_range_home(base, orc)
    if nl == 20 and asset == "dual_arm":                    # two mirrored arms rest with their spheres pairwise at one height: turn one arm's
        q0[11] += 0.02; q0[13] -= 0.03                      # shoulder and elbow a little, inside their ranges, so the order is strict
        c0 = R._ctrl_of(base, q0)
    ctr = R.sphere_centres(base, orc, q0)
    low = ctr[:, 2] - np.array(d.sphere_radius[:d.nsphere])
    order = np.argsort(low)
    out = []

    def raised(k):
        """table_z with exactly k sphere bottoms under it, midway between the k-th and the next."""
        assert low[order[k]] - low[order[k - 1]] > 4e-4, (k, low[order])
        return 0.5 * (low[order[k - 1]] + low[order[k]])

    def state(cm):
        q = q0.copy()
        q[nl:nl + 3] = [0.0, 0.5 * (cm.desc.table_rect[2] + cm.desc.table_rect[3]), cm.desc.table_z + 0.3]
        return q[None], R.jitter_qvel(cm, np.random.default_rng(13), 1), c0[None]

    k = CR.sphere_table_slots(nl) + 1
    cm = CM.with_contact(base, table_z=raised(k), table_rect=(-10.0, 10.0, -10.0, 10.0))
    out.append(("table_overflow", cm) + state(cm))
    a, b = order[0], order[1]
    axis = int(np.argmax(np.abs(ctr[a, :2] - ctr[b, :2])))
    bound = 0.5 * (ctr[a, axis] + ctr[b, axis])
    rect = [-10.0, 10.0, -10.0, 10.0]
    rect[2 * axis + (1 if ctr[a, axis] < bound else 0)] = bound                  # sphere a stays over the table, b falls beside it
    cm = CM.with_contact(base, table_z=raised(2), table_rect=rect)
    out.append(("table_rect", cm) + state(cm))
    _TABLE[asset] = out
    return out


# ------------------------------------------------------------------------------------------------- soft-constraint constants
MJ_MINVAL = 1e-15
# name -> (solref entries, solimp entries) replaced in BOTH parameter sets (the cube pairs' and the default set's).
# solref = (time constant, damping ratio); solimp = (d0, dw, width, mid, power)
SOFT_VARIANTS = {
    "power1": ({}, {4: 1.0}),
    "mid0.2": ({}, {3: 0.2, 4: 2.0}),
    "mid0.8": ({}, {3: 0.8, 4: 2.0}),
    "d0>dw": ({}, {0: 0.95, 1: 0.9}),
    "d0==dw": ({}, {0: 0.9, 1: 0.9}),
    "width_min": ({}, {2: MJ_MINVAL}),
    "timeconst0.003": ({0: 0.003}, {}),                     # below 2 dt = 0.004: the clamp fires
    "dampratio0.5": ({1: 0.5}, {}),
    "dampratio2": ({1: 2.0}, {}),
}
WIDTHS = (0.2, 0.7, 1.3)        # penetrations / limit violations, in widths of the impedance curve


def soft_model(cm, name):
    """cm with variant `name` of the soft-constraint constants, through contact_model.with_contact."""
    d = cm.desc
    ref_mod, imp_mod = SOFT_VARIANTS[name]
    sets = {}
    for which in ("cube", "def"):
        sr, si = list(getattr(d, "con_%s_solref" % which)), list(getattr(d, "con_%s_solimp" % which))
        for k, v in ref_mod.items():
            sr[k] = v
        for k, v in imp_mod.items():
            si[k] = v
        sets[which + "_solref"], sets[which + "_solimp"] = sr, si
    return CM.with_contact(cm, **sets)


_SOFT = {}


def soft_states(asset):
    """(box model, qpos[6], qvel[6], ctrl[6], labels): a finger sphere 0.2, 0.7 and 1.3 widths deep in a face of the box, and one
    joint 0.2, 0.7 and 1.3 widths beyond its range, the widths being the SHIPPED ones (cube pairs 5.5 mm, default set 1 mm or mrad);
    the states serve every variant (width_min, whose own width is 1e-15, is then beyond one width everywhere)."""
    from oracle.oracle import Oracle
    if asset in _SOFT:
        return _SOFT[asset]
    cm = CM.box(R.model(asset))
    d = cm.desc
    nl = cm.nlink
    orc = Oracle(cm, 1)
    rng = np.random.default_rng(21)
    half = np.array(d.cube_half)
    q0, _, _ = R._in_range_home(cm, orc)
    qs, labels = [], []
    for k in WIDTHS:
        pen = k * d.con_cube_solimp[2]
        for attempt in range(200):
            loc = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.008, 0.008), half[2] + d.sphere_radius[0] - pen])
            q = place(cm, orc, q0, 0, loc, rng)
            g = CR.geometry(cm, orc, q)
            if g["mask"] == 1 << 8 and abs(g["contacts"][0]["dist"] + pen) < 1e-12 and margins_ok(g["info"]):
                break
        else:
            raise AssertionError(("no soft contact state", k))
        qs.append(q); labels.append("contact%.1f" % k)
    j = R._limit_candidates(cm, orc, 0)[0]
    lo, hi = d.jnt_range[j]
    for k in WIDTHS:
        q = q0.copy()
        over = k * d.con_def_solimp[2]
        q[j] = hi + over if abs(hi - q0[j]) <= abs(q0[j] - lo) else lo - over
        assert not int(orc.contact_mask(q)[0]) & 0xFFFFFF00
        qs.append(q); labels.append("limit%.1f" % k)
    qpos = np.stack(qs)
    qvel = R.jitter_qvel(cm, np.random.default_rng(22), len(qs))
    ctrl = np.stack([R._ctrl_of(cm, q) for q in qs])
    _SOFT[asset] = (cm, qpos, qvel, ctrl, labels, j)
    return _SOFT[asset]
