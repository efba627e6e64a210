"""Contact geometry and contact rows of a state from definitions, in NumPy float64: a reference that shares nothing with the
oracle's collide, its body_jac or force_oracle.contact_geometry.  The only thing taken from the C oracle is Oracle.fk (link origins
and quaternions), which the fk_* fixtures pin.

GEOMETRY
  sphere against box   the closest point of the box SURFACE to the collider centre, found by enumerating the 6 faces, 12 edges and 8
                       vertices as point-to-feature projections (a projection counts where it falls on its feature); a centre inside
                       the box: the nearest face.  dist = signed distance - radius.  The normal points from the sphere into the box
                       (checked here against minus the central-difference gradient of the signed distance).  The contact point is the
                       midpoint of the deepest points of the two surfaces.
  capsule collider     the sphere at the point of the link's segment closest to the cube CENTRE (the rule of include/kmanip.h).
  frame                orthonormal, right-handed, row 0 the normal; row 1 the normalised projection of +y, or of +z where
                       |n_y| >= 0.5 (MuJoCo's mju_makeFrame convention, as a definition).
  plane pairs          a cube corner / a sphere's lowest point below table_z with its x, y inside table_rect; kept: the first four
                       penetrating corners in corner-index order, the first KM_SPHERE_SLOTS / KM_SPHERE_TABLE_SLOTS spheres in
                       sphere order.
ROWS
  The 3 x nv translational Jacobian of a world point fixed in a body comes from central differences of Oracle.fk at the steps H and
  H / 2, Richardson-extrapolated, (4 D(H/2) - D(H)) / 3; |D(H) - D(H/2)| is the reference's own error estimate (it overstates the
  error of the extrapolated value, as in lagrange_oracle).  The cube's three angular dofs are perturbed by RIGHT-multiplying its
  quaternion (body-frame rates); a body's rotational Jacobian comes from finite differences of its rotation matrix.
  basis rows: frame . (Jp2 - Jp1), and n . (Jr2 - Jr1) for torsion; body order table -> cube, link -> cube, table -> link.
VIRTUAL WORK
  Q = sum over contacts of (Jp2 - Jp1)^T (frame^T F[0:3]) + (Jr2 - Jr1)^T n F[3].
SWITCHES
  Every sensitivity control is a field of Switches: a deliberately wrong version of the REFERENCE, never of the code under test."""
import dataclasses
import itertools

import numpy as np

from regime_states import quat2mat

H = 1e-4          # central-difference steps H and H / 2 (rad, m)


def sphere_slots(nlink):
    return 2 * (nlink // 10)            # KM_SPHERE_SLOTS


def sphere_table_slots(nlink):
    return 6 if nlink >= 20 else 2      # KM_SPHERE_TABLE_SLOTS


@dataclasses.dataclass(frozen=True)
class Switches:
    swap_half: tuple = None             # (a, b): the two half sizes exchanged
    negate_normal: bool = False
    point: str = "mid"                  # "mid" | "box" (the box surface) | "centre" (the sphere centre)
    t_mode: str = "clamp"               # "clamp" | "unclamped" | "zero"
    inside_rule: str = "nearest"        # "nearest" (face) | "smallest_loc" (the axis of smallest |loc|)
    corners: str = "first"              # "first" four | "deepest" four
    cube_angular: str = "body"          # "body" | "world": frame of the cube's angular columns
    drop_link_torsion: bool = False     # the torsion torque on the link side left out
    drop_ancestor: bool = False         # the column of the contact link's parent joint left out


RIGHT = Switches()


# ------------------------------------------------------------------------------------------------------------ box distance
def box_features(half):
    """[(kind, id, fixed)]: kind "face" / "edge" / "vertex"; fixed = {axis: sign}.  Ids: face 2 a + (sign > 0); edge 4 a + 2 (s_b > 0)
    + (s_c > 0) with a the free axis and b < c the others; vertex = the corner index of the collision (bit a set: +half_a)."""
    out = []
    for a in range(3):
        for s in (-1, 1):
            out.append(("face", 2 * a + (s > 0), {a: s}))
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for sb, sc in itertools.product((-1, 1), repeat=2):
            out.append(("edge", 4 * a + 2 * (sb > 0) + (sc > 0), {b: sb, c: sc}))
    for sg in itertools.product((-1, 1), repeat=3):
        out.append(("vertex", sum((sg[a] > 0) << a for a in range(3)), dict(enumerate(sg))))
    return out


def closest_on_box(half, p, inside_rule="nearest"):
    """(signed distance, closest surface point, kind, id) of point p in the box frame."""
    half, p = np.asarray(half, dtype=np.float64), np.asarray(p, dtype=np.float64)
    inside = bool((np.abs(p) < half).all())
    best = None
    for kind, fid, fixed in box_features(half):
        if inside and kind != "face":
            continue
        q = p.copy()
        for a, s in fixed.items():
            q[a] = s * half[a]
        if any(abs(p[a]) > half[a] for a in range(3) if a not in fixed):
            continue                                        # the projection misses the feature: a lower-dimensional one covers it
        dd = float(np.linalg.norm(q - p))
        if best is None or dd < best[0]:
            best = (dd, q, kind, fid)
    dd, q, kind, fid = best
    if inside and inside_rule == "smallest_loc":            # a wrong rule, kept as a sensitivity control
        a = int(np.argmin(np.abs(p)))
        s = 1 if p[a] >= 0 else -1
        q = p.copy(); q[a] = s * half[a]
        dd, fid = float(abs(q[a] - p[a])), 2 * a + (s > 0)
    return (-dd if inside else dd), q, ("inside" if inside else kind), fid


def _check_normal(half, p, n_loc):
    """n_loc against minus the central-difference gradient of the signed distance at p (box frame)."""
    e = 1e-7
    g = np.array([(closest_on_box(half, p + e * np.eye(3)[a])[0] - closest_on_box(half, p - e * np.eye(3)[a])[0]) / (2 * e) for a in range(3)])
    assert np.abs(n_loc + g).max() < 1e-6, (p, n_loc, g)


def make_frame(n):
    n = np.asarray(n, dtype=np.float64)
    n = n / np.linalg.norm(n)
    y = np.array([0.0, 1.0, 0.0]) if abs(n[1]) < 0.5 else np.array([0.0, 0.0, 1.0])
    t1 = y - (n @ y) * n
    t1 /= np.linalg.norm(t1)
    fr = np.stack([n, t1, np.cross(n, t1)])
    assert np.abs(fr @ fr.T - np.eye(3)).max() < 1e-14 and np.linalg.det(fr) > 0
    return fr


# ---------------------------------------------------------------------------------------------------------------- geometry
def body_poses(cm, orc, qpos):
    """(pos[nl + 1, 3], mat[nl + 1, 3, 3]): the links from Oracle.fk, body nl the cube from qpos itself."""
    nl = cm.nlink
    qpos = np.asarray(qpos, dtype=np.float64)
    xpos, xquat, _, _ = orc.fk(qpos)
    q = qpos[nl + 3:nl + 7]
    pos = np.concatenate([xpos, qpos[None, nl:nl + 3]])
    mat = np.stack([quat2mat(x) for x in xquat] + [quat2mat(q / np.linalg.norm(q))])
    return pos, mat


def geometry(cm, orc, qpos, sw=RIGHT):
    """dict(contacts, mask, info).  contacts: the kept contacts in mask-bit order, each dict(bit, kind, pos[3], frame[3, 3], dist,
    b1, b2 (-1 world, 0..nl-1 link, nl cube), dim, and for census and margins: sphere, region, feature, loc, t, t_raw, faces).
    info: n_corners (penetrating, kept or not), n_sphere_cube, n_sphere_table, and `margin`: dict of the smallest distances of
    the state to a branch boundary."""
    d = cm.desc
    nl = cm.nlink
    half = np.array(d.cube_half)
    if sw.swap_half is not None:
        a, b = sw.swap_half
        half[[a, b]] = half[[b, a]]
    rect = np.array(d.table_rect)
    pos, mat = body_poses(cm, orc, qpos)
    cpos, cmat = pos[nl], mat[nl]
    up = make_frame([0.0, 0.0, 1.0])
    margin = dict(dist=np.inf, rect=np.inf, loc=np.inf, faces=np.inf, ny=np.inf, t=np.inf)

    def over(p, penetrating):
        if penetrating:
            margin["rect"] = min(margin["rect"], float(np.abs([p[0] - rect[0], p[0] - rect[1], p[1] - rect[2], p[1] - rect[3]]).min()))
        return rect[0] <= p[0] <= rect[1] and rect[2] <= p[1] <= rect[3]

    contacts = []
    # table -> cube: corners
    pen = []
    for i in range(8):
        c = cpos + cmat @ (half * [(1 if i & 1 else -1), (1 if i & 2 else -1), (1 if i & 4 else -1)])
        dist = float(c[2] - d.table_z)
        margin["dist"] = min(margin["dist"], abs(dist))
        if dist < 0 and over(c, True):
            pen.append((i, c, dist))
    keep = pen[:4] if sw.corners == "first" else sorted(sorted(pen, key=lambda x: x[2])[:4], key=lambda x: x[0])
    for i, c, dist in keep:
        contacts.append(dict(bit=i, kind="corner", pos=c - [0.0, 0.0, 0.5 * dist], frame=up, dist=dist, b1=-1, b2=nl, dim=4))
    n_corners = len(pen)
    # link -> cube: spheres and capsule sections
    n_sc, kept = 0, 0
    for s in range(d.nsphere):
        l = d.sphere_link[s]
        rad = float(d.sphere_radius[s])
        ctr = pos[l] + mat[l] @ np.array(d.sphere_pos[s])
        seg = mat[l] @ np.array(d.sphere_seg[s])
        t = t_raw = None
        if seg @ seg > 0:
            t_raw = float((cpos - ctr) @ seg / (seg @ seg))
            t = {"clamp": min(max(t_raw, 0.0), 1.0), "unclamped": t_raw, "zero": 0.0}[sw.t_mode]
            ctr = ctr + t * seg
        loc = cmat.T @ (ctr - cpos)
        sd, q, region, fid = closest_on_box(half, loc, sw.inside_rule)
        dist = sd - rad
        margin["dist"] = min(margin["dist"], abs(dist))
        if not dist < 0:
            continue
        n_sc += 1
        if kept == sphere_slots(nl):
            continue
        kept += 1
        n_loc = (q - loc) / np.linalg.norm(q - loc) * (1.0 if sd > 0 else -1.0)
        faces = np.sort(half - np.abs(loc))
        margin["loc"] = min(margin["loc"], float(np.abs(np.abs(loc) - half).min()))
        # (the difference quotient needs the centre clear of every feature boundary by more than its step; nearer than that the
        # state is reported through margin["loc"] / margin["faces"], which every builder rejects)
        if sw == RIGHT and float(np.abs(np.abs(loc) - half).min()) > 1e-6 and (region != "inside" or faces[1] - faces[0] > 1e-6):
            _check_normal(half, loc, n_loc)
        if region == "inside":
            margin["faces"] = min(margin["faces"], float(faces[1] - faces[0]))
        if t_raw is not None:
            margin["t"] = min(margin["t"], abs(t_raw), abs(t_raw - 1.0))
        n = cmat @ n_loc * (-1.0 if sw.negate_normal else 1.0)
        margin["ny"] = min(margin["ny"], abs(abs(n[1]) - 0.5))
        surf = cpos + cmat @ q
        p = {"mid": 0.5 * (surf + ctr + n * rad), "box": surf, "centre": ctr}[sw.point]
        contacts.append(dict(bit=8 + s, kind="sphere_cube", pos=p, frame=make_frame(n), dist=dist, b1=l, b2=nl, dim=4, sphere=s,
                             region=region, feature=fid, loc=loc, t=t, t_raw=t_raw, centre=ctr))
    # table -> link: spheres (a capsule touches the table in its end spheres, which are candidates of their own)
    n_st, kept = 0, 0
    for s in range(d.nsphere):
        l = d.sphere_link[s]
        rad = float(d.sphere_radius[s])
        ctr = pos[l] + mat[l] @ np.array(d.sphere_pos[s])
        dist = float(ctr[2] - rad - d.table_z)
        margin["dist"] = min(margin["dist"], abs(dist))
        if dist < 0 and over(ctr, True):
            n_st += 1
            if kept == sphere_table_slots(nl):
                continue
            kept += 1
            low = ctr - [0.0, 0.0, rad]
            contacts.append(dict(bit=20 + s, kind="sphere_table", pos=0.5 * (low + [low[0], low[1], d.table_z]), frame=up, dist=dist,
                                 b1=-1, b2=l, dim=3, sphere=s))
    mask = 0
    for c in contacts:
        mask |= 1 << c["bit"]
    return dict(contacts=contacts, mask=mask, info=dict(n_corners=n_corners, n_sphere_cube=n_sc, n_sphere_table=n_st, margin=margin))


# -------------------------------------------------------------------------------------------------------------------- rows
def _perturbed(cm, qpos, j, h, world=False):
    """qpos moved by h along dof j: a joint coordinate, a cube translation, or a rotation of the cube by h about its body axis
    j - nl - 3 (its quaternion right-multiplied; left-multiplied with `world`)."""
    nl = cm.nlink
    q = np.array(qpos, dtype=np.float64)
    if j < nl + 3:
        q[j] += h
        return q
    k = j - nl - 3
    dq = np.zeros(4); dq[0] = np.cos(0.5 * h); dq[1 + k] = np.sin(0.5 * h)
    a, b = (dq, q[nl + 3:nl + 7]) if world else (q[nl + 3:nl + 7], dq)
    q[nl + 3:nl + 7] = [a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))]
    return q


class Rows:
    """The finite-difference Jacobians of one state: the body poses at qpos +- H and +- H / 2 along every dof, evaluated once."""

    def __init__(self, cm, orc, qpos, sw=RIGHT, h=H):
        self.cm, self.sw, self.nl, self.nv = cm, sw, cm.nlink, cm.nv
        self.steps = (h, 0.5 * h)
        self.pos0, self.mat0 = body_poses(cm, orc, qpos)
        world = sw.cube_angular == "world"
        self.pm = [[(body_poses(cm, orc, _perturbed(cm, qpos, j, +st, world)), body_poses(cm, orc, _perturbed(cm, qpos, j, -st, world)))
                    for j in range(cm.nv)] for st in self.steps]

    def jac(self, body, pt):
        """(Jp[2, 3, nv], Jr[2, 3, nv]) of the world point pt fixed in `body`, at the two step sizes (unextrapolated)."""
        jp, jr = np.zeros((2, 3, self.nv)), np.zeros((2, 3, self.nv))
        if body < 0:
            return jp, jr
        local = self.mat0[body].T @ (np.asarray(pt) - self.pos0[body])
        for i, st in enumerate(self.steps):
            for j in range(self.nv):
                (pa, ma), (pb, mb) = self.pm[i][j]
                jp[i, :, j] = ((pa[body] + ma[body] @ local) - (pb[body] + mb[body] @ local)) / (2 * st)
                W = (ma[body] - mb[body]) / (2 * st) @ self.mat0[body].T
                jr[i, :, j] = 0.5 * np.array([W[2, 1] - W[1, 2], W[0, 2] - W[2, 0], W[1, 0] - W[0, 1]])
        return jp, jr

    def basis(self, c):
        """(rows[4, nv], err): normal, tangent 1, tangent 2, torsion of contact c, Richardson-extrapolated, and the largest
        |rows(H) - rows(H / 2)|."""
        d = self.cm.desc
        jp1, jr1 = self.jac(c["b1"], c["pos"])
        jp2, jr2 = self.jac(c["b2"], c["pos"])
        if self.sw.drop_link_torsion and 0 <= c["b1"] < self.nl:
            jr1 = np.zeros_like(jr1)
        if self.sw.drop_ancestor:
            for b, jp, jr in ((c["b1"], jp1, jr1), (c["b2"], jp2, jr2)):
                if 0 <= b < self.nl and d.link_parent[b] >= 0:
                    jp[:, :, d.link_parent[b]] = 0.0
                    jr[:, :, d.link_parent[b]] = 0.0
        fr = c["frame"]
        at = [np.concatenate([fr @ (jp2[i] - jp1[i]), (fr[0] @ (jr2[i] - jr1[i]))[None]]) for i in range(2)]
        return (4.0 * at[1] - at[0]) / 3.0, float(np.abs(at[0] - at[1]).max())


def rows(cm, orc, qpos, geo=None, sw=RIGHT, h=H):
    """[(basis[4, nv], err)] for the contacts of geometry(cm, orc, qpos, sw) (or of `geo`), in their order."""
    geo = geometry(cm, orc, qpos, sw) if geo is None else geo
    r = Rows(cm, orc, qpos, sw, h)
    return [r.basis(c) for c in geo["contacts"]]


def virtual_work(basis_rows, forces):
    """Q[nv] = sum_c basis_c^T F_c: F_c[0:3] along the frame rows, F_c[3] the torsion torque about the normal."""
    return sum(b.T @ np.asarray(f) for (b, _), f in zip(basis_rows, forces))


# ---------------------------------------------------------------------------------------------- the oracle's rows, decoded
def oracle_basis(cm, dyn, types, qpos, contacts):
    """The oracle's basis rows [4, nv] per contact from Oracle.dynamics' J: normal = half the sum of an edge pair, tangent and torsion =
    its difference over 2 mu.  Row order: friction loss, limits, then the contacts in mask-bit order (dim - 1 edge pairs each)."""
    d = cm.desc
    nl = cm.nlink
    row = int((types == 0).sum()) + sum(qpos[j] < d.jnt_range[j][0] or qpos[j] > d.jnt_range[j][1] for j in range(nl))
    out = []
    for c in contacts:
        fr = d.con_cube_friction if c["dim"] == 4 else d.con_def_friction
        mu = [fr[0], fr[0], fr[1]]
        b = np.zeros((4, cm.nv))
        for e in range(c["dim"] - 1):
            jp, jm = dyn["J"][row + 2 * e], dyn["J"][row + 2 * e + 1]
            if e == 0:
                b[0] = 0.5 * (jp + jm)
            else:
                assert np.abs(0.5 * (jp + jm) - b[0]).max() < 1e-12
            b[1 + e] = (jp - jm) / (2 * mu[e])
        out.append(b)
        row += 2 * (c["dim"] - 1)
    assert row == dyn["nefc"], (row, dyn["nefc"])
    return out
