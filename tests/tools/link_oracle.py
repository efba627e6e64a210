"""Float64 NumPy ray caster of the whole camera scene WITH link capsules: the reference of tests/test_render_links_*.py.

It restates render_any of oracle/kmanip_oracle.c operation for operation -- table rectangle, cube slab test, visible spheres,
Lambert shading under an env's `vis` vector -- so that with an empty capsule list its bytes ARE Oracle.render_rgb's
(tests/test_render_links_cpu.py pins that), and adds the capsule ray test of DESIGN.md section 14 and the per-pixel labels.  The
link frames come from Oracle.fk; the per-env camera offset is the desc's cam_pos (model.with_visual_params), as for the oracle.

A capsule is a dict with the fields of KLinkCapsule (model.link_capsules).  With ray o + t d, dd = |d|^2, A / B the world end
points, u = (B - A) / |B - A|, L = |B - A|, oa = o - A, ou = oa.u, c = oa.oa - ou^2 - r^2:
  body         du = d.u, a = dd - du^2, b = d.oa - du ou, h = b^2 - a c; if h >= 0: t = (-b - sqrt(h)) / a, valid while
               0 < ou + t du < L;
  end spheres  the entry root (-b_s - sqrt(disc_s)) / dd at A and at B, as for the finger spheres;
  the capsule's t is the body's if valid, else the smaller end-sphere root; it wins while t > 0 and t < best (objects in the order
  table, cube, spheres, capsules in list order: an earlier object keeps a tie);
  normal       (P - (A + clamp(s, 0, L) u)) / r with s = (P - A).u; material 3, shaded as a sphere; label = the capsule's."""
import numpy as np

from gym_kmanip_amd.model import (KM_SEG_ROBOT_R, KM_VP_N, VISUAL_PARAMS, sphere_arm, visual_param_vector,
                                  with_visual_params)

R3, R2 = 0.57735026918962576451, 0.70710678118654752440
LIGHTS = ((-R3, -R3, R3), (R3, -R3, R3), (0.0, R2, R2))


def _q2m(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _dot(a, b):
    """dot3 of the oracle, in its order; a, b: [..., 3] or (3,)."""
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


class LinkOracle:
    """render(qpos, cam, h, w, caps, vis, arm) -> (rgb uint8 [h, w, 3], labels uint8 [h, w] of KM_SEG_*, capsule mask bool [h, w])
    for one env's qpos.  vis: the env's float64[KM_VP_N] (model.visual_param_vector) or None; arm: draw only that arm's spheres
    and capsules (the arm split of the label tests).  camera_offset: the env's per-env camera offset."""

    def __init__(self, cm, camera_offset=None):
        from oracle.oracle import Oracle
        if camera_offset is not None:
            cm = with_visual_params(cm, camera_offset=camera_offset)
        self.cm = cm
        self.orc = Oracle(cm, 1)
        self.sarm = sphere_arm(cm)

    def render(self, qpos, cam, H, W, caps=(), vis=None, arm=None):
        d = self.cm.desc
        qpos = np.asarray(qpos, dtype=np.float64)
        xpos, xquat, _, _ = self.orc.fk(qpos)
        xmat = [_q2m(xquat[i]) for i in range(d.nlink)]

        def world(l, p):
            p = np.array(list(p), dtype=np.float64)
            return p if l < 0 else xpos[l] + xmat[l] @ p
        co = world(d.cam_link[cam], d.cam_pos[cam])
        to = world(d.cam_target_link[cam], d.cam_target_pos[cam])
        z = co - to
        z /= np.linalg.norm(z)
        x = np.cross([0, 0, 1.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        y /= np.linalg.norm(y)
        f = 0.5 * H / np.tan(0.5 * d.cam_fovy[cam] * (np.pi / 180.0))
        c, r = np.meshgrid(np.arange(W), np.arange(H))
        dx = (c + 0.5 - 0.5 * W) / f
        dy = -(r + 0.5 - 0.5 * H) / f
        D = x[None, None] * dx[..., None] + y[None, None] * dy[..., None] - z[None, None]
        best = np.full((H, W), float(d.cam_zfar))
        mat = np.zeros((H, W), dtype=np.int64)
        lab = np.zeros((H, W), dtype=np.int64)
        nrm = np.zeros((H, W, 3))
        nrm[..., 2] = 1
        capmask = np.zeros((H, W), dtype=bool)
        with np.errstate(all="ignore"):
            # table
            t = (d.table_z - co[2]) / D[..., 2]
            hx, hy = co[0] + t * D[..., 0], co[1] + t * D[..., 1]
            tr = list(d.table_rect)
            ok = (D[..., 2] != 0) & (t > 0) & (t < best) & (hx >= tr[0]) & (hx <= tr[1]) & (hy >= tr[2]) & (hy <= tr[3])
            best = np.where(ok, t, best); mat = np.where(ok, 1, mat); lab = np.where(ok, 1, lab)
            # cube
            nq = d.nlink
            cp, cm_ = qpos[nq:nq + 3], _q2m(qpos[nq + 3:nq + 7])
            rel = co - cp
            ol = np.array([_dot(cm_[:, a], rel) for a in range(3)])
            dl = np.stack([cm_[0, a] * D[..., 0] + cm_[1, a] * D[..., 1] + cm_[2, a] * D[..., 2] for a in range(3)], axis=-1)
            t0 = np.full((H, W), -np.inf); t1 = np.full((H, W), np.inf)
            a0 = np.zeros((H, W), dtype=np.int64); a1 = np.zeros((H, W), dtype=np.int64)
            s0 = np.zeros((H, W)); s1 = np.zeros((H, W))
            okc = np.ones((H, W), dtype=bool)
            for a in range(3):
                h = d.cube_half[a]
                ta = (-h - ol[a]) / dl[..., a]; tb = (h - ol[a]) / dl[..., a]
                sw = ta > tb
                ta, tb = np.where(sw, tb, ta), np.where(sw, ta, tb)
                sa = np.where(sw, 1.0, -1.0); sb = -sa
                nz = dl[..., a] != 0
                up = nz & (ta > t0); t0 = np.where(up, ta, t0); a0 = np.where(up, a, a0); s0 = np.where(up, sa, s0)
                up = nz & (tb < t1); t1 = np.where(up, tb, t1); a1 = np.where(up, a, a1); s1 = np.where(up, sb, s1)
                okc &= nz | ~((ol[a] < -h) | (ol[a] > h))
            front = t0 > 0
            tt = np.where(front, t0, t1)
            hit = okc & (t0 <= t1) & (t1 > 0) & (tt < best)
            ax = np.where(front, a0, a1); sg = np.where(front, s0, s1)
            best = np.where(hit, tt, best); mat = np.where(hit, 2, mat); lab = np.where(hit, 2, lab)
            nrm = np.where(hit[..., None], sg[..., None] * cm_.T[ax], nrm)
            # visible spheres
            dd = _dot(D, D)
            for s in range(d.nsphere):
                if not d.sphere_visible[s] or (arm is not None and self.sarm[s] != arm):
                    continue
                oc = co - world(d.sphere_link[s], d.sphere_pos[s])
                R = d.sphere_radius[s]
                b = _dot(D, oc); disc = b * b - dd * (_dot(oc, oc) - R * R)
                t = (-b - np.sqrt(disc)) / dd
                hit = (disc >= 0) & (t > 0) & (t < best)
                best = np.where(hit, t, best); mat = np.where(hit, 3, mat); lab = np.where(hit, KM_SEG_ROBOT_R + self.sarm[s], lab)
                nrm = np.where(hit[..., None], (oc[None, None] + t[..., None] * D) / R, nrm)
            # link capsules
            for cap in caps:
                if not (int(cap["cam_mask"]) >> cam) & 1 or (arm is not None and cap["label"] != KM_SEG_ROBOT_R + arm):
                    continue
                l, R = cap["link"], float(cap["radius"])
                p0, seg = np.asarray(cap["p0"], dtype=np.float64), np.asarray(cap["seg"], dtype=np.float64)
                A = world(l, p0)
                sv = xmat[l] @ seg
                B = A + sv
                L = np.sqrt(_dot(sv, sv))
                u = sv / L if L > 0 else np.array([0.0, 0.0, 1.0])
                oa, ob = co - A, co - B
                ou = _dot(oa, u)
                cc = _dot(oa, oa) - ou * ou - R * R
                du = _dot(D, u)
                a_ = dd - du * du
                b_ = _dot(D, oa) - du * ou
                h = b_ * b_ - a_ * cc
                tb = (-b_ - np.sqrt(h)) / a_
                sb = ou + tb * du
                body = (h >= 0) & (sb > 0) & (sb < L)
                te = np.full((H, W), np.inf)
                for oe in (oa, ob):
                    bs = _dot(D, oe); disc = bs * bs - dd * (_dot(oe, oe) - R * R)
                    ts = (-bs - np.sqrt(disc)) / dd
                    te = np.minimum(te, np.where(disc >= 0, ts, np.inf))
                t = np.where(body, tb, te)
                hit = np.isfinite(t) & (t > 0) & (t < best)
                t = np.where(hit, t, 0.0)
                s = np.clip(ou + t * du, 0.0, L)
                n = (oa[None, None] + t[..., None] * D - s[..., None] * u[None, None]) / R
                best = np.where(hit, t, best); mat = np.where(hit, 3, mat); lab = np.where(hit, int(cap["label"]), lab)
                nrm = np.where(hit[..., None], n, nrm)
                capmask = np.where(hit, True, capmask)                      # (a later sphere cannot follow: capsules are last)
            # Lambert shading, in the oracle's order of operations
            col = np.array([[0, 0, 0], [0.2, 0.2, 0.2], [1, 0, 0], [0.647059] * 3], dtype=np.float64)
            amb, hl, dls = 0.4, 0.4, 0.3
            if vis is not None:
                vis = np.asarray(vis, dtype=np.float64)
                assert vis.shape == (KM_VP_N,)
                for m_, name in enumerate(("background_rgb", "table_rgb", "cube_rgb", "robot_rgb")):
                    k = VISUAL_PARAMS[name][0]
                    col[m_] = vis[k:k + 3]
                amb, hl = vis[VISUAL_PARAMS["ambient"][0]], vis[VISUAL_PARAMS["headlight"][0]]
                dls = 0.3 * vis[VISUAL_PARAMS["directional"][0]]
            head = np.maximum(0.0, -_dot(nrm, D) / np.sqrt(dd))
            I = amb + hl * head
            for Ll in LIGHTS:
                I = I + dls * np.maximum(0.0, nrm[..., 0] * Ll[0] + nrm[..., 1] * Ll[1] + nrm[..., 2] * Ll[2])
            I = np.minimum(I, 1.0)
            rgb = np.where((mat > 0)[..., None], 255.0 * col[mat] * I[..., None], 255.0 * col[0][None, None]) + 0.5
        return rgb.astype(np.uint8), lab.astype(np.uint8), capmask

    def rgb(self, qpos, cam, H, W, caps=(), vis=None):
        return self.render(qpos, cam, H, W, caps, vis)[0]

    def labels(self, qpos, cam, H, W, caps=(), arm=None):
        return self.render(qpos, cam, H, W, caps, None, arm)[1]


def flat_vector():
    """tests/tools/label_oracle.py FLAT as a vector: the RGB render then stores the material id."""
    from label_oracle import FLAT
    return visual_param_vector(dict(FLAT))
