"""Float64 reference of the depth render WITH link capsules: the reference of tests/test_depth_links_*.py.

Casting to float32 and clamping to [znear, zfar] are monotonic, and a capsule wins exactly where it is strictly nearer, so the depth
image with capsules is

    np.minimum(Oracle.render_depth(qpos, cam, h, w), float32(clip(t_caps, znear, zfar)))

with t_caps the minimum, over the capsules the camera draws, of the positive capsule root (inf where no capsule is hit).  The CPU
oracle stays the reference of the scene; only the capsule block of tests/tools/link_oracle.py is restated here, operation for
operation (the camera frame and the rays as LinkOracle.render builds them; the ray test of DESIGN.md section 14).  A ray is
o + t d with d's component along the optical axis equal to 1, so t is the depth the oracle stores.  The per-env camera offset is the
desc's cam_pos (model.with_visual_params), as for LinkOracle."""
import numpy as np

from gym_kmanip_amd.model import with_visual_params
from link_oracle import _dot, _q2m


class LinkDepthOracle:
    """render(qpos, cam, h, w, caps) -> (depth float32 [h, w], capsule mask bool [h, w]: capsule depth < scene depth) for one env's
    qpos.  camera_offset: the env's per-env camera offset."""

    def __init__(self, cm, camera_offset=None):
        from oracle.oracle import Oracle
        if camera_offset is not None:
            cm = with_visual_params(cm, camera_offset=camera_offset)
        self.cm = cm
        self.orc = Oracle(cm, 1)

    def capsule_t(self, qpos, cam, H, W, caps):
        """float64 [H, W]: the smallest positive capsule root of every pixel's ray, inf where no capsule is hit."""
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
        dd = _dot(D, D)
        best = np.full((H, W), np.inf)
        with np.errstate(all="ignore"):
            for cap in caps:
                if not (int(cap["cam_mask"]) >> cam) & 1:
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
                best = np.where(hit, t, best)
        return best

    def render(self, qpos, cam, H, W, caps=()):
        d = self.cm.desc
        scene = self.orc.render_depth(qpos, cam, H, W)
        if not len(caps):
            return scene, np.zeros((H, W), dtype=bool)
        tc = np.clip(self.capsule_t(qpos, cam, H, W, caps), d.cam_znear, d.cam_zfar).astype(np.float32)
        return np.minimum(scene, tc), tc < scene

    def depth(self, qpos, cam, H, W, caps=()):
        return self.render(qpos, cam, H, W, caps)[0]
