"""Float64 reference of the camera poses and of the point-cloud render: the reference of tests/test_points_*.py.

The camera frame is built from Oracle.fk exactly as tests/tools/link_depth_oracle.py builds it (MuJoCo's targetbody camera:
z = (camera - target) / |.|, x = (0, 0, 1) x z, y = z x x; the per-env camera offset is the desc's cam_pos, through
model.with_visual_params).  The depth is LinkDepthOracle.render: the CPU oracle's ko_render_depth plus the capsule restatement.
A pixel's point is the back-projection of that float32 depth D32 along the oracle's own ray (oracle/kmanip_oracle.c render_any):

    dx = (c + 0.5 - W/2) / f,  dy = -(r + 0.5 - H/2) / f,  f = (H/2) / tan(fovy/2)
    camera frame  (D32 dx, D32 dy, -D32)           world frame  o + D32 (x dx + y dy - z)

in float64, not rounded: the tests' bar accounts for the float32 of the depth and of the stored component."""
import numpy as np

from link_depth_oracle import LinkDepthOracle
from link_oracle import _q2m


class PointOracle:
    """One env's reference.  camera_offset: the env's per-env camera offset."""

    def __init__(self, cm, camera_offset=None):
        self.ldo = LinkDepthOracle(cm, camera_offset=camera_offset)
        self.cm = self.ldo.cm                      # (with the offset in cam_pos)
        self.orc = self.ldo.orc

    def pose(self, qpos, cam):
        """(pos float64 [3], mat float64 [3, 3] with the camera's x, y, z axes as COLUMNS): MuJoCo's cam_xpos / cam_xmat."""
        d = self.cm.desc
        qpos = np.asarray(qpos, dtype=np.float64)
        xpos, xquat, _, _ = self.orc.fk(qpos)

        def world(l, p):
            p = np.array(list(p), dtype=np.float64)
            return p if l < 0 else xpos[l] + _q2m(xquat[l]) @ p
        co = world(d.cam_link[cam], d.cam_pos[cam])
        to = world(d.cam_target_link[cam], d.cam_target_pos[cam])
        z = co - to
        z /= np.linalg.norm(z)
        x = np.cross([0, 0, 1.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        y /= np.linalg.norm(y)
        return co, np.stack([x, y, z], axis=1)

    def target(self, qpos, cam):
        """The world point the camera tracks."""
        d = self.cm.desc
        xpos, xquat, _, _ = self.orc.fk(np.asarray(qpos, dtype=np.float64))
        l, p = d.cam_target_link[cam], np.array(list(d.cam_target_pos[cam]), dtype=np.float64)
        return p if l < 0 else xpos[l] + _q2m(xquat[l]) @ p

    def focal(self, cam, H):
        return 0.5 * H / np.tan(0.5 * self.cm.desc.cam_fovy[cam] * (np.pi / 180.0))

    def rays(self, cam, H, W):
        """dx, dy float64 [H, W] of every pixel."""
        f = self.focal(cam, H)
        c, r = np.meshgrid(np.arange(W), np.arange(H))
        return (c + 0.5 - 0.5 * W) / f, -(r + 0.5 - 0.5 * H) / f

    def render(self, qpos, cam, H, W, caps=(), frame="world"):
        """-> (points float64 [H, W, 3], depth float32 [H, W], capsule mask bool [H, W], dx, dy)."""
        depth, mask = self.ldo.render(qpos, cam, H, W, caps)
        dx, dy = self.rays(cam, H, W)
        D = depth.astype(np.float64)
        if frame == "camera":
            pts = np.stack([D * dx, D * dy, -D], axis=-1)
        else:
            o, m = self.pose(qpos, cam)
            d = m[:, 0][None, None] * dx[..., None] + m[:, 1][None, None] * dy[..., None] - m[:, 2][None, None]
            pts = o[None, None] + D[..., None] * d
        return pts, depth, mask, dx, dy
