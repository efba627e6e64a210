"""Reference segmentation labels from the CPU oracle's RGB ray caster, without touching the oracle.

Oracle.render_rgb with flat visual parameters -- ambient 1, no headlight, no directional lights, colours k / 255 -- stores
round(255 * 1 * k / 255) = k in all three channels: the ray caster's own `mat` (0 background, 1 table, 2 cube, 3 robot).  For the
arm split the same render runs on a copy of the model whose desc has `sphere_visible` cleared for the other arm's spheres
(model.sphere_arm): the robot pixels that remain belong to that arm."""
import dataclasses

import numpy as np

from gym_kmanip_amd.model import KModelDesc, sphere_arm, visual_param_vector, with_visual_params

FLAT = dict(table_rgb=(1 / 255,) * 3, cube_rgb=(2 / 255,) * 3, robot_rgb=(3 / 255,) * 3, background_rgb=(0.0, 0.0, 0.0),
            ambient=1.0, headlight=0.0, directional=0.0)


def flat_vector():
    """The visual parameter vector whose render is the material id."""
    return visual_param_vector(dict(FLAT))


def only_arm(cm, arm):
    """A copy of `cm` that draws the spheres of `arm` only (copied as model.with_visual_params copies)."""
    d = KModelDesc.from_buffer_copy(cm.desc)
    for s, a in enumerate(sphere_arm(cm)):
        if a != arm:
            d.sphere_visible[s] = 0
    return dataclasses.replace(cm, desc=d)


class LabelOracle:
    """labels(qpos, cam, h, w) -> uint8 [h, w] in 0..3 for one env's qpos; arm_labels(..., arm) the same with only that arm's
    spheres drawn.  camera_offset: the env's per-env camera offset (model.with_visual_params)."""

    def __init__(self, cm, camera_offset=None):
        from oracle.oracle import Oracle
        if camera_offset is not None:
            cm = with_visual_params(cm, camera_offset=camera_offset)
        self.cm = cm
        self.all = Oracle(cm, 1)
        self.arms = {a: Oracle(only_arm(cm, a), 1) for a in sorted(set(sphere_arm(cm)))}
        self.vis = flat_vector()

    def _labels(self, orc, qpos, cam, h, w):
        img = orc.render_rgb(qpos, cam, h, w, vis=self.vis)
        assert (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all(), "flat render: channels differ"
        assert img.max() <= 3
        return img[..., 0].copy()

    def labels(self, qpos, cam, h, w):
        return self._labels(self.all, qpos, cam, h, w)

    def arm_labels(self, qpos, cam, h, w, arm):
        return self._labels(self.arms[arm], qpos, cam, h, w)
