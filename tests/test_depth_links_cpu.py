"""Link capsules in the depth renders, host side (no GPU): the reference the GPU tests are held to (tests/tools/link_depth_oracle.py)
against the CPU oracle and against the RGB / label reference of tests/tools/link_oracle.py, and the library's new kernels and entry
points."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd import model as M
from gym_kmanip_amd.model import KM_CAM_INDEX
from test_render_links_cpu import _cams, _states

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from link_depth_oracle import LinkDepthOracle  # noqa: E402
from link_oracle import LinkOracle  # noqa: E402

SHAPES = [(64, 64), (30, 50)]
ENVS = ["KManipSoloArm", "KManipTorso"]


@pytest.mark.parametrize("env", ENVS)
def test_reference_without_capsules_is_the_oracle(env):
    """With an empty list the reference is Oracle.render_depth bit for bit, with and without a per-env camera offset."""
    from oracle.oracle import Oracle
    cm, qpos = _states(env)
    off = np.array([0.03, -0.02, 0.04])
    for o, ref in ((Oracle(cm, 1), LinkDepthOracle(cm)),
                   (Oracle(M.with_visual_params(cm, camera_offset=off), 1), LinkDepthOracle(cm, camera_offset=off))):
        for cam in _cams(cm):
            ci = KM_CAM_INDEX[cam]
            for h, w in SHAPES:
                for e in range(len(qpos)):
                    got, mask = ref.render(qpos[e], ci, h, w, ())
                    want = o.render_depth(qpos[e], ci, h, w)
                    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cam, h, w, e)
                    assert not mask.any()
    a = LinkDepthOracle(cm).depth(qpos[0], KM_CAM_INDEX["grip_r"], 30, 50)
    b = LinkDepthOracle(cm, camera_offset=off).depth(qpos[0], KM_CAM_INDEX["grip_r"], 30, 50)
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("env", ENVS)
def test_reference_with_the_default_list(env):
    """Every camera, 64 x 64 and 30 x 50, 6 envs, the default list: the capsule mask equals LinkOracle.render(...)[2] on every pixel
    but float32 ties, depth differs from the empty-list depth exactly on that mask (and is nearer there), every camera and shape
    shows capsule pixels, and all values lie within [znear, zfar].
    Ties: LinkOracle compares in float64, the depth image stores float32.  Where a finger capsule's body meets its end sphere --
    which IS the drawn finger sphere -- the capsule is nearer than the sphere by ~1e-12 m: a capsule pixel in float64, the same
    float32 depth either way.  A pixel where the two masks differ must be exactly that: LinkOracle says capsule, and the capsule's
    float64 root rounds to the scene's float32 depth.  (KManipSoloArm grip_r 64 x 64 has 2 such pixels over the 6 envs.)"""
    cm, qpos = _states(env)
    d = cm.desc
    caps = M.link_capsules(cm)
    ref, lo = LinkDepthOracle(cm), LinkOracle(cm)
    for cam in _cams(cm):
        ci = KM_CAM_INDEX[cam]
        for h, w in SHAPES:
            npix = ties = 0
            for e in range(len(qpos)):
                base = ref.depth(qpos[e], ci, h, w)
                depth, mask = ref.render(qpos[e], ci, h, w, caps)
                want = lo.render(qpos[e], ci, h, w, caps)[2]
                tie = mask != want
                if tie.any():
                    tc = np.clip(ref.capsule_t(qpos[e], ci, h, w, caps), d.cam_znear, d.cam_zfar).astype(np.float32)
                    assert (want[tie] & (tc[tie] == base[tie])).all(), (cam, h, w, e, int(tie.sum()))
                    ties += int(tie.sum())
                assert np.array_equal(depth != base, mask) and (depth[mask] < base[mask]).all(), (cam, h, w, e)
                assert depth.dtype == np.float32 and (depth >= np.float32(d.cam_znear)).all() and (depth <= np.float32(d.cam_zfar)).all()
                npix += int(mask.sum())
            print(env, cam, h, w, "capsule pixels over the envs", npix, "float32 ties", ties)
            assert npix > 0 and ties <= 1e-3 * npix + 2, (cam, h, w, npix, ties)


def test_cam_mask_and_spheres_in_the_reference():
    """A capsule whose cam_mask lacks the camera is not drawn; a zero-length capsule at a finger sphere with its radius changes
    no depth value (the sphere's depth, to the float32 the image stores)."""
    cm, qpos = _states("KManipSoloArm")
    d = cm.desc
    ref = LinkDepthOracle(cm)
    ci = KM_CAM_INDEX["head"]
    caps = M.link_capsules(cm)
    base = ref.depth(qpos[0], ci, 30, 50)
    assert np.array_equal(ref.depth(qpos[0], ci, 30, 50, [dict(c, cam_mask=c["cam_mask"] & ~(1 << ci)) for c in caps]), base)
    assert not np.array_equal(ref.depth(qpos[0], ci, 30, 50, caps), base)
    s = next(s for s in range(d.nsphere) if d.sphere_visible[s])
    cap = {"link": d.sphere_link[s], "label": M.KM_SEG_ROBOT_R, "cam_mask": 15, "p0": tuple(d.sphere_pos[s]), "seg": (0.0, 0.0, 0.0),
           "radius": d.sphere_radius[s]}
    for cam in _cams(cm):
        a = ref.depth(qpos[1], KM_CAM_INDEX[cam], 40, 60)
        assert np.array_equal(ref.depth(qpos[1], KM_CAM_INDEX[cam], 40, 60, [cap]), a), cam


def test_depth_link_kernel_resources_and_exports():
    """The four k_render_depth_links instantiations (COLFIXED x VIS) exist, the COLFIXED ones do not spill to scratch, k_render_depth
    and k_render_links keep their four instantiations each, and the two new entry points are declared, exported and loadable."""
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    if not os.path.exists(klib.LIB_PATH):
        klib.build()
    all_dl = BM.kernels(klib.LIB_PATH, "k_render_depth_links")
    dl = {k.args[:2]: k for k in all_dl}                                    # (COLFIXED, VIS)
    assert len(dl) == 4 and len(all_dl) == 4, all_dl
    for key, v in dl.items():
        print("k_render_depth_links<COLFIXED=%d, VIS=%d>" % key, v)
        assert v.vgpr <= 128, (key, v)                                         # (four waves per SIMD, as k_render_depth)
        if key[0]:
            assert v.scratch == 0, (key, v)
    assert sum(type(k.args[0]) is bool for k in BM.kernels(klib.LIB_PATH, "k_render_depth")) == 4
    assert len(BM.kernels(klib.LIB_PATH, "k_render_links")) == 4
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    L = klib.load()
    for name in ("kmanip_set_depth_links", "kmanip_get_depth_links"):
        assert name + "(" in hdr and name in klib.EXPORTS and hasattr(L, name)
    assert "DEPTH IS NOT COVERED" not in hdr and "never draws link capsules" not in hdr
