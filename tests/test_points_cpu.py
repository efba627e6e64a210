"""Camera poses and the point-cloud render, host side (no GPU): the reference the GPU tests are held to (tests/tools/point_oracle.py)
against the CPU oracle, camera_intrinsics against that reference, and the library's new kernels and entry points (DESIGN.md
section 16)."""
import fnmatch
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd import model as M
from gym_kmanip_amd.model import KM_CAM_INDEX
from test_render_links_cpu import _cams, _states

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from point_oracle import PointOracle  # noqa: E402

SHAPES = [(64, 64), (30, 50)]
ENVS = ["KManipSoloArm", "KManipTorso"]
OFFSET = np.array([0.03, -0.02, 0.04])


@pytest.mark.parametrize("offset", [None, OFFSET], ids=["plain", "camera_offset"])
@pytest.mark.parametrize("env", ENVS)
def test_reference_is_pinned_to_the_oracle(env, offset):
    """Every camera, two shapes, 6 envs, with and without a per-env camera offset.  The reference's depth IS Oracle.render_depth
    (bit for bit), and its points are that depth back-projected: in the world frame -z . (p - o) reproduces the oracle's depth on
    every pixel (to float64 roundoff of the dot products: 1e-12 m), in the camera frame -p_z is it exactly.  The pose is a frame:
    mat is orthonormal and right-handed (det = +1), mat[:, 2] points from the target to the camera, and mat[:, 0] is horizontal
    (MuJoCo's targetbody camera has no roll)."""
    from oracle.oracle import Oracle
    cm, qpos = _states(env)
    ref = PointOracle(cm, camera_offset=offset)
    orc = Oracle(cm if offset is None else M.with_visual_params(cm, camera_offset=offset), 1)
    for cam in _cams(cm):
        ci = KM_CAM_INDEX[cam]
        for e in range(len(qpos)):
            o, m = ref.pose(qpos[e], ci)
            assert np.abs(m.T @ m - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(m) - 1.0) < 1e-14, (cam, e)
            v = o - ref.target(qpos[e], ci)
            assert np.abs(m[:, 2] - v / np.linalg.norm(v)).max() < 1e-15 and abs(m[2, 0]) < 1e-15, (cam, e)
            for h, w in SHAPES:
                want = orc.render_depth(qpos[e], ci, h, w)
                pw, dw, _, dx, dy = ref.render(qpos[e], ci, h, w, (), "world")
                pc, dc, _, _, _ = ref.render(qpos[e], ci, h, w, (), "camera")
                assert dw.dtype == np.float32 and np.array_equal(dw.view(np.uint32), want.view(np.uint32)), (cam, h, w, e)
                assert np.array_equal(dc, dw)
                assert np.array_equal(-pc[..., 2], want.astype(np.float64)), (cam, h, w, e)
                assert np.abs(-((pw - o) @ m[:, 2]) - want).max() < 1e-12, (cam, h, w, e)
                # the two frames are one point: p_w = o + mat p_c
                assert np.abs(o + pc @ m.T - pw).max() < 1e-12, (cam, h, w, e)
                # and the pixel it came from: the camera-frame point projects back onto the pixel's centre
                f = ref.focal(ci, h)
                c, r = np.meshgrid(np.arange(w), np.arange(h))
                assert np.abs(pc[..., 0] / -pc[..., 2] * f + 0.5 * w - 0.5 - c).max() < 1e-9
                assert np.abs(-pc[..., 1] / -pc[..., 2] * f + 0.5 * h - 0.5 - r).max() < 1e-9
    if offset is not None:
        a, b = PointOracle(cm).pose(qpos[0], KM_CAM_INDEX["grip_r"])[0], ref.pose(qpos[0], KM_CAM_INDEX["grip_r"])[0]
        assert abs(np.linalg.norm(a - b) - np.linalg.norm(offset)) < 1e-12            # (the offset is in the hand link's frame)


def test_reference_with_capsules_moves_points_nearer():
    """With the default list the reference's points differ from the no-capsule points exactly on the capsule mask, and lie nearer
    to the camera there."""
    cm, qpos = _states("KManipTorso")
    ref = PointOracle(cm)
    caps = M.link_capsules(cm)
    ci = KM_CAM_INDEX["head"]
    p0, d0, m0, _, _ = ref.render(qpos[0], ci, 30, 50, ())
    p1, d1, m1, _, _ = ref.render(qpos[0], ci, 30, 50, caps)
    o, _ = ref.pose(qpos[0], ci)
    assert m1.any() and not m0.any()
    assert np.array_equal((p1 != p0).any(axis=-1), m1)
    assert (np.linalg.norm(p1 - o, axis=-1)[m1] < np.linalg.norm(p0 - o, axis=-1)[m1]).all()


@pytest.mark.parametrize("shape", [(64, 64), (40, 60), (480, 640)])
def test_camera_intrinsics_agree_with_the_reference(shape):
    """model.camera_intrinsics (what KManipEnvHip.camera_intrinsics returns) against the reference's focal length and image centre
    for the four cameras at three shapes, and the default size is the camera's reference resolution."""
    h, w = shape
    cm = M.compile_model("KManipTorso")
    ref = PointOracle(cm)
    assert len(_cams(cm)) == 4
    for cam in _cams(cm):
        k = M.camera_intrinsics(cm, cam, h, w)
        assert sorted(k) == ["cx", "cy", "f", "fovy"]
        assert abs(k["f"] - ref.focal(KM_CAM_INDEX[cam], h)) <= 1e-12 * k["f"], cam
        assert k["cx"] == 0.5 * w and k["cy"] == 0.5 * h and k["fovy"] == cm.desc.cam_fovy[KM_CAM_INDEX[cam]]
        dx, dy = ref.rays(KM_CAM_INDEX[cam], h, w)
        c, r = np.meshgrid(np.arange(w), np.arange(h))
        assert np.abs((c + 0.5 - k["cx"]) / k["f"] - dx).max() < 1e-15 and np.abs(-(r + 0.5 - k["cy"]) / k["f"] - dy).max() < 1e-15
        d = M.camera_intrinsics(cm, cam)
        assert (d["cx"], d["cy"]) == (0.5 * M.CAMERAS[cam].w, 0.5 * M.CAMERAS[cam].h)
    solo = M.compile_model("KManipSoloArm")
    with pytest.raises(ValueError):
        M.camera_intrinsics(solo, "grip_l", 64, 64)
    with pytest.raises(ValueError):
        M.camera_intrinsics(solo, "head", 0, 64)


def test_header_export_map_and_binding_agree():
    """The two new entry points are declared in include/kmanip.h with the signatures of the binding, pass the export map, are
    listed in lib.EXPORTS and load; KM_POINTS_* of the header are the binding's frame numbers."""
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    emap = open(os.path.join(ROOT, "gym_kmanip_amd", "csrc", "exports.map")).read()
    pats = re.search(r"global:\s*([^;]+);", emap).group(1).split()
    flat = " ".join(hdr.split())
    assert "KMANIP_API int kmanip_get_camera_poses(KHandle h, int cam, double* pose_dev, void* stream);" in flat
    assert ("KMANIP_API int kmanip_render_points(KHandle h, int cam, int height, int width, int frame, float* xyz_dev, "
            "float* depth_dev, void* stream);") in flat
    assert re.search(r"enum\s*\{\s*KM_POINTS_CAMERA = 0,\s*KM_POINTS_WORLD = 1\s*\}", hdr)
    assert klib.KM_POINTS_FRAMES == {"camera": 0, "world": 1}
    if not os.path.exists(klib.LIB_PATH):
        klib.build()
    L = klib.load()
    for name, nargs in (("kmanip_get_camera_poses", 4), ("kmanip_render_points", 8)):
        assert name in klib.EXPORTS and any(fnmatch.fnmatchcase(name, p) for p in pats), name
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs, name


def test_point_kernel_resources():
    """The eight k_render_points instantiations (COLFIXED x VIS x LINKS) and the two k_camera_poses exist; every one fits four
    waves per SIMD (128 vector registers, the depth kernels' budget) without scratch; the existing depth kernels keep their
    four instantiations each."""
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    if not os.path.exists(klib.LIB_PATH):
        klib.build()
    all_pts = BM.kernels(klib.LIB_PATH, "k_render_points")
    pts = {k.args[:3]: k for k in all_pts}                  # (COLFIXED, VIS, LINKS)
    assert len(pts) == 8 and len(all_pts) == 8, all_pts
    for key, v in sorted(pts.items()):
        print("k_render_points<COLFIXED=%d, VIS=%d, LINKS=%d>" % key, v)
        assert v.vgpr <= 128 and v.scratch == 0, (key, v)
    poses = BM.kernels(klib.LIB_PATH, "k_camera_poses")
    assert len(poses) == 2
    for v in poses:
        print("k_camera_poses", v)
        assert v.vgpr <= 128 and v.scratch == 0, v
    assert sum(type(k.args[0]) is bool for k in BM.kernels(klib.LIB_PATH, "k_render_depth")) == 4
    assert len(BM.kernels(klib.LIB_PATH, "k_render_depth_links")) == 4
