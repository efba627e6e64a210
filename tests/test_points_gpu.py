"""Camera poses and the point-cloud render on the device (run with -m gpu on an MI355X): k_camera_poses and k_render_points through
kmanip_get_camera_poses / kmanip_render_points, against the float64 reference of tests/tools/point_oracle.py (pinned to the CPU
oracle by tests/test_points_cpu.py), against the scene's surfaces themselves, and the plumbing: one launch for points and depth,
opt-in, untouched paths, physics, snapshots and RenderBehind, validation.

THE BAR of a point (item 2 below and wherever "the point bar" is named).  The reference point is o + D32 d with D32 the reference's
float32 depth.  Component c of a pixel is off when

    |gpu - ref| > (1e-6 + 2^-24 D) max(1, |dx|, |dy|) + 2^-23 |ref_c|

-- the depth bar of 1e-6 m, the float32 rounding of the reference depth (half an ulp: 2^-24 D), both through the lever arm of the
ray, and one float32 ulp on the stored component.  A pixel is off when a component is; fewer than 5e-4 h w n pixels may be off (the
project's cap for grazing rays, where a hit is decided by the last bits of a discriminant); at 7 x 13 and 1 x 1 that admits none."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd import model as M
from gym_kmanip_amd.model import KM_CAM_INDEX
from test_kernel_paths_gpu import _cams, _stepped

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from link_oracle import _q2m  # noqa: E402
from point_oracle import PointOracle  # noqa: E402

pytestmark = pytest.mark.gpu

# the shapes of tests/test_depth_links_gpu.py (COLFIXED: the workgroup's 128 lanes are a whole number of rows; general: a partial last
# pass, fewer pixels than the workgroup, wider than the workgroup), plus one pixel
COLFIXED_SHAPES = [(64, 64), (32, 128), (48, 64)]
GENERAL_SHAPES = [(30, 50), (7, 13), (64, 200)]
SHAPES = COLFIXED_SHAPES + GENERAL_SHAPES + [(1, 1)]
ENVS = ("KManipSoloArm", "KManipTorso")
N = 6


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _np(t):
    return t.cpu().numpy()


def _make(env_id, n, seed=0):
    from gym_kmanip_amd import env_hip
    return env_hip.make(env_id, num_envs=n, seed=seed)


def _run(e, steps):
    for _ in range(steps):
        e.step_flat(e.sample_action())


def _offsets(n=N):
    return np.random.default_rng(5).uniform(-0.06, 0.06, (n, 3))


def _setup(env, vis, n=N):
    """A stepped handle (and, vis == "camera_offset", explicit per-env camera offsets: rng(5), +-0.06), its qpos and one reference
    per env."""
    dev, qpos = _stepped(env, n, 6, 12)
    if vis == "off":
        return dev, qpos, [PointOracle(dev.cm)] * n
    offs = _offsets(n)
    dev.set_visual_params(camera_offset=offs)
    return dev, qpos, [PointOracle(dev.cm, camera_offset=offs[e]) for e in range(n)]


def _pose_check(dev, refs, qpos, what):
    for cam in _cams(dev.cm):
        got = dev.camera_poses(cam)
        pos, mat = _np(got["pos"]), _np(got["mat"])
        assert pos.shape == (dev.num_envs, 3) and mat.shape == (dev.num_envs, 3, 3) and pos.dtype == np.float64
        worst = 0.0
        for e in range(dev.num_envs):
            o, m = refs[e].pose(qpos[e], KM_CAM_INDEX[cam])
            worst = max(worst, float(np.abs(pos[e] - o).max()), float(np.abs(mat[e] - m).max()))
        print("poses", *what, cam, "largest difference", worst)
        assert worst <= 1e-12, (what, cam, worst)


def _point_bar(gpu, ref, depth, dx, dy, what):
    """The point bar of the module docstring.  gpu float32 [n, h, w, 3], ref float64 [n, h, w, 3], depth [n, h, w], dx / dy [h, w]."""
    assert gpu.shape == ref.shape and gpu.dtype == np.float32, what
    n, h, w, _ = ref.shape
    lever = np.maximum(1.0, np.maximum(np.abs(dx), np.abs(dy)))
    tol = ((1e-6 + 2.0 ** -24 * depth.astype(np.float64)) * lever)[..., None] + 2.0 ** -23 * np.abs(ref)
    err = np.abs(gpu.astype(np.float64) - ref)
    bad = int((err > tol).any(axis=-1).sum())
    print("points", *what, "pixels off", bad, "of", h * w * n, "cap", 5e-4 * h * w * n, "largest difference", float(err.max()),
          "largest difference / bar", float((err / tol).max()))
    assert bad < 5e-4 * h * w * n, (what, bad)


# ------------------------------------------------------------------------------------------------ 1. poses
@pytest.mark.parametrize("env", ENVS)
def test_camera_poses_against_the_reference(env):
    """Every camera of the model, 6 envs: the live state, explicit per-env camera offsets (rng(5), +-0.06) and visual ranges mode
    after a reset (the offsets of every env's episode draw, from get_visual_params, which tests/test_visual_params_gpu.py holds to
    the host's draw bit for bit).  |gpu - reference| <= 1e-12 on all twelve numbers, the bar of kmanip_ik_eval's FK-derived
    quantities.  On an MI355X (library 0.33) the largest difference over the 21 rows (camera x mode) was 2.1e-15."""
    dev, qpos = _stepped(env, N, 6, 12)
    _pose_check(dev, [PointOracle(dev.cm)] * N, qpos, (env, "live"))
    offs = _offsets()
    dev.set_visual_params(camera_offset=offs)
    _pose_check(dev, [PointOracle(dev.cm, camera_offset=offs[e]) for e in range(N)], qpos, (env, "camera_offset"))
    dev.set_visual_param_ranges(camera_offset=(-0.06, 0.06))
    dev.k_reset()
    _run(dev, 3)
    drawn = _np(dev.get_visual_params()["camera_offset"])
    assert drawn.shape == (N, 3) and (np.abs(drawn) > 0).all() and len({tuple(r) for r in drawn}) == N
    qpos = dev.get_state()[0]
    _pose_check(dev, [PointOracle(dev.cm, camera_offset=drawn[e]) for e in range(N)], qpos, (env, "ranges"))
    out = _torch().empty((N, 12), dtype=_torch().float64, device=dev.device)
    got = dev.camera_poses("head", out=out)
    assert got["pos"].data_ptr() == out.data_ptr() and _torch().equal(got["mat"].reshape(N, 9), out[:, 3:])
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 2. points against the reference
@pytest.mark.parametrize("links", [False, True], ids=["scene", "links"])
@pytest.mark.parametrize("vis", ["off", "camera_offset"])
@pytest.mark.parametrize("env", ENVS)
def test_points_against_the_reference(env, vis, links):
    """Both frames, every camera, the seven shapes, 6 envs, VIS off and with explicit per-env camera offsets, without capsules and
    with the default list drawn (set_depth_links(True); the reference must then show capsule pixels, except in the one-pixel
    image).  One reference depth per (camera, shape, env) serves both frames.  Under the point bar of the module docstring, and
    the depth image of the same launch under the depth bar (1e-6 m, same cap).
    On an MI355X (library 0.33), over the 8 cases (196 rows per frame): no pixel off in any row; the largest difference was
    9.5e-7 m (points on the far plane, coordinates near 5 m: their float32 rounding) and the largest difference / bar 0.16 in the
    world frame and 0.15 in the camera frame; the 392 depth images of those launches equalled the reference's float32 images; the
    rows with capsules held 10 to 23 010 capsule pixels."""
    torch = _torch()
    dev, qpos, refs = _setup(env, vis)
    caps = M.link_capsules(dev.cm) if links else ()
    if links:
        dev.set_render_links(caps)
        dev.set_depth_links(True)
    for cam in _cams(dev.cm):
        ci = KM_CAM_INDEX[cam]
        for h, w in SHAPES:
            what = (env, vis, "links" if links else "scene", cam, h, w)
            ref = {f: [] for f in ("world", "camera")}
            depth, mask = [], []
            for e in range(N):
                pw, d32, mk, dx, dy = refs[e].render(qpos[e], ci, h, w, caps, "world")
                ref["world"].append(pw)
                ref["camera"].append(np.stack([d32 * dx, d32 * dy, -d32.astype(np.float64)], axis=-1))
                depth.append(d32); mask.append(mk)
            depth, mask = np.stack(depth), np.stack(mask)
            assert not links or h * w == 1 or mask.any(), ("the reference shows no capsule", what)
            for frame in ("world", "camera"):
                dout = torch.full((N, h, w), -1.0, dtype=torch.float32, device=dev.device)
                got = dev.render_points(cam, h, w, frame=frame, depth_out=dout)
                assert got.shape == (N, h, w, 3)
                _point_bar(_np(got), np.stack(ref[frame]), depth, dx, dy, what + (frame, "capsule pixels", int(mask.sum())))
                dg = _np(dout)
                bad = int((np.abs(dg - depth) > 1e-6).sum())
                print("depth of the launch", *what, frame, "pixels off by more than 1e-6 m", bad, "largest difference", float(np.abs(dg - depth).max()))
                assert bad < 5e-4 * h * w * N, (what, frame, bad)
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 3. points lie on the scene
def _on_scene(dev, cam, pts, depth, qpos, caps):
    """Distance of every hit pixel's point to the nearest of the scene's surfaces, and which surface that is: 0 table plane, 1 cube
    box, 2 a visible sphere, 3 a drawn capsule.  Geometry only -- link frames from the oracle's FK, the cube's pose from the state;
    no ray is cast."""
    from oracle.oracle import Oracle
    d = dev.cm.desc
    nl = d.nlink
    ci = KM_CAM_INDEX[cam]
    orc = Oracle(dev.cm, 1)
    worst, seen, count = 0.0, set(), 0
    for e in range(pts.shape[0]):
        hit = depth[e] < np.float32(d.cam_zfar)
        p = pts[e][hit].astype(np.float64)
        xpos, xquat, _, _ = orc.fk(qpos[e])
        xmat = [_q2m(xquat[i]) for i in range(nl)]
        dist = [np.abs(p[:, 2] - d.table_z)]
        cq = qpos[e][nl + 3:nl + 7] / np.linalg.norm(qpos[e][nl + 3:nl + 7])
        loc = np.abs((p - qpos[e][nl:nl + 3]) @ _q2m(cq)) - np.array(list(d.cube_half))
        dist.append(np.abs(np.linalg.norm(np.maximum(loc, 0.0), axis=1) + np.minimum(loc.max(axis=1), 0.0)))
        sph = np.full(len(p), np.inf)
        for s in range(d.nsphere):
            if d.sphere_visible[s]:
                c = xpos[d.sphere_link[s]] + xmat[d.sphere_link[s]] @ np.array(list(d.sphere_pos[s]))
                sph = np.minimum(sph, np.abs(np.linalg.norm(p - c, axis=1) - d.sphere_radius[s]))
        dist.append(sph)
        cap = np.full(len(p), np.inf)
        for k in caps:
            if (int(k["cam_mask"]) >> ci) & 1:
                A = xpos[k["link"]] + xmat[k["link"]] @ np.array(k["p0"], dtype=np.float64)
                sv = xmat[k["link"]] @ np.array(k["seg"], dtype=np.float64)
                t = np.clip(((p - A) @ sv) / max(sv @ sv, 1e-300), 0.0, 1.0)
                cap = np.minimum(cap, np.abs(np.linalg.norm(p - A - t[:, None] * sv, axis=1) - k["radius"]))
        dist.append(cap)
        dist = np.stack(dist)
        tol = 2e-6 + np.spacing(np.abs(pts[e][hit]).max(axis=1))                 # one float32 ulp of the coordinates' magnitude
        which = dist.argmin(axis=0)
        worst = max(worst, float((dist.min(axis=0) / tol).max()))
        assert (dist.min(axis=0) <= tol).all(), (cam, e, float(dist.min(axis=0).max()))
        seen |= set(which.tolist())
        count += int(hit.sum())
    return worst, seen, count


@pytest.mark.parametrize("env", ENVS)
def test_points_lie_on_the_scene(env):
    """Independent of the reference's ray cast: world frame, the default list drawn, head and top cameras at 48 x 64, 6 envs.  Every
    pixel with depth < zfar is within 2e-6 m plus one float32 ulp of its coordinates' magnitude of the plane z = table_z, the cube
    box (the cube's pose from get_state), a visible sphere or a drawn capsule; table, cube and capsule each receive a pixel.
    On an MI355X (library 0.33): 1537 to 4597 hit pixels of 18 432 per row, the largest distance 0.019 of that tolerance."""
    torch = _torch()
    dev, qpos = _stepped(env, N, 6, 12)
    caps = M.link_capsules(dev.cm)
    dev.set_render_links(caps)
    dev.set_depth_links(True)
    d = dev.cm.desc
    for cam in ("head", "top"):
        depth = torch.empty((N, 48, 64), dtype=torch.float32, device=dev.device)
        pts = dev.render_points(cam, 48, 64, frame="world", depth_out=depth)
        worst, seen, count = _on_scene(dev, cam, _np(pts), _np(depth), qpos, caps)
        print("on the scene", env, cam, "hit pixels", count, "of", N * 48 * 64, "surfaces", sorted(seen), "largest distance / tolerance", worst)
        assert {0, 1, 3} <= seen, (cam, seen)
        # a pixel without a hit is the point on the far plane (to the float32 of its coordinates)
        far = _np(depth) >= np.float32(d.cam_zfar)
        pose = dev.camera_poses(cam)
        o, z = _np(pose["pos"]), _np(pose["mat"])[:, :, 2]
        for e in range(N):
            on = -((_np(pts)[e][far[e]].astype(np.float64) - o[e]) @ z[e])
            assert (np.abs(on - d.cam_zfar) < 1e-5).all(), (cam, e)
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 4. one launch, one scene
@pytest.mark.parametrize("links", [False, True], ids=["scene", "links"])
def test_one_launch_one_scene(links):
    """KManipTorso, every camera, a COLFIXED and a general shape, with per-env camera offsets.  With depth_out, the camera-frame
    z is -depth_out bit for bit (in both frames' launches the depth is the same image); depth_out agrees with render_depth of the
    same arguments under the depth bar (1e-6 m on fewer than 5e-4 h w n pixels); the world points are pos + mat @ camera points
    (camera_poses) under the point bar.  On an MI355X (library 0.33) depth_out and render_depth were bit-equal on all 268 608
    pixels of the 16 rows, and the world points within 0.21 of the bar of pos + mat @ camera points."""
    torch = _torch()
    dev, qpos, refs = _setup("KManipTorso", "camera_offset")
    if links:
        dev.set_render_links(True)
        dev.set_depth_links(True)
    for cam in _cams(dev.cm):
        ci = KM_CAM_INDEX[cam]
        pose = dev.camera_poses(cam)
        pos, mat = _np(pose["pos"]), _np(pose["mat"])
        for h, w in ((64, 64), (30, 50)):
            what = ("KManipTorso", "links" if links else "scene", cam, h, w)
            dc = torch.empty((N, h, w), dtype=torch.float32, device=dev.device)
            dw = torch.empty_like(dc)
            pc = dev.render_points(cam, h, w, frame="camera", depth_out=dc)
            pw = dev.render_points(cam, h, w, frame="world", depth_out=dw)
            assert torch.equal(pc[..., 2], -dc) and torch.equal(dc, dw), what
            assert torch.equal(pc, dev.render_points(cam, h, w, frame="camera")), what          # (depth_out changes no point)
            plain = dev.render_depth(cam, h, w)
            bad = int((torch.abs(plain - dc) > 1e-6).sum())
            print("depth_out against render_depth", *what, "bit-equal pixels", int((plain == dc).sum()), "of", N * h * w, "off by more than 1e-6 m", bad)
            assert bad < 5e-4 * h * w * N, (what, bad)
            dx, dy = refs[0].rays(ci, h, w)
            ref = pos[:, None, None, :] + np.einsum("nij,nhwj->nhwi", mat, _np(pc).astype(np.float64))
            _point_bar(_np(pw), ref, _np(dc), dx, dy, what + ("world = pos + mat @ camera",))
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 5. opt-in and untouched paths
def test_other_renders_are_untouched_and_links_are_opt_in():
    """render_depth, render_rgb and render_seg images taken before and after render_points / camera_poses calls are equal; with
    the depth flag off (a list set), or the flag on and the list emptied, the points are the no-capsule points byte for byte; with
    both, they differ on head and top, and a capsule only ever brings a pixel nearer."""
    torch = _torch()
    dev, _ = _stepped("KManipTorso", N, 6, 12)
    dev.set_visual_params(camera_offset=_offsets())
    cams = _cams(dev.cm)
    shapes = ((64, 64), (30, 50))

    def images():
        out = {}
        for c in cams:
            for h, w in shapes:
                out[("depth", c, h, w)] = dev.render_depth(c, h, w).clone()
                out[("rgb", c, h, w)] = dev.render_rgb(c, h, w).clone()
                out[("seg", c, h, w)] = dev.render_seg(c, h, w).clone()
        return out

    def points():
        out = {}
        for c in cams:
            for h, w in shapes:
                for f in ("world", "camera"):
                    d = torch.empty((N, h, w), dtype=torch.float32, device=dev.device)
                    out[(c, h, w, f)] = dev.render_points(c, h, w, frame=f, depth_out=d).clone()
                    out[(c, h, w, f, "depth")] = d
            dev.camera_poses(c)
        return out

    def same(a, b):
        return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    before = images()
    first = points()
    assert same(images(), before)
    dev.set_render_links(True)
    with_list = images()
    assert same(points(), first)                                     # a list, the flag off
    assert same(images(), with_list)
    dev.set_depth_links(True)
    drawn = points()
    assert all(not torch.equal(drawn[k], first[k]) for k in first if k[0] in ("head", "top")), "the capsules are not drawn"
    assert all((drawn[k] <= first[k]).all() for k in first if k[-1] == "depth")
    with_flag = images()
    assert all(torch.equal(with_flag[k], with_list[k]) for k in with_list if k[0] != "depth")
    assert all(torch.equal(with_flag[("depth",) + k[:3]], drawn[k]) for k in drawn if k[-1] == "depth" and k[3] == "world")
    dev.set_render_links(None)
    assert same(points(), first)                                     # the flag on, no list
    assert same(images(), before)
    dev.k_close()


def test_physics_is_untouched_by_the_point_renders():
    """Over 70 steps of 128 envs (one auto-reset) obs, reward, done and the state are bit-identical to a plain handle while the
    other handle renders points and reads poses every fifth step."""
    n = 128
    a, b = _make("KManipSoloArm", n, seed=7), _make("KManipSoloArm", n, seed=7)
    b.set_render_links(True)
    b.set_depth_links(True)
    a.k_reset(); b.k_reset()
    for k in range(70):
        a.step_flat(a.sample_action()); b.step_flat(b.sample_action())
        assert a.obs.equal(b.obs) and a.reward.equal(b.reward) and a.done.equal(b.done), k
        if k % 5 == 0:
            b.render_points("head", 30, 50, frame="world")
            b.render_points("grip_r", 64, 64, frame="camera")
            b.camera_poses("grip_r")
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_episode(), b.get_episode())
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------ 6. snapshots and RenderBehind
@pytest.mark.parametrize("vis", ["off", "ranges"])
def test_snapshot_points_and_poses(vis):
    """After snapshot_render_state(0) and six more steps, set_render_source(0) gives the points and the poses taken live at the
    snapshot step, bit for bit -- in visual ranges mode across an auto-reset too (the snapshot keeps its episode's draw)."""
    torch = _torch()
    e = _make("KManipSoloArm", 16, seed=3)
    if vis == "ranges":
        e.set_visual_param_ranges(camera_offset=(-0.06, 0.06))
    e.k_reset()
    e.set_render_links(True)
    e.set_depth_links(True)
    _run(e, 60 if vis == "ranges" else 10)                # (ranges: the six steps below cross the auto-reset at step 64)

    def take():
        out = {}
        for c in _cams(e.cm):
            out[(c, "points")] = e.render_points(c, 48, 64, frame="world").clone()
            out[(c, "camera")] = e.render_points(c, 30, 50, frame="camera").clone()
            out[(c, "pose")] = e.camera_poses(c)["mat"].clone()
            out[(c, "pos")] = e.camera_poses(c)["pos"].clone()
        return out
    live = take()
    e.snapshot_render_state(0)
    _run(e, 6)
    if vis == "ranges":
        assert (e.get_episode() == 1).all()
    moved = take()
    assert any(not torch.equal(moved[k], live[k]) for k in live if k[1] == "points")
    assert any(not torch.equal(moved[k], live[k]) for k in live if k[1] == "pos")
    e.set_render_source(0)
    snap = take()
    e.set_render_source(-1)
    for k in live:
        assert torch.equal(snap[k], live[k]), k
    e.k_close()


@pytest.mark.parametrize("frame", ["world", "camera"])
def test_render_behind_points(frame):
    """RenderBehind(points=("grip_r", 64, 64[, frame]), depth=("grip_r", 64, 64)) over four steps: images(t)["points"] equals the
    live render_points after step t and images(t)["depth"] the depth of that launch; in the camera frame the points' z is -depth
    bit for bit.  A depth of another shape is a render of its own, and points alone carry no depth."""
    torch = _torch()
    from gym_kmanip_amd.pipeline import RenderBehind
    n = 6
    e = _make("KManipSoloArmVision", n, seed=9)
    e.k_reset()
    e.set_render_links(True)
    e.set_depth_links(True)
    _run(e, 10)
    rb = RenderBehind(e, cams=[], points=("grip_r", 64, 64) if frame == "world" else ("grip_r", 64, 64, frame), depth=("grip_r", 64, 64))
    live, ldepth = {}, {}
    for t in range(4):
        e.step_flat(e.sample_action())
        ldepth[t] = torch.empty((n, 64, 64), dtype=torch.float32, device=e.device)
        live[t] = e.render_points("grip_r", 64, 64, frame=frame, depth_out=ldepth[t]).clone()
        assert rb.after_step() == t
        if t:
            imgs = rb.images(t - 1)
            assert sorted(imgs) == ["depth", "points"]
            assert torch.equal(imgs["points"], live[t - 1]), t - 1
            assert torch.equal(imgs["depth"], ldepth[t - 1]), t - 1
            if frame == "camera":
                assert torch.equal(imgs["points"][..., 2], -imgs["depth"]), t - 1
    assert not torch.equal(live[0], live[3])
    rb.synchronize()
    other = RenderBehind(e, cams=[], points=("head", 30, 50), depth=("grip_r", 64, 64))
    other.after_step()
    imgs = other.images(0)
    assert tuple(imgs["points"].shape) == (n, 30, 50, 3) and torch.equal(imgs["depth"], e.render_depth("grip_r", 64, 64))
    assert torch.equal(imgs["points"], e.render_points("head", 30, 50))
    other.synchronize()
    alone = RenderBehind(e, cams=[], points=("head", 30, 50, "camera"))
    alone.after_step()
    assert sorted(alone.images(0)) == ["points"]
    alone.synchronize()
    e.k_close()


# ------------------------------------------------------------------------------------------------ 7. validation
def test_validation():
    """Every error case of the two entry points returns nonzero with the function's name in kmanip_last_error and launches nothing
    (the output buffers keep their fill); the handle is usable afterwards; the Python layer refuses wrong buffers and frames."""
    torch = _torch()
    from gym_kmanip_amd.lib import KManipError
    e = _make("KManipSoloArm", 4, seed=1)                 # (no grip_l camera: index 1 is absent from the model)
    e.k_reset()
    L = e.L
    xyz = torch.full((4, 8, 8, 3), -7.0, dtype=torch.float32, device=e.device)
    dep = torch.full((4, 8, 8), -7.0, dtype=torch.float32, device=e.device)
    pose = torch.full((4, 12), -7.0, dtype=torch.float64, device=e.device)
    px, pd, pp = C.c_void_p(xyz.data_ptr()), C.c_void_p(dep.data_ptr()), C.c_void_p(pose.data_ptr())
    head = KM_CAM_INDEX["head"]
    assert L.kmanip_render_points(None, head, 8, 8, 1, px, pd, None) != 0
    assert b"kmanip_render_points" in L.kmanip_last_error(None)
    assert L.kmanip_get_camera_poses(None, head, pp, None) != 0
    assert b"kmanip_get_camera_poses" in L.kmanip_last_error(None)
    bad_points = [(head, 8, 8, 1, None), (KM_CAM_INDEX["grip_l"], 8, 8, 1, px), (-1, 8, 8, 1, px), (M.KM_MAX_CAMS, 8, 8, 1, px),
                  (head, 0, 8, 1, px), (head, 8, 0, 1, px), (head, -3, 8, 0, px), (head, 8, 8, 2, px), (head, 8, 8, -1, px)]
    for i, (cam, h, w, frame, p) in enumerate(bad_points):
        e.render_depth("grip_r", 8, 8)                    # (a good call in between: the error text is this call's)
        assert L.kmanip_render_points(e.h, cam, h, w, frame, p, pd, None) != 0, i
        assert b"kmanip_render_points" in L.kmanip_last_error(e.h), i
    for i, (cam, p) in enumerate([(head, None), (KM_CAM_INDEX["grip_l"], pp), (-1, pp), (M.KM_MAX_CAMS, pp)]):
        assert L.kmanip_get_camera_poses(e.h, cam, p, None) != 0, i
        assert b"kmanip_get_camera_poses" in L.kmanip_last_error(e.h), i
    torch.cuda.synchronize()
    assert (xyz == -7.0).all() and (dep == -7.0).all() and (pose == -7.0).all()
    with pytest.raises(KManipError):
        e.render_points("head", 8, 8, frame="body")
    with pytest.raises(KManipError):
        e.render_points("grip_l", 8, 8)
    with pytest.raises(KManipError):
        e.render_points("head", 8, 8, out=xyz.double())
    with pytest.raises(KManipError):
        e.render_points("head", 8, 8, depth_out=dep[:, :4])
    with pytest.raises(KManipError):
        e.camera_poses("head", out=pose.float())
    # the handle is usable: a step, and both calls through the raw ABI and the Python layer
    e.step_flat(e.sample_action())
    assert L.kmanip_render_points(e.h, head, 8, 8, 0, px, None, None) == 0 and L.kmanip_get_camera_poses(e.h, head, pp, None) == 0
    torch.cuda.synchronize()
    assert (dep == -7.0).all() and torch.equal(xyz, e.render_points("head", 8, 8, frame="camera"))
    cp = e.camera_poses("head")
    assert torch.equal(pose, torch.cat([cp["pos"], cp["mat"].reshape(4, 9)], dim=1))
    k = e.camera_intrinsics("head", 8, 8)
    assert k == M.camera_intrinsics(e.cm, "head", 8, 8) and k["cx"] == 4.0
    e.k_close()
