"""Link capsules in the depth renders on the device (run with -m gpu on an MI355X): k_render_depth_links through
kmanip_set_depth_links, kmanip_render_depth and kmanip_bind_step_depth, against the float64 reference of
tests/tools/link_depth_oracle.py (pinned to the CPU oracle and to tests/tools/link_oracle.py by tests/test_depth_links_cpu.py),
and the plumbing: opt-in, the step's bound render, snapshots and RenderBehind, agreement with the labels, physics, validation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd import model as M
from gym_kmanip_amd.model import KM_CAM_INDEX
from test_kernel_paths_gpu import _cams, _stepped
from test_render_links_gpu import _Lists

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from link_depth_oracle import LinkDepthOracle  # noqa: E402

pytestmark = pytest.mark.gpu

# COLFIXED (the workgroup's 128 lanes are a whole number of rows): a wave is one row, half a row, two rows
COLFIXED_SHAPES = [(64, 64), (32, 128), (48, 64)]
# general: partial last pass, fewer pixels than the workgroup, wider than the workgroup
GENERAL_SHAPES = [(30, 50), (7, 13), (64, 200)]
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


def _reference(refs, qpos, cam, h, w, caps, envs, what, may_be_empty=False):
    """Reference depth images [len(envs), h, w] and capsule masks of the envs.  The reference must show capsule pixels: an empty
    comparison cannot pass."""
    out = [refs[e].render(qpos[e], KM_CAM_INDEX[cam], h, w, caps) for e in envs]
    depth, mask = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    assert may_be_empty or mask.any(), ("the reference shows no capsule", what)
    return depth, mask


def _depth_bar(dev, img, ref, mask, what):
    """test_kernel_paths_gpu._depth_check's bar, unchanged: |gpu - ref| > 1e-6 m on fewer than 5e-4 h w n pixels (grazing rays), and
    every value within [znear, zfar]."""
    d = dev.cm.desc
    assert img.shape == ref.shape, what
    n, h, w = ref.shape
    bad = int((np.abs(img - ref) > 1e-6).sum())
    print("depth", *what, "capsule pixels", int(mask.sum()), "pixels off by more than 1e-6 m", bad, "of", h * w * n, "cap", 5e-4 * h * w * n,
          "largest difference", float(np.abs(img - ref).max()))
    assert bad < 5e-4 * h * w * n, (what, bad)
    assert (img >= d.cam_znear - 1e-6).all() and (img <= d.cam_zfar + 1e-6).all(), what


def _setup(env, vis, n=N):
    """A stepped handle with the depth flag on (and, vis == "camera_offset", explicit per-env camera offsets: rng(5), +-0.06, as
    test_render_depth_shapes_vs_oracle), its qpos and one reference per env."""
    dev, qpos = _stepped(env, n, 6, 12)
    dev.set_depth_links(True)
    if vis == "off":
        return dev, qpos, [LinkDepthOracle(dev.cm)] * n
    offs = np.random.default_rng(5).uniform(-0.06, 0.06, (n, 3))
    dev.set_visual_params(camera_offset=offs)
    return dev, qpos, [LinkDepthOracle(dev.cm, camera_offset=offs[e]) for e in range(n)]


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("vis", ["off", "camera_offset"])
@pytest.mark.parametrize("env", ENVS)
def test_depth_against_the_reference(env, vis):
    """Every camera, the default list, 6 envs, three COLFIXED and three general shapes, VIS off and with explicit per-env camera
    offsets.  Culling never drops a hit: a capsule whose rectangle (or whose behind-the-camera test) wrongly excluded a pixel
    would show here as a pixel off by the whole capsule, and at 7 x 13 the cap admits no such pixel.  On an MI355X (library 0.32)
    all 84 rows had no pixel off by more than 1e-6 m and a largest difference of 0: the float32 images were equal."""
    dev, qpos, refs = _setup(env, vis)
    caps = M.link_capsules(dev.cm)
    dev.set_render_links(caps)
    for cam in _cams(dev.cm):
        for h, w in COLFIXED_SHAPES + GENERAL_SHAPES:
            what = (env, vis, cam, h, w)
            ref, mask = _reference(refs, qpos, cam, h, w, caps, range(N), what)
            _depth_bar(dev, _np(dev.render_depth(cam, h, w)), ref, mask, what)
    dev.k_close()


def test_head_camera_at_full_size():
    """480 x 640, the head camera's own size, 2 envs of KManipTorso (20 capsules; 100 957 capsule pixels, none off on an MI355X)."""
    dev, qpos, refs = _setup("KManipTorso", "off", n=2)
    caps = M.link_capsules(dev.cm)
    dev.set_render_links(caps)
    what = ("KManipTorso", "off", "head", 480, 640)
    ref, mask = _reference(refs, qpos, "head", 480, 640, caps, range(2), what)
    _depth_bar(dev, _np(dev.render_depth("head", 480, 640)), ref, mask, what)
    dev.k_close()


@pytest.mark.parametrize("env", ENVS)
def test_whole_image_rectangles_and_one_pixel(env):
    """The default list with every capsule's cam_mask = 0xF on the gripper cameras at 64 x 64, 30 x 50 and 1 x 1: the camera link's
    own capsules then pass the camera, with ends behind it and rectangles that cover the whole image (on KManipSoloArm grip_r
    every pixel is a capsule pixel, the 1 x 1 image's included; the Torso's gripper cameras look past their own links, their centre
    ray may meet no capsule, and their 1 x 1 image alone is compared without asking for one).  And 20 x 4, four pixels wide, on
    every camera with the probe capsules of test_render_links_gpu (the default list's capsules lie beside the centre column).
    Culling never drops a hit:
    capsules behind the camera plane, capsules with one end behind it and capsules in front all occur here, under the same bar."""
    dev, qpos, refs = _setup(env, "off")
    unmasked = [dict(c, cam_mask=15) for c in M.link_capsules(dev.cm)]
    dev.set_render_links(unmasked)
    for cam in [c for c in _cams(dev.cm) if c.startswith("grip")]:
        for h, w in ((64, 64), (30, 50), (1, 1)):
            what = (env, "unmasked", cam, h, w)
            ref, mask = _reference(refs, qpos, cam, h, w, unmasked, range(N), what, may_be_empty=env != "KManipSoloArm" and h * w == 1)
            if env == "KManipSoloArm":
                assert mask.all(), what
            _depth_bar(dev, _np(dev.render_depth(cam, h, w)), ref, mask, what)
    narrow = _Lists(dev.cm).narrow
    dev.set_render_links(narrow)
    for cam in _cams(dev.cm):
        what = (env, "narrow", cam, 20, 4)
        ref, mask = _reference(refs, qpos, cam, 20, 4, narrow, range(N), what)
        _depth_bar(dev, _np(dev.render_depth(cam, 20, 4)), ref, mask, what)
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 2. opt-in
@pytest.mark.parametrize("vis", ["off", "camera_offset"])
def test_opt_in(vis):
    """A list with the flag off, and the flag on with the list emptied, give the no-list depth image byte for byte at a COLFIXED and
    a general shape; with the flag on, setting and emptying the list switches the images as the list goes (the flag survives);
    flag and list together differ from the no-list image on head and top."""
    torch = _torch()
    dev, _ = _stepped("KManipTorso", N, 6, 12)
    if vis == "camera_offset":
        dev.set_visual_params(camera_offset=np.random.default_rng(5).uniform(-0.06, 0.06, (N, 3)))
    cams = _cams(dev.cm)

    def renders():
        return {(c, h, w): dev.render_depth(c, h, w).clone() for c in cams for h, w in ((64, 64), (30, 50))}

    def same(a, b):
        return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    first = renders()
    assert dev.get_depth_links() is False
    dev.set_render_links(True)
    assert same(renders(), first)                                    # a list, the flag off
    dev.set_depth_links(True)
    assert dev.get_depth_links() is True
    drawn = renders()
    assert all(not torch.equal(drawn[k], first[k]) for k in first if k[0] in ("head", "top")), "the capsules are not drawn"
    assert all((drawn[k] <= first[k]).all() for k in first)          # a capsule only ever brings a pixel nearer
    for clear in (None, []):
        dev.set_render_links(clear)
        assert dev.get_depth_links() is True and same(renders(), first)     # the flag on, no list
        dev.set_render_links(True)
        assert dev.get_depth_links() is True and same(renders(), drawn)
    dev.set_depth_links(False)
    assert dev.get_depth_links() is False and same(renders(), first)
    assert len(dev.get_render_links()) == 20
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 3. the step's bound render
def test_step_bound_depth():
    """With the flag and a list, the buffer bind_step_depth("grip_r", 64, 64) fills equals a separate render_depth after each of
    eight steps across the auto-reset at step 64, and shows the capsules; a step with cam_mask zeroed on every capsule leaves the
    default image."""
    torch = _torch()
    e = _make("KManipSoloArm", 32, seed=9)
    e.k_reset()
    caps = M.link_capsules(e.cm)
    e.set_render_links(caps)
    e.set_depth_links(True)
    _run(e, 60)
    buf = e.bind_step_depth("grip_r", 64, 64)
    changed = 0
    for t in range(8):                                   # steps 61 .. 68 of the run
        e.step_flat(e.sample_action())
        bound = buf.clone()
        assert torch.equal(bound, e.render_depth("grip_r", 64, 64)), t
        e.set_depth_links(False)
        plain = e.render_depth("grip_r", 64, 64)
        e.set_depth_links(True)
        changed += int((bound != plain).sum())
        assert (bound <= plain).all()
    assert (e.get_episode() == 1).all()
    assert changed > 0, "the bound render does not draw the capsules"
    e.set_render_links([dict(c, cam_mask=0) for c in caps])
    e.step_flat(e.sample_action())
    bound = buf.clone()
    e.set_depth_links(False)
    assert torch.equal(bound, e.render_depth("grip_r", 64, 64))
    e.bind_step_depth(None)
    e.k_close()


# ------------------------------------------------------------------------------------------------ 4. snapshots and RenderBehind
def test_snapshot_depth_with_links():
    """A snapshot's depth with capsules equals the live render taken at that step, after the live state has moved on."""
    torch = _torch()
    e = _make("KManipSoloArm", 16, seed=3)
    e.k_reset()
    e.set_render_links(True)
    e.set_depth_links(True)
    _run(e, 10)
    live = {c: e.render_depth(c, 48, 64).clone() for c in _cams(e.cm)}
    e.snapshot_render_state(0)
    _run(e, 6)
    assert any(not torch.equal(e.render_depth(c, 48, 64), live[c]) for c in live)
    e.set_render_source(0)
    for c in live:
        assert torch.equal(e.render_depth(c, 48, 64), live[c]), c
    e.set_render_source(-1)
    e.k_close()


def test_render_behind_depth_with_links():
    """RenderBehind(env, depth=("grip_r", 64, 64), segmentation=True): the depth of step t holds capsule pixels and agrees with
    the reference at that step's state, under the bar; it equals the live render_depth taken after step t."""
    torch = _torch()
    from gym_kmanip_amd.pipeline import RenderBehind
    n = 6
    e = _make("KManipSoloArmVision", n, seed=9)
    e.k_reset()
    caps = M.link_capsules(e.cm)
    e.set_render_links(caps)
    e.set_depth_links(True)
    _run(e, 10)
    rb = RenderBehind(e, depth=("grip_r", 64, 64), segmentation=True)
    lo = LinkDepthOracle(e.cm)
    live, qpos = {}, {}
    for t in range(4):
        e.step_flat(e.sample_action())
        live[t] = e.render_depth("grip_r", 64, 64).clone()
        qpos[t] = e.get_state()[0]
        assert rb.after_step() == t
        if t:
            imgs = rb.images(t - 1)
            assert "depth" in imgs and "segmentation/head" in imgs
            assert torch.equal(imgs["depth"], live[t - 1]), t - 1
            what = ("RenderBehind", "grip_r", 64, 64, "step", t - 1)
            ref, mask = _reference([lo] * n, qpos[t - 1], "grip_r", 64, 64, caps, range(n), what)
            _depth_bar(e, _np(imgs["depth"]), ref, mask, what)
    rb.synchronize()
    e.k_close()


# ------------------------------------------------------------------------------------------------ 5. depth and labels show one scene
def test_depth_agrees_with_the_labels():
    """Head camera, 68 x 100: the pixels where depth with capsules is nearer than depth without, and the pixels where render_seg
    with the list differs from render_seg without it, differ on fewer than 1e-3 h w n pixels (the label bar of section 14: the
    labels are float32 rays, depth float64).  A capsule pixel in front of a finger sphere of its own arm changes the depth and
    not the label; the head camera sees the fingers from too far for that to matter here.  On an MI355X (library 0.32): 14
    differing pixels on KManipSoloArm and 25 on KManipTorso against the cap of 40.8 (the float64 references alone: 12 and 21)."""
    torch = _torch()
    for env in ENVS:
        dev, _ = _stepped(env, N, 6, 12)
        h, w = 68, 100
        d0, s0 = dev.render_depth("head", h, w).clone(), dev.render_seg("head", h, w).clone()
        dev.set_render_links(True)
        dev.set_depth_links(True)
        d1, s1 = dev.render_depth("head", h, w), dev.render_seg("head", h, w)
        nearer, relabelled = d1 < d0, s1 != s0
        diff = int((nearer != relabelled).sum())
        print("consistency", env, "nearer", int(nearer.sum()), "relabelled", int(relabelled.sum()), "differing", diff, "cap", 1e-3 * h * w * N)
        assert int(nearer.sum()) > 0 and torch.equal(d1 != d0, nearer)
        assert diff < 1e-3 * h * w * N, (env, diff)
        dev.k_close()


# ------------------------------------------------------------------------------------------------ 6. physics
def test_physics_is_untouched_by_depth_links():
    """Over 70 steps (one auto-reset) obs, reward, done and the state are bit-identical with the flag, a list and a bound step
    depth against a plain handle."""
    n = 128
    a, b = _make("KManipSoloArm", n, seed=7), _make("KManipSoloArm", n, seed=7)
    b.set_render_links(True)
    b.set_depth_links(True)
    a.k_reset(); b.k_reset()
    b.bind_step_depth("grip_r", 64, 64)
    for k in range(70):
        a.step_flat(a.sample_action()); b.step_flat(b.sample_action())
        assert a.obs.equal(b.obs) and a.reward.equal(b.reward) and a.done.equal(b.done), k
        if k % 5 == 0:
            b.render_depth("head", 30, 50)
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_episode(), b.get_episode())
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------ 7. validation
def test_validation():
    """kmanip_get_depth_links with a NULL `on` is an error with kmanip_last_error set and leaves the flag alone; a NULL handle is
    rejected by both calls; any nonzero `on` turns the flag on."""
    e = _make("KManipSoloArm", 4, seed=1)
    e.k_reset()
    e.set_depth_links(True)
    assert e.L.kmanip_get_depth_links(e.h, None) != 0
    assert b"kmanip_get_depth_links" in e.L.kmanip_last_error(e.h)
    assert e.get_depth_links() is True
    on = C.c_int(-1)
    assert e.L.kmanip_get_depth_links(None, C.byref(on)) != 0 and on.value == -1
    assert e.L.kmanip_set_depth_links(None, 1) != 0
    assert e.L.kmanip_set_depth_links(e.h, 0) == 0 and e.get_depth_links() is False
    assert e.L.kmanip_set_depth_links(e.h, 7) == 0 and e.get_depth_links() is True
    e.render_depth("grip_r", 64, 64)                     # the flag on, no list: the default kernel
    e.k_close()
