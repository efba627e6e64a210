"""Segmentation labels of the camera renders on the device (run with -m gpu on an MI355X): k_render_labels through
kmanip_render_seg / kmanip_render_labels_multi, env_hip, RenderBehind and the gym shell -- exact against the RGB kernel's own
classification, against the CPU oracle's (tests/tools/label_oracle.py), the arm split, both outputs of one launch, invariance
under colours and lights, env isolation, renders behind the steps, validation and the shell's spaces."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd.model import CAMERAS, KM_CAM_INDEX, KM_SEG_N, KM_SEG_ROBOT_L, KM_SEG_ROBOT_R, sphere_arm
from test_kernel_paths_gpu import RENDER_ENVS, RGB_SHAPES, _cams, _stepped, _vis_values
from test_visual_params_gpu import RANGES

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from label_oracle import FLAT, LabelOracle  # noqa: E402

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def torch_to_np(t):
    return t.cpu().numpy()


def _shapes(cam):
    return RGB_SHAPES + [(CAMERAS[cam].h, CAMERAS[cam].w)]


def _make(env_id, n, seed=0, off=0):
    from gym_kmanip_amd import env_hip
    return env_hip.make(env_id, num_envs=n, seed=seed, env_id_offset=off)


def _run(e, steps):
    for _ in range(steps):
        e.step_flat(e.sample_action())


# ------------------------------------------------------------------------------------------------ 1. exact, against k_render_rgb
@pytest.mark.parametrize("env", RENDER_ENVS)
def test_labels_equal_the_rgb_kernels_classification(env):
    """min(render_seg, 3) equals, byte for byte, channel 0 of render_rgb on a second handle in the same state whose visual
    parameters make the RGB kernel store its material id (ambient 1, no other light, colours k / 255): the same float32 ray maths,
    no pixel exempt.  Every camera, every shape of RGB_SHAPES and the camera's own."""
    torch = _torch()
    a, qa = _stepped(env, 6, 6, 12)
    b, qb = _stepped(env, 6, 6, 12)
    assert np.array_equal(qa, qb)
    b.set_visual_params(**FLAT)
    seen = set()
    for cam in _cams(a.cm):
        for h, w in _shapes(cam):
            seg = a.render_seg(cam, h, w)
            assert seg.shape == (6, h, w) and seg.dtype == torch.uint8 and int(seg.max()) < KM_SEG_N
            mat = b.render_rgb(cam, h, w)
            assert torch.equal(mat[..., 0], mat[..., 1]) and torch.equal(mat[..., 0], mat[..., 2])
            diff = int((torch.clamp(seg, max=3) != mat[..., 0]).sum())
            print("exact", env, cam, h, w, "differing pixels", diff)
            assert diff == 0, (cam, h, w, diff)
            seen |= set(torch.unique(seg).tolist())
    assert {0, 1, 2, 3} <= seen
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------ 2. against the oracle
def _oracle_check(dev, refs, qpos, cam, h, w):
    """The RGB bar as the cap (mismatching pixels, summed over the envs, < 1e-3 h w n) and the floor: every class an env's
    reference image contains is present in that env's GPU image."""
    n = len(refs)
    seg = torch_to_np(dev.render_seg(cam, h, w))
    got = np.minimum(seg, 3)
    bad = 0
    missing = []
    for e, lo in enumerate(refs):
        ref = lo.labels(qpos[e], KM_CAM_INDEX[cam], h, w)
        bad += int((got[e] != ref).sum())
        miss = set(np.unique(ref).tolist()) - set(np.unique(got[e]).tolist())
        if miss:
            missing.append((e, sorted(miss)))
    print("oracle", cam, h, w, "mismatching pixels", bad, "of", h * w * n, "cap", 1e-3 * h * w * n, "missing classes", missing)
    assert bad < 1e-3 * h * w * n, (cam, h, w, bad)
    assert not missing, (cam, h, w, missing)
    return seg


@pytest.mark.parametrize("offsets", [False, True])
@pytest.mark.parametrize("env", RENDER_ENVS)
def test_labels_against_the_oracle(env, offsets):
    """Every camera and shape, 6 envs, against the helper's labels; with explicit per-env camera offsets the reference is the
    helper on model.with_visual_params(cm, camera_offset=o_e)."""
    n = 6
    dev, qpos = _stepped(env, n, 6, 12)
    if offsets:
        offs = np.random.default_rng(5).uniform(-0.05, 0.05, (n, 3))
        dev.set_visual_params(camera_offset=offs)
        refs = [LabelOracle(dev.cm, camera_offset=offs[e]) for e in range(n)]
    else:
        refs = [LabelOracle(dev.cm)] * n
    seen = set()
    for cam in _cams(dev.cm):
        for h, w in _shapes(cam):
            seen |= set(np.unique(_oracle_check(dev, refs, qpos, cam, h, w)).tolist())
    assert {0, 1, 2, 3} <= seen
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 3. arms
@pytest.mark.parametrize("env", ["KManipDualArm", "KManipTorso"])
def test_arm_labels(env):
    """Wherever the label is KM_SEG_ROBOT_R (KM_SEG_ROBOT_L) the helper's right-only (left-only) image says robot, up to the cap
    of the oracle test; both labels occur."""
    n = 6
    dev, qpos = _stepped(env, n, 6, 12)
    assert sorted(set(sphere_arm(dev.cm))) == [0, 1]
    lo = LabelOracle(dev.cm)
    count = {KM_SEG_ROBOT_R: 0, KM_SEG_ROBOT_L: 0}
    for cam in _cams(dev.cm):
        for h, w in [(37, 42), (68, 100), (CAMERAS[cam].h, CAMERAS[cam].w)]:
            seg = torch_to_np(dev.render_seg(cam, h, w))
            for arm, label in ((0, KM_SEG_ROBOT_R), (1, KM_SEG_ROBOT_L)):
                bad = 0
                for e in range(n):
                    ref = lo.arm_labels(qpos[e], KM_CAM_INDEX[cam], h, w, arm)
                    bad += int(((seg[e] == label) & (ref != 3)).sum())
                print("arms", env, cam, h, w, "label", label, "pixels", int((seg == label).sum()), "not the arm's in the reference", bad)
                assert bad < 1e-3 * h * w * n, (cam, h, w, label, bad)
                count[label] += int((seg == label).sum())
    assert count[KM_SEG_ROBOT_R] > 0 and count[KM_SEG_ROBOT_L] > 0, count
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 4. one launch, two outputs
@pytest.mark.parametrize("mode", ["default", "explicit", "ranges"])
def test_one_launch_writes_both_outputs(mode):
    """render_cameras(segmentation=True): the RGB buffers are render_cameras()'s byte for byte, the label buffers render_seg's --
    default kernels, explicit random visual parameters, ranges mode; `out` buffers are filled in place."""
    torch = _torch()
    n = 8
    e = _make("KManipDualArmVision", n, seed=3)
    if mode == "explicit":
        e.set_visual_params(**_vis_values(n, np.random.default_rng(7)))
    elif mode == "ranges":
        e.set_visual_param_ranges(**RANGES)
    e.k_reset(); _run(e, 9)
    plain = {k: v.clone() for k, v in e.render_cameras().items()}
    both = e.render_cameras(segmentation=True)
    names = list(plain)
    assert list(both) == names + ["segmentation/" + k for k in names]
    for k in names:
        assert torch.equal(both[k], plain[k]), (mode, k)
        assert torch.equal(both["segmentation/" + k], e.render_seg(k)), (mode, k)
        assert both["segmentation/" + k].shape == (n, CAMERAS[k].h, CAMERAS[k].w)
    out = {k: torch.full_like(v, 9) for k, v in both.items()}
    got = e.render_cameras(out=out, segmentation=True)
    for k in both:
        assert got[k] is out[k] and torch.equal(out[k], both[k]), (mode, k)
    e.k_close()


@pytest.mark.parametrize("vis", ["off", "explicit"])
def test_multi_job_launch_with_mixed_outputs(vis):
    """kmanip_render_labels_multi, one launch: a per-pixel job with both outputs, a quad job with labels only, a quad job with RGB
    only, a one-quad-wide job with both.  Every buffer lies inside a pre-filled allocation with 64 guard bytes on either side:
    what was asked for equals the single-camera renders, everything else keeps the fill."""
    torch = _torch()
    dev, _ = _stepped("KManipTorso", 6, 6, 12)
    n = dev.num_envs
    if vis == "explicit":
        dev.set_visual_params(**_vis_values(n, np.random.default_rng(7)))
    jobs = [("grip_r", 37, 42, True, True), ("grip_l", 50, 72, False, True), ("top", 68, 100, True, False), ("head", 20, 4, True, True)]
    G = 64

    def guarded(nbytes):
        return torch.full((nbytes + 2 * G,), 7, dtype=torch.uint8, device=dev.device)
    rgb = [guarded(n * h * w * 3) for _, h, w, _, _ in jobs]
    seg = [guarded(n * h * w) for _, h, w, _, _ in jobs]
    m = len(jobs)
    ci = (C.c_int32 * m)(*[KM_CAM_INDEX[j[0]] for j in jobs])
    hh = (C.c_int32 * m)(*[j[1] for j in jobs])
    ww = (C.c_int32 * m)(*[j[2] for j in jobs])
    pr = (C.c_void_p * m)(*[(b.data_ptr() + G) if j[3] else None for j, b in zip(jobs, rgb)])
    ps = (C.c_void_p * m)(*[(b.data_ptr() + G) if j[4] else None for j, b in zip(jobs, seg)])
    dev._check(dev.L.kmanip_render_labels_multi(dev.h, m, ci, hh, ww, pr, ps, dev._stream()), "kmanip_render_labels_multi")
    for (cam, h, w, want_rgb, want_seg), br, bs in zip(jobs, rgb, seg):
        for buf, want, ref in ((br, want_rgb, lambda: dev.render_rgb(cam, h, w)), (bs, want_seg, lambda: dev.render_seg(cam, h, w))):
            assert (buf[:G] == 7).all() and (buf[-G:] == 7).all(), (cam, "guard bytes")
            body = buf[G:-G]
            if want:
                assert torch.equal(body, ref().reshape(-1)), (cam, h, w)
            else:
                assert (body == 7).all(), (cam, "not asked for, yet written")
    # rgb_dev == NULL altogether: labels only
    seg2 = [torch.full((n, h, w), 7, dtype=torch.uint8, device=dev.device) for _, h, w, _, _ in jobs]
    ps2 = (C.c_void_p * m)(*[b.data_ptr() for b in seg2])
    dev._check(dev.L.kmanip_render_labels_multi(dev.h, m, ci, hh, ww, None, ps2, dev._stream()), "kmanip_render_labels_multi")
    for (cam, h, w, _, _), b in zip(jobs, seg2):
        assert torch.equal(b, dev.render_seg(cam, h, w)), cam
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 5. invariance
def test_labels_do_not_depend_on_colours_and_lights():
    """Explicit random colours and lights, and ranges mode across an auto-reset (camera offset pinned at 0), give the labels of a
    handle without visual parameters; a camera offset changes them.  (This is also what holds the VIS labels-only kernel,
    k_render_labels<true, false>, to an exact reference: no test compares it with the flat RGB render directly, but its labels
    equal the default kernel's here, and those equal the RGB kernel's classification in the exact test above.)"""
    torch = _torch()
    n = 16
    a, b = _make("KManipDualArmVision", n, seed=4), _make("KManipDualArmVision", n, seed=4)
    r = dict(RANGES, camera_offset=(0.0, 0.0))
    b.set_visual_param_ranges(**r)
    a.k_reset(); b.k_reset()
    cams = _cams(a.cm)

    def same(what):
        for cam in cams:
            for h, w in ((37, 42), (48, 64)):
                assert torch.equal(a.render_seg(cam, h, w), b.render_seg(cam, h, w)), (what, cam, h, w)
        la, lb = a.render_cameras(segmentation=True), b.render_cameras(segmentation=True)
        for k in la:
            if k.startswith("segmentation/"):
                assert torch.equal(la[k], lb[k]), (what, k)
        return any(not torch.equal(la[k], lb[k]) for k in la if not k.startswith("segmentation/"))
    for steps in (10, 53, 2):                     # steps 10, 63 and 65: before and after the auto-reset at step 64
        _run(a, steps); _run(b, steps)
        assert same(("ranges", steps))            # ... and the RGB images do differ
    assert (b.get_episode() == 1).all()
    v = _vis_values(n, np.random.default_rng(2))
    v["camera_offset"] = np.zeros((n, 3))
    b.set_visual_params(**v)
    assert same("explicit")
    v["camera_offset"] = np.random.default_rng(3).uniform(-0.05, 0.05, (n, 3))
    b.set_visual_params(**v)
    assert not torch.equal(a.render_seg("head"), b.render_seg("head"))
    b.clear_visual_params()
    assert torch.equal(a.render_seg("head"), b.render_seg("head"))
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------ 6. isolation
def test_env_isolation_and_shards():
    """An env's labels do not depend on num_envs or on the other envs: two 32-env shards (env_id_offset) reproduce the slices of
    one 64-env handle, in ranges mode with a drawn camera offset too."""
    torch = _torch()
    for ranges in (False, True):
        w = _make("KManipSoloArmVision", 64, seed=11)
        s0, s1 = _make("KManipSoloArmVision", 32, seed=11), _make("KManipSoloArmVision", 32, seed=11, off=32)
        for x in (w, s0, s1):
            if ranges:
                x.set_visual_param_ranges(**RANGES)
            x.k_reset(); _run(x, 7)
        for cam in _cams(w.cm):
            for h, wd in ((48, 64), (37, 42)):
                iw = w.render_seg(cam, h, wd)
                assert torch.equal(iw[:32], s0.render_seg(cam, h, wd)) and torch.equal(iw[32:], s1.render_seg(cam, h, wd)), (ranges, cam)
        both = w.render_cameras(segmentation=True)
        b0, b1 = s0.render_cameras(segmentation=True), s1.render_cameras(segmentation=True)
        for k in both:
            assert torch.equal(both[k][:32], b0[k]) and torch.equal(both[k][32:], b1[k]), (ranges, k)
        for x in (w, s0, s1):
            x.k_close()


def test_physics_is_untouched_by_label_renders():
    """Over 70 steps (one auto-reset) obs, reward, done and the state are bit-identical whether or not label renders are
    interleaved."""
    n = 128
    a, b = _make("KManipSoloArmVision", n, seed=7), _make("KManipSoloArmVision", n, seed=7)
    a.k_reset(); b.k_reset()
    for k in range(70):
        a.step_flat(a.sample_action()); b.step_flat(b.sample_action())
        assert a.obs.equal(b.obs) and a.reward.equal(b.reward) and a.done.equal(b.done), k
        if k % 3 == 0:
            b.render_cameras(segmentation=True)
        if k % 5 == 0:
            b.render_seg("grip_r", 37, 42)
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_episode(), b.get_episode())
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------ 7. behind the steps
def test_render_behind_with_labels_across_the_reset():
    """RenderBehind(segmentation=True).images(t) equals, entry for entry, what render_cameras(segmentation=True) produced right
    after step t -- through the auto-reset at step 64, in visual ranges mode."""
    torch = _torch()
    from gym_kmanip_amd.pipeline import RenderBehind
    n = 32
    e = _make("KManipSoloArmVision", n, seed=9)
    e.set_visual_param_ranges(**RANGES)
    e.k_reset()
    _run(e, 60)
    rb = RenderBehind(e, segmentation=True)
    live = {}
    for t in range(8):                                   # steps 61 .. 68 of the run
        e.step_flat(e.sample_action())
        live[t] = {k: v.clone() for k, v in e.render_cameras(segmentation=True).items()}
        assert rb.after_step() == t
        if t:
            imgs = rb.images(t - 1)
            assert list(imgs) == list(live[t - 1]) and "segmentation/head" in imgs
            for k in imgs:
                assert torch.equal(imgs[k], live[t - 1][k]), (t - 1, k)
    assert (e.get_episode() == 1).all()
    assert any(not torch.equal(live[2][k], live[5][k]) for k in live[2])
    rb.synchronize()
    e.k_close()


# ------------------------------------------------------------------------------------------------ 8. validation
def test_validation():
    """Both pointers NULL, an absent camera, zero sizes and a wrong `out` buffer are refused; the handle stays usable."""
    torch = _torch()
    from gym_kmanip_amd.lib import KManipError
    e = _make("KManipSoloArmVision", 4, seed=1)
    e.k_reset(); _run(e, 3)
    ref = e.render_seg("head", 48, 64).clone()
    buf = torch.full((4, 48, 64), 7, dtype=torch.uint8, device=e.device)
    one = lambda v: (C.c_int32 * 1)(v)
    L, p = e.L, (C.c_void_p * 1)(buf.data_ptr())
    null1 = (C.c_void_p * 1)(None)
    head, grip_l = KM_CAM_INDEX["head"], KM_CAM_INDEX["grip_l"]
    assert not e.cm.desc.cam_present[grip_l]
    calls = [
        lambda: L.kmanip_render_labels_multi(e.h, 1, one(head), one(48), one(64), None, None, None),
        lambda: L.kmanip_render_labels_multi(e.h, 1, one(head), one(48), one(64), null1, null1, None),
        lambda: L.kmanip_render_labels_multi(e.h, 1, one(head), one(48), one(64), None, null1, None),
        lambda: L.kmanip_render_labels_multi(e.h, 1, one(grip_l), one(48), one(64), None, p, None),
        lambda: L.kmanip_render_labels_multi(e.h, 1, one(7), one(48), one(64), None, p, None),
        lambda: L.kmanip_render_labels_multi(e.h, 1, one(head), one(0), one(64), None, p, None),
        lambda: L.kmanip_render_labels_multi(e.h, 1, one(head), one(48), one(-1), None, p, None),
        lambda: L.kmanip_render_labels_multi(e.h, 0, one(head), one(48), one(64), None, p, None),
        lambda: L.kmanip_render_labels_multi(e.h, 5, one(head), one(48), one(64), None, p, None),
        lambda: L.kmanip_render_seg(e.h, head, 48, 64, None, None),
        lambda: L.kmanip_render_seg(e.h, grip_l, 48, 64, C.c_void_p(buf.data_ptr()), None),
        lambda: L.kmanip_render_seg(e.h, head, 0, 64, C.c_void_p(buf.data_ptr()), None),
    ]
    for i, call in enumerate(calls):
        assert call() != 0, i
        assert len(L.kmanip_last_error(e.h)) > 0
    torch.cuda.synchronize()
    assert (buf == 7).all()
    for bad in (torch.zeros((4, 48, 64), dtype=torch.int32, device=e.device), torch.zeros((4, 48, 65), dtype=torch.uint8, device=e.device),
                torch.zeros((3, 48, 64), dtype=torch.uint8, device=e.device), torch.zeros((4, 48, 64), dtype=torch.uint8),
                torch.zeros((4, 48, 128), dtype=torch.uint8, device=e.device)[:, :, ::2]):
        with pytest.raises(KManipError):
            e.render_seg("head", 48, 64, out=bad)
    with pytest.raises(KManipError):
        e.render_seg("grip_l")
    with pytest.raises(KManipError):
        e.render_cameras(out={"head": None, "grip_r": None, "segmentation/head": torch.zeros((4, 480, 640, 3), dtype=torch.uint8, device=e.device)},
                         segmentation=True)
    assert torch.equal(e.render_seg("head", 48, 64, out=buf), ref) and buf.data_ptr() == e.render_seg("head", 48, 64, out=buf).data_ptr()
    e.k_close()


# ------------------------------------------------------------------------------------------------ 9. shell
def test_shell_observations_carry_labels():
    """KManipEnv(segmentation=True, device_outputs=True): observations after reset and step are inside observation_space (every
    env's row), the label keys follow the camera keys and equal render_seg; with the flag off the keys are today's."""
    torch = _torch()
    from gym_kmanip_amd.gym_shell import KManipEnv, spaces_for
    n = 3
    env = KManipEnv("KManipSoloArmVision", num_envs=n, seed=2, segmentation=True, device_outputs=True)
    keys = list(env.observation_space.spaces)
    assert keys[-2:] == ["segmentation/head", "segmentation/grip_r"] and keys[-4:-2] == ["camera/head", "camera/grip_r"]
    assert env.info["obs_list"][-2:] == ["segmentation/head", "segmentation/grip_r"]

    def member(obs):
        assert list(obs) == keys
        for k, sp in env.observation_space.spaces.items():
            assert obs[k].is_cuda
            v = obs[k].cpu().numpy()
            for i in range(n):
                assert sp.contains(v[i]), (k, v[i].shape, v[i].dtype, v[i].min(), v[i].max())
    obs, _ = env.reset(seed=2)
    member(obs)
    env.action_space.seed(3)
    for _ in range(3):
        a = env.action_space.sample()
        obs, r, term, trunc, info = env.step({k: torch.from_numpy(np.repeat(v[None], n, axis=0)).cuda() for k, v in a.items()})
        member(obs)
    assert torch.equal(obs["segmentation/head"], env.env.render_seg("head"))
    assert torch.equal(obs["camera/head"], env.env.render_rgb("head"))
    assert len(torch.unique(obs["segmentation/head"])) >= 3
    env.close()
    off = KManipEnv("KManipSoloArmVision", num_envs=n, seed=2, device_outputs=True)
    o, _ = off.reset(seed=2)
    assert list(o) == list(spaces_for("KManipSoloArmVision")["observation"]) == keys[:-2]
    assert off.info["obs_list"] == list(off.env.cm.spec.obs_list)
    off.close()


def test_label_render_is_the_timed_steps_render_leg():
    """kmanip_enable_timing: the label render that follows a timed step is that step's render leg, as kmanip_render_rgb_multi is;
    a render of a snapshot is not."""
    e = _make("KManipSoloArmVision", 256, seed=1)
    e.k_reset()
    e.enable_timing(True)
    for _ in range(4):
        e.step_flat(e.sample_action())
        e.render_cameras(segmentation=True)
    _, dyn, rend, nsteps = e.timing_summary()
    assert nsteps == 4 and dyn > 0 and rend > 0, (dyn, rend, nsteps)
    for _ in range(3):
        e.step_flat(e.sample_action())
        e.snapshot_render_state(0)
        e.set_render_source(0)
        e.render_seg("head")
        e.set_render_source(-1)
    _, dyn, rend, nsteps = e.timing_summary()
    assert nsteps == 3 and dyn > 0 and rend == 0, (dyn, rend, nsteps)
    e.enable_timing(False)
    e.k_close()
