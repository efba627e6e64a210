"""Link capsules in the RGB and label renders on the device (run with -m gpu on an MI355X): k_render_links through
kmanip_set_render_links and every render entry point, against the float64 reference of tests/tools/link_oracle.py (pinned to the
CPU oracle by tests/test_render_links_cpu.py), and the plumbing: one ray cast for both outputs, off means off, cam_mask,
renders behind the steps, env isolation, timing, the gym shell and validation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd import model as M
from gym_kmanip_amd.model import CAMERAS, KM_CAM_INDEX, KM_SEG_N, KM_SEG_ROBOT_L, KM_SEG_ROBOT_R, visual_param_vector
from test_kernel_paths_gpu import _cams, _stepped, _vis_values

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from label_oracle import FLAT  # noqa: E402
from link_oracle import LinkOracle  # noqa: E402

pytestmark = pytest.mark.gpu

# per-pixel path; quad path with partial tiles; one quad wide; one pixel wide; the gripper cameras' own size
SHAPES = [(37, 42), (68, 100), (20, 4), (9, 1), (40, 60)]
ENVS = ("KManipSoloArm", "KManipTorso")
N = 6


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _np(t):
    return t.cpu().numpy()


def _make(env_id, n, seed=0, off=0):
    from gym_kmanip_amd import env_hip
    return env_hip.make(env_id, num_envs=n, seed=seed, env_id_offset=off)


def _run(e, steps):
    for _ in range(steps):
        e.step_flat(e.sample_action())


def _probes(cm):
    """Capsules that cross the centre column of every camera.  The default list's capsules lie beside it: in an image four
    pixels or one pixel wide no camera sees them, and the comparison would be empty.  Per gripper camera a thin capsule through
    the camera's target point, in the camera link's frame (the image centre in every env); for the world-fixed cameras three
    1.4 m capsules of 0.1 m radius along the axes of the right arm's site link (one of them crosses the plane x = 0 the
    centre column looks along, whatever the link's orientation)."""
    d = cm.desc
    la = M.link_arm(cm)
    out, world = [], 0
    for c in range(M.KM_MAX_CAMS):
        if not d.cam_present[c]:
            continue
        cl = d.cam_link[c]
        if cl < 0:
            world |= 1 << c
            continue
        assert d.cam_target_link[c] == cl
        t = list(d.cam_target_pos[c])
        out.append({"link": cl, "label": KM_SEG_ROBOT_R + la[cl], "cam_mask": 1 << c, "p0": (t[0] - 0.05, t[1], t[2]),
                    "seg": (0.1, 0.0, 0.0), "radius": 0.01})
    for a in range(3):
        p0, seg = [0.0] * 3, [0.0] * 3
        p0[a], seg[a] = -0.7, 1.4
        out.append({"link": d.arm_site_link[0], "label": KM_SEG_ROBOT_R, "cam_mask": world, "p0": tuple(p0), "seg": tuple(seg), "radius": 0.1})
    return out


class _Lists:
    """The capsule list a shape is rendered with: the default list, or for the shapes less than 8 pixels wide its joint-to-joint
    capsules plus _probes (see there).  use(dev, h, w) sets it on the handle and returns (name, list)."""

    def __init__(self, cm):
        self.default = M.link_capsules(cm)
        self.narrow = [c for c in self.default if c["radius"] == 0.03] + _probes(cm)
        assert len(self.narrow) <= M.KM_MAX_LINK_CAPSULES
        self.now = None

    def use(self, dev, h, w):
        name = "narrow" if w < 8 else "default"
        if self.now != (id(dev), name):
            dev.set_render_links(getattr(self, name))
            self.now = (id(dev), name)
        return name, getattr(self, name)


def _setup(env, vis):
    """A stepped handle (with, vis == "explicit", per-env colours, lights and camera offsets), its qpos, the capsule lists, and
    per env (LinkOracle, visual parameter vector or None)."""
    dev, qpos = _stepped(env, N, 6, 12)
    caps = _Lists(dev.cm)
    if vis == "off":
        return dev, qpos, caps, [(LinkOracle(dev.cm), None)] * N
    v = _vis_values(N, np.random.default_rng(7))
    dev.set_visual_params(**v)
    refs = []
    for e in range(N):
        ve = {k: x[e] for k, x in v.items()}
        refs.append((LinkOracle(dev.cm, camera_offset=ve["camera_offset"]), visual_param_vector(ve)))
    return dev, qpos, caps, refs


_REF = {}


def _reference(env, vis, refs, qpos, lists, dev, cam, h, w):
    """Sets the shape's capsule list on the handle and returns the reference images of every env at one camera and shape --
    (rgb [n, h, w, 3], labels [n, h, w], capsule mask [n, h, w]) -- computed once and shared by the RGB and the label tests (the
    states are the same seeded run).  The reference must show capsule pixels: an empty comparison cannot pass."""
    name, caps = lists.use(dev, h, w)
    key = (env, vis, cam, h, w)
    if key not in _REF:
        out = [lo.render(qpos[e], KM_CAM_INDEX[cam], h, w, caps, vv) for e, (lo, vv) in enumerate(refs)]
        _REF[key] = tuple(np.stack([o[k] for o in out]) for k in range(3))
        for a in _REF[key]:
            a.setflags(write=False)
    assert _REF[key][2].any(), ("the reference shows no capsule", name, cam, h, w)
    return _REF[key]


def _rgb_bar(img, ref, what):
    """The project's RGB bar (test_kernel_paths_gpu._rgb_check): fewer than 0.1 % of the pixels of a shape, summed over the envs,
    may differ by more than one grey level in a channel."""
    assert img.shape == ref.shape, what
    n, h, w = ref.shape[:3]
    bad = int((np.abs(img.astype(int) - ref.astype(int)).max(axis=-1) > 1).sum())
    print("rgb", *what, "pixels off by more than one level", bad, "of", h * w * n, "cap", 1e-3 * h * w * n)
    assert bad < 1e-3 * h * w * n, (what, bad)


def _label_bar(seg, ref, what):
    """The project's label bar (test_label_render_gpu._oracle_check): fewer than 1e-3 h w n mismatching pixels, and every class of
    an env's reference image present in its GPU image."""
    assert seg.shape == ref.shape, what
    n, h, w = ref.shape
    bad = int((seg != ref).sum())
    missing = [(e, sorted(set(np.unique(ref[e]).tolist()) - set(np.unique(seg[e]).tolist()))) for e in range(n)]
    missing = [m for m in missing if m[1]]
    print("labels", *what, "mismatching pixels", bad, "of", h * w * n, "cap", 1e-3 * h * w * n, "missing classes", missing)
    assert bad < 1e-3 * h * w * n, (what, bad)
    assert not missing, (what, missing)


# ------------------------------------------------------------------------------------------------ 4. RGB against the reference
@pytest.mark.parametrize("vis", ["off", "explicit"])
@pytest.mark.parametrize("env", ENVS)
def test_rgb_against_the_reference(env, vis):
    """Every camera and shape, 6 envs, VIS off and with explicit per-env colours, lights and camera offsets.  On an MI355X
    (library 0.31) 70 of the 71 rows (the 480 x 640 one included) had no pixel off by more than one grey level and one row
    (KManipSoloArm, explicit, grip_r 40 x 60) had 1, against a cap of 14.4."""
    dev, qpos, caps, refs = _setup(env, vis)
    for cam in _cams(dev.cm):
        for h, w in SHAPES:
            rgb, _, _ = _reference(env, vis, refs, qpos, caps, dev, cam, h, w)
            _rgb_bar(_np(dev.render_rgb(cam, h, w)), rgb, (env, vis, cam, h, w))
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 5. labels against the reference
@pytest.mark.parametrize("vis", ["off", "explicit"])
@pytest.mark.parametrize("env", ENVS)
def test_labels_against_the_reference(env, vis):
    """The same grid for render_seg.  On an MI355X (library 0.31) 70 of the 71 rows had no mismatching pixel and one row
    (KManipSoloArm, explicit, grip_r 40 x 60: the same pixel as in the RGB test) had 1, against a cap of 14.4; the arm test
    found no pixel outside its arm's reference."""
    dev, qpos, caps, refs = _setup(env, vis)
    seen = set()
    for cam in _cams(dev.cm):
        for h, w in SHAPES:
            _, lab, _ = _reference(env, vis, refs, qpos, caps, dev, cam, h, w)
            seg = _np(dev.render_seg(cam, h, w))
            assert int(seg.max()) < KM_SEG_N
            _label_bar(seg, lab, (env, vis, cam, h, w))
            seen |= set(np.unique(seg).tolist())
    assert set(range(4 if env == "KManipSoloArm" else 5)) <= seen, seen
    dev.k_close()


@pytest.mark.parametrize("env", ["KManipDualArm", "KManipTorso"])
def test_arm_labels(env):
    """Both robot labels occur, and wherever the label is KM_SEG_ROBOT_R (KM_SEG_ROBOT_L) the reference rendered with only that
    arm's capsules and spheres says robot, up to the cap of the label bar."""
    dev, qpos = _stepped(env, N, 6, 12)
    lists = _Lists(dev.cm)
    lo = LinkOracle(dev.cm)
    count = {KM_SEG_ROBOT_R: 0, KM_SEG_ROBOT_L: 0}
    for cam in _cams(dev.cm):
        for h, w in SHAPES:
            _, caps = lists.use(dev, h, w)
            seg = _np(dev.render_seg(cam, h, w))
            for arm, label in ((0, KM_SEG_ROBOT_R), (1, KM_SEG_ROBOT_L)):
                ref = np.stack([lo.labels(qpos[e], KM_CAM_INDEX[cam], h, w, caps, arm=arm) for e in range(N)])
                bad = int(((seg == label) & (ref != label)).sum())
                print("arms", env, cam, h, w, "label", label, "pixels", int((seg == label).sum()), "not the arm's in the reference", bad)
                assert bad < 1e-3 * h * w * N, (cam, h, w, label, bad)
                count[label] += int((seg == label).sum())
    assert count[KM_SEG_ROBOT_R] > 0 and count[KM_SEG_ROBOT_L] > 0, count
    dev.k_close()


def test_head_camera_at_full_size():
    """480 x 640, the head camera's own size, 2 envs of KManipTorso (20 capsules): RGB and labels of one launch
    (render_cameras) against the reference, both bars."""
    dev, qpos = _stepped("KManipTorso", 2, 6, 12)
    caps = M.link_capsules(dev.cm)
    dev.set_render_links(caps)
    lo = LinkOracle(dev.cm)
    ref = [lo.render(qpos[e], KM_CAM_INDEX["head"], 480, 640, caps) for e in range(2)]
    assert all(r[2].any() for r in ref)
    got = dev.render_cameras(["head"], segmentation=True)
    _rgb_bar(_np(got["head"]), np.stack([r[0] for r in ref]), ("KManipTorso", "head", 480, 640))
    _label_bar(_np(got["segmentation/head"]), np.stack([r[1] for r in ref]), ("KManipTorso", "head", 480, 640))
    dev.k_close()


# ------------------------------------------------------------------------------------------------ 6. one ray cast
@pytest.mark.parametrize("env", ENVS)
def test_labels_equal_the_rgb_classification(env):
    """With a list set, min(render_seg, 3) equals, byte for byte, channel 0 of render_rgb on a second handle in the same state
    with the same list and the flat visual parameters (the RGB kernel then stores its material id): no pixel exempt.  And
    render_cameras(segmentation=True) equals the single-camera calls."""
    torch = _torch()
    a, qa = _stepped(env, N, 6, 12)
    b, qb = _stepped(env, N, 6, 12)
    assert np.array_equal(qa, qb)
    la, lb = _Lists(a.cm), _Lists(b.cm)
    b.set_visual_params(**FLAT)
    seen = set()
    for cam in _cams(a.cm):
        for h, w in SHAPES + [(CAMERAS[cam].h, CAMERAS[cam].w)]:
            la.use(a, h, w); lb.use(b, h, w)
            seg = a.render_seg(cam, h, w)
            mat = b.render_rgb(cam, h, w)
            assert torch.equal(mat[..., 0], mat[..., 1]) and torch.equal(mat[..., 0], mat[..., 2])
            diff = int((torch.clamp(seg, max=3) != mat[..., 0]).sum())
            print("exact", env, cam, h, w, "differing pixels", diff)
            assert diff == 0, (cam, h, w, diff)
            seen |= set(torch.unique(seg).tolist())
            assert h * w < 64 or bool((seg >= KM_SEG_ROBOT_R).any()), (cam, h, w)
    assert {0, 1, 2, 3} <= seen
    cams = _cams(a.cm)
    both = a.render_cameras(cams, segmentation=True)
    plain = a.render_cameras(cams)
    for cam in cams:
        assert torch.equal(both[cam], a.render_rgb(cam)) and torch.equal(plain[cam], both[cam]), cam
        assert torch.equal(both["segmentation/" + cam], a.render_seg(cam)), cam
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------ 7. off means off
@pytest.mark.parametrize("vis", ["off", "explicit"])
def test_off_means_off(vis):
    """Render RGB, labels and render_cameras; set the list; clear it; render again: the bytes are the first renders'.  While set,
    the images differ from them."""
    torch = _torch()
    dev, _ = _stepped("KManipTorso", N, 6, 12)
    if vis == "explicit":
        dev.set_visual_params(**_vis_values(N, np.random.default_rng(7)))
    cams = _cams(dev.cm)

    def renders():
        out = {}
        for cam in cams:
            for h, w in ((37, 42), (68, 100)):
                out[("rgb", cam, h, w)] = dev.render_rgb(cam, h, w).clone()
                out[("seg", cam, h, w)] = dev.render_seg(cam, h, w).clone()
        for k, v in dev.render_cameras(cams, segmentation=True).items():
            out[("both", k)] = v.clone()
        for k, v in dev.render_cameras(cams).items():
            out[("multi", k)] = v.clone()
        return out
    first = renders()
    assert dev.get_render_links() == []
    dev.set_render_links(True)
    assert len(dev.get_render_links()) == 20
    during = renders()
    assert all(not torch.equal(during[k], first[k]) for k in first if "head" in k or "top" in k), "the capsules are not drawn"
    for clear in (None, False, []):
        dev.set_render_links(clear)
        assert dev.get_render_links() == []
        again = renders()
        assert list(again) == list(first) and all(torch.equal(again[k], first[k]) for k in first)
        dev.set_render_links(True)
    depth = dev.render_depth("grip_r", 30, 50).clone()
    dev.set_render_links(None)
    assert torch.equal(dev.render_depth("grip_r", 30, 50), depth)                # depth never draws capsules
    dev.k_close()


def test_physics_is_untouched_by_link_renders():
    """Over 70 steps (one auto-reset) obs, reward, done and the state are bit-identical whether or not a list is set and renders
    are interleaved."""
    n = 128
    a, b = _make("KManipSoloArmVision", n, seed=7), _make("KManipSoloArmVision", n, seed=7)
    b.set_render_links(True)
    a.k_reset(); b.k_reset()
    for k in range(70):
        a.step_flat(a.sample_action()); b.step_flat(b.sample_action())
        assert a.obs.equal(b.obs) and a.reward.equal(b.reward) and a.done.equal(b.done), k
        if k % 3 == 0:
            b.render_cameras(segmentation=True)
        if k % 5 == 0:
            b.render_seg("grip_r", 37, 42); b.render_rgb("head", 68, 100)
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_episode(), b.get_episode())
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------ 8. plumbing
def test_cam_mask():
    """Clearing one camera's bit on every capsule gives that camera, and only that camera, the no-capsule image."""
    torch = _torch()
    dev, _ = _stepped("KManipTorso", N, 6, 12)
    cams = _cams(dev.cm)
    shapes = ((37, 42), (68, 100))
    none = {(c, s): (dev.render_rgb(c, *s).clone(), dev.render_seg(c, *s).clone()) for c in cams for s in shapes}
    caps = M.link_capsules(dev.cm)
    dev.set_render_links(caps)
    full = {(c, s): (dev.render_rgb(c, *s).clone(), dev.render_seg(c, *s).clone()) for c in cams for s in shapes}
    assert all(not torch.equal(full[k][1], none[k][1]) for k in full)
    for hide in cams:
        dev.set_render_links([dict(c, cam_mask=c["cam_mask"] & ~(1 << KM_CAM_INDEX[hide])) for c in caps])
        for (c, s) in full:
            want = none if c == hide else full
            assert torch.equal(dev.render_rgb(c, *s), want[(c, s)][0]) and torch.equal(dev.render_seg(c, *s), want[(c, s)][1]), (hide, c, s)
    dev.k_close()


def test_a_zero_length_capsule_at_a_finger_sphere_changes_nothing():
    torch = _torch()
    dev, _ = _stepped("KManipSoloArm", N, 6, 12)
    d = dev.cm.desc
    s = next(s for s in range(d.nsphere) if d.sphere_visible[s])
    cap = {"link": d.sphere_link[s], "label": KM_SEG_ROBOT_R, "cam_mask": 15, "p0": tuple(d.sphere_pos[s]), "seg": (0.0, 0.0, 0.0),
           "radius": d.sphere_radius[s]}
    shapes = ((37, 42), (68, 100), (40, 60))
    cams = _cams(dev.cm)
    before = {(c, sh): (dev.render_rgb(c, *sh).clone(), dev.render_seg(c, *sh).clone()) for c in cams for sh in shapes}
    assert any((v[1] == KM_SEG_ROBOT_R).any() for v in before.values())
    dev.set_render_links([cap])
    assert dev.get_render_links() == [cap]
    diff = {}
    for (c, sh), (rgb, seg) in before.items():
        diff[(c, sh)] = (int((dev.render_seg(c, *sh) != seg).sum()), int((dev.render_rgb(c, *sh) != rgb).any(-1).sum()))
    print("zero-length capsule: differing pixels (labels, rgb)", diff)
    assert all(v == (0, 0) for v in diff.values()), diff
    dev.k_close()


def test_render_behind_with_links_across_the_reset():
    """RenderBehind(segmentation=True).images(t) equals the live render_cameras(segmentation=True) after step t, through the
    auto-reset at step 64, with a list set."""
    torch = _torch()
    from gym_kmanip_amd.pipeline import RenderBehind
    n = 32
    e = _make("KManipSoloArmVision", n, seed=9)
    e.set_render_links(True)
    e.k_reset()
    bare = _make("KManipSoloArmVision", n, seed=9)
    bare.k_reset()
    assert not torch.equal(e.render_rgb("head"), bare.render_rgb("head"))
    bare.k_close()
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


def test_env_isolation_and_shards():
    """Two 32-env shards (env_id_offset) reproduce the slices of one 64-env handle, all three with the list set."""
    torch = _torch()
    w = _make("KManipSoloArmVision", 64, seed=11)
    s0, s1 = _make("KManipSoloArmVision", 32, seed=11), _make("KManipSoloArmVision", 32, seed=11, off=32)
    for x in (w, s0, s1):
        x.set_render_links(True)
        x.k_reset(); _run(x, 7)
    for cam in _cams(w.cm):
        for h, wd in ((48, 64), (37, 42)):
            for f in ("render_seg", "render_rgb"):
                iw = getattr(w, f)(cam, h, wd)
                assert torch.equal(iw[:32], getattr(s0, f)(cam, h, wd)) and torch.equal(iw[32:], getattr(s1, f)(cam, h, wd)), (f, cam)
    both = w.render_cameras(segmentation=True)
    b0, b1 = s0.render_cameras(segmentation=True), s1.render_cameras(segmentation=True)
    for k in both:
        assert torch.equal(both[k][:32], b0[k]) and torch.equal(both[k][32:], b1[k]), k
    assert (both["segmentation/head"] >= KM_SEG_ROBOT_R).float().mean() > 0.01
    for x in (w, s0, s1):
        x.k_close()


def test_link_render_is_the_timed_steps_render_leg():
    e = _make("KManipSoloArmVision", 256, seed=1)
    e.set_render_links(True)
    e.k_reset()
    e.enable_timing(True)
    for k in range(4):
        e.step_flat(e.sample_action())
        if k % 2:
            e.render_cameras(segmentation=True)
        else:
            e.render_cameras()
    _, dyn, rend, nsteps = e.timing_summary()
    assert nsteps == 4 and dyn > 0 and rend > 0, (dyn, rend, nsteps)
    for _ in range(3):
        e.step_flat(e.sample_action())
        e.snapshot_render_state(0)
        e.set_render_source(0)
        e.render_rgb("head")
        e.set_render_source(-1)
    _, dyn, rend, nsteps = e.timing_summary()
    assert nsteps == 3 and dyn > 0 and rend == 0, (dyn, rend, nsteps)
    e.enable_timing(False)
    e.k_close()


def test_shell_with_render_links():
    """KManipEnv(render_links=True): the spaces and keys are those of a shell without the flag, the observations lie inside them,
    camera/head equals env.env.render_rgb("head") and differs from the other shell's."""
    torch = _torch()
    from gym_kmanip_amd.gym_shell import KManipEnv
    n = 3
    env = KManipEnv("KManipSoloArmVision", num_envs=n, seed=2, render_links=True, device_outputs=True)
    off = KManipEnv("KManipSoloArmVision", num_envs=n, seed=2, device_outputs=True)
    assert list(env.observation_space.spaces) == list(off.observation_space.spaces)
    for k, sp in off.observation_space.spaces.items():
        mine = env.observation_space.spaces[k]
        assert mine.shape == sp.shape and mine.dtype == sp.dtype and np.array_equal(mine.low, sp.low) and np.array_equal(mine.high, sp.high), k
    assert len(env.env.get_render_links()) == 10 and off.env.get_render_links() == []
    obs, _ = env.reset(seed=2)
    obo, _ = off.reset(seed=2)
    env.action_space.seed(3)
    for _ in range(3):
        a = env.action_space.sample()
        act = {k: torch.from_numpy(np.repeat(v[None], n, axis=0)).cuda() for k, v in a.items()}
        obs = env.step(act)[0]
        obo = off.step(act)[0]
        assert list(obs) == list(env.observation_space.spaces)
        for k, sp in env.observation_space.spaces.items():
            v = obs[k].cpu().numpy()
            for i in range(n):
                assert sp.contains(v[i]), (k, v[i].shape, v[i].dtype)
    assert torch.equal(obs["camera/head"], env.env.render_rgb("head"))
    assert not torch.equal(obs["camera/head"], obo["camera/head"])
    assert torch.equal(obs["q_pos"], obo["q_pos"])
    env.close(); off.close()


# ------------------------------------------------------------------------------------------------ 9. validation
def test_validation():
    """n = 25, a link out of range, label 2, radius 0, a NaN radius, a NaN in seg and n > 0 with a NULL pointer are refused with
    an error text, leave the previous list in force and the handle usable; get_render_links returns what was set."""
    torch = _torch()
    from gym_kmanip_amd.lib import KLinkCapsule, KManipError
    e = _make("KManipSoloArmVision", 4, seed=1)
    e.k_reset(); _run(e, 3)
    caps = M.link_capsules(e.cm)[:7]
    caps[2] = dict(caps[2], p0=(0.01, -0.02, 0.03), radius=0.025)
    e.set_render_links(caps)
    assert e.get_render_links() == caps
    ref_rgb, ref_seg = e.render_rgb("head", 48, 64).clone(), e.render_seg("head", 48, 64).clone()

    def arr(items):
        a = (KLinkCapsule * len(items))()
        for x, c in zip(a, items):
            x.link, x.label, x.cam_mask, x.radius = c["link"], c["label"], c["cam_mask"], c["radius"]
            x.p0[:] = c["p0"]; x.seg[:] = c["seg"]
        return a
    nan = float("nan")
    good = M.link_capsules(e.cm)
    bad_lists = [(25, arr((good * 3)[:25])), (1, arr([dict(good[0], link=10)])), (1, arr([dict(good[0], link=-1)])),
                 (1, arr([dict(good[0], label=2)])), (2, arr([good[0], dict(good[1], radius=0.0)])), (1, arr([dict(good[0], radius=nan)])),
                 (1, arr([dict(good[0], radius=float("inf"))])), (1, arr([dict(good[0], seg=(0.0, nan, 0.0))])),
                 (1, arr([dict(good[0], p0=(nan, 0.0, 0.0))])), (3, None), (-1, arr(good))]
    for i, (n, a) in enumerate(bad_lists):
        assert e.L.kmanip_set_render_links(e.h, n, a) != 0, i
        assert len(e.L.kmanip_last_error(e.h)) > 0, i
        assert e.get_render_links() == caps, i
    assert torch.equal(e.render_rgb("head", 48, 64), ref_rgb) and torch.equal(e.render_seg("head", 48, 64), ref_seg)
    for bad in ([dict(good[0], label=2)], good * 3, [dict(good[0], radius=nan)], [(0, 3, 15, (0, 0, 0), (0, 0, nan), 0.03)]):
        with pytest.raises(KManipError):
            e.set_render_links(bad)
    assert e.get_render_links() == caps
    n = C.c_int(-1)
    assert e.L.kmanip_get_render_links(e.h, C.byref(n), None) == 0 and n.value == 7
    assert e.L.kmanip_get_render_links(e.h, None, None) != 0
    e.set_render_links(good * 2 + good[:4])                                       # 24: the most a handle takes
    assert len(e.get_render_links()) == 24
    e.render_seg("head", 48, 64)
    e.set_render_links(caps)
    assert torch.equal(e.render_rgb("head", 48, 64), ref_rgb) and torch.equal(e.render_seg("head", 48, 64), ref_seg)
    e.k_close()
