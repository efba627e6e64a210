"""Per-env visual parameters of the camera renders on the device (run with -m gpu on an MI355X): kmanip_set_visual_params /
_get_ / _ranges through env_hip -- identity with the default kernels, untouched physics, the camera offset against the CPU
oracle of model.with_visual_params, colours and lights, env isolation, ranges mode against model.draw_visual_params, renders
behind the steps across an auto-reset, validation and checkpoints."""
import ctypes as C

import numpy as np
import pytest

from gym_kmanip_amd.model import (ENV_SPECS, KM_CAM_INDEX, VISUAL_PARAMS, draw_visual_params,
                                  visual_param_defaults, visual_param_vector, with_visual_params)

pytestmark = pytest.mark.gpu

RANGES = {"cube_rgb": (0.3, 1.0), "table_rgb": (0.05, 0.6), "robot_rgb": (0.3, 0.9), "background_rgb": (0.0, 0.4),
          "ambient": (0.2, 0.6), "headlight": (0.2, 0.6), "directional": (0.5, 1.5), "camera_offset": (-0.03, 0.03)}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _make(env_id, n, seed=0, off=0):
    from gym_kmanip_amd import env_hip
    return env_hip.make(env_id, num_envs=n, seed=seed, env_id_offset=off)


def _cams(e):
    return [name for name, ci in KM_CAM_INDEX.items() if e.cm.desc.cam_present[ci]]


def _run(e, steps):
    for _ in range(steps):
        e.step_flat(e.sample_action())


def _random_values(n, rng, offset=0.05):
    return {"cube_rgb": rng.uniform(0, 1, (n, 3)), "table_rgb": rng.uniform(0, 1, (n, 3)), "robot_rgb": rng.uniform(0, 1, (n, 3)),
            "background_rgb": rng.uniform(0, 1, (n, 3)), "ambient": rng.uniform(0.1, 0.6, n), "headlight": rng.uniform(0, 0.8, n),
            "directional": rng.uniform(0, 1.5, n), "camera_offset": rng.uniform(-offset, offset, (n, 3))}


def _all_renders(e):
    """Every present camera: single-camera RGB at the reference size and at an odd width (the per-pixel path), the one-launch
    camera set, and depth on both depth kernels (64 x 64: a whole number of rows per workgroup; 30 x 50: not)."""
    out = {}
    for cam in _cams(e):
        out["rgb/" + cam] = e.render_rgb(cam).clone()
        out["rgb_odd/" + cam] = e.render_rgb(cam, 37, 42).clone()
        out["depth64/" + cam] = e.render_depth(cam, 64, 64).clone()
        out["depth_odd/" + cam] = e.render_depth(cam, 30, 50).clone()
    for cam, img in e.render_cameras(_cams(e)).items():
        out["multi/" + cam] = img.clone()
    return out


def _equal(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert _torch().equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("env_id", list(ENV_SPECS))
def test_identity_with_the_default_values(env_id):
    """Every env set to the defaults renders, byte for byte, what a handle without visual parameters renders: every camera of
    the id, single / multi / depth launches; clear_visual_params() then runs the default kernels again."""
    n = 12
    a, b = _make(env_id, n, seed=2, off=5), _make(env_id, n, seed=2, off=5)
    b.set_visual_params(**visual_param_defaults())
    a.k_reset(); b.k_reset()
    _run(a, 9); _run(b, 9)
    _equal(_all_renders(a), _all_renders(b), env_id)
    b.clear_visual_params()
    _run(a, 2); _run(b, 2)
    _equal(_all_renders(a), _all_renders(b), (env_id, "cleared"))
    a.k_close(); b.k_close()


def test_identity_of_the_step_bound_depth_across_a_reset():
    """Ranges pinned at the defaults (lo == hi) draw exactly the defaults: the depth kmanip_bind_step_depth renders after every
    step of a 70-step run (one auto-reset) is byte-identical to a handle without visual parameters."""
    torch = _torch()
    n = 64
    a, b = _make("KManipSoloArm", n, seed=4), _make("KManipSoloArm", n, seed=4)
    b.set_visual_param_ranges(**{k: (v, v) for k, v in visual_param_defaults().items()})
    da, db = a.bind_step_depth("grip_r", 64, 64), b.bind_step_depth("grip_r", 64, 64)
    a.k_reset(); b.k_reset()
    for k in range(70):
        a.step_flat(a.sample_action()); b.step_flat(b.sample_action())
        assert torch.equal(da, db), k
    assert (a.get_episode() == 1).all()
    p = b.get_visual_params()
    for name, v in visual_param_defaults().items():
        assert (p[name].cpu().numpy() == np.asarray(v)).all(), name
    a.k_close(); b.k_close()


def test_physics_is_untouched():
    """Over 130 steps (two auto-resets) with visual ranges on and renders in between, obs, reward, done and the state are
    bit-identical to a handle without visual parameters."""
    torch = _torch()
    n = 128
    a, b = _make("KManipSoloArmVision", n, seed=7), _make("KManipSoloArmVision", n, seed=7)
    b.set_visual_param_ranges(**RANGES)
    b.bind_step_depth("grip_r", 64, 64)
    a.k_reset(); b.k_reset()
    for k in range(130):
        a.step_flat(a.sample_action()); b.step_flat(b.sample_action())
        assert a.obs.equal(b.obs) and a.reward.equal(b.reward) and a.done.equal(b.done), k
        if k % 10 == 0:
            b.render_cameras()
        if k % 32 == 0 or k == 129:
            for x, y in zip(a.get_state(), b.get_state()):
                assert np.array_equal(x, y), k
    assert np.array_equal(a.get_episode(), b.get_episode())
    a.k_close(); b.k_close()


def _oracle_state(env_id, n, seed, steps):
    torch = _torch()
    from oracle.oracle import Oracle
    dev = _make(env_id, n, seed=seed)
    orc = Oracle(dev.cm, n, seed=seed)
    dev.k_reset(); orc.reset()
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        act = rng.uniform(-1, 1, (n, dev.cm.act_dim)).astype(np.float32)
        dev.step_flat(torch.from_numpy(act).cuda()); orc.step(act)
    return dev, orc.get_state()[0]


def test_camera_offset_rgb_against_the_oracle():
    """Each of 6 envs gets its own camera offset: its images equal the oracle's renders of with_visual_params(cm,
    camera_offset=o_e) on the same state up to one grey level (silhouette-grazing rays: < 0.1 % of the pixels), at 40 x 60 for
    every camera and at 480 x 640 for the head camera."""
    from oracle.oracle import Oracle
    n = 6
    dev, qpos = _oracle_state("KManipSoloArmVision", n, 4, 14)
    offs = np.random.default_rng(1).uniform(-0.08, 0.08, (n, 3))
    dev.set_visual_params(camera_offset=offs)
    orcs = [Oracle(with_visual_params(dev.cm, camera_offset=offs[e]), 1, seed=4) for e in range(n)]
    base = Oracle(dev.cm, 1, seed=4)
    moved = 0
    for cam in _cams(dev):
        sizes = [(40, 60)] + ([(480, 640)] if cam == "head" else [])
        for h, w in sizes:
            img = dev.render_rgb(cam, h, w).cpu().numpy()
            for e in range(n):
                ref = orcs[e].render_rgb(qpos[e], KM_CAM_INDEX[cam], h, w)
                diff = np.abs(img[e].astype(int) - ref.astype(int)).max(axis=-1)
                assert (diff > 1).mean() < 1e-3, (cam, h, e, int((diff > 1).sum()))
                moved += int(not np.array_equal(ref, base.render_rgb(qpos[e], KM_CAM_INDEX[cam], h, w)))
    assert moved > 0                                       # the offsets do move the cameras
    dev.k_close()


def test_camera_offset_depth_against_the_oracle():
    """Depth with per-env camera offsets: the bar of test_render_depth_parity (1e-6 m except < 0.05 % grazing rays), on the
    gripper camera and a world-fixed one, and the step-bound depth uses the offsets too."""
    torch = _torch()
    from oracle.oracle import Oracle
    n = 6
    dev, qpos = _oracle_state("KManipSoloArmVision", n, 4, 14)
    offs = np.random.default_rng(2).uniform(-0.1, 0.1, (n, 3))
    dev.set_visual_params(camera_offset=offs)
    for cam in ("grip_r", "top"):
        img = dev.render_depth(cam, 64, 64).cpu().numpy()
        for e in range(n):
            ref = Oracle(with_visual_params(dev.cm, camera_offset=offs[e]), 1, seed=4).render_depth(qpos[e], KM_CAM_INDEX[cam], 64, 64)
            bad = np.abs(img[e] - ref) > 1e-6
            assert bad.mean() < 5e-4, (cam, e, int(bad.sum()))
    buf = dev.bind_step_depth("grip_r", 64, 64)
    dev.step_flat(dev.sample_action())
    assert torch.equal(buf, dev.render_depth("grip_r", 64, 64))
    dev.k_close()


def _classes(dev, cam, h, w):
    """Material of every pixel from a render with cube red, table green, robot blue and a black background: 0 background,
    1 table, 2 cube, 3 robot."""
    dev.set_visual_params(cube_rgb=(1, 0, 0), table_rgb=(0, 1, 0), robot_rgb=(0, 0, 1), background_rgb=(0, 0, 0))
    img = dev.render_rgb(cam, h, w).cpu().numpy().astype(int)
    cls = np.zeros(img.shape[:3], dtype=int)
    cls[img[..., 1] > 0] = 1; cls[img[..., 0] > 0] = 2; cls[img[..., 2] > 0] = 3
    assert ((img > 0).sum(-1) <= 1).all()
    return cls


def test_colours():
    """A pixel of material m is rgb_m * (the pixel of an all-white render) within one level; a background pixel is exactly
    round(255 bg)."""
    n = 8
    dev, _ = _oracle_state("KManipSoloArmVision", n, 5, 10)
    rng = np.random.default_rng(3)
    for cam, (h, w) in (("head", (120, 160)), ("grip_r", (40, 60)), ("top", (96, 128))):
        cls = _classes(dev, cam, h, w)
        dev.set_visual_params(cube_rgb=(1, 1, 1), table_rgb=(1, 1, 1), robot_rgb=(1, 1, 1))
        white = dev.render_rgb(cam, h, w).cpu().numpy().astype(float)
        assert (white[..., 0] == white[..., 1]).all() and (white[..., 0] == white[..., 2]).all()
        v = _random_values(n, rng)
        v["camera_offset"] = np.zeros((n, 3))
        v.update(ambient=np.full(n, 0.4), headlight=np.full(n, 0.4), directional=np.full(n, 1.0))
        dev.set_visual_params(**v)
        img = dev.render_rgb(cam, h, w).cpu().numpy().astype(float)
        for e in range(n):
            for m, name in ((1, "table_rgb"), (2, "cube_rgb"), (3, "robot_rgb")):
                sel = cls[e] == m
                if sel.any():
                    exp = white[e][sel] * v[name][e][None, :]
                    assert np.abs(img[e][sel] - exp).max() <= 1.001, (cam, e, name)
            bg = np.floor(255 * v["background_rgb"][e] + 0.5)
            assert (img[e][cls[e] == 0] == bg[None, :]).all(), (cam, e)
        if cam == "head":
            assert (cls == 2).any() and (cls == 1).any() and (cls == 0).any()
    dev.k_close()


def test_lights():
    """Ambient only (headlight 0, directional 0): every object pixel of a white render is round(255 a) +- 1; raising the
    ambient by delta (other lights at their defaults) raises every unsaturated object pixel by 255 delta +- 1."""
    n = 8
    dev, _ = _oracle_state("KManipSoloArmVision", n, 6, 10)
    white = dict(cube_rgb=(1, 1, 1), table_rgb=(1, 1, 1), robot_rgb=(1, 1, 1))
    a = np.linspace(0.1, 0.8, n)
    for cam, (h, w) in (("head", (120, 160)), ("grip_r", (40, 60))):
        cls = _classes(dev, cam, h, w)
        dev.set_visual_params(ambient=a, headlight=0.0, directional=0.0, **white)
        img = dev.render_rgb(cam, h, w).cpu().numpy().astype(int)
        for e in range(n):
            obj = img[e][cls[e] > 0]
            assert obj.size and (np.abs(obj - np.floor(255 * a[e] + 0.5)) <= 1).all(), (cam, e)
        d = 0.1
        dev.set_visual_params(ambient=a * 0.5, **white)
        lo = dev.render_rgb(cam, h, w).cpu().numpy().astype(int)
        dev.set_visual_params(ambient=a * 0.5 + d, **white)
        hi = dev.render_rgb(cam, h, w).cpu().numpy().astype(int)
        sel = (cls > 0) & (hi[..., 0] < 255)
        assert sel.any()
        assert (np.abs((hi - lo)[sel] - 255 * d) <= 1).all(), cam
    dev.k_close()


def test_isolation_and_launch_shapes():
    """Half the envs get non-default values: the other half stays byte-identical to the default kernel's images, on every
    launch shape.  With every env in one state, permuting the parameter rows permutes the images."""
    torch = _torch()
    n = 16
    e = _make("KManipDualArmVision", n, seed=3)
    e.k_reset(); _run(e, 6)
    ref = _all_renders(e)
    rng = np.random.default_rng(4)
    v = _random_values(n, rng)
    d = visual_param_defaults()
    half = np.arange(n) % 2 == 1
    for k, (i, m) in VISUAL_PARAMS.items():
        base = np.broadcast_to(np.asarray(d[k], dtype=float), v[k].shape).copy()
        v[k] = np.where(half[:, None] if m == 3 else half, base, v[k])
    e.set_visual_params(**v)
    got = _all_renders(e)
    for k in ref:
        assert torch.equal(got[k][half], ref[k][half]), k
        assert not torch.equal(got[k][~half], ref[k][~half]), k
    # one state for all envs: permuted rows give permuted images
    st = e.get_state()
    e.set_state(*[np.repeat(x[:1], n, axis=0) for x in st])
    v = _random_values(n, rng)
    e.set_visual_params(**v)
    r1 = _all_renders(e)
    perm = rng.permutation(n)
    e.set_visual_params(**{k: x[perm] for k, x in v.items()})
    r2 = _all_renders(e)
    for k in r1:
        assert torch.equal(r2[k], r1[k][torch.as_tensor(perm, device=r1[k].device)]), k
    e.k_close()


def _ranges_vectors():
    lo, hi = visual_param_vector({}), visual_param_vector({})
    for name, (k, m) in VISUAL_PARAMS.items():
        lo[k:k + m], hi[k:k + m] = RANGES[name]
    return lo, hi


def test_ranges_mode():
    """get_visual_params equals draw_visual_params bit for bit for every env; the values are constant within an episode and
    change across the auto-reset; two shards (env_id_offset) agree with one wide handle."""
    n, seed = 64, 11
    lo, hi = _ranges_vectors()
    e = _make("KManipSoloArmVision", n, seed=seed, off=100)
    e.set_visual_param_ranges(**RANGES)

    def check():
        got = e._get_visual_raw().cpu().numpy()
        ep = e.get_episode()
        for j in range(n):
            assert np.array_equal(got[:, j], draw_visual_params(seed, 100 + j, int(ep[j]), lo, hi)), j
        return got
    e.k_reset()
    p0 = check()
    assert (p0 >= lo[:, None]).all() and (p0 <= hi[:, None]).all()
    _run(e, 20)
    assert np.array_equal(check(), p0)                          # constant within the episode
    _run(e, 44)                                                 # step 64: the auto-reset
    assert (e.get_episode() == 1).all()
    p1 = check()
    assert (p1 != p0).all(axis=0).any()
    # shards
    w = _make("KManipSoloArmVision", 64, seed=seed)
    s0, s1 = _make("KManipSoloArmVision", 32, seed=seed), _make("KManipSoloArmVision", 32, seed=seed, off=32)
    for x in (w, s0, s1):
        x.set_visual_param_ranges(**RANGES)
        x.k_reset()
    pw, p_0, p_1 = (x._get_visual_raw().cpu().numpy() for x in (w, s0, s1))
    assert np.array_equal(pw[:, :32], p_0) and np.array_equal(pw[:, 32:], p_1)
    for cam in _cams(w):
        iw = w.render_rgb(cam, 48, 64)
        assert _torch().equal(iw[:32], s0.render_rgb(cam, 48, 64)) and _torch().equal(iw[32:], s1.render_rgb(cam, 48, 64)), cam
    for x in (e, w, s0, s1):
        x.k_close()


def test_render_behind_across_the_reset():
    """Ranges mode: a render of a snapshot taken on the last step of an episode equals the live render of that step byte for
    byte, although the next step auto-resets every env (a new episode, new colours) before the snapshot is rendered."""
    torch = _torch()
    n = 32
    e = _make("KManipSoloArmVision", n, seed=9)
    e.set_visual_param_ranges(**RANGES)
    e.k_reset()
    _run(e, 63)
    live = {k: v.clone() for k, v in e.render_cameras().items()}
    depth = e.render_depth("grip_r", 64, 64).clone()
    e.snapshot_render_state(0)
    ep0 = e.get_episode()
    e.step_flat(e.sample_action())
    assert (e.get_episode() == ep0 + 1).all()
    e.set_render_source(0)
    try:
        snap = e.render_cameras()
        snap_depth = e.render_depth("grip_r", 64, 64)
    finally:
        e.set_render_source(-1)
    for k in live:
        assert torch.equal(snap[k], live[k]), k
    assert torch.equal(snap_depth, depth)
    now = e.render_cameras()
    assert any(not torch.equal(now[k], live[k]) for k in live)
    e.k_close()


def test_validation():
    """Every bad input to each of the three calls raises (in Python before the library; in the library itself for the raw
    calls) and leaves the values in force unchanged."""
    torch = _torch()
    from gym_kmanip_amd.lib import KManipError
    n = 8
    e = _make("KManipSoloArmVision", n, seed=1)
    rng = np.random.default_rng(0)
    v = _random_values(n, rng)
    e.set_visual_params(**v)
    before = e._get_visual_raw().clone()
    bad = [("cube_rgb", 1.1), ("table_rgb", -0.1), ("robot_rgb", float("nan")), ("background_rgb", 2.0), ("ambient", -0.1),
           ("headlight", float("inf")), ("directional", float("nan")), ("camera_offset", 0.3), ("camera_offset", -0.26)]
    for name, x in bad:
        k, m = VISUAL_PARAMS[name]
        with pytest.raises(ValueError):
            e.set_visual_params(**{name: (x,) * m if m == 3 else x})
        with pytest.raises(ValueError):
            e.set_visual_param_ranges(**{name: (x, x)})
        raw = before.clone()
        raw[k, 3] = x
        assert e.L.kmanip_set_visual_params(e.h, C.c_void_p(raw.data_ptr()), None) != 0, name
        lo, hi = visual_param_vector({}), visual_param_vector({})
        lo[k] = hi[k] = x
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert e.L.kmanip_set_visual_param_ranges(e.h, ptr(lo), ptr(hi)) != 0, name
        assert torch.equal(e._get_visual_raw(), before), name
    with pytest.raises(ValueError):
        e.set_visual_params(cube_rgb=np.zeros((n + 1, 3)))
    with pytest.raises(ValueError):
        e.set_visual_params(ambient=np.zeros((n, 3)))
    with pytest.raises(ValueError):
        e.set_visual_params(shininess=1.0)
    with pytest.raises(ValueError):
        e.set_visual_param_ranges(ambient=(0.5, 0.4))
    lo, hi = visual_param_vector({}), visual_param_vector({})
    lo[12], hi[12] = 0.5, 0.4
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert e.L.kmanip_set_visual_param_ranges(e.h, ptr(lo), ptr(hi)) != 0
    assert e.L.kmanip_set_visual_param_ranges(e.h, ptr(lo), None) != 0
    with pytest.raises(KManipError):
        e._check(e.L.kmanip_get_visual_params(e.h, None, None), "kmanip_get_visual_params")
    assert torch.equal(e._get_visual_raw(), before)
    e.k_close()


def test_checkpoint_round_trip():
    """checkpoint() / restore() carry explicit visual values and visual ranges: the restored handle reports the same values and
    renders the same images."""
    torch = _torch()
    n = 16
    a, b = _make("KManipSoloArmVision", n, seed=3), _make("KManipSoloArmVision", n, seed=3)
    a.k_reset(); b.k_reset()
    _run(a, 5)
    a.set_visual_params(**_random_values(n, np.random.default_rng(8)))
    b.restore(a.checkpoint())
    assert torch.equal(a._get_visual_raw(), b._get_visual_raw())
    for cam in _cams(a):
        assert torch.equal(a.render_rgb(cam, 48, 64), b.render_rgb(cam, 48, 64)), cam
    a.set_visual_param_ranges(**RANGES)
    _run(a, 70)
    ck = a.checkpoint()
    assert ck[7][0] is None and ck[7][1] is not None
    b.clear_visual_params()
    b.restore(ck)
    assert torch.equal(a._get_visual_raw(), b._get_visual_raw())
    for cam in _cams(a):
        assert torch.equal(a.render_rgb(cam, 48, 64), b.render_rgb(cam, 48, 64)), cam
    b.restore(a.checkpoint()[:7] + (None,))
    assert torch.equal(b._get_visual_raw()[:, 0].cpu(), torch.from_numpy(visual_param_vector({})))
    a.k_close(); b.k_close()
