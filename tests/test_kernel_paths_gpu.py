"""Every compiled step / reset object and every render path against the float64 CPU oracle (run with -m gpu on an MI355X).

The common paths have their own parity tests (test_gpu_parity, test_env_params_gpu, test_visual_params_gpu).  This module covers
the rest of what the library compiles and the public API reaches:
  - the step matrix: both link classes x both solvers x {no parameters, explicit per-env parameters, ranges mode}, i.e. all eight
    kmanip_dyn objects without an applied force ({class x solver} x {default, KM_VAR_PAR}), one-step samples against the oracle of
    the env's own values;
  - kmanip_step_chunk and the forced envs-per-wave launch shapes (KMANIP_EPB) of every variant, bit for bit against single steps
    and the default shape: the oracle parity above then carries over to them (an env's result does not depend on its wave slot);
  - k_render_depth on both instantiations (COLFIXED: a whole number of rows per 128-lane workgroup; general: any other shape),
    with and without the per-env camera offset;
  - k_render_rgb's per-pixel loop (width % 4 != 0), its quad-tile walk with partial tiles, and the multi-job launch, with and
    without per-env colours, lights and camera offset.
tests/test_kernel_paths_cpu.py keeps STEP_ROWS complete against the kmanip_dyn objects make builds."""
import ctypes as C

import numpy as np
import pytest

from gym_kmanip_amd.model import KM_CAM_INDEX, compile_model, visual_param_vector, with_env_params, with_visual_params
from test_env_params_gpu import _spread

pytestmark = pytest.mark.gpu

TOL_Q = 1e-7
SOLVERS = ("newton", "pgs")
STEP_ENVS = ("KManipSoloArm", "KManipDualArm", "KManipTorso")          # link classes 10 (SoloArm) and 20 (DualArm, Torso)
PARAM_MODES = ("none", "explicit", "ranges")
STEP_ROWS = [(env, solver, mode) for env in STEP_ENVS for solver in SOLVERS for mode in PARAM_MODES]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _hip(cm, n, seed=0, off=0):
    from gym_kmanip_amd import env_hip
    return env_hip.KManipEnvHip(cm, num_envs=n, seed=seed, env_id_offset=off)


def _ranges(cm):
    """Ranges around the model's values; the friction loss range starts at exactly 0."""
    d = cm.desc
    return {"cube_mass": (0.5 * d.cube_mass, 2.0 * d.cube_mass), "cube_friction": (0.3, 1.5),
            "cube_frictionloss": (0.0, 2.0 * d.cube_frictionloss), "kp_scale": (0.5, 1.5)}


def _with_params(dev, mode, cm, n, seed):
    torch = _torch()
    if mode == "explicit":
        P = _spread(cm, n, seed)
        dev.set_env_params(**{k: torch.from_numpy(v) for k, v in P.items()})
        got = dev.get_env_params()
        for k, v in P.items():
            assert np.array_equal(got[k].cpu().numpy(), v)
    elif mode == "ranges":
        dev.set_env_param_ranges(**_ranges(cm))


# ---------------------------------------------------------------------------------------------------------------- step matrix
def _step_parity(env, solver, mode, n, check, steps, seed):
    """test_env_params_gpu._parity with a solver and a parameter mode: at each sample the device state of env e is loaded into an
    oracle of with_env_params(cm, p_e), p_e the values in force for e before the step (mode "none": the model itself); both take
    the same action; contact mask and done byte identical, qpos within TOL_Q, float32 ctrl flips as in _parity.  Returns the
    largest qpos difference seen (outside flips) for the record."""
    torch = _torch()
    from oracle.oracle import Oracle
    cm = compile_model(env, solver=solver)
    off = 5
    dev = _hip(cm, n, seed=seed, off=off)
    _with_params(dev, mode, cm, n, seed)
    dev.k_reset()
    rng = np.random.default_rng(seed)
    saw_contact = saw_done = False
    flips = compared_contact = 0
    worst = 0.0
    redrawn = set()
    for k in range(steps):
        act = rng.uniform(-1, 1, (n, cm.act_dim)).astype(np.float32)
        sample = k % 9 == 8 or k in (63, steps - 1)        # (step 64 of an episode: the auto-reset, in ranges mode a redraw)
        if sample:
            st0, ep0 = dev.get_state(), dev.get_episode()
            p0 = {name: v.cpu().numpy() for name, v in dev.get_env_params().items()} if mode != "none" else None
        dev.step_flat(torch.from_numpy(act).cuda())
        if not sample:
            continue
        st1 = dev.get_state(); mask = dev.get_diag()[0]; done = dev.done.cpu().numpy()
        if mode == "ranges":
            p1 = dev.get_env_params()
            redrawn |= {e for e in check if done[e] and p1["cube_mass"][e].item() != p0["cube_mass"][e]}
        for e in check:
            cme = cm if p0 is None else with_env_params(cm, **{name: v[e] for name, v in p0.items()})
            o = Oracle(cme, 1, seed=seed, env_id_offset=off + e)
            o.set_state(*(x[e:e + 1] for x in st0)); o.set_episode(ep0[e:e + 1])
            _, _, do = o.step(act[e:e + 1])
            so = o.get_state()
            assert np.array_equal(do, done[e:e + 1]), (k, e)
            bad = so[2] != st1[2][e:e + 1]
            if bad.any():
                ulp = np.spacing(np.abs(so[2][bad]).astype(np.float32)).astype(np.float64)
                assert (np.abs(st1[2][e:e + 1][bad] - so[2][bad]) <= ulp).all(), ("ctrl", k, e)
                assert np.abs(so[0] - st1[0][e:e + 1]).max() < 10 * TOL_Q, (k, e)
                flips += 1
                continue
            assert np.array_equal(o.get_diag()[0], mask[e:e + 1]), (k, e)
            err = np.abs(so[0] - st1[0][e:e + 1]).max()
            assert err < TOL_Q, (k, e, err)
            worst = max(worst, float(err))
            saw_contact |= bool(mask[e] & 0xFF); saw_done |= bool(done[e])
            compared_contact += bool(mask[e])
    assert saw_contact and saw_done
    assert flips <= 2, flips
    assert compared_contact >= 10, compared_contact
    if mode == "ranges":
        assert len(redrawn) >= len(check) // 2, len(redrawn)      # the auto-reset drew new values, and the samples after it used them
    dev.k_close()
    print("step parity %s %s %s: max |dqpos| %.3e over %d envs, %d ctrl flips, %d samples with contact"
          % (env, solver, mode, worst, len(check), flips, compared_contact))
    return worst


@pytest.mark.parametrize("env,solver,mode", STEP_ROWS)
def test_step_variant_vs_oracle(env, solver, mode):
    """One-step samples of 52 of 256 envs over 66 steps (every 9th step, the auto-reset at step 64 and the step after it).  PGS
    keeps the Newton bar: on an MI355X the largest qpos difference of every row, PGS and Newton alike, was 4e-15 .. 5e-14
    (PGS 7e-15 .. 4.6e-14), with no ctrl flip in any row."""
    _step_parity(env, solver, mode, 256, list(range(0, 256, 5)), 66, seed=2)


# ---------------------------------------------------------------------------------------------------- chunked / forced EPB
def _rows(h):
    return h.obs.clone(), h.reward.clone(), h.done.clone()


@pytest.mark.parametrize("params", ["none", "ranges"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env", STEP_ENVS)
def test_chunk_and_forced_epb_launches_are_bitwise_equal(env, solver, params, monkeypatch):
    """On a ragged batch (37 envs of the 10-link class, 21 of the 20-link class), over 78 steps with the auto-reset (and in ranges
    mode the redraw) at step 64 inside the fifth chunk of 13:
      step_chunk(13) -- the chunk kernel at the class's widest envs per wave -- equals 13 step_flat calls of the default shape;
      a handle created with KMANIP_EPB = 1, 2 (and 4 for the 10-link class) equals the default handle,
    in obs, reward, done, the full state, the diagnostics, the episode counters and the parameters in force."""
    torch = _torch()
    cm = compile_model(env, solver=solver)
    small = cm.nlink <= 10
    n, epbs = (37, (1, 2, 4)) if small else (21, (1, 2))

    def make(epb=None):
        if epb is None:
            monkeypatch.delenv("KMANIP_EPB", raising=False)
        else:
            monkeypatch.setenv("KMANIP_EPB", str(epb))
        h = _hip(cm, n, seed=6, off=3)
        if params == "ranges":
            h.set_env_param_ranges(**_ranges(cm))
        return h
    forced = {e: make(e) for e in epbs}
    ref, chunk = make(), make()
    hs = [ref, chunk] + list(forced.values())
    for h in hs:
        h.k_reset()
    for e, h in forced.items():
        assert all(x.equal(y) for x, y in zip(_rows(h), _rows(ref))), ("reset", e)
    gen = torch.Generator(device="cuda"); gen.manual_seed(n)
    K, saw_done = 13, False
    for rnd in range(6):
        acts = (torch.rand((K, n, cm.act_dim), generator=gen, device="cuda") * 2 - 1).contiguous()
        obs_c, rew_c, done_c = chunk.step_chunk(acts)
        saw_done |= bool(done_c.any())
        for k in range(K):
            ref.step_flat(acts[k])
            r = _rows(ref)
            assert obs_c[k].equal(r[0]) and rew_c[k].equal(r[1]) and done_c[k].equal(r[2]), ("chunk", rnd, k)
            for e, h in forced.items():
                h.step_flat(acts[k])
                assert all(x.equal(y) for x, y in zip(_rows(h), r)), ("epb", e, rnd, k)
    assert saw_done
    s_ref, d_ref, ep_ref = ref.get_state(), ref.get_diag(), ref.get_episode()
    p_ref = ref.get_env_params()
    assert (ep_ref == 1).all()
    for what, h in [("chunk", chunk)] + [("epb%d" % e, h) for e, h in forced.items()]:
        for x, y in zip(h.get_state(), s_ref):
            assert np.array_equal(x, y), what
        for x, y in zip(h.get_diag(), d_ref):
            assert np.array_equal(x, y), what
        assert np.array_equal(h.get_episode(), ep_ref), what
        assert all(h.get_env_params()[k].equal(v) for k, v in p_ref.items()), what
    for h in hs:
        h.k_close()


# ------------------------------------------------------------------------------------------------------------------ renders
DEPTH_SHAPES = [(64, 64), (32, 128), (48, 64),                               # COLFIXED: 128 % w == 0 and h w % 128 == 0
                (30, 50), (40, 60), (7, 13), (1, 1), (64, 200)]              # general (64 x 200: wider than the workgroup)
# per-pixel loop (w % 4 != 0): 42, 61, 1 wide; quad tiles: 68 x 100 (25 quads: a full and a partial tile column), 20 x 4 (one
# quad a row), 50 x 72 (18 quads: a partial tile column; 50 rows: a partial tile row)
RGB_SHAPES = [(37, 42), (23, 61), (9, 1), (68, 100), (20, 4), (50, 72)]
RENDER_ENVS = ("KManipSoloArm", "KManipTorso")


def _stepped(env, n, seed, steps):
    """A handle after `steps` random steps (the cube has landed) and its own qpos: renders read nothing else of the state."""
    torch = _torch()
    cm = compile_model(env)
    dev = _hip(cm, n, seed=seed)
    dev.k_reset()
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        dev.step_flat(torch.from_numpy(rng.uniform(-1, 1, (n, cm.act_dim)).astype(np.float32)).cuda())
    return dev, dev.get_state()[0]


def _cams(cm):
    return [name for name, ci in KM_CAM_INDEX.items() if cm.desc.cam_present[ci]]


def _depth_check(dev, orcs, qpos, cam, h, w, envs):
    """test_render_depth_parity's bar: 1e-6 m except grazing rays (< 0.05 % of the pixels of the shape, over the envs compared)."""
    d = dev.cm.desc
    img = dev.render_depth(cam, h, w).cpu().numpy()
    assert img.shape == (dev.num_envs, h, w)
    bad = 0
    for e in envs:
        ref = orcs[e].render_depth(qpos[e], KM_CAM_INDEX[cam], h, w)
        bad += int((np.abs(img[e] - ref) > 1e-6).sum())
    assert bad < 5e-4 * h * w * len(envs), (cam, h, w, bad)
    assert (img >= d.cam_znear - 1e-6).all() and (img <= d.cam_zfar + 1e-6).all(), (cam, h, w)
    return img


@pytest.mark.parametrize("vis", ["off", "camera_offset"])
@pytest.mark.parametrize("env", RENDER_ENVS)
def test_render_depth_shapes_vs_oracle(env, vis):
    """Every camera of the model, both k_render_depth instantiations (COLFIXED and general), 6 envs at each shape of DEPTH_SHAPES
    and two at 480 x 640, VIS off and with a per-env camera offset (the oracle of with_visual_params(cm, camera_offset=o_e))."""
    from oracle.oracle import Oracle
    n = 6
    dev, qpos = _stepped(env, n, 4, 14)
    cm = dev.cm
    if vis == "off":
        orcs = [Oracle(cm, 1)] * n
    else:
        offs = np.random.default_rng(5).uniform(-0.06, 0.06, (n, 3))
        dev.set_visual_params(camera_offset=offs)
        orcs = [Oracle(with_visual_params(cm, camera_offset=offs[e]), 1) for e in range(n)]
    for cam in _cams(cm):
        for h, w in DEPTH_SHAPES:
            img = _depth_check(dev, orcs, qpos, cam, h, w, range(n))
            # a real image, not a constant (at 7 x 13 the world-fixed cameras see a few pixels of the scene and the background)
            if h * w >= 64:
                assert np.unique(np.round(img, 3)).size > (10 if h * w >= 1024 else 1), (cam, h, w)
        img = _depth_check(dev, orcs, qpos, cam, 480, 640, (0, 3))
        assert np.unique(np.round(img, 3)).size > 10, cam
    dev.k_close()


def _vis_values(n, rng):
    return {"cube_rgb": rng.uniform(0, 1, (n, 3)), "table_rgb": rng.uniform(0, 1, (n, 3)), "robot_rgb": rng.uniform(0, 1, (n, 3)),
            "background_rgb": rng.uniform(0, 1, (n, 3)), "ambient": rng.uniform(0.1, 0.5, n), "headlight": rng.uniform(0, 0.6, n),
            "directional": rng.uniform(0, 1.2, n), "camera_offset": rng.uniform(-0.05, 0.05, (n, 3))}


def _rgb_setup(env, vis, n=6):
    """A stepped handle and, per env, (oracle, visual parameter vector or None) for Oracle.render_rgb."""
    from oracle.oracle import Oracle
    dev, qpos = _stepped(env, n, 6, 12)
    if vis == "off":
        return dev, qpos, [(Oracle(dev.cm, 1), None)] * n
    v = _vis_values(n, np.random.default_rng(7))
    dev.set_visual_params(**v)
    refs = []
    for e in range(n):
        ve = {k: x[e] for k, x in v.items()}
        refs.append((Oracle(with_visual_params(dev.cm, camera_offset=ve["camera_offset"]), 1), visual_param_vector(ve)))
    return dev, qpos, refs


def _rgb_check(img, refs, qpos, cam, h, w):
    """The existing RGB bar: at most one grey level per channel, except < 0.1 % of the pixels (over the envs)."""
    assert img.shape == (len(refs), h, w, 3)
    bad = 0
    for e, (o, vv) in enumerate(refs):
        ref = o.render_rgb(qpos[e], KM_CAM_INDEX[cam], h, w, vis=vv)
        bad += int((np.abs(img[e].astype(int) - ref.astype(int)).max(axis=-1) > 1).sum())
    assert bad < 1e-3 * h * w * len(refs), (cam, h, w, bad)


@pytest.mark.parametrize("vis", ["off", "explicit"])
@pytest.mark.parametrize("env", RENDER_ENVS)
def test_render_rgb_shapes_vs_oracle(env, vis):
    """Every camera at each shape of RGB_SHAPES, 6 envs, VIS off and with explicit per-env colours, lights and camera offset."""
    dev, qpos, refs = _rgb_setup(env, vis)
    lit = 0
    for cam in _cams(dev.cm):
        for h, w in RGB_SHAPES:
            img = dev.render_rgb(cam, h, w).cpu().numpy()
            _rgb_check(img, refs, qpos, cam, h, w)
            lit += int((img != img[:, :1, :1]).any())
    assert lit > 0
    dev.k_close()


@pytest.mark.parametrize("vis", ["off", "explicit"])
def test_render_rgb_multi_job_odd_shapes(vis):
    """kmanip_render_rgb_multi with one job per camera at shapes other than the cameras' own -- a per-pixel job, a quad job with
    partial tiles and a one-quad-wide job in one launch: each job equals its single-camera render byte for byte and the oracle."""
    torch = _torch()
    dev, qpos, refs = _rgb_setup("KManipTorso", vis)
    jobs = [("grip_r", 37, 42), ("grip_l", 50, 72), ("top", 68, 100), ("head", 20, 4)]
    bufs = [torch.full((dev.num_envs, h, w, 3), 7, dtype=torch.uint8, device=dev.device) for _, h, w in jobs]
    m = len(jobs)
    ci = (C.c_int32 * m)(*[KM_CAM_INDEX[c] for c, _, _ in jobs])
    hh = (C.c_int32 * m)(*[h for _, h, _ in jobs])
    ww = (C.c_int32 * m)(*[w for _, _, w in jobs])
    pp = (C.c_void_p * m)(*[b.data_ptr() for b in bufs])
    dev._check(dev.L.kmanip_render_rgb_multi(dev.h, m, ci, hh, ww, pp, dev._stream()), "kmanip_render_rgb_multi")
    for (cam, h, w), b in zip(jobs, bufs):
        assert torch.equal(b, dev.render_rgb(cam, h, w)), cam
        _rgb_check(b.cpu().numpy(), refs, qpos, cam, h, w)
    dev.k_close()
