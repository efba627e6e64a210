"""Segmentation labels of the camera renders, host side (no GPU): the sphere -> arm rule, the reference labels the GPU tests are
held to (tests/tools/label_oracle.py, built on the CPU oracle's RGB ray caster), the C ABI's declarations, the shell's spaces,
the episode logger's label datasets and the label kernels' resources."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd import model as M
from gym_kmanip_amd.model import CAMERAS, ENV_SPECS, KM_CAM_INDEX, MAX_EPISODE_STEPS, compile_model, sphere_arm

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import h5_recorder as H5  # noqa: E402
from label_oracle import LabelOracle, flat_vector  # noqa: E402

VISION = ["KManipSoloArmVision", "KManipDualArmVision", "KManipTorsoVision"]
DUAL = [0, 0, 1, 1, 0, 1, 0, 1, 0, 1, 0, 1]
LIB = os.path.join(ROOT, "gym_kmanip_amd", "libkmanip_hip.so")


@pytest.mark.parametrize("env_id,table", [("KManipSoloArm", [0] * 6), ("KManipDualArm", DUAL), ("KManipTorso", DUAL)])
def test_sphere_arm_tables(env_id, table):
    """The rule of include/kmanip.h names exactly one arm for every sphere (strict=True raises otherwise) and gives these tables."""
    cm = compile_model(env_id)
    assert sphere_arm(cm, strict=True) == table and sphere_arm(cm) == table and len(table) == cm.desc.nsphere


def test_sphere_arm_of_a_sphere_on_no_chain():
    """A sphere on no arm's chain is no error of the model (kmanip_create accepts such a desc as it always did): it counts as
    arm 0, on the host and here alike; only strict=True refuses it."""
    import dataclasses
    cm = compile_model("KManipDualArm")
    d = M.KModelDesc.from_buffer_copy(cm.desc)
    d.arm_present[1] = 0
    one = dataclasses.replace(cm, desc=d)
    assert sphere_arm(one) == [0] * cm.desc.nsphere
    with pytest.raises(ValueError):
        sphere_arm(one, strict=True)


def _stepped_qpos(cm, steps=12, seed=3):
    from oracle.oracle import Oracle
    o = Oracle(cm, 1, seed=seed)
    o.reset()
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        o.step(rng.uniform(-1, 1, (1, cm.act_dim)).astype(np.float32))
    return o.get_state()[0][0]


def _cams(cm):
    return [name for name, ci in KM_CAM_INDEX.items() if cm.desc.cam_present[ci]]


@pytest.mark.parametrize("env_id", VISION)
def test_reference_labels(env_id):
    """On a stepped state, every camera at its own resolution: three equal channels (asserted by the helper), values 0..3, every
    class in at least one camera's image; right-only and left-only robot pixels together are the all-visible robot pixels."""
    cm = compile_model(env_id)
    qpos = _stepped_qpos(cm)
    lo = LabelOracle(cm)
    arms = sorted(set(sphere_arm(cm)))
    full = set()
    for cam in _cams(cm):
        spec = CAMERAS[cam]
        lab = lo.labels(qpos, KM_CAM_INDEX[cam], spec.h, spec.w)
        assert lab.dtype == np.uint8 and lab.shape == (spec.h, spec.w) and lab.max() <= 3
        print(env_id, cam, np.bincount(lab.ravel(), minlength=4).tolist())
        if set(np.unique(lab).tolist()) == {0, 1, 2, 3}:
            full.add(cam)
        union = np.zeros(lab.shape, dtype=bool)
        for a in arms:
            la = lo.arm_labels(qpos, KM_CAM_INDEX[cam], spec.h, spec.w, a)
            assert ((la == 3) <= (lab == 3)).all(), (cam, a)
            assert np.array_equal(la[lab != 3], lab[lab != 3]), (cam, a)     # hiding spheres changes robot pixels only
            union |= la == 3
        assert np.array_equal(union, lab == 3), cam
    assert full, "no camera of %s sees all four classes" % env_id


def test_flat_vector():
    v = flat_vector()
    assert np.allclose(v[0:3], 2 / 255) and np.allclose(v[3:6], 1 / 255) and np.allclose(v[6:9], 3 / 255)
    assert v[9:15].tolist() == [0, 0, 0, 1, 0, 0] and v[15:].tolist() == [0, 0, 0]


def test_abi_declarations():
    """The header declares KM_SEG_* with the issue's values and both entry points; lib.py has their prototypes."""
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    m = re.search(r"enum\s*\{\s*KM_SEG_BACKGROUND = 0, KM_SEG_TABLE = 1, KM_SEG_CUBE = 2, KM_SEG_ROBOT_R = 3, KM_SEG_ROBOT_L = 4, KM_SEG_N = 5\s*\}", hdr)
    assert m
    assert (M.KM_SEG_BACKGROUND, M.KM_SEG_TABLE, M.KM_SEG_CUBE, M.KM_SEG_ROBOT_R, M.KM_SEG_ROBOT_L, M.KM_SEG_N) == (0, 1, 2, 3, 4, 5)
    assert re.search(r"KMANIP_API int kmanip_render_labels_multi\(KHandle h, int ncam, const int\* cams, const int\* heights, const int\* widths,\s*"
                     r"uint8_t\* const\* rgb_dev, uint8_t\* const\* seg_dev, void\* stream\);", hdr)
    assert re.search(r"KMANIP_API int kmanip_render_seg\(KHandle h, int cam, int height, int width, uint8_t\* seg_dev, void\* stream\);", hdr)
    from gym_kmanip_amd import lib
    assert "kmanip_render_labels_multi" in lib.EXPORTS and "kmanip_render_seg" in lib.EXPORTS
    src = open(os.path.join(ROOT, "gym_kmanip_amd", "lib.py")).read()
    assert "lib.kmanip_render_labels_multi.argtypes" in src and "lib.kmanip_render_seg.argtypes" in src


@pytest.mark.skipif(not os.path.exists(LIB), reason="the library is not built")
def test_prototypes_are_bound():
    from gym_kmanip_amd import lib
    L = lib.load()
    assert len(L.kmanip_render_labels_multi.argtypes) == 8 and len(L.kmanip_render_seg.argtypes) == 6
    assert L.kmanip_render_seg(None, 0, 4, 4, None, None) != 0          # a null handle is refused, not dereferenced
    assert L.kmanip_render_labels_multi(None, 0, None, None, None, None, None, None) != 0
    assert b"null handle" in L.kmanip_last_error(None)


@pytest.mark.parametrize("env_id", list(ENV_SPECS))
def test_shell_spaces(env_id):
    """segmentation=True: "segmentation/<cam>" Boxes (0 .. KM_SEG_N - 1, (h, w), uint8) after the camera keys, nothing else
    changes; False: spaces_for is what it was."""
    from gym_kmanip_amd import gym_shell
    base, off, on = gym_shell.spaces_for(env_id), gym_shell.spaces_for(env_id, segmentation=False), gym_shell.spaces_for(env_id, segmentation=True)
    assert list(base["observation"]) == list(off["observation"]) and list(base["action"]) == list(on["action"])
    cams = [o.split("/")[-1] for o in ENV_SPECS[env_id].obs_list if "camera" in o]
    keys = list(on["observation"])
    assert keys == list(base["observation"]) + ["segmentation/" + c for c in cams]
    for c in cams:
        b = on["observation"]["segmentation/" + c]
        assert tuple(b.shape) == (CAMERAS[c].h, CAMERAS[c].w) and b.dtype == np.uint8
        assert (np.asarray(b.low) == 0).all() and (np.asarray(b.high) == M.KM_SEG_N - 1).all()
        assert keys.index("segmentation/" + c) > keys.index(CAMERAS[c].log_name)
    for k in base["observation"]:
        assert tuple(on["observation"][k].shape) == tuple(base["observation"][k].shape)


def _episode(lg, n, q_len, a_len, cams, labels, seed=1):
    import torch
    rng = np.random.default_rng(seed)
    last = None
    for _ in range(MAX_EPISODE_STEPS):
        imgs = {c.name: torch.from_numpy(rng.integers(0, 256, (n, c.h, c.w, 3), dtype=np.uint8)) for c in cams}
        segs = {"segmentation/" + c.name: torch.from_numpy(rng.integers(0, M.KM_SEG_N, (n, c.h, c.w), dtype=np.uint8)) for c in cams} if labels else None
        lg.step(torch.from_numpy(rng.uniform(-1, 1, (n, a_len)).astype(np.float32)), torch.from_numpy(rng.uniform(0, 1, (n, q_len))),
                torch.from_numpy(rng.uniform(-1, 1, (n, q_len))), images=imgs or None, labels=segs)
        last = segs
    return last


def _logger(tmp_path, cm, cams, labels, **kw):
    from gym_kmanip_amd.episode_log import EpisodeLogger
    lg = EpisodeLogger(str(tmp_path), 3, 10, cm.act_dim, env_ids=[1], info={"sim": True}, backend="h5py", h5py_module=H5, **kw)
    for c in cams:
        lg.cam(c, labels=labels) if labels else lg.cam(c)
    return lg


def test_episode_logger_labels(tmp_path):
    """With labels the tree gains exactly observations/segmentation/<name> [T, h, w] uint8, chunked one frame at a time, holding
    the selected env's labels; without, the tree is today's; the reference layout with labels raises."""
    pytest.importorskip("torch")
    cm = compile_model("KManipSoloArmVision")
    cams = [CAMERAS[c] for c in ("head", "grip_r")]
    H5.FILES.clear()
    (tmp_path / "a").mkdir()
    a = _logger(tmp_path / "a", cm, cams, False)
    _episode(a, 3, 10, cm.act_dim, cams, False)
    plain = H5.tree(H5.FILES[a.end_episode()[0]], skip_attr_values=("cpu_time",))
    (tmp_path / "b").mkdir()
    b = _logger(tmp_path / "b", cm, cams, True)
    last = _episode(b, 3, 10, cm.act_dim, cams, True)
    f = H5.FILES[b.end_episode()[0]]
    with_labels = H5.tree(f, skip_attr_values=("cpu_time",))
    seg = with_labels["groups"]["observations"]["groups"].pop("segmentation")
    assert with_labels == plain
    assert seg["groups"] == {} and seg["attrs"] == {} and set(seg["datasets"]) == {"head", "grip_r"}
    for c in cams:
        assert seg["datasets"][c.name] == {"shape": [MAX_EPISODE_STEPS, c.h, c.w], "dtype": "uint8", "chunks": [1, c.h, c.w]}
        data = np.asarray(f["observations/segmentation/" + c.name][:])
        assert np.array_equal(data[-1], last["segmentation/" + c.name][1].numpy())
    # a step without the labels of a camera registered with them is an error, as a missing frame is
    import torch
    with pytest.raises(KeyError):
        b.step(torch.zeros((3, cm.act_dim)), torch.zeros((3, 10)), torch.zeros((3, 10)),
               images={c.name: torch.zeros((3, c.h, c.w, 3), dtype=torch.uint8) for c in cams})
    # the reference layout has no such node
    (tmp_path / "c").mkdir()
    q = _logger(tmp_path / "c", cm, [], False, grip_r_col=cm.act_slices["grip_r"].start, reference_action_quirk=True, ref_a_len=3)
    with pytest.raises(ValueError):
        q.cam(cams[0], labels=True)
    q.cam(cams[1])
    with pytest.raises(ValueError):
        q.step(torch.zeros((3, cm.act_dim)), torch.zeros((3, 10)), torch.zeros((3, 10)),
               images={"grip_r": torch.zeros((3, 40, 60, 3), dtype=torch.uint8)},
               labels={"segmentation/grip_r": torch.zeros((3, 40, 60), dtype=torch.uint8)})


def test_episode_logger_late_labels(tmp_path):
    """late_images takes the segmentation/<name> frames with the camera frames (what RenderBehind(segmentation=True).images()
    returns)."""
    torch = pytest.importorskip("torch")
    cm = compile_model("KManipSoloArmVision")
    cam = CAMERAS["grip_r"]
    H5.FILES.clear()
    lg = _logger(tmp_path, cm, [cam], True)
    with pytest.raises(ValueError):       # labels now, frames later: refused, not dropped
        lg.step(torch.zeros((3, cm.act_dim)), torch.zeros((3, 10)), torch.zeros((3, 10)), images_later=True,
                labels={"segmentation/grip_r": torch.zeros((3, cam.h, cam.w), dtype=torch.uint8)})
    assert lg.t == 0
    t = lg.step(torch.zeros((3, cm.act_dim)), torch.zeros((3, 10)), torch.zeros((3, 10)), images_later=True)
    with pytest.raises(KeyError):
        lg.late_images(t, {"grip_r": torch.zeros((3, cam.h, cam.w, 3), dtype=torch.uint8)})
    seg = torch.randint(0, M.KM_SEG_N, (3, cam.h, cam.w), dtype=torch.uint8)
    lg.late_images(t, {"grip_r": torch.ones((3, cam.h, cam.w, 3), dtype=torch.uint8), "segmentation/grip_r": seg})
    f = H5.FILES[lg.end_episode()[0]]
    assert np.array_equal(np.asarray(f["observations/segmentation/grip_r"][:])[0], seg[1].numpy())


@pytest.mark.skipif(not os.path.exists(LIB), reason="the library is not built")
def test_label_kernel_resources():
    """Every k_render_labels instantiation keeps the RGB kernel's occupancy: <= 128 VGPR (four waves per SIMD), no scratch; the
    four instantiations (VIS x RGB) exist, and k_render_rgb still has exactly its two."""
    import build_matrix as BM
    all_lab = BM.kernels(LIB, "k_render_labels")
    lab = {k.args[:2]: k for k in all_lab}                                  # (VIS, RGB)
    assert len(lab) == 4 and len(all_lab) == 4, all_lab
    for key, v in lab.items():
        print("k_render_labels<VIS=%d, RGB=%d>" % key, v)
        assert v.vgpr <= 128 and v.scratch == 0, (key, v)
    assert sum(type(k.args[0]) is bool for k in BM.kernels(LIB, "k_render_rgb")) == 2
