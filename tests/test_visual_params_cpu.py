"""Per-env visual parameters, host side (no GPU): the NumPy restatement of the ranges draw, model.with_visual_params -- the
definition the camera offset is held to -- the Python setters' validation, and the VIS render kernels' resources."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gym_kmanip_amd.model import (ENV_PARAMS, ENV_SPECS, KM_EP_CTR3, KM_VP_CTR3, KM_VP_N, VISUAL_PARAMS, _philox4x32_10, _u53,
                                  compile_model, draw_env_params, draw_visual_params, visual_param_defaults,
                                  visual_param_vector, with_visual_params)


def _ranges(rng):
    a, b = rng.uniform(0, 1, KM_VP_N), rng.uniform(0, 1, KM_VP_N)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    lo[15:], hi[15:] = -0.2 * lo[15:], 0.2 * hi[15:]
    return lo, hi


def test_philox_matches_the_known_answers():
    kat = np.load(os.path.join(GOLDEN, "philox_kat.npz"))["kat"]
    for row in kat:
        assert np.array_equal(_philox4x32_10(row[:4], row[4:6]), row[6:])


def test_draw_is_inside_the_ranges_and_deterministic():
    rng = np.random.default_rng(0)
    lo, hi = _ranges(rng)
    seen = set()
    for seed, genv, ep in [(0, 0, 0), (1, 5, 3), (2**40 + 7, 2**33 + 11, 9), (3, 4095, 1000)]:
        p = draw_visual_params(seed, genv, ep, lo, hi)
        assert p.shape == (KM_VP_N,) and (p >= lo).all() and (p <= hi).all()
        assert np.array_equal(p, draw_visual_params(seed, genv, ep, lo, hi))
        seen.add(p.tobytes())
    assert len(seen) == 4
    base = draw_visual_params(1, 5, 3, lo, hi)
    for other in [(2, 5, 3), (1, 6, 3), (1, 5, 4)]:
        assert not (draw_visual_params(*other, lo, hi) == base).any()
    pinned = draw_visual_params(1, 5, 3, lo, lo)
    assert np.array_equal(pinned, lo)


def test_draw_restates_the_counter_layout():
    """Value k: lo + (hi - lo) * u53 of words (0, 1) / (2, 3) of the block with counter word 3 = KM_VP_CTR3 + k // 2, and the
    stream is disjoint from the physics draw's (KM_EP_CTR3) for the same counter."""
    assert KM_VP_CTR3 == 0x100 and KM_VP_CTR3 > KM_EP_CTR3 + 1 and KM_VP_CTR3 + KM_VP_N // 2 < 0x10000
    seed, genv, ep = 12345, 77, 6
    lo, hi = np.zeros(KM_VP_N), np.ones(KM_VP_N)
    p = draw_visual_params(seed, genv, ep, lo, hi)
    for k in range(KM_VP_N):
        o = _philox4x32_10((genv, 0, ep, KM_VP_CTR3 + k // 2), (seed, 0))
        assert p[k] == _u53(o[2 * (k % 2)], o[2 * (k % 2) + 1])
    q = draw_env_params(seed, genv, ep, np.zeros(len(ENV_PARAMS)), np.ones(len(ENV_PARAMS)))
    assert not np.isin(q, p).any()


def test_defaults_vector():
    v = visual_param_vector({})
    assert v.tolist() == [1, 0, 0, .2, .2, .2, .647059, .647059, .647059, 0, 0, 0, .4, .4, 1, 0, 0, 0]
    assert sorted(k for k, _ in VISUAL_PARAMS.values()) == [0, 3, 6, 9, 12, 13, 14, 15]
    assert set(visual_param_defaults()) == set(VISUAL_PARAMS)
    assert visual_param_vector({"ambient": 0.7, "camera_offset": (0.1, 0, -0.1)})[[12, 15, 16, 17]].tolist() == [0.7, 0.1, 0, -0.1]


def _fields(d):
    return {name: np.array(getattr(d, name)).tolist() for name, _ in type(d)._fields_}


@pytest.mark.parametrize("env_id", list(ENV_SPECS))
def test_with_visual_params_shifts_only_cam_pos(env_id):
    cm = compile_model(env_id)
    o = (0.03, -0.02, 0.1)
    m = with_visual_params(cm, camera_offset=o)
    f0, f1 = _fields(cm.desc), _fields(m.desc)
    assert {k for k in f0 if f0[k] != f1[k]} == {"cam_pos"}
    for c in range(4):
        for k in range(3):
            exp = cm.desc.cam_pos[c][k] + o[k] if cm.desc.cam_present[c] else cm.desc.cam_pos[c][k]
            assert m.desc.cam_pos[c][k] == exp
    assert bytes(with_visual_params(cm).desc) == bytes(cm.desc)
    assert bytes(with_visual_params(cm, ambient=0.9, cube_rgb=(0, 1, 0)).desc) == bytes(cm.desc)
    assert m.desc is not cm.desc and m.cameras == cm.cameras


@pytest.mark.parametrize("kw", [{"camera_offset": (0.3, 0, 0)}, {"camera_offset": (0, 0, math.nan)}, {"camera_offset": (0.1, 0.1)},
                                {"ambient": -0.1}, {"cube_rgb": (1.2, 0, 0)}, {"shininess": 1.0}])
def test_with_visual_params_refuses_bad_values(kw):
    with pytest.raises(ValueError):
        with_visual_params(compile_model("KManipSoloArmVision"), **kw)


class _NoLib:
    """Stands in for the ctypes library: any call fails the test (validation must happen before it)."""

    def __getattr__(self, name):
        raise AssertionError("ctypes call %s reached" % name)


def _env(n=4):
    from gym_kmanip_amd import env_hip
    e = env_hip.KManipEnvHip.__new__(env_hip.KManipEnvHip)
    e.cm, e.num_envs, e.device, e.L, e.h = compile_model("KManipSoloArmVision"), n, "cpu", _NoLib(), None
    e._vp_active, e._vp_ranges = False, None
    return e


@pytest.mark.parametrize("kw", [{"cube_rgb": (1.1, 0, 0)}, {"table_rgb": -0.5}, {"robot_rgb": np.full((4, 3), math.nan)},
                                {"background_rgb": np.zeros((5, 3))}, {"background_rgb": np.zeros((4, 2))},
                                {"ambient": -1.0}, {"headlight": math.inf}, {"directional": np.zeros((4, 3))},
                                {"directional": np.zeros(3)}, {"camera_offset": (0.26, 0, 0)},
                                {"camera_offset": np.zeros((4, 2))}, {"specular": 0.5}])
def test_setter_validation_before_the_library(kw):
    pytest.importorskip("torch")
    with pytest.raises(ValueError):
        _env().set_visual_params(**kw)


@pytest.mark.parametrize("kw", [{"ambient": (0.5, 0.4)}, {"ambient": (-0.1, 0.4)}, {"cube_rgb": (0.0, 1.5)},
                                {"camera_offset": (-0.3, 0.0)}, {"camera_offset": ((0, 0, 0), (0.1, 0.1))},
                                {"ambient": ((0, 0, 0), (1, 1, 1))}, {"headlight": (0.1,)}, {"fog": (0, 1)},
                                {"table_rgb": ((0.2, 0.5, 0.2), (0.3, 0.4, 0.3))}])
def test_ranges_validation_before_the_library(kw):
    pytest.importorskip("torch")
    with pytest.raises(ValueError):
        _env().set_visual_param_ranges(**kw)


LIB = os.path.join(ROOT, "gym_kmanip_amd", "libkmanip_hip.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="the library is not built")
def test_vis_kernel_resources():
    """The VIS render kernels keep the default's occupancy: rgb <= 128 VGPR and no scratch; depth no more scratch than the
    default kernels (0 with a whole number of rows per workgroup, 52 B without)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import build_matrix as BM
    rgb = BM.kernels(LIB, "k_render_rgb")
    rgb_vis = [k for k in rgb if k.args[0] is True]
    rgb_def = [k for k in rgb if k.args[0] is False]
    d = {k.args[:2]: k for k in BM.kernels(LIB, "k_render_depth")}          # (COLFIXED, VIS)
    assert len(rgb_vis) == 1 and len(rgb_def) == 1 and len(d) == 4, (rgb, d)
    assert rgb_vis[0].vgpr <= 128 and rgb_vis[0].scratch == 0
    assert d[(1, 1)].scratch == 0 and d[(0, 1)].scratch <= d[(0, 0)].scratch
