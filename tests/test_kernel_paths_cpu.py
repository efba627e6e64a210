"""CPU guards of tests/test_kernel_paths_gpu.py: its step matrix has a row for every kmanip_dyn object the Makefile compiles, and its
render shape lists reach every pixel-loop path of k_render_depth and k_render_rgb."""
import os
import sys

from conftest import ROOT
from gym_kmanip_amd.model import compile_model
from test_kernel_paths_gpu import DEPTH_SHAPES, RGB_SHAPES, STEP_ROWS

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import build_matrix as BM  # noqa: E402

SOLVER_OF = {"pgs": 0, "newton": 1}


def dyn_objects(makefile_path):
    """The kmanip_dyn objects without an applied force (tests/test_applied_force_gpu.py's guard answers for the _frc_ ones)."""
    return [o for o in BM.objects(makefile_path, "dyn") if not o.frc]


def covered(rows):
    """The (NL, G, SOLVER, per-env params) objects the rows launch: kmanip_dispatch.hip picks the 10-link class for nlink <= 10,
    the 20-link class otherwise; parameter mode "none" runs the default object, "explicit" and "ranges" the KM_VAR_PAR one."""
    nlink = {}
    out = set()
    for env, solver, mode in rows:
        if env not in nlink:
            nlink[env] = compile_model(env).nlink
        cls = (10, 16) if nlink[env] <= 10 else (20, 32)
        out.add(cls + (SOLVER_OF[solver], mode != "none"))
    return out


def missing_rows(makefile_path, rows):
    have = covered(rows)
    return [(o.NL, o.G, o.solver, o.ep) for o in dyn_objects(makefile_path) if (o.NL, o.G, o.solver, o.ep) not in have]


def test_every_compiled_step_object_has_an_oracle_row():
    assert len(dyn_objects(BM.MAKEFILE)) >= 2 * 4
    assert missing_rows(BM.MAKEFILE, STEP_ROWS) == []


def test_the_guard_fails_for_a_variant_without_a_row(tmp_path):
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    assert sorted(missing_rows(more, STEP_ROWS)) == [(30, 64, s, par) for s in (0, 1) for par in (False, True)]
    # ... and for a row set that drops one solver's parameter rows
    rows = [r for r in STEP_ROWS if not (r[1] == "pgs" and r[2] != "none")]
    assert (10, 16, 0, True) in missing_rows(BM.MAKEFILE, rows) and (20, 32, 0, True) in missing_rows(BM.MAKEFILE, rows)


def _colfixed(h, w):
    """kmanip_render.hip kmanip_launch_render_depth: the COLFIXED instantiation runs when a 128-lane workgroup spans whole rows."""
    return 128 % w == 0 and (h * w) % 128 == 0


def test_render_shapes_reach_every_pixel_loop():
    assert {_colfixed(h, w) for h, w in DEPTH_SHAPES} == {True, False}
    assert any(w > 128 for _, w in DEPTH_SHAPES) and (1, 1) in DEPTH_SHAPES
    assert {w for _, w in RGB_SHAPES if w % 4} >= {42, 61, 1}                          # k_render_rgb's per-pixel loop
    quad = [(h, w) for h, w in RGB_SHAPES if w % 4 == 0]
    assert any(w // 4 > 16 and (w // 4) % 16 for _, w in quad)                          # a partial tile column after a full one
    assert any(h % 16 for h, _ in quad) and any(w == 4 for _, w in quad)                # a partial tile row; one quad a row


def test_oracle_rgb_with_visual_values():
    """Oracle.render_rgb(vis=...), the reference of the VIS render tests: at the default values it is the default render bit for
    bit; with white materials lit by the ambient term alone every object pixel is round(255 a) and every background pixel
    round(255 bg)."""
    import numpy as np
    from gym_kmanip_amd.model import KM_CAM_INDEX, visual_param_defaults, visual_param_vector
    from oracle.oracle import Oracle
    cm = compile_model("KManipSoloArm")
    o = Oracle(cm, 1, seed=3)
    o.reset()
    qpos = o.get_state()[0][0]
    seen_bg = seen_obj = False
    for cam in ("grip_r", "top", "head"):
        base = o.render_rgb(qpos, KM_CAM_INDEX[cam], 48, 64)
        assert np.array_equal(o.render_rgb(qpos, KM_CAM_INDEX[cam], 48, 64, vis=visual_param_vector(visual_param_defaults())), base)
        bg = (base == 0).all(axis=-1)                          # the default background is black; every lit material is not
        seen_bg |= bool(bg.any()); seen_obj |= bool((~bg).any())
        a, b = 0.35, (0.2, 0.5, 0.9)
        img = o.render_rgb(qpos, KM_CAM_INDEX[cam], 48, 64, vis=visual_param_vector(dict(
            cube_rgb=(1, 1, 1), table_rgb=(1, 1, 1), robot_rgb=(1, 1, 1), background_rgb=b, ambient=a, headlight=0.0,
            directional=0.0)))
        assert (img[~bg] == np.floor(255 * a + 0.5)).all(), cam
        assert (img[bg] == np.floor(255 * np.array(b) + 0.5)).all(), cam
    assert seen_bg and seen_obj
