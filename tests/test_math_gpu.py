"""The kernels' FP64 math and quaternion helpers on the device (run with -m gpu on an MI355X): every function of
kmanip_dbg_math over the whole fixture tests/golden/math_edges.npz -- one launch each, on a handle of 2 envs -- against the 50-digit
reference stored with it.  The bars are tests/tools/math_reference.py's: tools/libm_check.hip's exit criteria for kmanip_math.hpp
and the reciprocals, ten times the NumPy restatement's measured error for the quaternion helpers (tests/test_math_cpu.py measures
it).  Also: the probe's refusals, the same rows in reversed order, and the handle's next steps beside a twin that never called it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import math_reference as MR  # noqa: E402

pytestmark = pytest.mark.gpu

SCALAR_FNS = ("km_sincos", "km_atan2", "km_sqrt", "km_rcp", "frcp", "rsqrt_nr")
_RUN = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _handle(seed=5):
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.model import compile_model
    dev = env_hip.KManipEnvHip(compile_model("KManipSoloArm"), num_envs=2, device=0, seed=seed)
    dev.k_reset()
    return dev


def _run():
    """(fixture, the probed handle, {fn: results}, {fn: results of the reversed rows, reversed back}): every launch made once."""
    if not _RUN:
        torch = _torch()
        fx = MR.load()
        dev = _handle()
        got, rev = {}, {}
        for fn, sname in MR.FN_SET.items():
            rows = torch.from_numpy(fx[sname + "_in"]).cuda()
            got[fn] = dev.dbg_math(fn, rows).cpu().numpy()
            rev[fn] = dev.dbg_math(fn, rows.flip(0).contiguous()).cpu().numpy()[::-1]
        _RUN.update(fx=fx, dev=dev, got=got, rev=rev)
    return _RUN["fx"], _RUN["dev"], _RUN["got"], _RUN["rev"]


@pytest.mark.parametrize("fn", SCALAR_FNS)
def test_math_functions_against_50_digits(fn):
    """km_sincos below 4 ulp where the reduction index is 0 and below 4 x 2^-53 absolute elsewhere (its relative error next to a
    zero is printed, not bounded), km_atan2 below 4 ulp on its domain, km_sqrt / km_rcp / frcp / rsqrt_nr below 2 ulp, perfect
    squares exact, km_sqrt 0 at 0, -0 and negative arguments."""
    fx, _, got, _ = _run()
    assert MR.report("device " + fn, MR.scalar_figures(fx, fn, got[fn])) == []


@pytest.mark.parametrize("fn", sorted(MR.NP_FN))
def test_quaternion_helpers_against_50_digits(fn):
    """Per component |device - reference| <= C_DEVICE x 2^-53 x scale (scale 1 for unit vectors and quaternions, max(|r|, 1) for a
    log map, the norm itself for normalize3_fast's return), C_DEVICE ten times the NumPy restatement's worst; per tag for the record."""
    fx, _, got, _ = _run()
    sname = MR.FN_SET[fn]
    u = MR.quat_units(fx, fn, got[fn])
    for t in fx[sname + "_tags"]:
        print("device %s: %s worst %.3f x 2^-53 x scale" % (fn, t, u[MR.tag_mask(fx, sname, t)].max()))
    print("device %s: worst %.3f at row %d (bar %.1f, NumPy %.2f)" % (fn, u.max(), int(u.argmax()), MR.C_DEVICE[fn], MR.C_HOST[fn]))
    assert u.max() <= MR.C_DEVICE[fn]
    if fn == "quat_log_diff":
        assert (got[fn][MR.tag_mask(fx, sname, "equal")] == 0).all()           # equal quaternions: exactly zero
    if fn == "sub_quat_sc":                                                    # sub_quat's result and the half angle's sine and |cosine| in one call
        assert got[fn][:, :3].tobytes() == got["sub_quat"].tobytes()
        half = 0.5 * np.sqrt((got[fn][:, :3] ** 2).sum(1))
        assert np.abs(np.arctan2(got[fn][:, 3], got[fn][:, 4]) - half).max() < 0.5 * MR.C_DEVICE[fn] * 2.0 ** -53 * np.pi


def test_reversed_rows_give_reversed_bytes():
    """Element-wise: a row's results do not depend on where the row stands or on its neighbours in the wave."""
    _, _, got, rev = _run()
    assert [fn for fn in got if got[fn].tobytes() != np.ascontiguousarray(rev[fn]).tobytes()] == []


def test_probe_refusals():
    """An unknown fn, wrong column counts, a NULL pointer or a negative n: an error through kmanip_last_error and nothing launched
    (the output keeps its bytes); n = 0 succeeds, also with NULL pointers."""
    torch = _torch()
    _, dev, _, _ = _run()
    L = dev.L
    rows = torch.ones((4, 2), dtype=torch.float64, device="cuda")
    out = torch.full((4, 2), -7.0, dtype=torch.float64, device="cuda")
    i, o = C.c_void_p(rows.data_ptr()), C.c_void_p(out.data_ptr())
    refused = [((dev.h, -1, 4, i, 1, o, 2), b"kmanip_dbg_math: no such function"), ((dev.h, 13, 4, i, 1, o, 2), b"kmanip_dbg_math: no such function"),
               ((dev.h, 0, 4, i, 2, o, 2), b"kmanip_dbg_math: in_cols is not the function's argument count"),
               ((dev.h, 0, 4, i, 1, o, 1), b"kmanip_dbg_math: out_cols is not the function's result count"),
               ((dev.h, 1, 4, i, 2, o, 2), b"kmanip_dbg_math: out_cols is not the function's result count"),
               ((dev.h, 0, 4, None, 1, o, 2), b"kmanip_dbg_math: in_dev is NULL"), ((dev.h, 0, 4, i, 1, None, 2), b"kmanip_dbg_math: out_dev is NULL"),
               ((dev.h, 0, -1, i, 1, o, 2), b"kmanip_dbg_math: n is negative")]
    for args, msg in refused:
        assert L.kmanip_dbg_math(*args, None) != 0 and L.kmanip_last_error(dev.h) == msg, msg
    assert L.kmanip_dbg_math(None, 0, 4, i, 1, o, 2, None) != 0 and L.kmanip_last_error(None) == b"kmanip_dbg_math: null handle"
    assert L.kmanip_dbg_math(dev.h, 0, 0, None, 1, None, 2, None) == 0 and L.kmanip_dbg_math(dev.h, 0, 0, i, 1, o, 2, None) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert L.kmanip_dbg_math(dev.h, 0, 4, i, 1, o, 2, None) == 0           # and the call the refusals were variations of runs
    torch.cuda.synchronize()
    assert np.abs(out.cpu().numpy() - [np.sin(1.0), np.cos(1.0)]).max() < 1e-15


def test_handle_steps_like_a_twin_that_never_probed():
    """The probe reads no handle state and leaves none: after every function ran on it, the handle's next steps have the bytes of
    a twin handle's that never called it."""
    torch = _torch()
    _, dev, _, _ = _run()
    twin = _handle()
    rng = np.random.default_rng(3)
    for _ in range(3):
        act = torch.from_numpy(rng.uniform(-1, 1, (2, dev.cm.act_dim)).astype(np.float32)).cuda()
        dev.step_flat(act); twin.step_flat(act)
    for a, b in zip(dev.get_state(), twin.get_state()):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert torch.equal(dev.obs, twin.obs) and torch.equal(dev.reward, twin.reward) and torch.equal(dev.done, twin.done)
    twin.k_close()


@pytest.mark.parametrize("env", ["KManipSoloArm", "KManipDualArm", "KManipTorso"])
def test_ik_eval_orientation_rows_where_the_coefficient_cancels(env):
    """Rows 3 to 5 of kmanip_ik_eval's residual and Jacobian on subquat_jac's sweep (8 poses x the rotation sweep; theta = 1.2e-7 is
    the `half < 6e-8` switch, from both sides down to the rounding of the goal) against the 50-digit composition evaluated at the
    residual the same call returned: ten times the oracle's measured error.  The rows below the switch show the expected jump (the
    coefficient h^2 / 3 <= 1.2e-15 dropped) once more than the rows above it: the jump is there and no larger.  (The difference of
    the two shares: the device's IK frames are 1.1e-15 too long (un-normalised asset quaternions), which moves both shares alike --
    measured 1.93 / 0.91, 1.88 / 0.88, 1.63 / 0.65 where the oracle has 0.99 / 0.03; DESIGN.md section 38, finding 5.)"""
    pytest.importorskip("mpmath")
    import subquat_jac as SJ
    from gym_kmanip_amd import env_hip
    _torch()
    sw = SJ.sweep(env)
    dev = env_hip.KManipEnvHip(sw["cm"], num_envs=2, device=0, seed=1)
    dev.k_reset()
    res, jac = dev.ik_eval(SJ.ARM, sw["qpos"], sw["goal_pos"], sw["goal_quat"])
    dev.k_close()
    f = SJ.jac_figures(sw, res, jac)
    e = SJ.res_figures(sw, res)
    print("device %s: ik_jac rows 3-5 worst %.2f x 2^-53 rad (%s; bar %.0f), ik_res rows 3-5 worst %.2f (bar %.0f); below the switch %d rows show %.3f of the jump %.3g, above it %d rows %.3f"
          % (env, f["worst"].max(), sw["tag"][f["worst"].argmax()], 10 * SJ.C_HOST_JAC, e.max(), 10 * SJ.C_HOST_RES, f["below"], f["share_below"], f["jump"],
             f["above"], f["share_above"]))
    assert f["worst"].max() <= 10 * SJ.C_HOST_JAC and e.max() <= 10 * SJ.C_HOST_RES
    assert f["below"] >= 16 and f["above"] >= 16
    assert 0.8 < f["share_below"] - f["share_above"] < 1.2
    assert 1.0e-15 < f["jump"] <= 1.2e-15
