"""Per-env physics parameters, host side (no GPU): model.with_env_params -- the definition the kernels are held to -- and the
NumPy restatement of the ranges-mode draw."""
import math

import numpy as np
import pytest

from conftest import ENVS3
from gym_kmanip_amd.model import (ENV_PARAMS, KM_EP_CTR3, _philox4x32_10, _u53, compile_model, draw_env_params,
                                  env_param_defaults, invweight0, trace_robot, with_env_params)


def _fields(d):
    return {name: np.array(getattr(d, name)).tolist() if not isinstance(getattr(d, name), (int, float)) else getattr(d, name)
            for name, _ in type(d)._fields_}


@pytest.mark.parametrize("env", ENVS3)
def test_own_values_give_the_compiled_desc(env):
    cm = compile_model(env)
    same = with_env_params(cm, **env_param_defaults(cm))
    assert bytes(same.desc) == bytes(cm.desc)
    assert _fields(same.desc) == _fields(cm.desc)
    assert bytes(with_env_params(cm).desc) == bytes(cm.desc)
    assert same.desc is not cm.desc and same.nlink == cm.nlink and same.act_slices == cm.act_slices


@pytest.mark.parametrize("env", ENVS3)
@pytest.mark.parametrize("mass_f,mu,fl_f,kps", [(0.5, 0.3, 0.0, 0.5), (2.0, 1.5, 2.0, 1.5), (1.37, 0.0, 1.0, 1.0)])
def test_derived_constants_agree_with_invweight0(env, mass_f, mu, fl_f, kps):
    cm = compile_model(env)
    d0 = cm.desc
    m = with_env_params(cm, cube_mass=d0.cube_mass * mass_f, cube_friction=mu, cube_frictionloss=d0.cube_frictionloss * fl_f,
                        kp_scale=kps).desc
    dofw, bodyw, cubew, mi = invweight0(m)
    assert abs(m.cube_invweight0[0] - cubew[0]) <= 1e-15 * cubew[0]
    assert abs(m.cube_invweight0[1] - cubew[1]) <= 1e-15 * cubew[1]
    assert abs(m.meaninertia - mi) <= 1e-15 * mi
    for k in range(3):            # uniform density, unchanged size
        assert m.cube_inertia[k] == d0.cube_inertia[k] * (m.cube_mass / d0.cube_mass)
    assert m.con_cube_friction[0] == mu and m.con_cube_friction[1] == d0.con_cube_friction[1]
    assert m.cube_frictionloss == d0.cube_frictionloss * fl_f
    assert [m.kp[i] for i in range(m.nlink)] == [d0.kp[i] * kps for i in range(m.nlink)]
    # nothing the parameters do not own changes
    owned = {"cube_mass", "cube_inertia", "cube_invweight0", "meaninertia", "con_cube_friction", "cube_frictionloss", "kp"}
    f0, f1 = _fields(d0), _fields(m)
    assert {k for k in f0 if f0[k] != f1[k]} <= owned
    # the robot part of the trace is the library's (meaninertia * nv minus the cube's part)
    assert abs(trace_robot(d0) - (mi * (m.nlink + 6) - 3 * m.cube_mass - sum(m.cube_inertia))) < 1e-14


@pytest.mark.parametrize("name,bad", [("cube_mass", 0.0), ("cube_mass", -0.1), ("cube_friction", -1e-3),
                                      ("cube_frictionloss", -1.0), ("kp_scale", 0.0), ("kp_scale", -2.0),
                                      ("cube_mass", math.nan), ("cube_friction", math.inf), ("kp_scale", -math.inf)])
def test_bad_values_raise(name, bad):
    cm = compile_model("KManipSoloArm")
    with pytest.raises(ValueError):
        with_env_params(cm, **{name: bad})


def test_zero_friction_terms_are_allowed():
    cm = compile_model("KManipSoloArm")
    d = with_env_params(cm, cube_friction=0.0, cube_frictionloss=0.0).desc
    assert d.con_cube_friction[0] == 0.0 and d.cube_frictionloss == 0.0


def test_draw_restatement_matches_the_oracle_philox():
    """Counter words 2 and 3 of the (seed, global env id, episode) stream, as the device draws them, against the oracle's own
    Philox4x32-10 (the one the cube spawn parity is built on)."""
    from oracle.oracle import Oracle
    orc = Oracle(compile_model("KManipSoloArm"), 1)
    lo = np.array([0.025, 0.3, 0.0, 0.5]); hi = np.array([0.1, 1.5, 0.02, 1.5])
    for seed, genv, episode in [(0, 0, 0), (7, 3, 1), (2**40 + 5, 2**33 + 17, 12), (123456789, 4095, 2**31 - 1)]:
        key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
        ctr = lambda w3: np.array([genv & 0xFFFFFFFF, genv >> 32, episode, w3], dtype=np.uint32)
        for w3 in (KM_EP_CTR3, KM_EP_CTR3 + 1):
            assert np.array_equal(_philox4x32_10(ctr(w3), key), orc.philox(ctr(w3), key))
        o0, o1 = orc.philox(ctr(KM_EP_CTR3), key), orc.philox(ctr(KM_EP_CTR3 + 1), key)
        u = [_u53(o0[0], o0[1]), _u53(o0[2], o0[3]), _u53(o1[0], o1[1]), _u53(o1[2], o1[3])]
        want = np.array([lo[k] + (hi[k] - lo[k]) * u[k] for k in range(4)])
        got = draw_env_params(seed, genv, episode, lo, hi)
        assert np.array_equal(got, want)
        assert ((got >= lo) & (got <= hi)).all()
    assert np.array_equal(draw_env_params(3, 9, 4, lo, lo), lo)        # lo == hi pins
    assert len(ENV_PARAMS) == 4
