"""The seam on the reference's OWN object (VERDICT r5 task 7).

`env_hip.new(gym_env)` is meant to be called from the reference's `KManipEnv.__init__` where it calls `env_sim.new(self)`
(env_base.py:192-200), i.e. with the reference's own instance -- whose attributes carry the reference's types (tuples, NumPy
arrays, `None` masks), not the ones `gym_shell.KManipEnv` happens to use.  tests/golden/ref_instances.json records that instance
as the reference built it (tests/tools/make_golden_ref.py over tests/tools/refrun.py): the value and the Python type of every
attribute env_sim reads, the attributes it lacks, its Dict spaces in insertion order.  `make_env` rebuilds it here with exactly
those types; `spec_from_gym_env` + `compile_model` must turn it into, byte for byte, the `KModelDesc` the registered-id shortcut
(`ENV_SPECS[id]`) compiles, with the action / observation columns in the order the reference's Dict spaces were filled
(env_base.py:115-188)."""
import collections
import json
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN
from gym_kmanip_amd import env_hip
from gym_kmanip_amd.model import CAMERAS, ENV_SPECS, compile_model

IDS = sorted(ENV_SPECS)
PY_TYPES = {"str": str, "int": int, "list": list, "tuple": tuple}


def _value(rec):
    """One attribute as the reference's instance held it: same Python type, same dtype."""
    if rec["type"] == "NoneType":
        assert rec["value"] is None
        return None
    if rec["type"] == "ndarray":
        return np.asarray(rec["value"], dtype=rec["dtype"])
    return PY_TYPES[rec["type"]](rec["value"])


def _space(rows):
    return collections.OrderedDict((n, types.SimpleNamespace(shape=tuple(shape), dtype=np.dtype(dt))) for n, shape, dt in rows)


@pytest.fixture(scope="module")
def ref_instances():
    with open(os.path.join(GOLDEN, "ref_instances.json")) as f:
        recs = json.load(f)
    assert sorted(recs) == IDS

    def make_env(env_id):
        rec = recs[env_id]
        assert rec["cls"] == "gym_kmanip.env_base:KManipEnv"              # recorded from the reference's class, not the build's shell
        env = types.SimpleNamespace(**{a: _value(r) for a, r in rec["attrs"].items()})
        for a in rec["absent"]:
            assert not hasattr(env, a), a
        env.action_space = types.SimpleNamespace(spaces=_space(rec["action_space"]))
        env.observation_space = types.SimpleNamespace(spaces=_space(rec["observation_space"]))
        return env
    return types.SimpleNamespace(make_env=make_env, recs=recs)


def test_the_fixture_holds_the_reference_types(ref_instances):
    """The stand-in carries what the reference's instance carried: NumPy int64 masks, a float32 home pose, `None` for an absent arm."""
    for env_id in IDS:
        e = ref_instances.make_env(env_id)
        assert type(e.q_pos_home) is np.ndarray and e.q_pos_home.dtype == np.float32, env_id
        assert type(e.q_id_r_mask) is np.ndarray and e.q_id_r_mask.dtype == np.int64, env_id
        assert type(e.ctrl_id_r_grip) is np.ndarray and e.ctrl_id_r_grip.dtype == np.int64, env_id
        assert (e.q_id_l_mask is None) == (e.ctrl_id_l_grip is None) == (ENV_SPECS[env_id].q_id_l_mask is None), env_id


@pytest.mark.parametrize("env_id", IDS)
def test_reference_instance_compiles_to_the_registered_model(ref_instances, env_id):
    ref_env = ref_instances.make_env(env_id)
    spec = env_hip.spec_from_gym_env(ref_env)
    cm, cm0 = compile_model(spec), compile_model(ENV_SPECS[env_id])
    assert bytes(cm.desc) == bytes(cm0.desc)                                 # what kmanip_create receives
    for f in ("asset", "obs_list", "act_list", "q_id_r_mask", "q_id_l_mask", "ctrl_id_r_grip", "ctrl_id_l_grip", "max_episode_steps"):
        assert getattr(spec, f) == getattr(ENV_SPECS[env_id], f), f
    assert np.array_equal(spec.q_pos_home, ENV_SPECS[env_id].q_pos_home) and spec.q_pos_home.dtype == ENV_SPECS[env_id].q_pos_home.dtype

    # action columns: the flat [num_envs, act_dim] layout follows the insertion order of the reference's action Dict space
    ref_act = ref_env.action_space.spaces
    assert list(cm.act_slices) == list(ref_act)
    col = 0
    for key, sl in cm.act_slices.items():
        assert (sl.start, sl.stop) == (col, col + ref_act[key].shape[0]), key
        col = sl.stop
    assert col == cm.act_dim == sum(b.shape[0] for b in ref_act.values())

    # observation keys: state keys in obs_list order as the reference's observation Dict holds them, then its cameras
    ref_obs = ref_env.observation_space.spaces
    mine = [k for k in cm.obs_slices if k in spec.obs_list] + ["camera/" + c for c in cm.cameras]
    ref_keys = [k if not k.startswith("camera") else "camera/" + k.split("/")[-1] for k in ref_obs]
    assert mine == ref_keys
    for k in cm.obs_slices:
        if k in ref_obs:
            assert cm.obs_slices[k].stop - cm.obs_slices[k].start == ref_obs[k].shape[0], k
    for c, (name, box) in zip(cm.cameras, [(k, b) for k, b in ref_obs.items() if k.startswith("camera")]):
        assert name.endswith(c) and box.shape == (CAMERAS[c].h, CAMERAS[c].w, 3) and box.dtype == np.uint8


def test_the_seam_reads_only_what_env_sim_reads(ref_instances):
    """spec_from_gym_env must not need an attribute the reference's instance lacks (it has no `env_id`; single-arm ids keep
    q_id_l_mask / ctrl_id_l_grip as None)."""
    ref_env = ref_instances.make_env("KManipSoloArm")
    assert "env_id" in ref_instances.recs["KManipSoloArm"]["absent"] and not hasattr(ref_env, "env_id")
    spec = env_hip.spec_from_gym_env(ref_env)
    assert spec.env_id == "custom" and spec.q_id_l_mask is None and spec.ctrl_id_l_grip is None
    assert env_hip.MJCF_TO_ASSET[ref_env.mjcf_filename] == "solo_arm"
