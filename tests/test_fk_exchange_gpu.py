"""The one-row step kernel's forward kinematics exchanges link frames between the lanes of an env's 16-lane group in registers
(fk_parallel, kmanip_dyn_tree.hpp: a lane gather per pointer-jumping round).  A gather reads other lanes, so what it returns
depends on which lanes of the wave are alive and where the group sits in the wave -- the things these tests vary (run with -m gpu
on an MI355X):

  N = 1, 3, 5 envs of KManipSoloArm   a partly filled wave, groups that leave the kernel at once (no env), one full wave plus one env
  KMANIP_EPB = 1, 2, 4                one, two or four envs per wave: the env's group at lane 0, 16, 32 or 48

States: every hinge drawn over its full range, both gripper slides off zero (inside their range), env 2 with every joint at exact
zero; the cube where the reset spawned it.  One control step (ten sub-steps, eleven forward kinematics passes), compared with the
oracle's step under the bars tests/test_gpu_parity.py uses for a step (qpos / obs 1e-7, qvel 1e-5, reward 1e-6; done and contact
mask bit for bit; ctrl bit for bit up to the two cases _check_ctrl names), and each env of the N = 5 run bit for bit with the same env stepped alone (N = 1, its env_id_offset).
The oracle's step is computed once for the five envs (envs are independent: a prefix of them is the smaller batch)."""
import numpy as np
import pytest

from gym_kmanip_amd.model import compile_model

pytestmark = pytest.mark.gpu

TOL_Q, TOL_V, TOL_R = 1e-7, 1e-5, 1e-6      # tests/test_gpu_parity.py
ENV = "KManipSoloArm"
NMAX, SEED, OFF = 5, 13, 40
ZERO_ENV = 2

_REF = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _reference():
    """(cm, start state of the five envs, their actions, the oracle's state / obs / reward / done / contact mask after one step)."""
    if _REF:
        return _REF["v"]
    from oracle.oracle import Oracle
    cm = compile_model(ENV)
    d, nl = cm.desc, cm.nlink
    orc = Oracle(cm, NMAX, seed=SEED, env_id_offset=OFF)
    orc.reset()
    qpos, qvel, ctrl, warm, step = orc.get_state()
    rng = np.random.default_rng(20250)
    slides = [j for j in range(nl) if d.jnt_type[j] == 1]
    assert len(slides) == 2
    for e in range(NMAX):
        for j in range(nl):
            lo, hi = d.jnt_range[j][0], d.jnt_range[j][1]
            if d.jnt_type[j] == 1:
                qpos[e, j] = lo + (hi - lo) * rng.uniform(0.25, 0.95)      # off zero, inside the range
                assert qpos[e, j] != 0.0
            else:
                qpos[e, j] = rng.uniform(lo, hi)
    qpos[ZERO_ENV, :nl] = 0.0
    ctrl[:, :nl] = qpos[:, :nl].astype(np.float32).astype(np.float64)
    start = (qpos.copy(), qvel.copy(), ctrl.copy(), warm.copy(), step.copy())
    act = rng.uniform(-1, 1, (NMAX, cm.act_dim)).astype(np.float32)
    orc.set_state(*start)
    obs, rew, done = orc.step(act)
    after = orc.get_state()
    mask = orc.get_diag()[0]
    _REF["v"] = (cm, start, act, after, np.array(obs), np.array(rew), np.array(done), mask)
    return _REF["v"]


def _step_device(cm, start, act, envs, off):
    """One control step of the given envs (indices into the five) in a handle of their own: (state, obs, reward, done, mask)."""
    from gym_kmanip_amd import env_hip
    torch = _torch()
    n = len(envs)
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=SEED, env_id_offset=off)
    dev.k_reset()
    dev.set_state(*[a[envs] for a in start])
    dev.step_flat(torch.from_numpy(np.ascontiguousarray(act[envs])).cuda())
    out = (dev.get_state(), dev.obs.cpu().numpy().copy(), dev.reward.cpu().numpy().copy(), dev.done.cpu().numpy().copy(), dev.get_diag()[0])
    dev.k_close()
    return out


BOUND_EPS = 1e-12


def _check_ctrl(cm, ctrl_dev, ctrl_orc):
    """ctrl as tests/test_gpu_parity.py's _cmp_state takes it for a step: bit for bit, or -- two float64 IK results either side of a
    float32 rounding boundary -- one float32 ulp apart.  One more case exists only in states like the zero env's, which START on a
    bound (joint 1's range begins at 0): the bounded trust-region IK moves such a start 1e-10 inside and then presses it back on
    the bound, where it ends at a distance that is a product of step-back factors and rounding residues (8.4e-37 rad here).  Device
    and oracle agree on that distance to six digits -- a few float32 ulps OF THE RESIDUE, 4e-43 rad -- which the one-ulp rule, made
    for entries of ordinary size, does not cover.  Both values then lie within BOUND_EPS = 1e-12 of the SAME bound, five orders
    below the 1e-7 rad the IK is held to against the oracle; that is all that is asked of such an entry."""
    d, nl = cm.desc, cm.nlink
    bad = ctrl_dev != ctrl_orc
    for e, j in zip(*np.nonzero(bad)):
        a, b = ctrl_dev[e, j], ctrl_orc[e, j]
        print("ctrl[%d, %d]: device %.17e oracle %.17e" % (e, j, a, b))
        if abs(a - b) <= float(np.spacing(np.float32(abs(b)))):
            continue
        at_bound = j < nl and any(abs(a - d.jnt_range[j][k]) <= BOUND_EPS and abs(b - d.jnt_range[j][k]) <= BOUND_EPS for k in range(2))
        assert at_bound, ("ctrl", e, j, a, b)


@pytest.mark.parametrize("epb", ["1", "2", "4"])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_one_step_from_full_range_poses_vs_oracle(n, epb, monkeypatch):
    monkeypatch.setenv("KMANIP_EPB", epb)
    cm, start, act, after, obs_o, rew_o, done_o, mask_o = _reference()
    envs = np.arange(n)
    sg, obs, rew, done, mask = _step_device(cm, start, act, envs, OFF)
    dq, dv = np.abs(sg[0] - after[0][:n]).max(), np.abs(sg[1] - after[1][:n]).max()
    do, dr = np.abs(obs - obs_o[:n]).max(), np.abs(rew - rew_o[:n]).max()
    print("\nn %d epb %s: |dqpos| %.2e |dqvel| %.2e |dobs| %.2e |dreward| %.2e" % (n, epb, dq, dv, do, dr))
    assert np.isfinite(sg[0]).all() and np.isfinite(sg[1]).all()
    assert dq < TOL_Q and dv < TOL_V and do < TOL_Q and dr < TOL_R
    _check_ctrl(cm, sg[2], after[2][:n])
    assert np.array_equal(sg[4], after[4][:n]) and np.array_equal(done, done_o[:n]) and np.array_equal(mask, mask_o[:n])


@pytest.mark.parametrize("epb", ["1", "2", "4"])
def test_env_in_a_batch_equals_the_env_alone_bit_for_bit(epb, monkeypatch):
    monkeypatch.setenv("KMANIP_EPB", epb)
    cm, start, act = _reference()[:3]
    sb, obs_b, rew_b, done_b, mask_b = _step_device(cm, start, act, np.arange(NMAX), OFF)
    for e in range(NMAX):
        s1, obs_1, rew_1, done_1, mask_1 = _step_device(cm, start, act, np.array([e]), OFF + e)
        for k in range(5):
            assert np.array_equal(sb[k][e:e + 1], s1[k]), (epb, e, k)
        assert np.array_equal(obs_b[e:e + 1], obs_1) and np.array_equal(rew_b[e:e + 1], rew_1), (epb, e)
        assert np.array_equal(done_b[e:e + 1], done_1) and np.array_equal(mask_b[e:e + 1], mask_1), (epb, e)
