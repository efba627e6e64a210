"""kmanip_actor on the device (run with -m gpu on an MI355X): KManipEnvHip.actor_eval and collect against Actor.reference in float64
and the head's definition in NumPy float64.  Handles of 33 envs (three tiles of 16 rows, the last of one row), KManipSoloArm (27
inputs) and KManipDualArm (47), a few random steps in, env ids offset so that the counter's env words are not small.  The mean's bar is
test_actor_cpu's BAR as it stands; everything that compares the kernel with itself is bit for bit.  What the device showed: DESIGN.md
section 45."""
import ctypes as C

import numpy as np
import pytest

from test_actor_cpu import ACTIVATIONS, BAR, HIDDEN, IN_DIMS, mean_of, network

pytestmark = pytest.mark.gpu

N, SEED, OFFSET = 33, 11, (1 << 33) + 5
_DEV = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _make(env_id):
    from gym_kmanip_amd import env_hip
    env = env_hip.make(env_id, num_envs=N, seed=SEED, env_id_offset=OFFSET)
    env.k_reset()
    return env


def _handle(env_id):
    """(the asset's handle three random steps in, its observation): made once; the tests that step it work on a clone."""
    if env_id not in _DEV:
        env = _make(env_id)
        for _ in range(3):
            env.step_flat(env.sample_action())
        _DEV[env_id] = (env, env.obs.clone())
        assert env.cm.obs_dim == IN_DIMS[env_id]
    return _DEV[env_id]


def _actor(env, hidden, activation, out_dim=None):
    from gym_kmanip_amd.actor import Actor
    torch = _torch()
    a = Actor(env, hidden=hidden, activation=activation, out_dim=out_dim)
    net = network(a.in_dim, hidden, a.out_dim)
    for k, v in net.items():
        t = torch.from_numpy(v).to(env.device)
        setattr(a, k, t) if k.startswith("obs_") else getattr(a, k).copy_(t)
    a.repack()
    return a, net


@pytest.mark.parametrize("env_id", sorted(IN_DIMS))
@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_the_mean_meets_the_float32_bar_against_float64(env_id, hidden, activation):
    """n = 3 (a partial tile), 17 (a tile of one row) and 33 rows.  With these weights a wrong layout is an O(1) error."""
    env, obs = _handle(env_id)
    a, net = _actor(env, hidden, activation)
    for n in (3, 17, 33):
        got = env.actor_eval(a, obs[:n].contiguous(), deterministic=True)
        assert sorted(got) == ["mean", "status"] and not got["status"].any()
        err = float((got["mean"].double() - a.reference(obs[:n])["mean"]).abs().max())
        f32 = float(np.abs(mean_of(net, obs[:n].cpu().numpy(), activation, np.float32) - a.reference(obs[:n])["mean"].cpu().numpy()).max())
        print("\n%s %s %s n=%d: device %.3e, NumPy float32 %.3e" % (env_id, hidden, activation, n, err, f32))
        assert err <= BAR


@pytest.mark.parametrize("env_id", sorted(IN_DIMS))
def test_the_head_is_its_definition(env_id):
    from gym_kmanip_amd import model
    torch = _torch()
    env = _make(env_id)
    env.copy_envs_from(_handle(env_id)[0], episode=True)
    obs = env.observe()[0].clone()
    a, net = _actor(env, (64, 32), "tanh")
    got = env.actor_eval(a, obs)
    st = {k: v.cpu().numpy() for k, v in env.state_tensors().items()}
    assert st["step"].min() == 3
    want = np.stack([model.draw_policy_noise(SEED, OFFSET + e, st["episode"][e], st["step"][e], a.out_dim) for e in range(N)])
    noise, mean = got["noise"].cpu().numpy(), got["mean"].cpu().numpy()
    ulps = np.abs(noise.view(np.int32).astype(np.int64) - want.view(np.int32))
    print("\n%s: noise bit-equal %.4f, worst %d ulp" % (env_id, float((ulps == 0).mean()), ulps.max()))
    assert ulps.max() <= 1 and (ulps == 0).mean() >= 0.99
    raw = mean + np.exp(net["log_std"].astype(np.float64)).astype(np.float32) * noise
    assert raw.dtype == np.float32 and np.array_equal(got["raw"].cpu().numpy(), raw)
    assert np.array_equal(got["act"].cpu().numpy(), np.clip(raw, -1.0, 1.0)) and (np.abs(raw) > 1).any()
    ref = a.reference(obs, noise=got["noise"])["logp"]
    assert float(((got["logp"] - ref).abs() / ref.abs()).max()) <= 1e-12 * a.out_dim
    again = env.actor_eval(a, obs)
    assert all(torch.equal(got[k], again[k]) for k in got)
    env.step_flat(got["act"])
    moved = env.actor_eval(a, obs)
    assert torch.equal(moved["mean"], got["mean"]) and not (moved["noise"] == got["noise"]).any()


@pytest.mark.parametrize("hidden", [(64, 32), (256, 256)])
def test_a_row_depends_on_its_env_and_inputs_only(hidden):
    torch = _torch()
    env, obs = _handle("KManipDualArm")
    a, _ = _actor(env, hidden, "tanh")
    full = env.actor_eval(a, obs)
    same = lambda got, rows: all(torch.equal(got[k], full[k][rows]) for k in full)
    rev = torch.arange(N - 1, -1, -1, device=env.device)
    assert same(env.actor_eval(a, obs[rev].contiguous(), envs=rev.int()), rev)
    assert same(env.actor_eval(a, obs[5:6].contiguous(), envs=[5]), [5])
    assert same(env.actor_eval(a, obs[7:8].repeat(20, 1), envs=[7] * 20), [7] * 20)
    assert same(env.actor_eval(a, obs, envs=torch.arange(N)), slice(None))
    # a bad env index: status 2 and zeros in that row, the others unaffected
    got = env.actor_eval(a, obs[:4].contiguous(), envs=[0, N, -1, 3])
    assert got["status"].tolist() == [0, 2, 2, 0]
    for k in set(got) - {"status"}:
        assert not got[k][1:3].any() and torch.equal(got[k][[0, 3]], full[k][[0, 3]]), k


@pytest.mark.parametrize("with_critic", [False, True])
def test_collect_is_the_hand_loop(with_critic):
    torch = _torch()
    src = _handle("KManipSoloArm")[0]
    envs = [_make("KManipSoloArm") for _ in range(2)]
    for e in envs:
        e.copy_envs_from(src, episode=True)
    a, _ = _actor(envs[0], (64, 32), "tanh")
    critic = _actor(envs[0], (16, 16), "relu", out_dim=1)[0] if with_critic else None
    got = envs[0].collect(a, 3, critic=critic)
    e, obs, rows = envs[1], [envs[1].observe()[0].clone()], {k: [] for k in ("act", "raw", "logp", "reward", "done", "value")}
    for t in range(3):
        o = e.actor_eval(a, obs[t])
        ob, rew, done = e.step_flat(o["act"])
        obs.append(ob.clone())
        for k, v in (("act", o["act"]), ("raw", o["raw"]), ("logp", o["logp"]), ("reward", rew.clone()), ("done", done.clone())):
            rows[k].append(v)
    if with_critic:
        rows["value"] = [e.actor_eval(critic, ob, deterministic=True)["mean"][:, 0] for ob in obs]
    want = dict({k: torch.stack(v) for k, v in rows.items() if v}, obs=torch.stack(obs))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_refusals_launch_nothing():
    from gym_kmanip_amd import lib as klib
    torch = _torch()
    env, obs = _handle("KManipSoloArm")
    a, _ = _actor(env, (64, 32), "tanh")
    before = env.state_tensors()
    mean = torch.full((N, a.out_dim), 7.0, dtype=torch.float32, device=env.device)
    dev, good = klib.KActorDev(mean=mean.data_ptr()), (a.in_dim, a.hidden, a.out_dim, 0)

    def call(desc=good, packed=a.packed.data_ptr(), obs_ptr=obs.data_ptr(), n=N):
        d = klib.KActorDesc(desc[0], (C.c_int32 * 2)(*desc[1]), desc[2], desc[3])
        ai = klib.KActorIn(obs=obs_ptr, obs_mean=a.obs_mean.data_ptr(), obs_inv_std=a.obs_inv_std.data_ptr())
        return env.L.kmanip_actor(env.h, C.byref(d), packed, C.byref(ai), n, C.byref(dev), env._stream())

    assert call(n=0) == 0
    bad = [dict(desc=(a.in_dim, (24, 32), a.out_dim, 0)), dict(desc=(a.in_dim, (64, 272), a.out_dim, 0)), dict(desc=(a.in_dim, (0, 32), a.out_dim, 0)),
           dict(desc=(0, a.hidden, a.out_dim, 0)), dict(desc=(65, a.hidden, a.out_dim, 0)), dict(desc=(a.in_dim, a.hidden, 0, 0)),
           dict(desc=(a.in_dim, a.hidden, 17, 0)), dict(desc=(a.in_dim, a.hidden, a.out_dim, 2)), dict(obs_ptr=None), dict(packed=None)]
    for kw in bad:
        assert call(**kw) != 0 and env.L.kmanip_last_error(env.h).startswith(b"kmanip_actor: "), kw
    torch.cuda.synchronize()
    assert (mean == 7.0).all()
    after = env.state_tensors()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert call() == 0 and torch.equal(mean, env.actor_eval(a, obs, deterministic=True)["mean"])
