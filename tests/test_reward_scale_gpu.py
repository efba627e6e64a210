"""kmanip_reward_scale on the device (run with -m gpu on an MI355X): normalize.RewardScale.update over two successive calls -- so the
carried returns and the running moments matter -- against the longdouble loop over both, at test_normalize_cpu's BAR; and one PPO case
with both normalisations on.  What the device showed: DESIGN.md section 51."""
import ctypes as C

import numpy as np
import pytest

from test_actor_gpu import OFFSET, SEED, _make, _torch
from test_normalize_cpu import EPS, GAMMA, PATTERNS, SHAPES, close, reward_inputs

pytestmark = pytest.mark.gpu
_ENVS = {}


def _env(n):
    if n not in _ENVS:
        from gym_kmanip_amd import env_hip
        _ENVS[n] = env_hip.make("KManipSoloArm", num_envs=n, seed=SEED, env_id_offset=OFFSET)
    return _ENVS[n]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_two_calls_match_the_loop_over_both(shape, pattern):
    from gym_kmanip_amd.normalize import RewardScale
    torch, env = _torch(), _env(shape[1])
    a, b, hist = RewardScale(env, GAMMA, EPS), RewardScale(env, GAMMA, EPS), []
    for call in range(2):
        reward, done = reward_inputs(*shape, pattern, call)
        hist.append((reward, done))
        buf = dict(reward=torch.from_numpy(reward).to(env.device), done=torch.from_numpy(done).to(env.device))
        scaled = a.update(buf)
        assert torch.equal(scaled, b.update(buf)) and torch.equal(a.state, b.state) and torch.equal(a.stats, b.stats)      # the same bytes
        mean, var, carry = a.reference(np.concatenate([h[0] for h in hist]), np.concatenate([h[1] for h in hist]))
        state = a.state.cpu().numpy()
        assert state[0] == (call + 1) * reward.size
        for name, got, want in (("scaled", scaled.cpu().numpy(), reward / np.sqrt(var + EPS)), ("stats", a.stats.cpu().numpy(), np.array([mean, np.sqrt(var)])),
                                ("M2 / n", state[2] / state[0], var), ("carried", state[3:], carry)):
            ok, err = close(got, want)
            print("\n%s %s call %d %s: worst relative error %.2e" % (shape, pattern, call, name, err))
            assert ok, (name, err)


@pytest.mark.parametrize("bad", ["handle", "in", "reward", "done", "state", "workspace", "scaled", "T", "N", "gamma>1", "gamma nan", "eps 0", "eps inf",
                                 "odd reward", "odd state", "odd workspace", "odd scaled", "odd stats"])
def test_reward_scale_refuses(bad):
    from gym_kmanip_amd import lib as klib
    torch, env = _torch(), _env(5)
    T, N = 3, 5
    t = {k: torch.zeros((32,), dtype=torch.uint8 if k == "done" else torch.float64, device=env.device) for k in ("reward", "done", "state", "workspace", "scaled", "stats")}
    ptr = {k: None if k == bad else v.data_ptr() + (4 if bad == "odd " + k else 0) for k, v in t.items()}
    ri = klib.KRewardScaleIn(reward=ptr["reward"], done=ptr["done"], T=0 if bad == "T" else T, N=0 if bad == "N" else N,
                             gamma={"gamma>1": 1.5, "gamma nan": float("nan")}.get(bad, GAMMA), eps={"eps 0": 0.0, "eps inf": float("inf")}.get(bad, EPS))
    h = None if bad == "handle" else env.h
    rc = env.L.kmanip_reward_scale(h, None if bad == "in" else C.byref(ri), C.c_void_p(ptr["state"]), C.c_void_p(ptr["workspace"]), C.c_void_p(ptr["scaled"]),
                                   C.c_void_p(ptr["stats"]), env._stream())
    assert rc != 0 and b"kmanip_reward_scale" in env.L.kmanip_last_error(h)
    torch.cuda.synchronize()
    assert not any(bool(v.any()) for v in t.values())


def _ppo():
    from gym_kmanip_amd.actor import Actor
    from gym_kmanip_amd.ppo import PPO
    env = _make("KManipSoloArm")
    actor, critic = Actor(env, hidden=(64, 64), seed=1), Actor(env, hidden=(80, 48), out_dim=1, seed=2)
    ppo = PPO(env, actor, critic, nsteps=4, epochs=2, minibatches=2, lr=1e-3, seed=7, normalize_obs=True, normalize_reward=True)
    res, seen = [], []
    for k in range(2):
        res.append(ppo.iterate())
        seen.append(ppo.buf["obs"][:4].clone().view(-1, env.cm.obs_dim).cpu().numpy())
        assert float(ppo.obs_stats.state[0]) == float(ppo.reward_scale.state[0]) == (k + 1) * 4 * env.num_envs
        ok, err = close(ppo.obs_stats.mean.cpu().numpy(), ppo.obs_stats.reference(np.concatenate(seen))[0])
        print("\niteration %d: the running mean's worst relative error %.2e" % (k, err))
        assert ok, err
    return actor, critic, ppo, res


def test_ppo_with_both_normalisations_is_reproducible_and_counts_every_record():
    torch = _torch()
    (actor, critic, ppo, res), (actor2, critic2, ppo2, res2) = _ppo(), _ppo()
    assert actor.obs_mean is ppo.obs_stats.mean and critic.obs_inv_std is ppo.obs_stats.inv_std
    for a, b in ((actor, actor2), (critic, critic2)):
        assert all(torch.equal(p, q) and bool(torch.isfinite(p).all()) for p, q in zip(a.parameters(), b.parameters()))
        assert torch.equal(a.packed, b.packed) and torch.equal(a.packed_t, b.packed_t) and torch.equal(a.adam_state, b.adam_state)
    assert torch.equal(ppo.obs_stats.state, ppo2.obs_stats.state) and torch.equal(ppo.reward_scale.state, ppo2.reward_scale.state)
    assert all(torch.equal(r[k], r2[k]) and bool(torch.isfinite(r[k]).all()) for r, r2 in zip(res, res2) for k in r)
    assert torch.equal(res[1]["reward"], ppo.buf["reward"].mean())                 # the reported reward is the raw one
