"""gym_kmanip_amd.ppo.PPO on the device (run with -m gpu on an MI355X): two iterations on 33 envs, T = 4, two minibatches.  The same
seeds give the same bytes, and the packed copy the kernels read has not drifted from the torch tensors: after the updates actor_eval's
mean meets Actor.reference within test_actor_cpu's BAR, with no repack() anywhere in the loop."""
import pytest

from test_actor_cpu import BAR
from test_actor_gpu import _make, _torch

pytestmark = pytest.mark.gpu


def _run():
    from gym_kmanip_amd.actor import Actor
    from gym_kmanip_amd.ppo import PPO
    env = _make("KManipSoloArm")
    actor, critic = Actor(env, hidden=(64, 64), seed=1), Actor(env, hidden=(80, 48), out_dim=1, seed=2)
    ppo = PPO(env, actor, critic, nsteps=4, epochs=2, minibatches=2, lr=1e-3, seed=7)
    return env, actor, critic, ppo, [ppo.iterate() for _ in range(2)]


def test_two_iterations_are_reproducible_finite_and_leave_the_packed_copy_current():
    torch = _torch()
    (env, actor, critic, ppo, res), (_, actor2, critic2, _, res2) = _run(), _run()
    for a, b in ((actor, actor2), (critic, critic2)):
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
        assert torch.equal(a.packed, b.packed) and torch.equal(a.packed_t, b.packed_t) and torch.equal(a.adam_state, b.adam_state)
        assert a.adam_step == 8 and all(bool(torch.isfinite(p).all()) for p in a.parameters())
    for r, r2 in zip(res, res2):
        assert all(torch.equal(r[k], r2[k]) and bool(torch.isfinite(r[k]).all()) for k in r) and r["policy_loss"].shape == (2, 2)
    assert not torch.equal(actor.w0, type(actor)(env, hidden=(64, 64), seed=1).w0)              # the parameters did move
    obs = ppo.buf["obs"][0]
    for net in (actor, critic):
        got = env.actor_eval(net, obs, deterministic=True)
        err = float((got["mean"].double() - net.reference(obs)["mean"]).abs().max())
        print("\nmean after the updates: worst |device - float64| %.3e" % err)
        assert not got["status"].any() and err <= BAR
