"""kmanip_actor_bf16 on the device (run with -m gpu on an MI355X): actor_eval / collect / PPO with precision "bf16" against
Actor.reference(precision="bf16") in float64, the pack against the header's formula, the head against kmanip_actor's.  One handle of 33
envs; the shapes, cases and bars are test_actor_bf16_cpu's.  What the device showed: DESIGN.md section 49."""
import ctypes as C

import numpy as np
import pytest

import test_actor_cpu as AC
from test_actor_bf16_cpu import BAR, CASES, LOGP_BAR, NS, PPO_SHAPE, SHAPES, case_net, packed_bf16
from test_actor_gpu import N, _handle, _make, _torch

pytestmark = pytest.mark.gpu


def _actor(env, shape, activation, net):
    from gym_kmanip_amd.actor import Actor
    torch = _torch()
    a = Actor(env, hidden=shape[1], activation=activation, out_dim=shape[2], in_dim=shape[0])
    for k, v in net.items():
        t = torch.from_numpy(v).to(env.device)
        setattr(a, k, t) if k.startswith("obs_") else getattr(a, k).copy_(t)
    a.repack()
    a.repack_bf16()
    return a


def _obs(env, obs):
    return _torch().from_numpy(np.ascontiguousarray(obs, dtype=np.float64)).to(env.device)


@pytest.mark.parametrize("shape", SHAPES)
def test_small_integers_come_out_exact(shape):
    """The layout test: ReLU, every weight, bias and input a small integer, four +-1 a weight row at seeded places, so that every
    intermediate is an integer of magnitude <= 256 -- exact in bf16 and in any order of summation.  A misplaced weight or slot shows."""
    env = _handle("KManipSoloArm")[0]
    rng, dims, net = np.random.default_rng(sum(shape[1]) + shape[0]), (shape[0],) + shape[1] + (shape[2],), {}
    for l, (i, o) in enumerate(zip(dims, dims[1:])):
        w = np.zeros((o, i), np.float32)
        for r in range(o):
            w[r, rng.choice(i, min(i, 4), replace=False)] = rng.choice([-1.0, 1.0], min(i, 4))
        net["w%d" % l], net["b%d" % l] = w, rng.integers(-2, 3, o).astype(np.float32)
    obs = rng.integers(-2, 3, (N, shape[0])).astype(np.float64)
    h = obs
    for l in range(3):
        h = h @ net["w%d" % l].T.astype(np.float64) + net["b%d" % l]
        h = np.maximum(h, 0) if l < 2 else h
        assert np.array_equal(h, np.rint(h)) and np.abs(h).max() <= 256 and (l == 2 or (h > 0).mean() > 0.2)
    a = _actor(env, shape, "relu", net)
    assert np.array_equal(a.reference(_obs(env, obs), precision="bf16")["mean"].cpu().numpy(), h)
    for n in NS:
        got = env.actor_eval(a, _obs(env, obs[:n]), deterministic=True, precision="bf16")
        assert not got["status"].any() and np.array_equal(got["mean"].cpu().numpy(), h[:n].astype(np.float32))


@pytest.mark.parametrize("shape,activation,norm", CASES)
def test_the_mean_meets_the_bar_against_the_bf16_definition(shape, activation, norm):
    env = _handle("KManipSoloArm")[0]
    net, obs = case_net(shape, norm)
    a = _actor(env, shape, activation, {k: v for k, v in net.items() if norm == "both" or not k.startswith("obs_")})
    for n in NS:
        o = _obs(env, obs[:n])
        got = env.actor_eval(a, o, deterministic=True, precision="bf16")["mean"].double()
        err, cost = (float((got - a.reference(o, precision=p)["mean"]).abs().max()) for p in ("bf16", "f32"))
        print("\n%s %s %s n=%d: |device - bf16 definition| %.3e, |device - unquantised| %.3e" % (shape, activation, norm, n, err, cost))
        assert err <= BAR


@pytest.mark.parametrize("shape", SHAPES[1:3] + SHAPES[7:])
def test_the_pack_is_the_formula_with_nearest_even_rounding(shape):
    """NT = 4, an odd tile count (80: five tiles) and NT = 16; exact ties planted: 1 + 2^-8 rounds down to even, 1 + 3 2^-8 up."""
    torch = _torch()
    env, net = _handle("KManipSoloArm")[0], AC.network(*shape)
    net["w0"][0, 0], net["w1"][0, 1], net["w2"][0, 0] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)
    a = _actor(env, shape, "tanh", net)
    want = packed_bf16(net, (shape[0],) + shape[1] + (shape[2],))
    assert want[0] == 0x3F80 and 0x3F82 in want and 0xBF80 in want
    assert torch.equal(a.packed_bf16.view(torch.int16).cpu(), torch.from_numpy(want.view(np.int16)))


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_the_head_is_kmanip_actors_on_the_calls_own_mean(shape):
    torch = _torch()
    env, (net, obs) = _handle("KManipSoloArm")[0], case_net(shape, "both")
    a, o = _actor(env, shape, "tanh", net), _obs(env, obs)
    f32, got = env.actor_eval(a, o), env.actor_eval(a, o, precision="bf16")
    assert torch.equal(got["noise"], f32["noise"]) and torch.equal(got["logp"], f32["logp"]) and not torch.equal(got["mean"], f32["mean"])
    noise, mean = got["noise"].cpu().numpy(), got["mean"].cpu().numpy()
    raw = mean + np.exp(net["log_std"].astype(np.float64)).astype(np.float32) * noise
    assert raw.dtype == np.float32 and np.array_equal(got["raw"].cpu().numpy(), raw)
    assert np.array_equal(got["act"].cpu().numpy(), np.clip(raw, -1.0, 1.0)) and (np.abs(raw) > 1).any()


def test_a_row_depends_on_its_env_and_inputs_only():
    torch = _torch()
    env, (net, obs) = _handle("KManipSoloArm")[0], case_net(SHAPES[6], "both")
    a, o = _actor(env, SHAPES[6], "tanh", net), _obs(env, obs)
    full = env.actor_eval(a, o, precision="bf16")
    same = lambda got, rows: all(torch.equal(got[k], full[k][rows]) for k in full)
    rev = torch.arange(N - 1, -1, -1, device=env.device)
    assert same(env.actor_eval(a, o[rev].contiguous(), envs=rev.int(), precision="bf16"), rev)
    assert same(env.actor_eval(a, o[7:8].repeat(20, 1), envs=[7] * 20, precision="bf16"), [7] * 20)
    got = env.actor_eval(a, o[:4].contiguous(), envs=[0, N, -1, 3], precision="bf16")
    assert got["status"].tolist() == [0, 2, 2, 0]
    for k in set(got) - {"status"}:
        assert not got[k][1:3].any() and torch.equal(got[k][[0, 3]], full[k][[0, 3]]), k


def test_collect_is_the_hand_loop():
    torch = _torch()
    envs = [_make("KManipSoloArm") for _ in range(2)]
    for e in envs:
        e.copy_envs_from(_handle("KManipSoloArm")[0], episode=True)
    a = _actor(envs[0], PPO_SHAPE, "tanh", AC.network(*PPO_SHAPE))
    critic = _actor(envs[0], (27, (16, 16), 1), "relu", AC.network(27, (16, 16), 1))
    got = envs[0].collect(a, 3, critic=critic, precision="bf16")
    e, obs = envs[1], envs[1].observe()[0].clone()
    for t in range(3):
        o = e.actor_eval(a, obs, precision="bf16")
        assert torch.equal(got["value"][t], e.actor_eval(critic, obs, deterministic=True)["mean"][:, 0])
        assert all(torch.equal(got[k][t], o[k]) for k in ("act", "raw", "logp")) and torch.equal(got["obs"][t], obs)
        obs, rew, done = (v.clone() for v in e.step_flat(o["act"]))
        assert torch.equal(got["reward"][t], rew) and torch.equal(got["done"][t], done)
    assert torch.equal(got["obs"][3], obs)


def _ppo(epochs, iterations):
    from gym_kmanip_amd.ppo import PPO
    env = _make("KManipSoloArm")
    actor, critic = _actor(env, PPO_SHAPE, "tanh", AC.network(*PPO_SHAPE)), _actor(env, (27, (80, 48), 1), "tanh", AC.network(27, (80, 48), 1))
    ppo = PPO(env, actor, critic, nsteps=4, epochs=epochs, minibatches=epochs, lr=1e-3, seed=7, collect_precision="bf16")
    return actor, critic, ppo, [ppo.iterate() for _ in range(iterations)]


def test_ppo_with_a_bf16_behaviour_policy_is_reproducible_and_its_ratio_starts_near_one():
    torch = _torch()
    (actor, critic, _, res), (actor2, critic2, _, res2) = _ppo(2, 2), _ppo(2, 2)
    for a, b in ((actor, actor2), (critic, critic2)):
        assert all(torch.equal(p, q) and bool(torch.isfinite(p).all()) for p, q in zip(a.parameters(), b.parameters()))
    assert torch.equal(actor.packed_bf16, actor2.packed_bf16)
    assert all(torch.equal(r[k], r2[k]) and bool(torch.isfinite(r[k]).all()) for r, r2 in zip(res, res2) for k in r)
    # one epoch of one minibatch: its actor_grad runs before any Adam step, on the parameters the bf16 policy was rounded from
    _, _, ppo, _ = _ppo(1, 1)
    err = float((ppo.grads[0][ppo.n]["logp"] - ppo.buf["logp"].view(-1)[ppo.idx[0].long()]).abs().max())
    print("\nworst |actor_grad's logp - logp_old| in the first minibatch: %.3e" % err)
    assert 0.0 < err <= LOGP_BAR


def test_refusals_launch_nothing():
    from gym_kmanip_amd import lib as klib
    torch = _torch()
    env, (net, obs) = _handle("KManipSoloArm")[0], case_net(SHAPES[1], "both")
    a, o = _actor(env, SHAPES[1], "tanh", net), _obs(env, obs)
    mean = torch.full((N, a.out_dim), 7.0, dtype=torch.float32, device=env.device)
    dev, good = klib.KActorDev(mean=mean.data_ptr()), (a.in_dim, a.hidden, a.out_dim, 0)

    def call(desc=good, packed=a.packed_bf16.data_ptr(), obs_ptr=o.data_ptr(), n=N):
        d = klib.KActorDesc(desc[0], (C.c_int32 * 2)(*desc[1]), desc[2], desc[3])
        ai = klib.KActorIn(obs=obs_ptr, obs_mean=a.obs_mean.data_ptr(), obs_inv_std=a.obs_inv_std.data_ptr())
        return env.L.kmanip_actor_bf16(env.h, C.byref(d), packed, C.byref(ai), n, C.byref(dev), env._stream())

    assert call(n=0) == 0
    bad = [dict(desc=(a.in_dim, (24, 32), a.out_dim, 0)), dict(desc=(a.in_dim, (64, 272), a.out_dim, 0)), dict(desc=(65, a.hidden, a.out_dim, 0)),
           dict(desc=(a.in_dim, a.hidden, 17, 0)), dict(desc=(a.in_dim, a.hidden, a.out_dim, 2)), dict(obs_ptr=None), dict(packed=None),
           dict(packed=a.packed_bf16.data_ptr() + 8), dict(n=-1), dict(n=N + 1)]
    for kw in bad:
        assert call(**kw) != 0 and env.L.kmanip_last_error(env.h).startswith(b"kmanip_actor_bf16: "), kw
    wt = klib.KActorWeights(*(getattr(a, nm).data_ptr() for nm in ("w0", "b0", "w1", "b1", "w2", "b2")))
    for packed in (None, a.packed_bf16.data_ptr() + 8):
        assert env.L.kmanip_actor_bf16_pack(env.h, C.byref(a.desc), C.byref(wt), packed, env._stream()) != 0
    torch.cuda.synchronize()
    assert (mean == 7.0).all()
    assert call() == 0 and torch.equal(mean, env.actor_eval(a, o, deterministic=True, precision="bf16")["mean"])
