"""The edges of kmanip_actor on the device (run with -m gpu on an MI355X): the mean at the shapes of test_actor_edges_cpu.SHAPES --
input tiles full, empty or of one column, output lane groups full or empty, padded K groups, NT = 16 by either hidden size -- and with
each of the four normalisation settings, against NumPy float64 within test_actor_edges_cpu.BAR; the Gaussian head at out_dim 1, 5
and 16 against its definition; Actor.from_module.  All on test_actor_gpu's KManipSoloArm handle of 33 envs.  The gradient kernels'
edges are in test_actor_edges_grad_gpu.py.  What the device showed: DESIGN.md section 47."""
import copy

import numpy as np
import pytest

import test_actor_cpu as AC
from test_actor_edges_cpu import BAR, NS, SHAPES, forward_cases, forward_obs, normed
from test_actor_gpu import N, OFFSET, SEED, _handle, _torch

pytestmark = pytest.mark.gpu
_ACTORS = {}


def _edge_actor(shape, norm="both", cache=True):
    """(env, an Actor of (in_dim, hidden, out_dim, activation) with test_actor_cpu.network's distinct weights and the normalisation
    setting `norm`, those weights as `normed` gives them): made once per (shape, norm) unless the test changes the parameters."""
    from gym_kmanip_amd.actor import Actor
    torch = _torch()
    if not cache or (shape, norm) not in _ACTORS:
        env, (in_dim, hidden, od, activation) = _handle("KManipSoloArm")[0], shape
        a = Actor(env, hidden=hidden, activation=activation, out_dim=od, in_dim=in_dim)
        assert a.obs_mean is None and a.obs_inv_std is None                      # the default every user starts with
        net = normed(AC.network(in_dim, hidden, od), norm)
        for k in ("w0", "b0", "w1", "b1", "w2", "b2", "log_std"):
            getattr(a, k).copy_(torch.from_numpy(net[k]).to(env.device))
        if norm in ("both", "mean"):
            a.obs_mean = torch.from_numpy(net["obs_mean"]).to(env.device)
        if norm in ("both", "inv_std"):
            a.obs_inv_std = torch.from_numpy(net["obs_inv_std"]).to(env.device)
        a.repack()
        if not cache:
            return env, a, net
        _ACTORS[shape, norm] = env, a, net
    return _ACTORS[shape, norm]


@pytest.mark.parametrize("shape,norm", forward_cases(), ids=str)
def test_the_mean_of_the_edge_shapes_meets_the_float32_bar_against_float64(shape, norm):
    """n = 1, 16 (exactly one tile) and 33 rows; the reference is NumPy float64 (mean_of), and Actor.reference -- whose obs_mean /
    obs_inv_std branches are the kernel's -- must be that too."""
    torch = _torch()
    env, a, net = _edge_actor(shape, norm)
    obs64 = forward_obs(shape[0])
    obs, want = torch.from_numpy(obs64).to(env.device), AC.mean_of(net, obs64, shape[3], np.float64)
    assert float(np.abs(a.reference(obs)["mean"].cpu().numpy() - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))
    for n in NS:
        got = env.actor_eval(a, obs[:n].contiguous(), deterministic=True)
        assert not got["status"].any() and tuple(got["mean"].shape) == (n, shape[2])
        err = float(np.abs(got["mean"].cpu().numpy().astype(np.float64) - want[:n]).max())
        print("\n%s %s n=%d: device %.3e (bar %.1e, max|mean| %.2f)" % (shape, norm, n, err, BAR, float(np.abs(want[:n]).max())))
        assert err <= BAR


def test_a_zero_row_of_w2_gives_exactly_its_bias():
    """out_dim 5: output 1 (inside lane group 0) and output 4 (the only one of lane group 1) with zero weights; the accumulator starts
    at the bias and every product is a zero."""
    torch = _torch()
    shape = SHAPES[2]
    assert shape[2] == 5
    env, a, net = _edge_actor(shape, "none", cache=False)
    a.w2[[1, 4]] = 0.0
    a.repack()
    net = dict(net, w2=net["w2"].copy())
    net["w2"][[1, 4]] = 0.0
    obs64 = forward_obs(shape[0])
    got = env.actor_eval(a, torch.from_numpy(obs64).to(env.device), deterministic=True)["mean"].cpu().numpy()
    for j in (1, 4):
        assert net["b2"][j] != 0 and np.array_equal(got[:, j], np.full(N, net["b2"][j], dtype=np.float32)), j
    assert float(np.abs(got - AC.mean_of(net, obs64, shape[3], np.float64)).max()) <= BAR


@pytest.mark.parametrize("out_dim", [1, 5, 16])
def test_the_head_is_its_definition_at_other_widths(out_dim):
    """test_actor_gpu.test_the_head_is_its_definition's checks with one output (three lanes of group 0 idle), five and sixteen."""
    from gym_kmanip_amd import model
    from gym_kmanip_amd.actor import Actor
    torch = _torch()
    env, obs = _handle("KManipSoloArm")
    a = Actor(env, hidden=(64, 32), activation="tanh", out_dim=out_dim)
    net = AC.network(a.in_dim, (64, 32), out_dim)
    for k, v in net.items():
        t = torch.from_numpy(v).to(env.device)
        setattr(a, k, t) if k.startswith("obs_") else getattr(a, k).copy_(t)
    a.repack()
    got = env.actor_eval(a, obs)
    st = {k: v.cpu().numpy() for k, v in env.state_tensors().items()}
    assert st["step"].min() == 3 and tuple(got["noise"].shape) == (N, out_dim)
    want = np.stack([model.draw_policy_noise(SEED, OFFSET + e, st["episode"][e], st["step"][e], out_dim) for e in range(N)])
    noise, mean = got["noise"].cpu().numpy(), got["mean"].cpu().numpy()
    ulps = np.abs(noise.view(np.int32).astype(np.int64) - want.view(np.int32))
    raw = mean + np.exp(net["log_std"].astype(np.float64)).astype(np.float32) * noise
    print("\nout_dim %d: noise bit-equal %.4f, worst %d ulp; %d of %d |raw| > 1" % (out_dim, float((ulps == 0).mean()), ulps.max(),
                                                                                 int((np.abs(raw) > 1).sum()), raw.size))
    assert ulps.max() <= 1 and (ulps == 0).mean() >= 0.99
    assert raw.dtype == np.float32 and np.array_equal(got["raw"].cpu().numpy(), raw)
    assert np.array_equal(got["act"].cpu().numpy(), np.clip(raw, -1.0, 1.0)) and (out_dim == 1 or (np.abs(raw) > 1).any())
    ref = a.reference(obs, noise=got["noise"])["logp"]
    assert float(((got["logp"] - ref).abs() / ref.abs()).max()) <= 1e-12 * out_dim
    assert torch.equal(env.actor_eval(a, obs, deterministic=True)["mean"], got["mean"])


def _module(activation):
    """A torch.nn.Sequential 27 -> 64 -> 32 -> 7 holding test_actor_cpu.network's weights (no draw from torch's global generator)."""
    torch = _torch()
    nn = torch.nn
    act = nn.Tanh if activation == "tanh" else nn.ReLU
    m = nn.Sequential(nn.Linear(27, 64), act(), nn.Linear(64, 32), act(), nn.Linear(32, 7))
    net = AC.network(27, (64, 32), 7)
    with torch.no_grad():
        for l, lin in enumerate(m[::2]):
            lin.weight.copy_(torch.from_numpy(net["w%d" % l]))
            lin.bias.copy_(torch.from_numpy(net["b%d" % l]))
    return m


@pytest.mark.parametrize("activation", AC.ACTIVATIONS)
def test_from_module_is_the_module(activation):
    """The module runs in float64 on the CPU on the float32-rounded input; (27, (64, 32), 7) is one of test_actor_cpu's measured shapes."""
    from gym_kmanip_amd.actor import Actor
    torch = _torch()
    env, obs = _handle("KManipSoloArm")
    m = _module(activation)
    a = Actor.from_module(env, m.to(env.device))
    assert (a.in_dim, a.hidden, a.out_dim, a.activation) == (27, (64, 32), 7, activation) and a.obs_mean is None and a.obs_inv_std is None
    assert all(torch.equal(getattr(a, "w%d" % l), lin.weight) and torch.equal(getattr(a, "b%d" % l), lin.bias) for l, lin in enumerate(m[::2]))
    with torch.no_grad():
        want = copy.deepcopy(m).cpu().double()(obs.cpu().float().double())
    got = env.actor_eval(a, obs, deterministic=True)["mean"]
    err = float((got.cpu().double() - want).abs().max())
    print("\nfrom_module %s: device %.3e (bar %.1e)" % (activation, err, AC.BAR))
    assert err <= AC.BAR


def test_from_module_refuses_what_is_no_three_layer_mlp():
    from gym_kmanip_amd.actor import Actor
    nn = _torch().nn
    env = _handle("KManipSoloArm")[0]
    bad = {"two layers": nn.Sequential(nn.Linear(27, 64), nn.Tanh(), nn.Linear(64, 7)),
           "mixed activations": nn.Sequential(nn.Linear(27, 64), nn.Tanh(), nn.Linear(64, 32), nn.ReLU(), nn.Linear(32, 7)),
           "no bias": nn.Sequential(nn.Linear(27, 64), nn.Tanh(), nn.Linear(64, 32, bias=False), nn.Tanh(), nn.Linear(32, 7))}
    for what, m in bad.items():
        with pytest.raises(ValueError, match="from_module"):
            Actor.from_module(env, m)
        print("refused: %s" % what)
