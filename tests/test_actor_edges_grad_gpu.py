"""The edges of kmanip_actor_grad on the device (run with -m gpu on an MI355X): the K-split plan from one row to 16385 (64 splits, the
last three empty) against Actor.loss_reference within test_actor_edges_cpu.GRAD_BAR; probes of single elements, which a bar relative
to a tensor's largest entry cannot see; the forward of k_actor_bwd against k_actor's, bit for bit; and the PPO path a user runs,
collect() into actor_grad().  The records are test_actor_grad_cpu.inputs' 33.  What the device showed: DESIGN.md section 47."""
import numpy as np
import pytest

import test_actor_cpu as AC
import test_actor_grad_cpu as AG
from test_actor_edges_cpu import BAR, GRAD_BAR, GRAD_HEADS, GRAD_NS, GRAD_SHAPES, forward_obs, grad_rows
from test_actor_edges_gpu import _edge_actor
from test_actor_gpu import _actor, _handle, _make, _torch
from test_actor_grad_gpu import _case, _head

pytestmark = pytest.mark.gpu
CLIP, NREC = AG.CLIP, AG.NREC
PROBES = [((49, (80, 48), 13), "tanh"), ((64, (64, 64), 16), "tanh"), ((49, (80, 48), 13), "relu")]      # NT = 16, NT = 4, and relu
R0, R1 = 5, 22                   # the records the probes use
_PROBE = {}


@pytest.mark.parametrize("n", GRAD_NS)
@pytest.mark.parametrize("act_head", GRAD_HEADS, ids="-".join)
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=str)
def test_the_k_split_plan_meets_the_float32_bar_against_float64_autograd(shape, act_head, n):
    """Rows (7 r + 3) % 33 through idx.  n = 1, 16 and 256 are one split: a reduce that loses a split other than the only one passes
    there and fails from n = 257 up (two splits, the second with 128 of its 144 rows).  n = 16385 RUNS EMPTY SPLITS: the clamp of
    k_actor_wgrad, its zero partials, and the reduce's sum over them."""
    from gym_kmanip_amd import lib as klib
    torch = _torch()
    (activation, head), rows = act_head, grad_rows(n)
    np_, splits, length = klib.actor_grad_splits(n)
    held = [max(0, min(np_, (s + 1) * length) - s * length) for s in range(splits)]
    assert sum(held) == np_ and splits == {1: 1, 16: 1, 256: 1, 257: 2, 4096: 16, 16385: 64}[n]
    if n == 16385:
        assert (np_, splits, length) == (16400, 64, 272) and held == [272] * 60 + [80] + [0] * 3
    env, a, rec = _case(shape, activation)
    got = env.actor_grad(a, rec["obs"], idx=rows, set_grad=False, **_head(rec, head))
    ref = a.loss_reference(rec["obs"], head, idx=rows, **_head(rec, head))
    assert tuple(got["status"].shape) == (n,) and not got["status"].any() and set(ref["grads"]) == set(got) - {"status", "row_loss", "logp"}
    if head == "ppo":            # THE CONDITION of test_actor_grad_gpu: no row's active / inactive decision can flip under float32 rounding
        rho = (ref["logp"] - rec["logp_old"][rows]).exp()
        assert float(torch.minimum((rho - (1 - CLIP)).abs(), (rho - (1 + CLIP)).abs()).min()) > 1e-3
        assert float((got["logp"] - ref["logp"]).abs().max()) <= AG.BAR * a.out_dim
    if head != "given":
        assert float((got["row_loss"] - ref["row_loss"]).abs().max() / ref["row_loss"].abs().max()) <= AG.BAR * a.out_dim
    for k, g64 in ref["grads"].items():
        err = float((got[k].double() - g64).abs().max() / g64.abs().max())
        print("%s %s %s n=%d %s: %.3e (bar %.1e)" % (shape, activation, head, n, k, err, GRAD_BAR))
        assert err <= GRAD_BAR, k


def _probe(shape, activation):
    """(env, actor, the network, the records as arrays, as device tensors) of a probe shape, both normalisation vectors set."""
    if (shape, activation) not in _PROBE:
        env, a, net = _edge_actor((shape[0], shape[1], shape[2], activation), "both")
        rec = AG.inputs(net, shape[0], shape[2], activation)
        _PROBE[shape, activation] = env, a, net, rec, {k: _torch().from_numpy(v).to(env.device) for k, v in rec.items()}
    return _PROBE[shape, activation]


def _forward64(net, obs, activation):
    """x (the float32-rounded normalised input), the pre-activations and the activations of both hidden layers, in NumPy float64."""
    f = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0))
    x = ((obs - net["obs_mean"]) * net["obs_inv_std"]).astype(np.float32)
    z1 = x.astype(np.float64) @ net["w0"].T.astype(np.float64) + net["b0"]
    z2 = f(z1) @ net["w1"].T.astype(np.float64) + net["b1"]
    return x, z1, f(z1), z2, f(z2)


@pytest.mark.parametrize("shape,activation", PROBES, ids=str)
def test_one_row_and_a_unit_cotangent_leave_h2_in_one_row_of_w2(shape, activation):
    """GIVEN head, scale 1, one row, g = e_j for j = 0 and out_dim - 1: b2's gradient is e_j, w2's is zero but for row j, and row j is
    the kernel's h2, element by element against float64 (|h| <= 1 with tanh; relative to max|h2| with relu).  With relu a unit whose
    float64 pre-activation is negative by more than the bar has exactly zero gradients: no rounding flips it."""
    torch = _torch()
    env, a, net, rec, dev = _probe(shape, activation)
    od = shape[2]
    x, z1, h1, z2, h2 = _forward64(net, rec["obs"][R0], activation)
    for j in (0, od - 1):
        g = torch.zeros((NREC, od), dtype=torch.float32, device=env.device)
        g[R0, j] = 1.0
        got = {k: v.cpu().numpy() for k, v in env.actor_grad(a, dev["obs"], g=g, idx=[R0], scale=1.0, set_grad=False).items()}
        for k, g64 in a.loss_reference(dev["obs"], "given", g=g, idx=[R0], scale=1.0)["grads"].items():      # e_j through W2^T and W1^T
            assert float(np.abs(got[k] - g64.cpu().numpy()).max() / g64.abs().max()) <= AG.BAR, (j, k)
        assert got["status"].tolist() == [0] and np.array_equal(got["b2"], np.eye(od, dtype=np.float32)[j])
        assert not np.delete(got["w2"], j, axis=0).any()
        err, top = float(np.abs(got["w2"][j] - h2).max()), 1.0 if activation == "tanh" else float(np.abs(h2).max())
        print("\n%s %s j=%d: worst |w2 grad row - h2| %.3e (bar %.1e x %.2f)" % (shape, activation, j, err, BAR, top))
        assert got["w2"][j].shape == h2.shape and err <= BAR * top
        if activation == "relu":
            for z, w, b in ((z2, "w1", "b1"), (z1, "w0", "b0")):
                off = z < -BAR * max(1.0, float(np.abs(z).max()))
                assert off.any() and (~off).any() and not got[w][off].any() and not got[b][off].any()
                assert got[b][~off].any()


@pytest.mark.parametrize("shape,activation", PROBES, ids=str)
def test_one_row_makes_w0s_gradient_the_outer_product_to_the_bit(shape, activation):
    """GIVEN head, scale 1, one row, a random g: every sum has one non-zero term, so w0's gradient is float32(b0's gradient x) as
    numbers, x the float32-rounded normalised input from NumPy float64 -- all in_dim columns of it, 48 of the 49-wide shape among
    them.  THE CONDITION: no non-zero product of the float64 reference is below 1e-30 (nothing near float32's subnormals)."""
    env, a, net, rec, dev = _probe(shape, activation)
    x = _forward64(net, rec["obs"][R0], activation)[0]
    got = env.actor_grad(a, dev["obs"], g=dev["g"], idx=[R0], scale=1.0, set_grad=False)
    ref = a.loss_reference(dev["obs"], "given", g=dev["g"], idx=[R0], scale=1.0)["grads"]
    prod = np.abs(ref["b0"].cpu().numpy()[:, None] * x.astype(np.float64)[None, :])
    assert prod.shape == (shape[1][0], shape[0]) and prod.any() and prod[prod > 0].min() >= 1e-30
    b0, w0 = got["b0"].cpu().numpy(), got["w0"].cpu().numpy()
    want = b0[:, None] * x[None, :]
    assert want.dtype == np.float32 and w0.shape == want.shape and np.array_equal(w0, want)
    assert b0.any() and (activation == "tanh" or (b0 == 0).any()) and np.count_nonzero(w0[:, -1]) == np.count_nonzero(b0)
    for k, g64 in ref.items():
        err = float((got[k].double() - g64).abs().max() / g64.abs().max())
        print("%s %s one row %s: %.3e" % (shape, activation, k, err))
        assert err <= AG.BAR, k


@pytest.mark.parametrize("shape,activation", PROBES, ids=str)
def test_two_rows_among_bad_indices_give_the_two_row_gradient(shape, activation):
    """n = 17: good records at positions 0 (tile 0) and 16 (the tile of one row), every other position an index out of range.  Each
    element is within the bar, relative to the tensor's largest entry, of the float64 gradient of the two rows; status is 2 on
    exactly the others."""
    env, a, net, rec, dev = _probe(shape, activation)
    idx = [R0] + [NREC if r % 2 else -1 for r in range(15)] + [R1]
    got = env.actor_grad(a, dev["obs"], g=dev["g"], idx=idx, scale=1.0, set_grad=False)
    assert got["status"].tolist() == [0] + [2] * 15 + [0]
    ref = a.loss_reference(dev["obs"], "given", g=dev["g"], idx=[R0, R1], scale=1.0)["grads"]
    for k, g64 in ref.items():
        err = (got[k].double() - g64).abs() / g64.abs().max()
        print("%s %s two rows %s: %.3e" % (shape, activation, k, float(err.max())))
        assert got[k].shape == g64.shape and bool((err <= AG.BAR).all()), k


@pytest.mark.parametrize("norm", ["both", "none"])
@pytest.mark.parametrize("shape", [(27, (64, 64), 7, "tanh"), (64, (144, 208), 16, "relu")], ids=str)
def test_k_actor_bwd_and_k_actor_agree_to_the_bit(shape, norm):
    """THIS COMPARES THE TWO KERNELS WITH EACH OTHER (each is tied to float64 elsewhere): with the MSE head and a target of zeros,
    row_loss is a float64 function of k_actor_bwd's float32 mean in a documented order -- per lane group of four outputs
    ((e0^2 + e1^2) + e2^2) + e3^2 from 0.0, then (p0 + p1) + (p2 + p3), then x 0.5 -- so it must be that function of kmanip_actor's
    mean to the bit.  NT = 4 and NT = 16, out_dim 7 and 16, 33 rows."""
    torch = _torch()
    env, a, _ = _edge_actor(shape, norm)
    od = shape[2]
    obs = torch.from_numpy(forward_obs(shape[0])).to(env.device)
    mean = env.actor_eval(a, obs, deterministic=True)["mean"].cpu().numpy().astype(np.float64)
    got = env.actor_grad(a, obs, target=torch.zeros((33, od), dtype=torch.float32, device=env.device), set_grad=False)
    p = np.zeros((4, 33))
    for j in range(od):
        p[j // 4] = p[j // 4] + mean[:, j] * mean[:, j]
    want = ((p[0] + p[1]) + (p[2] + p[3])) * 0.5
    assert not got["status"].any() and want.min() > 0 and np.array_equal(got["row_loss"].cpu().numpy(), want)


def test_collect_feeds_actor_grad():
    """collect(actor, 3) on 33 envs, its [T, N, ...] buffers flattened to 99 records, PPO with collect's own logp as logp_old, on all
    records and on a minibatch of 40 through idx: the device's logp is logp_old up to float32 (rho is 1), and every gradient, log_std's
    included, meets test_actor_grad_cpu's bar against loss_reference."""
    torch = _torch()
    env = _make("KManipSoloArm")
    env.copy_envs_from(_handle("KManipSoloArm")[0], episode=True)
    a, _ = _actor(env, (64, 32), "tanh")
    buf = env.collect(a, 3)
    obs, raw, logp_old = buf["obs"][:3].reshape(99, a.in_dim), buf["raw"].reshape(99, a.out_dim), buf["logp"].reshape(99)
    adv = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, 99).astype(np.float32)).to(env.device)
    ppo = dict(raw=raw, logp_old=logp_old, adv=adv, clip=CLIP)
    assert float(obs.std()) > 0 and not torch.equal(buf["obs"][0], buf["obs"][2])
    for idx in (None, np.random.default_rng(7).permutation(99)[:40].tolist()):
        pick = slice(None) if idx is None else idx
        got = env.actor_grad(a, obs, ppo=ppo, idx=idx, set_grad=False)
        ref = a.loss_reference(obs, "ppo", ppo=ppo, idx=idx)
        rho = (ref["logp"] - logp_old[pick]).exp()
        assert float(torch.minimum((rho - (1 - CLIP)).abs(), (rho - (1 + CLIP)).abs()).min()) > 1e-3 and float((rho - 1).abs().max()) < 1e-3
        err = float((got["logp"] - logp_old[pick]).abs().max())
        print("\ncollect -> actor_grad, n=%d: worst |logp - logp_old| %.3e (bar %.1e)" % (len(got["status"]), err, AG.BAR * a.out_dim))
        assert not got["status"].any() and err <= AG.BAR * a.out_dim
        assert float((got["row_loss"] - ref["row_loss"]).abs().max() / ref["row_loss"].abs().max()) <= AG.BAR * a.out_dim
        assert set(ref["grads"]) == {"w0", "b0", "w1", "b1", "w2", "b2", "log_std"}
        for k, g64 in ref["grads"].items():
            err = float((got[k].double() - g64).abs().max() / g64.abs().max())
            print("%s: %.3e" % (k, err))
            assert err <= AG.BAR, k
