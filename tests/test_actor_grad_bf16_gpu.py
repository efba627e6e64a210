"""kmanip_actor_grad_bf16 on the device (run with -m gpu on an MI355X): KManipEnvHip.actor_grad(precision="bf16") against
Actor.loss_reference(precision="bf16"), the definition in torch float64, within test_actor_grad_bf16_cpu's BAR relative to each
tensor's max|g64|; exact integers, the forward against kmanip_actor_bf16 and the kernels against themselves are bit for bit.  One
handle of 33 envs.  What the device showed: DESIGN.md section 50."""
import ctypes as C

import numpy as np
import pytest

import test_actor_cpu as AC
from test_actor_bf16_cpu import PPO_SHAPE, bf16
from test_actor_bf16_gpu import _actor, _obs
from test_actor_edges_cpu import forward_obs
from test_actor_edges_gpu import _edge_actor
from test_actor_grad_bf16_cpu import BAR, ROWS, SHAPES
from test_actor_grad_cpu import CLIP, HEADS, NREC
from test_actor_gpu import _handle, _make, _torch
from test_actor_grad_gpu import _case, _head

pytestmark = pytest.mark.gpu
NAMES = ("w0", "b0", "w1", "b1", "w2", "b2")


def _errors(got, ref, tag):
    """Every gradient tensor of the reference against the call's, relative to the tensor's largest entry; printed, the worst returned."""
    err = {k: float((got[k].double() - g).abs().max() / g.abs().max()) for k, g in ref["grads"].items()}
    print("\n%s: %s" % (tag, {k: "%.2e" % v for k, v in err.items()}))
    assert set(err) == set(got) - {"status", "row_loss", "logp"}
    return max(err.values())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_small_integers_come_out_bit_equal(shape):
    """The layout test: ReLU, the GIVEN head, scale 1; the weights +-1 on four circulant diagonals, biases, inputs and g small integers,
    so that every activation and every dz is an integer bf16 holds and every sum is exact in float32, in any order.  n = 1, 31, 32, 33:
    the edges of the 32-row K-step; 300 and 600 rows through idx: two and three K-splits."""
    from gym_kmanip_amd.actor import round_bf16
    torch = _torch()
    env, rng, dims, net = _handle("KManipSoloArm")[0], np.random.default_rng(shape[0]), (shape[0],) + shape[1] + (shape[2],), {}
    for l, (i, o) in enumerate(zip(dims, dims[1:])):
        w = np.zeros((o, i), np.float32)
        for off in (0, 1, 5, 11):
            w[np.arange(o), (np.arange(o) + off) % i] = rng.choice([-1.0, 1.0], o)
        net["w%d" % l], net["b%d" % l] = w, rng.integers(-2, 3, o).astype(np.float32)
    a, obs = _actor(env, shape, "relu", net), _obs(env, rng.integers(-2, 3, (NREC, shape[0])))
    g = torch.from_numpy(rng.integers(-2, 3, (NREC, shape[2])).astype(np.float32)).to(env.device)
    for rows in [list(range(n)) for n in (1, 31, 32, 33)] + [[(7 * r + 3) % NREC for r in range(n)] for n in (300, 600)]:
        ref = a.loss_reference(obs, "given", g=g, idx=rows, scale=1.0, precision="bf16")
        it = ref["inter"]
        assert all(torch.equal(round_bf16(v), v) for v in it.values()) and (len(rows) < 31 or bool(ref["grads"]["w0"].any()))
        assert all(float((it["dz%d" % (l + 1)].abs().T @ it["h%d" % l if l else "x"].abs()).max()) < 2 ** 24 for l in range(3))
        got = env.actor_grad(a, obs, g=g, idx=rows, scale=1.0, set_grad=False, precision="bf16")
        assert not got["status"].any() and all(torch.equal(got[k].double(), ref["grads"][k]) for k in NAMES), len(rows)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("activation", AC.ACTIVATIONS)
@pytest.mark.parametrize("head", HEADS)
def test_the_gradients_meet_the_bar_against_the_bf16_definition(shape, activation, head):
    torch = _torch()
    env, a, rec = _case(shape, activation)
    for rows in ROWS:
        got = env.actor_grad(a, rec["obs"], idx=rows, set_grad=False, precision="bf16", **_head(rec, head))
        ref = a.loss_reference(rec["obs"], head, idx=rows, precision="bf16", **_head(rec, head))
        if head == "ppo":        # THE CONDITION of section 46: no row's active / inactive decision can flip under rounding
            rho = (ref["logp"] - rec["logp_old"][slice(None) if rows is None else rows]).exp()
            assert float(torch.minimum((rho - (1 - CLIP)).abs(), (rho - (1 + CLIP)).abs()).min()) > 1e-3
        assert not got["status"].any() and _errors(got, ref, "%s %s %s n=%d" % (shape, activation, head, len(rows or range(NREC)))) <= BAR


@pytest.mark.parametrize("norm", ["both", "none"])
@pytest.mark.parametrize("shape", [(27, (64, 64), 7, "tanh"), (64, (144, 208), 16, "relu")], ids=str)
def test_the_forward_is_k_actor_bf16s_to_the_bit(shape, norm):
    """The MSE head with a target of zeros: row_loss is section 47's fixed-order float64 function of the kernel's float32 mean, so it
    must be that function of actor_eval(precision="bf16")'s mean to the bit.  NT = 4 and NT = 16, 33 rows."""
    torch = _torch()
    env, a, _ = _edge_actor(shape, norm)
    obs = torch.from_numpy(forward_obs(shape[0])).to(env.device)
    mean = env.actor_eval(a, obs, deterministic=True, precision="bf16")["mean"].cpu().numpy().astype(np.float64)
    got = env.actor_grad(a, obs, target=torch.zeros((33, shape[2]), dtype=torch.float32, device=env.device), set_grad=False, precision="bf16")
    p = np.zeros((4, 33))
    for j in range(shape[2]):
        p[j // 4] = p[j // 4] + mean[:, j] * mean[:, j]
    assert not got["status"].any() and np.array_equal(got["row_loss"].cpu().numpy(), ((p[0] + p[1]) + (p[2] + p[3])) * 0.5)


def test_the_learner_is_the_behaviour_policy():
    """THE POINT: collect(precision="bf16") on 33 envs, flattened to 99 records.  The bf16 call's logp is logp_old up to section 46's
    6e-5 x out_dim (the rounding of raw); the float32 call's on the same buffer is not -- run only to show that the case discriminates."""
    torch = _torch()
    env = _make("KManipSoloArm")
    env.copy_envs_from(_handle("KManipSoloArm")[0], episode=True)
    a = _actor(env, PPO_SHAPE, "tanh", AC.network(*PPO_SHAPE))
    buf = env.collect(a, 3, precision="bf16")
    obs, logp_old = buf["obs"][:3].reshape(99, a.in_dim), buf["logp"].reshape(99)
    adv = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, 99).astype(np.float32)).to(env.device)
    ppo = dict(raw=buf["raw"].reshape(99, a.out_dim), logp_old=logp_old, adv=adv, clip=CLIP)
    got, f32 = (env.actor_grad(a, obs, ppo=ppo, set_grad=False, precision=p) for p in ("bf16", "f32"))
    err, err32 = (float((o["logp"] - logp_old).abs().max()) for o in (got, f32))
    print("\nworst |logp - logp_old|: bf16 %.3e, float32 %.3e (bar %.1e)" % (err, err32, 6e-5 * a.out_dim))
    assert err <= 6e-5 * a.out_dim < err32
    assert _errors(got, a.loss_reference(obs, "ppo", ppo=ppo, precision="bf16"), "collect -> actor_grad bf16") <= BAR


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=str)
def test_the_transposed_pack_is_the_formula_with_nearest_even_rounding(shape):
    """NT = 4, five tiles and NT = 16; exact ties planted: 1 + 2^-8 rounds down to even, 1 + 3 2^-8 up."""
    torch = _torch()
    env, net = _handle("KManipSoloArm")[0], AC.network(*shape)
    net["w2"][0, 0], net["w1"][0, 1], net["w1"][1, 0] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)
    a, parts = _actor(env, shape, "tanh", net), []
    a.repack_bf16(with_t=True)
    for w in (net["w2"].T, net["w1"].T):             # layers out_dim -> hidden[1] -> hidden[0] of kmanip_actor_bf16's layout, zero biases
        (o, i), ot, ks = w.shape, w.shape[0] // 16, 2 * -(-w.shape[1] // 64)
        full = np.zeros((16 * ot, 32 * ks), np.float32)
        full[:o, :i] = w
        bits = (bf16(full).view(np.uint32) >> 16).astype(np.uint16).reshape(ot, 16, ks, 2, 4, 4)          # [t2, m, s, half, g, c]
        parts += [bits.transpose(0, 2, 4, 1, 3, 5).reshape(-1), np.zeros(32 * ot, np.uint16)]              # [t2, s, lane (g, m), half, c]
    want = np.concatenate(parts)
    assert want[0] == 0x3F80 and 0x3F82 in want and 0xBF80 in want
    assert torch.equal(a.packed_bf16_t.view(torch.int16).cpu(), torch.from_numpy(want.view(np.int16)))


@pytest.mark.parametrize("head", HEADS)
def test_same_bytes_bad_rows_and_no_rows(head):
    torch = _torch()
    env, a, rec = _case(SHAPES[1], "tanh")
    call = lambda rows, **kw: env.actor_grad(a, rec["obs"], idx=rows, set_grad=False, precision="bf16", **_head(rec, head), **kw)
    one, two = call(ROWS[2]), call(ROWS[2])
    assert all(torch.equal(one[k], two[k]) for k in one)
    rows = [5, 9, 9, 2, 30]
    got, want = call(rows + [NREC], scale=0.25), call(rows, scale=0.25)
    assert got["status"].tolist() == [0] * 5 + [2]
    assert all(torch.equal(got[k][:5] if k in ("status", "row_loss", "logp") else got[k], want[k]) for k in want)
    out = {k: v[:0].clone() if k in ("status", "row_loss", "logp") else torch.full_like(v, 7.0) for k, v in want.items()}
    assert all(not v.any() for v in call([], out=out).values())


def test_refusals():
    from gym_kmanip_amd import lib as klib
    from gym_kmanip_amd.ppo import PPO
    torch = _torch()
    env, a, rec = _case(SHAPES[0], "tanh")
    env.actor_grad(a, rec["obs"], g=rec["g"], set_grad=False, precision="bf16")
    grads = {k: torch.full_like(getattr(a, k), 7.0) for k in NAMES}
    gi = klib.KActorGradIn(head=0, n_records=NREC, obs=rec["obs"].data_ptr(), g=rec["g"].data_ptr(), scale=1.0)
    dev = klib.KActorGradDev(**{k: v.data_ptr() for k, v in grads.items()})
    good = [a.packed_bf16.data_ptr(), a.packed_bf16_t.data_ptr(), a.grad_workspace[NREC, "bf16"].data_ptr()]
    for at in range(3):
        for bad in (None, good[at] + 8):
            p = good[:at] + [bad] + good[at + 1:]
            assert env.L.kmanip_actor_grad_bf16(env.h, C.byref(a.desc), p[0], p[1], C.byref(gi), NREC, p[2], C.byref(dev), env._stream()) != 0
            assert env.L.kmanip_last_error(env.h).startswith(b"kmanip_actor_grad_bf16: ")
    wt = klib.KActorWeights(*(getattr(a, nm).data_ptr() for nm in NAMES))
    assert env.L.kmanip_actor_grad_bf16_pack(env.h, C.byref(a.desc), C.byref(wt), good[1] + 8, env._stream()) != 0
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in grads.values())
    with pytest.raises(ValueError):
        env.actor_grad(a, rec["obs"], g=rec["g"], set_grad=False, precision="fp8")
    with pytest.raises(ValueError):
        PPO(env, a, a, update_precision="bf16")


def _ppo():
    from gym_kmanip_amd.ppo import PPO
    env = _make("KManipSoloArm")
    actor, critic = _actor(env, PPO_SHAPE, "tanh", AC.network(*PPO_SHAPE)), _actor(env, (27, (80, 48), 1), "tanh", AC.network(27, (80, 48), 1))
    ppo = PPO(env, actor, critic, nsteps=4, epochs=2, minibatches=2, lr=1e-3, seed=7, collect_precision="bf16", update_precision="bf16")
    return actor, critic, [ppo.iterate() for _ in range(2)]


def test_ppo_in_bf16_is_reproducible_and_keeps_both_bf16_copies_fresh():
    torch = _torch()
    (actor, critic, res), (actor2, critic2, res2) = _ppo(), _ppo()
    for p, q in ((actor, actor2), (critic, critic2)):
        assert all(torch.equal(u, v) and bool(torch.isfinite(u).all()) for u, v in zip(p.parameters(), q.parameters()))
    assert all(torch.equal(r[k], r2[k]) and bool(torch.isfinite(r[k]).all()) for r, r2 in zip(res, res2) for k in r)
    held = actor.packed_bf16.clone(), actor.packed_bf16_t.clone()
    actor.packed_bf16.zero_(), actor.packed_bf16_t.zero_()
    actor.repack_bf16()
    assert torch.equal(actor.packed_bf16, held[0]) and torch.equal(actor.packed_bf16_t, held[1]) and bool(held[1].any())
