"""kmanip_actor_grad on the device (run with -m gpu on an MI355X): KManipEnvHip.actor_grad against Actor.loss_reference, the same loss
in torch float64 under autograd, within test_actor_grad_cpu's BAR relative to each tensor's max|g64|; what compares the kernels with
themselves is bit for bit.  One handle of 33 envs; the records are test_actor_grad_cpu.inputs'.  What the device showed: DESIGN.md
section 46."""
import ctypes as C

import pytest

import test_actor_cpu as AC
from test_actor_grad_cpu import BAR, CASES, CLIP, HEADS, NREC, ROWS, inputs
from test_actor_gpu import _handle, _torch

pytestmark = pytest.mark.gpu
_CASE = {}


def _new_actor(shape, activation):
    """(env, an Actor of the shape with test_actor_cpu.network's distinct weights, those weights)."""
    from gym_kmanip_amd.actor import Actor
    torch = _torch()
    env, (in_dim, hidden, od) = _handle("KManipSoloArm")[0], shape
    a = Actor(env, hidden=hidden, activation=activation, out_dim=od, in_dim=in_dim)
    net = AC.network(in_dim, hidden, od)
    for k, v in net.items():
        t = torch.from_numpy(v).to(env.device)
        setattr(a, k, t) if k.startswith("obs_") else getattr(a, k).copy_(t)
    a.repack()
    return env, a, net


def _case(shape, activation):
    """(env, actor, the records as device tensors) of a network shape: made once, the parameters never changed."""
    if (shape, activation) not in _CASE:
        env, a, net = _new_actor(shape, activation)
        _CASE[shape, activation] = env, a, {k: _torch().from_numpy(v).to(env.device) for k, v in inputs(net, *shape[::2], activation).items()}
    return _CASE[shape, activation]


def _head(rec, head):
    return {"given": dict(g=rec["g"]), "mse": dict(target=rec["target"]), "ppo": dict(ppo=dict(raw=rec["raw"], logp_old=rec["logp_old"], adv=rec["adv"], clip=CLIP))}[head]


@pytest.mark.parametrize("shape", CASES, ids=str)
@pytest.mark.parametrize("activation", AC.ACTIVATIONS)
@pytest.mark.parametrize("head", HEADS)
def test_the_gradients_meet_the_float32_bar_against_float64_autograd(shape, activation, head):
    """n = 3, 17, 33 and 300 rows through idx (two K-splits of 160).  With these weights a wrong layout is an O(1) error."""
    torch = _torch()
    env, a, rec = _case(shape, activation)
    for rows in ROWS:
        got = env.actor_grad(a, rec["obs"], idx=rows, set_grad=False, **_head(rec, head))
        ref = a.loss_reference(rec["obs"], head, idx=rows, **_head(rec, head))
        assert not got["status"].any() and set(ref["grads"]) == set(got) - {"status", "row_loss", "logp"}
        if head == "ppo":        # THE CONDITION: no row's active / inactive decision can flip under float32 rounding; all four regimes
            pick = slice(None) if rows is None else rows
            rho, adv = (ref["logp"] - rec["logp_old"][pick]).exp(), rec["adv"][pick]
            assert float(torch.minimum((rho - (1 - CLIP)).abs(), (rho - (1 + CLIP)).abs()).min()) > 1e-3
            if rows is None:
                assert all(bool((m & sgn).any()) for m in (rho < 1 - CLIP, rho > 1 + CLIP) for sgn in (adv > 0, adv < 0))
            err = float((got["logp"] - ref["logp"]).abs().max())
            print("\nlogp: worst |device - float64| %.3e" % err)
            assert err <= BAR * a.out_dim
        if head != "given":      # row_loss inherits the mean's error through the head: relative to the largest row
            err = float((got["row_loss"] - ref["row_loss"]).abs().max() / ref["row_loss"].abs().max())
            print("row_loss: worst relative %.3e" % err)
            assert err <= BAR * a.out_dim
        for k, g64 in ref["grads"].items():
            err = float((got[k].double() - g64).abs().max() / g64.abs().max())
            print("%s %s %s n=%d %s: %.3e" % (shape, activation, head, len(rows or range(NREC)), k, err))
            assert err <= BAR, k


@pytest.mark.parametrize("head", HEADS)
def test_same_bytes_bad_rows_and_no_rows(head):
    torch = _torch()
    env, a, rec = _case(CASES[1], "tanh")
    rows = [5, 9, 9, 2, 30]
    one, two = (env.actor_grad(a, rec["obs"], idx=ROWS[3], set_grad=False, **_head(rec, head)) for _ in range(2))
    assert all(torch.equal(one[k], two[k]) for k in one)
    # a record index out of range: status 2 on that row, and the gradients of the call with the other rows in the same places
    for bad in (NREC, -1):
        got = env.actor_grad(a, rec["obs"], idx=rows + [bad], scale=0.25, set_grad=False, **_head(rec, head))
        want = env.actor_grad(a, rec["obs"], idx=rows, scale=0.25, set_grad=False, **_head(rec, head))
        assert got["status"].tolist() == [0] * 5 + [2]
        assert all(torch.equal(got[k][:5] if k in ("status", "row_loss", "logp") else got[k], want[k]) for k in want)
    out = {k: v[:0].clone() if k in ("status", "row_loss", "logp") else torch.full_like(v, 7.0) for k, v in want.items()}
    none = env.actor_grad(a, rec["obs"], idx=[], out=out, set_grad=False, **_head(rec, head))
    assert all(not v.any() for v in none.values())


def test_set_grad_makes_a_training_step():
    torch = _torch()
    rec = _case(CASES[1], "tanh")[2]
    env, a, _ = _new_actor(CASES[1], "tanh")                          # an actor of its own: this test changes the parameters
    got = env.actor_grad(a, rec["obs"], target=rec["target"])
    assert all(p.grad is got[k] for k, p in zip(("w0", "b0", "w1", "b1", "w2", "b2"), a.parameters())) and a.log_std.grad is None
    before = a.w1.clone()
    torch.optim.SGD(a.parameters(), lr=0.5).step()
    a.repack()
    assert not torch.equal(before, a.w1)
    mean = env.actor_eval(a, rec["obs"], deterministic=True)["mean"]
    assert float((mean.double() - a.reference(rec["obs"])["mean"]).abs().max()) <= AC.BAR
    after = env.actor_grad(a, rec["obs"], target=rec["target"], set_grad=False)      # the transposed copy was rebuilt as well
    ref = a.loss_reference(rec["obs"], "mse", target=rec["target"])["grads"]
    assert all(float((after[k].double() - g).abs().max() / g.abs().max()) <= BAR for k, g in ref.items())


@pytest.mark.parametrize("change", [dict(n=-1), dict(n=NREC + 1), dict(n_records=0), dict(head=3), dict(obs=None), dict(raw=None), dict(adv=None),
                                    dict(clip=0.0), dict(clip=1.0), dict(w1=None), dict(log_std_grad=None), dict(desc=(27, (24, 32), 7, 0)),
                                    dict(packed=None), dict(packed_t=4), dict(ws=None), dict(ws=4)], ids=str)
def test_refusals_launch_nothing(change):
    from gym_kmanip_amd import lib as klib
    torch = _torch()
    env, a, rec = _case(CASES[0], "tanh")
    grads = {k: torch.full_like(getattr(a, k), 7.0) for k in ("w0", "b0", "w1", "b1", "w2", "b2", "log_std")}
    ws = torch.empty((klib.actor_grad_workspace_floats(a.in_dim, a.hidden, a.out_dim, NREC),), dtype=torch.float32, device=env.device)
    args = dict(n=NREC, n_records=NREC, head=2, clip=CLIP, desc=(a.in_dim, a.hidden, a.out_dim, 0), packed=0, packed_t=0, ws=0, log_std_grad=0,
                **{k: rec[k].data_ptr() for k in ("obs", "raw", "logp_old", "adv")}, **{k: v.data_ptr() for k, v in grads.items() if k != "log_std"})
    bases = dict(packed=a.packed.data_ptr(), packed_t=a.packed_t.data_ptr(), ws=ws.data_ptr(), log_std_grad=grads["log_std"].data_ptr())

    def call(**kw):
        v = dict(args, **kw)
        ptr = {k: None if v[k] is None else bases[k] + v[k] for k in bases}             # (an offset of 4 bytes: misaligned)
        d = klib.KActorDesc(v["desc"][0], (C.c_int32 * 2)(*v["desc"][1]), v["desc"][2], v["desc"][3])
        gi = klib.KActorGradIn(head=v["head"], n_records=v["n_records"], obs=v["obs"], log_std=a.log_std.data_ptr(), raw=v["raw"], logp_old=v["logp_old"],
                               adv=v["adv"], clip=v["clip"], scale=1.0)
        dev = klib.KActorGradDev(log_std=ptr["log_std_grad"], **{k: v[k] for k in ("w0", "b0", "w1", "b1", "w2", "b2")})
        return env.L.kmanip_actor_grad(env.h, C.byref(d), ptr["packed"], ptr["packed_t"], C.byref(gi), v["n"], ptr["ws"], C.byref(dev), env._stream())

    assert call(**change) != 0 and env.L.kmanip_last_error(env.h).startswith(b"kmanip_actor_grad: ")
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in grads.values())
    assert call() == 0 and not bool((grads["w1"] == 7.0).all())
