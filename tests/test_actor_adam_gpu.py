"""kmanip_actor_adam on the device (run with -m gpu on an MI355X): KManipEnvHip.actor_adam against test_ppo_update_cpu.adam_reference,
the header's step in NumPy float64, and both packed buffers bit for bit against what kmanip_actor_pack and kmanip_actor_grad_pack write
into fresh buffers from the updated tensors.  The shapes are the layout's corners: rows of 27 and 49 floats (no 16-byte access, a last
K-block of 11 columns and one of a single column), 5 x 3 and 9 x 13 tiles (no multiples of KM_ACTOR_KGROUP), full tiles everywhere, and
the critic.  What the device showed: DESIGN.md section 48."""
import ctypes as C

import numpy as np
import pytest

from test_actor_gpu import _handle, _torch
from test_ppo_update_cpu import NAMES, adam_reference

pytestmark = pytest.mark.gpu
SHAPES = [(27, (64, 64), 7), (49, (80, 48), 13), (64, (144, 208), 16), (27, (16, 16), 1)]
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.99, eps=1e-8)


def _actor(shape, seed=3):
    from gym_kmanip_amd.actor import Actor
    env, (in_dim, hidden, od) = _handle("KManipSoloArm")[0], shape
    a = Actor(env, hidden=hidden, out_dim=od, in_dim=in_dim, seed=seed)
    a.log_std.copy_(_torch().linspace(-1.0, 0.2, od))
    return env, a


def _fresh_packs(env, a):
    """(packed, packed_t) as the two pack calls write them from the tensors as they are, into buffers of their own."""
    from gym_kmanip_amd import lib as klib
    torch = _torch()
    wt = klib.KActorWeights(**{nm: getattr(a, nm).data_ptr() for nm in NAMES[:6]})
    pk, pkt = torch.full_like(a.packed, 7.0), torch.full_like(a.packed_t, 7.0)
    assert env.L.kmanip_actor_pack(env.h, C.byref(a.desc), C.byref(wt), C.c_void_p(pk.data_ptr()), env._stream()) == 0
    assert env.L.kmanip_actor_grad_pack(env.h, C.byref(a.desc), C.byref(wt), C.c_void_p(pkt.data_ptr()), env._stream()) == 0
    return pk, pkt


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("clip", ["below", "above", None])
@pytest.mark.parametrize("log_std", [True, False])
def test_three_steps_match_float64_and_the_packed_buffers_a_repack(shape, clip, log_std):
    torch = _torch()
    env, a = _actor(shape)
    names = NAMES if log_std else NAMES[:6]
    rng = np.random.default_rng(shape[0] + shape[2])
    p = {k: getattr(a, k).cpu().numpy() for k in NAMES}
    m, v = ({k: np.zeros_like(p[k]) for k in NAMES} for _ in range(2))
    off = np.cumsum([0] + [p[k].size for k in NAMES])
    max_norm = {"below": 1.0, "above": 1e6, None: None}[clip]
    differ = total = 0
    for step in (1, 2, 3):
        g = {k: rng.normal(0.0, 1.0, p[k].shape).astype(np.float32) for k in names}
        gnorm = env.actor_adam(a, HYPER["lr"], (HYPER["beta1"], HYPER["beta2"]), HYPER["eps"], max_grad_norm=max_norm,
                               grads={k: torch.from_numpy(x).to(env.device) for k, x in g.items()}, log_std=log_std)
        p, m, v, norm = adam_reference(p, g, m, v, step, max_grad_norm=max_norm, **HYPER)
        assert (norm > 1.0) and abs(float(gnorm) - norm) <= 1e-12 * norm and a.adam_step == step
        state = a.adam_state.cpu().numpy()
        for i, k in enumerate(NAMES):
            got = (getattr(a, k).cpu().numpy().ravel(), state[off[i]:off[i + 1]], state[off[-1] + off[i]:off[-1] + off[i + 1]])
            for x, ref in zip(got, (p[k].ravel(), m[k].ravel(), v[k].ravel())):
                assert np.all(np.abs(x - ref) <= np.spacing(np.abs(ref))), (k, step)
                differ, total = differ + int((x != ref).sum()), total + ref.size
            p[k], m[k], v[k] = (x.reshape(p[k].shape).copy() for x in got)             # the next step starts from the device's bits
        pk, pkt = _fresh_packs(env, a)
        assert torch.equal(a.packed, pk) and torch.equal(a.packed_t, pkt), step
    print("\n%s clip=%s log_std=%s: %d of %d entries of p, m, v not bit-equal" % (shape, clip, log_std, differ, total))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_zero_learning_rate_keeps_every_byte(shape):
    torch = _torch()
    env, a = _actor(shape)
    before = [getattr(a, k).clone() for k in NAMES] + [a.packed.clone(), a.packed_t.clone()]
    gen = torch.Generator().manual_seed(5)
    env.actor_adam(a, 0.0, max_grad_norm=0.5, grads={k: torch.randn(getattr(a, k).shape, generator=gen).to(env.device) for k in NAMES})
    after = [getattr(a, k) for k in NAMES] + [a.packed, a.packed_t]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, after)) and bool(a.adam_state.any())


@pytest.mark.parametrize("bad", ["handle", "desc", "in", "params", "hidden 40", "gw1", "b2", "glog_std only", "log_std only", "step 0", "lr nan",
                                 "beta1 1", "beta2 <0", "eps 0", "eps inf", "state NULL", "state +4", "packed NULL", "packed_t +8", "workspace NULL"])
def test_actor_adam_refuses(bad):
    from gym_kmanip_amd import lib as klib
    torch = _torch()
    env, a = _actor(SHAPES[0])
    grads = {k: torch.ones_like(getattr(a, k)) for k in NAMES}
    ai = klib.KActorAdamIn(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0, step=1)
    pr = klib.KActorParams()
    for k in NAMES:
        setattr(ai, "g" + k, None if bad == "g" + k or (bad == "log_std only" and k == "log_std") else grads[k].data_ptr())
        setattr(pr, k, None if bad == k or (bad == "glog_std only" and k == "log_std") else getattr(a, k).data_ptr())
    field, value = {"step 0": ("step", 0), "lr nan": ("lr", float("nan")), "beta1 1": ("beta1", 1.0), "beta2 <0": ("beta2", -0.1),
                    "eps 0": ("eps", 0.0), "eps inf": ("eps", float("inf"))}.get(bad, ("step", 1))
    setattr(ai, field, value)
    desc = klib.KActorDesc(27, (C.c_int32 * 2)(64, 40), 7, 0) if bad == "hidden 40" else a.desc
    state = torch.zeros((env.L.kmanip_actor_adam_state_floats(C.byref(a.desc)),), dtype=torch.float32, device=env.device)
    ws = torch.zeros((klib.KM_ACTOR_ADAM_WS_DOUBLES,), dtype=torch.float64, device=env.device)
    sp = {"state NULL": None, "state +4": state.data_ptr() + 4}.get(bad, state.data_ptr())
    pp = None if bad == "packed NULL" else a.packed.data_ptr()
    tp = a.packed_t.data_ptr() + (8 if bad == "packed_t +8" else 0)
    rc = env.L.kmanip_actor_adam(None if bad == "handle" else env.h, None if bad == "desc" else C.byref(desc), None if bad == "in" else C.byref(ai),
                                 None if bad == "params" else C.byref(pr), C.c_void_p(sp), C.c_void_p(pp), C.c_void_p(tp),
                                 None if bad == "workspace NULL" else C.c_void_p(ws.data_ptr()), None, env._stream())
    assert rc != 0 and b"kmanip_actor_adam" in env.L.kmanip_last_error(None if bad == "handle" else env.h)
    torch.cuda.synchronize()
    assert not state.any()                     # nothing was launched: a step would have left moments
