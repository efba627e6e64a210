"""kmanip_gae on the device (run with -m gpu on an MI355X): KManipEnvHip.gae against test_ppo_update_cpu.gae_reference, the header's
recursion as a NumPy float64 reverse loop.  The shapes sit on either side of the time chunk (8), the wave (64) and the block (256 is
not reached by 130: two waves, one block; 65 and 130 leave a partial wave).  What the device showed: DESIGN.md section 48."""
import ctypes as C

import numpy as np
import pytest

from test_actor_gpu import _make, _torch
from test_ppo_update_cpu import gae_reference

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (2, 33), (8, 64), (9, 65), (17, 130)]
PATTERNS = ["none", "first", "last", "every", "bits"]
CASES = [(p, False) for p in PATTERNS] + [(p, True) for p in PATTERNS[1:]]
GAMMA, LAM = 0.97, 0.9
_ENV = []


def _env():
    if not _ENV:
        _ENV.append(_make("KManipSoloArm"))
    return _ENV[0]


def _inputs(T, N, pattern, with_tv):
    rng = np.random.default_rng(100 * T + N)
    reward, value = rng.normal(0.0, 1.0, (T, N)), rng.normal(0.0, 1.0, (T + 1, N)).astype(np.float32)
    tv = rng.normal(0.0, 1.0, (T, N)).astype(np.float32) if with_tv else None
    done = np.zeros((T, N), np.uint8)
    if pattern == "first":
        done[0, 0::2], done[0, 1::2] = 1, 2
    elif pattern == "last":
        done[T - 1, 0::2], done[T - 1, 1::2] = 1, 2
    elif pattern == "every":
        done[:] = 1 + (np.arange(T * N).reshape(T, N) % 3)
    elif pattern == "bits":      # a TRUNCATED step and a DIVERGED | TRUNCATED step in one column, first and last column
        done[0, 0] = done[T - 1, N - 1] = 1
        done[T - 1, 0] = done[0, N - 1] = 3 if T > 1 else 1
    return reward, done, value, tv


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("pattern,with_tv", CASES)
def test_gae_matches_the_float64_reverse_loop(shape, pattern, with_tv):
    torch, env, (T, N) = _torch(), _env(), shape
    reward, done, value, tv = _inputs(T, N, pattern, with_tv)
    a, ret, mean, std = gae_reference(reward, done, value, GAMMA, LAM, tv)
    assert std > 1e-3 or T * N == 1          # (one value has no spread: std is exactly 0 there, and its normalised advantage 0)
    dev = lambda x: None if x is None else torch.from_numpy(x).to(env.device)
    buf = dict(reward=dev(reward), done=dev(done), value=dev(value))
    for normalize in (False, True):
        got = [env.gae(buf, GAMMA, LAM, normalize=normalize, timeout_value=dev(tv)) for _ in range(2)]
        assert all(torch.equal(got[0][k], got[1][k]) for k in got[0])                    # the same call twice: the same bytes
        adv, gret, stats = (got[0][k].cpu().numpy() for k in ("adv", "ret", "stats"))
        assert np.all(np.abs(gret - ret) <= np.spacing(np.abs(ret)))
        assert abs(stats[0] - mean) <= 1e-12 * abs(mean) and abs(stats[1] - std) <= 1e-12 * std
        if not normalize:
            print("\n%s %s tv=%d: %d of %d adv and %d ret entries not bit-equal" % (shape, pattern, with_tv, (adv != a).sum(), a.size, (gret != ret).sum()))
            assert np.all(np.abs(adv - a) <= np.spacing(np.abs(a)))
        else:
            ref = ((a.astype(np.float64) - mean) / (std + 1e-8)).astype(np.float32)
            assert np.all(np.abs(adv.astype(np.float64) - ref) <= 2.0 ** -23 * np.maximum(np.abs(ref), 1.0))


def test_a_collect_buffer_goes_through_gae_into_the_ppo_head():
    from gym_kmanip_amd.actor import Actor
    torch, env = _torch(), _env()
    actor, critic = Actor(env, hidden=(64, 64), seed=1), Actor(env, hidden=(16, 16), out_dim=1, seed=2)
    buf = env.collect(actor, 3, critic=critic)
    g = env.gae(buf)
    n = 3 * env.num_envs
    got = env.actor_grad(actor, buf["obs"][:3].view(n, -1), ppo=dict(raw=buf["raw"].view(n, -1), logp_old=buf["logp"].view(-1), adv=g["adv"].view(-1), clip=0.2))
    val = env.actor_grad(critic, buf["obs"][:3].view(n, -1), target=g["ret"].view(-1, 1))
    assert not got["status"].any() and not val["status"].any()
    assert all(bool(torch.isfinite(v).all()) for v in list(got.values()) + list(val.values()) + list(g.values()))


@pytest.mark.parametrize("bad", ["handle", "in", "out", "reward", "done", "value", "adv", "ret", "workspace", "T", "N", "gamma>1", "gamma<0",
                                 "gamma nan", "lambda>1", "lambda inf"])
def test_gae_refuses(bad):
    from gym_kmanip_amd import lib as klib
    torch, env = _torch(), _env()
    T, N = 2, 33
    t = {k: torch.zeros(s, dtype=dt, device=env.device) for k, (s, dt) in dict(reward=((T, N), torch.float64), done=((T, N), torch.uint8),
         value=((T + 1, N), torch.float32), adv=((T, N), torch.float32), ret=((T, N), torch.float32), workspace=((2,), torch.float64)).items()}
    ptr = {k: None if k == bad else v.data_ptr() for k, v in t.items()}
    gi = klib.KGaeIn(reward=ptr["reward"], done=ptr["done"], value=ptr["value"], gamma={"gamma>1": 1.5, "gamma<0": -0.1, "gamma nan": float("nan")}.get(bad, 0.9))
    setattr(gi, "lambda", {"lambda>1": 1.0000001, "lambda inf": float("inf")}.get(bad, 0.9))
    out = klib.KGaeDev(adv=ptr["adv"], ret=ptr["ret"])
    rc = env.L.kmanip_gae(None if bad == "handle" else env.h, None if bad == "in" else C.byref(gi), 0 if bad == "T" else T, 0 if bad == "N" else N,
                          C.c_void_p(ptr["workspace"]), None if bad == "out" else C.byref(out), env._stream())
    assert rc != 0 and b"kmanip_gae" in env.L.kmanip_last_error(None if bad == "handle" else env.h)
    torch.cuda.synchronize()
    assert not t["adv"].any() and not t["ret"].any()
