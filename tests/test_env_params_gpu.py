"""Per-env physics parameters on the device (run with -m gpu on an MI355X): kmanip_set_env_params / _get_ / _ranges through
env_hip, against handles without parameters, against the CPU oracle of model.with_env_params, across launch shapes, and in
ranges mode against the NumPy restatement of the draw."""
import numpy as np
import pytest

from conftest import ENVS3
from gym_kmanip_amd.model import ENV_PARAMS, compile_model, draw_env_params, env_param_defaults, with_env_params

pytestmark = pytest.mark.gpu

TOL_Q = 1e-7


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _hip(cm, n, seed=0, off=0):
    from gym_kmanip_amd import env_hip
    return env_hip.KManipEnvHip(cm, num_envs=n, seed=seed, env_id_offset=off)


def _spread(cm, n, seed=0):
    """n envs over mass 0.5x-2x, friction 0.3-1.5, frictionloss 0-2x (some exactly 0) and kp scale 0.5-1.5, independently permuted."""
    d = cm.desc
    rng = np.random.default_rng(seed)
    fl = d.cube_frictionloss * np.linspace(0.0, 2.0, n)
    fl[rng.permutation(n)[: max(1, n // 8)]] = 0.0
    return {"cube_mass": d.cube_mass * np.linspace(0.5, 2.0, n)[rng.permutation(n)],
            "cube_friction": np.linspace(0.3, 1.5, n)[rng.permutation(n)],
            "cube_frictionloss": fl[rng.permutation(n)],
            "kp_scale": np.linspace(0.5, 1.5, n)[rng.permutation(n)]}


def _same(a, b, k=""):
    assert a.obs.equal(b.obs) and a.reward.equal(b.reward) and a.done.equal(b.done), k


@pytest.mark.parametrize("env,solver", [("KManipSoloArm", "newton"), ("KManipSoloArm", "pgs"), ("KManipDualArm", "newton"),
                                        ("KManipTorso", "newton")])
def test_identity_with_the_model_values(env, solver):
    """Every env set to the model's own values: the parameter kernels give the default kernels' bits (130 steps, two
    auto-resets); clear_env_params() then runs the default kernels again."""
    torch = _torch()
    cm = compile_model(env, solver=solver)
    n = 256
    a, b = _hip(cm, n, seed=3, off=11), _hip(cm, n, seed=3, off=11)
    b.set_env_params(**env_param_defaults(cm))
    a.k_reset(); b.k_reset()
    _same(a, b)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    for k in range(130):
        act = torch.rand((n, cm.act_dim), generator=gen, device="cuda") * 2 - 1
        a.step_flat(act); b.step_flat(act)
        _same(a, b, k)
        if k % 16 == 0 or k == 129:
            for x, y in zip(a.get_state(), b.get_state()):
                assert np.array_equal(x, y), k
            assert np.array_equal(a.get_diag()[0], b.get_diag()[0]), k
    assert (a.get_episode() == 2).all()                          # episodes 0, 1, 2
    p = b.get_env_params()
    for name, v in env_param_defaults(cm).items():
        assert (p[name] == v).all()
    b.clear_env_params()
    for k in range(10):
        act = torch.rand((n, cm.act_dim), generator=gen, device="cuda") * 2 - 1
        a.step_flat(act); b.step_flat(act)
        _same(a, b, ("cleared", k))
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    for name, v in env_param_defaults(cm).items():          # no parameters: get returns the model's
        assert (b.get_env_params()[name] == v).all()
    a.k_close(); b.k_close()


def _parity(env, n, check, steps, seed):
    """One-step samples: the device state of env e is loaded into an oracle of with_env_params(cm, p_e); both take the same
    action; contact mask and done byte identical, qpos within the oracle parity bar."""
    torch = _torch()
    from oracle.oracle import Oracle
    cm = compile_model(env)
    P = _spread(cm, n, seed)
    dev = _hip(cm, n, seed=seed, off=5)
    dev.set_env_params(**{k: torch.from_numpy(v) for k, v in P.items()})
    got = dev.get_env_params()
    for k, v in P.items():
        assert np.array_equal(got[k].cpu().numpy(), v)
    orcs = {e: Oracle(with_env_params(cm, **{k: v[e] for k, v in P.items()}), 1, seed=seed, env_id_offset=5 + e) for e in check}
    dev.k_reset()
    rng = np.random.default_rng(seed)
    saw_contact = saw_done = False
    flips = compared_contact = 0
    for k in range(steps):
        act = rng.uniform(-1, 1, (n, cm.act_dim)).astype(np.float32)
        sample = k % 9 == 8 or k in (63, steps - 1)        # (step 64 of an episode: the auto-reset)
        if sample:
            st0, ep0 = dev.get_state(), dev.get_episode()
        dev.step_flat(torch.from_numpy(act).cuda())
        if not sample:
            continue
        st1 = dev.get_state(); mask = dev.get_diag()[0]; done = dev.done.cpu().numpy()
        for e in check:
            o = orcs[e]
            o.set_state(*(x[e:e + 1] for x in st0)); o.set_episode(ep0[e:e + 1])
            _, _, do = o.step(act[e:e + 1])
            so = o.get_state()
            assert np.array_equal(do, done[e:e + 1]), (k, e)
            bad = so[2] != st1[2][e:e + 1]
            if bad.any():
                # a float32 ctrl flip: two float64 IK results 1e-9 apart straddle a float32 rounding boundary (test_gpu_parity
                # _cmp_state).  Every differing entry must be within one float32 ulp; the env gets that test's looser bar
                ulp = np.spacing(np.abs(so[2][bad]).astype(np.float32)).astype(np.float64)
                assert (np.abs(st1[2][e:e + 1][bad] - so[2][bad]) <= ulp).all(), ("ctrl", k, e)
                assert np.abs(so[0] - st1[0][e:e + 1]).max() < 10 * TOL_Q, (k, e)
                flips += 1
                continue
            assert np.array_equal(o.get_diag()[0], mask[e:e + 1]), (k, e)
            assert np.abs(so[0] - st1[0][e:e + 1]).max() < TOL_Q, (k, e, np.abs(so[0] - st1[0][e:e + 1]).max())
            saw_contact |= bool(mask[e] & 0xFF); saw_done |= bool(done[e])
            compared_contact += bool(mask[e])
    assert saw_contact and saw_done
    assert flips <= 2, flips                         # (a handful in 799 k samples: profiles/r03_parity_soak.txt)
    assert compared_contact >= 10, compared_contact
    dev.k_close()


@pytest.mark.parametrize("env", ENVS3)
def test_parity_heterogeneous_params_vs_oracle(env):
    _parity(env, 256, list(range(0, 256, 5)), 66, seed=2)


@pytest.mark.parametrize("env", ["KManipDualArm", "KManipTorso"])
def test_parity_heterogeneous_params_8192(env):
    """The two-arm launch of several residency rounds (cost-sorted dispatch) with parameters: an oracle slice."""
    _parity(env, 8192, list(range(0, 8192, 331)), 66, seed=4)


@pytest.mark.parametrize("env,n,epb,sort", [("KManipSoloArm", 1, None, None), ("KManipSoloArm", 5, None, None),
                                            ("KManipSoloArm", 37, "1", None), ("KManipSoloArm", 37, "2", None),
                                            ("KManipSoloArm", 300, None, None), ("KManipDualArm", 3, None, None),
                                            ("KManipDualArm", 21, "1", None), ("KManipTorso", 21, "1", None),
                                            ("KManipTorso", 33, None, None), ("KManipDualArm", 96, None, "1")])
def test_env_isolation_under_permutation(env, n, epb, sort, monkeypatch):
    """Handle B holds handle A's envs in permuted order -- parameters, state, episode and actions -- so its envs sit in other
    wave slots next to other wave-mates: every env follows its own parameters bit for bit."""
    torch = _torch()
    if epb:
        monkeypatch.setenv("KMANIP_EPB", epb)
    if sort:
        monkeypatch.setenv("KMANIP_COST_SORT", sort)
    cm = compile_model(env)
    P = _spread(cm, n, n)
    perm = np.random.default_rng(n + 1).permutation(n)
    a, b = _hip(cm, n, seed=8), _hip(cm, n, seed=8)
    a.set_env_params(**{k: torch.from_numpy(v) for k, v in P.items()})
    b.set_env_params(**{k: torch.from_numpy(v[perm]) for k, v in P.items()})
    a.k_reset()
    b.set_state(*(x[perm] for x in a.get_state())); b.set_episode(a.get_episode()[perm])
    gen = torch.Generator(device="cuda"); gen.manual_seed(n)
    tp = torch.from_numpy(perm).cuda()
    for k in range(40):
        act = torch.rand((n, cm.act_dim), generator=gen, device="cuda") * 2 - 1
        a.step_flat(act); b.step_flat(act[tp].contiguous())
        assert b.obs.equal(a.obs[tp]) and b.reward.equal(a.reward[tp]) and b.done.equal(a.done[tp]), k
    sa, sb = a.get_state(), b.get_state()
    for x, y in zip(sa, sb):
        assert np.array_equal(y, x[perm])
    assert np.array_equal(b.get_diag()[0], a.get_diag()[0][perm])
    a.k_close(); b.k_close()


def _ranges(cm):
    d = cm.desc
    return {"cube_mass": (0.5 * d.cube_mass, 2.0 * d.cube_mass), "cube_friction": (0.3, 1.5),
            "cube_frictionloss": (0.02, 0.02), "kp_scale": (0.5, 1.5)}


def _check_draw(dev, seed, off, lo, hi):
    ep = dev.get_episode()
    p = np.stack([v.cpu().numpy() for v in dev.get_env_params().values()])
    want = np.stack([draw_env_params(seed, off + e, ep[e], lo, hi) for e in range(dev.num_envs)], axis=1)
    assert np.array_equal(p, want)
    assert ((p >= lo[:, None]) & (p <= hi[:, None])).all()
    return p


def test_ranges_mode_draws_redraws_and_replays():
    torch = _torch()
    cm = compile_model("KManipSoloArm")
    n, seed, off = 128, 17, 40
    R = _ranges(cm)
    lo = np.array([R[k][0] for k in ENV_PARAMS]); hi = np.array([R[k][1] for k in ENV_PARAMS])
    a, c = _hip(cm, n, seed=seed, off=off), _hip(cm, n, seed=seed, off=off)
    for h in (a, c):
        h.set_env_param_ranges(**R)
    # before any reset the values in force are the model's
    for name, v in env_param_defaults(cm).items():
        assert (a.get_env_params()[name] == v).all()
    a.k_reset(); c.k_reset()
    p1 = _check_draw(a, seed, off, lo, hi)
    assert (p1[2] == 0.02).all() and len(np.unique(p1[0])) == n          # lo == hi pins; the others vary per env
    # a masked k_reset redraws only the selected envs
    mask = np.zeros(n, dtype=np.uint8); mask[[4, 77]] = 1
    a.k_reset(mask); c.k_reset(mask)
    p2 = _check_draw(a, seed, off, lo, hi)
    keep = mask == 0
    assert np.array_equal(p2[:, keep], p1[:, keep]) and not np.array_equal(p2[:, ~keep], p1[:, ~keep])
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    acts = torch.rand((140, n, cm.act_dim), generator=gen, device="cuda") * 2 - 1
    ck = None
    for k in range(70):                                          # auto-reset inside k_step at step 64
        a.step_flat(acts[k])
        if k == 30:
            ck = a.checkpoint()
    _check_draw(a, seed, off, lo, hi)
    assert (a.get_episode() >= 1).all()
    c.step_chunk(acts[:35]); c.step_chunk(acts[35:70])           # ... and inside step_chunk: the same values and bits
    _same(a, c)
    for x, y in zip(a.get_state(), c.get_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(np.stack([v.cpu().numpy() for v in c.get_env_params().values()]),
                          np.stack([v.cpu().numpy() for v in a.get_env_params().values()]))
    # a restored handle replays bit for bit, across the next redraw
    b = _hip(cm, n, seed=seed, off=off)
    b.restore(ck)
    for k in range(31, 140):
        b.step_flat(acts[k])
        if k >= 70:
            a.step_flat(acts[k])
    _same(a, b)
    for x, y in zip(a.checkpoint()[:6], b.checkpoint()[:6]):
        assert np.array_equal(x, y)
    _check_draw(b, seed, off, lo, hi)
    # ranges off: the drawn values stay in force through the next reset
    a.set_env_param_ranges()
    before = a.get_env_params()
    a.k_reset()
    after = a.get_env_params()
    assert all(before[k].equal(after[k]) for k in ENV_PARAMS)
    for h in (a, b, c):
        h.k_close()


def test_kp_scale_weakens_tracking():
    """Half the servo stiffness: the joints lag their targets further after a step."""
    torch = _torch()
    cm = compile_model("KManipSoloArmQPos")
    n = 64
    dev = _hip(cm, n, seed=1)
    ks = np.where(np.arange(n) < n // 2, 0.5, 1.0)
    dev.set_env_params(kp_scale=torch.from_numpy(ks))
    dev.k_reset()
    act = torch.zeros((n, cm.act_dim), device="cuda")
    act[:, cm.act_slices["q_pos_r"]] = 0.8                       # one joint-delta step for every arm joint
    dev.step_flat(act)
    qpos, _, ctrl, _, _ = dev.get_state()
    err = np.abs(ctrl[:, :7] - qpos[:, :7]).mean(axis=1)
    assert err[: n // 2].mean() > 1.05 * err[n // 2:].mean(), (err[: n // 2].mean(), err[n // 2:].mean())
    dev.k_close()


def test_friction_controls_sliding():
    """A cube resting on the table, pushed sideways at 0.5 m/s: without friction it slides further than at mu = 1.5."""
    torch = _torch()
    cm = compile_model("KManipSoloArmQPos")
    d = cm.desc
    n = 2
    dev = _hip(cm, n, seed=1)
    dev.set_env_params(cube_friction=torch.tensor([0.0, 1.5], dtype=torch.float64))
    dev.k_reset()
    qpos, qvel, ctrl, warm, step = dev.get_state()
    x0, y0 = 0.5 * (d.cube_spawn_lo[0] + d.cube_spawn_hi[0]), 0.5 * (d.cube_spawn_lo[1] + d.cube_spawn_hi[1])     # clear of the arm
    nl = cm.nlink
    qpos[:, nl:nl + 3] = [x0, y0, d.table_z + d.cube_half[2]]
    qpos[:, nl + 3:] = [1.0, 0.0, 0.0, 0.0]
    qvel[:, nl:] = 0.0
    qvel[:, nl] = 0.5
    warm[:] = 0.0
    dev.set_state(qpos, qvel, ctrl, warm, step)
    act = torch.zeros((n, cm.act_dim), device="cuda")
    for _ in range(5):
        dev.step_flat(act)
    q1 = dev.get_state()[0]
    slide = q1[:, nl] - x0
    assert slide[0] > 2 * slide[1] and slide[1] >= 0, slide
    dev.k_close()


def test_validation_leaves_the_handle_unchanged():
    from gym_kmanip_amd.lib import KManipError
    torch = _torch()
    cm = compile_model("KManipSoloArm")
    n = 16
    dev = _hip(cm, n, seed=2)
    dev.set_env_params(cube_mass=torch.linspace(0.03, 0.08, n, dtype=torch.float64))
    dev.k_reset()
    ref_p = {k: v.clone() for k, v in dev.get_env_params().items()}
    ref_s = dev.get_state()
    bad = [("cube_mass", 0.0), ("cube_mass", -1.0), ("cube_friction", -0.1), ("cube_frictionloss", -1e-9), ("kp_scale", 0.0),
           ("cube_mass", float("nan")), ("kp_scale", float("inf")), ("cube_friction", float("-inf"))]
    for name, v in bad:
        vals = torch.ones(n, dtype=torch.float64) * env_param_defaults(cm)[name]
        vals[n - 1] = v                                          # one bad env among good ones
        with pytest.raises(KManipError):
            dev.set_env_params(**{name: vals})
        d = cm.desc
        lo = {"cube_mass": (d.cube_mass, d.cube_mass), name: (v, 1.0)}
        with pytest.raises(KManipError):
            dev.set_env_param_ranges(**lo)
    with pytest.raises(KManipError):
        dev.set_env_param_ranges(cube_friction=(1.0, 0.5))       # lo > hi
    with pytest.raises(ValueError):
        dev.set_env_params(cube_size=1.0)
    got = dev.get_env_params()
    assert all(got[k].equal(ref_p[k]) for k in ENV_PARAMS)
    for x, y in zip(dev.get_state(), ref_s):
        assert np.array_equal(x, y)
    # still explicit mode: a reset keeps the values
    dev.k_reset()
    assert all(dev.get_env_params()[k].equal(ref_p[k]) for k in ENV_PARAMS)
    dev.k_close()


def test_gym_shell_domain_randomization():
    from gym_kmanip_amd.gym_shell import KManipEnv
    _torch()
    cm = compile_model("KManipSoloArm")
    R = _ranges(cm)
    env = KManipEnv("KManipSoloArm", num_envs=8, seed=5, domain_randomization=R)
    env.reset()
    p = env.env.get_env_params()
    for k, (lo, hi) in R.items():
        v = p[k].cpu().numpy()
        assert ((v >= lo) & (v <= hi)).all()
    assert len(np.unique(p["cube_mass"].cpu().numpy())) == 8


def _rows(h):
    return [h.obs.clone(), h.reward.clone(), h.done.clone()]


def test_spread_dispatch_with_ranges_headline_shape(monkeypatch):
    """The headline shape -- SoloArm Newton at 4096 envs -- runs SPREAD: every launch deals the envs of each 64-env block to
    waves by the flags the previous launch wrote, so an env changes wave slot and wave-mates from step to step.  In ranges mode,
    across two auto-resets (the values redrawn inside k_step), every env must compute what it computes (a) with SPREAD off
    (KMANIP_SPREAD=0: identity slots) and (b) in a small handle holding only a slice of the env ids (other launch shape, no
    SPREAD), with the actions of the counter-based action stream."""
    torch = _torch()
    cm = compile_model("KManipSoloArm")
    n, seed = 4096, 12
    R = _ranges(cm)
    lo = np.array([R[k][0] for k in ENV_PARAMS]); hi = np.array([R[k][1] for k in ENV_PARAMS])
    a = _hip(cm, n, seed=seed)
    monkeypatch.setenv("KMANIP_SPREAD", "0")
    b = _hip(cm, n, seed=seed)
    monkeypatch.delenv("KMANIP_SPREAD")
    s0, sn = 1000, 100
    c = _hip(cm, sn, seed=seed, off=s0)
    for h in (a, b, c):
        h.set_env_param_ranges(**R)
        h.k_reset()
    act_a = torch.empty((n, cm.act_dim), dtype=torch.float32, device="cuda")
    act_c = torch.empty((sn, cm.act_dim), dtype=torch.float32, device="cuda")
    for k in range(140):                              # resets at steps 64 and 128
        a.sample_action(act_a); c.sample_action(act_c)
        assert act_c.equal(act_a[s0:s0 + sn]), k
        a.step_flat(act_a); b.step_flat(act_a); c.step_flat(act_c)
        ra, rb, rc = _rows(a), _rows(b), _rows(c)
        assert all(x.equal(y) for x, y in zip(ra, rb)), k
        assert all(x[s0:s0 + sn].equal(y) for x, y in zip(ra, rc)), k
    assert (a.get_episode() == 2).all()
    sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
    for x, y, z in zip(sa, sb, sc):
        assert np.array_equal(x, y) and np.array_equal(x[s0:s0 + sn], z)
    assert np.array_equal(a.get_diag()[0], b.get_diag()[0])
    pa = _check_draw(a, seed, 0, lo, hi)
    pc = np.stack([v.cpu().numpy() for v in c.get_env_params().values()])
    assert np.array_equal(pa[:, s0:s0 + sn], pc)
    for h in (a, b, c):
        h.k_close()


def test_spread_dispatch_isolation_explicit_params():
    """Explicit heterogeneous values at the headline shape: handle B holds A's envs permuted (values, state, episode, actions);
    both run SPREAD, whose wave assignment follows each env's own contact state, so the permutation changes every wave."""
    torch = _torch()
    cm = compile_model("KManipSoloArm")
    n = 4096
    P = _spread(cm, n, 7)
    perm = np.random.default_rng(3).permutation(n)
    a, b = _hip(cm, n, seed=9), _hip(cm, n, seed=9)
    a.set_env_params(**{k: torch.from_numpy(v) for k, v in P.items()})
    b.set_env_params(**{k: torch.from_numpy(v[perm]) for k, v in P.items()})
    a.k_reset()
    b.set_state(*(x[perm] for x in a.get_state())); b.set_episode(a.get_episode()[perm])
    gen = torch.Generator(device="cuda"); gen.manual_seed(4)
    tp = torch.from_numpy(perm).cuda()
    for k in range(60):
        act = torch.rand((n, cm.act_dim), generator=gen, device="cuda") * 2 - 1
        a.step_flat(act); b.step_flat(act[tp].contiguous())
        assert b.obs.equal(a.obs[tp]) and b.reward.equal(a.reward[tp]) and b.done.equal(a.done[tp]), k
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(y, x[perm])
    assert np.array_equal(b.get_diag()[0], a.get_diag()[0][perm])
    a.k_close(); b.k_close()

