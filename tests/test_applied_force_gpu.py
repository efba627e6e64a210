"""kmanip_bind_applied_force (MuJoCo's data.qfrc_applied) on the device (run with -m gpu on an MI355X).

All states are the regime cells of tests/tools/regime_states.py (47 envs for the single arm, 72 for the two-arm models: the smallest
batches that hold every constraint regime), all three assets in the joint-delta action mode.  The reference is
tests/tools/applied_oracle.py, the physics step with a force restated in NumPy over the CPU oracle (tests/test_applied_force_cpu.py
holds it against the oracle itself).  The "test forces" are applied_oracle.draw_test_forces: default_rng(11), +-2 on every joint,
+-2 m g on the cube's force components, +-1e-3 on its torque components; they move every env's qpos by more than 1e-5 in one control
step (test_applied_force_cpu), so no parity test here passes without the feature.

The guard at the end runs without a GPU: the rows of the zero-force, parity and forces() tests launch every force object make
builds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import build_matrix as BM  # noqa: E402
import force_oracle as FO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from gym_kmanip_amd.model import ENV_PARAMS, KM_DONE_DIVERGED, with_env_params  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_V  # noqa: E402

gpu = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")
# (asset, solver, explicit per-env parameters): every row runs single steps AND one chunk (test 1); the rows without parameters and
# PARITY_PARAM_ROW also run the parity with the restatement (test 2)
STEP_ROWS = [(a, s, p) for a in ASSETS for s in SOLVERS for p in (False, True)]
PARITY_PARAM_ROW = ("solo_arm", "newton", True)
# (asset, uniform per-env parameters) of the forces() test (Newton handles only)
FORCES_ROWS = [(a, p) for a in ASSETS for p in (False, True)]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _env_params(cm, n, seed=7):
    """Explicit per-env parameters, different in every env: cube mass x 0.5 .. 2, friction 0.5 .. 1.5, friction loss 0 .. 2 x the
    model's (0 .. 0.01 where the model has none), kp scale 0.8 .. 1.3."""
    rng = np.random.default_rng(seed)
    d = cm.desc
    fl = d.cube_frictionloss if d.cube_frictionloss > 0 else 0.005
    return dict(cube_mass=d.cube_mass * rng.uniform(0.5, 2.0, n), cube_friction=rng.uniform(0.5, 1.5, n),
                cube_frictionloss=fl * rng.uniform(0.0, 2.0, n), kp_scale=rng.uniform(0.8, 1.3, n))


def _device(cm, qpos, qvel, ctrl, warm, params=None):
    torch = _torch()
    from gym_kmanip_amd import env_hip
    n = len(qpos)
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=0)
    dev.k_reset()
    if params is not None:
        dev.set_env_params(**{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    dev.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, step=np.zeros(n, dtype=np.int32))
    return dev


def _bind(dev, tau):
    t = dev.new_applied_force()
    t.copy_(_torch().from_numpy(np.ascontiguousarray(tau)))
    return t


def _snapshot(dev):
    qpos, qvel, ctrl, warm, step = dev.get_state()
    return dict(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, step=step, episode=dev.get_episode(), obs=dev.obs.cpu().numpy(),
                reward=dev.reward.cpu().numpy(), done=dev.done.cpu().numpy(), mask=dev.get_diag()[0])


def _same_bits(a, b):
    """Per-env equality of two arrays' BYTES (a -0.0 is not a +0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    n = len(a)
    return (a.view(np.uint8).reshape(n, -1) == b.view(np.uint8).reshape(n, -1)).all(axis=1)


def _assert_same(x, y, what, labels=None, skip=()):
    for key in x:
        eq = _same_bits(x[key], y[key])
        for e in skip:
            eq[e] = True
        assert eq.all(), (what, key, [(labels[e] if labels else None, int(e)) for e in np.where(~eq)[0]])


def _actions(cm, n, seed=3):
    return np.random.default_rng(seed).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)


def _cells(asset, solver):
    from oracle.oracle import Oracle
    cm = R.model(asset, solver)
    qpos, qvel, ctrl, labels = R.cells(asset)
    warm = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
    return cm, qpos, qvel, ctrl, warm, labels


# ------------------------------------------------------------------------------------------------------ 1. zero force changes nothing
@gpu
@pytest.mark.parametrize("asset,solver,par", STEP_ROWS)
def test_a_buffer_of_zeros_changes_no_bit(asset, solver, par):
    """A bound buffer of zeros against no buffer: state, warm start, counters, obs, reward, done and contact mask bit for bit over
    three control steps of small random actions, as single steps and as one chunk of three; unbinding returns to the default
    kernels; a reset with a NON-zero buffer bound equals the reset without one (state and warm start)."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset, solver)
    n = len(labels)
    params = _env_params(cm, n) if par else None
    acts = _actions(cm, n)
    a, b = _device(cm, qpos, qvel, ctrl, warm, params), _device(cm, qpos, qvel, ctrl, warm, params)
    zeros = b.new_applied_force()
    assert b.applied_force is zeros and a.applied_force is None and not zeros.any()
    for k in range(3):
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        _assert_same(_snapshot(a), _snapshot(b), ("step", k), labels)
    after3 = _snapshot(a)
    assert not zeros.any()                                   # the library never writes the buffer
    b.bind_applied_force(None)
    assert b.applied_force is None
    act = torch.from_numpy(acts[0]).cuda()
    a.step_flat(act); b.step_flat(act)
    _assert_same(_snapshot(a), _snapshot(b), "unbound", labels)
    # a reset ignores the buffer
    tau = AO.draw_test_forces(cm, n)
    t = _bind(b, tau)
    a.k_reset(); b.k_reset()
    _assert_same(_snapshot(a), _snapshot(b), "reset", labels)
    assert np.array_equal(t.cpu().numpy(), tau)
    a.k_close(); b.k_close()
    # one chunk of three
    c = _device(cm, qpos, qvel, ctrl, warm, params)
    c.new_applied_force()
    obs, rew, done = c.step_chunk(torch.from_numpy(acts).cuda())
    _assert_same(after3, _snapshot(c), "chunk", labels)
    c.k_close()


# ------------------------------------------------------------------------------------------------------ 2. parity with the restatement
def _parity(cm, run, g, labels, tag):
    """One control step of the device (snapshot g) against a control_step result of the restatement and its twin."""
    ref, twin = run["ref"], run["twin"]
    n = len(labels)
    assert not (g["done"] & KM_DONE_DIVERGED).any()
    for key in ("ctrl", "done", "step"):
        eq = _same_bits(g[key], ref[key].astype(g[key].dtype))
        assert eq.all(), (tag, key, [(labels[e], int(e)) for e in np.where(~eq)[0]])
    eq = g["mask"] == ref["mask"]
    assert eq.all(), (tag, "mask", [(labels[e], int(e), hex(int(g["mask"][e])), hex(int(ref["mask"][e]))) for e in np.where(~eq)[0]])
    cell_of = np.array(labels)
    worst = {}
    for key, bar in (("qpos", TOL_Q), ("qvel", TOL_V)):
        d = np.abs(g[key] - ref[key]).max(axis=1)
        s = np.abs(twin[key] - ref[key]).max(axis=1)
        worst[key] = (float(d.max()), float(s.max()))
        for c in dict.fromkeys(labels):
            assert 10.0 * s[cell_of == c].max() <= bar, ("the reference's own spread in this cell is no longer far below the bar", c, key)
    print("\n%s: worst |device - restatement| (restatement's own spread): %s" % (
        tag, "  ".join("%s %.1e (%.1e)" % (k, v[0], v[1]) for k, v in worst.items())))
    for key, bar in (("qpos", TOL_Q), ("qvel", TOL_V)):
        d = np.abs(g[key] - ref[key]).max(axis=1)
        assert (d < bar).all(), (tag, key, [(labels[e], int(e), float(d[e])) for e in np.where(~(d < bar))[0]])


@gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_parity_with_the_restatement_under_the_test_forces(asset, solver):
    """One control step, zero action, the test forces: ctrl, done byte and step counter bit for bit, the contact mask equal, qpos
    and qvel within TOL_Q / TOL_V, and ten times the restatement's own spread below the bars in every cell."""
    torch = _torch()
    run = AO.cell_runs(asset, solver)
    cm, labels = run["cm"], run["labels"]
    dev = _device(cm, run["qpos"], run["qvel"], run["ctrl"], run["warm"])
    _bind(dev, run["tau"])
    dev.step_flat(torch.zeros((len(labels), cm.act_dim), dtype=torch.float32, device="cuda"))
    g = _snapshot(dev)
    dev.k_close()
    _parity(cm, run, g, labels, "%s %s" % (asset, solver))


@gpu
def test_parity_with_explicit_per_env_parameters():
    """The same parity on PARITY_PARAM_ROW with different physics parameters in every env: the reference's model of env e is
    model.with_env_params(cm, **values of e)."""
    torch = _torch()
    from oracle.oracle import Oracle
    asset, solver, _ = PARITY_PARAM_ROW
    cm = R.model(asset, solver)
    qpos, qvel, ctrl, labels = R.cells(asset)
    n = len(labels)
    params = _env_params(cm, n)
    models = [with_env_params(cm, **{k: float(params[k][e]) for k in ENV_PARAMS}) for e in range(n)]
    warm = np.stack([Oracle(models[e], 1).after_reset(qpos[e], qvel[e], ctrl[e]) for e in range(n)])
    tau = AO.draw_test_forces(cm, n)
    run = dict(ref=AO.control_step(cm, qpos, qvel, ctrl, warm, tau, models=models),
               twin=AO.control_step(cm, qpos, qvel * (1.0 + 1e-15), ctrl, warm, tau, models=models))
    dev = _device(cm, qpos, qvel, ctrl, warm, params)
    _bind(dev, tau)
    dev.step_flat(torch.zeros((n, cm.act_dim), dtype=torch.float32, device="cuda"))
    g = _snapshot(dev)
    dev.k_close()
    _parity(cm, run, g, labels, "%s %s with per-env parameters" % (asset, solver))


# ------------------------------------------------------------------------------------------------------ 4. isolation
def _orders(coupled):
    n = len(coupled)
    c = [e for e in range(n) if coupled[e]]
    u = [e for e in range(n) if not coupled[e]]
    inter = []
    for i in range(max(len(c), len(u))):
        inter += c[i:i + 1] + u[i:i + 1]
    return {"cell-major": np.arange(n), "interleaved": np.array(inter), "reversed": np.arange(n)[::-1].copy()}


@gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_forced_envs_in_any_order_wave_shape_and_chunk_keep_their_bits(asset, solver, monkeypatch):
    """A different force in every env (the test forces; the row travels with its env): the envs in three orders at KMANIP_EPB = 2
    (and 4 on the 10-link model) against KMANIP_EPB = 1 in cell-major order, three steps of small random actions, and one chunk of
    three in two orders: every env's qpos, qvel, ctrl, warm start, obs, reward, done and contact mask bit for bit the same."""
    torch = _torch()
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset, solver)
    n = len(labels)
    tau = AO.draw_test_forces(cm, n)
    acts = _actions(cm, n, seed=4)
    one = Oracle(cm, 1)
    coupled = [R.regime(cm, one, qpos[e], qvel[e], ctrl[e])["coupled"] for e in range(n)]
    orders = _orders(coupled)
    epbs = (2, 4) if cm.nlink == 10 else (2,)

    def run(perm, epb, chunk=False):
        monkeypatch.setenv("KMANIP_EPB", str(epb)) if epb else monkeypatch.delenv("KMANIP_EPB", raising=False)
        assert sorted(perm) == list(range(n))
        inv = np.argsort(perm)
        dev = _device(cm, qpos[perm], qvel[perm], ctrl[perm], warm[perm])
        _bind(dev, tau[perm])
        runs = []
        if chunk:
            obs_c, rew_c, done_c = dev.step_chunk(torch.from_numpy(np.ascontiguousarray(acts[:, perm])).cuda())
            runs = [dict(obs=obs_c[k].cpu().numpy()[inv], reward=rew_c[k].cpu().numpy()[inv], done=done_c[k].cpu().numpy()[inv]) for k in range(3)]
            runs[2].update({key: v[inv] for key, v in _snapshot(dev).items() if key in ("qpos", "qvel", "ctrl", "warm", "step", "mask")})
        else:
            for k in range(3):
                dev.step_flat(torch.from_numpy(np.ascontiguousarray(acts[k][perm])).cuda())
                runs.append({key: v[inv] for key, v in _snapshot(dev).items()})
        dev.k_close()
        return runs

    def same(runs, what):
        for k in range(3):
            _assert_same(runs[k], {key: ref[k][key] for key in runs[k]}, (what, k), labels)

    ref = run(orders["cell-major"], 1)
    for epb in epbs:
        for name, perm in orders.items():
            same(run(perm, epb), (name, epb))
    for name in ("cell-major", "interleaved"):
        same(run(orders[name], None, chunk=True), (name, "chunk"))
    monkeypatch.delenv("KMANIP_EPB", raising=False)


# ------------------------------------------------------------------------------------------------------ 5. forces() under a bound force
@gpu
@pytest.mark.parametrize("asset,par", FORCES_ROWS)
def test_forces_report_the_forced_state(asset, par):
    """forces() with the test forces bound against the restatement's first sub-step (force_oracle.decode with a_s shifted), under the
    bars and normalisers of tests/test_forces_cpu.py; and the balance M qacc + qfrc_bias = qfrc_actuator (padded) + qfrc_applied +
    qfrc_constraint with kinematics()' qM and qfrc_bias, its residual (relative to the largest term, at least 1) at most ten times
    the same residual of the restatement itself."""
    torch = _torch()
    from oracle.oracle import Oracle
    from test_forces_gpu import _compare, _host, _report
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset, "newton")
    n, nl = len(labels), cm.nlink
    p = dict(cube_mass=2.0 * cm.desc.cube_mass, cube_friction=0.5, cube_frictionloss=0.0, kp_scale=1.3) if par else None
    cmr = with_env_params(cm, **p) if par else cm
    one = Oracle(cmr, 1)
    if par:
        warm = R.warm_start(cmr, one, qpos, qvel, ctrl)
    tau = AO.draw_test_forces(cm, n)
    dev = _device(cm, qpos, qvel, ctrl, warm, None if p is None else {k: np.full(n, v) for k, v in p.items()})
    unforced = _host(dev.forces(fields=("qacc",)))
    _bind(dev, tau)
    f = _host(dev.forces())
    kin = {k: v.cpu().numpy() for k, v in dev.kinematics(fields=("qM", "qfrc_bias")).items()}
    dev.k_close()
    assert (np.abs(f["qacc"] - unforced["qacc"]).max(axis=1) > 1e-6).all()          # the force reaches every env's qacc

    def balance(M, a, bias, fa, fc, t):
        terms = [M @ a, bias, np.concatenate([fa, np.zeros(6)]), t, fc]
        return float(np.abs(terms[0] + terms[1] - terms[2] - terms[3] - terms[4]).max()) / max(1.0, max(float(np.abs(x).max()) for x in terms))
    figures, bad, res_dev, res_ref = [], [], 0.0, 0.0
    for e in range(n):
        o = AO.forces_decode(cmr, one, qpos[e], qvel[e], ctrl[e], warm[e], tau[e])
        bad += _compare(cmr, f, e, o, (labels[e], e), figures)
        res_ref = max(res_ref, balance(o["M"], o["qacc"], o["bias"], o["qfrc_actuator"], o["qfrc_constraint"], tau[e]))
        res_dev = max(res_dev, balance(kin["qM"][e], f["qacc"][e], kin["qfrc_bias"][e], f["qfrc_actuator"][e], f["qfrc_constraint"][e], tau[e]))
    _report("%s%s under the test forces" % (asset, " with parameters" if par else ""), figures)
    print("balance residual: device %.1e, restatement %.1e" % (res_dev, res_ref))
    assert not bad, bad
    assert res_dev <= 10.0 * res_ref, (res_dev, res_ref)


# ------------------------------------------------------------------------------------------------------ 6. physics anyone can read
@gpu
def test_the_cube_hovers_on_its_own_weight():
    """Home pose, cube 0.3 m over the table.  Envs 0-2 of the model's mass with 0, m g and 2 m g on the cube's z dof: m g leaves z
    and vz unchanged to the bit, 2 m g mirrors free fall, and all three follow the restatement.  Then two envs of half and three
    times the mass (KM_EP_CUBE_MASS), each hovering on its own m g.  The mirror's bar: the two runs apply opposite accelerations,
    so they differ only by the rounding of z + dt vz at z = 1.1 m: ten sub-steps of at most half an ulp (1.1e-16) in each run, 2.2e-15
    in all, held to 1e-14; vz (0.19 m/s: ulp 2.8e-17) to 1e-13."""
    torch = _torch()
    from oracle.oracle import Oracle
    cm = R.model("solo_arm")
    nl = cm.nlink
    one = Oracle(cm, 1)
    qpos, qvel, ctrl = AO.hover_state(cm)
    warm = one.after_reset(qpos, qvel, ctrl)
    g = abs(cm.desc.gravity[2])
    rep = lambda x, n: np.repeat(np.asarray(x)[None], n, axis=0)
    tau = np.zeros((3, cm.nv))
    tau[:, nl + 2] = np.array([0.0, 1.0, 2.0]) * (cm.desc.cube_mass * g)
    dev = _device(cm, rep(qpos, 3), rep(qvel, 3), rep(ctrl, 3), rep(warm, 3))
    _bind(dev, tau)
    dev.step_flat(torch.zeros((3, cm.act_dim), dtype=torch.float32, device="cuda"))
    q, v = dev.get_state()[:2]
    dev.k_close()
    dz, dvz = q[:, nl + 2] - qpos[nl + 2], v[:, nl + 2]
    print("\nhover: dz %r vz %r" % (dz.tolist(), dvz.tolist()))
    assert dz[1] == 0.0 and dvz[1] == 0.0
    assert dz[0] < -1.9e-3 and abs(dz[2] + dz[0]) <= 1e-14 and abs(dvz[2] + dvz[0]) <= 1e-13
    for e in range(3):
        qr, vr, _ = AO.physics_step(cm, one, qpos, qvel, ctrl, warm, tau[e])
        assert np.abs(q[e] - qr).max() < TOL_Q and np.abs(v[e] - vr).max() < TOL_V, e
    mass = cm.desc.cube_mass * np.array([0.5, 3.0])
    tau = np.zeros((2, cm.nv))
    tau[:, nl + 2] = mass * g
    dev = _device(cm, rep(qpos, 2), rep(qvel, 2), rep(ctrl, 2), rep(warm, 2), dict(cube_mass=mass))
    _bind(dev, tau)
    dev.step_flat(torch.zeros((2, cm.act_dim), dtype=torch.float32, device="cuda"))
    q, v = dev.get_state()[:2]
    dev.k_close()
    assert (q[:, nl + 2] == qpos[nl + 2]).all() and (v[:, nl + 2] == 0.0).all(), (q[:, nl + 2] - qpos[nl + 2], v[:, nl + 2])


@gpu
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_gravity_compensation_holds_the_arm(asset):
    """Eight zero-action steps from home with kinematics()' qfrc_bias[:, :nlink] bound anew before each: the arm's drift is at most
    a hundredth of the drift without the binding (the restatement: 8.0e-2 rad without, below 2e-16 rad with).  The Torso is left
    out: its home pose drifts 0.33 rad either way (three joints start beyond their ranges), so the ratio says nothing there."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    cm = R.model(asset)
    nl, n = cm.nlink, 4
    drift = {}
    for comp in (False, True):
        dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=0)
        dev.k_reset()
        home = dev.state_tensors()["qpos"][:, :nl].clone()
        act = torch.zeros((n, cm.act_dim), dtype=torch.float32, device="cuda")
        for _ in range(8):
            if comp:
                t = torch.zeros((n, cm.nv), dtype=torch.float64, device="cuda")
                t[:, :nl] = dev.kinematics(fields=("qfrc_bias",))["qfrc_bias"][:, :nl]
                dev.bind_applied_force(t)
            dev.step_flat(act)
        assert not dev.done.cpu().numpy().any()
        drift[comp] = float((dev.state_tensors()["qpos"][:, :nl] - home).abs().max())
        dev.k_close()
    print("\n%s: arm drift without %.3e rad, with %.3e rad" % (asset, drift[False], drift[True]))
    assert drift[False] > 1e-2 and drift[True] <= drift[False] / 100.0, drift


# ------------------------------------------------------------------------------------------------------ 7. non-finite force
@gpu
def test_a_non_finite_force_diverges_its_env_alone(monkeypatch):
    """One env with a NaN component and one with an inf component among finite ones, four envs per wave: those two report
    KM_DONE_DIVERGED with zero observation-before-reset semantics (zero reward, empty mask) and are reset; every other env equals
    the run in which those two had finite forces, bit for bit; forces() gives the two status 1 and zero outputs."""
    torch = _torch()
    from test_forces_gpu import FLOAT_FIELDS
    monkeypatch.setenv("KMANIP_EPB", "4")
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm", "newton")
    n, nl = len(labels), cm.nlink
    tau = AO.draw_test_forces(cm, n)
    i, j = 5, 18
    bad_tau = tau.copy()
    bad_tau[i, 3] = np.nan
    bad_tau[j, nl + 1] = -np.inf
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    _bind(a, tau)
    _bind(b, bad_tau)
    fa, fb = a.forces(), b.forces()
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[[i, j]] = False
    assert fb["status"][i] == 1 and fb["status"][j] == 1 and fb["status"].sum() == 2 and not fa["status"].any()
    for e in (i, j):
        assert (fb["contact_bit"][e] == -1).all() and fb["contact_mask"][e] == 0
        for key in FLOAT_FIELDS:
            assert not fb[key][e].any(), key
    for key in fa:
        assert torch.equal(fa[key][keep], fb[key][keep]), key
    act = torch.from_numpy(_actions(cm, n)[0]).cuda()
    a.step_flat(act); b.step_flat(act)
    sa, sb = _snapshot(a), _snapshot(b)
    _assert_same(sa, sb, "finite envs", labels, skip=(i, j))
    home = np.array(cm.desc.q_home[:nl])
    for e in (i, j):
        assert sb["done"][e] & KM_DONE_DIVERGED and not sa["done"][e]
        assert sb["reward"][e] == 0.0 and sb["mask"][e] == 0 and sb["step"][e] == 0 and sb["episode"][e] == sa["episode"][e] + 1
        assert (sb["qpos"][e, :nl] == home).all() and not sb["qvel"][e].any() and np.isfinite(sb["qpos"][e]).all()
        assert np.isfinite(sb["obs"][e]).all() and np.isfinite(sb["warm"][e]).all()
    monkeypatch.delenv("KMANIP_EPB", raising=False)
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------------ 8. shell and wrapper
@gpu
def test_shell_exposes_the_bound_tensor():
    torch = _torch()
    from gym_kmanip_amd.gym_shell import KManipEnv
    env = KManipEnv("KManipSoloArm", num_envs=8, applied_force=True, device_outputs=True)
    plain = KManipEnv("KManipSoloArm", num_envs=8, device_outputs=True)
    _, info = env.reset()
    _, info0 = plain.reset()
    t = env.applied_force
    assert "applied_force" not in info0 and plain.applied_force is None and info["applied_force"] is t is env.env.applied_force
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (8, env.env.cm.nv) and not t.any()
    zero = {key: np.zeros((8,) + tuple(sp.shape), np.float32) for key, sp in env.action_space.spaces.items()}
    o1, *_ = env.step(zero)
    o0, *_ = plain.step(zero)
    assert all(torch.equal(o1[k], o0[k]) for k in o0)
    t[:, 0] = 5.0                                            # a torque on the first joint
    o1, *_ = env.step(zero)
    o0, *_ = plain.step(zero)
    assert not torch.equal(o1["q_pos"], o0["q_pos"])
    assert (t[:, 0] == 5.0).all() and not t[:, 1:].any()    # the shell never changes its contents
    env.reset()
    assert (t[:, 0] == 5.0).all()
    env.close(); plain.close()


@gpu
def test_refusals_and_state_calls_leave_the_binding_alone():
    """bind_applied_force refuses a wrong dtype, shape, layout or device before the C call and leaves handle and binding usable;
    copy_envs_from and set_state_tensors carry neither the binding nor the buffer; a NULL handle is an error."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.lib import KManipError
    cm = R.model("solo_arm")
    n, nv = 8, cm.nv
    dev, twin, src = (env_hip.KManipEnvHip(cm, num_envs=n, seed=0) for _ in range(3))
    for d in (dev, twin, src):
        d.k_reset()
    t = dev.new_applied_force()
    t[:, 0] = 3.0
    for bad in (torch.zeros((n, nv), dtype=torch.float32, device="cuda"), torch.zeros((n, nv + 1), dtype=torch.float64, device="cuda"),
                torch.zeros((n - 1, nv), dtype=torch.float64, device="cuda"), torch.zeros((nv, n), dtype=torch.float64, device="cuda").t(),
                torch.zeros((n, nv), dtype=torch.float64), np.zeros((n, nv))):
        with pytest.raises(KManipError):
            dev.bind_applied_force(bad)
        assert dev.applied_force is t
    assert dev.L.kmanip_bind_applied_force(None, None) != 0
    # state calls: the destination keeps its binding and buffer; the source's (none) does not travel
    dev.copy_envs_from(src)
    st = src.state_tensors()
    dev.set_state_tensors(qpos=st["qpos"], qvel=st["qvel"])
    twin.copy_envs_from(src)
    assert dev.applied_force is t and (t[:, 0] == 3.0).all() and not t[:, 1:].any() and src.applied_force is None
    act = torch.zeros((n, cm.act_dim), dtype=torch.float32, device="cuda")
    dev.step_flat(act); twin.step_flat(act); src.step_flat(act)
    assert torch.equal(twin.state_tensors()["qpos"], src.state_tensors()["qpos"])
    assert not torch.equal(dev.state_tensors()["qpos"][:, 0], twin.state_tensors()["qpos"][:, 0])      # the force still acts
    assert not dev.done.cpu().numpy().any()
    for d in (dev, twin, src):
        d.k_close()


# ------------------------------------------------------------------------------------------------------ 3. a row for every object
SOLVER_OF = {"pgs": 0, "newton": 1}


def force_objects(makefile_path):
    """Every force object of kmanip_dyn and kmanip_forces that make builds and every launch shape of it: ("dyn", NL, G, SOLVER, per-env
    parameters, chunk) for the kmanip_dyn_frc_* / kmanip_dyn_ep_frc_* objects, ("forces", NL, G, per-env parameters) for the
    kmanip_forces_frc_* / kmanip_forces_ep_frc_* objects."""
    objs = [o for o in BM.objects(makefile_path) if o.frc]
    return ([("dyn", o.NL, o.G, o.solver, o.ep, chunk) for o in objs if o.unit == "dyn" for chunk in (False, True)]
            + [("forces", o.NL, o.G, o.ep) for o in objs if o.unit == "forces"])


def covered(step_rows, parity_rows, forces_rows):
    """What the rows launch: kmanip_dispatch.hip picks the 10-link class for nlink <= 10, the 20-link class otherwise, the
    KM_VAR_PAR build while the handle has per-env parameters.  A step row runs single steps and one chunk with a zero buffer
    (test 1); it counts only if the same object also runs a parity row against the restatement (test 2)."""
    cls = lambda asset: (10, 16) if R.model(asset).nlink <= 10 else (20, 32)
    parity = {cls(a) + (SOLVER_OF[s], p) for a, s, p in parity_rows}
    out = set()
    for a, s, p in step_rows:
        if cls(a) + (SOLVER_OF[s], False) in parity:         # (the parameter builds share every line of the force path with these)
            out |= {("dyn",) + cls(a) + (SOLVER_OF[s], p, chunk) for chunk in (False, True)}
    out |= {("forces",) + cls(a) + (p,) for a, p in forces_rows}
    return out


def _parity_rows():
    return [(a, s, False) for a in ASSETS for s in SOLVERS] + [PARITY_PARAM_ROW]


def test_every_compiled_force_object_has_a_row():
    objs = force_objects(BM.MAKEFILE)
    assert len(objs) >= 2 * 2 * 4 + 2 * 2
    have = covered(STEP_ROWS, _parity_rows(), FORCES_ROWS)
    assert [o for o in objs if o not in have] == []


def test_the_guard_fails_for_an_object_without_a_row(tmp_path):
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    have = covered(STEP_ROWS, _parity_rows(), FORCES_ROWS)
    miss = [o for o in force_objects(more) if o not in have]
    assert sorted(o for o in miss if o[0] == "dyn") == [("dyn", 30, 64, s, p, c) for s in (0, 1) for p in (False, True) for c in (False, True)]
    assert [o for o in miss if o[0] == "forces"] == [("forces", 30, 64, False), ("forces", 30, 64, True)]
    rows = [r for r in STEP_ROWS if not (r[1] == "pgs" and r[2])]
    miss = [o for o in force_objects(BM.MAKEFILE) if o not in covered(rows, _parity_rows(), FORCES_ROWS)]
    assert ("dyn", 10, 16, 0, True, True) in miss and ("dyn", 20, 32, 0, True, False) in miss
    miss = [o for o in force_objects(BM.MAKEFILE) if o not in covered(STEP_ROWS, _parity_rows(), [r for r in FORCES_ROWS if not r[1]])]
    assert miss == [("forces", 10, 16, True), ("forces", 20, 32, True)]
