"""kmanip_kinematics against the kinematics oracle (run with -m gpu on an MI355X).

One handle per asset holds every regime cell's copies (tests/tools/regime_states.py: 47 envs for the single arm, 72 for the two-arm
models -- not a multiple of the 4 / 2 envs a wave holds; qvel up to 28 rad/s).  Every field kmanip_kinematics writes is compared
with tests/tools/kin_oracle.py under the bars of tests/test_kinematics_cpu.py: geometry 1e-12 absolute (site_vel divided by
max(1, max|qvel|)), qM and qfrc_bias 1000 x the oracle's own spread.  Then: the two-row path without the block split, per-env
parameters, a PGS handle, the call after a step, the equation of motion with kmanip_forces' numbers, the handle left untouched,
the launch shapes, the refusals, the Gymnasium shell's info keys and the resolved-rate example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import kin_oracle as KO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_forces_cpu import BAR_GEOMETRY, BAR_QFRC_CONSTRAINT  # noqa: E402
from test_kinematics_cpu import BAR_QFRC_BIAS, BAR_QM  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
BARS = dict({k: BAR_GEOMETRY for k in KO.GEOMETRY}, qM=BAR_QM, qfrc_bias=BAR_QFRC_BIAS)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_WARM = {}


def _cells(asset):
    """(cm, qpos, qvel, ctrl, warm, labels) of the asset's cells; the warm start computed once."""
    from oracle.oracle import Oracle
    cm = R.model(asset)
    qpos, qvel, ctrl, labels = R.cells(asset)
    if asset not in _WARM:
        _WARM[asset] = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
    return cm, qpos, qvel, ctrl, _WARM[asset], labels


def _device(cm, qpos, qvel, ctrl, warm):
    from gym_kmanip_amd import env_hip
    n = len(qpos)
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=0)
    dev.k_reset()
    dev.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, step=np.zeros(n, dtype=np.int32))
    return dev


def _host(k):
    return {name: v.cpu().numpy() for name, v in k.items()}


def _compare(k, e, o, qvel, what, figures, fields=KO.FIELDS):
    """Env e of a kinematics() result (host arrays) against the decode o: appends the normalised differences to `figures` and
    returns the violations."""
    if "status" in k and k["status"][e] != 0:
        return [(what, "status", int(k["status"][e]))]
    d = KO.differences({name: k[name][e] for name in fields if name in k}, o, qvel)
    figures.append((what, d))
    return [(what, name, v, BARS[name]) for name, v in d.items() if not v <= BARS[name]]


def _report(tag, figures):
    worst = {}
    for what, d in figures:
        for name, v in d.items():
            if v >= worst.get(name, (-1.0, None))[0]:
                worst[name] = (v, what)
    print("\n%s: worst normalised |device - oracle|: %s" % (tag, "  ".join("%s %.1e %s" % (name, v, w) for name, (v, w) in worst.items())))


def _structure(cm, k):
    """What holds exactly: symmetry and zero pattern of qM, zero columns of the Jacobians, zeros of an absent arm."""
    d = cm.desc
    nl = cm.nlink
    M = k["qM"]
    assert np.array_equal(M, M.transpose(0, 2, 1))
    assert not M[:, :nl, nl:].any()
    blocks = R.blocks(cm)
    if len(blocks) == 2:
        s = blocks[1][0]
        assert not M[:, :s, s:nl].any()
    for a in range(2):
        if not d.arm_present[a]:
            assert not any(k[name][:, a].any() for name in ("site_xpos", "site_xmat", "site_jacp", "site_jacr", "site_vel"))
            continue
        off = [j for j in range(cm.nv) if j not in KO.site_chain(cm, a)]
        assert (k["site_jacp"][:, a][:, :, off] == 0).all() and (k["site_jacr"][:, a][:, :, off] == 0).all()


@pytest.mark.parametrize("asset", ASSETS)
def test_parity_with_the_kinematics_oracle_on_every_cell(asset):
    """Worst normalised differences measured on an MI355X: DESIGN.md section 20."""
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    _, dec, _ = KO.cell_decodes(asset)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    full = dev.kinematics()
    J = dev.site_jacobian(full, 0).cpu().numpy()
    k = _host(full)
    dev.k_close()
    figures, bad = [], []
    for e, o in enumerate(dec):
        bad += _compare(k, e, o, qvel[e], (labels[e], e), figures)
    _report(asset, figures)
    assert not bad, bad
    assert not k["status"].any()
    _structure(cm, k)
    d = cm.desc
    cube = np.diag([d.cube_mass] * 3 + list(d.cube_inertia))
    assert all(np.array_equal(M[cm.nlink:, cm.nlink:], cube) for M in k["qM"])
    assert J.shape == (len(labels), 6, cm.nv) and np.array_equal(J[:, :3], k["site_jacp"][:, 0]) and np.array_equal(J[:, 3:], k["site_jacr"][:, 0])
    assert np.abs(qvel).max() > 20.0


def test_two_row_path_without_the_block_split(monkeypatch):
    cm, qpos, qvel, ctrl, warm, labels = _cells("dual_arm")
    _, dec, _ = KO.cell_decodes("dual_arm")
    a = _device(cm, qpos, qvel, ctrl, warm)
    monkeypatch.setenv("KMANIP_NO_BLOCK_SPLIT", "1")
    b = _device(cm, qpos, qvel, ctrl, warm)
    monkeypatch.delenv("KMANIP_NO_BLOCK_SPLIT")
    ka, kb = _host(a.kinematics()), _host(b.kinematics())
    a.k_close(); b.k_close()
    figures, bad, between = [], [], {}
    for e, o in enumerate(dec):
        bad += _compare(kb, e, o, qvel[e], (labels[e], e), figures)
        d = KO.differences({name: kb[name][e] for name in KO.FIELDS}, {name: ka[name][e] for name in KO.FIELDS}, qvel[e])
        bad += [((labels[e], e), "against the default handle", name, v) for name, v in d.items() if not v <= 1e-12]
        between = {name: max(v, between.get(name, 0.0)) for name, v in d.items()}
    _report("dual_arm without the block split", figures)
    print("against the default handle: %s" % "  ".join("%s %.1e" % kv for kv in between.items()))
    assert not bad, bad
    _structure(cm, kb)


@pytest.mark.parametrize("asset", ASSETS)
def test_per_env_parameters_on_the_device(asset):
    """set_env_params (cube mass x 2, friction 0.5, kp scale 1.3) against the with_env_params oracle on all cells; then a handle in
    ranges mode after a reset against the values get_env_params returns."""
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.model import with_env_params
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    nl = cm.nlink
    p = dict(cube_mass=2.0 * cm.desc.cube_mass, cube_friction=0.5, cube_frictionloss=0.0, kp_scale=1.3)
    cmp_ = with_env_params(cm, **p)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    dev.set_env_params(**p)
    k = _host(dev.kinematics())
    dev.k_close()
    orc = Oracle(cmp_, 1)
    figures, bad = [], []
    for e in range(len(labels)):
        bad += _compare(k, e, KO.decode(cmp_, orc, qpos[e], qvel[e]), qvel[e], (labels[e], e), figures)
    _report(asset + " with parameters", figures)
    assert not bad, bad
    cube = np.diag([cmp_.desc.cube_mass] * 3 + list(cmp_.desc.cube_inertia))
    assert all(np.array_equal(M[nl:, nl:], cube) for M in k["qM"]) and cube[0, 0] == 2.0 * cm.desc.cube_mass
    # ranges mode: the values drawn at the reset
    n = 6
    rng_dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=2)
    rng_dev.set_env_param_ranges(cube_mass=(0.5 * cm.desc.cube_mass, 3.0 * cm.desc.cube_mass))
    rng_dev.k_reset()
    vals = {name: v.cpu().numpy() for name, v in rng_dev.get_env_params().items()}
    k = _host(rng_dev.kinematics())
    q, v = rng_dev.get_state()[:2]
    rng_dev.k_close()
    assert len(set(vals["cube_mass"])) == n
    figures, bad = [], []
    for e in range(n):
        cme = with_env_params(cm, cube_mass=float(vals["cube_mass"][e]))
        bad += _compare(k, e, KO.decode(cme, Oracle(cme, 1), q[e], v[e]), v[e], ("ranges", e), figures)
        assert np.array_equal(np.diag(k["qM"][e])[nl:], [cme.desc.cube_mass] * 3 + list(cme.desc.cube_inertia))
    _report(asset + " in ranges mode", figures)
    assert not bad, bad


def test_a_pgs_handle_returns_the_newton_handles_bits():
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm")
    newton = _device(cm, qpos, qvel, ctrl, warm)
    pgs = _device(R.model("solo_arm", "pgs"), qpos, qvel, ctrl, warm)
    a, b = newton.kinematics(), pgs.kinematics()
    newton.k_close(); pgs.k_close()
    assert set(a) == set(b) and all(torch.equal(a[name], b[name]) for name in a)
    assert not a["status"].any() and a["qM"].abs().max() > 0


@pytest.mark.parametrize("asset", ASSETS)
def test_kinematics_after_a_step_use_the_state_the_step_left(asset):
    """One step_flat with small actions, then kinematics on the same stream: compared with the oracle at the device's own
    read-back state."""
    torch = _torch()
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    act = np.random.default_rng(5).uniform(-0.2, 0.2, (len(labels), cm.act_dim)).astype(np.float32)
    dev.step_flat(torch.from_numpy(act).cuda())
    k = _host(dev.kinematics())
    q1, v1 = dev.get_state()[:2]
    assert not dev.done.cpu().numpy().any() and np.abs(q1 - qpos).max() > 0
    dev.k_close()
    orc = Oracle(cm, 1)
    figures, bad = [], []
    for e in range(len(labels)):
        bad += _compare(k, e, KO.decode(cm, orc, q1[e], v1[e]), v1[e], (labels[e], e), figures)
    _report(asset + " after a step", figures)
    assert not bad, bad


@pytest.mark.parametrize("asset", ASSETS)
def test_equation_of_motion_on_the_devices_own_numbers(asset):
    """M qacc + qfrc_bias = pad(qfrc_actuator) + qfrc_constraint with kinematics() and forces() of one Newton handle, all cells;
    normalised by max(1, max|qfrc_constraint|, max|M qacc|).  Worst figures measured on an MI355X: DESIGN.md section 20."""
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    nl = cm.nlink
    dev = _device(cm, qpos, qvel, ctrl, warm)
    k = _host(dev.kinematics(fields=("qM", "qfrc_bias", "status")))
    f = _host(dev.forces(fields=("qacc", "qfrc_constraint", "qfrc_actuator", "status")))
    dev.k_close()
    assert not k["status"].any() and not f["status"].any()
    mq = np.einsum("eij,ej->ei", k["qM"], f["qacc"])
    rhs = f["qfrc_constraint"].copy()
    rhs[:, :nl] += f["qfrc_actuator"]
    scale = np.maximum(1.0, np.maximum(np.abs(f["qfrc_constraint"]).max(axis=1), np.abs(mq).max(axis=1)))
    r = np.abs(mq + k["qfrc_bias"] - rhs).max(axis=1) / scale
    e = int(np.argmax(r))
    print("\n%s: M qacc + bias - (qfrc_actuator + qfrc_constraint) on the device, worst %.1e (%s, env %d)" % (asset, r[e], labels[e], e))
    assert (r <= BAR_QFRC_CONSTRAINT).all(), (labels[e], e, r[e])


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """Two identical handles, three steps; one calls kinematics before each.  State, obs, reward, done, sim time and diagnostics
    bit for bit."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, len(labels), cm.act_dim)).astype(np.float32)
    for s in range(3):
        before = a.state_tensors()
        diag = a.get_diag()
        a.kinematics()
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), s
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), s
        act = torch.from_numpy(acts[s]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), s
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), s
        assert torch.equal(a.sim_time, b.sim_time)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_diag(), b.get_diag())), s
    a.k_close(); b.k_close()


def test_launch_shapes_single_field_and_a_non_finite_env():
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm")
    # one env; three envs of a two-arm model (a ragged last wave)
    for model, n in ((cm, 1), (R.model("dual_arm"), 3)):
        small = env_hip.KManipEnvHip(model, num_envs=n, seed=3)
        small.k_reset()
        k = _host(small.kinematics())
        q, v = small.get_state()[:2]
        small.k_close()
        orc = Oracle(model, 1)
        figures, bad = [], []
        for e in range(n):
            bad += _compare(k, e, KO.decode(model, orc, q[e], v[e]), v[e], ("reset", e), figures)
        _report("%d env(s), %d links" % (n, model.nlink), figures)
        assert not bad, bad
    # every field NULL but one; and a reused `out`
    dev = _device(cm, qpos, qvel, ctrl, warm)
    full = dev.kinematics()
    only = dev.kinematics(fields=["site_jacp"])
    assert list(only) == ["site_jacp"] and torch.equal(only["site_jacp"], full["site_jacp"])
    mine = {"status": torch.full_like(full["status"], 7), "qM": torch.zeros_like(full["qM"])}
    again = dev.kinematics(out=mine)
    assert again is mine and torch.equal(again["qM"], full["qM"]) and not again["status"].any()
    with pytest.raises(ValueError):
        dev.kinematics(fields=["nonsense"])
    # NaN in one env's qpos: status 1 and zeros for that env, its neighbours' bits unchanged
    e = 5
    qn = qpos.copy()
    qn[e, 0] = np.nan
    dev.set_state(qpos=qn)
    g = dev.kinematics()
    dev.k_close()
    assert g["status"][e] == 1 and g["status"].sum() == 1
    for key in KO.FIELDS:
        assert not g[key][e].any(), key
    keep = torch.arange(len(labels), device=g["status"].device) != e
    for key in g:
        assert torch.equal(g[key][keep], full[key][keep]), key


def test_refusals_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.lib import KKinDev
    dev = env_hip.KManipEnvHip(R.model("solo_arm"), num_envs=4, seed=0)
    dev.k_reset()
    assert dev.L.kmanip_kinematics(dev.h, None, None) != 0
    assert b"KKinDev pointer is NULL" in dev.L.kmanip_last_error(dev.h)
    assert dev.L.kmanip_kinematics(None, None, None) != 0
    assert b"kmanip_kinematics: null handle" in dev.L.kmanip_last_error(None)
    assert dev.L.kmanip_kinematics(dev.h, C.byref(KKinDev()), None) == 0         # every field NULL: succeeds, does nothing
    dev.step_flat(torch.zeros((4, dev.cm.act_dim), dtype=torch.float32, device="cuda"))
    assert not dev.done.cpu().numpy().any()
    assert not dev.kinematics()["status"].any()
    dev.k_close()


def test_shell_reports_the_site_poses():
    torch = _torch()
    from gym_kmanip_amd.gym_shell import KManipEnv
    env = KManipEnv("KManipSoloArm", num_envs=8, ee_pose=True)
    plain = KManipEnv("KManipSoloArm", num_envs=8)
    _, info = env.reset()
    _, info0 = plain.reset()
    assert "site_xpos" not in info0 and "site_xmat" not in info0
    for s in range(2):
        for key, shape in (("site_xpos", (8, 2, 3)), ("site_xmat", (8, 2, 9))):
            t = info[key]
            assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape, key
        k = env.env.kinematics()
        assert torch.equal(info["site_xpos"], k["site_xpos"]) and torch.equal(info["site_xmat"], k["site_xmat"])
        assert info["site_xpos"][:, 0].abs().max() > 0 and not info["site_xpos"][:, 1].any()
        _, _, _, _, info = env.step({key: np.zeros((8,) + tuple(sp.shape), np.float32) for key, sp in env.action_space.spaces.items()})
    _, _, _, _, info0 = plain.step({key: np.zeros((8,) + tuple(sp.shape), np.float32) for key, sp in plain.action_space.spaces.items()})
    assert "site_xpos" not in info0 and "site_xmat" not in info0
    env.close(); plain.close()


@pytest.mark.parametrize("env_id", ["KManipSoloArmQPos", "KManipDualArmQPos"])
def test_resolved_rate_example_reaches_on_the_device(env_id):
    """gym_kmanip_amd/examples/resolved_rate_reach.py: 4 envs, 24 steps; the median site-to-goal distance falls below 0.6 x its
    start."""
    _torch()
    from gym_kmanip_amd.examples import resolved_rate_reach
    out = resolved_rate_reach.main(["--env", env_id, "--num-envs", "4", "--steps", "24", "--seed", "3"])
    print("\n%s: median site-to-goal distance %.4f -> %.4f m (%.2f x)" % (env_id, out["start"], out["end"], out["end"] / out["start"]))
    assert out["end"] < 0.6 * out["start"]
