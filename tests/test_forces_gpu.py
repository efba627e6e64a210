"""kmanip_forces against the force oracle (run with -m gpu on an MI355X).

One handle per asset holds every regime cell's copies (tests/tools/regime_states.py: 47 envs for the single arm, 72 for the two-arm
models -- not a multiple of the 4 / 2 envs a wave holds), warm start from Oracle.after_reset.  Every field kmanip_forces writes is
compared with tests/tools/force_oracle.py, contact by contact through the mask bit, under the bars of tests/test_forces_cpu.py
(1000 x the oracle's own spread; geometry 1e-12).  Then: ctrl read as stored, per-env parameters on the device, the call after a
step, the handle left untouched, the launch shapes, the refusals and the Gymnasium shell's info keys."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import force_oracle as FO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_forces_cpu import BAR_CONTACT_FORCE, BAR_GEOMETRY, BAR_QACC, BAR_QFRC_ACTUATOR, BAR_QFRC_CONSTRAINT  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
FLOAT_FIELDS = ("qacc", "qfrc_constraint", "qfrc_actuator", "contact_force", "contact_frame", "contact_pos", "contact_dist")
UP = FO.make_frame([0.0, 0.0, 1.0])


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


def _host(f):
    out = {k: v.cpu().numpy() for k, v in f.items()}
    if "contact_mask" in out:
        out["contact_mask"] = out["contact_mask"].view(np.uint32)
    return out


def _slot_kind_ok(nlink, slot, bit):
    nss = 2 * (nlink // 10)
    return bit < 8 if slot < 4 else (8 <= bit < 20 if slot < 4 + nss else bit >= 20)


def _compare(cm, f, e, o, what, figures):
    """Every field of env e of a forces() result (host arrays) against the decode o.  Appends the normalised differences to
    `figures` and returns the list of violations."""
    nl = cm.nlink
    sq, sf, sa = FO.scales(o)
    bad = []
    if f["status"][e] != 0:
        return [(what, "status", int(f["status"][e]))]
    if int(f["contact_mask"][e]) != o["mask"]:
        return [(what, "mask", hex(int(f["contact_mask"][e])), hex(o["mask"]))]
    bits = f["contact_bit"][e]
    used = [int(b) for b in bits if b >= 0]
    if sorted(used) != FO.mask_bits(o["mask"]):
        return [(what, "contact_bit", used, FO.mask_bits(o["mask"]))]
    d = dict(qacc=float(np.abs(f["qacc"][e] - o["qacc"]).max()) / sq,
             qfrc_constraint=float(np.abs(f["qfrc_constraint"][e] - o["qfrc_constraint"]).max()) / sf,
             qfrc_actuator=float(np.abs(f["qfrc_actuator"][e] - o["qfrc_actuator"]).max()) / sa, contact_force=0.0, geometry=0.0)
    for s, b in enumerate(bits):
        if b < 0:                                            # an empty slot: every field zero
            if any(np.any(f[k][e, s] != 0) for k in ("contact_force", "contact_frame", "contact_pos", "contact_dist")):
                bad.append((what, "empty slot not zero", s))
            continue
        c = o["contacts"][int(b)]
        if not _slot_kind_ok(nl, s, int(b)):
            bad.append((what, "bit in a slot of another kind", s, int(b)))
        d["contact_force"] = max(d["contact_force"], float(np.abs(f["contact_force"][e, s] - c["force"]).max()) / sf)
        fr = f["contact_frame"][e, s].reshape(3, 3)
        normal = c["normal"] if c["normal"] is not None else UP[:3]      # the oracle's own normal (rows of its J); table pairs: +z
        g = max(float(np.abs(fr @ fr.T - np.eye(3)).max()), float(np.abs(fr[0] - normal).max()),
                float(np.abs(fr.reshape(-1) - c["frame"]).max()), float(np.abs(f["contact_pos"][e, s] - c["pos"]).max()),
                abs(float(f["contact_dist"][e, s]) - c["dist"]))
        d["geometry"] = max(d["geometry"], g)
    figures.append((what, d))
    bars = dict(qacc=BAR_QACC, qfrc_constraint=BAR_QFRC_CONSTRAINT, qfrc_actuator=BAR_QFRC_ACTUATOR, contact_force=BAR_CONTACT_FORCE,
                geometry=BAR_GEOMETRY)
    bad += [(what, k, v, bars[k]) for k, v in d.items() if not v <= bars[k]]
    return bad


def _report(tag, figures):
    worst = {}
    for what, d in figures:
        for k, v in d.items():
            if v >= worst.get(k, (-1.0, None))[0]:
                worst[k] = (v, what)
    print("\n%s: worst normalised |device - oracle|: %s" % (tag, "  ".join("%s %.1e %s" % (k, v, w) for k, (v, w) in worst.items())))


@pytest.mark.parametrize("asset", ASSETS)
def test_parity_with_the_force_oracle_on_every_cell(asset):
    """Worst normalised differences measured on an MI355X: DESIGN.md section 19."""
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    _, dec, _ = FO.cell_decodes(asset)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    full = dev.forces()
    f = _host(full)
    by_bit, finger = dev.normal_by_bit(full).cpu().numpy(), dev.finger_force(full).cpu().numpy()
    dev.k_close()
    figures, bad = [], []
    for e, o in enumerate(dec):
        bad += _compare(cm, f, e, o, (labels[e], e), figures)
        want = np.zeros(32)
        for b, c in o["contacts"].items():
            want[b] = c["force"][0]
        if not np.abs(by_bit[e] - want).max() / FO.scales(o)[1] <= BAR_CONTACT_FORCE or (by_bit[e][want == 0] != 0).any():
            bad.append(((labels[e], e), "normal_by_bit"))
    _report(asset, figures)
    assert not bad, bad
    assert finger.shape == (len(labels), 2 * (cm.nlink // 10)) and np.array_equal(finger, by_bit[:, 8:8 + finger.shape[1]])
    assert max((b >= 0).sum() for b in f["contact_bit"]) >= (7 if cm.nlink == 10 else 8)
    assert f["contact_force"][:, :, 0].max() > 30.0


def test_ctrl_is_read_as_stored():
    """One env whose ctrl is its cell's + 1e-9 -- not a float32 number: the float32 rounding of before_step would move a servo force
    by kp x 1e-9 = 2e-7 .. 1e-6 N, 1e4 times the bar."""
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm")
    e = labels.index("G1")
    c = ctrl[e] + 1e-9
    assert (c != c.astype(np.float32).astype(np.float64)).all()
    dev = _device(cm, qpos[e:e + 1], qvel[e:e + 1], c[None], warm[e:e + 1])
    f = _host(dev.forces())
    assert (dev.get_state()[2][0] == c).all()
    dev.k_close()
    orc = Oracle(cm, 1)
    o = FO.decode(cm, orc, qpos[e], qvel[e], c)
    rounded = FO.decode(cm, orc, qpos[e], qvel[e], c.astype(np.float32).astype(np.float64), geometry=False)
    assert np.abs(rounded["qfrc_actuator"] - o["qfrc_actuator"]).max() / FO.scales(o)[2] > 1e3 * BAR_QFRC_ACTUATOR
    figures = []
    bad = _compare(cm, f, 0, o, ("G1", e), figures)
    _report("ctrl + 1e-9", figures)
    assert not bad, bad


@pytest.mark.parametrize("asset", ASSETS)
def test_per_env_parameters_on_the_device(asset):
    """set_env_params (cube mass x 2, friction 0.5, friction loss 0, kp scale 1.3) against the with_env_params oracle on the grasp
    and pinch cells; and, for every env of the handle, the cube identity: with no friction loss on the cube, the linear part of
    its qfrc_constraint is the summed world force of the slots whose bit is a cube pair."""
    from gym_kmanip_amd.model import with_env_params
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    nl = cm.nlink
    p = dict(cube_mass=2.0 * cm.desc.cube_mass, cube_friction=0.5, cube_frictionloss=0.0, kp_scale=1.3)
    cmp_ = with_env_params(cm, **p)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    dev.set_env_params(**p)
    f = _host(dev.forces())
    dev.k_close()
    orc = Oracle(cmp_, 1)
    figures, bad = [], []
    chosen = [e for e, c in enumerate(labels) if c[0] in "GP" or c == "T1G2"]
    assert len(chosen) >= 18
    for e in chosen:
        o = FO.decode(cmp_, orc, qpos[e], qvel[e], ctrl[e])
        assert o["mask"] & 0x000FFF00
        bad += _compare(cmp_, f, e, o, (labels[e], e), figures)
    _report(asset + " with parameters", figures)
    worst = 0.0
    for e in range(len(labels)):
        assert f["status"][e] == 0
        tot = np.zeros(3)
        for s, b in enumerate(f["contact_bit"][e]):
            if 0 <= b < 20:
                tot += f["contact_force"][e, s, :3] @ f["contact_frame"][e, s].reshape(3, 3)
        r = float(np.abs(tot - f["qfrc_constraint"][e, nl:nl + 3]).max()) / max(1.0, float(np.abs(f["qfrc_constraint"][e]).max()))
        worst = max(worst, r)
        if not r <= BAR_CONTACT_FORCE:
            bad.append(((labels[e], e), "cube identity", r))
    print("%s: cube identity, worst %.1e" % (asset, worst))
    assert not bad, bad


@pytest.mark.parametrize("asset", ASSETS)
def test_forces_after_a_step_use_the_state_the_step_left(asset):
    """One step_flat with small actions, then forces on the same stream: compared with the oracle at the device's own read-back
    state.  The device starts its solve from the warm start the step stored, the oracle from zero."""
    torch = _torch()
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    act = np.random.default_rng(5).uniform(-0.2, 0.2, (len(labels), cm.act_dim)).astype(np.float32)
    dev.step_flat(torch.from_numpy(act).cuda())
    f = _host(dev.forces())
    q1, v1, c1, w1, _ = dev.get_state()
    assert not dev.done.cpu().numpy().any() and np.abs(w1).max() > 0
    dev.k_close()
    orc = Oracle(cm, 1)
    figures, bad = [], []
    for e in range(len(labels)):
        bad += _compare(cm, f, e, FO.decode(cm, orc, q1[e], v1[e], c1[e]), (labels[e], e), figures)
    _report(asset + " after a step", figures)
    assert not bad, bad


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """Two identical handles, three steps; one calls forces before each.  State, obs, reward, done and diagnostics bit for bit."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, len(labels), cm.act_dim)).astype(np.float32)
    for k in range(3):
        before = a.state_tensors()
        diag = a.get_diag()
        a.forces()
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), k
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), k
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), k
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
        assert torch.equal(a.sim_time, b.sim_time)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_diag(), b.get_diag())), k
    a.k_close(); b.k_close()


def test_launch_shapes_single_field_and_a_non_finite_env():
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm")
    # one env
    one = env_hip.KManipEnvHip(cm, num_envs=1, seed=3)
    one.k_reset()
    f1 = _host(one.forces())
    q, v, c, _, _ = one.get_state()
    one.k_close()
    figures = []
    bad = _compare(cm, f1, 0, FO.decode(cm, Oracle(cm, 1), q[0], v[0], c[0]), ("reset", 0), figures)
    _report("one env", figures)
    assert not bad, bad
    # every field NULL but one; and a reused `out`
    dev = _device(cm, qpos, qvel, ctrl, warm)
    full = dev.forces()
    only = dev.forces(fields=["contact_force"])
    assert list(only) == ["contact_force"] and torch.equal(only["contact_force"], full["contact_force"])
    again = dev.forces(out={"status": torch.full_like(full["status"], 7), "qacc": torch.zeros_like(full["qacc"])})
    assert torch.equal(again["qacc"], full["qacc"]) and not again["status"].any()
    with pytest.raises(ValueError):
        dev.forces(fields=["nonsense"])
    # NaN in one env's qpos: status 1 and zeros for that env, its neighbours' bits unchanged
    e = 5
    qn = qpos.copy()
    qn[e, 0] = np.nan
    dev.set_state(qpos=qn)
    g = dev.forces()
    dev.k_close()
    assert g["status"][e] == 1 and g["status"].sum() == 1
    assert (g["contact_bit"][e] == -1).all() and g["contact_mask"][e] == 0
    for key in FLOAT_FIELDS:
        assert not g[key][e].any(), key
    keep = torch.arange(len(labels), device=g["status"].device) != e
    for key in g:
        assert torch.equal(g[key][keep], full[key][keep]), key


def test_refusals_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.lib import KManipError
    pgs = env_hip.KManipEnvHip(R.model("solo_arm", "pgs"), num_envs=4, seed=0)
    pgs.k_reset()
    with pytest.raises(KManipError, match="contact forces need the Newton solver"):
        pgs.forces()
    pgs.step_flat(torch.zeros((4, pgs.cm.act_dim), dtype=torch.float32, device="cuda"))
    assert not pgs.done.cpu().numpy().any()
    pgs.k_close()
    dev = env_hip.KManipEnvHip(R.model("solo_arm"), num_envs=4, seed=0)
    dev.k_reset()
    assert dev.L.kmanip_forces(dev.h, None, None) != 0
    assert b"KForcesDev pointer is NULL" in dev.L.kmanip_last_error(dev.h)
    assert dev.L.kmanip_forces(None, None, None) != 0
    from gym_kmanip_amd.lib import KForcesDev
    assert dev.L.kmanip_forces(dev.h, C.byref(KForcesDev()), None) == 0          # every field NULL: succeeds, does nothing
    assert not dev.forces()["status"].any()
    dev.k_close()


def test_shell_reports_finger_force_and_qfrc_actuator():
    torch = _torch()
    from gym_kmanip_amd.gym_shell import KManipEnv
    env = KManipEnv("KManipSoloArm", num_envs=8, contact_forces=True)
    plain = KManipEnv("KManipSoloArm", num_envs=8)
    _, info = env.reset()
    _, info0 = plain.reset()
    assert "finger_force" not in info0 and "qfrc_actuator" not in info0
    for k in range(2):
        for key, shape in (("finger_force", (8, 2)), ("qfrc_actuator", (8, env.q_len))):
            t = info[key]
            assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape, key
        f = env.env.forces()
        assert torch.equal(info["finger_force"], env.env.finger_force(f)) and torch.equal(info["qfrc_actuator"], f["qfrc_actuator"])
        assert tuple(env.env.normal_by_bit(f).shape) == (8, 32)
        _, _, _, _, info = env.step({key: np.zeros((8,) + tuple(sp.shape), np.float32) for key, sp in env.action_space.spaces.items()})
    env.close(); plain.close()
