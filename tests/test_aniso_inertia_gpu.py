"""The device's dynamics on models with ANISOTROPIC link and cube inertias (run with -m gpu on an MI355X).

Every other GPU test runs the shipped, isotropic assets, on which R diag(I) R^T = I 1 and w x I w = 0: none of the device's copies
of that arithmetic (the composite inertias and the link wrenches of kmanip_dyn_tree.hpp, through LDS and through registers; the
cube's bias; the per-env scaled cube inertia; the cube's 1 / I_k of the constraint solves; the qM block of kmanip_kinematics) could
be told from a wrong version of itself.  Here the models are tests/tools/aniso_model.py's (three different principal values on every
link and on the cube) and the handle of a case holds the asset's regime cells plus 16 random states with velocity on every dof
(tests/test_aniso_inertia_cpu.states: 63 / 88 / 88 envs), nothing larger:
  kinematics()  every field against kin_oracle.decode at the bars of test_kinematics_gpu, and qM / qfrc_bias against the Lagrange
                reference (tests/tools/lagrange_oracle.py, no CRBA, no RNE) at the bars of test_aniso_inertia_cpu; with heterogeneous
                per-env cube masses; on a PGS handle; on the two-row path without the block split;
  forces()      qacc, qfrc_constraint, qfrc_actuator and the contact forces against force_oracle at the bars of test_forces_gpu;
  the step      test_regimes_gpu._free_run (its bars, its guard) on the cells plus the C1 / C2 placements with the cube spinning at
                5 rad/s about a body axis that is not a principal one; a rollout across the auto-reset in the shape and at the
                tolerances of test_gpu_parity.test_step_parity_vs_oracle;
  launch shapes one env per wave against the default and the widest shape, and one step_chunk against single steps: every bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import aniso_model as AM  # noqa: E402
import force_oracle as FO  # noqa: E402
import kin_oracle as KO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import test_forces_gpu as TF  # noqa: E402
import test_gpu_parity as TP  # noqa: E402
import test_kinematics_gpu as TK  # noqa: E402
import test_regimes_gpu as TR  # noqa: E402
from gym_kmanip_amd.model import compile_model, with_env_params  # noqa: E402
from test_aniso_inertia_cpu import N_RANDOM, bias_bar, m_bar, states  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")
SPIN = 5.0 * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)       # rad/s, body frame: no principal axis, no symmetry plane

_WARM = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _case(asset):
    """states(asset) plus the warm start of every state, computed once."""
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, labels, refs = states(asset)
    if asset not in _WARM:
        _WARM[asset] = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
    return cm, qpos, qvel, ctrl, _WARM[asset], labels, refs


def _against_lagrange(k, e, M, bias, bar_m, bar_b, what, figures):
    """qM and qfrc_bias of env e against the Lagrange reference: the violations; the figures in bars."""
    dM, db = float(np.abs(k["qM"][e] - M).max()), float(np.abs(k["qfrc_bias"][e] - bias).max())
    figures.append((what, dict(qM=dM / bar_m, qfrc_bias=db / bar_b)))
    return [(what, "Lagrange " + name, v, bar) for name, v, bar in (("qM", dM, bar_m), ("qfrc_bias", db, bar_b)) if not v <= bar]


def _kinematics_case(cm, k, qpos, qvel, labels, refs, tag):
    from oracle.oracle import Oracle
    orc = Oracle(cm, 1)
    figures, lag, bad = [], [], []
    for e, ref in enumerate(refs):
        what = (labels[e], e)
        bad += TK._compare(k, e, KO.decode(cm, orc, qpos[e], qvel[e]), qvel[e], what, figures)
        bad += _against_lagrange(k, e, ref["M"], ref["bias"], m_bar(ref), bias_bar(ref), what, lag)
    TK._report(tag, figures)
    TK._report(tag + ", Lagrange reference, in bars", lag)
    assert not bad, bad
    assert not k["status"].any()
    TK._structure(cm, k)
    d = cm.desc
    cube = np.diag([d.cube_mass] * 3 + list(d.cube_inertia))
    assert all(np.array_equal(M[cm.nlink:, cm.nlink:], cube) for M in k["qM"]) and len(set(np.diag(cube)[3:])) == 3


@pytest.mark.parametrize("asset", ASSETS)
def test_kinematics_against_the_oracle_and_the_lagrange_reference(asset):
    cm, qpos, qvel, ctrl, warm, labels, refs = _case(asset)
    dev = TK._device(cm, qpos, qvel, ctrl, warm)
    k = TK._host(dev.kinematics())
    dev.k_close()
    _kinematics_case(cm, k, qpos, qvel, labels, refs, asset + " anisotropic")


def test_kinematics_on_the_two_row_path_without_the_block_split(monkeypatch):
    cm, qpos, qvel, ctrl, warm, labels, refs = _case("dual_arm")
    monkeypatch.setenv("KMANIP_NO_BLOCK_SPLIT", "1")
    dev = TK._device(cm, qpos, qvel, ctrl, warm)
    monkeypatch.delenv("KMANIP_NO_BLOCK_SPLIT")
    k = TK._host(dev.kinematics())
    dev.k_close()
    _kinematics_case(cm, k, qpos, qvel, labels, refs, "dual_arm anisotropic without the block split")


@pytest.mark.parametrize("asset", ["solo_arm", "torso"])
def test_kinematics_with_a_different_cube_mass_in_every_env(asset):
    """Explicit per-env cube masses from 0.5 to 3 times the model's: env e against the oracle of with_env_params(aniso(cm),
    cube_mass = m_e), and against the Lagrange reference with the three cube values scaled by m_e / m0."""
    torch = _torch()
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels, refs = _case(asset)
    nl, n = cm.nlink, len(labels)
    m0 = cm.desc.cube_mass
    mass = m0 * np.linspace(0.5, 3.0, n)[np.random.default_rng(2).permutation(n)]
    dev = TK._device(cm, qpos, qvel, ctrl, warm)
    dev.set_env_params(cube_mass=torch.tensor(mass, dtype=torch.float64))
    k = TK._host(dev.kinematics())
    dev.k_close()
    I, _ = AM.inertias(cm)
    g = np.array(list(cm.desc.gravity))
    figures, lag, bad = [], [], []
    for e, ref in enumerate(refs):
        what = (labels[e], e)
        cme = with_env_params(cm, cube_mass=float(mass[e]))
        Ic = np.array(list(cme.desc.cube_inertia))
        assert np.array_equal(Ic, np.array(AM.CUBE_INERTIA) * (mass[e] / m0))
        bad += TK._compare(k, e, KO.decode(cme, Oracle(cme, 1), qpos[e], qvel[e]), qvel[e], what, figures)
        M, bias = ref["M"].copy(), ref["bias"].copy()
        M[nl:, nl:] = np.diag([mass[e]] * 3 + list(Ic))
        bias[nl:nl + 3], bias[nl + 3:] = -mass[e] * g, ref["state"].cube_euler(Ic)
        bad += _against_lagrange(k, e, M, bias, m_bar(ref), bias_bar(ref), what, lag)
        assert np.array_equal(np.diag(k["qM"][e])[nl:], [mass[e]] * 3 + list(Ic)), what
    TK._report(asset + " anisotropic, per-env cube masses", figures)
    TK._report(asset + " anisotropic, per-env cube masses, Lagrange reference, in bars", lag)
    assert not bad, bad
    assert len(set(mass)) == n


def test_a_pgs_handle_returns_the_newton_handles_bits():
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels, refs = _case("solo_arm")
    newton = TK._device(cm, qpos, qvel, ctrl, warm)
    pgs = TK._device(AM.aniso(R.model("solo_arm", "pgs")), qpos, qvel, ctrl, warm)
    a, b = newton.kinematics(), pgs.kinematics()
    newton.k_close(); pgs.k_close()
    assert set(a) == set(b) and all(torch.equal(a[name], b[name]) for name in a)
    assert not a["status"].any() and a["qM"].abs().max() > 0


@pytest.mark.parametrize("asset", ASSETS)
def test_forces_against_the_force_oracle(asset):
    """Every regime cell (the random states ride along: status 0).  The cells with a sphere on the cube press it off-centre: the
    torque reaches the cube's angular rows, where the solve divides by I_k axis by axis."""
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, warm, labels, refs = _case(asset)
    nl = cm.nlink
    dev = TF._device(cm, qpos, qvel, ctrl, warm)
    f = TF._host(dev.forces())
    dev.k_close()
    orc = Oracle(cm, 1)
    figures, bad, torque = [], [], 0
    assert not f["status"].any()
    for e in range(len(labels) - N_RANDOM):
        o = FO.decode(cm, orc, qpos[e], qvel[e], ctrl[e])
        bad += TF._compare(cm, f, e, o, (labels[e], e), figures)
        if o["mask"] & 0x000FFF00 and np.abs(o["qfrc_constraint"][nl + 3:]).max() > 1e-3:
            torque += 1
    TF._report(asset + " anisotropic", figures)
    assert not bad, bad
    assert torque >= 6, torque


def _spinning(cm, states3, labels):
    """The C1 and C2 placements once more (labels C1s, C2s), the cube spinning at SPIN.  Impact rows by construction: a C1 cube
    starts with corners under the table top, a C2 cube at most 3 mm over it and falling at 1 m/s or more."""
    nl = cm.nlink
    rows = [e for e, c in enumerate(labels) if c in ("C1", "C2")]
    assert len(rows) == 2 * R.J_COPIES
    for e in rows:
        low = R.cube_corners_z(cm, states3[0][e]).min() - cm.desc.table_z
        assert low < 0 if labels[e] == "C1" else (low <= 3e-3 and states3[1][e][nl + 2] <= -1.0), (labels[e], e, low)
    extra = [a[rows].copy() for a in states3]
    extra[1][:, nl + 3:nl + 6] = SPIN
    return tuple(np.concatenate([a, x]) for a, x in zip(states3, extra)), list(labels) + [labels[e] + "s" for e in rows]


@pytest.mark.parametrize("kind", ["zero", "random"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_cells_free_running_parity(asset, solver, kind):
    """test_regimes_gpu._free_run on the anisotropic model: the cells' states (built from geometry: they carry over unchanged) plus
    the spinning corner placements; three control steps at its bars, with its guard on the oracle's own spread."""
    cm = AM.aniso(R.model(asset, solver))
    qpos, qvel, ctrl, labels = R.cells(asset)
    st, labels = _spinning(cm, (qpos, qvel, ctrl), labels)
    worst, spread, masks, _ = TR._free_run(cm, st, labels, TR._actions(cm, len(labels), kind))
    TR._report("%s anisotropic %s %s" % (asset, solver, kind), worst, spread)
    coupled = (masks[0] & 0x000FFF00) != 0
    assert any(coupled[e] for e, c in enumerate(labels) if c[0] == "G")
    on_table = [any(masks[s][e] & 0xFF for s in range(3)) for e, c in enumerate(labels) if c in ("C1s", "C2s")]
    assert len(on_table) == 2 * R.J_COPIES and any(on_table)            # (the masks are sampled at the steps' ends, between bounces)


@pytest.mark.parametrize("solver", ["pgs", "newton"])
@pytest.mark.parametrize("env,n,steps", [("KManipSoloArm", 32, 70), ("KManipDualArm", 16, 66), ("KManipTorso", 16, 66)])
def test_rollout_across_the_auto_reset(env, n, steps, solver):
    """test_gpu_parity.test_step_parity_vs_oracle on the anisotropic models: full episodes on identical seeded actions, its
    comparisons and tolerances.  A float32 ctrl entry that straddles a rounding boundary re-synchronises the oracle, as there; at
    most twice per run, the bound of its least determinate variant."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from oracle.oracle import Oracle
    cm = AM.aniso(compile_model(env, auto_reset=True, solver=solver))
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=5, env_id_offset=7)
    orc = Oracle(cm, n, seed=5, env_id_offset=7)
    dev.k_reset(); orc.reset()
    rng = np.random.default_rng(42)
    saw_contact = saw_reset = False
    resync = [0]
    for k in range(steps):
        act = rng.uniform(-1, 1, (n, cm.act_dim)).astype(np.float32)
        dev.step_flat(torch.from_numpy(act).cuda())
        oo, ro, do = orc.step(act)
        flip = TP._cmp_state(dev, orc, k, resync)
        assert (np.abs(dev.obs.cpu().numpy() - oo) < np.where(flip, 10 * TP.TOL_V, TP.TOL_Q)[:, None]).all(), k
        assert (np.abs(dev.reward.cpu().numpy() - ro) < np.where(flip, 10 * TP.TOL_R, TP.TOL_R)).all(), k
        assert np.array_equal(dev.done.cpu().numpy(), do), k
        mg, nfg, stg = dev.get_diag(); mo, nfo, sto = orc.get_diag()
        assert np.array_equal(mg, mo), (k, mg, mo)
        assert np.array_equal(stg == -2, sto == -2) and np.abs(nfg - nfo).max() <= 1, k
        saw_contact |= bool(mg.any()); saw_reset |= bool(do.any())
    dev.k_close()
    print("\n%s %s anisotropic: %d ctrl re-synchronisations" % (env, solver, resync[0]))
    assert saw_contact and saw_reset
    assert resync[0] <= 2, resync


@pytest.mark.parametrize("asset", ["solo_arm", "torso"])
def test_launch_shapes_change_no_bit(asset, monkeypatch):
    """The handle of the kinematics case (cells and random states) through three steps of small random actions: one env per wave
    (KMANIP_EPB=1) against the default shape, against the widest shape (4 / 2 envs per wave), and against one step_chunk(3).
    qpos, qvel, ctrl, obs, reward, done, step counter and contact mask of every env, bit for bit."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels, refs = _case(asset)
    n = len(labels)
    acts = TR._actions(cm, n, "random", seed=4)

    def run(epb, chunk=False):
        monkeypatch.setenv("KMANIP_EPB", str(epb)) if epb else monkeypatch.delenv("KMANIP_EPB", raising=False)
        dev = TR._device(cm, qpos, qvel, ctrl, warm)
        runs = []
        if chunk:
            obs_c, rew_c, done_c = dev.step_chunk(torch.from_numpy(acts).cuda())
            runs = [dict(obs=obs_c[s].cpu().numpy(), reward=rew_c[s].cpu().numpy(), done=done_c[s].cpu().numpy()) for s in range(3)]
            runs[2].update({key: v for key, v in TR._snapshot(dev).items() if key in ("qpos", "qvel", "ctrl", "step", "mask")})
        else:
            for s in range(3):
                dev.step_flat(torch.from_numpy(acts[s]).cuda())
                runs.append(TR._snapshot(dev))
        dev.k_close()
        return runs

    ref = run(1)
    assert np.abs(ref[2]["qpos"] - qpos).max() > 0 and not (ref[2]["done"] & 2).any()
    for what, runs in (("default", run(None)), ("widest", run(4 if cm.nlink == 10 else 2)), ("chunk", run(None, chunk=True))):
        for s in range(3):
            for key in runs[s]:
                eq = (runs[s][key] == ref[s][key]).reshape(n, -1).all(axis=1)
                assert eq.all(), (what, s, key, [(labels[e], e) for e in np.where(~eq)[0]])
    monkeypatch.delenv("KMANIP_EPB", raising=False)
    assert n == len(R.cells(asset)[3]) + N_RANDOM
