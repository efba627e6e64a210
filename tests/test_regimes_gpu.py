"""k_step in the grasp, pinch, limit and impact states of tests/tools/regime_states.py (run with -m gpu on an MI355X).

Every other parity test takes its states from random rollouts, which reach these cells in fewer than 10 of the 468 states a step
matrix row compares (tests/test_regimes_cpu.py: the census).  Here one handle holds every cell's copies (47 envs for the single
arm, 72 for the two-arm models) and
  - runs three control steps against the oracle at the bars of test_gpu_parity (qpos / obs 1e-7, qvel 1e-5, reward 1e-6; ctrl, contact
    mask, done byte and step counter bit for bit), on zero and on small random actions;
  - repeats them with the envs in three orders at 2 (and 4) envs per wave against one env per wave, and in chunked launches:
    every env's bits the same;
  - holds and drops the grasped cube at twice and half the Coulomb friction, as the oracle does (test_regimes_cpu).
The models are the three assets in the joint-delta action mode (no IK between action and ctrl: ctrl must match bit for bit), plus
the grasp and the pinch on the registered EE-delta ids."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from regime_states import cells, loaded_oracle, model  # noqa: E402
from gym_kmanip_amd.model import KM_DONE_DIVERGED, compile_model  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_R, TOL_V  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _device(cm, qpos, qvel, ctrl, warm):
    from gym_kmanip_amd import env_hip
    n = len(qpos)
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=0)
    dev.k_reset()
    dev.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, step=np.zeros(n, dtype=np.int32))
    return dev


def _snapshot(dev):
    qpos, qvel, ctrl, warm, step = dev.get_state()
    return dict(qpos=qpos, qvel=qvel, ctrl=ctrl, step=step, obs=dev.obs.cpu().numpy(), reward=dev.reward.cpu().numpy(),
                done=dev.done.cpu().numpy(), mask=dev.get_diag()[0])


def _oracle_snapshot(orc, out):
    qpos, qvel, ctrl, warm, step = orc.get_state()
    return dict(qpos=qpos, qvel=qvel, ctrl=ctrl, step=step, obs=out[0], reward=out[1], done=out[2], mask=orc.get_diag()[0])


BARS = {"qpos": TOL_Q, "qvel": TOL_V, "obs": TOL_Q, "reward": TOL_R}
EXACT = ("ctrl", "mask", "done", "step")


def _diff(a, b, key):
    d = np.abs(a[key] - b[key])
    return d.reshape(len(d), -1).max(axis=1)


def _free_run(cm, states, labels, actions, ee_delta=False):
    """Three control steps of the device and of the oracle from the same arrays (warm from Oracle.after_reset, step 0), free
    running.  A second oracle starts from qvel * (1 + 1e-15): the spread between the two oracles is the reference's own error
    in the cell.  Measured over all cells, models, solvers and both action sets it is at most 3.3e-15 (qpos), 3.6e-13 (qvel),
    1.1e-13 (obs) and 9.8e-13 (reward), so every cell keeps the project's bars; the run FAILS if ten times a cell's spread ever
    exceeds its bar (an impact cell whose reference bifurcates would need a bar of its own, set here in the open, not a silent
    one).  Returns the worst difference per cell and quantity, the worst spread per cell, and the device's contact masks after
    every step."""
    torch = _torch()
    from oracle.oracle import Oracle
    qpos, qvel, ctrl = states
    n = len(labels)
    warm = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    orc = loaded_oracle(cm, qpos, qvel, ctrl)
    twin = loaded_oracle(cm, qpos, qvel * (1.0 + 1e-15), ctrl)
    cell_of = np.array(labels)
    worst = {c: {k: 0.0 for k in BARS} for c in dict.fromkeys(labels)}
    spread = {c: {k: 0.0 for k in BARS} for c in worst}
    masks, flips = [], 0
    for k in range(3):
        act = actions[k]
        dev.step_flat(torch.from_numpy(act).cuda())
        g = _snapshot(dev)
        o = _oracle_snapshot(orc, orc.step(act))
        t = _oracle_snapshot(twin, twin.step(act))
        masks.append(g["mask"].copy())
        assert not (g["done"] & KM_DONE_DIVERGED).any(), (k, list(cell_of[(g["done"] & KM_DONE_DIVERGED) != 0]))
        loose = np.zeros(n, dtype=bool)
        if ee_delta:                                         # float32 ctrl may straddle a rounding boundary: one ulp, that env x 10
            bad = g["ctrl"] != o["ctrl"]
            if bad.any():
                ulp = np.spacing(np.abs(o["ctrl"][bad]).astype(np.float32)).astype(np.float64)
                assert (np.abs(g["ctrl"][bad] - o["ctrl"][bad]) <= ulp).all(), ("ctrl", k)
                loose = bad.any(axis=1)
                flips += int(loose.sum())
        for key in EXACT:
            same = (g[key] == o[key]).reshape(n, -1).all(axis=1) | (loose if key == "ctrl" else False)
            assert same.all(), (key, k, [(cell_of[e], e) for e in np.where(~same)[0]])
        for key, bar in BARS.items():
            d, s = _diff(g, o, key), _diff(t, o, key)
            for c in worst:
                sel = cell_of == c
                worst[c][key] = max(worst[c][key], float(d[sel & ~loose].max(initial=0.0)))
                spread[c][key] = max(spread[c][key], float(s[sel].max()))
            for c in worst:
                assert 10.0 * spread[c][key] <= bar, ("the oracle's own spread in this cell is no longer far below the bar", c, key, spread[c][key])
            for e in range(n):
                lim = bar * (10.0 if loose[e] else 1.0)
                assert d[e] < lim, (key, k, cell_of[e], e, d[e], lim)
        if loose.any():
            sg = dev.get_state()
            orc.set_state(*sg); twin.set_state(*sg)
    dev.k_close()
    return worst, spread, masks, flips


def _report(tag, worst, spread):
    print("\n%s: worst |device - oracle| per cell (oracle's own spread under a 1e-15 relative change of qvel)" % tag)
    for c in worst:
        print("  %-5s %s" % (c, "  ".join("%s %.1e (%.1e)" % (k, worst[c][k], spread[c][k]) for k in BARS)))


def _actions(cm, n, kind, seed=3):
    if kind == "zero":
        return np.zeros((3, n, cm.act_dim), dtype=np.float32)
    return np.random.default_rng(seed).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)


@pytest.mark.parametrize("kind", ["zero", "random"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_cells_free_running_parity(asset, solver, kind):
    """Every cell's copies in one handle, three control steps, zero actions and actions uniform in +-0.2.  Also the coverage: the
    classifier finds every cell in the handle at step 0, and after the first step the device still has a grasp (G) env and, on
    the two-arm models, a pinch (P) env with a sphere on the cube.  Worst differences measured on an MI355X: DESIGN.md section 17."""
    from oracle.oracle import Oracle
    cm = model(asset, solver)
    qpos, qvel, ctrl, labels = cells(asset)
    one = Oracle(cm, 1)
    for e, cell in enumerate(labels):
        assert R.IN_CELL[cell](R.regime(cm, one, qpos[e], qvel[e], ctrl[e])), (cell, e)
    assert set(labels) == set(R.BUILDERS) - set(R.UNREACHABLE[asset])
    worst, spread, masks, _ = _free_run(cm, (qpos, qvel, ctrl), labels, _actions(cm, len(labels), kind))
    _report("%s %s %s" % (asset, solver, kind), worst, spread)
    coupled = (masks[0] & 0x000FFF00) != 0
    assert any(coupled[e] for e, c in enumerate(labels) if c[0] == "G")
    if cm.nlink == 20:
        assert any(coupled[e] for e, c in enumerate(labels) if c[0] == "P")


@pytest.mark.parametrize("env", ["KManipSoloArm", "KManipTorso"])
def test_grasp_and_pinch_on_the_ee_delta_ids(env):
    """G1 (and P1 on the Torso) once more with the IK between action and ctrl: the registered EE-delta ids, zero actions, the
    usual allowance for a float32 ctrl entry one ulp apart (that env alone at ten times the bars, the oracle then re-synchronised)."""
    from oracle.oracle import Oracle
    cm = compile_model(env, auto_reset=False)
    one = Oracle(cm, 1)
    rng = np.random.default_rng(1)
    parts, labels = [], []
    for cell in ("G1", "P1"):
        st = R.BUILDERS[cell](cm, one, rng)
        if st is not None:
            parts.append(st); labels += [cell] * len(st[0])
    states = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    for e, cell in enumerate(labels):
        assert R.IN_CELL[cell](R.regime(cm, one, states[0][e], states[1][e], states[2][e])), (cell, e)
    worst, spread, masks, flips = _free_run(cm, states, labels, _actions(cm, len(labels), "zero"), ee_delta=True)
    _report("%s (EE-delta)" % env, worst, spread)
    assert flips <= 2, flips
    assert ((masks[0] & 0x000FFF00) != 0).any()


def _orders(coupled):
    """cell-major (as built), interleaved (coupled and uncoupled envs alternate, so every wave of 2 or 4 that holds a coupled env
    holds an uncoupled one too, while there are coupled ones left) and reversed."""
    n = len(coupled)
    c = [e for e in range(n) if coupled[e]]
    u = [e for e in range(n) if not coupled[e]]
    inter = []
    for i in range(max(len(c), len(u))):
        inter += c[i:i + 1] + u[i:i + 1]
    return {"cell-major": np.arange(n), "interleaved": np.array(inter), "reversed": np.arange(n)[::-1].copy()}


def _mixed_waves(perm, coupled, epb):
    """Waves (epb consecutive envs of the handle) that hold a coupled and an uncoupled env."""
    c = np.asarray(coupled)[perm]
    return sum(1 for w in range(0, len(c), epb) if c[w:w + epb].any() and not c[w:w + epb].all())


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_wave_mates_order_and_chunk_change_no_bit(asset, solver, monkeypatch):
    """kmanip.h: "an env's bits depend neither on its wave-mates nor on the order its wave is dispatched in" -- where the joint
    loop's hand-over happens.  A handle this small would get one env per wave by itself (km_pick_epb), so the envs per wave are
    forced: the cells' copies in three orders with KMANIP_EPB = 2 (and 4 on the 10-link model), three steps of small random
    actions, against KMANIP_EPB = 1 in cell-major order: qpos, qvel, ctrl, obs, reward, done and contact mask of every env bit
    for bit the same.  In the interleaved order every wave of every forced shape that holds a coupled env holds an uncoupled one
    too, at least 9 such waves (asserted from the permutation).  step_chunk(3), which launches at the widest envs per wave, equals the three step_flat
    calls in cell-major and in interleaved order."""
    _wave_mates_change_no_bit(model(asset, solver), asset, monkeypatch)


def _wave_mates_change_no_bit(cm, asset, monkeypatch):
    """The body of test_wave_mates_order_and_chunk_change_no_bit for a compiled model of the asset (tests/test_solver_caps_gpu.py
    runs it with the Newton solver capped)."""
    torch = _torch()
    from oracle.oracle import Oracle
    qpos, qvel, ctrl, labels = cells(asset)
    n = len(labels)
    warm = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
    acts = _actions(cm, n, "random", seed=4)
    one = Oracle(cm, 1)
    coupled = [R.regime(cm, one, qpos[e], qvel[e], ctrl[e])["coupled"] for e in range(n)]
    assert 0 < sum(coupled) < n
    orders = _orders(coupled)
    epbs = (2, 4) if cm.nlink == 10 else (2,)
    for epb in epbs:                                         # every wave that holds a coupled env is a mixed one
        c = np.asarray(coupled)[orders["interleaved"]]
        assert _mixed_waves(orders["interleaved"], coupled, epb) == sum(1 for w in range(0, n, epb) if c[w:w + epb].any()) >= 9, epb

    def run(perm, epb, chunk=False):
        monkeypatch.setenv("KMANIP_EPB", str(epb)) if epb else monkeypatch.delenv("KMANIP_EPB", raising=False)
        assert sorted(perm) == list(range(n))
        inv = np.argsort(perm)
        dev = _device(cm, qpos[perm], qvel[perm], ctrl[perm], warm[perm])
        runs = []
        if chunk:
            obs_c, rew_c, done_c = dev.step_chunk(torch.from_numpy(np.ascontiguousarray(acts[:, perm])).cuda())
            runs = [dict(obs=obs_c[k].cpu().numpy()[inv], reward=rew_c[k].cpu().numpy()[inv], done=done_c[k].cpu().numpy()[inv]) for k in range(3)]
            runs[2].update({key: v[inv] for key, v in _snapshot(dev).items() if key in ("qpos", "qvel", "ctrl", "step", "mask")})
        else:
            for k in range(3):
                dev.step_flat(torch.from_numpy(np.ascontiguousarray(acts[k][perm])).cuda())
                runs.append({key: v[inv] for key, v in _snapshot(dev).items()})
        dev.k_close()
        return runs

    def same(runs, what):
        for k in range(3):
            for key in runs[k]:
                eq = (runs[k][key] == ref[k][key]).reshape(n, -1).all(axis=1)
                assert eq.all(), (what, k, key, [(labels[e], e) for e in np.where(~eq)[0]])

    ref = run(orders["cell-major"], 1)
    for epb in epbs:
        for name, perm in orders.items():
            same(run(perm, epb), (name, epb))
    for name in ("cell-major", "interleaved"):
        same(run(orders[name], None, chunk=True), (name, "chunk"))
    monkeypatch.delenv("KMANIP_EPB", raising=False)


@pytest.mark.parametrize("asset", ASSETS)
def test_grasp_holds_and_slips_at_the_coulomb_threshold_gpu(asset):
    """test_regimes_cpu's Coulomb check on the device, same state, same thresholds: env 0 with mu = 2 m g / (2 N) keeps the cube
    within 1 mm over 32 control steps, env 1 with mu = 0.5 m g / (2 N) has dropped it by more than 5 mm."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    cm, st, target, N = R.held_cube(asset)
    nl = cm.nlink
    two = [np.repeat(x, 2, axis=0) for x in st]
    dev = env_hip.KManipEnvHip(cm, num_envs=2, seed=0)
    dev.k_reset()
    dev.set_env_params(cube_friction=torch.tensor(R.coulomb_frictions(cm, N), dtype=torch.float64))
    dev.set_state(qpos=two[0], qvel=two[1], ctrl=two[2], warm=two[3], step=np.zeros(2, dtype=np.int32))
    for _ in range(R.HOLD_STEPS):
        dev.step_flat(torch.from_numpy(R.hold_action(cm, dev.get_state()[0], target)).cuda())
        assert not dev.done.cpu().numpy().any()
    dz = dev.get_state()[0][:, nl + 2] - st[0][0, nl + 2]
    print("\n%s: N = %.3f N, dz hold %+.3f mm, slip %+.3f mm" % (asset, N, 1e3 * dz[0], 1e3 * dz[1]))
    dev.k_close()
    assert abs(dz[0]) < 1e-3 and dz[1] < -5e-3, dz
