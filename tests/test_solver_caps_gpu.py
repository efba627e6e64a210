"""k_step and the row kernels at small iteration caps and loose tolerances (run with -m gpu on an MI355X).

tests/test_solver_caps_cpu.py pins the reference side: on the regime cells the oracle's Newton solves never come near the default
cap of 100, so only a small cap runs the `iter + 1 >= maxit` exit of newton_loop_sl, the arm -> cube switch it triggers inside the
joint loop and the iteration count the joint loop hands to an uncoupled env's own loops; a cap of 0 must do no iteration at all.
Here the device runs the cells at the settings of that module:
  a. free running against the oracle at every setting, through test_regimes_gpu._free_run as it stands;
  b. wave-mates, dispatch order and chunked launches change no bit at caps 1 and 3;
  c. a cap of 1000 gives the bytes of cap 100;
  d. forward() and rollout() read the same cap;
  e. kmanip_create still refuses a negative cap."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402
from regime_states import cells  # noqa: E402
from test_forces_cpu import BAR_QACC  # noqa: E402
from test_regimes_gpu import _actions, _device, _free_run, _report, _snapshot, _wave_mates_change_no_bit  # noqa: E402
from test_rollout_gpu import _against_the_oracle, _dev_rows, _fresh, _host  # noqa: E402
from test_solver_caps_cpu import SETTINGS, capped_model  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
FREE_ROWS = [(a, s, cap, tol) for a in ASSETS for s in ("newton", "pgs") for cap, tol in SETTINGS[s]]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# ------------------------------------------------------------------------------------------------- a. free running at each setting
@pytest.mark.parametrize("asset,solver,cap,tol", FREE_ROWS)
def test_free_running_parity_at_each_setting(asset, solver, cap, tol):
    """Every cell's copies in one handle, three control steps of actions uniform in +-0.2, device against oracle through
    _free_run: its bars (qpos / obs 1e-7, qvel 1e-5, reward 1e-6), its exact fields (ctrl, contact mask, done byte, step counter),
    its condition that ten times the oracle's own spread stays under every bar.  Both sides start from the warm start the capped
    model's Oracle.after_reset gives.  Worst differences measured on an MI355X: DESIGN.md section 32."""
    cm = capped_model(asset, solver, cap, tol)
    assert cm.desc.solver_iterations == cap and cm.desc.solver_tolerance == tol
    qpos, qvel, ctrl, labels = cells(asset)
    worst, spread, masks, _ = _free_run(cm, (qpos, qvel, ctrl), labels, _actions(cm, len(labels), "random"))
    _report("%s %s cap %d tolerance %.0e" % (asset, solver, cap, tol), worst, spread)
    assert ((masks[0] & 0x000FFF00) != 0).any() and ((masks[0] & 0x000FFF00) == 0).any()      # coupled and uncoupled envs ran


# ------------------------------------------------------------------------------------- b. wave-mates change no bit under a cap
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("asset", ASSETS)
def test_wave_mates_order_and_chunk_change_no_bit_under_a_cap(asset, cap, monkeypatch):
    """test_regimes_gpu.test_wave_mates_order_and_chunk_change_no_bit with the Newton solver capped at 1 and at 3 iterations: every
    solve of the interleaved order's mixed waves now leaves the joint loop through the cap -- the coupled env at `cap` iterations,
    its uncoupled wave-mate through the capped arm -> cube switch or, once the coupled env is done, through the hand-over of its
    problem, cost and iteration count to its own loops, which must stop at the same count.  The cells' copies in three orders with
    KMANIP_EPB = 2 (and 4 on the 10-link model), three steps of small random actions, against KMANIP_EPB = 1 in cell-major order:
    every field of every env bit for bit the same; step_chunk(3) likewise.  In the interleaved order every wave that holds a coupled
    env holds an uncoupled one too, at least 9 such waves."""
    _wave_mates_change_no_bit(capped_model(asset, "newton", cap, 1e-8), asset, monkeypatch)


# --------------------------------------------------------------------------------------------------- c. the cap enters nowhere else
@pytest.mark.parametrize("asset", ASSETS)
def test_a_cap_no_solve_reaches_changes_no_byte(asset):
    """No Newton solve of this run reaches 100 iterations (test_solver_caps_cpu: the sum over a control step's sub-steps and both
    problems stays below 100), so the cap is read by nothing but the exit test: at a cap of 1000 qpos, qvel, ctrl, step counter, obs,
    reward, done byte and contact mask of every cell are the bytes of cap 100, after each of three control steps."""
    torch = _torch()
    from oracle.oracle import Oracle
    qpos, qvel, ctrl, labels = cells(asset)
    n = len(labels)
    runs = []
    for cap in (100, 1000):
        cm = capped_model(asset, "newton", cap, 1e-8)
        acts = _actions(cm, n, "random")
        dev = _device(cm, qpos, qvel, ctrl, R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl))
        snaps = []
        for k in range(3):
            dev.step_flat(torch.from_numpy(acts[k]).cuda())
            snaps.append(_snapshot(dev))
        dev.k_close()
        runs.append(snaps)
    for k in range(3):
        for key in runs[0][k]:
            eq = (runs[0][k][key] == runs[1][k][key]).reshape(n, -1).all(axis=1)
            assert eq.all(), (k, key, [(labels[e], e) for e in np.where(~eq)[0]])


# -------------------------------------------------------------------------------------------------- d. the row kernels read the cap
_ROW_RUNS = {}


def _row_run(asset, cap):
    """rollout_oracle.cell_runs' dict for the Newton model at a cap: the cells as caller rows of a 2-env handle, one mj_step (nsub = 1,
    nstep = 1) on OracleRollout, the twin from qvel (1 + 1e-15).  The oracle's own qacc of that step is the qacc_warm it leaves."""
    from oracle.oracle import Oracle
    if (asset, cap) not in _ROW_RUNS:
        cm = capped_model(asset, "newton", cap, 1e-8)
        qpos, qvel, ctrl, labels = cells(asset)
        n = len(labels)
        rows = dict(envs=(np.arange(n) % 2).astype(np.int32), qpos=qpos, qvel=qvel, ctrl=ctrl, warm=R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl))
        twin = dict(rows, qvel=qvel * (1.0 + 1e-15))
        env = RO.OracleRollout(cm, 2)
        _ROW_RUNS[(asset, cap)] = dict(cm=cm, rows=rows, labels=labels, ref=env.rollout(nstep=1, nsub=1, **rows),
                                       twin=env.rollout(nstep=1, nsub=1, **twin), twin_rows=np.arange(n))
    return _ROW_RUNS[(asset, cap)]


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_forward_and_rollout_read_the_same_cap(asset, cap):
    """More rows than envs on a handle of 2 envs, Newton, caps 0 and 1.  forward(): qacc of every cell against the capped
    oracle's -- forward_oracle.row solves to the exact minimiser whatever the cap, so the reference is the qacc the oracle's own
    solver, started from the row's warm start, leaves in qacc_warm after one mj_step -- at BAR_QACC over max(1, max|qacc|), the
    normalisation of the forces tests; the rows are far from converged (asserted against the converged model's qacc).
    rollout(nsub = 1, nstep = 1): qpos, qvel and reward under test_rollout_gpu's bars, mask, status and steps_done exactly."""
    from oracle.oracle import Oracle
    run = _row_run(asset, cap)
    cm, rows, labels = run["cm"], run["rows"], run["labels"]
    n = len(labels)
    dev = _fresh(cm, 2)
    f = _host(dev.forward(**_dev_rows(rows), fields=["qacc", "contact_mask", "status"]))
    got = _host(dev.rollout(**_dev_rows(rows), nsub=1, nstep=1))
    dev.k_close()
    assert n > 2 and f["qacc"].shape == (n, cm.nv) and not f["status"].any()
    want = run["ref"]["qacc_warm"][:, 0]
    scale = np.maximum(1.0, np.abs(want).max(axis=1))
    d = np.abs(f["qacc"] - want).max(axis=1) / scale
    s = np.abs(run["twin"]["qacc_warm"][:, 0] - want).max(axis=1) / scale
    print("\n%s newton cap %d, forward(): worst normalised |qacc - oracle| per cell (the oracle's own spread)" % (asset, cap))
    for c in dict.fromkeys(labels):
        sel = np.array(labels) == c
        print("  %-5s %.1e (%.1e)" % (c, d[sel].max(), s[sel].max()))
    assert (1000.0 * s <= BAR_QACC).all(), ("the oracle's own spread is no longer far below the bar", float(s.max()))
    one = Oracle(cm, 1)
    assert np.array_equal(f["contact_mask"], np.array([one.contact_mask(q)[0] for q in rows["qpos"]], dtype=np.uint32))
    bad =[(labels[e], e, float(d[e])) for e in range(n) if not d[e] <= BAR_QACC]
    assert not bad, bad
    conv = _row_run_converged(asset)
    assert (np.abs(want - conv).max(axis=1) > 1e-6).sum() >= n // 2            # the cap bites: these are not the minimisers
    assert tuple(got["qpos"].shape) == (n, 1, cm.nq) and (got["steps_done"] == 1).all()
    bad = _against_the_oracle("%s newton cap %d, one mj_step" % (asset, cap), run, got)
    assert not bad, bad


_CONV = {}


def _row_run_converged(asset):
    """qacc of the cells' first mj_step on the converged model (cap 100, tolerance 1e-8), from the same kind of warm start."""
    from oracle.oracle import Oracle
    if asset not in _CONV:
        cm = capped_model(asset, "newton", 100, 1e-8)
        qpos, qvel, ctrl, labels = cells(asset)
        warm = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
        _CONV[asset] = RO.OracleRollout(cm, 1).rollout(envs=np.zeros(len(labels), dtype=np.int32), qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm,
                                                       nstep=1, nsub=1, fields=["qacc_warm"])["qacc_warm"][:, 0]
    return _CONV[asset]


# ---------------------------------------------------------------------------------------------------- e. the create-time refusal
def test_a_negative_cap_is_still_refused_at_create():
    """solver_iterations = -1: kmanip_create returns -2 with "bad n_sub_steps / solver_iterations" and hands out no handle; a handle
    made before the refusal steps on as if nothing had happened (the bytes of a handle that never saw one)."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    from gym_kmanip_amd.model import compile_model
    good = compile_model("KManipSoloArm", auto_reset=True)
    bad = compile_model("KManipSoloArm", auto_reset=True, solver_iterations=-1)
    a = env_hip.KManipEnvHip(good, num_envs=8, seed=2)
    a.k_reset()
    act = a.sample_action().clone()
    a.step_flat(act)
    L = klib.load()
    h = C.c_void_p()
    rc = L.kmanip_create(C.byref(bad.desc), 8, 0, C.c_uint64(2), C.c_int64(0), C.byref(h))
    assert rc == -2 and not h.value and L.kmanip_last_error(None).decode() == "bad n_sub_steps / solver_iterations"
    with pytest.raises(klib.KManipError, match="bad n_sub_steps / solver_iterations"):
        env_hip.KManipEnvHip(bad, num_envs=8, seed=2)
    b = env_hip.KManipEnvHip(good, num_envs=8, seed=2)
    b.k_reset()
    b.step_flat(act)
    a.step_flat(act); b.step_flat(act)
    assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state()))
    assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done)
    a.k_close(); b.k_close()
