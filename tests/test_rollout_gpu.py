"""kmanip_rollout and transition_fd on the device (run with -m gpu on an MI355X).

The rows are the regime cells of tests/tools/regime_states.py (47 for the single arm, 72 for the two-arm models) sent as CALLER rows
to handles of 2 envs (envs = arange(n) % 2): more rows than envs, not a multiple of the 4 / 2 rows a wave holds; 3 steps unless a test
says otherwise.  The reference is tests/tools/rollout_oracle.py (computed once per argument set and shared); the bars are
test_gpu_parity's -- qpos 1e-7, qvel 1e-5, reward 1e-6 -- and contact mask, status and steps_done are compared exactly.  Everything
that compares the kernel with itself (resuming, row order, neighbours, the handle's size) is bit for bit.  Worst figures measured
on an MI355X: DESIGN.md section 27."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402
from test_forces_cpu import BAR_QACC  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_R, TOL_V  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
BARS = {"qpos": TOL_Q, "qvel": TOL_V, "reward": TOL_R}
EXACT = ("contact_mask", "status", "steps_done")
NSTEP = RO.NSTEP

# (asset, solver, mode, nsub) of every parity run; nsub None = the model's 10 sub-steps.  The plain runs take the oracle's own step;
# a run with a force or with per-env parameters takes the restatement in NumPy, 7 ms a sub-step, and is given fewer sub-steps -- 3
# under the per-step test forces of every asset, 1 (MuJoCo's own step) where the row is there for the object it launches.
# tests/test_rollout_cpu.py checks that these rows and IDENTITY_ROWS launch every k_rollout object the Makefile compiles.
PARITY_ROWS = ([(a, s, "plain", None) for a in ASSETS for s in ("newton", "pgs")]
               + [(a, "newton", "forced", 3) for a in ASSETS]
               + [(a, "pgs", "forced", 1) for a in ("solo_arm", "dual_arm")]
               + [(a, s, m, 1) for a in ("solo_arm", "dual_arm") for s in ("newton", "pgs") for m in ("params", "params+forced")])
# (env id, solver) of the step identity: the QPos ids, whose actions bypass the IK -- nothing teleports
IDENTITY_ROWS = [(e, s) for e in ("KManipSoloArmQPos", "KManipDualArmQPos") for s in ("newton", "pgs")]
# rollout() from the state before a step_flat, with the ctrl the step stored, against the state after it: qpos, qvel, qacc_warm,
# contact mask and reward were equal byte for byte in the first measurement on an MI355X (every row of IDENTITY_ROWS, single steps
# and three steps in one call), so equality is what is asserted
IDENTITY_BYTES_EQUAL = True


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _t(x, dtype=None):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _fresh(cm, n, seed=0):
    from gym_kmanip_amd import env_hip
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=seed)
    dev.k_reset()
    return dev


def _host(f):
    out = {k: v.cpu().numpy() for k, v in f.items()}
    if "contact_mask" in out:
        out["contact_mask"] = out["contact_mask"].view(np.uint32)
    return out


def _dev_rows(rows):
    """rollout()'s keyword arguments as device tensors."""
    return {k: _t(v) for k, v in rows.items()}


def _same(f, g, rows_f=None, rows_g=None):
    """Names of the fields whose rows differ in any bit."""
    torch = _torch()
    bad = []
    for k in f:
        a = f[k] if rows_f is None else f[k][rows_f]
        b = g[k] if rows_g is None else g[k][rows_g]
        if not torch.equal(a, b):
            bad.append(k)
    return bad


def _cellwise(d, labels):
    out = {}
    for c, v in zip(labels, d):
        out[c] = max(out.get(c, 0.0), float(v))
    return out


def _against_the_oracle(tag, run, got):
    """Every row and step of a rollout() result (host arrays) against the shared reference run: mask, status and steps_done exactly,
    qpos / qvel / reward under the bars; prints the worst difference per cell next to the reference's own spread in the cell."""
    ref, labels = run["ref"], run["labels"]
    n = len(labels)
    bad = []
    for k in EXACT:
        same = (got[k].reshape(n, -1) == np.asarray(ref[k]).view(got[k].dtype).reshape(n, -1)).all(axis=1)
        bad += [(k, labels[e], e) for e in np.where(~same)[0]]
    tl = [labels[e] for e in run["twin_rows"]]
    print("\n%s: worst |device - oracle| per cell over all steps (the oracle's own spread under a 1e-15 relative change of qvel)" % tag)
    worst, spread = {}, {}
    for k, bar in BARS.items():
        d = np.abs(got[k] - ref[k]).reshape(n, -1).max(axis=1)
        worst[k] = _cellwise(d, labels)
        spread[k] = _cellwise(np.abs(run["twin"][k] - ref[k][run["twin_rows"]]).reshape(len(tl), -1).max(axis=1), tl)
        bad += [(k, labels[e], e, float(d[e]), bar) for e in range(n) if not d[e] < bar]
    for c in dict.fromkeys(labels):
        print("  %-5s %s" % (c, "  ".join("%s %.1e (%s)" % (k, worst[k][c], "%.1e" % spread[k][c] if c in spread[k] else "-") for k in BARS)))
    return bad


def _rollout_cells(run, mode, **kw):
    """The device's rollout of a cell_runs entry on a fresh handle of 2 envs (with env_params where the mode has parameters)."""
    cm = run["cm"]
    dev = _fresh(cm, 2)
    if "params" in mode:
        dev.set_env_params(**RO.env_params(cm)[0])
    before = dev.state_tensors()
    got = dev.rollout(**_dev_rows(run["rows"]), **kw)
    after = dev.state_tensors()
    assert all(_torch().equal(before[k], after[k]) for k in before)
    dev.k_close()
    return got


# ---------------------------------------------------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("asset,solver,mode,nsub", PARITY_ROWS)
def test_parity_with_the_oracle_on_every_cell(asset, solver, mode, nsub):
    run = RO.cell_runs(asset, solver, mode, nsub)
    n = len(run["labels"])
    got = _rollout_cells(run, mode, nsub=nsub, nstep=NSTEP)
    assert n > 2 and tuple(got["qpos"].shape) == (n, NSTEP, run["cm"].nq) and tuple(got["reward"].shape) == (n, NSTEP)
    got = _host(got)
    assert not run["ref"]["status"].any() and (got["contact_mask"] != 0).any()
    if "forced" in mode:
        assert run["rows"]["qfrc_applied"].shape == (n, NSTEP, run["cm"].nv) and not np.array_equal(got["qvel"][:, 0], got["qvel"][:, 1])
    bad = _against_the_oracle("%s %s %s, %d rows on 2 envs, %d steps of %s sub-steps" % (asset, solver, mode, n, NSTEP, nsub or "the model's"), run, got)
    assert not bad, bad


@pytest.mark.parametrize("solver", ["newton", "pgs"])
@pytest.mark.parametrize("asset", ASSETS)
def test_a_single_mj_step_on_every_cell(asset, solver):
    """nsub = 1, nstep = 1: the smallest shape, MuJoCo's own granularity.  Same bars."""
    run = RO.cell_runs(asset, solver, "plain", 1, 1)
    got = _host(_rollout_cells(run, "plain", nsub=1, nstep=1))
    assert tuple(got["qpos"].shape) == (len(run["labels"]), 1, run["cm"].nq) and (got["steps_done"] == 1).all()
    bad = _against_the_oracle("%s %s, one mj_step" % (asset, solver), run, got)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ bit-exact with itself
def _stepwise_rows(asset, solver):
    """The cells with a ctrl and a force row of their own for every step: (cm, rows, labels)."""
    run = RO.cell_runs(asset, solver)
    cm, rows = run["cm"], dict(run["rows"])
    n = len(run["labels"])
    rows["ctrl"] = np.ascontiguousarray(rows["ctrl"][:, None, :] + 0.01 * np.arange(NSTEP)[None, :, None] * np.cos(np.arange(n * cm.nu).reshape(n, 1, cm.nu)))
    rows["qfrc_applied"] = RO.step_forces(cm, n)
    return cm, rows, run["labels"]


@pytest.mark.parametrize("solver", ["newton", "pgs"])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_three_steps_are_three_resumed_calls_of_one(asset, solver):
    """rollout(nstep = 3) against three rollout(nstep = 1) calls, each fed the previous call's qpos, qvel and qacc_warm and the
    matching ctrl / force rows: every byte of every output equal.  The same kernel on both sides, so no bar applies; this is what
    pins qacc_warm."""
    torch = _torch()
    cm, rows, labels = _stepwise_rows(asset, solver)
    r = _dev_rows(rows)
    dev = _fresh(cm, 2)
    whole = dev.rollout(**r)
    assert not whole["status"].any() and bool((whole["steps_done"] == NSTEP).all())
    q, v, w = r["qpos"], r["qvel"], r["warm"]
    for t in range(NSTEP):
        one = dev.rollout(envs=r["envs"], qpos=q, qvel=v, warm=w, ctrl=r["ctrl"][:, t].contiguous(), qfrc_applied=r["qfrc_applied"][:, t].contiguous(),
                          nstep=1)
        for k in ("qpos", "qvel", "qacc_warm", "contact_mask", "reward"):
            assert torch.equal(one[k][:, 0], whole[k][:, t]), (t, k)
        assert not one["status"].any() and bool((one["steps_done"] == 1).all())
        q, v, w = (one[k][:, 0].contiguous() for k in ("qpos", "qvel", "qacc_warm"))
    # held rows are the per-step path with the same row every step
    held = dev.rollout(envs=r["envs"], qpos=r["qpos"], qvel=r["qvel"], warm=r["warm"], ctrl=r["ctrl"][:, 0].contiguous(),
                       qfrc_applied=r["qfrc_applied"][:, 0].contiguous(), nstep=NSTEP)
    rep = dev.rollout(envs=r["envs"], qpos=r["qpos"], qvel=r["qvel"], warm=r["warm"], ctrl=r["ctrl"][:, :1].repeat(1, NSTEP, 1).contiguous(),
                      qfrc_applied=r["qfrc_applied"][:, :1].repeat(1, NSTEP, 1).contiguous())
    assert _same(held, rep) == []
    # without mask and reward the kernel skips its trailing pass: the states are the same bytes
    lean = dev.rollout(fields=("qpos", "qvel", "qacc_warm", "status", "steps_done"), **r)
    assert sorted(lean) == ["qacc_warm", "qpos", "qvel", "status", "steps_done"] and _same(lean, {k: whole[k] for k in lean}) == []
    dev.k_close()


@pytest.mark.parametrize("solver", ["newton", "pgs"])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_rows_do_not_see_each_other(asset, solver):
    """The same rows (a) reversed, (b) each alone with n = 1, (c) on a handle of 5 envs: the same bytes per row."""
    torch = _torch()
    cm, rows, labels = _stepwise_rows(asset, solver)
    n = len(labels)
    r = _dev_rows(rows)
    dev = _fresh(cm, 2)
    ref = dev.rollout(**r)
    assert not ref["status"].any()
    rev = torch.arange(n - 1, -1, -1, device="cuda")
    assert _same(ref, dev.rollout(**{k: v[rev].contiguous() for k, v in r.items()}), rows_f=rev) == []
    for e in range(n):
        one = dev.rollout(**{k: v[e:e + 1].contiguous() for k, v in r.items()})
        assert _same(ref, one, rows_f=slice(e, e + 1)) == [], (labels[e], e)
    five = _fresh(cm, 5, seed=3)
    assert _same(ref, five.rollout(**r)) == []
    dev.k_close(); five.k_close()


# --------------------------------------------------------------------------------------------------------------- the step identity
@pytest.mark.parametrize("env_id,solver", IDENTITY_ROWS)
def test_a_rollout_from_the_state_before_a_step_is_the_step(env_id, solver):
    """On the QPos ids the actions bypass the IK, so nothing teleports: rollout() from the state before a step_flat, with the ctrl
    the step stored, nstep = 1 and the model's sub-steps, gives the stepped qpos, qvel, warm start, contact mask and reward; three
    consecutive steps are one nstep = 3 rollout with per-step ctrl.  37 envs, row r = env r (no index); no episode ends inside."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    dev = env_hip.make(env_id, num_envs=37, seed=5, auto_reset=False, solver=solver)
    dev.k_reset()
    for _ in range(2):
        dev.step_flat(dev.sample_action())
    start = dev.state_tensors()
    assert int(start["step"].max()) + NSTEP < dev.cm.desc.max_episode_steps
    before, stepped = start, []
    worst = {}
    for t in range(NSTEP):
        dev.step_flat(dev.sample_action())
        assert not dev.done.any()
        after = dev.state_tensors()
        want = dict(qpos=after["qpos"], qvel=after["qvel"], qacc_warm=after["warm"], contact_mask=_t(dev.get_diag()[0].view(np.int32)),
                    reward=dev.reward.clone())
        stepped.append((after["ctrl"], want))
        got = dev.rollout(qpos=before["qpos"], qvel=before["qvel"], warm=before["warm"], ctrl=after["ctrl"], nstep=1)
        assert not got["status"].any()
        _identity(got, 0, want, worst, (env_id, solver, "step %d" % t))
        before = after
    ctrl3 = torch.stack([c for c, _ in stepped], dim=1).contiguous()
    got = dev.rollout(qpos=start["qpos"], qvel=start["qvel"], warm=start["warm"], ctrl=ctrl3)
    assert tuple(got["qpos"].shape) == (37, NSTEP, dev.cm.nq) and bool((got["steps_done"] == NSTEP).all())
    for t in range(NSTEP):
        _identity(got, t, stepped[t][1], worst, (env_id, solver, "step %d of one call" % t))
    dev.k_close()
    print("\n%s %s: rollout() vs step_flat: %s" % (env_id, solver, "bytes equal" if not any(worst.values()) else
                                                     "largest differences relative to the state's scale %s" % "  ".join("%s %.1e" % kv for kv in worst.items())))


def _identity(got, t, want, worst, what):
    torch = _torch()
    assert torch.equal(got["contact_mask"][:, t], want["contact_mask"]), what
    for k in ("qpos", "qvel", "qacc_warm", "reward"):
        a, b = got[k][:, t], want[k]
        d = float(((a - b).abs() / b.abs().max().clamp(min=1.0)).max())
        worst[k] = max(worst.get(k, 0.0), d)
        assert d <= BAR_QACC, (what, k, d)
        if IDENTITY_BYTES_EQUAL:
            assert torch.equal(a, b), (what, k, d)


# ------------------------------------------------------------------------------------------------------------------ handle read-only
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """Two identical handles holding every cell, three steps; one calls rollout -- stored rows, overriding rows, more rows than
    envs, with and without a force -- before each.  State, diagnostics and sample_action before and after equal; the next
    step_flat gives the bytes of the twin that never called rollout."""
    torch = _torch()
    from test_forces_gpu import _cells, _device
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    n = len(labels)
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    tau = _t(RO.step_forces(cm, n))
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)
    for k in range(3):
        before, diag, sample = a.state_tensors(), a.get_diag(), a.sample_action().clone()
        a.rollout(nstep=2)
        a.rollout(qpos=_t(qpos), qvel=_t(qvel), ctrl=_t(ctrl), warm=_t(warm), nstep=2, nsub=3)
        a.rollout(envs=np.arange(2 * n)[::-1] % n, qvel=_t(np.concatenate([qvel, qvel])), qfrc_applied=torch.cat([tau, tau]), nsub=2)
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), k
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), k
        assert torch.equal(sample, a.sample_action()), k
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), k
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
        assert torch.equal(a.sim_time, b.sim_time)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_diag(), b.get_diag())), k
    a.k_close(); b.k_close()


# ---------------------------------------------------------------------------------------------------------------------------- status
def test_bad_rows_get_their_status_and_zeros_and_harm_nobody():
    torch = _torch()
    cm, rows, labels = _stepwise_rows("solo_arm", "newton")
    n = len(labels)
    r = _dev_rows(rows)
    dev = _fresh(cm, 2)
    assert dev.state_index_errors() == 0
    clean = dev.rollout(**r)
    assert not clean["status"].any()

    def check(g, e, status, done):
        assert g["status"][e] == status and int(g["status"].ne(0).sum()) == 1, (e, status, g["status"])
        assert int(g["steps_done"][e]) == done and int(g["steps_done"].ne(NSTEP).sum()) == 1
        for key in ("qpos", "qvel", "qacc_warm", "contact_mask", "reward"):
            assert not g[key][e, done:].any(), key                                   # zeros from the step the row stopped at
            assert torch.equal(g[key][e, :done], clean[key][e, :done]), key          # the records before it intact
        keep = torch.arange(n, device="cuda") != e
        assert _same(clean, g, rows_f=keep, rows_g=keep) == []
    e = 5
    # indices outside the handle, in the middle of the rows: status 2, never an address
    for idx in (2, -1, 2 ** 31 - 1, -2 ** 31):
        ie = rows["envs"].copy()
        ie[e] = idx
        check(dev.rollout(**dict(r, envs=_t(ie, np.int32))), e, 2, 0)
    assert dev.state_index_errors() == 0
    # a NaN in a given qpos, in a per-step ctrl at t = 1, in a per-step force at t = 2
    for name, at, done in (("qpos", (e, -1), 0), ("ctrl", (e, 1, 2), 1), ("qfrc_applied", (e, 2, 0), 2), ("qvel", (e, 3), 0), ("warm", (e, 0), 0),
                           ("ctrl", (e, 0, 0), 0), ("qfrc_applied", (e, 0, 4), 0)):
        for value in (float("nan"), float("inf")):
            bad = dict(r)
            bad[name] = r[name].clone()
            bad[name][at] = value
            check(dev.rollout(**bad), e, 1, done)
    # without the force rows (the default build) as well
    plain = {k: v for k, v in r.items() if k != "qfrc_applied"}
    clean = dev.rollout(**plain)
    bad = dict(plain, ctrl=plain["ctrl"].clone())
    bad["ctrl"][e, 2, 0] = float("nan")
    check(dev.rollout(**bad), e, 1, 2)
    # a stored non-finite value reaches the rows that use it, and only those
    q = dev.state_tensors()["qpos"]
    q[1, 0] = float("nan")
    dev.set_state_tensors(qpos=q)
    g = dev.rollout(envs=[0, 1, 1, 0], qvel=plain["qvel"][:4].contiguous(), nstep=2)
    assert g["status"].tolist() == [0, 1, 1, 0] and g["steps_done"].tolist() == [2, 0, 0, 2]
    assert not dev.rollout(envs=[0, 1, 1, 0], qpos=plain["qpos"][:4].contiguous())["status"].any()
    dev.k_close()


def test_refusals_launch_nothing_and_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd.lib import KManipError, KRolloutDev, KRolloutIn
    dev = _fresh(R.model("solo_arm"), 4)
    cm = dev.cm
    good = dev.rollout(nstep=2)
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    with pytest.raises(KManipError, match="more rows than envs"):
        dev.rollout(qvel=z(5, cm.nv))
    with pytest.raises(KManipError, match="negative"):
        dev.rollout(nsub=-1)
    with pytest.raises(KManipError, match="disagree"):
        dev.rollout(ctrl=z(4, 3, cm.nu), nstep=2)
    for kw in (dict(qpos=z(4, cm.nq, dtype=torch.float32)), dict(qvel=z(4, cm.nv + 1)), dict(ctrl=z(4, cm.nu, device="cpu")),
               dict(ctrl=z(4, 2, cm.nu + 1)), dict(ctrl=z(4, 2, cm.nu), qfrc_applied=z(4, 3, cm.nv)), dict(warm=z(4, 2, cm.nv)),
               dict(qfrc_applied=z(8, cm.nv)[::2]), dict(envs=[0, 1], qpos=z(3, cm.nq)), dict(qpos=np.zeros((4, cm.nq))),
               dict(out={"qpos": z(4, 2, cm.nq)}, nstep=1), dict(out={"status": z(4, dtype=torch.int32)})):
        with pytest.raises(KManipError):
            dev.rollout(**kw)
    with pytest.raises(ValueError):
        dev.rollout(fields=["nonsense"])
    # the C ABI's own refusals: nonzero, last_error set, nothing launched -- the outputs keep their sentinel
    L = dev.L
    sent = dict(qpos=torch.full((4, 2, cm.nq), 77.0, dtype=torch.float64, device="cuda"), status=torch.full((4,), 77, dtype=torch.uint8, device="cuda"),
                steps_done=torch.full((4,), 77, dtype=torch.int32, device="cuda"))
    ro = KRolloutDev()
    for k, v in sent.items():
        setattr(ro, k, v.data_ptr())
    ri = KRolloutIn()
    per_ctrl, per_frc = KRolloutIn(), KRolloutIn()
    per_ctrl.ctrl_per_step, per_frc.frc_per_step = 1, 1
    refused = ((None, ri, 4, 2, 0, ro, b""), (dev.h, None, 4, 2, 0, ro, b"kmanip_rollout: the KRolloutIn pointer is NULL"), (dev.h, ri, 4, 2, 0, None, b"kmanip_rollout: the KRolloutDev pointer is NULL"),
               (dev.h, ri, -1, 2, 0, ro, b"n is negative"), (dev.h, ri, 4, -1, 0, ro, b"kmanip_rollout: nstep is negative"), (dev.h, ri, 4, 2, -1, ro, b"kmanip_rollout: nsub is negative"),
               (dev.h, ri, 5, 2, 0, ro, b"more rows than envs"), (dev.h, per_ctrl, 4, 2, 0, ro, b"kmanip_rollout: ctrl_per_step is set and KRolloutIn::ctrl is NULL"), (dev.h, per_frc, 4, 2, 0, ro, b"kmanip_rollout: frc_per_step is set and KRolloutIn::qfrc_applied is NULL"))
    for h, i, n, ns, nsub, o, msg in refused:
        rc = L.kmanip_rollout(h, None if i is None else C.byref(i), n, ns, nsub, None if o is None else C.byref(o), None)
        err = L.kmanip_last_error(h)
        # (a message spelt out in full is the whole text: the NULL struct pointers and the refusals the two stepping entries share)
        assert rc != 0 and (err == msg if msg.startswith(b"kmanip_") else msg in err), (n, ns, nsub, msg, err)
    for n, ns in ((0, 2), (4, 0)):                                               # succeed and do nothing
        assert L.kmanip_rollout(dev.h, C.byref(ri), n, ns, 0, C.byref(ro), None) == 0
    assert L.kmanip_rollout(dev.h, C.byref(ri), 4, 2, 0, C.byref(KRolloutDev()), None) == 0          # every output NULL
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in sent.values())
    assert L.kmanip_rollout(dev.h, C.byref(ri), 4, 2, 0, C.byref(ro), None) == 0
    assert torch.equal(sent["qpos"], good["qpos"]) and not sent["status"].any() and bool((sent["steps_done"] == 2).all())
    empty = dev.rollout(envs=torch.zeros((0,), dtype=torch.int32, device="cuda"), nstep=2)
    assert tuple(empty["qpos"].shape) == (0, 2, cm.nq)
    assert _same(good, dev.rollout(nstep=2)) == []
    dev.step_flat(z(4, cm.act_dim, dtype=torch.float32))
    assert not dev.done.cpu().numpy().any()
    dev.k_close()


# ----------------------------------------------------------------------------------------------------------------------- derivatives
class _Recorder:
    """transition_fd's view of a handle -- .cm and .rollout -- that keeps the rows of every call."""

    def __init__(self, dev):
        self.dev, self.cm, self.calls = dev, dev.cm, []

    def rollout(self, **kw):
        self.calls.append({k: None if v is None else v.cpu().numpy() for k, v in kw.items() if k in ("envs", "qpos", "qvel", "ctrl", "warm", "qfrc_applied")})
        return self.dev.rollout(**kw)


@pytest.mark.parametrize("nsub", [1, None], ids=["mj_step", "control_step"])
@pytest.mark.parametrize("asset", ASSETS)
def test_transition_fd_against_the_oracles(asset, nsub):
    """transition_fd on the device against transition_fd over OracleRollout on six cells (rollout_oracle.FD_CELLS), the model
    compiled at FD_TOLERANCE, one mj_step and one control step: both sides are handed bit-equal perturbed rows, the contact masks
    of all perturbed rows are equal, and every block of A and B is within tests/test_rollout_cpu.py's BAR_FD -- 1000 x the
    reference's own spread, derived and re-asserted there -- of the reference's."""
    torch = _torch()
    from gym_kmanip_amd.derivatives import transition_fd
    from test_rollout_cpu import BAR_FD, SPREAD_FD
    cm, rows, ref_env, ref = RO.fd_reference(asset, nsub)
    n, nv = len(rows["qpos"]), cm.nv
    dev = _fresh(cm, 2)
    rec = _Recorder(dev)
    got = transition_fd(rec, nsub=nsub, **_dev_rows(rows))
    dev.k_close()
    assert len(rec.calls) == len(ref_env.calls) == 2 and len(rec.calls[1]["qpos"]) == 2 * (2 * nv + cm.nu) * n
    for mine, theirs in zip(rec.calls, ref_env.calls):
        for k in ("envs", "qpos", "qvel", "ctrl"):
            assert np.array_equal(mine[k], theirs[k]), k
        assert mine["qfrc_applied"] is None and theirs["qfrc_applied"] is None
    assert np.array_equal(rec.calls[0]["warm"], ref_env.calls[0]["warm"]) and np.array_equal(rec.calls[1]["warm"], ref_env.calls[1]["warm"])
    assert not got["status"].any() and not got["status_fd"].any() and not ref["status_fd"].any()
    assert torch.equal(got["contact_mask_fd"].cpu(), ref["contact_mask_fd"]) and torch.equal(got["contact_mask"].cpu(), ref["contact_mask"])
    dist = RO.fd_dist(RO.fd_blocks(ref, nv), RO.fd_blocks(got, nv))
    print("\n%s, nsub %s: worst normalised |device - oracle| per block (the reference's spread; the bar): %s"
          % (asset, nsub or "the model's", "  ".join("%s %.1e in %s (%.1e; %.0e)" % (k, v.max(), RO.FD_CELLS[asset][int(v.argmax())], SPREAD_FD[nsub][k], BAR_FD[nsub][k])
                                                     for k, v in dist.items())))
    bad = [(k, RO.FD_CELLS[asset][e], float(v[e]), BAR_FD[nsub][k]) for k, v in dist.items() for e in range(n) if not v[e] <= BAR_FD[nsub][k]]
    assert not bad, bad
    assert float(got["A"].abs().max()) > 1.0 and float(got["B"].abs().max()) > 1e-3


# --------------------------------------------------------------------------------------------------------------------------- example
def test_the_example_plans_in_ctrl_space_and_prints_a_pair(capsys):
    import math
    from gym_kmanip_amd.examples import ctrl_rollouts
    out = ctrl_rollouts.main(["--num-envs", "6", "--samples", "9", "--horizon", "4", "--iters", "2"])
    print(capsys.readouterr().out)
    nv, nu = 16, 10
    assert out["rows_per_launch"] == 54 and len(out["cost"]) == 2 and all(math.isfinite(c) for c in out["cost"])
    assert out["A_shape"] == [2 * nv, 2 * nv] and out["B_shape"] == [2 * nv, nu] and out["fd_status"] == 0
    assert math.isfinite(out["A_spectral_radius"]) and out["B_max"] > 0
