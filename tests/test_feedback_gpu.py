"""kmanip_feedback on the device (run with -m gpu on an MI355X): closed-loop rollouts under a per-step affine state feedback.

The rows are the regime cells of tests/tools/regime_states.py sent as CALLER rows to handles of 2 envs, one gain trajectory per cell,
3 steps.  The reference is tests/tools/feedback_oracle.py OracleFeedback under its fixed gains (computed once per argument set and
shared); the state bars are test_gpu_parity's -- qpos 1e-7, qvel 1e-5, reward 1e-6 -- contact mask, status and steps_done are compared
exactly, and the recorded ctrl is held to tests/test_feedback_cpu.py's BAR_U.  Everything that compares the kernel with itself or with
rollout() is bit for bit.  Worst figures measured on an MI355X: DESIGN.md section 29."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import feedback_oracle as FO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402
from test_rollout_gpu import _against_the_oracle, _dev_rows, _fresh, _host, _same, _stepwise_rows, _t, _torch  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
NSTEP = FO.NSTEP
SHARED = ("qpos", "qvel", "qacc_warm", "contact_mask", "reward", "status", "steps_done")

# (asset, solver, mode, nsub) of every parity run; nsub None = the model's 10 sub-steps.  The plain runs take the oracle's own step; a
# run with per-step forces or with per-env parameters on env 1 takes the restatement in NumPy and one sub-step (MuJoCo's own step).
# tests/test_feedback_cpu.py checks that these rows launch every k_feedback object the Makefile compiles.
PARITY_ROWS = ([(a, s, "plain", None) for a in ASSETS for s in ("newton", "pgs")]
               + [(a, s, m, 1) for a in ("solo_arm", "dual_arm") for s in ("newton", "pgs") for m in ("forced", "params", "params+forced")])
# the one-step check's constant c: |device u - (ctrl + K dx in torch float64)| <= c 2 nv 2^-53 (|ctrl| + sum_j |K_ij| |dx_j|).
# Measured WITHOUT the device: the same sums taken in ascending and in descending order of j in NumPy differ by at most C_ORDER of
# that unit over the rows of test_one_step_in_isolation (measured 0.128 on the single arm's 49 rows, 0.139 on the two arms' 74); the
# device gets a factor 10 over it.
C_ORDER = 0.15
C_ONE_STEP = 10.0 * C_ORDER


def _policy(pol):
    return {k: _t(v) for k, v in pol.items()}


# ---------------------------------------------------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("asset,solver,mode,nsub", PARITY_ROWS)
def test_parity_with_the_oracle_on_every_cell(asset, solver, mode, nsub):
    from test_feedback_cpu import BAR_U
    torch = _torch()
    run = FO.cell_runs(asset, solver, mode, nsub)
    cm, n = run["cm"], len(run["labels"])
    dev = _fresh(cm, 2)
    if "params" in mode:
        dev.set_env_params(**RO.env_params(cm)[0])
    before = dev.state_tensors()
    got = dev.rollout_feedback(**_dev_rows(run["rows"]), **_policy(run["policy"]), nsub=nsub, nstep=NSTEP)
    after = dev.state_tensors()
    assert all(torch.equal(before[k], after[k]) for k in before)
    dev.k_close()
    assert n > 2 and tuple(got["qpos"].shape) == (n, NSTEP, cm.nq) and tuple(got["ctrl"].shape) == (n, NSTEP, cm.nu)
    got = _host(got)
    ref = run["ref"]
    assert not ref["status"].any() and (got["contact_mask"] != 0).any()
    assert np.abs(ref["ctrl"] - run["rows"]["ctrl"][:, None]).max() > 0.5 and np.abs(ref["ctrl"]).max() <= 5.0          # (the gains matter)
    bad = _against_the_oracle("%s %s %s, %d rows on 2 envs, %d steps of %s sub-steps, fixed gains" % (asset, solver, mode, n, NSTEP, nsub or "the model's"), run, got)
    du = np.abs(got["ctrl"] - ref["ctrl"]).reshape(n, -1).max(axis=1)
    spread = float(np.abs(run["twin"]["ctrl"] - ref["ctrl"][run["twin_rows"]]).max())
    print("  recorded u: worst |device - oracle| %.2e in %s (the oracle's own spread %.1e; the bar %.0e)" % (du.max(), run["labels"][int(du.argmax())], spread, BAR_U))
    bad += [("ctrl", run["labels"][e], e, float(du[e]), BAR_U) for e in range(n) if not du[e] <= BAR_U]
    assert not bad, bad


# --------------------------------------------------------------------------------- bit for bit against rollout() and against itself
def _setup(asset, solver):
    """The cells with per-step ctrl and force rows (test_rollout_gpu._stepwise_rows), the fixed policy about them, on a 2-env handle."""
    cm, rows, labels = _stepwise_rows(asset, solver)
    K, qr, vr = FO.fixed_policy(cm, rows["qpos"], rows["qvel"], NSTEP)
    return cm, _dev_rows(rows), dict(gains=_t(K), qpos_ref=_t(qr), qvel_ref=_t(vr)), labels, _fresh(cm, 2)


@pytest.mark.parametrize("solver", ["newton", "pgs"])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_identities_with_rollout_and_resumed_calls(asset, solver):
    torch = _torch()
    cm, r, pol, labels, dev = _setup(asset, solver)
    n = len(labels)
    ol = dev.rollout(**r)
    assert not ol["status"].any()
    # (a) zero gains under perturbed references: rollout()'s bytes, and ctrl out is ctrl in
    zero = dev.rollout_feedback(**r, **dict(pol, gains=torch.zeros_like(pol["gains"])))
    assert _same(ol, {k: zero[k] for k in SHARED}) == [] and torch.equal(zero["ctrl"], r["ctrl"])
    # (b) the fixed gains with the references on the open-loop trajectory -- the state BEFORE step t: the row, then record t - 1:
    # every dx is exactly zero (an off-by-one index or a contracted quaternion product would not give zeros)
    qr = torch.cat([r["qpos"][:, None], ol["qpos"][:, :-1]], dim=1).contiguous()
    vr = torch.cat([r["qvel"][:, None], ol["qvel"][:, :-1]], dim=1).contiguous()
    assert bool(pol["gains"].ne(0).all()) and bool(torch.isfinite(pol["gains"]).all())
    on = dev.rollout_feedback(**r, gains=pol["gains"], qpos_ref=qr, qvel_ref=vr)
    assert _same(ol, {k: on[k] for k in SHARED}) == [] and torch.equal(on["ctrl"], r["ctrl"])
    off = dev.rollout_feedback(**r, gains=pol["gains"], qpos_ref=ol["qpos"], qvel_ref=ol["qvel"])          # (record t for step t: not the identity)
    assert not torch.equal(off["ctrl"], r["ctrl"])
    # (c) three steps are three resumed calls of one, fed qpos / qvel / qacc_warm and the slices of every per-step tensor
    whole = dev.rollout_feedback(**r, **pol)
    assert not whole["status"].any() and bool((whole["steps_done"] == NSTEP).all()) and float((whole["ctrl"] - r["ctrl"]).abs().max()) > 0.5
    q, v, w = r["qpos"], r["qvel"], r["warm"]
    for t in range(NSTEP):
        one = dev.rollout_feedback(envs=r["envs"], qpos=q, qvel=v, warm=w, ctrl=r["ctrl"][:, t].contiguous(), qfrc_applied=r["qfrc_applied"][:, t].contiguous(),
                                   nstep=1, **{k: x[:, t:t + 1].contiguous() for k, x in pol.items()})
        for k in ("qpos", "qvel", "qacc_warm", "contact_mask", "reward", "ctrl"):
            assert torch.equal(one[k][:, 0], whole[k][:, t]), (t, k)
        assert not one["status"].any() and bool((one["steps_done"] == 1).all())
        q, v, w = (one[k][:, 0].contiguous() for k in ("qpos", "qvel", "qacc_warm"))
    # (d) held gains and references are the same entry repeated per step; the transposed tensor skips the copy
    held = dev.rollout_feedback(**r, **{k: x[:, 0].contiguous() for k, x in pol.items()})
    rep = dev.rollout_feedback(**r, **{k: x[:, :1].repeat(1, NSTEP, *([1] * (x.dim() - 2))).contiguous() for k, x in pol.items()})
    assert _same(held, rep) == [] and not torch.equal(held["ctrl"], whole["ctrl"])
    tr = dev.rollout_feedback(**r, gains_t=pol["gains"].transpose(-1, -2).contiguous(), qpos_ref=pol["qpos_ref"], qvel_ref=pol["qvel_ref"])
    assert _same(whole, tr) == []
    # (e) rows that share a trajectory through gain_index against private copies of it
    gi = (torch.arange(n, device="cuda") // 3 * 3).to(torch.int32)
    shared = dev.rollout_feedback(**r, **pol, gain_index=gi)
    private = dev.rollout_feedback(**r, **{k: x[gi.long()].contiguous() for k, x in pol.items()})
    assert _same(shared, private) == [] and not torch.equal(shared["ctrl"], whole["ctrl"])
    # without mask and reward the kernel skips its trailing pass: the states and the ctrl are the same bytes
    lean = dev.rollout_feedback(fields=("qpos", "qvel", "qacc_warm", "ctrl", "status", "steps_done"), **r, **pol)
    assert sorted(lean) == ["ctrl", "qacc_warm", "qpos", "qvel", "status", "steps_done"] and _same(lean, {k: whole[k] for k in lean}) == []
    dev.k_close()


@pytest.mark.parametrize("solver", ["newton", "pgs"])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_rows_do_not_see_each_other(asset, solver):
    """The same rows (a) reversed, their trajectories named through gain_index, (b) each alone with n = 1, (c) on a handle of 5 envs."""
    torch = _torch()
    cm, r, pol, labels, dev = _setup(asset, solver)
    n = len(labels)
    ref = dev.rollout_feedback(**r, **pol)
    assert not ref["status"].any()
    rev = torch.arange(n - 1, -1, -1, device="cuda")
    assert _same(ref, dev.rollout_feedback(**{k: v[rev].contiguous() for k, v in r.items()}, **pol, gain_index=rev.to(torch.int32)), rows_f=rev) == []
    for e in range(n):
        one = dev.rollout_feedback(**{k: v[e:e + 1].contiguous() for k, v in r.items()}, **{k: v[e:e + 1].contiguous() for k, v in pol.items()})
        assert _same(ref, one, rows_f=slice(e, e + 1)) == [], (labels[e], e)
    five = _fresh(cm, 5, seed=3)
    assert _same(ref, five.rollout_feedback(**r, **pol)) == []
    dev.k_close(); five.k_close()


# --------------------------------------------------------------------------------------------------------------- one step in isolation
def _one_step_rows(asset):
    """The cells, the fixed policy's step 0, and two more rows: the first cell with its reference's cube turned by pi - 1e-3 about a
    skew axis, and by 1e-9 (the small-angle branch of the log map)."""
    import torch
    from gym_kmanip_amd.derivatives import tangent_perturb
    cm = R.model(asset)
    qpos, qvel, ctrl, labels = R.cells(asset)
    K, qr, vr = FO.fixed_policy(cm, qpos, qvel, 1)
    q0 = torch.from_numpy(qpos[:1].copy())
    far = tangent_perturb(cm, q0, cm.nlink + 4, np.pi - 1e-3).numpy()
    near = tangent_perturb(cm, q0, cm.nlink + 5, 1e-9).numpy()
    twice = lambda x: np.ascontiguousarray(np.concatenate([x, x[:1], x[:1]]))
    return (cm, dict(qpos=twice(qpos), qvel=twice(qvel), ctrl=twice(ctrl)), twice(K), np.ascontiguousarray(np.concatenate([qr, far[:, None], near[:, None]])),
            twice(vr))


def _order_gap(K, dx, ctrl):
    """max over rows and actuators of |ascending - descending| / (2 nv 2^-53 (|ctrl| + sum |K| |dx|)) and that unit [n, nu]."""
    nx = dx.shape[1]
    fwd, bwd = np.zeros(ctrl.shape), np.zeros(ctrl.shape)
    for j in range(nx):
        fwd = fwd + K[:, :, j] * dx[:, None, j]
        bwd = bwd + K[:, :, nx - 1 - j] * dx[:, None, nx - 1 - j]
    unit = nx * 2.0 ** -53 * (np.abs(ctrl) + (np.abs(K) * np.abs(dx)[:, None, :]).sum(axis=2))
    return float((np.abs((ctrl + fwd) - (ctrl + bwd)) / unit).max()), unit


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_one_step_in_isolation(asset):
    """ctrl[:, 0] of a one-step launch against ctrl + K dx with dx from derivatives.tangent_diff and torch float64 on the device, held
    to C_ONE_STEP 2 nv 2^-53 (|ctrl| + sum_j |K_ij| |dx_j|): the rounding of 2 nv + 1 operations at the size of the terms.  C_ORDER is
    re-measured here in NumPy (ascending against descending j) and must stay below the committed value."""
    torch = _torch()
    from gym_kmanip_amd.derivatives import tangent_diff
    cm, rows, K, qr, vr = _one_step_rows(asset)
    n = len(rows["qpos"])
    r = {k: _t(v) for k, v in rows.items()}
    r["envs"] = _t((np.arange(n) % 2).astype(np.int32))
    Kd, qrd, vrd = _t(K), _t(qr), _t(vr)
    dev = _fresh(cm, 2)
    got = dev.rollout_feedback(**r, gains=Kd, qpos_ref=qrd, qvel_ref=vrd, nstep=1, nsub=1, fields=("ctrl", "status"))
    dev.k_close()
    assert not got["status"].any()
    dx = torch.cat([tangent_diff(cm, r["qpos"], qrd[:, 0]), r["qvel"] - vrd[:, 0]], dim=1)
    ang = dx[:, cm.nlink + 3:cm.nlink + 6].norm(dim=1)
    assert abs(float(ang[n - 2]) - (np.pi - 1e-3)) < 1e-9 and abs(float(ang[n - 1]) - 1e-9) < 1e-15
    want = r["ctrl"] + (Kd[:, 0] * dx[:, None, :]).sum(dim=2)
    c_np, unit = _order_gap(K[:, 0], dx.cpu().numpy(), rows["ctrl"])
    gap = (got["ctrl"][:, 0] - want).abs().cpu().numpy() / unit
    e = int(gap.max(axis=1).argmax())
    print("\n%s: one step, %d rows: worst |device u - torch| = %.3f units of 2 nv 2^-53 (|ctrl| + sum |K| |dx|) in row %d (the two rotated rows: %.3f, %.3f); "
          "NumPy ascending vs descending %.3f; c = %.2f" % (asset, n, gap.max(), e, gap[n - 2].max(), gap[n - 1].max(), c_np, C_ONE_STEP))
    assert c_np <= C_ORDER, c_np
    assert gap.max() <= C_ONE_STEP, (e, float(gap.max()))
    assert float((got["ctrl"][:, 0] - r["ctrl"]).abs().max()) > 0.01


# ---------------------------------------------------------------------------------------------------------------------------- status
def test_bad_rows_get_their_status_and_zeros_and_harm_nobody():
    torch = _torch()
    cm, r, pol, labels, dev = _setup("solo_arm", "newton")
    n = len(labels)
    clean = dev.rollout_feedback(**r, **pol)
    assert not clean["status"].any() and dev.state_index_errors() == 0

    def check(g, e, status, done):
        assert g["status"][e] == status and int(g["status"].ne(0).sum()) == 1, (e, status, g["status"])
        assert int(g["steps_done"][e]) == done and int(g["steps_done"].ne(NSTEP).sum()) == 1
        for key in ("qpos", "qvel", "qacc_warm", "contact_mask", "reward", "ctrl"):
            assert not g[key][e, done:].any(), key                                   # zeros from the step the row stopped at
            assert torch.equal(g[key][e, :done], clean[key][e, :done]), key          # the records before it intact
        keep = torch.arange(n, device="cuda") != e
        assert _same(clean, g, rows_f=keep, rows_g=keep) == []
    e = 5
    # gain indices outside 0 .. ng-1 in the middle of the rows: status 2, never an address
    for idx in (2 * n, -1, 2 ** 31 - 1, -2 ** 31):
        gi = np.arange(n, dtype=np.int64)
        gi[e] = idx
        check(dev.rollout_feedback(**r, **pol, gain_index=_t(gi, np.int32)), e, 2, 0)
    assert dev.state_index_errors() == 0
    # a non-finite gain or reference entry at step t: status 1, t steps recorded; the same entry changes nothing while no row
    # names its trajectory (row e follows its neighbour's)
    gi = torch.arange(n, device="cuda", dtype=torch.int32)
    gi[e] = e + 1
    elsewhere = dev.rollout_feedback(**r, **pol, gain_index=gi)
    for name, at in (("gains", (3, 7)), ("qpos_ref", (cm.nq - 2,)), ("qpos_ref", (1,)), ("qvel_ref", (cm.nv - 1,))):
        for t in range(NSTEP):
            for value in (float("nan"), float("inf")):
                bad = dict(pol)
                bad[name] = pol[name].clone()
                bad[name][(e, t) + at] = value
                check(dev.rollout_feedback(**r, **bad), e, 1, t)
                assert _same(elsewhere, dev.rollout_feedback(**r, **bad, gain_index=gi)) == []
    # without the force rows (the default build) as well
    plain = {k: v for k, v in r.items() if k != "qfrc_applied"}
    clean = dev.rollout_feedback(**plain, **pol)
    bad = dict(pol, gains=pol["gains"].clone())
    bad["gains"][e, 2, 0, 0] = float("nan")
    check(dev.rollout_feedback(**plain, **bad), e, 1, 2)
    dev.k_close()


def test_refusals_launch_nothing_and_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd.lib import KFeedbackDev, KFeedbackIn, KManipError
    dev = _fresh(R.model("solo_arm"), 4)
    cm = dev.cm
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    st = dev.state_tensors()
    pol = dict(gains=z(4, 2, cm.nu, 2 * cm.nv), qpos_ref=st["qpos"][:, None].repeat(1, 2, 1), qvel_ref=z(4, 2, cm.nv))
    good = dev.rollout_feedback(**pol)
    assert _same(dev.rollout(nstep=2), {k: good[k] for k in SHARED}) == []
    with pytest.raises(KManipError, match="disagree"):
        dev.rollout_feedback(**pol, nstep=3)
    with pytest.raises(KManipError, match="one of them"):
        dev.rollout_feedback(qpos_ref=pol["qpos_ref"], qvel_ref=pol["qvel_ref"])
    with pytest.raises(KManipError, match="gain trajectories"):
        dev.rollout_feedback(**{k: v[:3].contiguous() for k, v in pol.items()})
    for kw in (dict(pol, gains=z(4, 2, cm.nu, 2 * cm.nv, dtype=torch.float32)), dict(pol, gains=z(4, 2, 2 * cm.nv, cm.nu)), dict(pol, qpos_ref=z(4, 2, cm.nv)),
               dict(pol, qvel_ref=z(4, cm.nv)), dict(pol, qvel_ref=None), dict(pol, gain_index=[0, 1, 2]), dict(pol, gains=z(4, 2, cm.nu, 2 * cm.nv, device="cpu")),
               dict(pol, out={"ctrl": z(4, 2, cm.nu + 1)})):
        with pytest.raises(KManipError):
            dev.rollout_feedback(**kw)
    # the C ABI's own refusals: nonzero, last_error set, nothing launched -- the outputs keep their sentinel
    L = dev.L
    sent = dict(qpos=torch.full((4, 2, cm.nq), 77.0, dtype=torch.float64, device="cuda"), ctrl=torch.full((4, 2, cm.nu), 77.0, dtype=torch.float64, device="cuda"),
                status=torch.full((4,), 77, dtype=torch.uint8, device="cuda"), steps_done=torch.full((4,), 77, dtype=torch.int32, device="cuda"))
    fo = KFeedbackDev()
    for k, v in sent.items():
        setattr(fo, k, v.data_ptr())
    gt = pol["gains"].transpose(-1, -2).contiguous()

    def fin(**kw):
        fi = KFeedbackIn()
        fi.qpos_ref, fi.qvel_ref, fi.gain_t, fi.ng, fi.gain_per_step = pol["qpos_ref"].data_ptr(), pol["qvel_ref"].data_ptr(), gt.data_ptr(), 4, 1
        for k, v in kw.items():
            setattr(fi, k, v)
        return fi
    ok = fin()
    refused = ((None, ok, 4, 2, 0, fo, b""), (dev.h, None, 4, 2, 0, fo, b"kmanip_feedback: the KFeedbackIn pointer is NULL"), (dev.h, ok, 4, 2, 0, None, b"kmanip_feedback: the KFeedbackDev pointer is NULL"),
               (dev.h, ok, -1, 2, 0, fo, b"n is negative"), (dev.h, ok, 4, -1, 0, fo, b"kmanip_feedback: nstep is negative"), (dev.h, ok, 4, 2, -1, fo, b"kmanip_feedback: nsub is negative"),
               (dev.h, ok, 5, 2, 0, fo, b"more rows than envs"), (dev.h, fin(ctrl_per_step=1), 4, 2, 0, fo, b"kmanip_feedback: ctrl_per_step is set and KFeedbackIn::ctrl is NULL"),
               (dev.h, fin(frc_per_step=1), 4, 2, 0, fo, b"kmanip_feedback: frc_per_step is set and KFeedbackIn::qfrc_applied is NULL"), (dev.h, fin(qpos_ref=None), 4, 2, 0, fo, b"qpos_ref is NULL"),
               (dev.h, fin(qvel_ref=None), 4, 2, 0, fo, b"qvel_ref is NULL"), (dev.h, fin(gain_t=None), 4, 2, 0, fo, b"gain_t is NULL"),
               (dev.h, fin(ng=0), 4, 2, 0, fo, b"ng is not positive"), (dev.h, fin(ng=-3), 4, 2, 0, fo, b"ng is not positive"),
               (dev.h, fin(ng=3), 4, 2, 0, fo, b"gain trajectories"))
    for h, i, n, ns, nsub, o, msg in refused:
        rc = L.kmanip_feedback(h, None if i is None else C.byref(i), n, ns, nsub, None if o is None else C.byref(o), None)
        err = L.kmanip_last_error(h)
        # (a message spelt out in full is the whole text: the NULL struct pointers and the refusals the two stepping entries share)
        assert rc != 0 and (err == msg if msg.startswith(b"kmanip_") else msg in err), (n, ns, nsub, msg, err)
    for n, ns in ((0, 2), (4, 0)):                                               # succeed and do nothing
        assert L.kmanip_feedback(dev.h, C.byref(ok), n, ns, 0, C.byref(fo), None) == 0
    assert L.kmanip_feedback(dev.h, C.byref(ok), 4, 2, 0, C.byref(KFeedbackDev()), None) == 0          # every output NULL
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in sent.values())
    assert L.kmanip_feedback(dev.h, C.byref(ok), 4, 2, 0, C.byref(fo), None) == 0
    assert torch.equal(sent["qpos"], good["qpos"]) and torch.equal(sent["ctrl"], good["ctrl"]) and not sent["status"].any() and bool((sent["steps_done"] == 2).all())
    dev.step_flat(z(4, cm.act_dim, dtype=torch.float32))
    assert not dev.done.cpu().numpy().any()
    dev.k_close()


# ------------------------------------------------------------------------------------------------------------------ handle read-only
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """Two identical handles holding every cell, three steps; one calls rollout_feedback -- stored rows, overriding rows, more rows
    than envs with shared trajectories, with a force -- before each.  State, diagnostics and sample_action before and after equal;
    the next step_flat gives the bytes of the twin that never made the call."""
    torch = _torch()
    from test_forces_gpu import _cells, _device
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    n = len(labels)
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    pol = _policy(dict(zip(("gains", "qpos_ref", "qvel_ref"), FO.fixed_policy(cm, qpos, qvel, 2))))
    tau = _t(RO.step_forces(cm, n, 2))
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)
    for k in range(3):
        before, diag, sample = a.state_tensors(), a.get_diag(), a.sample_action().clone()
        a.rollout_feedback(**pol)
        a.rollout_feedback(qpos=_t(qpos), qvel=_t(qvel), ctrl=_t(ctrl), warm=_t(warm), nsub=3, **pol)
        a.rollout_feedback(envs=np.arange(2 * n)[::-1] % n, gain_index=np.arange(2 * n) % n, qfrc_applied=torch.cat([tau, tau]), nsub=2, **pol)
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


# ------------------------------------------------------------------------------------------------------------------------------ iLQR
def test_ilqr_on_the_device_and_the_example(capsys):
    """KManipSoloArmQPos, 4 envs, horizon 4, 2 iterations, 3 alphas: the accepted cost never increases, every env's is lower after the
    first iteration, and the line search is one rollout_feedback launch of 12 rows.  The example runs under the same flags."""
    import math
    from gym_kmanip_amd.examples import ilqr_reach
    out = ilqr_reach.main(["--num-envs", "4", "--horizon", "4", "--iters", "2", "--alphas", "1.0", "0.5", "0.25"])
    print(capsys.readouterr().out)
    cost = np.asarray(out["cost_per_env"])
    assert cost.shape == (3, 4) and np.isfinite(cost).all()
    assert (np.diff(cost, axis=0) <= 0).all() and (cost[1] < cost[0]).all()
    assert out["rows_per_line_search"] == 12 and out["feedback_launches"] == 2 and len(out["cost"]) == 3 and all(math.isfinite(c) for c in out["cost"])
