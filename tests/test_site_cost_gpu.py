"""kmanip_site_cost (KManipEnvHip.site_cost, ilqr.SiteCost(device=True)) on the device (run with -m gpu on an MI355X).

Over the input family of tests/tools/site_cost_reference.py -- the regime cells of the three assets, targets displaced from the site's
own pose, the nine weight patterns, both follow_cube values -- the kernel's cost, lx and lxx are compared with the np.longdouble
restatement and with ilqr.site_cost_rows (SiteCost(device=False)'s arithmetic) on the device, each output relative to the row's
largest entry, under tests/test_site_cost_cpu.BAR_SITE_COST.  Then what holds exactly, the status values, the refusals, the handle
left untouched, the planner with either cost path and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import regime_states as R  # noqa: E402
import site_cost_reference as SR  # noqa: E402
from test_kinematics_gpu import _cells, _device, _torch  # noqa: E402
from test_site_cost_cpu import BAR_SITE_COST, OUTPUTS, REACH_ASSERTED, REACH_MEASURED, worst_relative  # noqa: E402

pytestmark = pytest.mark.gpu

# (asset, mode) of the parity test: together they launch every sitekin object (tests/test_site_cost_cpu.py checks that)
LAUNCH_ROWS = [("solo_arm", "plain"), ("dual_arm", "plain"), ("torso", "plain"), ("solo_arm", "params"), ("dual_arm", "params")]


def _cuda(x):
    torch = _torch()
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _call(dev, fam, rows=None, envs=None, **kw):
    """site_cost over the family's rows (all, or `rows`) on a handle; every row names env 0 unless envs is given."""
    torch = _torch()
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    n = len(pick(fam["qpos"]))
    args = dict(envs=torch.zeros(n, dtype=torch.int32, device="cuda") if envs is None else envs, qpos=_cuda(pick(fam["qpos"])),
                target_quat=_cuda(pick(fam["target_quat"])), follow_cube=fam["follow"])
    args.update(kw)
    return dev.site_cost(_cuda(pick(fam["target_pos"])), _cuda(pick(fam["weight"])), **args)


def _small(cm, n=2):
    from gym_kmanip_amd import env_hip
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=1)
    dev.k_reset()
    return dev


@pytest.mark.parametrize("follow", [False, True])
@pytest.mark.parametrize("asset,mode", LAUNCH_ROWS)
def test_parity_with_the_longdouble_restatement_and_the_torch_definition(asset, mode, follow):
    """Worst figures measured on an MI355X: DESIGN.md section 40."""
    torch = _torch()
    from gym_kmanip_amd import ilqr
    fam = SR.family(asset, follow)
    cm = fam["cm"]
    n, nl, nv = len(fam["ref"]), cm.nlink, cm.nv
    dev = _small(cm)
    if mode == "params":
        dev.set_env_params(cube_mass=np.array([2.0, 3.0]) * cm.desc.cube_mass)
    r = _call(dev, fam)
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    t = ilqr.site_cost_rows(dev, idx, _cuda(fam["qpos"]), _cuda(fam["qvel"]), _cuda(fam["target_pos"]), _cuda(fam["target_quat"]),
                            _cuda(fam["weight"]), fam["follow"])
    dev.k_close()
    got = {k: v.cpu().numpy() for k, v in r.items()}
    ref_t = {k: v.cpu().numpy() for k, v in t.items()}
    assert not got["status"].any() and not ref_t["status"].any()
    w = worst_relative(got, fam)
    print("\n%s %s follow %d, device vs longdouble: %s" % (asset, mode, follow, "  ".join("%s %.1e (row %d)" % ((k,) + w[k]) for k in OUTPUTS)))
    wt = {k: max(SR.relative(got[k][e], ref_t[k][e]) for e in range(n)) for k in OUTPUTS}
    print("device vs SiteCost(device=False) on the device: %s" % "  ".join("%s %.1e" % kv for kv in wt.items()))
    assert all(v <= BAR_SITE_COST for v, _ in w.values()), w
    assert all(v <= BAR_SITE_COST for v in wt.values()), wt
    resid = np.stack([np.asarray(x["resid"], dtype=np.float64) for x in fam["ref"]])
    assert np.abs(got["resid"] - resid).max() <= BAR_SITE_COST * max(1.0, np.abs(resid).max())
    # ---- what holds exactly
    H, g = got["lxx"], got["lx"]
    assert np.array_equal(H, H.transpose(0, 2, 1))
    assert not g[:, nv:].any() and not H[:, nv:].any() and not H[:, :, nv:].any()
    assert not np.signbit(g[:, nv:]).any() and not np.signbit(H[:, nv:]).any() and not np.signbit(H[:, :nv, nv:]).any()      # +0.0
    assert not g[:, nl + 3:nv].any() and not H[:, nl + 3:nv].any()
    assert bool(g[:, nl:nl + 3].any()) == follow and bool(H[:, nl:nl + 3].any()) == follow
    assert np.abs(g[:, :nl]).max() > 1.0 and np.abs(H[:, :nl, :nl]).max() > 1.0


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_all_zero_weights_give_zeros_with_status_zero(asset):
    torch = _torch()
    fam = SR.family(asset, True)
    dev = _small(fam["cm"])
    r = _call(dev, dict(fam, weight=np.zeros_like(fam["weight"])))
    dev.k_close()
    assert not r["status"].any() and not r["cost"].any() and not r["lx"].any() and not r["lxx"].any()
    assert not torch.signbit(r["cost"]).any() and not torch.signbit(r["lx"]).any() and not torch.signbit(r["lxx"]).any()
    assert r["site_xpos"][:, 0].abs().min() > 0 and r["resid"][:, 0, :3].abs().max() > 0          # the geometry is still reported


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_a_row_alone_in_a_batch_and_permuted_and_a_single_field(asset):
    torch = _torch()
    fam = SR.family(asset, True)
    dev = _small(fam["cm"])
    n = len(fam["ref"])
    full = _call(dev, fam)
    perm = np.random.default_rng(2).permutation(n)
    shuffled = _call(dev, fam, rows=perm)
    for k in full:
        assert torch.equal(shuffled[k], full[k][torch.from_numpy(perm).cuda()]), k
    for r in (0, n // 2, n - 1):
        one = _call(dev, fam, rows=slice(r, r + 1))
        assert all(torch.equal(one[k], full[k][r:r + 1]) for k in full), r
    for name in full:
        only = _call(dev, fam, fields=[name])
        assert list(only) == [name] and torch.equal(only[name], full[name]), name
    mine = {"lxx": torch.full_like(full["lxx"], 3.0), "status": torch.full_like(full["status"], 7)}
    assert _call(dev, fam, out=mine) is mine and torch.equal(mine["lxx"], full["lxx"]) and not mine["status"].any()
    dev.k_close()


def test_the_absent_arm_contributes_nothing():
    """The solo arm: NaN targets and non-zero weights in the absent arm's slots change no bit and raise no status."""
    torch = _torch()
    fam = SR.family("solo_arm", False)
    dev = _small(fam["cm"])
    full = _call(dev, fam)
    tp, tq, w = fam["target_pos"].copy(), fam["target_quat"].copy(), fam["weight"].copy()
    tp[:, 1], tq[:, 1], w[:, 1] = np.nan, np.nan, 7.0
    noisy = dev.site_cost(_cuda(tp), _cuda(w), envs=torch.zeros(len(tp), dtype=torch.int32, device="cuda"), qpos=_cuda(fam["qpos"]),
                          target_quat=_cuda(tq))
    dev.k_close()
    assert not noisy["status"].any() and all(torch.equal(noisy[k], full[k]) for k in full)
    assert not full["resid"][:, 1].any() and not full["site_xpos"][:, 1].any()


def test_status_values_and_a_stored_nan_velocity():
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells("dual_arm")
    fam = SR.family("dual_arm", True)
    n = len(labels)
    vn = qvel.copy()
    vn[:, 3] = np.nan                                  # a stored NaN velocity does not enter
    dev = _device(cm, qpos, vn, ctrl, warm)
    tp, tq, w = _cuda(fam["target_pos"]), _cuda(fam["target_quat"]), _cuda(fam["weight"])
    clean = dev.site_cost(tp, w, target_quat=tq, follow_cube=True)           # every input the env's own: row r is env r
    other = _small(cm)
    given = _call(other, fam)
    other.k_close()
    assert not clean["status"].any() and all(torch.equal(clean[k], given[k]) for k in clean)
    # status 2 by index
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    idx[4], idx[7] = -1, n
    s2 = dev.site_cost(tp, w, envs=idx, target_quat=tq, follow_cube=True)
    bad = torch.zeros(n, dtype=torch.bool, device="cuda")
    bad[[4, 7]] = True
    assert s2["status"].tolist() == [2 if e in (4, 7) else 0 for e in range(n)]
    assert all(not s2[k][bad].any() for k in s2 if k != "status") and all(torch.equal(s2[k][~bad], clean[k][~bad]) for k in s2 if k != "status")
    # status 1: NaN qpos, NaN target, NaN weight of a present arm, a NaN quaternion where it is read
    qn = _cuda(qpos.copy()); qn[5, 1] = float("nan")
    tpn = tp.clone(); tpn[11, 1, 2] = float("nan")
    wn = w.clone(); wn[20, 0, 1] = float("nan")
    rot = int(np.flatnonzero(fam["weight"][:, 1, 1] != 0)[0])
    none = int(np.flatnonzero(fam["weight"][:, 1, 1] == 0)[0])
    tqn = tq.clone(); tqn[rot, 1, 0] = float("nan"); tqn[none, 1, 0] = float("nan")      # (the second is never read)
    s1 = dev.site_cost(tpn, wn, qpos=qn, target_quat=tqn, follow_cube=True)
    hit = sorted({5, 11, 20, rot})
    bad = torch.zeros(n, dtype=torch.bool, device="cuda")
    bad[hit] = True
    assert s1["status"].tolist() == [1 if e in hit else 0 for e in range(n)]
    assert all(not s1[k][bad].any() for k in s1 if k != "status") and all(torch.equal(s1[k][~bad], clean[k][~bad]) for k in s1 if k != "status")
    # no target_quat: every rotation weight counts as 0
    norot = dev.site_cost(tp, w, follow_cube=True)
    w0 = w.clone(); w0[:, :, 1] = 0.0
    same = dev.site_cost(tp, w0, target_quat=tq, follow_cube=True)
    assert all(torch.equal(norot[k], same[k]) for k in norot) and not norot["resid"][:, :, 3:].any()
    dev.k_close()


def test_refusals_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd.lib import KSiteCostDev, KSiteCostIn
    dev = _small(R.model("solo_arm"), 4)
    call, err = dev.L.kmanip_site_cost, dev.L.kmanip_last_error
    tp = torch.zeros((8, 2, 3), dtype=torch.float64, device="cuda")
    w = torch.ones((8, 2, 2), dtype=torch.float64, device="cuda")
    status = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    si, sd = KSiteCostIn(), KSiteCostDev()
    si.target_pos, si.weight, sd.status = tp.data_ptr(), w.data_ptr(), status.data_ptr()
    assert call(None, C.byref(si), 4, C.byref(sd), None) != 0 and b"kmanip_site_cost: null handle" in err(None)
    assert call(dev.h, None, 4, C.byref(sd), None) != 0 and b"KSiteCostIn pointer is NULL" in err(dev.h)
    assert call(dev.h, C.byref(si), 4, None, None) != 0 and b"KSiteCostDev pointer is NULL" in err(dev.h)
    assert call(dev.h, C.byref(si), -1, C.byref(sd), None) != 0 and b"n is negative" in err(dev.h)
    assert call(dev.h, C.byref(si), 5, C.byref(sd), None) != 0 and b"more rows than envs" in err(dev.h)
    si.target_pos = None
    assert call(dev.h, C.byref(si), 4, C.byref(sd), None) != 0 and b"target_pos is NULL" in err(dev.h)
    si.target_pos, si.weight = tp.data_ptr(), None
    assert call(dev.h, C.byref(si), 4, C.byref(sd), None) != 0 and b"weight is NULL" in err(dev.h)
    torch.cuda.synchronize()
    assert status.eq(9).all()                                               # nothing was launched
    si.weight = w.data_ptr()
    assert call(dev.h, C.byref(si), 0, C.byref(sd), None) == 0 and call(dev.h, C.byref(si), 4, C.byref(KSiteCostDev()), None) == 0
    assert call(dev.h, C.byref(si), 4, C.byref(sd), None) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0, 9, 9, 9, 9]
    dev.k_close()


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    fam = SR.family(asset, True)
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (2, len(labels), cm.act_dim)).astype(np.float32)
    for s in range(2):
        before, diag = a.state_tensors(), a.get_diag()
        _call(a, fam, envs=torch.arange(len(labels), dtype=torch.int32, device="cuda"))
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), s
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), s
        act = torch.from_numpy(acts[s]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), s
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done) and torch.equal(a.sim_time, b.sim_time)
    a.k_close(); b.k_close()


def test_the_planner_agrees_on_either_cost_path():
    """ilqr.ilqr on KManipSoloArmQPos, 4 envs, horizon 4, 2 iterations, fused linearisation and the device backward pass:
    SiteCost(device=True) and device=False agree on the first iteration's accepted cost under the bar, scaled by the cost (later
    accept decisions are discrete); neither history increases."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.examples import ilqr_site_reach as EX
    hist = []
    for device_cost in (False, True):
        env = env_hip.make("KManipSoloArmQPos", num_envs=4, seed=3)
        env.k_reset()
        out = EX.plan(env, env.state_tensors(), horizon=4, iters=2, device_cost=device_cost, fused=True, device_backward=True)
        env.k_close()
        J = out["res"]["cost"].cpu().numpy()
        assert np.isfinite(J).all() and (np.diff(J, axis=0) <= 0).all() and (J[1] < J[0]).all()
        hist.append(J)
    gap = np.abs(hist[0][:2] - hist[1][:2]) / np.abs(hist[0][:2])
    print("\ncost per iteration (torch cost) %s\n                   (device cost) %s\nrelative gap after the first iteration %.1e"
          % (hist[0].mean(axis=1).tolist(), hist[1].mean(axis=1).tolist(), gap.max()))
    assert gap.max() <= BAR_SITE_COST


@pytest.mark.parametrize("env_id,cube", sorted(REACH_MEASURED))
def test_the_example_reaches_on_the_device(env_id, cube):
    """gym_kmanip_amd/examples/ilqr_site_reach.py with the stand-in's shapes (2 envs, horizon 3, 2 iterations, seed 3), the device cost,
    the fused linearisation and the device backward pass: the median site-to-target distance ends below REACH_ASSERTED x its start --
    the stand-in's measured ratio (test_site_cost_cpu.REACH_MEASURED: 0.009 / 0.322 solo arm goal / cube, 0.011 / 0.685 dual arm) with
    the margin resolved_rate_reach took, 0.6 / 0.23, at most 1: 0.023 / 0.84 and 0.029 / 1.0."""
    _torch()
    from gym_kmanip_amd.examples import ilqr_site_reach as EX
    out = EX.main(["--env", env_id, "--num-envs", "2", "--horizon", "3", "--iters", "2", "--seed", "3", "--device-cost", "--fused",
                   "--device-backward"] + (["--cube"] if cube else []))
    ratio = out["end"] / out["start"]
    print("\n%s cube %d: median distance %.4f -> %.4f m (%.3f x; stand-in %.3f x, asserted %.3f x)"
          % (env_id, cube, out["start"], out["end"], ratio, REACH_MEASURED[(env_id, cube)], REACH_ASSERTED[(env_id, cube)]))
    assert all(b <= a for a, b in zip(out["cost"], out["cost"][1:]))
    assert ratio < REACH_ASSERTED[(env_id, cube)]
