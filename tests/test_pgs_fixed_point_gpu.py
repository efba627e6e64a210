"""The device's PGS against the Newton minimiser at a converged sweep cap (run with -m gpu on an MI355X).

tests/test_pgs_fixed_point_cpu.py pins the reference side: PGS_CAP sweeps per solve at tolerance 0 bring the oracle's PGS to within
KEEP = 1e-10 (qvel) of the oracle's Newton at tolerance 1e-12 in the kept envs, at least 80 % of every asset's regime cells, and the
bars BAR_PGS / BAR_PGS_QPOS follow from KEEP and the oracle's own spread.  Here the device's PGS kernels run the same cells at the
same cap, one zero-action control step from the states test_regimes_gpu loads:
  a. against the oracle's Newton reference, kept envs, at the bars: the point the device's sweeps converge to is the minimiser -- the
     comparison no sweep-for-sweep parity test at 100 sweeps makes;
  b. against the oracle's PGS at the same cap, every env (the unconverged G2 / G3 copies included): after up to 4e5 sweeps the two
     iterates still track each other at the project's bars, done bytes and contact masks exact;
  c. against a device Newton handle at tolerance 1e-12, kept envs, device against device;
  d. the other PGS builds reach the same point: the per-env-parameter kernels (cube mass x 2, friction 0.5), the applied-force
     kernels (a non-zero qfrc_applied on every joint and on the cube) and the launch shapes of 1, 2 and 4 envs per wave on the
     single arm;
  e. rollout() of one step at PGS_CAP returns the bytes of step_flat.
The device reports no sweep count (kmanip_get_diag has the IK's counters only), so "tolerance 0 never leaves early" is asserted on
the oracle's KoDiag.solver_iter here and shows on the device only through (b).  Wall times and worst differences measured on an
MI355X: DESIGN.md section 34."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mujoco_pin  # noqa: E402
import pgs_fixed_point as P  # noqa: E402
import regime_states as R  # noqa: E402
from pgs_fixed_point import PGS_CAP  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_V  # noqa: E402
from test_pgs_fixed_point_cpu import BAR_PGS, BAR_PGS_QPOS  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
PARAM_ASSETS = ("solo_arm", "dual_arm")
BARS = {"qvel": BAR_PGS, "qpos": BAR_PGS_QPOS}

_DEVICE_RUNS = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _loaded(asset, solver, cap, tol, build, friction_scale=None):
    """A handle of the capped model holding every cell's copies as test_regimes_gpu._device loads them (warm start from
    Oracle.after_reset of the model the env behaves like, step 0), with the build's parameters set in every env and its forces
    bound.  friction_scale: the cube friction of every env times it, on the device alone."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from oracle.oracle import Oracle
    cm = P.model(asset, solver, cap, tol)
    cmo = P.model(asset, solver, cap, tol, build)
    qpos, qvel, ctrl, labels = R.cells(asset)
    n = len(labels)
    warm = R.warm_start(cmo, Oracle(cmo, 1), qpos, qvel, ctrl)
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=0)
    dev.k_reset()
    p = P.params_of(cm, build)
    if friction_scale is not None:
        p = dict(p or {}, cube_friction=friction_scale * (p or {}).get("cube_friction", cm.desc.con_cube_friction[0]))
    if p is not None:
        dev.set_env_params(**{k: torch.full((n,), v, dtype=torch.float64) for k, v in p.items()})
    tau = P.forces_of(cm, n, build)
    if tau is not None:
        dev.new_applied_force().copy_(torch.from_numpy(tau))
    dev.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, step=np.zeros(n, dtype=np.int32))
    return dev, cm


def _device_run(asset, solver="pgs", build="plain", friction_scale=None):
    """One zero-action control step of the device, computed once per (asset, solver, build): dict(qpos, qvel, done, mask, seconds).
    PGS at PGS_CAP and tolerance 0, Newton at the reference's cap and tolerance."""
    torch = _torch()
    key = (asset, solver, build, os.environ.get("KMANIP_EPB"), friction_scale)
    if key not in _DEVICE_RUNS:
        cap, tol = (PGS_CAP[asset], 0.0) if solver == "pgs" else P.REFERENCE[1:]
        dev, cm = _loaded(asset, solver, cap, tol, build, friction_scale)
        act = torch.zeros((dev.num_envs, cm.act_dim), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.step_flat(act)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        qpos, qvel = dev.get_state()[:2]
        _DEVICE_RUNS[key] = dict(qpos=qpos, qvel=qvel, done=dev.done.cpu().numpy(), mask=dev.get_diag()[0], seconds=seconds)
        dev.k_close()
        print("\n%s %s %s cap %d%s: step_flat of %d envs took %.2f s" % (asset, solver, build, cap, "" if key[3] is None else " KMANIP_EPB=" + key[3],
                                                                       len(qpos), seconds))
    return _DEVICE_RUNS[key]


def _within_the_bars(tag, got, ref, kept, labels):
    """qvel and qpos of every kept env within BAR_PGS / BAR_PGS_QPOS of the reference; prints the worst differences."""
    bad = []
    for key, bar in BARS.items():
        d = P.distance(got, ref, key)
        print("%s: worst |%s - reference| over the %d kept envs %.1e (bar %.0e); over the %d others %.1e" % (
            tag, key, int(kept.sum()), d[kept].max(), bar, int((~kept).sum()), d[~kept].max(initial=0.0)))
        bad += [(key, labels[e], int(e), float(d[e])) for e in np.where(kept & ~(d <= bar))[0]]
    assert not bad, (tag, bad)


def _tracks_the_oracles_pgs(tag, got, orc, asset, labels):
    """Done bytes and contact masks exact, qvel / qpos of EVERY env within TOL_V / TOL_Q of the oracle's PGS at the same cap, whose
    sweep count shows that no solve left early."""
    nsub = P.model(asset, "pgs", PGS_CAP[asset], 0.0).desc.n_sub_steps
    assert (orc["iters"] == nsub * PGS_CAP[asset]).all(), sorted(set(orc["iters"].tolist()))
    for key in ("done", "mask"):
        eq = got[key] == orc[key]
        assert eq.all(), (tag, key, [(labels[e], int(e)) for e in np.where(~eq)[0]])
    assert not got["done"].any()
    for key, bar in (("qvel", TOL_V), ("qpos", TOL_Q)):
        d = P.distance(got, orc, key)
        print("%s: worst |%s - oracle PGS at the same cap| over all envs %.1e (bar %.0e)" % (tag, key, d.max(), bar))
        assert (d < bar).all(), (tag, key, [(labels[e], int(e), float(d[e])) for e in np.where(~(d < bar))[0]])


# ---------------------------------------------------------------------------------------------------- a. against the Newton reference
@pytest.mark.parametrize("asset", ASSETS)
def test_device_pgs_reaches_the_newton_minimiser(asset):
    """The default launch shape, every cell's copies in one handle: qvel and qpos of every kept env within BAR_PGS / BAR_PGS_QPOS
    (1e-9) of the oracle's Newton at tolerance 1e-12.  A device PGS whose fixed point is not the minimiser -- a wrong R in a
    contact's Gram rows, a wrong edge sign, a clamp on the wrong side -- fails here by the factor test_a_wrong_input_is_seen shows
    for a 1 % error (1e5 bars and more), while it passes every parity test against an oracle that shares the error."""
    labels = R.cells(asset)[3]
    kept = P.kept_conditions(asset)
    got = _device_run(asset)
    _within_the_bars("%s pgs cap %d against the oracle's Newton" % (asset, PGS_CAP[asset]), got, P.reference(asset), kept, labels)


def test_a_wrong_input_on_the_device_is_seen():
    """test_pgs_fixed_point_cpu.test_a_wrong_input_is_seen on the device: the single arm's handle with the cube friction of every
    env times 1.01 (set_env_params), the reference as it was.  At least SEEN_SHARE of the kept envs with a cube contact leave the
    bar by a factor of 100 or more, so (a) has the power the CPU file claims for it; the same handle is within TOL_V of the oracle's
    PGS on the same wrong model, which is all a sweep-for-sweep comparison would have asked.  Measured on an MI355X: 33 of 34 envs
    moved, median 1.2e-3."""
    from test_pgs_fixed_point_cpu import BLIND, SEEN_SHARE
    asset = "solo_arm"
    labels = R.cells(asset)[3]
    sel = P.kept_conditions(asset) & P.has_rows(asset)[1]
    got = _device_run(asset, friction_scale=1.01)
    d = P.distance(got, P.reference(asset))[sel]
    print("%s: %d kept envs with a cube contact, %d moved by more than %.0e (median %.1e)" % (asset, len(d), int((d > BLIND).sum()), BLIND, np.median(d)))
    assert (d > BLIND).sum() >= SEEN_SHARE * len(d), (len(d), int((d > BLIND).sum()))
    _tracks_the_oracles_pgs("%s pgs cap %d at 1.01 x the cube friction" % (asset, PGS_CAP[asset]), got, P.pgs(asset, friction_scale=1.01), asset, labels)


# ------------------------------------------------------------------------------------------------ b. against the oracle's PGS, every env
@pytest.mark.parametrize("asset", ASSETS)
def test_device_pgs_tracks_the_oracles_pgs_to_the_last_sweep(asset):
    """n_sub_steps x PGS_CAP sweeps (3e5, 4e5, 1e5) on both sides: the iterates are within TOL_V / TOL_Q in every env, the G2 / G3
    copies that are still 1e-6 from their fixed point included -- rounding accumulated in the device's block form over that many
    sweeps stays where it is after 100 (measured: 1e-12).  Done bytes and contact masks are exact."""
    labels = R.cells(asset)[3]
    _tracks_the_oracles_pgs("%s pgs cap %d" % (asset, PGS_CAP[asset]), _device_run(asset), P.pgs(asset), asset, labels)


# ------------------------------------------------------------------------------------------------- c. against the device's own Newton
@pytest.mark.parametrize("asset", ASSETS)
def test_device_pgs_reaches_the_device_newton(asset):
    """The same states in a device Newton handle at cap 100 and tolerance 1e-12: the kept envs of the device's PGS are within the
    bars of it.  Device against device: the oracle enters through the kept set and the warm starts alone."""
    labels = R.cells(asset)[3]
    kept = P.kept_conditions(asset)
    newton = _device_run(asset, "newton")
    assert not newton["done"].any()
    _within_the_bars("%s pgs cap %d against the device's Newton" % (asset, PGS_CAP[asset]), _device_run(asset), newton, kept, labels)


# ------------------------------------------------------------------------------------------------------------- d. the other PGS builds
@pytest.mark.parametrize("asset", PARAM_ASSETS)
def test_the_per_env_parameter_build_reaches_the_minimiser(asset):
    """set_env_params(cube mass x 2, cube friction 0.5) in every env launches the per-env-parameter PGS kernels.  The reference is
    the oracle's Newton on model.with_env_params of the same values, the kept set is recomputed for these inputs by the same rule
    (80 % of the envs at least), and the device is held to both as in (a) and (b)."""
    labels = R.cells(asset)[3]
    kept = P.kept_conditions(asset, "params")
    got = _device_run(asset, build="params")
    plain = P.reference(asset)
    assert (P.distance(P.reference(asset, "params"), plain) > 100.0 * BAR_PGS).sum() >= len(labels) // 2      # the parameters bite
    tag = "%s pgs cap %d with parameters" % (asset, PGS_CAP[asset])
    _within_the_bars(tag + " against the oracle's Newton", got, P.reference(asset, "params"), kept, labels)
    _tracks_the_oracles_pgs(tag, got, P.pgs(asset, build="params"), asset, labels)


@pytest.mark.parametrize("asset", PARAM_ASSETS)
def test_the_applied_force_build_reaches_the_minimiser(asset):
    """A bound qfrc_applied (applied_oracle.draw_test_forces: +-2 on every joint, +-2 m g on the cube's force components, +-1e-3 on
    its torques) launches the applied-force PGS kernels.  Reference and kept set are the oracle's Newton and PGS under the same
    forces (Oracle.physics_step_applied, which tests/test_pgs_fixed_point_cpu.py holds to the NumPy restatement of the applied-force
    tests); the device is held to both as in (a) and (b)."""
    labels = R.cells(asset)[3]
    kept = P.kept_conditions(asset, "forced")
    got = _device_run(asset, build="forced")
    assert (P.distance(P.reference(asset, "forced"), P.reference(asset)) > 100.0 * BAR_PGS).all()              # the forces bite
    tag = "%s pgs cap %d under applied forces" % (asset, PGS_CAP[asset])
    _within_the_bars(tag + " against the oracle's Newton", got, P.reference(asset, "forced"), kept, labels)
    _tracks_the_oracles_pgs(tag, got, P.pgs(asset, build="forced"), asset, labels)


@pytest.mark.parametrize("epb", [1, 2, 4])
def test_every_launch_shape_reaches_the_minimiser(epb, monkeypatch):
    """The single arm at KMANIP_EPB = 1, 2 and 4 envs per wave (a handle this small gets one env per wave by itself; training
    batches run four): the kept envs within the bars of the oracle's Newton, every env within TOL_V of the oracle's PGS -- and the
    bytes of the default shape's run, as kmanip.h promises of wave-mates."""
    asset = "solo_arm"
    labels = R.cells(asset)[3]
    kept = P.kept_conditions(asset)
    default = _device_run(asset)
    monkeypatch.setenv("KMANIP_EPB", str(epb))
    got = _device_run(asset)
    monkeypatch.delenv("KMANIP_EPB")
    tag = "%s pgs cap %d at %d envs per wave" % (asset, PGS_CAP[asset], epb)
    _within_the_bars(tag + " against the oracle's Newton", got, P.reference(asset), kept, labels)
    _tracks_the_oracles_pgs(tag, got, P.pgs(asset), asset, labels)
    for key in ("qpos", "qvel", "done", "mask"):
        assert np.array_equal(got[key], default[key]), (epb, key)


# --------------------------------------------------------------------------------------------------------------------- e. the row kernel
@pytest.mark.parametrize("asset", ASSETS)
def test_a_rollout_of_one_step_is_the_step_at_the_converged_cap(asset):
    """test_rollout_gpu's step identity at a cap where it has never run: rollout() from the cells' rows, with the ctrl the step
    stored, nstep = 1 and the model's sub-steps, gives the bytes of step_flat's qpos, qvel, warm start, contact mask and reward."""
    torch = _torch()
    dev, cm = _loaded(asset, "pgs", PGS_CAP[asset], 0.0, "plain")
    start = {k: v.clone() for k, v in dev.state_tensors().items()}
    dev.step_flat(torch.zeros((dev.num_envs, cm.act_dim), dtype=torch.float32, device="cuda"))
    after = dev.state_tensors()
    want = dict(qpos=after["qpos"], qvel=after["qvel"], qacc_warm=after["warm"], reward=dev.reward.clone(),
                contact_mask=torch.from_numpy(dev.get_diag()[0].view(np.int32)).cuda())
    assert not dev.done.any()
    t0 = time.perf_counter()
    got = dev.rollout(qpos=start["qpos"], qvel=start["qvel"], warm=start["warm"], ctrl=after["ctrl"], nstep=1)
    torch.cuda.synchronize()
    print("\n%s pgs cap %d: rollout() of %d rows took %.2f s" % (asset, PGS_CAP[asset], dev.num_envs, time.perf_counter() - t0))
    assert not got["status"].any() and bool((got["steps_done"] == 1).all())
    for key, w in want.items():
        assert torch.equal(got[key][:, 0], w), (asset, key, float((got[key][:, 0].double() - w.double()).abs().max()))
    dev.k_close()
