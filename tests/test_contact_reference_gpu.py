"""The device's contact geometry and contact rows against the independent reference, on a box that is not a cube (run with -m gpu
on an MI355X).

The models are tests/tools/contact_model.py's box (cube_half = (0.03, 0.02, 0.012)) and box0 (box without friction loss), the states
tests/tools/contact_states.py's (the box at every collider over every face, edge and vertex and inside under every face, every
capsule section at t clamped to 0, interior and clamped to 1, 5 .. 8 corners under the table, a cube across every table_rect bound,
one sphere more on the box than there are slots; 59 / 89 / 89 states in one handle per asset and model), the reference
tests/tools/contact_reference.py (closest point by enumerating the box's features, Jacobians by finite differences of Oracle.fk):
  forces() on box    mask, contact_bit, frame, point and distance against the REFERENCE at BAR_GEOMETRY; forces, qacc and qfrc_constraint
                     against force_oracle.decode at the bars of test_forces_gpu; the raised-table models (one sphere more under the
                     table than slots, a rectangle bound between two penetrating spheres) the same way;
  forces() on box0   the virtual-work identity: sum over the device's own reported wrenches of (reference Jacobian)^T wrench equals
                     the device's qfrc_constraint, at the bar of test_contact_reference_cpu -- the device's rows (ancestor masks,
                     slide / hinge split, the cube's body-frame angular columns, b1 / b2 per slot kind, the torsion row) pinned
                     without the oracle's body_jac;
  the step           test_regimes_gpu._free_run (its bars, its guard) on every state, Newton and PGS, zero and +-0.2 random actions;
  launch shapes      one env per wave against the default shape and against step_chunk: every bit;
  kmanip_observe     its contact mask on the same states against the reference's;
  renders            depth, RGB, labels and points of a rotated non-cubic box against the existing oracles at those tests' own bars.
  soft constraints   every variant of contact_states.SOFT_VARIANTS (solref / solimp values no shipped asset has): forces() and
                     the step against the oracle.
Measured on an MI355X: DESIGN.md section 23."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import contact_model as CM  # noqa: E402
import contact_reference as CR  # noqa: E402
import contact_states as CS  # noqa: E402
import force_oracle as FO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import test_forces_gpu as TF  # noqa: E402
import test_regimes_gpu as TR  # noqa: E402
from test_contact_reference_cpu import refs, render_states, virtual_work_case  # noqa: E402
from test_forces_cpu import BAR_GEOMETRY  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")

_WARM = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _case(asset, variant="cm"):
    """(cm, states dict, refs, warm) of the asset on box ("cm") or box0 ("cm0"); the warm start computed once per model."""
    from oracle.oracle import Oracle
    st, rf = refs(asset)
    cm = st[variant]
    if (asset, variant) not in _WARM:
        _WARM[asset, variant] = R.warm_start(cm, Oracle(cm, 1), st["qpos"], st["qvel"], st["ctrl"])
    return cm, st, rf, _WARM[asset, variant]


def _against_reference(f, e, geo, what):
    """Mask, contact_bit, frame, point and distance of env e of a forces() result against the reference's geometry: the violations
    and the largest difference."""
    if f["status"][e] != 0:
        return [(what, "status", int(f["status"][e]))], 0.0
    if int(f["contact_mask"][e]) != geo["mask"]:
        return [(what, "mask", hex(int(f["contact_mask"][e])), hex(geo["mask"]))], 0.0
    bits = [int(b) for b in f["contact_bit"][e]]
    if sorted(b for b in bits if b >= 0) != [c["bit"] for c in geo["contacts"]]:
        return [(what, "contact_bit", bits)], 0.0
    worst, bad = 0.0, []
    for c in geo["contacts"]:
        s = bits.index(c["bit"])
        dd = max(float(np.abs(f["contact_frame"][e, s] - c["frame"].reshape(-1)).max()), float(np.abs(f["contact_pos"][e, s] - c["pos"]).max()),
                 abs(float(f["contact_dist"][e, s]) - c["dist"]))
        worst = max(worst, dd)
        if not dd <= BAR_GEOMETRY:
            bad.append((what, "geometry", c["bit"], dd))
    return bad, worst


@pytest.mark.parametrize("asset", ASSETS)
def test_forces_geometry_against_the_reference_and_forces_against_the_oracle(asset):
    from oracle.oracle import Oracle
    cm, st, rf, warm = _case(asset)
    dev = TF._device(cm, st["qpos"], st["qvel"], st["ctrl"], warm)
    f = TF._host(dev.forces())
    dev.k_close()
    orc = Oracle(cm, 1)
    figures, bad, worst = [], [], 0.0
    for e, ref in enumerate(rf):
        what = (st["labels"][e], e)
        b, w = _against_reference(f, e, ref["geo"], what)
        bad += b
        worst = max(worst, w)
        bad += TF._compare(cm, f, e, FO.decode(cm, orc, st["qpos"][e], st["qvel"][e], st["ctrl"][e]), what, figures)
    print("\n%s box: |device - reference| geometry, worst %.1e" % (asset, worst))
    TF._report(asset + " box", figures)
    assert not bad, bad
    assert max((b >= 0).sum() for b in f["contact_bit"]) >= 4


@pytest.mark.parametrize("asset", ASSETS)
def test_forces_and_the_observe_mask_on_the_raised_table_models(asset):
    """One handle per model, one env each: more spheres under the table than KM_SPHERE_TABLE_SLOTS, and a table_rect bound between
    two penetrating spheres -- the ranks taken from the ballot and over_table on spheres."""
    from oracle.oracle import Oracle
    bad, figures = [], []
    for name, cm, qpos, qvel, ctrl in CS.table_states(asset):
        orc = Oracle(cm, 1)
        geo = CR.geometry(cm, orc, qpos[0])
        assert len(geo["contacts"]) >= 1 and geo["info"]["n_sphere_table"] >= 1
        dev = TF._device(cm, qpos, qvel, ctrl, R.warm_start(cm, orc, qpos, qvel, ctrl))
        f = TF._host(dev.forces())
        dev.observe()
        seen = int(dev.get_diag()[0][0])
        dev.k_close()
        b, w = _against_reference(f, 0, geo, (name, 0))
        bad += b + TF._compare(cm, f, 0, FO.decode(cm, orc, qpos[0], qvel[0], ctrl[0]), (name, 0), figures)
        if seen != geo["mask"]:
            bad.append((name, "observe mask", hex(seen), hex(geo["mask"])))
        print("\n%s %s: mask %s, |device - reference| geometry %.1e" % (asset, name, hex(geo["mask"]), w))
    TF._report(asset + " raised table", figures)
    assert not bad, bad


@pytest.mark.parametrize("asset", ASSETS)
def test_virtual_work_of_the_devices_wrenches_is_its_qfrc_constraint(asset):
    """box0.  The wrenches and qfrc_constraint are the DEVICE's, the Jacobians the reference's finite differences: a wrong column
    of the device's rows leaves J^T f of its own solve different from the work its reported wrenches do."""
    cm0, st, rf, warm = _case(asset, "cm0")
    dev = TF._device(cm0, st["qpos"], st["qvel"], st["ctrl"], warm)
    f = TF._host(dev.forces())
    dev.k_close()
    bad, frac, worst, big = [], 0.0, 0.0, 0.0
    for e, ref in enumerate(rf):
        what = (st["labels"][e], e)
        b, _ = _against_reference(f, e, ref["geo"], what)
        if b:
            bad += b
            continue
        by_bit = {int(bit): f["contact_force"][e, s] for s, bit in enumerate(f["contact_bit"][e]) if bit >= 0}
        dd, bar, fmax = virtual_work_case(cm0, ref, by_bit, f["qfrc_constraint"][e], st["qpos"][e])
        frac, big = max(frac, dd / bar), max(big, fmax)
        worst = max(worst, dd / max(1.0, float(np.abs(f["qfrc_constraint"][e]).max())))
        if not dd <= bar:
            bad.append((what, "virtual work", dd, bar))
    print("\n%s box0: virtual work of the device's wrenches: worst |Q - qfrc_constraint| / max(1, max|qfrc_constraint|) %.1e, worst fraction "
          "of the bar %.1e, largest contact force %.1e" % (asset, worst, frac, big))
    assert not bad, bad
    assert big > 1.0


@pytest.mark.parametrize("kind", ["zero", "random"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_states_free_running_parity(asset, solver, kind):
    """test_regimes_gpu._free_run on box: every state, its three control steps, its bars, its guard on the oracle's own spread."""
    st, _ = refs(asset)
    cm = CM.box(R.model(asset, solver))
    assert bytes(cm.desc.cube_half) == bytes(st["cm"].desc.cube_half)
    n = len(st["labels"])
    worst, spread, masks, _ = TR._free_run(cm, (st["qpos"], st["qvel"], st["ctrl"]), st["labels"], TR._actions(cm, n, kind))
    TR._report("%s box %s %s" % (asset, solver, kind), worst, spread)
    assert ((masks[0] & 0x000FFF00) != 0).any()


@pytest.mark.parametrize("asset", ASSETS)
def test_launch_shapes_change_no_bit(asset, monkeypatch):
    """The same handle through three steps of small random actions: one env per wave (KMANIP_EPB=1) against the default shape and
    against one step_chunk(3).  qpos, qvel, ctrl, obs, reward, done, step counter and contact mask of every env, bit for bit."""
    torch = _torch()
    cm, st, rf, warm = _case(asset)
    n = len(st["labels"])
    acts = TR._actions(cm, n, "random", seed=4)

    def run(epb, chunk=False):
        monkeypatch.setenv("KMANIP_EPB", str(epb)) if epb else monkeypatch.delenv("KMANIP_EPB", raising=False)
        dev = TR._device(cm, st["qpos"], st["qvel"], st["ctrl"], warm)
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
    assert np.abs(ref[2]["qpos"] - st["qpos"]).max() > 0 and not (ref[2]["done"] & TR.KM_DONE_DIVERGED).any()
    for what, runs in (("default", run(None)), ("chunk", run(None, chunk=True))):
        for s in range(3):
            for key in runs[s]:
                eq = (runs[s][key] == ref[s][key]).reshape(n, -1).all(axis=1)
                assert eq.all(), (what, s, key, [(st["labels"][e], e) for e in np.where(~eq)[0]])
    monkeypatch.delenv("KMANIP_EPB", raising=False)


@pytest.mark.parametrize("asset", ASSETS)
def test_the_observe_mask_is_the_references(asset):
    cm, st, rf, warm = _case(asset)
    dev = TF._device(cm, st["qpos"], st["qvel"], st["ctrl"], warm)
    dev.observe()
    seen = dev.get_diag()[0]
    dev.k_close()
    want = np.array([ref["geo"]["mask"] for ref in rf], dtype=np.uint32)
    diff = np.where(seen != want)[0]
    assert not len(diff), [(st["labels"][e], hex(int(seen[e])), hex(int(want[e]))) for e in diff]
    assert len(set(want.tolist())) >= 10


@pytest.mark.parametrize("asset", ["solo_arm", "torso"])
def test_renders_of_a_rotated_box_that_is_not_a_cube(asset):
    """Depth, RGB, labels and points of the right gripper camera on box, six states with the rotated box at a finger: against
    ko_render_depth / ko_render_rgb, label_oracle and point_oracle at the bars of test_gpu_parity.test_render_depth_parity (1e-6 m,
    < 0.05 % of the pixels), test_check_env_gpu's RGB check (more than one grey level off in < 0.1 % of the pixels),
    test_label_render_gpu._oracle_check and test_points_gpu._point_bar.  (That swapping two half sizes in the oracle changes
    every one of these images is asserted on the CPU: test_contact_reference_cpu.)"""
    from label_oracle import LabelOracle
    from oracle.oracle import Oracle
    from point_oracle import PointOracle
    from test_check_env_gpu import RGB_BAD_SHARE, RGB_LEVELS
    from test_gpu_parity import DEPTH_BAD_SHARE, DEPTH_TOL
    from test_label_render_gpu import _oracle_check
    from test_points_gpu import _point_bar
    cm, qpos = render_states(asset)
    n = len(qpos)
    orc = Oracle(cm, 1)
    dev = TF._device(cm, qpos, np.zeros((n, cm.nv)), R.f32(qpos[:, :cm.nlink]), np.zeros((n, cm.nv)))
    depth = dev.render_depth("grip_r", 64, 64).cpu().numpy()
    for e in range(n):
        bad = np.abs(depth[e] - orc.render_depth(qpos[e], 0, 64, 64)) > DEPTH_TOL
        assert bad.mean() < DEPTH_BAD_SHARE, ("depth", e, int(bad.sum()))
    rgb = dev.render_rgb("grip_r", 40, 60).cpu().numpy()
    for e in range(n):
        diff = np.abs(rgb[e].astype(int) - orc.render_rgb(qpos[e], 0, 40, 60).astype(int)).max(axis=-1)
        assert (diff > RGB_LEVELS).mean() < RGB_BAD_SHARE, ("rgb", e, int((diff > RGB_LEVELS).sum()))
    seg = _oracle_check(dev, [LabelOracle(cm)] * n, qpos, "grip_r", 40, 60)
    assert (seg == 2).any()
    po = PointOracle(cm)
    ref = [po.render(qpos[e], 0, 30, 50, (), "world") for e in range(n)]
    got = dev.render_points("grip_r", 30, 50, frame="world").cpu().numpy()
    _point_bar(got, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), ref[0][3], ref[0][4], (asset, "box", "grip_r", 30, 50))
    dev.k_close()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("variant", list(CS.SOFT_VARIANTS))
@pytest.mark.parametrize("asset", ASSETS)
def test_soft_constraint_constants_forces_and_a_step(asset, variant, solver):
    """contact_states.SOFT_VARIANTS: the device's impedance spline (impedance_c: staged reciprocals, no pow) on its power-1 path, with
    the midpoint off 0.5, with d0 above and equal to dw, a width at MJ_MINVAL, a time constant that the 2 dt clamp replaces and
    damping ratios off 1 -- set on the cube pairs and on the default set.  Six states (a finger 0.2, 0.7 and 1.3 widths deep in the
    box, a joint as far beyond its range): forces() against force_oracle.decode at the bars of test_forces_gpu (Newton handle), and
    test_regimes_gpu._free_run's steps at its bars with its guard (both solvers).  Device against the oracle, whose rows
    test_contact_reference_cpu holds to a NumPy restatement of MuJoCo's documented curve: a restatement, not an independent reference."""
    from oracle.oracle import Oracle
    base, qpos, qvel, ctrl, labels, _ = CS.soft_states(asset)
    cm = CS.soft_model(CM.box(R.model(asset, solver)), variant)
    assert bytes(cm.desc.con_cube_solimp) == bytes(CS.soft_model(base, variant).desc.con_cube_solimp)
    if solver == "newton":
        orc = Oracle(cm, 1)
        dev = TF._device(cm, qpos, qvel, ctrl, R.warm_start(cm, orc, qpos, qvel, ctrl))
        f = TF._host(dev.forces())
        dev.k_close()
        figures, bad = [], []
        for e in range(len(labels)):
            bad += TF._compare(cm, f, e, FO.decode(cm, orc, qpos[e], qvel[e], ctrl[e]), (labels[e], e), figures)
        TF._report("%s %s" % (asset, variant), figures)
        assert not bad, bad
        assert all(f["contact_mask"][e] & 0x100 for e in range(3))
    worst, spread, masks, _ = TR._free_run(cm, (qpos, qvel, ctrl), labels, TR._actions(cm, len(labels), "random"))
    TR._report("%s %s %s" % (asset, variant, solver), worst, spread)
