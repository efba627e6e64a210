"""The PGS solver against the Newton minimiser at a converged sweep cap, on the CPU oracle alone: the reference side of
tests/test_pgs_fixed_point_gpu.py.

Every other PGS test compares the device's iterate with the oracle's iterate, sweep for sweep, at the shipped cap of 100 sweeps --
where PGS is nowhere near its fixed point, and where a formula error the two restatements of mj_solPGS share (a wrong R in a block's
Gram matrix, a wrong edge sign, a box clamp on the wrong side) passes.  PGS's fixed point is the KKT point of the dual; for pyramidal
cones that is the unique minimiser Newton finds, and Newton has outside references (test_newton_solution_vs_scipy_minimize, DESIGN.md
section 24).  So here the oracle's PGS runs the regime cells at PGS_CAP sweeps and tolerance 0 (tests/tools/pgs_fixed_point.py) and is
held to the oracle's Newton at tolerance 1e-12, one zero-action control step on:
  - the kept set (the envs in which PGS has arrived, to KEEP = 1e-10 in qvel) holds 80 % of every asset's envs and an env of every
    cell but G2 and G3;
  - the distance to the reference does not grow from cap 100 to 1000 to PGS_CAP, and tolerance 0 never leaves a solve early;
  - the shipped cap cannot see any of this: most kept envs with a contact or a limit are more than 100 bars away at cap 100;
  - BAR_PGS / BAR_PGS_QPOS, the bars of the GPU test, follow from KEEP and the oracle's own spread at PGS_CAP;
  - a solve with one wrong input (the cube friction off by 1 %) lands more than 100 bars away in most envs with a cube contact.
Measured figures: DESIGN.md section 34."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import mujoco_pin  # noqa: E402
import pgs_fixed_point as P  # noqa: E402
import regime_states as R  # noqa: E402
from pgs_fixed_point import KEEP, PGS_CAP  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_V  # noqa: E402
from test_solver_caps_cpu import capped_model, control_steps  # noqa: E402

ASSETS = mujoco_pin.ASSETS
# (asset, build) of every kept set a GPU row uses: the plain build of all assets, the parameter and the applied-force build of two
KEPT_ROWS = [(a, "plain") for a in ASSETS] + [(a, b) for b in ("params", "forced") for a in ("solo_arm", "dual_arm")]

# the oracle PGS's own spread at PGS_CAP: the largest |twin - oracle| of an env after the control step, the twin started from
# qvel (1 + 1e-15), over all envs of KEPT_ROWS (measured: see test_the_bars_follow_from_the_spread)
SPREAD_QVEL = 3.1e-13
SPREAD_QPOS = 2.0e-15


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


# the bar of the GPU test: ten times KEEP (a kept env of the oracle may sit at KEEP itself; the device's iterate, 1e-12 from the
# oracle's, must not fail for that) or 1000 x the spread, the project's margin between two formulations, whichever is larger
BAR_PGS = max(_round_up_one_digit(10.0 * KEEP), _round_up_one_digit(1000.0 * SPREAD_QVEL))
BAR_PGS_QPOS = max(_round_up_one_digit(10.0 * KEEP), _round_up_one_digit(1000.0 * SPREAD_QPOS))
# distances below ten times the spread are rounding, and cannot be ordered
NOISE = 10.0 * SPREAD_QVEL
BLIND = 100.0 * BAR_PGS                  # "far from the reference": a hundred bars
BLIND_SHARE = 0.5                        # the least share of kept envs with rows that cap 100 leaves further than BLIND away
# the least share of kept envs with a cube contact that a 1 % change of the cube friction moves by more than BLIND; measured
# shares in the docstring of test_a_wrong_input_is_seen
SEEN_SHARE = 0.9


# ------------------------------------------------------------------------------------------------------------------- the kept set
@pytest.mark.parametrize("asset,build", KEPT_ROWS)
def test_the_kept_set_is_large_and_covers_the_cells(asset, build):
    """At least 80 % of the asset's envs are within KEEP of the Newton reference after PGS_CAP sweeps per solve, and every cell but
    G2 and G3 has such an env.  Measured (kept / envs at PGS_CAP; plain build): SoloArm 40 / 47 at 30000, DualArm 67 / 72 at 40000,
    Torso 62 / 72 at 10000, all left out G2 or G3 copies but one L1 copy of the Torso (1.8e-10); with parameters SoloArm 42 / 47,
    DualArm 66 / 72; under the test forces SoloArm 39 / 47, DualArm 67 / 72.  The cells are asked of the plain build, the share of every build (pgs_fixed_point.kept_conditions)."""
    labels = np.array(R.cells(asset)[3])
    d = P.distance(P.pgs(asset, build=build), P.reference(asset, build))
    k = P.kept_conditions(asset, build)
    print("\n%s %s cap %d: kept %d of %d (%.3f); worst kept %.1e, worst of all %.1e" % (asset, build, PGS_CAP[asset], int(k.sum()), len(k), k.mean(),
                                                                                   d[k].max(), d.max()))
    for c in dict.fromkeys(labels):
        sel = labels == c
        print("  %-5s kept %d of %d, worst %.1e" % (c, int(k[sel].sum()), int(sel.sum()), d[sel].max()))
    ref = P.reference(asset, build)
    assert not ref["done"].any() and np.isfinite(ref["qvel"]).all()
    assert ref["iters"].max() < 100                                                                 # no Newton solve ends at its cap


# ------------------------------------------------------------------------------------------------------------------- convergence
@pytest.mark.parametrize("asset", ASSETS)
def test_the_distance_to_the_minimiser_falls_with_the_cap(asset):
    """On the kept envs the distance to the reference at cap 1000 is no larger than at cap 100, and at PGS_CAP no larger than at
    1000 -- where it is not already rounding (NOISE, ten times the oracle's spread).  Tolerance 0 never leaves a solve early: the
    sweeps KoDiag.solver_iter counts over the control step are n_sub_steps x cap in every env, at every cap.  Measured max (median)
    over all envs at caps 100 / 1000 / PGS_CAP: DESIGN.md section 34."""
    k = P.kept_conditions(asset)
    ref = P.reference(asset)
    nsub = capped_model(asset, "pgs", 100, 0.0).desc.n_sub_steps
    caps = P.LOWER_CAPS + (PGS_CAP[asset],)
    dist = []
    print()
    for cap in caps:
        run = P.pgs(asset, cap)
        assert (run["iters"] == nsub * cap).all(), (cap, sorted(set(run["iters"].tolist())))
        dist.append(P.distance(run, ref))
        print("%s cap %6d: max |qvel - newton| %.1e (median %.1e); kept envs %.1e; share within KEEP %.3f" % (
            asset, cap, dist[-1].max(), np.median(dist[-1]), dist[-1][k].max(), (dist[-1] <= KEEP).mean()))
    for a, b, cap in zip(dist, dist[1:], caps[1:]):
        grew = k & (b > np.maximum(a, NOISE))
        assert not grew.any(), (cap, [(int(e), float(a[e]), float(b[e])) for e in np.where(grew)[0]])


@pytest.mark.parametrize("asset", ASSETS)
def test_the_shipped_cap_cannot_see_the_fixed_point(asset):
    """Of the kept envs with a contact or a joint beyond its range, at least half are more than 100 x BAR_PGS from the reference
    at the shipped cap of 100 sweeps.  Measured: SoloArm 24 of 34 (median distance of the 34: 3.8e-3), DualArm 47 of 61 (3.6e-3),
    Torso 36 of 62 (2.2e-5; its home pose has joints beyond their ranges, so every env counts): what the 100-sweep parity tests
    compare is two unconverged iterates."""
    k = P.kept_conditions(asset)
    rows = P.has_rows(asset)[0]
    d = P.distance(P.pgs(asset, 100), P.reference(asset))[k & rows]
    print("\n%s: %d kept envs with rows, %d further than %.0e at cap 100 (median %.1e)" % (asset, len(d), int((d > BLIND).sum()), BLIND, np.median(d)))
    assert len(d) >= 20 and (d > BLIND).sum() >= BLIND_SHARE * len(d), (len(d), int((d > BLIND).sum()))


# -------------------------------------------------------------------------------------------------------------------------- the bars
def test_the_bars_follow_from_the_spread():
    """BAR_PGS = max(10 KEEP, 1000 x the oracle PGS's twin spread at PGS_CAP), rounded up to one digit, and the same for qpos.
    The spread is re-measured over every env of KEPT_ROWS (the unconverged G2 / G3 copies included) and must stay a factor 1000 under
    the bars; the recorded constants must be the measured ones to their two digits, so the bars cannot drift from their source.
    Measured (qvel / qpos): SoloArm 3.1e-13 / 2.0e-15, DualArm 2.5e-13 / 1.3e-15, Torso 6.9e-14 / 4.4e-16; with parameters SoloArm
    3.1e-13 / 8.9e-16, DualArm 2.5e-13 / 1.3e-15; under the test forces SoloArm 2.2e-13 / 1.0e-15, DualArm 2.3e-13 / 1.3e-15.  1000 x 3.1e-13 rounds up to 4e-10, below 10 KEEP: both bars are 1e-9."""
    worst = {"qvel": 0.0, "qpos": 0.0}
    print()
    for asset, build in KEPT_ROWS:
        a, b = P.pgs(asset, build=build), P.pgs(asset, build=build, twin=True)
        s = {key: float(P.distance(a, b, key).max()) for key in worst}
        print("%s %s cap %d: spread qvel %.1e qpos %.1e" % (asset, build, PGS_CAP[asset], s["qvel"], s["qpos"]))
        worst = {key: max(worst[key], s[key]) for key in worst}
    for key, rec, bar in (("qvel", SPREAD_QVEL, BAR_PGS), ("qpos", SPREAD_QPOS, BAR_PGS_QPOS)):
        assert 1000.0 * worst[key] <= bar, (key, worst[key], bar)
        assert worst[key] <= rec * 1.05 and worst[key] >= rec / 1.05, (key, worst[key], rec)
        assert bar == pytest.approx(max(10.0 * KEEP, _round_up_one_digit(1000.0 * rec)), rel=1e-12)
    assert BAR_PGS == pytest.approx(1e-9, rel=1e-12) and BAR_PGS_QPOS == pytest.approx(1e-9, rel=1e-12)
    # the reference is not in question: Newton at the shipped tolerance gives the same point
    for asset in ASSETS:
        d = P.distance(P.run(asset, "newton", 100, 1e-8), P.reference(asset))
        print("%s: newton at 1e-8 against 1e-12: %.1e" % (asset, d.max()))
        assert 1000.0 * d.max() <= BAR_PGS


# --------------------------------------------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("asset", ASSETS)
def test_a_wrong_input_is_seen(asset):
    """A solve that consumes one wrong number must fail the comparison: the cube friction of the PGS model alone times 1.01
    (model.with_env_params: mu of every cube contact's pyramid, and through it the edges' R), the Newton reference as it was.  Of
    the kept envs with a cube contact (a corner on the table or a sphere on the cube) those that move further than 100 x BAR_PGS
    from the reference (measured): SoloArm 33 of 34, DualArm 60 of 61, Torso 53 of 56, median move 1.2e-3 .. 1.6e-3; SEEN_SHARE
    asks for 0.9 of them.  (In the rest no friction edge carries load: they move by 1e-14 or less.)"""
    k = P.kept_conditions(asset)
    cube = P.has_rows(asset)[1]
    d = P.distance(P.pgs(asset, friction_scale=1.01), P.reference(asset))[k & cube]
    print("\n%s: %d kept envs with a cube contact, %d moved by more than %.0e (smallest move %.1e, median %.1e)" % (
        asset, len(d), int((d > BLIND).sum()), BLIND, d.min(), np.median(d)))
    assert len(d) >= 20 and (d > BLIND).sum() >= SEEN_SHARE * len(d), (len(d), int((d > BLIND).sum()))


# ------------------------------------------------------------------------------------------------- the oracle's applied-force step
@pytest.mark.parametrize("solver", ["newton", "pgs"])
@pytest.mark.parametrize("asset", ASSETS)
def test_a_zero_applied_force_is_the_oracles_own_step(asset, solver):
    """Oracle.physics_step_applied, which the forced build's reference and kept set come from, with a force of zeros on the ctrl
    the oracle's own control step stored: qpos, qvel, done byte, contact mask and sweep count of every cell are the bits of that
    step (the shipped cap and tolerance, both solvers)."""
    cm = capped_model(asset, solver, 100, 1e-8)
    got = P._forced_run(cm, asset, False, tau=np.zeros((len(R.cells(asset)[3]), cm.nv)))
    want = control_steps(asset, solver, 100, 1e-8)[0]
    for key in ("qpos", "qvel", "done", "mask", "iters"):
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("asset,solver", [("solo_arm", "newton"), ("solo_arm", "pgs"), ("dual_arm", "pgs")])
def test_the_oracles_applied_force_step_is_the_restatement(asset, solver):
    """The same call under the test forces against tests/tools/applied_oracle.py, the NumPy restatement the applied-force tests hold
    the device to (applied_oracle.cell_runs: the shipped cap and tolerance): contact masks equal, qpos / qvel within TOL_Q / TOL_V
    with ten times the restatement's own spread under the bars.  The two add the force in different places (to the right-hand side
    before M^-1 here and on the device, M^-1 tau to qacc_smooth there) and PGS at 100 sweeps is unconverged, so roundoff is what is
    left: measured worst qvel 5.0e-13, qpos 1.5e-15, the size of the restatement's own spread (4.2e-13, 1.3e-15)."""
    run = AO.cell_runs(asset, solver)
    cm = capped_model(asset, solver, 100, 1e-8)
    assert bytes(cm.desc) == bytes(run["cm"].desc)
    got = P._forced_run(cm, asset, False, tau=run["tau"])
    assert np.array_equal(got["mask"], run["ref"]["mask"]) and np.array_equal(got["done"], run["ref"]["done"])
    for key, bar in (("qpos", TOL_Q), ("qvel", TOL_V)):
        d, sp = P.distance(got, run["ref"], key), P.distance(run["twin"], run["ref"], key)
        print("\n%s %s %s: worst |oracle - restatement| %.1e (the restatement's own spread %.1e)" % (asset, solver, key, d.max(), sp.max()))
        assert 10.0 * sp.max() <= bar and (d < bar).all(), (key, float(d.max()), float(sp.max()))
