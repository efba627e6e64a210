"""The force oracle of kmanip_forces (tests/tools/force_oracle.py) on the CPU, and the bars of tests/test_forces_gpu.py.

The oracle's contact forces are the mj_contactForce decode of its own constraint rows; here they are checked against the one
identity they must satisfy -- J^T f over all rows = M (qacc - qacc_smooth) -- and against the friction pyramid, on every regime cell
of tests/tools/regime_states.py for the three assets (47 / 72 / 72 states: normal forces up to 51 N, up to 8 contacts at once), and
again on a model with per-env parameters.  The bars of the device parity are 1000 x the oracle's own spread under qvel * (1 + 1e-15),
measured here per quantity and committed as constants; the margin is the one the step shows between the two formulations (qpos
differs by 1.0e-12 against a spread of 3.3e-15: DESIGN.md section 17)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import force_oracle as FO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402

ASSETS = mujoco_pin.ASSETS

# the oracle's worst spread over all cells of the three assets, each difference normalised per env by force_oracle.scales:
# qacc by max(1, max|qacc|); qfrc_constraint and the contact forces by max(1, max|qfrc_constraint|); qfrc_actuator by the larger of
# its own maximum and the largest arm bias force (scales' docstring: why "its own maximum" alone cannot be used)
SPREAD_QACC = 1.76e-14
SPREAD_QFRC_CONSTRAINT = 3.25e-14
SPREAD_CONTACT_FORCE = 1.45e-12
SPREAD_QFRC_ACTUATOR = 9.3e-16
# BAR_* = 1000 x the spread, rounded up to one digit
BAR_QACC = 2e-11
BAR_QFRC_CONSTRAINT = 4e-11
BAR_CONTACT_FORCE = 2e-9
BAR_QFRC_ACTUATOR = 1e-12
# contact geometry (point, frame, distance) is forward kinematics and a box test in metres and unit vectors of size <= 1: a chain of
# ten frames at 2.2e-16 per operation stays below 1e-13; 1e-12 leaves the two evaluation orders room
BAR_GEOMETRY = 1e-12
# the identity J^T f = M (qacc - qacc_smooth) on the oracle itself holds to its solver's convergence: 9.1e-13 measured over the cells
# (9.9e-12 on the model with parameters), relative to max(1, max|qfrc_constraint|), against the contact-force bar
IDENTITY_MEASURED = 9.1e-13


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def _check_state(o, what):
    """identity and friction pyramid of one decode; returns the identity's residual."""
    sf = FO.scales(o)[1]
    res = float(np.abs(o["jtf"] - o["qfrc_constraint"]).max()) / sf
    assert res <= BAR_CONTACT_FORCE, (what, res)
    assert set(o["contacts"]) == set(FO.mask_bits(o["mask"])), what
    for b, c in o["contacts"].items():
        F = c["force"]
        slack = 1.0 + 1e-12
        assert F[0] >= 0, (what, b, F)
        assert abs(F[1]) <= c["mu"] * F[0] * slack and abs(F[2]) <= c["mu"] * F[0] * slack, (what, b, F)
        assert abs(F[3]) <= c["mu3"] * F[0] * slack, (what, b, F)
        if b >= 20:
            assert F[3] == 0 and c["normal"] is None
        else:                                                # the restated geometry agrees with the rows the oracle built
            assert np.abs(c["normal"] - c["frame"][:3]).max() < BAR_GEOMETRY, (what, b)
            assert np.abs(c["tangent1"] - c["frame"][3:6]).max() < BAR_GEOMETRY, (what, b)
    return res


@pytest.mark.parametrize("asset", ASSETS)
def test_oracle_forces_satisfy_the_identity_and_the_pyramid(asset):
    cm, dec, _ = FO.cell_decodes(asset)
    labels = R.cells(asset)[3]
    worst = max(_check_state(o, (asset, labels[e], e)) for e, o in enumerate(dec))
    print("\n%s: J^T f vs M (qacc - qacc_smooth), worst over %d states: %.1e" % (asset, len(dec), worst))
    free = [e for e, o in enumerate(dec) if o["mask"] == 0]
    assert free and all(dec[e]["contacts"] == {} for e in free)           # a state without contacts: an empty dict
    assert max(len(o["contacts"]) for o in dec) >= (7 if cm.nlink == 10 else 8)
    assert max(c["force"][0] for o in dec for c in o["contacts"].values()) > 30.0


@pytest.mark.parametrize("asset", ASSETS)
def test_oracle_forces_with_env_params(asset):
    """The same on a with_env_params model: cube mass x 2, friction 0.5, friction loss 0."""
    from gym_kmanip_amd.model import with_env_params
    from oracle.oracle import Oracle
    cm = R.model(asset)
    cmp_ = with_env_params(cm, cube_mass=2.0 * cm.desc.cube_mass, cube_friction=0.5, cube_frictionloss=0.0)
    orc = Oracle(cmp_, 1)
    qpos, qvel, ctrl, labels = R.cells(asset)
    worst = 0.0
    for e in range(len(labels)):
        o = FO.decode(cmp_, orc, qpos[e], qvel[e], ctrl[e])
        worst = max(worst, _check_state(o, (asset, labels[e], e)))
        assert all(c["mu"] == (0.5 if b < 20 else cm.desc.con_def_friction[0]) for b, c in o["contacts"].items())
    print("\n%s with parameters: identity %.1e" % (asset, worst))


def test_bars_are_a_thousand_times_the_oracles_spread():
    worst = np.zeros(4)
    for asset in ASSETS:
        _, dec, tw = FO.cell_decodes(asset)
        for o, t in zip(dec, tw):
            worst = np.maximum(worst, FO.spreads(o, t))
    print("\nspreads under qvel (1 + 1e-15): qacc %.2e  qfrc_constraint %.2e  contact force %.2e  qfrc_actuator %.2e" % tuple(worst))
    recorded = (SPREAD_QACC, SPREAD_QFRC_CONSTRAINT, SPREAD_CONTACT_FORCE, SPREAD_QFRC_ACTUATOR)
    bars = (BAR_QACC, BAR_QFRC_CONSTRAINT, BAR_CONTACT_FORCE, BAR_QFRC_ACTUATOR)
    for name, s, rec, bar in zip(("qacc", "qfrc_constraint", "contact_force", "qfrc_actuator"), worst, recorded, bars):
        assert 1000.0 * s <= bar, (name, s, bar)                        # the bar cannot drift below its source ...
        assert bar == pytest.approx(_round_up_one_digit(1000.0 * rec), rel=1e-12), (name, rec, bar)
        assert s > 0.5 * rec, (name, s, rec)                              # ... nor the recorded spread far above what is measured


def test_kforcesdev_binding_matches_the_header():
    """lib.KForcesDev lists the header's fields in the header's order (all pointers), and model.contact_slots is KM_CONTACT_SLOTS."""
    import re
    from gym_kmanip_amd import lib as klib
    from gym_kmanip_amd.model import contact_slots
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kmanip.h")).read()
    body = re.search(r"typedef struct KForcesDev \{(.*?)\} KForcesDev;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert fields == [n for n, _ in klib.KForcesDev._fields_] and len(fields) == 10
    assert "#define KM_CONTACT_SLOTS(nlink) (4 + KM_SPHERE_SLOTS(nlink) + KM_SPHERE_TABLE_SLOTS(nlink))" in hdr
    assert (contact_slots(10), contact_slots(20)) == (8, 14)


def test_shipped_forces_kernels_run_without_scratch():
    """k_forces / k_forces_ep of the built library (parsed from the .so: no GPU): four variants, none spills, the LDS of their
    k_step siblings."""
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, r"k_forces\w*")
    assert sorted((r.base,) + r.args for r in rows) == [("k_forces", 10, 16, 4), ("k_forces", 20, 32, 2),
                                                        ("k_forces_ep", 10, 16, 4), ("k_forces_ep", 20, 32, 2)]
    for r in rows:
        assert r.scratch == 0 and r.vgpr <= 512 and r.lds <= 40 * 1024, r
