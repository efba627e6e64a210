"""The reference of kmanip_inverse (tests/tools/inverse_oracle.py) on the CPU, and the bars of tests/test_inverse_gpu.py.

The reference is NumPy over the unchanged oracle: qfrc_inverse = M a + bias - J^T f(a) with the row forces of applied_oracle._rows.
Here, on every regime cell of tests/tools/regime_states.py for the three assets (47 / 72 / 72 states) and the eleven test
accelerations of a cell (the forward solution a*, zero, a* + s z for s in {1, 30, 1000}, three draws each):
  * the accelerations visit every branch of every row type (friction loss saturated low / quadratic / saturated high, one-sided rows
    active / inactive) on each asset -- asserted, so that a changed recipe cannot silently lose a branch;
  * the forward/inverse identity inverse(a*) = M a_smooth + bias holds to the exact forward solve's convergence;
  * the round trip: the forward problem under tau = qfrc_inverse(a) - pad(qfrc_actuator) returns a;
  * the reference's own error -- its spread under qvel * (1 + 1e-15) -- per quantity.
The bars of the device tests are 1000 x these figures, rounded up to one digit (the rule of DESIGN.md section 19: the margin is the one
the step shows between the two formulations), measured here and committed as constants; none comes from the device's numbers."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import inverse_oracle as IO  # noqa: E402
import mujoco_pin  # noqa: E402

ASSETS = mujoco_pin.ASSETS

# the reference's worst spread over all cells x test accelerations of the three assets, each difference normalised per env and
# acceleration by inverse_oracle.scales: qfrc_inverse by max(1, max|qfrc_inverse|); qfrc_constraint and the contact forces by
# max(1, max|qfrc_constraint|)
SPREAD_QFRC_INVERSE = 2.78e-11
SPREAD_QFRC_CONSTRAINT = 1.16e-11
SPREAD_CONTACT_FORCE = 6.99e-12
# the forward/inverse identity on the reference: max|inverse(a*) - (M a_smooth + bias)| over max(1, max|qfrc_actuator|, max|M a* + bias|)
FWDINV_MEASURED = 8.23e-13
# the round trip on the reference: max|accel(tau = from_inverse(a)) - a| over max(1, max|a|), a = a* + s z, per s in ROUND_TRIP_SCALES.
# At s = 30 the figure is the reference solver's: applied_oracle.newton_exact stops when the cost no longer decreases, and under
# forces of that size the cost's rounding hides the last digits of the minimiser.  One bar per scale, so that the s = 1 bar is not
# widened by it.
ROUND_TRIP_SCALES = (1.0, 30.0)
ROUNDTRIP_MEASURED = {1.0: 2.55e-13, 30.0: 2.68e-5}
# BAR_* = 1000 x the figure, rounded up to one digit
BAR_QFRC_INVERSE = 3e-8
BAR_QFRC_CONSTRAINT = 2e-8
BAR_CONTACT_FORCE = 7e-9
BAR_FWDINV = 9e-10
BAR_ROUNDTRIP = {1.0: 3e-10, 30.0: 3e-2}
# the thinnest branch of the coverage condition must keep at least this many hits per asset
MIN_BRANCH_HITS = 20
BRANCHES = ("friction loss low", "friction loss quadratic", "friction loss high", "one-sided active", "one-sided inactive")


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def fwdinv_scale(cm, dyn, a_star):
    """The normaliser of the forward/inverse residual of one state: max(1, max|qfrc_actuator|, max|M a* + bias|)."""
    fa = (dyn["M"] @ dyn["qacc_smooth"] + dyn["bias"])[:cm.nlink]
    return max(1.0, float(np.abs(fa).max()), float(np.abs(dyn["M"] @ a_star + dyn["bias"]).max()))


def round_trip_indices(s):
    """Indices into a cell's test accelerations of the draws a* + s z."""
    return [2 + IO.SCALES.index(s) * IO.DRAWS + k for k in range(IO.DRAWS)]


@pytest.mark.parametrize("asset", ASSETS)
def test_the_test_accelerations_visit_every_branch_of_every_row_type(asset):
    c = IO.cell_inverses(asset)
    counts = sum(IO.branches(o) for per_cell in c["ref"] for o in per_cell)
    print("\n%s: %d states x %d accelerations; rows per branch: %s" % (asset, len(c["labels"]), IO.N_ACCELS,
                                                                        "  ".join("%s %d" % kv for kv in zip(BRANCHES, counts))))
    assert c["qacc"].shape == (len(c["labels"]), IO.N_ACCELS, c["cm"].nv) and IO.N_ACCELS == 11
    assert len(c["labels"]) == (47 if asset == "solo_arm" else 72)
    assert (counts >= MIN_BRANCH_HITS).all(), dict(zip(BRANCHES, counts))


@pytest.mark.parametrize("asset", ASSETS)
def test_forward_inverse_identity_on_the_reference(asset):
    """inverse(a*) = M a_smooth + bias = pad(qfrc_actuator): the constraint force at the minimiser is M (a* - a_smooth)."""
    c = IO.cell_inverses(asset)
    cm = c["cm"]
    worst = 0.0
    for e, per_cell in enumerate(c["ref"]):
        dyn = c["rows"][e][0]
        want = dyn["M"] @ c["a_smooth"][e] + dyn["bias"]
        assert not want[cm.nlink:].any() or np.abs(want[cm.nlink:]).max() < 1e-9          # (no actuator on the cube)
        res = float(np.abs(per_cell[0]["qfrc_inverse"] - want).max()) / fwdinv_scale(cm, dyn, c["a_star"][e])
        worst = max(worst, res)
        assert 1000.0 * res <= BAR_FWDINV, (asset, c["labels"][e], e, res)
    print("\n%s: inverse(a*) vs M a_smooth + bias, worst over %d states: %.1e" % (asset, len(c["ref"]), worst))


_ROUND_TRIPS = {}


def reference_round_trips(asset):
    """{s: (worst error, label, env, k)} of the asset's cells: the forward problem (applied_oracle.accel) under
    tau = qfrc_inverse(a) - pad(qfrc_actuator) against a = a* + s z, normalised by max(1, max|a|).  Computed once."""
    from oracle.oracle import Oracle
    if asset not in _ROUND_TRIPS:
        c = IO.cell_inverses(asset)
        cm = c["cm"]
        orc = Oracle(cm, 1)
        worst = {s: (0.0, None, -1, -1) for s in ROUND_TRIP_SCALES}
        for e, per_cell in enumerate(c["ref"]):
            dyn = c["rows"][e][0]
            pad = np.zeros(cm.nv)
            pad[:cm.nlink] = (dyn["M"] @ dyn["qacc_smooth"] + dyn["bias"])[:cm.nlink]
            for s in ROUND_TRIP_SCALES:
                for k in round_trip_indices(s):
                    a = c["qacc"][e, k]
                    got = AO.accel(cm, orc, c["qpos"][e], c["qvel"][e], c["ctrl"][e], np.zeros(cm.nv), per_cell[k]["qfrc_inverse"] - pad)[0]
                    res = float(np.abs(got - a).max()) / max(1.0, float(np.abs(a).max()))
                    if res >= worst[s][0]:
                        worst[s] = (res, c["labels"][e], e, k)
        _ROUND_TRIPS[asset] = worst
    return _ROUND_TRIPS[asset]


@pytest.mark.parametrize("asset", ASSETS)
def test_round_trip_on_the_reference(asset):
    """The forward problem under tau = qfrc_inverse(a) - pad(qfrc_actuator) has the minimiser a."""
    worst = reference_round_trips(asset)
    print("\n%s: round trip, worst per scale: %s" % (asset, "  ".join("s=%g %.2e (%s, env %d, k %d)" % ((s,) + worst[s]) for s in ROUND_TRIP_SCALES)))
    for s in ROUND_TRIP_SCALES:
        assert 1000.0 * worst[s][0] <= BAR_ROUNDTRIP[s], (asset, s, worst[s])


def test_bars_are_a_thousand_times_the_references_own_figures():
    worst = np.zeros(3)
    fwdinv = 0.0
    roundtrip = {s: 0.0 for s in ROUND_TRIP_SCALES}
    for asset in ASSETS:
        c = IO.cell_inverses(asset)
        cm = c["cm"]
        for e, (per_cell, per_twin) in enumerate(zip(c["ref"], c["twin"])):
            for o, t in zip(per_cell, per_twin):
                worst = np.maximum(worst, IO.spreads(o, t))
            dyn = c["rows"][e][0]
            want = dyn["M"] @ c["a_smooth"][e] + dyn["bias"]
            fwdinv = max(fwdinv, float(np.abs(per_cell[0]["qfrc_inverse"] - want).max()) / fwdinv_scale(cm, dyn, c["a_star"][e]))
        for s in ROUND_TRIP_SCALES:
            roundtrip[s] = max(roundtrip[s], reference_round_trips(asset)[s][0])
    print("\nspreads under qvel (1 + 1e-15): qfrc_inverse %.2e  qfrc_constraint %.2e  contact force %.2e;  forward/inverse %.2e;  round trip %s"
          % (tuple(worst) + (fwdinv, "  ".join("s=%g %.2e" % (s, roundtrip[s]) for s in ROUND_TRIP_SCALES))))
    names = ("qfrc_inverse", "qfrc_constraint", "contact_force", "fwdinv") + tuple("roundtrip s=%g" % s for s in ROUND_TRIP_SCALES)
    measured = tuple(worst) + (fwdinv,) + tuple(roundtrip[s] for s in ROUND_TRIP_SCALES)
    recorded = (SPREAD_QFRC_INVERSE, SPREAD_QFRC_CONSTRAINT, SPREAD_CONTACT_FORCE, FWDINV_MEASURED) + tuple(ROUNDTRIP_MEASURED[s] for s in ROUND_TRIP_SCALES)
    bars = (BAR_QFRC_INVERSE, BAR_QFRC_CONSTRAINT, BAR_CONTACT_FORCE, BAR_FWDINV) + tuple(BAR_ROUNDTRIP[s] for s in ROUND_TRIP_SCALES)
    for name, s, rec, bar in zip(names, measured, recorded, bars):
        assert 1000.0 * s <= bar, (name, s, bar)                        # the bar cannot drift below its source ...
        assert bar == pytest.approx(_round_up_one_digit(1000.0 * rec), rel=1e-12), (name, rec, bar)
        # ... nor the recorded figure far above what is measured (the round trips are a solver's stopping point, not rounding: looser)
        assert s > (0.1 if name.startswith("roundtrip") else 0.5) * rec, (name, s, rec)


def test_from_inverse_and_fwdinv_residual_on_numpy_backed_tensors():
    import torch
    from gym_kmanip_amd import applied
    rng = np.random.default_rng(3)
    n, nv, nu = 5, 16, 10
    # (multiples of 2^-10: every sum and difference below is exact)
    qi, fa, tau = (np.round(rng.standard_normal(shape) * 1024.0) / 1024.0 for shape in ((n, nv), (n, nu), (n, nv)))
    inv, f = {"qfrc_inverse": torch.from_numpy(qi)}, {"qfrc_actuator": torch.from_numpy(fa), "qacc": torch.zeros((n, nv), dtype=torch.float64)}
    pad = np.concatenate([fa, np.zeros((n, nv - nu))], axis=1)
    rows = applied.from_inverse(inv, f)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (n, nv) and rows.is_contiguous()
    assert np.array_equal(rows.numpy(), qi - pad)
    assert np.array_equal(inv["qfrc_inverse"].numpy(), qi)                        # a new tensor: the inputs are not written
    assert np.array_equal(applied.fwdinv_residual(f, inv).numpy(), np.abs(qi - pad).max(axis=1))
    assert np.array_equal(applied.fwdinv_residual(f, inv, torch.from_numpy(tau)).numpy(), np.abs(qi - pad - tau).max(axis=1))
    exact = {"qfrc_inverse": torch.from_numpy(pad + tau)}
    assert not applied.fwdinv_residual(f, exact, torch.from_numpy(tau)).any()


def test_kinverse_bindings_match_the_header():
    """lib.KInverseIn / lib.KInverseDev list the header's fields in the header's order (all pointers); the library exports the entry point."""
    import re
    from gym_kmanip_amd import lib as klib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kmanip.h")).read()
    for name, cls, count in (("KInverseIn", klib.KInverseIn, 3), ("KInverseDev", klib.KInverseDev, 6)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"\*\s*(\w+)\s*;", body)
        assert fields == [n for n, _ in cls._fields_] and len(fields) == count, name
    assert "kmanip_inverse" in klib.EXPORTS
    if not os.path.exists(klib.LIB_PATH):
        klib.build()
    L = klib.load()
    assert [a.__name__ for a in L.kmanip_inverse.argtypes] == ["c_void_p", "LP_KInverseIn", "LP_KInverseDev", "c_void_p"]


def test_shipped_inverse_kernels_run_without_scratch():
    """k_inverse / k_inverse_ep of the built library (parsed from the .so: no GPU): four variants, none spills, the LDS of their
    k_forces siblings at most."""
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    if not os.path.exists(klib.LIB_PATH):
        klib.build()
    rows = BM.kernels(klib.LIB_PATH, r"k_inverse\w*")
    assert sorted((r.base,) + r.args for r in rows) == [("k_inverse", 10, 16, 4), ("k_inverse", 20, 32, 2),
                                                        ("k_inverse_ep", 10, 16, 4), ("k_inverse_ep", 20, 32, 2)]
    for r in rows:
        print("%s<%s,%s,%s> vgpr %s scratch %s lds %s" % ((r.base,) + r.args + (r.vgpr, r.scratch, r.lds)))
        assert r.scratch == 0 and r.vgpr <= 512 and r.lds <= 40 * 1024, r
