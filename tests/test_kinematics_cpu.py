"""The kinematics oracle of kmanip_kinematics (tests/tools/kin_oracle.py) on the CPU, and the bars of tests/test_kinematics_gpu.py.

The oracle's Jacobians are geometric, built from Oracle.fk; here they are pinned three ways on every regime cell of
tests/tools/regime_states.py for the three assets (47 / 72 / 72 states, qvel up to 28 rad/s): against Oracle.ik_jac on the IK's own
columns, against central differences of Oracle.fk on all nlink columns, and by the zero pattern.  M and bias are Oracle.dynamics';
they are checked by symmetry, definiteness, the cube block and the identity M qacc + bias = qfrc_actuator + qfrc_constraint with the
force oracle's numbers.  The device bars of M and bias are 1000 x the oracle's own spread under (1 + 1e-15) on joint positions and
qvel (the rule of DESIGN.md section 19), measured here and committed as constants; geometry is held to test_forces_cpu.BAR_GEOMETRY.
Last, the resolved-rate loop of examples/resolved_rate_reach.py on Oracle.step."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import force_oracle as FO  # noqa: E402
import kin_oracle as KO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_forces_cpu import BAR_GEOMETRY  # noqa: E402

ASSETS = mujoco_pin.ASSETS

# the oracle's worst spread over all cells of the three assets under (1 + 1e-15) on the joint positions and qvel, per env normalised
# by max(1, max|M|) and max(1, max|bias|)
SPREAD_QM = 2.0e-15
SPREAD_QFRC_BIAS = 5.6e-15
# BAR_* = 1000 x the spread, rounded up to one digit, never below 1e-12
BAR_QM = 2e-12
BAR_QFRC_BIAS = 6e-12
# jacp against Oracle.ik_jac: the same formula evaluated twice (3.3e-16 measured)
BAR_IK_JAC = 1e-12
# central differences with h = 1e-6: truncation ~ h^2 |d3| / 6 ~ 1e-12, round-off ~ eps / h = 2e-10 (5.3e-10 measured)
FD_H = 1e-6
BAR_FD = 1e-8
# M qacc + bias = pad(qfrc_actuator) + qfrc_constraint on the oracle's own numbers (1.1e-15 measured)
BAR_IDENTITY = 1e-12


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def _cells(asset):
    cm, dec, tw = KO.cell_decodes(asset)
    qpos, qvel, ctrl, labels = R.cells(asset)
    return cm, dec, tw, qpos, qvel, ctrl, labels


@pytest.mark.parametrize("asset", ASSETS)
def test_jacp_is_the_ik_jacobian_on_the_ik_columns(asset):
    from oracle.oracle import Oracle
    cm, dec, _, qpos, _, _, labels = _cells(asset)
    d = cm.desc
    orc = Oracle(cm, 1)
    worst = 0.0
    for e, o in enumerate(dec):
        for a in range(2):
            if not d.arm_present[a]:
                continue
            ids = R.arm_joints(cm, a)
            J = orc.ik_jac(a, qpos[e], qpos[e][ids], qpos[e], o["site_xpos"][a], R.mat2quat(o["site_xmat"][a].reshape(3, 3)))
            worst = max(worst, float(np.abs(J[:3] - o["site_jacp"][a][:, ids]).max()))
    print("\n%s: jacp vs Oracle.ik_jac, worst over %d states: %.1e" % (asset, len(dec), worst))
    assert worst <= BAR_IK_JAC


def _rotvec(Rm):
    """Rotation vector of a rotation by a small angle (here 2e-6 rad: sin t / t = 1 to 1e-12)."""
    return 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])


@pytest.mark.parametrize("asset", ASSETS)
def test_jacobians_against_central_differences_of_fk(asset):
    from oracle.oracle import Oracle
    cm, dec, _, qpos, _, _, labels = _cells(asset)
    d = cm.desc
    orc = Oracle(cm, 1)
    worst = 0.0
    for e, o in enumerate(dec):
        for j in range(cm.nlink):
            qa, qb = qpos[e].copy(), qpos[e].copy()
            qa[j] += FD_H; qb[j] -= FD_H
            _, _, spa, sma = orc.fk(qa)
            _, _, spb, smb = orc.fk(qb)
            for a in range(2):
                if not d.arm_present[a]:
                    continue
                dp = (spa[a] - spb[a]) / (2 * FD_H)
                dr = _rotvec(sma[a] @ smb[a].T) / (2 * FD_H)
                worst = max(worst, float(np.abs(dp - o["site_jacp"][a][:, j]).max()), float(np.abs(dr - o["site_jacr"][a][:, j]).max()))
    print("\n%s: jacp / jacr vs central differences of fk (h = %g), worst over %d states x %d columns: %.1e"
          % (asset, FD_H, len(dec), cm.nlink, worst))
    assert worst <= BAR_FD


@pytest.mark.parametrize("asset", ASSETS)
def test_zero_pattern_of_the_jacobians(asset):
    cm, dec, _, _, _, _, _ = _cells(asset)
    d = cm.desc
    nl = cm.nlink
    for a in range(2):
        if not d.arm_present[a]:
            assert all(not o[k][a].any() for o in dec for k in ("site_xpos", "site_xmat", "site_jacp", "site_jacr", "site_vel"))
            continue
        chain = KO.site_chain(cm, a)
        off = [j for j in range(cm.nv) if j not in chain]
        assert set(range(nl, cm.nv)) <= set(off)
        for o in dec:
            assert (o["site_jacp"][a][:, off] == 0).all() and (o["site_jacr"][a][:, off] == 0).all()
            assert all(o["site_jacp"][a][:, j].any() or o["site_jacr"][a][:, j].any() for j in chain)
        outside = [j for j in chain if j not in R.arm_joints(cm, a)]       # (the Torso: the hand joint that carries the site)
        for j in outside:
            assert all(o["site_jacp"][a][:, j].any() or o["site_jacr"][a][:, j].any() for o in dec), (asset, a, j)
        print("\n%s arm %d: site chain %s, outside arm_q_id %s" % (asset, a, chain, outside))


@pytest.mark.parametrize("asset", ASSETS)
def test_inertia_is_symmetric_positive_with_the_cubes_block(asset):
    cm, dec, _, _, _, _, _ = _cells(asset)
    d = cm.desc
    nl = cm.nlink
    cube = np.diag([d.cube_mass] * 3 + list(d.cube_inertia))
    blocks = R.blocks(cm)
    for o in dec:
        M = o["qM"]
        assert np.array_equal(M, M.T)
        assert np.linalg.eigvalsh(M).min() > 0
        assert np.array_equal(M[nl:, nl:], cube) and not M[:nl, nl:].any()
        if len(blocks) == 2:
            s = blocks[1][0]
            assert not M[:s, s:nl].any()


@pytest.mark.parametrize("asset", ASSETS)
def test_equation_of_motion_with_the_force_oracle(asset):
    """M qacc + bias = pad(qfrc_actuator) + qfrc_constraint, the force oracle's qacc and forces with this oracle's M and bias."""
    cm, dec, _, _, _, _, labels = _cells(asset)
    _, fdec, _ = FO.cell_decodes(asset)
    nl = cm.nlink
    worst = 0.0
    for e, (o, f) in enumerate(zip(dec, fdec)):
        mq = o["qM"] @ f["qacc"]
        rhs = f["qfrc_constraint"].copy()
        rhs[:nl] += f["qfrc_actuator"]
        r = float(np.abs(mq + o["qfrc_bias"] - rhs).max()) / max(1.0, float(np.abs(f["qfrc_constraint"]).max()), float(np.abs(mq).max()))
        worst = max(worst, r)
        assert r <= BAR_IDENTITY, (asset, labels[e], e, r)
    print("\n%s: M qacc + bias - (qfrc_actuator + qfrc_constraint), worst over %d states: %.1e" % (asset, len(dec), worst))


def test_bars_are_a_thousand_times_the_oracles_spread():
    worst = np.zeros(2)
    for asset in ASSETS:
        cm, dec, tw, qpos, qvel, _, _ = _cells(asset)
        for e, (o, t) in enumerate(zip(dec, tw)):
            _, sm, sb = KO.scales(o, qvel[e])
            worst = np.maximum(worst, (np.abs(o["qM"] - t["qM"]).max() / sm, np.abs(o["qfrc_bias"] - t["qfrc_bias"]).max() / sb))
    print("\nspreads under (1 + 1e-15) on joint positions and qvel: qM %.2e  qfrc_bias %.2e" % tuple(worst))
    for name, s, rec, bar in (("qM", worst[0], SPREAD_QM, BAR_QM), ("qfrc_bias", worst[1], SPREAD_QFRC_BIAS, BAR_QFRC_BIAS)):
        assert 1000.0 * s <= bar, (name, s, bar)                          # the exported bar is at least 1000 x what is measured
        assert bar == pytest.approx(max(1e-12, _round_up_one_digit(1000.0 * rec)), rel=1e-12), (name, rec, bar)
        assert s > 0.5 * rec, (name, s, rec)                              # ... and the recorded spread not far above it


@pytest.mark.parametrize("env_id", ["KManipSoloArmQPos", "KManipDualArmQPos"])
def test_resolved_rate_reach_on_the_oracle(env_id):
    """The loop of gym_kmanip_amd/examples/resolved_rate_reach.py with the oracle's own Jacobians on Oracle.step: 4 envs, seed 3,
    24 steps; the median site-to-goal distance falls below 0.6 x its start (0.23 x / 0.18 x measured)."""
    from gym_kmanip_amd.model import compile_model
    from oracle.oracle import Oracle
    cm = compile_model(env_id)
    n = 4
    orc, one = Oracle(cm, n, seed=3), Oracle(cm, 1)
    orc.reset()

    def geo():
        qpos = orc.get_state()[0]
        g = [KO.geometry(cm, one, qpos[e]) for e in range(n)]
        return np.stack([x["site_xpos"] for x in g]), np.stack([x["site_jacp"] for x in g])
    sx, jp = geo()
    goal = KO.reach_goals(cm, sx, 3)
    start = KO.median_distance(cm, sx, goal)
    for _ in range(24):
        _, _, done = orc.step(KO.resolved_rate_action(cm, sx, jp, goal))
        assert not done.any()
        sx, jp = geo()
    end = KO.median_distance(cm, sx, goal)
    print("\n%s: median site-to-goal distance %.4f -> %.4f m (%.2f x)" % (env_id, start, end, end / start))
    assert end < 0.6 * start


def test_kkindev_binding_matches_the_header():
    """lib.KKinDev lists the header's fields in the header's order (all pointers); env_hip knows the same names."""
    import re
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kmanip.h")).read()
    body = re.search(r"typedef struct KKinDev \{(.*?)\} KKinDev;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert fields == [n for n, _ in klib.KKinDev._fields_] and len(fields) == 10
    assert list(env_hip.KManipEnvHip._KIN_FIELDS) == fields and fields[:-1] == list(KO.FIELDS)


def test_shipped_kinematics_kernels_run_without_scratch():
    """k_kinematics / k_kinematics_ep of the built library (parsed from the .so: no GPU): four variants, none spills, the LDS of
    their k_step siblings."""
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, r"k_kinematics\w*")
    assert sorted((r.base,) + r.args for r in rows) == [("k_kinematics", 10, 16, 4), ("k_kinematics", 20, 32, 2),
                                                        ("k_kinematics_ep", 10, 16, 4), ("k_kinematics_ep", 20, 32, 2)]
    for r in rows:
        assert r.scratch == 0 and r.vgpr <= 512 and r.lds <= 40 * 1024, r
