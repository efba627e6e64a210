"""The oracle's M and bias on models with ANISOTROPIC link and cube inertias, against the Lagrange equations (no GPU).

Every shipped asset is isotropic, so R diag(I) R^T = I 1 and w x I w = 0 in every other test: a transposed rotation, a principal
value used twice or a gyroscopic term with the wrong sign, frame or none at all would move nothing.  Here every link of the three
assets has three different principal values (tests/tools/aniso_model.py: the shipped value x a seeded permutation of 0.6, 1.0, 1.5,
never the same permutation on two consecutive links) and the cube (0.001, 0.002, 0.0028).  The reference is
tests/tools/lagrange_oracle.py: M from geometric centre-of-mass Jacobians and the bias from the Lagrange equations with
Richardson-extrapolated central differences of M -- it takes Oracle.fk and nothing else of the oracle, no CRBA, no RNE.

States: 16 per asset from aniso_model.random_states (seed 11; hinges within 0.4 rad of home, 0.5 .. 2.5 rad/s or m/s of either sign on
every dof, the cube's angular velocity included) and every regime cell of tests/tools/regime_states.py (47 / 72 / 72).

Bars.  M: 1e-12 max(1, max|M|).  Bias: per state, 10 x the reference's own step-halving estimate |bias(h) - bias(h/2)| (h = 1e-4),
never below the bar the project already holds a device bias to against its own oracle (test_kinematics_cpu.BAR_QFRC_BIAS x
max(1, max|bias|)): where qvel is almost zero the estimate vanishes with the velocity products while rounding does not.
Measured over the cells and the random states (solo_arm / dual_arm / torso):
    step-halving estimate, largest                 3.9e-09 / 3.8e-09 / 3.5e-09
    bias bar, largest                              3.9e-08 / 3.8e-08 / 3.5e-08
    |oracle - Lagrange| M, worst                   1.3e-15 / 1.7e-15 / 1.2e-15   (x max(1, max|M|))
    |oracle - Lagrange| bias, worst                2.1e-11 / 3.9e-11 / 2.2e-11   (absolute; bias scale 3 .. 8)
    ... as a fraction of the state's bar, worst    9.1e-03 / 2.8e-03 / 1.2e-03
    isotropic -> anisotropic moves the bias by     0.34 / 0.25 / 0.28
Sensitivity controls, computed in the reference alone (it is linear in the principal values, so one evaluation serves every
assignment), on every random state: swapping ANY two principal values of ANY link moves the reference's M or bias by at least
1000 x the bar (smallest measured: 5.8e6 / 5.4e6 / 5.4e6 bars; the bias alone, in every pair's best state: 1.2e4 / 7.0e3 / 6.3e3),
and so does negating the cube's w x I w (smallest: 2.2e5 / 7.4e4 / 1.1e5 bars).
One kind of pair is different, by construction and not by measurement: the first two principal values of a link whose parent
is the fixed base and whose joint is a hinge about its own z -- such a link only ever turns about its third axis, so those two
values enter neither M nor the bias of any state, on the device no more than in the reference.  Those pairs (one per root link: 1, 2
and 3 of them) are not skipped: the test asserts that the swap moves the reference by exactly nothing."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import aniso_model as AM  # noqa: E402
import force_oracle as FO  # noqa: E402
import lagrange_oracle as LO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_kinematics_cpu import BAR_IDENTITY, BAR_QFRC_BIAS  # noqa: E402

ASSETS = mujoco_pin.ASSETS
N_RANDOM = 16
SEED = 11
BAR_M = 1e-12                    # x max(1, max|M|)
SENSITIVITY = 1000.0             # a control must move the reference by this many bars
PAIRS = ((0, 1), (0, 2), (1, 2))


def bias_bar(ref):
    """The bias bar of one state (absolute): 10 x the reference's step-halving estimate, floored at BAR_QFRC_BIAS max(1, max|bias|)."""
    return max(10.0 * ref["err"], BAR_QFRC_BIAS * max(1.0, float(np.abs(ref["bias"]).max())))


def m_bar(ref):
    return BAR_M * max(1.0, float(np.abs(ref["M"]).max()))


_STATES = {}


def states(asset):
    """(cm, qpos, qvel, ctrl, labels, refs) of the asset's anisotropic model: the regime cells' copies, then N_RANDOM random states
    (label "R"); refs[e] is the Lagrange reference of state e.  Built once and shared (the GPU tests read it too)."""
    from oracle.oracle import Oracle
    if asset not in _STATES:
        cm = AM.aniso(R.model(asset))
        qc, vc, cc, labels = R.cells(asset)
        qr, vr = AM.random_states(cm, N_RANDOM, SEED)
        qpos, qvel = np.concatenate([qc, qr]), np.concatenate([vc, vr])
        ctrl = np.concatenate([cc, R.f32(qr[:, :cm.nlink])])
        orc = Oracle(cm, 1)
        tree = LO.Tree(cm)
        I, Ic = AM.inertias(cm)
        refs = []
        for e in range(len(qpos)):
            st = LO.State(tree, orc, qpos[e], qvel[e])
            b, err = st.bias(I, Ic)
            refs.append(dict(M=st.M(I, Ic), bias=b, err=err, state=st))
        _STATES[asset] = (cm, qpos, qvel, ctrl, list(labels) + ["R"] * N_RANDOM, refs)
    return _STATES[asset]


def unobservable_pair(cm, link, pair):
    """True for the one kind of swap no output can see: the first two principal values of a hinge-about-z link on the fixed base."""
    d = cm.desc
    return (pair == (0, 1) and d.link_parent[link] < 0 and d.jnt_type[link] == 0 and list(d.jnt_axis[link]) == [0.0, 0.0, 1.0])


def _fields(d):
    return {name: np.array(getattr(d, name)).tolist() if not isinstance(getattr(d, name), (int, float)) else getattr(d, name)
            for name, _ in type(d)._fields_}


@pytest.mark.parametrize("asset", ASSETS)
def test_shipped_values_give_the_compiled_desc(asset):
    cm = R.model(asset)
    same = AM.with_inertias(cm, *AM.inertias(cm))
    assert bytes(same.desc) == bytes(cm.desc) and same.desc is not cm.desc
    assert same.asset == cm.asset and same.asset is not cm.asset
    assert same.nlink == cm.nlink and same.act_slices == cm.act_slices


@pytest.mark.parametrize("asset", ASSETS)
def test_the_canonical_model_is_anisotropic_physical_and_consistent(asset):
    from gym_kmanip_amd.model import invweight0
    cm0 = R.model(asset)
    cm = AM.aniso(cm0)
    I0, _ = AM.inertias(cm0)
    I, Ic = AM.inertias(cm)
    perms = AM.permutations(cm.nlink)
    assert all(a != b for a, b in zip(perms, perms[1:])) and len(set(perms)) >= 4
    for i in range(cm.nlink):
        assert len(set(I[i])) == 3 and AM.is_physical(I[i])
        assert np.array_equal(I[i], I0[i] * np.array([AM.FACTORS[k] for k in perms[i]]))
    assert len(set(Ic)) == 3 and AM.is_physical(Ic) and tuple(Ic) == AM.CUBE_INERTIA
    assert bytes(AM.aniso(cm0).desc) == bytes(cm.desc)                  # seeded
    # the derived constants are invweight0's of the new desc; nothing else changed; the asset says the same
    dofw, bodyw, cubew, mi = invweight0(cm.desc)
    d = cm.desc
    assert [d.dof_invweight0[i] for i in range(cm.nlink)] == list(dofw)
    assert [list(d.body_invweight0[i]) for i in range(cm.nlink)] == [list(b) for b in bodyw]
    assert tuple(d.cube_invweight0) == cubew and d.meaninertia == mi
    assert cubew[1] == np.mean([1.0 / x for x in Ic]) and d.meaninertia != cm0.desc.meaninertia
    owned = {"inertia", "cube_inertia", "dof_invweight0", "body_invweight0", "cube_invweight0", "meaninertia"}
    f0, f1 = _fields(cm0.desc), _fields(d)
    assert {name for name in f0 if f0[name] != f1[name]} == owned
    assert [l["inertial"]["diaginertia"] for l in cm.asset["links"]] == I.tolist() and cm.asset["cube"]["diaginertia"] == Ic.tolist()
    assert cm0.asset["cube"]["diaginertia"] == [0.002] * 3              # the shipped asset is untouched


@pytest.mark.parametrize("asset", ASSETS)
def test_oracle_against_the_lagrange_reference(asset):
    """Figures: the module docstring."""
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, labels, refs = states(asset)
    nl = cm.nlink
    orc = Oracle(cm, 1)
    worst = dict(est=0.0, bar=0.0, dM=0.0, db=0.0, frac=0.0)
    moved = 0.0
    iso = Oracle(R.model(asset), 1)
    for e, ref in enumerate(refs):
        dyn = orc.dynamics(qpos[e], qvel[e], ctrl[e])
        dM = float(np.abs(dyn["M"] - ref["M"]).max()) / max(1.0, float(np.abs(ref["M"]).max()))
        db = float(np.abs(dyn["bias"] - ref["bias"]).max())
        bar = bias_bar(ref)
        print("%s %-5s %3d  est %.1e  bar %.1e  dM %.1e  dbias %.1e" % (asset, labels[e], e, ref["err"], bar, dM, db))
        worst = dict(est=max(worst["est"], ref["err"]), bar=max(worst["bar"], bar), dM=max(worst["dM"], dM), db=max(worst["db"], db),
                     frac=max(worst["frac"], db / bar))
        assert dM <= BAR_M, (labels[e], e, dM)
        assert db <= bar, (labels[e], e, db, bar)
        if labels[e] == "R":
            moved = max(moved, float(np.abs(dyn["bias"] - iso.dynamics(qpos[e], qvel[e], ctrl[e])["bias"]).max()))
    print("%s: worst over %d states: %s; isotropic -> anisotropic moves the bias by up to %.2e" %
          (asset, len(refs), "  ".join("%s %.1e" % kv for kv in worst.items()), moved))
    assert moved > 1e-2                                                 # the anisotropy is not a rounding-size effect


@pytest.mark.parametrize("asset", ASSETS)
def test_sensitivity_controls_in_the_reference(asset):
    """Every link, every pair of its principal values, every random state: the swap moves the reference's M or bias by at least
    1000 x the bar; the cube's Euler term negated moves its bias rows by as much.  The bar is at most 1e-3 of the smallest
    sensitivity -- the same statement."""
    cm, qpos, qvel, ctrl, labels, refs = states(asset)
    nl = cm.nlink
    I, Ic = AM.inertias(cm)
    smallest, euler, dead = np.inf, np.inf, 0
    bias_alone = {}                                                     # (link, pair): the largest move of the bias alone, in bars
    for e, ref in enumerate(refs):
        if labels[e] != "R":
            continue
        st = ref["state"]
        bar_b, bar_m = bias_bar(ref), m_bar(ref)
        assert (np.abs(qvel[e]) >= 0.5).all()
        for link, pair in itertools.product(range(nl), PAIRS):
            J = I.copy()
            J[link, pair[0]], J[link, pair[1]] = I[link, pair[1]], I[link, pair[0]]
            dM = float(np.abs(st.M(J, Ic) - ref["M"]).max())
            db = float(np.abs(st.bias(J, Ic)[0] - ref["bias"]).max())
            if unobservable_pair(cm, link, pair):
                assert dM == 0.0 and db <= 1e-15, (link, pair, dM, db)  # (the bias: two sums in another order)
                dead += 1
                continue
            s = max(dM / bar_m, db / bar_b)
            smallest = min(smallest, s)
            if cm.desc.link_parent[link] >= 0:                          # (a root link turns about one fixed axis: M_00 is constant, w x I w = 0)
                bias_alone[link, pair] = max(bias_alone.get((link, pair), 0.0), db / bar_b)
            assert s >= SENSITIVITY, (e, link, pair, dM, db, bar_m, bar_b)
        neg = st.bias(I, Ic, euler_sign=-1.0)[0]
        assert np.array_equal(neg[:nl + 3], ref["bias"][:nl + 3])
        s = float(np.abs(neg[nl + 3:] - ref["bias"][nl + 3:]).max()) / bar_b
        euler = min(euler, s)
        assert s >= SENSITIVITY, (e, "cube", s)
    roots = sum(1 for i in range(nl) if cm.desc.link_parent[i] < 0)
    assert dead == roots * N_RANDOM and roots == {"solo_arm": 1, "dual_arm": 2, "torso": 3}[asset]
    weakest = min(bias_alone, key=bias_alone.get)
    print("\n%s: smallest sensitivity over %d states x %d links x 3 pairs: %.1e bars; cube Euler term negated: %.1e bars; the bias alone, "
          "every pair's best state: at least %.1e bars (link %d, pair %s)" % (asset, N_RANDOM, nl, smallest, euler, bias_alone[weakest], *weakest))
    # M alone would carry the control (its bar is 1e-12): the bias test too sees every pair of every link that has a parent, in
    # at least one state
    assert len(bias_alone) == 3 * (nl - roots) and bias_alone[weakest] >= SENSITIVITY, (weakest, bias_alone[weakest])


@pytest.mark.parametrize("asset", ASSETS)
def test_equation_of_motion_with_the_force_oracle(asset):
    """M qacc + bias = pad(qfrc_actuator) + qfrc_constraint on every regime cell of the anisotropic model: the force oracle's
    qacc and forces with the LAGRANGE M and bias, at test_kinematics_cpu's bar (3.2e-13 measured)."""
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, labels, refs = states(asset)
    nl = cm.nlink
    orc = Oracle(cm, 1)
    worst, touched = 0.0, 0
    for e, ref in enumerate(refs):
        if labels[e] == "R":
            continue
        f = FO.decode(cm, orc, qpos[e], qvel[e], ctrl[e], geometry=False)
        touched += bool(f["mask"] & 0x000FFF00)
        mq = ref["M"] @ f["qacc"]
        rhs = f["qfrc_constraint"].copy()
        rhs[:nl] += f["qfrc_actuator"]
        r = float(np.abs(mq + ref["bias"] - rhs).max()) / max(1.0, float(np.abs(f["qfrc_constraint"]).max()), float(np.abs(mq).max()))
        worst = max(worst, r)
        assert r <= BAR_IDENTITY, (asset, labels[e], e, r)
    print("\n%s: Lagrange M qacc + bias - (qfrc_actuator + qfrc_constraint), worst over %d cells: %.1e" % (asset, len(refs) - N_RANDOM, worst))
    assert touched >= 6                                                 # cells with a sphere on the cube: torque about its centre


@pytest.mark.parametrize("asset", ASSETS)
def test_per_env_cube_mass_scales_the_three_values(asset):
    from gym_kmanip_amd.model import with_env_params
    cm = AM.aniso(R.model(asset))
    m0 = cm.desc.cube_mass
    for m in (0.5 * m0, 1.37 * m0, 3.0 * m0):
        d = with_env_params(cm, cube_mass=m).desc
        I = np.array(list(d.cube_inertia))
        assert np.array_equal(I, np.array(AM.CUBE_INERTIA) * (m / m0))
        ratio = np.array(AM.CUBE_INERTIA) / AM.CUBE_INERTIA[0]         # the ratios stay: two rounded products and a rounded quotient
        assert (np.abs(I / I[0] - ratio) <= 4 * np.finfo(np.float64).eps * ratio).all()
        assert d.cube_invweight0[0] == 1.0 / m
        assert abs(d.cube_invweight0[1] - np.mean(1.0 / I)) <= 1e-15 * d.cube_invweight0[1]
        assert [list(d.inertia[i]) for i in range(cm.nlink)] == [list(cm.desc.inertia[i]) for i in range(cm.nlink)]
    assert bytes(with_env_params(cm, cube_mass=m0).desc) == bytes(cm.desc)
