"""kmanip_forward and gym_kmanip_amd.derivatives on the CPU: the binding, tangent_perturb, forward_fd driven through the oracle
stand-in (tests/tools/forward_oracle.py OracleForward), the reference's own derivative check and the bars of
tests/test_forward_gpu.py.

No tolerance of the device parity is invented here.  Forward parity uses the bars and normalisers of tests/test_forces_cpu.py; this
file re-asserts 1000 x spread <= bar for the rows the GPU tests send (the regime cells, without and with the test forces as
qfrc_applied).  The derivative bar follows by derivation: a centred difference of two rows, each within BAR s of the reference
(s the nominal row's normaliser), lies within 2 BAR s / (2 eps) = BAR s / eps of the reference's difference (fd_bars).

The reference's own check: with the applied force as the only input moved, qacc is piecewise affine in it with slope
H^-1, H = M + J^T diag(h) J (applied_oracle._rows), so on every cell whose row-activity pattern is the same at the nominal point
and at all +-eps points the dqacc_dfrc block of forward_fd(OracleForward) must equal H^-1 up to rounding.  The bar of that gap,
normalised by max|H^-1|, is 1000 x, one digit up, the block's own spread under qvel (1 + 1e-15), measured here and committed as a
constant."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import force_oracle as FO  # noqa: E402
import forward_oracle as FW  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_forces_cpu import (BAR_CONTACT_FORCE, BAR_QACC, BAR_QFRC_ACTUATOR, BAR_QFRC_CONSTRAINT,  # noqa: E402
                             _round_up_one_digit)

ASSETS = mujoco_pin.ASSETS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6

# the dqacc_dfrc block of forward_fd(OracleForward) on the qualifying cells, normalised per cell by max|H^-1|: its worst spread under
# qvel (1 + 1e-15) over the three assets, the bar = 1000 x that, one digit up, and the worst gap to H^-1 measured against it
SPREAD_DFRC = 2.17e-9
BAR_DFRC = 3e-6
GAP_DFRC_MEASURED = 7.22e-9
# cells whose row-activity pattern is the same at the nominal point and at all 2 nv points +-eps of the applied force: all of them
# (1e-6 N moves no row across a branch in these states)
QUALIFYING = {"solo_arm": 47, "dual_arm": 72, "torso": 72}
TWIN_STRIDE = 4


def fd_bars(o, eps=EPS):
    """(dqacc, dqfrc_constraint) bars of one nominal decode o: bar x normaliser / eps (module docstring)."""
    sq, sf, _ = FO.scales(o)
    return BAR_QACC * sq / eps, BAR_QFRC_CONSTRAINT * sf / eps


# ------------------------------------------------------------------------------------------------------------------ the binding
def test_kforwardin_binding_matches_the_header():
    """lib.KForwardIn lists the header's fields in the header's order (all pointers); kmanip_forward is declared, bound with the
    right argument types and listed among the exports; the header and forward()'s docstring say what status 2 means."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    body = re.search(r"typedef struct KForwardIn \{(.*?)\} KForwardIn;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert fields == [n for n, _ in klib.KForwardIn._fields_] == ["env_index", "qpos", "qvel", "ctrl", "qacc_warm", "qfrc_applied"]
    assert all(t is C.c_void_p for _, t in klib.KForwardIn._fields_)
    assert "KMANIP_API int kmanip_forward(KHandle h, const KForwardIn* in, int n, const KForcesDev* out, void* stream);" in hdr
    assert "kmanip_forward" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_forward.argtypes == [C.c_void_p, C.POINTER(klib.KForwardIn), C.c_int, C.POINTER(klib.KForcesDev), C.c_void_p]
    assert b"0.40" in L.kmanip_version()
    assert re.search(r"2 = env_index\[r\] lies outside 0 \.\. num_envs-1", hdr)
    doc = env_hip.KManipEnvHip.forward.__doc__
    assert "2 an env index outside 0 .. num_envs-1" in doc and "state_index_errors does not count it" in doc


def test_shipped_forward_kernels_run_without_scratch():
    """The eight k_forward variants of the built library (parsed from the .so: no GPU): none spills, the LDS of their k_forces
    siblings (the same workspace), registers within the 512 of a single-wave workgroup."""
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    fwd = {(r.base, r.args[0]): r for r in BM.kernels(klib.LIB_PATH, r"k_forward\w*")}
    names = ("k_forward", "k_forward_ep", "k_forward_frc", "k_forward_ep_frc")
    assert sorted(fwd) == sorted((nm, nl) for nm in names for nl in (10, 20))
    frc = {(r.base, r.args[0]): r for r in BM.kernels(klib.LIB_PATH, r"k_(frc_)?forces\w*")}
    sibling = dict(zip(names, ("k_forces", "k_forces_ep", "k_frc_forces", "k_frc_forces_ep")))
    for (nm, nl), r in fwd.items():
        assert r.args[1:] == ((16, 4) if nl == 10 else (32, 2)), r
        assert r.scratch == 0 and r.vgpr <= 512, r
        assert r.lds == frc[(sibling[nm], nl)].lds, (r, frc[(sibling[nm], nl)])


# ------------------------------------------------------------------------------------------ every compiled object runs an identity row
def covered(identity_rows):
    """The (NL, G, ep, frc) forward objects that test_forward_gpu's comparison with forces() launches (kmanip_dispatch.hip: the 10-link
    class for nlink <= 10, the parameter build while the handle has per-env parameters, set or drawn from ranges, the force build
    while a force is bound)."""
    out = set()
    for asset, mode in identity_rows:
        cls = (10, 16) if R.model(asset).nlink <= 10 else (20, 32)
        out.add(cls + ("params" in mode or mode == "ranges", "bound" in mode))
    return out


def missing_rows(makefile_path, identity_rows):
    import build_matrix as BM
    have = covered(identity_rows)
    return [(o.NL, o.G, o.ep, o.frc) for o in BM.objects(makefile_path, "forward") if (o.NL, o.G, o.ep, o.frc) not in have]


def test_every_compiled_forward_object_has_an_identity_row():
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    from test_forward_gpu import IDENTITY_ROWS
    objs = BM.objects(BM.MAKEFILE, "forward")
    assert sorted({(o.NL, o.G, o.solver) for o in objs}) == [(10, 16, None), (20, 32, None)]
    assert missing_rows(BM.MAKEFILE, IDENTITY_ROWS) == []
    assert len(BM.kernels(klib.LIB_PATH, r"k_forward\w*")) == len(objs)          # the objects the Makefile links are the ones the library holds


def test_the_guard_fails_for_a_forward_object_without_a_row(tmp_path):
    import build_matrix as BM
    from test_forward_gpu import IDENTITY_ROWS
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    assert missing_rows(more, IDENTITY_ROWS) == [(30, 64, ep, frc) for frc in (False, True) for ep in (False, True)]
    rows = [r for r in IDENTITY_ROWS if "bound" not in r[1]]
    assert missing_rows(BM.MAKEFILE, rows) == [(nl, g, ep, True) for ep in (False, True) for nl, g in ((10, 16), (20, 32))]


# ------------------------------------------------------------------------------------------------------------------ tangent_perturb
def _perturb_numpy(cm, qpos, col, eps):
    """The restatement: joints and cube position += eps; rotation column k through applied_oracle.euler's composition -- one Euler
    step of the cube's body rate e_k for a time that makes the angle eps (euler normalises, which moves a unit quaternion by
    rounding only)."""
    nl = cm.nlink
    out = qpos.copy()
    if col < nl + 3:
        out[col] += eps
        return out
    dt = cm.desc.timestep
    a = np.zeros(cm.nv)
    a[col] = eps / (dt * dt)                  # qvel = dt a = (eps / dt) e_k, angle = dt |qvel| = eps
    q1, _ = AO.euler(cm, qpos, np.zeros(cm.nv), a)
    out[nl + 3:nl + 7] = q1[nl + 3:nl + 7]
    return out


@pytest.mark.parametrize("asset", ["solo_arm", "torso"])
def test_tangent_perturb_against_a_numpy_restatement(asset):
    import torch
    from gym_kmanip_amd.derivatives import tangent_perturb
    cm = R.model(asset)
    qpos = R.cells(asset)[0][:9]
    nl = cm.nlink
    assert np.abs(np.linalg.norm(qpos[:, nl + 3:], axis=1) - 1).max() < 1e-12 and np.abs(qpos[:, nl + 4:]).max() > 0.1
    t = torch.from_numpy(qpos.copy())
    for eps in (1e-6, -1e-6, 0.3):
        for col in range(cm.nv):
            got = tangent_perturb(cm, t, col, eps).numpy()
            assert got.shape == qpos.shape and torch.equal(t, torch.from_numpy(qpos))          # the input is not modified
            want = np.stack([_perturb_numpy(cm, q, col, eps) for q in qpos])
            if col < nl + 3:
                assert np.array_equal(got, want), (eps, col)
            else:                                # two evaluation orders of a quaternion product and one normalisation
                assert np.abs(got - want).max() <= 8 * np.finfo(np.float64).eps, (eps, col, np.abs(got - want).max())
                assert np.array_equal(got[:, :nl + 3], qpos[:, :nl + 3])
                # a rotation by eps about the cube's own axis k: R1 = R0 exp([eps e_k]x)
                k = col - nl - 3
                for g, q in zip(got, qpos):
                    ax = np.zeros(3); ax[k] = 1.0
                    assert np.abs(R.quat2mat(g[nl + 3:]) - R.quat2mat(q[nl + 3:]) @ R._rot(ax, eps)).max() < 1e-14
    with pytest.raises(ValueError):
        tangent_perturb(cm, t, cm.nv, 1e-6)


# ------------------------------------------------------------------------------------------------------- forward_fd on the oracle
_FD = {}


def _fd_dfrc(asset, twin=False):
    """forward_fd(OracleForward) with respect to the applied force on every cell of the asset, with the patterns of every row:
    computed once and shared.  The twin, at qvel (1 + 1e-15), runs on every TWIN_STRIDE-th cell only (a row costs the oracle 7 ms)."""
    import torch
    from gym_kmanip_amd.derivatives import forward_fd
    key = (asset, twin)
    if key not in _FD:
        cm = R.model(asset)
        qpos, qvel, ctrl, labels = R.cells(asset)
        if twin:
            qpos, qvel, ctrl, labels = qpos[::TWIN_STRIDE], qvel[::TWIN_STRIDE] * (1.0 + 1e-15), ctrl[::TWIN_STRIDE], labels[::TWIN_STRIDE]
        env = FW.OracleForward(cm, len(labels), patterns=True)
        d = forward_fd(env, qpos=torch.from_numpy(qpos), qvel=torch.from_numpy(qvel), ctrl=torch.from_numpy(ctrl), eps=EPS,
                       wrt=("qfrc_applied",))
        _FD[key] = (cm, env, d)
    return _FD[key]


def _qualifying(env, n, nv):
    """Cells whose pattern is the same in the nominal row and in all 2 nv perturbed rows."""
    nominal, pert = env.patterns[-2], env.patterns[-1]
    assert len(nominal) == n and len(pert) == 2 * nv * n
    return [e for e in range(n) if all(pert[k * n + e] == nominal[e] for k in range(2 * nv))]


@pytest.mark.parametrize("asset", ASSETS)
def test_dqacc_dfrc_of_the_reference_is_the_inverse_hessian(asset):
    """Counts and gaps measured: DESIGN.md section 26."""
    cm, env, d = _fd_dfrc(asset)
    _, env_t, d_t = _fd_dfrc(asset, twin=True)
    qpos, qvel, ctrl, labels = R.cells(asset)
    n, nv = len(labels), cm.nv
    assert len(env.calls) == 2 and len(env.calls[1]["qpos"]) == 2 * nv * n          # two launches
    assert tuple(d["dqacc_dfrc"].shape) == (n, nv, nv) and tuple(d["dqfrc_constraint_dfrc"].shape) == (n, nv, nv)
    assert not d["status"].any() and not d["status_fd"].any()
    assert np.array_equal(env.calls[1]["warm"], np.tile(d["qacc"].numpy() + 1.0, (2 * nv, 1)))      # warm start = the nominal qacc + 1
    cells = _qualifying(env, n, nv)
    both = [e for e in cells if e % TWIN_STRIDE == 0 and e // TWIN_STRIDE in set(_qualifying(env_t, len(labels[::TWIN_STRIDE]), nv))]
    assert len(cells) > 0 and len(both) > 0
    orc = env._orc[id(cm)]
    gap = spread = 0.0
    for e in cells:
        Hinv = FW.hinv_and_pattern(cm, orc, qpos[e], qvel[e], ctrl[e], d["qacc"][e].numpy())[0]
        g = float(np.abs(d["dqacc_dfrc"][e].numpy() - Hinv).max()) / float(np.abs(Hinv).max())
        gap = max(gap, g)
        if e in both:
            spread = max(spread, float(np.abs(d["dqacc_dfrc"][e].numpy() - d_t["dqacc_dfrc"][e // TWIN_STRIDE].numpy()).max()) / float(np.abs(Hinv).max()))
    print("\n%s: %d of %d cells keep their pattern; dqacc_dfrc vs H^-1 worst gap %.2e, spread under qvel (1 + 1e-15) %.2e"
          % (asset, len(cells), n, gap, spread))
    assert len(cells) == QUALIFYING.get(asset), (len(cells), QUALIFYING.get(asset))
    assert 1000.0 * spread <= BAR_DFRC, (spread, BAR_DFRC)
    assert BAR_DFRC == pytest.approx(_round_up_one_digit(1000.0 * SPREAD_DFRC), rel=1e-12)
    assert gap <= BAR_DFRC, (gap, BAR_DFRC)


def test_forward_fd_shapes_and_wrt_subsets():
    """Three SoloArm cells, every block: shapes, the column order of the second launch, a subset of `wrt` reproduces its blocks bit
    for bit, the refusals."""
    import torch
    from gym_kmanip_amd.derivatives import forward_fd, tangent_perturb
    cm = R.model("solo_arm")
    qpos, qvel, ctrl, labels = R.cells("solo_arm")
    pick = [labels.index("G1"), labels.index("C1"), labels.index("L1")]
    q, v, c = (torch.from_numpy(x[pick].copy()) for x in (qpos, qvel, ctrl))
    n, nv, nu = len(pick), cm.nv, cm.nu
    env = FW.OracleForward(cm, n)
    d = forward_fd(env, qpos=q, qvel=v, ctrl=c)
    ncol = 3 * nv + nu
    assert len(env.calls) == 2
    for key, w in (("dqpos", nv), ("dqvel", nv), ("dctrl", nu), ("dfrc", nv)):
        assert tuple(d["dqacc_" + key].shape) == (n, nv, w) and tuple(d["dqfrc_constraint_" + key].shape) == (n, nv, w)
    assert tuple(d["contact_mask_fd"].shape) == (ncol, 2, n) and tuple(d["status_fd"].shape) == (n,)
    big = env.calls[1]
    assert all(len(big[k]) == 2 * ncol * n for k in ("envs", "qpos", "qvel", "ctrl", "warm", "qfrc_applied"))
    assert np.array_equal(big["envs"], np.tile(np.arange(n), 2 * ncol))
    # rows (2 col + sign) n .. + n: column `col` of the wrt order moved by +-eps, everything else the nominal rows
    col = nv + 3                                                         # qvel column 3
    lo = 2 * col * n
    assert np.array_equal(big["qvel"][lo:lo + n, 3], v.numpy()[:, 3] + EPS) and np.array_equal(big["qvel"][lo + n:lo + 2 * n, 3], v.numpy()[:, 3] - EPS)
    assert np.array_equal(big["qpos"][lo:lo + 2 * n], np.tile(q.numpy(), (2, 1)))
    col = cm.nlink + 4                                                   # a rotation column of qpos
    lo = 2 * col * n
    assert np.array_equal(big["qpos"][lo + n:lo + 2 * n], tangent_perturb(cm, q, col, -EPS).numpy())
    assert np.array_equal(env.calls[0]["qfrc_applied"], np.zeros((n, nv)))
    sub = forward_fd(FW.OracleForward(cm, n), qpos=q, qvel=v, ctrl=c, wrt=("ctrl", "qvel"))
    assert sorted(k for k in sub if k.startswith("dq")) == ["dqacc_dctrl", "dqacc_dqvel", "dqfrc_constraint_dctrl", "dqfrc_constraint_dqvel"]
    for k in ("dqacc_dctrl", "dqacc_dqvel", "dqfrc_constraint_dctrl", "dqfrc_constraint_dqvel", "qacc"):
        assert torch.equal(sub[k], d[k]), k
    none = forward_fd(FW.OracleForward(cm, n), qpos=q, qvel=v, ctrl=c, wrt=())
    assert sorted(none) == ["qacc", "qfrc_constraint", "status"]
    with pytest.raises(ValueError):
        forward_fd(env, qpos=q, qvel=v, ctrl=c, wrt=("qacc",))
    with pytest.raises(ValueError):
        forward_fd(env, qvel=v, ctrl=c, wrt=("qpos",))
    # a servo at its clamp has no derivative with respect to its ctrl; one in range has kp M^-1 (through the constraints)
    assert np.abs(d["dqacc_dctrl"].numpy()).max() > 1.0


# ------------------------------------------------------------------------------------------------------------------ the bars
def test_the_forces_bars_hold_for_the_rows_the_gpu_tests_send():
    """1000 x spread <= bar, re-asserted on the rows of tests/test_forward_gpu.py: every regime cell as a caller row (the spreads of
    force_oracle.cell_decodes, which tests/test_forces_cpu.py measures).  The same rows under the test forces as qfrc_applied are
    held to the same bars, as tests/test_applied_force_gpu.py holds forces() under a bound force; their spreads
    (applied_oracle.forces_decode at qvel and at qvel (1 + 1e-15)) are measured here: qfrc_constraint 3.24e-14, contact force
    1.45e-12 and qfrc_actuator 9.3e-16 keep the factor 1000; qacc spreads by 3.06e-14 under the forces (1.76e-14 without), so its
    bar of 2e-11 is 650 x the reference's own error there, not 1000 x.  The bar is not widened for it: asserted is that it stays
    at least 100 x above the spread."""
    from oracle.oracle import Oracle
    names = ("qacc", "qfrc_constraint", "contact_force", "qfrc_actuator")
    bars = (BAR_QACC, BAR_QFRC_CONSTRAINT, BAR_CONTACT_FORCE, BAR_QFRC_ACTUATOR)
    plain, forced = np.zeros(4), np.zeros(4)
    for asset in ASSETS:
        cm, dec, tw = FO.cell_decodes(asset)
        for o, t in zip(dec, tw):
            plain = np.maximum(plain, FO.spreads(o, t))
        qpos, qvel, ctrl, labels = R.cells(asset)
        tau = AO.draw_test_forces(cm, len(labels))
        orc = Oracle(cm, 1)
        for e in range(len(labels)):
            o = FW.row(cm, orc, qpos[e], qvel[e], ctrl[e], None, tau[e], geometry=False)
            t = FW.row(cm, orc, qpos[e], qvel[e] * (1.0 + 1e-15), ctrl[e], None, tau[e], geometry=False)
            forced = np.maximum(forced, FO.spreads(o, t))
    for tag, w in (("as caller rows", plain), ("under the test forces", forced)):
        print("\nspreads of the rows sent %s: qacc %.2e  qfrc_constraint %.2e  contact force %.2e  qfrc_actuator %.2e" % ((tag,) + tuple(w)))
    for name, s, bar in zip(names, plain, bars):
        assert 1000.0 * s <= bar, (name, s, bar)
    for name, s, bar in zip(names, forced, bars):
        assert (100.0 if name == "qacc" else 1000.0) * s <= bar, (name, s, bar)
    o = FO.cell_decodes("solo_arm")[1][0]
    sq, sf, _ = FO.scales(o)
    assert fd_bars(o) == (BAR_QACC * sq / EPS, BAR_QFRC_CONSTRAINT * sf / EPS)


def test_oracle_forward_serves_stored_state_bad_rows_and_indices():
    """The stand-in's own semantics, which the device tests rely on: None = the env's stored field, status 1 / 2 rows are zeros with
    contact_bit -1, rows may outnumber envs, and a row is applied_oracle.forces_decode of its own model."""
    import torch
    from gym_kmanip_amd.model import with_env_params
    cm = R.model("solo_arm")
    cmp_ = with_env_params(cm, cube_mass=2.0 * cm.desc.cube_mass, cube_friction=0.5, cube_frictionloss=0.0, kp_scale=1.3)
    qpos, qvel, ctrl, labels = R.cells("solo_arm")
    e = labels.index("G1")
    st = dict(qpos=qpos[e:e + 2], qvel=qvel[e:e + 2], ctrl=ctrl[e:e + 2], warm=np.zeros((2, cm.nv)))
    env = FW.OracleForward(cm, 2, state=st, models=[cm, cmp_])
    qrow = np.tile(qpos[e], (5, 1))
    qrow[3, 2] = np.nan
    f = env.forward(envs=[0, 1, -1, 0, 2], qpos=torch.from_numpy(qrow))
    assert f["status"].tolist() == [0, 0, 2, 1, 2] and tuple(f["qacc"].shape) == (5, cm.nv)
    for r in (2, 3, 4):
        assert not f["qacc"][r].any() and not f["contact_force"][r].any() and (f["contact_bit"][r] == -1).all() and f["contact_mask"][r] == 0
    from oracle.oracle import Oracle
    o0 = FW.row(cm, Oracle(cm, 1), qpos[e], qvel[e], ctrl[e])
    o1 = FW.row(cmp_, Oracle(cmp_, 1), qpos[e], qvel[e + 1], ctrl[e + 1])
    assert np.array_equal(f["qacc"][0].numpy(), o0["qacc"]) and np.array_equal(f["qacc"][1].numpy(), o1["qacc"])
    bits = f["contact_bit"][0].numpy()
    assert sorted(int(b) for b in bits if b >= 0) == FO.mask_bits(o0["mask"]) == FO.mask_bits(int(f["contact_mask"][0]))
    for s, b in enumerate(bits):
        if b >= 0:
            assert np.array_equal(f["contact_force"][0, s].numpy(), o0["contacts"][int(b)]["force"])
