"""kmanip_rollout and transition_fd on the CPU: the binding, the reference's own checks (tests/tools/rollout_oracle.py OracleRollout),
tangent_diff, transition_fd driven through the oracle stand-in, and the guard that the device tests launch every compiled rollout
object.

No tolerance of the device parity is invented here: the state bars are test_gpu_parity's (qpos 1e-7, qvel 1e-5, reward 1e-6), and the
reference's own spread under qvel (1 + 1e-15) must stay ten times below them on every cell (test_regimes_gpu's rule).  The bar of
the derivative check is tests/test_forward_cpu.py's BAR_DFRC (3e-6 on the H^-1 normaliser), scaled by dt."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import build_matrix as BM  # noqa: E402
import forward_oracle as FW  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402
from test_forward_cpu import BAR_DFRC, EPS, QUALIFYING  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_R, TOL_V  # noqa: E402

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = {"qpos": TOL_Q, "qvel": TOL_V, "reward": TOL_R}


# ------------------------------------------------------------------------------------------------------------------ the binding
def test_rollout_binding_matches_the_header():
    """lib.KRolloutIn / KRolloutDev list the header's fields in the header's order; kmanip_rollout is declared, bound with the right
    argument types and listed among the exports."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    for name, cls in (("KRolloutIn", klib.KRolloutIn), ("KRolloutDev", klib.KRolloutDev)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(\*?)\s*(\w+)\s*;", body)
        assert [f for _, f in fields] == [n for n, _ in cls._fields_], name
        assert [C.c_void_p if star else C.c_int32 for star, _ in fields] == [t for _, t in cls._fields_], name
    assert [n for n, _ in klib.KRolloutIn._fields_] == ["env_index", "qpos", "qvel", "qacc_warm", "ctrl", "qfrc_applied", "ctrl_per_step", "frc_per_step"]
    assert [n for n, _ in klib.KRolloutDev._fields_] == ["qpos", "qvel", "qacc_warm", "contact_mask", "reward", "status", "steps_done"]
    assert ("KMANIP_API int kmanip_rollout(KHandle h, const KRolloutIn* in, int n, int nstep, int nsub, const KRolloutDev* out, void* stream);"
            in hdr)
    assert "kmanip_rollout" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_rollout.argtypes == [C.c_void_p, C.POINTER(klib.KRolloutIn), C.c_int, C.c_int, C.c_int, C.POINTER(klib.KRolloutDev), C.c_void_p]
    assert set(env_hip.KManipEnvHip._ROLLOUT_FIELDS) == {n for n, _ in klib.KRolloutDev._fields_} == set(RO.FIELDS)


def _rollout_table():
    """The k_rollout* kernels of the built library; args = (NL, G, SOLVER, rows per wave)."""
    from gym_kmanip_amd import lib as klib
    return BM.kernels(klib.LIB_PATH, r"k_rollout\w*")


def test_shipped_rollout_kernels_run_without_scratch():
    """The sixteen k_rollout variants of the built library (parsed from the .so: no GPU): one per (class, solver) in each of the four
    builds, 64 / G rows per wave, none spills, registers within the 512 of a single-wave workgroup."""
    rows = _rollout_table()
    names = ("k_rollout", "k_rollout_ep", "k_rollout_frc", "k_rollout_ep_frc")
    assert sorted((r.base, r.args[0], r.args[2]) for r in rows) == sorted((nm, nl, s) for nm in names for nl in (10, 20) for s in (0, 1))
    for r in rows:
        assert len(r.args) == 4 and (r.args[1], r.args[3]) == ((16, 4) if r.args[0] == 10 else (32, 2)), r
        assert r.scratch == 0 and r.vgpr <= 512, r


# ------------------------------------------------------------------------------------------------------- the reference's own spread
def _cellwise(d, labels):
    out = {}
    for c, v in zip(labels, d):
        out[c] = max(out.get(c, 0.0), float(v))
    return out


def spreads(run):
    """{quantity: {cell: worst |twin - ref| over the cell's rows and all steps}} of a rollout_oracle.cell_runs entry."""
    rows = run["twin_rows"]
    labels = [run["labels"][e] for e in rows]
    return {k: _cellwise(np.abs(run["twin"][k] - run["ref"][k][rows]).reshape(len(rows), -1).max(axis=1), labels) for k in BARS}


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_the_references_own_spread_stays_ten_times_below_the_bars(asset, solver):
    """OracleRollout at qvel and at qvel (1 + 1e-15), every cell, 3 steps of the model's sub-steps: the run FAILS if ten times any
    cell's spread exceeds its bar (no cell may be left out; a cell that breaks the rule is a finding to report)."""
    run = RO.cell_runs(asset, solver)
    n = len(run["labels"])
    assert n == QUALIFYING[asset] and len(run["twin_rows"]) == n and run["cm"].desc.n_sub_steps == 10
    assert not run["ref"]["status"].any() and (run["ref"]["steps_done"] == RO.NSTEP).all() and not run["twin"]["status"].any()
    assert np.array_equal(run["ref"]["contact_mask"], run["twin"]["contact_mask"])
    sp = spreads(run)
    print("\n%s %s: the reference's own spread per cell over 3 steps" % (asset, solver))
    for c in dict.fromkeys(run["labels"]):
        print("  %-5s %s" % (c, "  ".join("%s %.1e" % (k, sp[k][c]) for k in BARS)))
    broken = [(c, k, s) for k, bar in BARS.items() for c, s in sp[k].items() if not 10.0 * s <= bar]
    assert not broken, broken


# --------------------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_ten_steps_of_one_sub_step_are_one_step_of_ten(asset, solver):
    """nsub = 1, nstep = 10 ends where nsub = 10, nstep = 1 ends, and both are Oracle.physics_step(.., 10): the same code path, so
    equality.  The intermediate records of the first are the states physics_step(.., k) reaches."""
    from oracle.oracle import Oracle
    run = RO.cell_runs(asset, solver)
    cm, rows = run["cm"], run["rows"]
    env = RO.OracleRollout(cm, 2)
    fine = env.rollout(nstep=10, nsub=1, **rows)
    coarse = env.rollout(nstep=1, nsub=10, **rows)
    orc = Oracle(cm, 1)
    for k in ("qpos", "qvel", "qacc_warm", "contact_mask", "reward"):
        assert np.array_equal(fine[k][:, -1], coarse[k][:, 0]), k
        assert np.array_equal(coarse[k][:, 0], run["ref"][k][:, 0]), k           # (the shared run's first step: nsub = None is the model's 10)
    for e in range(len(run["labels"])):
        q, v, w, bad = orc.physics_step(rows["qpos"][e], rows["qvel"][e], rows["ctrl"][e], rows["warm"][e], rows["qpos"][e], 10)[:4]
        assert not bad and np.array_equal(q, coarse["qpos"][e, 0]) and np.array_equal(v, coarse["qvel"][e, 0]) and np.array_equal(w, coarse["qacc_warm"][e, 0])
    e = 3
    q, v, w = orc.physics_step(rows["qpos"][e], rows["qvel"][e], rows["ctrl"][e], rows["warm"][e], rows["qpos"][e], 4)[:3]
    assert np.array_equal(q, fine["qpos"][e, 3]) and np.array_equal(w, fine["qacc_warm"][e, 3])


def test_oracle_rollout_serves_stored_state_bad_rows_and_indices():
    """The stand-in's own semantics, which the device tests rely on: None = the env's stored field, held and per-step rows, status 1
    with steps_done where the non-finite value first acts, status 2, zeros after a stop, a row with parameters takes its own model."""
    cm = R.model("solo_arm")
    qpos, qvel, ctrl, labels = R.cells("solo_arm")
    e = labels.index("G1")
    models = RO.env_params(cm)[1]
    st = dict(qpos=qpos[e:e + 2], qvel=qvel[e:e + 2], ctrl=ctrl[e:e + 2], warm=np.zeros((2, cm.nv)))
    env = RO.OracleRollout(cm, 2, state=st, models=models)
    c3 = np.tile(ctrl[e], (5, 3, 1))
    c3[3, 1, 0] = np.nan
    f = env.rollout(envs=[0, 1, -1, 0, 2], ctrl=c3, nsub=1)
    assert f["status"].tolist() == [0, 0, 2, 1, 2] and f["steps_done"].tolist() == [3, 3, 0, 1, 0] and f["qpos"].shape == (5, 3, cm.nq)
    assert not f["qpos"][2].any() and not f["qpos"][3, 1:].any() and f["qpos"][3, 0].any() and not f["contact_mask"][3, 1:].any()
    assert np.array_equal(f["qpos"][3, 0], f["qpos"][0, 0]) and not np.array_equal(f["qpos"][0], f["qpos"][1])
    held = env.rollout(envs=[0, 1], nstep=3, nsub=1)                                  # everything stored, ctrl held
    assert np.array_equal(held["qpos"][0], f["qpos"][0]) and held["qpos"][1].any()
    assert sorted(env.rollout(envs=[0], fields=("qvel", "status"))) == ["qvel", "status"]


# -------------------------------------------------------------------------------------------------------------------- tangent_diff
@pytest.mark.parametrize("asset", ["solo_arm", "torso"])
def test_tangent_diff_inverts_tangent_perturb(asset):
    """tangent_diff(tangent_perturb(q, k, eps), q) = eps e_k for eps = 1e-6 on every column, every cell's qpos.
    THE BAR.  1e-12 relative to the state's scale, max(1, |q|_inf): the perturbed point is STORED in float64, so (q + eps) - q
    carries the rounding of q + eps, half an ulp of q, whatever computes the difference -- measured 1.4e-16 on joints of up to
    3.3 rad and 2.2e-16 on the rotation columns, i.e. 1.4e-10 and 2.2e-10 relative to eps; a bar of 1e-12 relative to EPS (1e-18)
    cannot be met by any tangent_diff in this number format.  What it can be held to, and is: on the joint and cube-position
    columns the result equals the realised perturbation fl(q + eps) - q bit for bit (the subtraction of neighbours is exact),
    and nothing but column k moves.  The rotation part's own error is the O(eps^3) curvature of the log map, 1e-18, far below
    the rounding of the stored quaternion."""
    import torch
    from gym_kmanip_amd.derivatives import tangent_diff, tangent_perturb
    cm = R.model(asset)
    qpos = R.cells(asset)[0]
    nl, nv = cm.nlink, cm.nv
    q = torch.from_numpy(qpos.copy())
    scale = max(1.0, float(np.abs(qpos).max()))
    worst = 0.0
    for eps in (EPS, -EPS):
        for k in range(nv):
            p = tangent_perturb(cm, q, k, eps)
            d = tangent_diff(cm, p, q).numpy()
            assert d.shape == (len(qpos), nv) and torch.equal(q, torch.from_numpy(qpos))
            want = np.zeros(nv); want[k] = eps
            worst = max(worst, float(np.abs(d - want).max()))
            assert np.abs(d - want).max() <= 1e-12 * scale, (eps, k, np.abs(d - want).max())
            if k < nl + 3:
                assert np.array_equal(d[:, k], p.numpy()[:, k] - qpos[:, k]) and not np.delete(d, k, axis=1).any(), (eps, k)
            else:
                assert not d[:, :nl + 3].any(), (eps, k)
    print("\n%s: worst |tangent_diff(tangent_perturb(q, k, eps), q) - eps e_k| = %.2e (%.2e relative to eps) with |q| up to %.2f"
          % (asset, worst, worst / EPS, scale))
    # a finite rotation: the body-frame rotation vector between two orientations, whatever the quaternions' norms
    a = q[:5].clone()
    b = tangent_perturb(cm, tangent_perturb(cm, a, nl + 3, 0.7), nl + 5, -0.4)
    d = tangent_diff(cm, 3.0 * b, 0.5 * a).numpy()
    for i in range(5):
        ex, ez = np.array([1.0, 0, 0]), np.array([0, 0, 1.0])
        Rrel = R._rot(ex, 0.7) @ R._rot(ez, -0.4)
        ang = np.linalg.norm(d[i, nl + 3:])
        assert np.abs(R._rot(d[i, nl + 3:] / ang, ang) - Rrel).max() < 1e-14
    assert not tangent_diff(cm, q[:5], q[:5]).numpy().any()


# ------------------------------------------------------------------------------------------------- transition_fd's own reference
def _right_jacobian(phi):
    """J_r(phi) of SO(3): log(exp(phi)^-1 exp(phi + d)) = J_r(phi) d + O(d^2), the differential of the body-frame log map."""
    t = np.linalg.norm(phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if t < 1e-8:
        return np.eye(3) - 0.5 * K
    return np.eye(3) - (1 - np.cos(t)) / t ** 2 * K + (t - np.sin(t)) / t ** 3 * (K @ K)


class _Keep:
    """transition_fd's view of a rollout stand-in -- .cm and .rollout -- that keeps what every call returned."""

    def __init__(self, env):
        self.env, self.cm, self.results = env, env.cm, []

    def rollout(self, **kw):
        self.results.append(self.env.rollout(**kw))
        return self.results[-1]


_TFD = {}


def _tfd_dfrc(asset):
    """transition_fd(OracleRollout) of one mj_step with respect to the applied force on every cell, computed once."""
    import torch
    from gym_kmanip_amd.derivatives import transition_fd
    if asset not in _TFD:
        run = RO.cell_runs(asset)
        cm, rows = run["cm"], run["rows"]
        env = RO.OracleRollout(cm, 2)
        t = {k: torch.from_numpy(v) for k, v in rows.items()}
        keep = _Keep(env)
        _TFD[asset] = (cm, rows, env, keep, transition_fd(keep, envs=t["envs"], qpos=t["qpos"], qvel=t["qvel"], ctrl=t["ctrl"], warm=t["warm"],
                                                    nsub=1, eps=EPS, wrt=("qfrc_applied",)))
    return _TFD[asset]


@pytest.mark.parametrize("asset", ASSETS)
def test_dnext_dfrc_of_the_reference_is_dt_times_the_inverse_hessian(asset):
    """One mj_step (nsub = 1), the applied force the only input moved: on every cell whose row-activity pattern
    (forward_oracle.hinv_and_pattern) is the same at the nominal point and at all +-eps points, qacc is affine in the force with
    slope H^-1, so the qvel rows of dnext_dfrc are dt H^-1; and semi-implicit Euler moves the positions with the NEW velocity, so
    the qpos rows are dt times the qvel rows.  Bar: section 26's 3e-6 on the H^-1 normaliser max|H^-1|, scaled by dt (and by dt
    again for the qpos rows); every cell must qualify.
    THE ROTATION ROWS.  Joints and cube position are q + dt v', linear in v'.  The cube's quaternion is q (x) exp(dt w'), and the
    tangent difference of two such products is log(exp(dt w'-)^-1 exp(dt w'+)) = dt J_r(dt w') (w'+ - w'-) + O(eps^2), J_r the
    right Jacobian of SO(3) -- the identity only while the cube does not spin.  Against dt times the qvel rows themselves these
    three rows miss by dt |w'| / 2 of their size, measured 2.6e-2 in the cell C2 (w' = 25.7 rad/s) against the bar of 3e-6; with J_r
    they are held to the same bar as every other row."""
    cm, rows, env, keep, d = _tfd_dfrc(asset)
    n, nv, nl, dt = len(rows["qpos"]), cm.nv, cm.nlink, cm.desc.timestep
    assert len(env.calls) == 2 and len(env.calls[1]["qpos"]) == 2 * nv * n and env.calls[1]["nstep"] == 1 and env.calls[1]["nsub"] == 1
    assert tuple(d["dnext_dfrc"].shape) == (n, 2 * nv, nv) and "A" not in d and "B" not in d
    assert not d["status"].any() and not d["status_fd"].any()
    assert np.array_equal(env.calls[1]["warm"], np.tile(rows["warm"] + 1.0, (2 * nv, 1)))      # the nominal warm start + 1
    orc = env._orc[id(cm)]
    # every perturbed row's own solution: with one sub-step a row's qacc_warm after the step is its qacc (the force moves no row
    # of the constraint Jacobian: the rows are those of the nominal state)
    pert_acc = keep.results[1]["qacc_warm"][:, 0].numpy().reshape(2 * nv, n, nv)
    qualifying, gap_v, gap_q, gap_naive = [], 0.0, 0.0, 0.0
    D = d["dnext_dfrc"].numpy()
    for e in range(n):
        q0, v0, c0 = rows["qpos"][e], rows["qvel"][e], rows["ctrl"][e]
        a0 = d["qacc_warm"][e].numpy()
        Hinv, pat = FW.hinv_and_pattern(cm, orc, q0, v0, c0, a0)
        same = all(FW.hinv_and_pattern(cm, orc, q0, v0, c0, pert_acc[k, e])[1] == pat for k in range(2 * nv))
        if not same:
            continue
        qualifying.append(e)
        nm = float(np.abs(Hinv).max())
        gap_v = max(gap_v, float(np.abs(D[e, nv:] - dt * Hinv).max()) / (dt * nm))
        want = dt * D[e, nv:].copy()
        gap_naive = max(gap_naive, float(np.abs(D[e, :nv] - want).max()) / (dt * dt * nm))
        want[nl + 3:] = dt * _right_jacobian(dt * d["qvel"][e].numpy()[nl + 3:]) @ D[e, nv + nl + 3:]
        gap_q = max(gap_q, float(np.abs(D[e, :nv] - want).max()) / (dt * dt * nm))
    print("\n%s: %d of %d cells keep their pattern; qvel rows vs dt H^-1 worst gap %.2e; qpos rows vs dt (J_r) qvel rows %.2e "
          "(%.2e with the identity in place of J_r); bar %.0e" % (asset, len(qualifying), n, gap_v, gap_q, gap_naive, BAR_DFRC))
    assert len(qualifying) == QUALIFYING[asset], (len(qualifying), QUALIFYING[asset])
    assert gap_v <= BAR_DFRC and gap_q <= BAR_DFRC, (gap_v, gap_q, BAR_DFRC)


def test_transition_fd_shapes_and_wrt_subsets():
    """Three SoloArm cells, every block: shapes, the column order of the second launch, A's column halves, a subset of `wrt`
    reproduces its blocks bit for bit, the refusals; a kinematic identity of one semi-implicit Euler step: d qpos' / d qvel holds
    dt on the diagonal of the joints that nothing constrains."""
    import torch
    from gym_kmanip_amd.derivatives import tangent_perturb, transition_fd
    cm = R.model("solo_arm")
    qpos, qvel, ctrl, labels = R.cells("solo_arm")
    pick = [labels.index("G1"), labels.index("C1"), labels.index("L1")]
    q, v, c = (torch.from_numpy(x[pick].copy()) for x in (qpos, qvel, ctrl))
    n, nv, nu = len(pick), cm.nv, cm.nu
    w = torch.zeros((n, nv), dtype=torch.float64)
    env = RO.OracleRollout(cm, n)
    d = transition_fd(env, qpos=q, qvel=v, ctrl=c, warm=w, nsub=1)
    ncol = 2 * nv + nu
    assert len(env.calls) == 2
    assert tuple(d["A"].shape) == (n, 2 * nv, 2 * nv) and tuple(d["B"].shape) == (n, 2 * nv, nu) and "dnext_dfrc" not in d
    assert tuple(d["contact_mask_fd"].shape) == (ncol, 2, n) and tuple(d["status_fd"].shape) == (n,) and tuple(d["qpos"].shape) == (n, cm.nq)
    big = env.calls[1]
    assert all(len(big[k]) == 2 * ncol * n for k in ("envs", "qpos", "qvel", "ctrl", "warm")) and big["ctrl"].ndim == 2 and big["qfrc_applied"] is None
    assert np.array_equal(big["envs"], np.tile(np.arange(n), 2 * ncol))
    col = nv + 3                                                         # qvel column 3
    lo = 2 * col * n
    assert np.array_equal(big["qvel"][lo:lo + n, 3], v.numpy()[:, 3] + EPS) and np.array_equal(big["qvel"][lo + n:lo + 2 * n, 3], v.numpy()[:, 3] - EPS)
    assert np.array_equal(big["qpos"][lo:lo + 2 * n], np.tile(q.numpy(), (2, 1)))
    col = cm.nlink + 4                                                   # a rotation column of qpos
    lo = 2 * col * n
    assert np.array_equal(big["qpos"][lo + n:lo + 2 * n], tangent_perturb(cm, q, col, -EPS).numpy())
    assert np.array_equal(big["warm"], np.ones((2 * ncol * n, nv)))
    # the force block on request: rows of zeros given explicitly to both launches
    fenv = RO.OracleRollout(cm, n)
    f = transition_fd(fenv, qpos=q[:1], qvel=v[:1], ctrl=c[:1], warm=w[:1], nsub=1, wrt=("qfrc_applied",))
    assert tuple(f["dnext_dfrc"].shape) == (1, 2 * nv, nv) and np.array_equal(fenv.calls[0]["qfrc_applied"], np.zeros((1, nv)))
    assert len(fenv.calls[1]["qfrc_applied"]) == 2 * nv and np.abs(fenv.calls[1]["qfrc_applied"]).max() == EPS
    sub = transition_fd(RO.OracleRollout(cm, n), qpos=q, qvel=v, ctrl=c, warm=w, nsub=1, wrt=("ctrl", "qvel"))
    assert "A" not in sub and torch.equal(sub["B"], d["B"]) and torch.equal(sub["dnext_dqvel"], d["A"][:, :, nv:]) and torch.equal(sub["qpos"], d["qpos"])
    none = transition_fd(RO.OracleRollout(cm, n), qpos=q, qvel=v, ctrl=c, warm=w, nsub=1, wrt=())
    assert sorted(none) == ["contact_mask", "qacc_warm", "qpos", "qvel", "status"]
    with pytest.raises(ValueError):
        transition_fd(env, qpos=q, qvel=v, ctrl=c, wrt=("qacc",))
    with pytest.raises(ValueError):
        transition_fd(env, qvel=v, ctrl=c, wrt=("qpos",))
    with pytest.raises(ValueError):
        transition_fd(env, qpos=q, qvel=v, ctrl=c.unsqueeze(1), wrt=("qvel",))
    # semi-implicit Euler on joints and cube position, q' = q + dt v': their rows of A and B are the identity's plus dt times the
    # velocity rows (the quotients' own rounding: 1e-16 / eps)
    A, B = d["A"].numpy(), d["B"].numpy()
    dt = cm.desc.timestep
    k = cm.nlink + 3
    eye = np.concatenate([np.eye(nv), np.zeros((nv, nv))], axis=1)[:k]
    assert np.abs(A[:, :k] - (eye + dt * A[:, nv:nv + k])).max() < 1e-8 and np.abs(B[:, :k] - dt * B[:, nv:nv + k]).max() < 1e-8
    assert np.abs(B).max() > 1e-3 and np.abs(A[:, nv:, :nv]).max() > 1.0


# ------------------------------------------------------------------------------------------- the bars of the device's derivatives
# transition_fd(OracleRollout) on rollout_oracle.FD_CELLS with the model compiled at FD_TOLERANCE: the worst spread of each block
# under qvel (1 + 1e-15) over the three assets (rollout_oracle.fd_dist: per cell, normalised by max(1, max|block|)), measured here
# and committed; the bar of tests/test_rollout_gpu.py is 1000 x that, one digit up -- section 26's margin: the device rounds
# differently at every operation but solves the same problem.  Keys: nsub (None = the model's 10 sub-steps).
# The states' bars divided by eps would be 0.1 and 10: useless, hence these.  The qpos rows' spread at nsub = 1 is one ulp of a
# coordinate of size 1 divided by eps.
SPREAD_FD = {1: {"A_qpos": 2.220e-10, "A_qvel": 4.235e-11, "B_qpos": 2.220e-10, "B_qvel": 1.295e-11},
             None: {"A_qpos": 1.332e-09, "A_qvel": 1.250e-09, "B_qpos": 6.090e-10, "B_qvel": 1.401e-09}}
BAR_FD = {1: {"A_qpos": 3e-7, "A_qvel": 5e-8, "B_qpos": 3e-7, "B_qvel": 2e-8},
          None: {"A_qpos": 2e-6, "A_qvel": 2e-6, "B_qpos": 7e-7, "B_qvel": 2e-6}}


@pytest.mark.parametrize("nsub", [1, None], ids=["mj_step", "control_step"])
def test_the_derivative_bars_are_1000_times_the_references_own_spread(nsub):
    """Also the choice of FD_TOLERANCE: between it, ten times it and a tenth of it the reference's A and B do not change in a single
    bit (the forward problem is piecewise quadratic, so the Newton step taken once the active set is right lands on the solution
    whatever the tolerance that let it be taken; scanned from 1e-5 to 1e-11: DESIGN.md section 27)."""
    from test_forces_cpu import _round_up_one_digit
    worst = {k: 0.0 for k in RO.FD_BLOCKS}
    for asset in ASSETS:
        cm, rows, env, d = RO.fd_reference(asset, nsub)
        t = RO.fd_reference(asset, nsub, twin=True)[3]
        assert len(rows["qpos"]) == 6 and len(env.calls) == 2 and env.calls[1]["nsub"] == (nsub or 10) and cm.desc.solver_tolerance == RO.FD_TOLERANCE
        assert not d["status"].any() and not d["status_fd"].any()
        assert np.array_equal(d["contact_mask_fd"].numpy(), t["contact_mask_fd"].numpy())
        for k, v in RO.fd_dist(RO.fd_blocks(d, cm.nv), RO.fd_blocks(t, cm.nv)).items():
            worst[k] = max(worst[k], float(v.max()))
        for tol in (10.0 * RO.FD_TOLERANCE, 0.1 * RO.FD_TOLERANCE):
            o = RO.fd_reference(asset, nsub, tolerance=tol)[3]
            assert all(np.array_equal(d[k].numpy(), o[k].numpy()) for k in ("A", "B")), (asset, tol)
    print("\nnsub %s: spread of the reference's blocks under qvel (1 + 1e-15): %s" % (nsub, "  ".join("%s %.3e" % kv for kv in worst.items())))
    for k in RO.FD_BLOCKS:
        assert 1000.0 * worst[k] <= BAR_FD[nsub][k], (k, worst[k])
        assert BAR_FD[nsub][k] == pytest.approx(_round_up_one_digit(1000.0 * SPREAD_FD[nsub][k]), rel=1e-12), k


# ------------------------------------------------------------------------------------------ every compiled object runs a parity row
SOLVER_OF = {"pgs": 0, "newton": 1}


def covered(parity_rows, identity_rows):
    """The (NL, G, SOLVER, ep, frc) objects the device tests launch.  kmanip_dispatch.hip picks the 10-link class for nlink <= 10,
    the parameter build while the handle has per-env parameters, the force build while the call gives a force or one is bound."""
    from gym_kmanip_amd.model import compile_model
    out = set()
    for asset, solver, mode, _ in parity_rows:
        cls = (10, 16) if R.model(asset).nlink <= 10 else (20, 32)
        out.add(cls + (SOLVER_OF[solver], "params" in mode, "forced" in mode))
    for env_id, solver in identity_rows:
        cls = (10, 16) if compile_model(env_id).nlink <= 10 else (20, 32)
        out.add(cls + (SOLVER_OF[solver], False, False))
    return out


def missing_rows(makefile_path, parity_rows, identity_rows):
    have = covered(parity_rows, identity_rows)
    return [tuple(o[1:]) for o in BM.objects(makefile_path, "rollout") if tuple(o[1:]) not in have]


def test_every_compiled_rollout_object_has_a_parity_row():
    from test_rollout_gpu import IDENTITY_ROWS, PARITY_ROWS
    objs = BM.objects(BM.MAKEFILE, "rollout")
    assert sorted({o[1:4] for o in objs}) == sorted([(10, 16, 1), (10, 16, 0), (20, 32, 1), (20, 32, 0)])
    assert missing_rows(BM.MAKEFILE, PARITY_ROWS, IDENTITY_ROWS) == []
    # the objects the Makefile links are the ones the library holds
    assert len(_rollout_table()) == len(objs)


def test_the_guard_fails_for_a_rollout_variant_without_a_row(tmp_path):
    from test_rollout_gpu import IDENTITY_ROWS, PARITY_ROWS
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    assert sorted(missing_rows(more, PARITY_ROWS, IDENTITY_ROWS)) == [(30, 64, s, ep, frc) for s in (0, 1) for ep in (False, True) for frc in (False, True)]
    # ... and for a row set that drops the PGS force rows
    rows = [r for r in PARITY_ROWS if not (r[1] == "pgs" and "forced" in r[2])]
    miss = missing_rows(BM.MAKEFILE, rows, IDENTITY_ROWS)
    assert (10, 16, 0, False, True) in miss and (20, 32, 0, True, True) in miss
