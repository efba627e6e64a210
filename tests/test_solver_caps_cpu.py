"""solver_iterations and solver_tolerance on the CPU oracle alone: the reference side of tests/test_solver_caps_gpu.py.

Every other test compiles its models at 100 iterations and a tolerance of 1e-8 (1e-10 for the derivative tests).  On the regime
cells no Newton solve comes near 100 iterations, so the capped exit of the solver, the arm -> cube switch it triggers and the
iteration count the joint loop hands over are never taken.  Here the oracle runs the cells at the caps and tolerances of SETTINGS,
and the module pins what the device is then compared with:
  - the iteration counts respect the cap and reach it (KoDiag.solver_iter), and at the default cap no Newton solve reaches it;
  - a cap of 0 does no iteration: one mj_step is qvel + dt * (the cheaper of the warm start and qacc_smooth);
  - the unconverged iterates do not bifurcate: the spread of a twin started from qvel (1 + 1e-15), times ten, stays under the
    project's bars in every cell (the condition test_regimes_gpu._free_run asserts next to the device's run);
  - the settings bite: most envs end a control step more than 1e-9 in qvel away from the converged result."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402
from gym_kmanip_amd.model import compile_model  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_R, TOL_V  # noqa: E402

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")
# (solver_iterations, solver_tolerance) of the capped runs, shared with tests/test_solver_caps_gpu.py
SETTINGS = {"newton": ((0, 1e-8), (1, 1e-8), (3, 1e-8), (100, 1e-2)), "pgs": ((0, 1e-8), (1, 1e-8), (100, 1e-2))}
CONVERGED = (100, 1e-8)
BARS = {"qpos": TOL_Q, "qvel": TOL_V, "obs": TOL_Q, "reward": TOL_R}
BITE = 1e-9                  # an env "moves" if its qvel after one control step is further than this from the converged one
# the least share of envs a setting must move (newton, pgs), set below the measured counts of the docstring of
# test_the_settings_bite: all envs at caps 0 and 1, half of them at cap 3 and at the loose tolerance
BITE_SHARE = {(0, 1e-8): (1.0, 1.0), (1, 1e-8): (1.0, 1.0), (3, 1e-8): (0.5, None), (100, 1e-2): (0.5, 0.5)}

_MODELS, _RUNS = {}, {}


def capped_model(asset, solver, cap, tol):
    """The asset in the joint-delta action mode at a cap and a tolerance, no auto-reset; one object per argument set."""
    key = (asset, solver, cap, tol)
    if key not in _MODELS:
        _MODELS[key] = compile_model(mujoco_pin.qpos_spec(asset), auto_reset=False, solver=solver, solver_iterations=cap, solver_tolerance=tol)
    return _MODELS[key]


def actions(cm, n):
    """test_regimes_gpu._actions(cm, n, "random"): three steps of actions uniform in +-0.2."""
    return np.random.default_rng(3).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)


def control_steps(asset, solver, cap, tol, kind="zero", twin=False, nthreads=1):
    """The cells one control step on under a zero action (kind "zero") or three steps on under actions() ("random"), on the oracle
    of capped_model: a list of dict(qpos, qvel, obs, reward, done, mask, iters) per step, computed once.  twin: from qvel (1 + 1e-15).
    nthreads: the oracle's threads over the envs (an env's result does not depend on it)."""
    key = (asset, solver, cap, tol, kind, twin)
    if key not in _RUNS:
        cm = capped_model(asset, solver, cap, tol)
        qpos, qvel, ctrl, labels = R.cells(asset)
        n = len(labels)
        orc = R.loaded_oracle(cm, qpos, qvel * (1.0 + 1e-15) if twin else qvel, ctrl)
        acts = np.zeros((1, n, cm.act_dim), dtype=np.float32) if kind == "zero" else actions(cm, n)
        out = []
        for act in acts:
            obs, rew, done = orc.step(act, nthreads)
            q, v = orc.get_state()[:2]
            out.append(dict(qpos=q, qvel=v, obs=obs.copy(), reward=rew.copy(), done=done.copy(), mask=orc.get_diag()[0],
                            iters=np.array([d.solver_iter for d in orc.diag])))
        _RUNS[key] = out
    return _RUNS[key]


def _coupled_sub_steps(cm, asset):
    """[n]: in how many of the control step's sub-steps (zero action) each cell's Newton solve is the coupled, whole-problem one.
    The sub-steps are replayed one mj_step at a time (Oracle.physics_step, ctrl as before_step left it) and must end in the bits
    of the oracle's own control step."""
    qpos, qvel, ctrl, labels = R.cells(asset)
    n, nsub = len(labels), cm.desc.n_sub_steps
    orc = R.loaded_oracle(cm, qpos, qvel, ctrl)
    warm = orc.get_state()[3]
    orc.step(np.zeros((n, cm.act_dim), dtype=np.float32))
    q1, v1, c1 = orc.get_state()[:3]
    one = Oracle(cm, 1)
    count = np.zeros(n, dtype=np.int64)
    for e in range(n):
        q, v, w = qpos[e], qvel[e], warm[e]
        for _ in range(nsub):
            count[e] += bool(one.contact_mask(q)[0] & 0x000FFF00)
            q, v, w, bad = one.physics_step(q, v, c1[e], w, q, 1)[:4]
            assert not bad
        assert np.array_equal(q, q1[e]) and np.array_equal(v, v1[e]), (asset, labels[e], e)
    return count


# ----------------------------------------------------------------------------------------------------------------- iteration counts
@pytest.mark.parametrize("asset", ASSETS)
def test_iteration_counts_respect_the_cap_and_reach_it(asset):
    """KoDiag.solver_iter is the sum over the sub-steps of a control step.  It is 0 at cap 0; at most n_sub_steps * cap for PGS and
    for a Newton env whose solves are all coupled, with a second problem's `cap` more for every sub-step whose solve is the
    uncoupled pair (arm problem, then cube problem, each with a count of its own); at caps 1 and 3 at least one env of the asset
    sits AT its bound, under both solvers.  At the default cap no Newton env's SUM over the ten sub-steps and both problems
    reaches 100 (measured worst: SoloArm 73, DualArm 78, Torso 79), so no single Newton solve ends at the cap: Newton results at a cap
    of 1000 must be those of cap 100 (tests/test_solver_caps_gpu.py compares the bytes)."""
    labels = R.cells(asset)[3]
    print()
    for solver in SOLVERS:
        nsub = capped_model(asset, solver, *CONVERGED).desc.n_sub_steps
        for cap in (0, 1, 3):
            if (cap, 1e-8) not in SETTINGS[solver]:
                continue
            cm = capped_model(asset, solver, cap, 1e-8)
            it = control_steps(asset, solver, cap, 1e-8)[0]["iters"]
            bound = np.full(len(labels), nsub * cap)
            if solver == "newton" and cap:
                bound = cap * (2 * nsub - _coupled_sub_steps(cm, asset))
            print("%s %s cap %d: solver_iter %d..%d, %d of %d envs at their bound" % (asset, solver, cap, it.min(), it.max(), int((it == bound).sum()), len(it)))
            assert (it >= 0).all() and (it <= bound).all(), (solver, cap, [(labels[e], e, it[e], bound[e]) for e in np.where(it > bound)[0]])
            if cap == 0:
                assert not it.any()
            else:
                assert (it == bound).any(), (solver, cap)
    it = control_steps(asset, "newton", *CONVERGED)[0]["iters"]
    print("%s newton cap 100: worst solver_iter %d (ten sub-steps, both problems)" % (asset, it.max()))
    assert 0 < it.max() < 100
    it = np.stack([s["iters"] for s in control_steps(asset, "newton", *CONVERGED, "random")])
    print("%s newton cap 100: worst solver_iter %d over the three control steps of small random actions" % (asset, it.max()))
    assert it.max() < 100                                   # (the run the device repeats at cap 1000)
    it = control_steps(asset, "pgs", *CONVERGED)[0]["iters"]
    print("%s pgs cap 100: %d of %d envs ran 100 sweeps in every sub-step" % (asset, int((it == 1000).sum()), len(it)))
    assert (it == 1000).any()                               # PGS is at its cap by default


# ------------------------------------------------------------------------------------------------------------------- cap 0, closed form
def _cost(dyn, types, floss, a):
    d = a - dyn["qacc_smooth"]
    return 0.5 * d @ (dyn["M"] @ d) + (AO._rows(dyn["J"] @ a - dyn["aref"], dyn["R"], types, floss)[0].sum() if dyn["nefc"] else 0.0)


@pytest.mark.parametrize("asset", ASSETS)
def test_cap_zero_is_the_start_point(asset):
    """One mj_step (OracleRollout, nsub = 1) of every cell at solver_iterations = 0, Newton: qvel_next is qvel + dt * a with a the
    warm start where its cost (Oracle.dynamics' M, J, aref, R and qacc_smooth; the row costs of applied_oracle) is below
    qacc_smooth's, else qacc_smooth -- to the last bit, qacc_warm_next is that a, and both cases occur.  The rows' warm start is
    the converged model's (Oracle.after_reset: the solution without actuation, near the solution with it)."""
    cm = capped_model(asset, "newton", 0, 1e-8)
    qpos, qvel, ctrl, labels = R.cells(asset)
    n = len(labels)
    one = Oracle(cm, 1)
    warm = R.warm_start(capped_model(asset, "newton", *CONVERGED), Oracle(capped_model(asset, "newton", *CONVERGED), 1), qpos, qvel, ctrl)
    got = RO.OracleRollout(cm, 1).rollout(envs=np.zeros(n, dtype=np.int32), qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, nsub=1, nstep=1)
    assert not got["status"].any()
    kept = np.zeros(n, dtype=bool)
    for e in range(n):
        dyn = one.dynamics(qpos[e], qvel[e], ctrl[e])
        types, floss = one.constraint_rows(qpos[e], qvel[e])
        cw, cs = _cost(dyn, types, floss, warm[e]), _cost(dyn, types, floss, dyn["qacc_smooth"])
        assert abs(cw - cs) > 1e-9 * max(abs(cw), abs(cs)), (labels[e], e, cw, cs)          # no tie a rounding could decide
        kept[e] = cw < cs
        a = warm[e] if kept[e] else dyn["qacc_smooth"]
        assert np.array_equal(got["qacc_warm"][e, 0], a), (labels[e], e, kept[e])
        assert np.array_equal(got["qvel"][e, 0], qvel[e] + cm.desc.timestep * a), (labels[e], e, kept[e])
    print("\n%s cap 0: %d of %d cells keep the warm start, %d fall back to qacc_smooth" % (asset, int(kept.sum()), n, int((~kept).sum())))
    assert kept.any() and not kept.all()


# -------------------------------------------------------------------------------------------------------------------------- spread
def spread_table(asset, solver, cap, tol):
    """{cell: {quantity: worst |twin - oracle| over the three control steps of actions()}}."""
    labels = np.array(R.cells(asset)[3])
    a, b = control_steps(asset, solver, cap, tol, "random"), control_steps(asset, solver, cap, tol, "random", twin=True)
    out = {c: {k: 0.0 for k in BARS} for c in dict.fromkeys(labels)}
    for sa, sb in zip(a, b):
        for k in BARS:
            d = np.abs(sa[k] - sb[k]).reshape(len(labels), -1).max(axis=1)
            for c in out:
                out[c][k] = max(out[c][k], float(d[labels == c].max()))
    return out


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_unconverged_iterates_do_not_bifurcate(asset, solver):
    """test_regimes_gpu._free_run's condition, at every setting: three control steps of the small random actions, a twin oracle
    started from qvel (1 + 1e-15); ten times the spread of every cell stays under the bar of every quantity, no env diverges or
    sets done.  Measured worst over all assets, solvers and settings: qpos 2.8e-14, qvel 3.9e-12, obs 1.2e-12, reward 3.7e-11 --
    against bars of 1e-7, 1e-5, 1e-7 and 1e-6."""
    print()
    for cap, tol in SETTINGS[solver]:
        sp = spread_table(asset, solver, cap, tol)
        worst = {k: max(sp[c][k] for c in sp) for k in BARS}
        print("%s %s cap %d tol %.0e: worst spread %s" % (asset, solver, cap, tol, "  ".join("%s %.1e" % kv for kv in worst.items())))
        for c in sp:
            for k, bar in BARS.items():
                assert 10.0 * sp[c][k] <= bar, (cap, tol, c, k, sp[c][k])
        for s in control_steps(asset, solver, cap, tol, "random"):
            assert not s["done"].any() and np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all()


# ---------------------------------------------------------------------------------------------------------------------------- bite
@pytest.mark.parametrize("asset", ASSETS)
def test_the_settings_bite(asset):
    """Envs whose qvel after one control step (zero action) lies more than 1e-9 from the converged model's (cap 100, tolerance
    1e-8).  Measured (newton / pgs), of 47 SoloArm, 72 DualArm and 72 Torso envs:
        cap 0            47 47 / 72 72 / 72 72
        cap 1            47 47 / 72 72 / 72 72
        cap 3            38  - / 55  - / 56  -
        tolerance 1e-2   30 45 / 62 70 / 61 72
    BITE_SHARE asks for all envs at caps 0 and 1 and for half of them at cap 3 and at the loose tolerance."""
    n = len(R.cells(asset)[3])
    print()
    for si, solver in enumerate(SOLVERS):
        ref = control_steps(asset, solver, *CONVERGED)[0]["qvel"]
        for cap, tol in SETTINGS[solver]:
            moved = int((np.abs(control_steps(asset, solver, cap, tol)[0]["qvel"] - ref).max(axis=1) > BITE).sum())
            print("%s %s cap %d tol %.0e: %d of %d envs move" % (asset, solver, cap, tol, moved, n))
            assert moved >= BITE_SHARE[(cap, tol)][si] * n, (solver, cap, tol, moved, n)
