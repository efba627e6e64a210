"""The IK where the default-goal fixtures never go: a coordinate pressed onto its bound, goals 0.3-1.5 m away (hundreds of
evaluations, status 0), starts on and next to bounds, no motion, rotations up to pi, infeasible starts, and runs capped after
k evaluations, which pin the path of the iterates and not only its end.  tests/golden/ik_edges_<env>.npz holds what the real
scipy.optimize.least_squares answers (tests/tools/make_golden_ik_edges.py); here the fixtures' own conditions, a live
SciPy re-run, and the C oracle against every row.  CPU only.

Worst |q - q_scipy| of the oracle per category, rad (Solo / Dual / Torso), SciPy 1.15.3; nfev and status differ nowhere:
  pressed      2e-14 / 7e-15 / 6e-15    far          5e-10 / 2e-10 / 4e-10    on_bound   2e-14 / 8e-15 / 9e-15
  near_bound   3e-14 / 9e-10 / 9e-14    still        2e-16 / 2e-16 / 4e-16    infeasible 0
  big_rotation 7e-13 / 3e-14 / 1e-14    capped       3e-13 / 6e-13 / 6e-14
Before the oracle's Jacobi SVD kept the exact small couplings of a pressed column the SoloArm's pressed rows
missed the bar: 1.4e-4 rad, nfev off in 3 of 48."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

import ik_edges as E  # noqa: E402
from conftest import ENVS3  # noqa: E402
from gym_kmanip_amd.model import compile_model  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402


@pytest.mark.parametrize("env", ENVS3)
def test_fixture_conditions(env):
    E.check_fixture(env, compile_model(env), E.load(env))


def test_fixtures_hold_every_status():
    """-2 (infeasible start), 0 (cap), 1 (gtol), 2 (ftol), 3 (xtol); 4 (ftol and xtol at once) is kept where it turns up."""
    assert set(np.concatenate([E.load(env)["status"] for env in ENVS3]).tolist()) >= {-2, 0, 1, 2, 3}


@pytest.mark.parametrize("env", ENVS3)
def test_live_scipy_reproduces_every_eighth_row(env):
    """Guards the fixture against drift of the generator and of oracle/ik_scipy.py: bit for bit."""
    from make_golden_ik_edges import ARMS, solve
    g = E.load(env)
    for i in range(0, len(g["arm"]), 8):
        arm = int(g["arm"][i]); n = compile_model(env).desc.arm_nq[arm]
        q, after, nfev, status = solve(env, arm, dict(ARMS[env])[arm], g["qpos"][i], g["goal_pos"][i], g["goal_quat"][i],
                                       int(g["max_nfev"][i]))
        assert np.array_equal(q, g["q_out"][i][:n]) and np.array_equal(after, g["qpos_after"][i]), i
        assert nfev == g["nfev"][i] and status == g["status"][i], i


@pytest.mark.parametrize("env", ENVS3)
def test_oracle_against_every_row(env):
    g = E.load(env)
    rows = len(g["arm"])
    q = np.zeros((rows, 7)); after = np.zeros_like(g["qpos"]); nfev = np.zeros(rows, dtype=np.int32); st = np.zeros(rows, dtype=np.int32)
    for arm, cap, idx in E.groups(g):
        o = Oracle(compile_model(env, ik_max_nfev=cap), 1)
        n = o.desc.arm_nq[arm]
        for i in idx:
            q[i, :n], after[i], nfev[i], st[i] = o.ik(arm, g["qpos"][i], g["goal_pos"][i], g["goal_quat"][i])
    E.compare(compile_model(env), g, q, after, nfev, st, "oracle %s" % env)
