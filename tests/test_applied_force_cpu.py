"""The reference of the applied force (tests/tools/applied_oracle.py: the physics step with MuJoCo's qfrc_applied, restated in NumPy
over the CPU oracle), the tensor helpers of gym_kmanip_amd/applied.py and the wrapper's refusals, without a GPU.

The bars of the device parity (tests/test_applied_force_gpu.py) are the project's TOL_Q / TOL_V; here the reference must agree with
the C oracle at zero force, and with itself under a 1e-15 relative change of qvel, to a tenth of them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_V  # noqa: E402

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_restatement_equals_the_oracle_at_zero_force(asset, solver):
    """Ten sub-steps from every regime cell with tau = 0 against Oracle.physics_step: a tenth of TOL_Q / TOL_V.  Measured (worst over
    the assets, absolute): newton qpos 1.8e-15, qvel 2.6e-13; pgs qpos 8.1e-16, qvel 1.5e-13."""
    from oracle.oracle import Oracle
    cm = R.model(asset, solver)
    qpos, qvel, ctrl, labels = R.cells(asset)
    one = Oracle(cm, 1)
    warm = R.warm_start(cm, one, qpos, qvel, ctrl)
    wq = wv = 0.0
    for e in range(len(labels)):
        q1, v1, _, bad, _, _, _ = one.physics_step(qpos[e], qvel[e], ctrl[e], warm[e], qpos[e], cm.desc.n_sub_steps)
        assert not bad, (labels[e], e)
        q2, v2, _ = AO.physics_step(cm, one, qpos[e], qvel[e], ctrl[e], warm[e], np.zeros(cm.nv))
        wq, wv = max(wq, float(np.abs(q1 - q2).max())), max(wv, float(np.abs(v1 - v2).max()))
    print("\n%s %s: restatement - oracle at zero force: qpos %.1e qvel %.1e" % (asset, solver, wq, wv))
    assert wq <= 0.1 * TOL_Q and wv <= 0.1 * TOL_V, (wq, wv)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_twin_spread_under_the_test_forces(asset, solver):
    """The restatement's own error under the test forces: ten times the spread between the run and its twin (qvel * (1 + 1e-15))
    stays below the bars (measured: qpos at most 1.3e-15, qvel 4.2e-13).  And the forces matter: every env's qpos moves by more than 1e-5 against the unforced oracle step, so no
    parity test can pass without the feature."""
    run = AO.cell_runs(asset, solver)
    sq = float(np.abs(run["ref"]["qpos"] - run["twin"]["qpos"]).max())
    sv = float(np.abs(run["ref"]["qvel"] - run["twin"]["qvel"]).max())
    print("\n%s %s: twin spread qpos %.1e qvel %.1e" % (asset, solver, sq, sv))
    assert 10.0 * sq <= TOL_Q and 10.0 * sv <= TOL_V, (sq, sv)
    assert (run["ref"]["mask"] == run["twin"]["mask"]).all()
    orc = R.loaded_oracle(run["cm"], run["qpos"], run["qvel"], run["ctrl"])
    orc.step(np.zeros((len(run["labels"]), run["cm"].act_dim), dtype=np.float32))
    moved = np.abs(run["ref"]["qpos"] - orc.get_state()[0]).max(axis=1)
    assert (moved > 1e-5).all(), float(moved.min())
    assert (run["ref"]["ctrl"] == orc.get_state()[2]).all()


def test_hover_and_mirrored_free_fall():
    """Home pose, cube 0.3 m above the table: +m g on the cube's z dof leaves its z and vz unchanged to the bit; 2 m g mirrors free
    fall (measured: -+2.114e-3 m in one control step, exactly mirrored; the bar of 1e-14 allows for the rounding of z + dt vz at
    z = 1.1 m in ten sub-steps of either run)."""
    from oracle.oracle import Oracle
    cm = R.model("solo_arm")
    nl = cm.nlink
    one = Oracle(cm, 1)
    qpos, qvel, ctrl = AO.hover_state(cm)
    warm = one.after_reset(qpos, qvel, ctrl)
    mg = cm.desc.cube_mass * abs(cm.desc.gravity[2])
    dz = {}
    for k in (0.0, 1.0, 2.0):
        tau = np.zeros(cm.nv)
        tau[nl + 2] = k * mg
        q, v, _ = AO.physics_step(cm, one, qpos, qvel, ctrl, warm, tau)
        dz[k] = (q[nl + 2] - qpos[nl + 2], v[nl + 2])
    print("\nhover: dz %r" % (dz,))
    assert dz[1.0] == (0.0, 0.0)
    assert dz[0.0][0] < -1.9e-3 and abs(dz[2.0][0] + dz[0.0][0]) <= 1e-14 and abs(dz[2.0][1] + dz[0.0][1]) <= 1e-13, dz


def test_cube_and_site_wrench_against_numpy():
    import torch
    from gym_kmanip_amd import applied
    cm = R.model("dual_arm")
    nl, nv, n = cm.nlink, cm.nv, 5
    rng = np.random.default_rng(2)
    qpos = rng.normal(size=(n, cm.nq))
    qpos[:, nl + 3:nl + 7] *= rng.uniform(0.5, 2.0, (n, 1))              # unnormalised quaternions: the helper normalises
    qpos[0, nl + 3:nl + 7] = [1.0, 0.0, 0.0, 0.0]
    f, t = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    out = applied.cube_wrench(cm, torch.from_numpy(qpos), force=torch.from_numpy(f), torque=torch.from_numpy(t))
    assert tuple(out.shape) == (n, nv) and out.dtype == torch.float64
    want = np.zeros((n, nv))
    for e in range(n):
        Rm = R.quat2mat(qpos[e, nl + 3:nl + 7] / np.linalg.norm(qpos[e, nl + 3:nl + 7]))
        want[e, nl:nl + 3] = f[e]
        want[e, nl + 3:nl + 6] = Rm.T @ t[e]
    assert np.abs(out.numpy() - want).max() < 1e-14
    assert np.array_equal(out.numpy()[0, nl + 3:nl + 6], t[0])           # the identity orientation: world = body
    assert np.abs(out.numpy()[1, nl + 3:nl + 6] - t[1]).max() > 1e-3     # a rotated cube: not the world torque
    # accumulation into `out`, broadcast of a (3,) vector, None = zero
    again = applied.cube_wrench(cm, torch.from_numpy(qpos), force=(0.0, 0.0, 1.0), out=out)
    assert again is out
    want[:, nl + 2] += 1.0
    assert np.abs(out.numpy() - want).max() < 1e-14
    assert not applied.cube_wrench(cm, torch.from_numpy(qpos)).any()
    # site_wrench: jacp^T f + jacr^T tau
    jp, jr = rng.normal(size=(n, 2, 3, nv)), rng.normal(size=(n, 2, 3, nv))
    kin = {"site_jacp": torch.from_numpy(jp), "site_jacr": torch.from_numpy(jr)}
    for arm in (0, 1):
        got = applied.site_wrench(cm, kin, arm, force=torch.from_numpy(f), torque=torch.from_numpy(t))
        ref = np.einsum("nij,ni->nj", jp[:, arm], f) + np.einsum("nij,ni->nj", jr[:, arm], t)
        assert np.abs(got.numpy() - ref).max() < 1e-13
    base = torch.ones((n, nv), dtype=torch.float64)
    got = applied.site_wrench(cm, kin, 1, force=torch.from_numpy(f), out=base)
    assert got is base and np.abs(got.numpy() - 1.0 - np.einsum("nij,ni->nj", jp[:, 1], f)).max() < 1e-13
    with pytest.raises(ValueError):
        applied.cube_wrench(cm, torch.from_numpy(qpos), force=torch.zeros(n, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        applied.site_wrench(cm, kin, 0, force=torch.from_numpy(f), out=torch.zeros(n, nv - 1, dtype=torch.float64))


class _CountingLib:
    """Stands in for the loaded library: counts the bind calls and what they were given."""
    def __init__(self):
        self.calls = []

    def kmanip_bind_applied_force(self, h, p):
        self.calls.append(p)
        return 0


def test_wrapper_refuses_before_the_library_is_called():
    """bind_applied_force on a handle object built without a device: whatever is not a float64 [num_envs, nv] tensor on the handle's
    device raises before the C call and leaves the binding as it was; None reaches the library as NULL.  (Wrong dtype and shape ON
    the device: tests/test_applied_force_gpu.py.)"""
    import torch
    from gym_kmanip_amd.env_hip import KManipEnvHip
    from gym_kmanip_amd.lib import KManipError
    cm = R.model("solo_arm")
    env = object.__new__(KManipEnvHip)
    env.cm, env.num_envs, env.device, env.h, env.L, env.applied_force = cm, 4, torch.device("cuda", 0), None, _CountingLib(), None
    for bad in (torch.zeros((4, cm.nv), dtype=torch.float64), torch.zeros((4, cm.nv), dtype=torch.float32),
                torch.zeros((3, cm.nv), dtype=torch.float64), np.zeros((4, cm.nv)), [[0.0] * cm.nv] * 4):
        with pytest.raises(KManipError):
            env.bind_applied_force(bad)
    assert env.L.calls == [] and env.applied_force is None
    assert env.bind_applied_force(None) is None and env.L.calls == [None] and env.applied_force is None
    env.h = None                                             # (nothing to destroy)


def test_the_abi_names_the_entry_point():
    from gym_kmanip_amd import lib
    assert "kmanip_bind_applied_force" in lib.EXPORTS
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "kmanip.h")) as f:
        assert "KMANIP_API int kmanip_bind_applied_force(KHandle h, const double* qfrc_dev);" in f.read()
