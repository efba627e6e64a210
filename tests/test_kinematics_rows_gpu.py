"""kmanip_kinematics_rows (KManipEnvHip.kinematics_at) on the device (run with -m gpu on an MI355X): kinematics() at rows the caller
passes.  The invariant against kinematics() bit for bit, the regime cells handed over as rows against tests/tools/kin_oracle.py under
the bars of tests/test_kinematics_cpu.py, rows that outnumber, repeat and permute envs, per-env parameters by index, field
selection, the two status values, a PGS handle, the handle left untouched and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import kin_oracle as KO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_kinematics_gpu import _cells, _compare, _device, _host, _report, _torch  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
# (asset, mode) of the invariant test: together they launch every sitekin object (tests/test_site_cost_cpu.py checks that)
LAUNCH_ROWS = [("solo_arm", "plain"), ("dual_arm", "plain"), ("torso", "plain"), ("solo_arm", "params"), ("dual_arm", "params")]


def _equal(a, b, rows_a=None, rows_b=None):
    torch = _torch()
    pick = lambda t, r: t if r is None else t[r]
    return [k for k in a if not torch.equal(pick(a[k], rows_a), pick(b[k], rows_b))]


def _masses(cm, n):
    return np.array([cm.desc.cube_mass * (1.0 + 0.25 * (e % 5)) for e in range(n)])


@pytest.mark.parametrize("asset,mode", LAUNCH_ROWS)
def test_the_invariant_every_input_null_is_kinematics(asset, mode):
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    if mode == "params":
        dev.set_env_params(cube_mass=_masses(cm, len(labels)))
    a, b = dev.kinematics(), dev.kinematics_at()
    dev.k_close()
    assert set(a) == set(b) and _equal(a, b) == [] and not b["status"].any()
    assert tuple(b["qM"].shape) == (len(labels), cm.nv, cm.nv) and b["qM"].abs().max() > 0


@pytest.mark.parametrize("asset", ASSETS)
def test_the_cells_as_rows_of_a_handle_that_holds_reset_states(asset):
    """A 2-env handle after a reset gets the cells as rows (row r names env r % 2): against the oracle under the bars, and bit for
    bit against kinematics() of a handle that stores those states."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    _, dec, _ = KO.cell_decodes(asset)
    n = len(labels)
    small = env_hip.KManipEnvHip(cm, num_envs=2, seed=1)
    small.k_reset()
    idx = torch.arange(n, dtype=torch.int32, device="cuda") % 2
    rows = small.kinematics_at(envs=idx, qpos=torch.from_numpy(qpos).cuda(), qvel=torch.from_numpy(qvel).cuda())
    small.k_close()
    store = _device(cm, qpos, qvel, ctrl, warm)
    full = store.kinematics()
    store.k_close()
    assert _equal(rows, full) == []
    k = _host(rows)
    figures, bad = [], []
    for e, o in enumerate(dec):
        bad += _compare(k, e, o, qvel[e], (labels[e], e), figures)
    _report(asset + " as rows", figures)
    assert not bad, bad


@pytest.mark.parametrize("asset,n", [("solo_arm", 5), ("dual_arm", 3)])
def test_rows_outnumber_repeat_and_permute_envs(asset, n):
    """A 2-env handle, n rows: a row alone, in the batch and in the reversed batch gives the same bits; a repeated index repeats
    the row; rows without a given state take the named env's."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    dev = env_hip.KManipEnvHip(cm, num_envs=2, seed=1)
    dev.k_reset()
    q, v = torch.from_numpy(qpos[:n].copy()).cuda(), torch.from_numpy(qvel[:n].copy()).cuda()
    idx = torch.tensor([1, 0, 1, 1, 0][:n], dtype=torch.int32, device="cuda")
    batch = dev.kinematics_at(envs=idx, qpos=q, qvel=v)
    rev = dev.kinematics_at(envs=idx.flip(0), qpos=q.flip(0).contiguous(), qvel=v.flip(0).contiguous())
    assert _equal(batch, rev, None, torch.arange(n - 1, -1, -1, device="cuda")) == []
    for r in range(n):
        one = dev.kinematics_at(envs=idx[r:r + 1], qpos=q[r:r + 1], qvel=v[r:r + 1])
        assert _equal(one, batch, None, slice(r, r + 1)) == [], r
    stored = dev.kinematics()
    named = dev.kinematics_at(envs=idx)
    assert _equal(named, stored, None, idx.long()) == [] and not named["status"].any()
    dev.k_close()


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_a_row_takes_the_named_envs_parameters(asset):
    torch = _torch()
    from gym_kmanip_amd import env_hip
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    nl = cm.nlink
    dev = env_hip.KManipEnvHip(cm, num_envs=2, seed=1)
    dev.k_reset()
    mass = np.array([2.0, 3.5]) * cm.desc.cube_mass
    dev.set_env_params(cube_mass=mass)
    idx = [1, 0, 0, 1, 1]
    k = _host(dev.kinematics_at(envs=idx, qpos=torch.from_numpy(qpos[:5].copy()).cuda(), qvel=torch.from_numpy(qvel[:5].copy()).cuda(),
                                fields=("qM", "qfrc_bias", "status")))
    dev.k_close()
    assert not k["status"].any()
    for r, e in enumerate(idx):
        assert np.array_equal(np.diag(k["qM"][r])[nl:nl + 3], [mass[e]] * 3), r
        assert np.allclose(np.diag(k["qM"][r])[nl + 3:], np.array(cm.desc.cube_inertia) * mass[e] / cm.desc.cube_mass, rtol=1e-14, atol=0)
    assert k["qfrc_bias"][0, nl + 2] != k["qfrc_bias"][1, nl + 2]


def test_field_selection_and_a_reused_out():
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells("dual_arm")
    dev = _device(cm, qpos, qvel, ctrl, warm)
    q = torch.from_numpy(qpos[::-1].copy()).cuda()
    full = dev.kinematics_at(qpos=q)
    light = dev.kinematics_at(qpos=q, fields=[k for k in full if k not in ("qM", "qfrc_bias")])
    assert "qM" not in light and _equal(light, full) == []
    mine = {"status": torch.full_like(full["status"], 7), "site_jacp": torch.zeros_like(full["site_jacp"]), "qM": torch.zeros_like(full["qM"])}
    again = dev.kinematics_at(qpos=q, out=mine)
    assert again is mine and _equal(again, full) == []
    with pytest.raises(ValueError):
        dev.kinematics_at(fields=["nonsense"])
    dev.k_close()


def test_status_two_for_an_index_out_of_range():
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm")
    dev = _device(cm, qpos, qvel, ctrl, warm)
    n = len(labels)
    idx = [3, -1, 5, n, 0]
    k = dev.kinematics_at(envs=idx)
    good = dev.kinematics()
    dev.k_close()
    assert k["status"].tolist() == [0, 2, 0, 2, 0]
    for r in (1, 3):
        assert all(not k[key][r].any() for key in KO.FIELDS)
    assert _equal(k, good, [0, 2, 4], [3, 5, 0]) == []


def test_status_one_for_a_non_finite_state_given_or_stored():
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm")
    dev = _device(cm, qpos, qvel, ctrl, warm)
    clean = dev.kinematics_at()
    n = len(labels)
    qn = torch.from_numpy(qpos.copy()).cuda()
    qn[6, 2] = float("nan")
    g = dev.kinematics_at(qpos=qn)
    keep = torch.arange(n, device="cuda") != 6
    assert g["status"][6] == 1 and int(g["status"].sum()) == 1 and all(not g[key][6].any() for key in KO.FIELDS)
    assert _equal(g, clean, keep, keep) == []
    # a NaN in a stored qvel: status 1 with qvel=None, none with a qvel given
    vn = qvel.copy()
    vn[9, 1] = np.nan
    dev.set_state(qvel=vn)
    s = dev.kinematics_at()
    keep = torch.arange(n, device="cuda") != 9
    assert s["status"][9] == 1 and int(s["status"].sum()) == 1 and _equal(s, clean, keep, keep) == []
    given = dev.kinematics_at(qvel=torch.from_numpy(qvel).cuda())
    assert not given["status"].any() and _equal(given, clean) == []
    dev.k_close()


def test_a_pgs_handle_returns_the_newton_handles_bits():
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells("solo_arm")
    newton = _device(cm, qpos, qvel, ctrl, warm)
    pgs = _device(R.model("solo_arm", "pgs"), qpos, qvel, ctrl, warm)
    idx = torch.arange(len(labels) - 1, -1, -1, dtype=torch.int32, device="cuda")
    a, b = newton.kinematics_at(envs=idx), pgs.kinematics_at(envs=idx)
    newton.k_close(); pgs.k_close()
    assert _equal(a, b) == [] and not a["status"].any() and a["qM"].abs().max() > 0


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """test_kinematics_gpu's twin-handle test with kinematics_at (rows with given states) in place of kinematics."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, len(labels), cm.act_dim)).astype(np.float32)
    q = torch.from_numpy(qpos[::-1].copy()).cuda()
    for s in range(3):
        before = a.state_tensors()
        diag = a.get_diag()
        a.kinematics_at(qpos=q)
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), s
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), s
        act = torch.from_numpy(acts[s]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), s
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), s
        assert torch.equal(a.sim_time, b.sim_time)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_diag(), b.get_diag())), s
    a.k_close(); b.k_close()


def test_refusals_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.lib import KKinDev, KKinRowsIn
    dev = env_hip.KManipEnvHip(R.model("solo_arm"), num_envs=4, seed=0)
    dev.k_reset()
    call, err = dev.L.kmanip_kinematics_rows, dev.L.kmanip_last_error
    ki, kd = KKinRowsIn(), KKinDev()
    status = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    kd.status = status.data_ptr()
    assert call(None, C.byref(ki), 4, C.byref(kd), None) != 0 and b"kmanip_kinematics_rows: null handle" in err(None)
    assert call(dev.h, None, 4, C.byref(kd), None) != 0 and b"KKinRowsIn pointer is NULL" in err(dev.h)
    assert call(dev.h, C.byref(ki), 4, None, None) != 0 and b"KKinDev pointer is NULL" in err(dev.h)
    assert call(dev.h, C.byref(ki), -1, C.byref(kd), None) != 0 and b"n is negative" in err(dev.h)
    assert call(dev.h, C.byref(ki), 5, C.byref(kd), None) != 0 and b"more rows than envs" in err(dev.h)
    torch.cuda.synchronize()
    assert status.eq(9).all()                                               # nothing was launched
    assert call(dev.h, C.byref(ki), 0, C.byref(kd), None) == 0              # n == 0 succeeds
    assert call(dev.h, C.byref(ki), 4, C.byref(KKinDev()), None) == 0       # every field NULL: succeeds, does nothing
    dev.step_flat(torch.zeros((4, dev.cm.act_dim), dtype=torch.float32, device="cuda"))
    assert not dev.done.cpu().numpy().any() and not dev.kinematics_at()["status"].any()
    dev.k_close()
