"""kmanip_forward and the finite-difference derivatives on the device (run with -m gpu on an MI355X).

The rows are the regime cells of tests/tools/regime_states.py (47 for the single arm, 72 for the two-arm models) sent as CALLER rows
to handles of 2 envs: more rows than envs, not a multiple of the 4 / 2 rows a wave holds.  The reference is
tests/tools/forward_oracle.py (applied_oracle.forces_decode per row), the bars and normalisers are those of tests/test_forces_cpu.py
(tests/test_forward_cpu.py re-asserts them for these rows); masks, bits and status are compared exactly.  The derivative bar is
bar x normaliser / eps, derived in tests/test_forward_cpu.py.  Worst figures measured on an MI355X: DESIGN.md section 26."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import force_oracle as FO  # noqa: E402
import forward_oracle as FW  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_forces_cpu import BAR_CONTACT_FORCE, BAR_QACC, BAR_QFRC_ACTUATOR, BAR_QFRC_CONSTRAINT  # noqa: E402
from test_forces_gpu import FLOAT_FIELDS, _cells, _compare, _device, _host, _report  # noqa: E402
from test_forward_cpu import EPS, fd_bars  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
PARAMS = dict(cube_mass=2.0, cube_friction=0.5, cube_frictionloss=0.0, kp_scale=1.3)      # (cube_mass: a factor on the model's)
# forward() with every input None against forces() on the same handle: the bytes were equal in the first measurement on an
# MI355X (every field, every mode below), so equality is what is asserted
IDENTITY_BYTES_EQUAL = True


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _t(x, dtype=None):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _fresh(cm, n, seed=0):
    from gym_kmanip_amd import env_hip
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=seed)
    dev.k_reset()
    return dev


def _params(cm):
    return dict(PARAMS, cube_mass=PARAMS["cube_mass"] * cm.desc.cube_mass)


def _rows(asset, warm=False):
    """The asset's cells as keyword arguments of forward() (device tensors; warm: the cells' warm start, else zeros)."""
    cm, qpos, qvel, ctrl, w, labels = _cells(asset)
    return dict(qpos=_t(qpos), qvel=_t(qvel), ctrl=_t(ctrl), warm=_t(w if warm else np.zeros_like(w)))


_FORCED = {}


def _forced_decodes(asset):
    """forward_oracle.row of every cell under the test forces, computed once."""
    from oracle.oracle import Oracle
    if asset not in _FORCED:
        cm, qpos, qvel, ctrl, _, labels = _cells(asset)
        tau = AO.draw_test_forces(cm, len(labels))
        orc = Oracle(cm, 1)
        _FORCED[asset] = (tau, [FW.row(cm, orc, qpos[e], qvel[e], ctrl[e], None, tau[e]) for e in range(len(labels))])
    return _FORCED[asset]


def _same(f, g, rows_f=None, rows_g=None):
    """Names of the fields whose rows differ in any bit."""
    torch = _torch()
    bad = []
    for k in f:
        a = f[k] if rows_f is None else f[k][rows_f]
        b = g[k] if rows_g is None else g[k][rows_g]
        if not torch.equal(a, b):
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------------------ more rows than envs
@pytest.mark.parametrize("forced", [False, True], ids=["plain", "forced"])
@pytest.mark.parametrize("asset", ASSETS)
def test_more_rows_than_envs_against_the_oracle(asset, forced):
    cm, qpos, qvel, ctrl, _, labels = _cells(asset)
    n = len(labels)
    if forced:
        tau, dec = _forced_decodes(asset)
    else:
        tau, dec = None, FO.cell_decodes(asset)[1]
    dev = _fresh(cm, 2)
    before = dev.state_tensors()
    f = _host(dev.forward(envs=np.arange(n) % 2, qfrc_applied=None if tau is None else _t(tau), **_rows(asset)))
    after = dev.state_tensors()
    dev.k_close()
    assert n > 2 and f["qacc"].shape == (n, cm.nv) and f["contact_bit"].shape[0] == n
    assert all(_torch().equal(before[k], after[k]) for k in before)
    figures, bad = [], []
    for e, o in enumerate(dec):
        bad += _compare(cm, f, e, o, (labels[e], e), figures)
    _report("%s, %d rows on 2 envs%s" % (asset, n, " under the test forces" if forced else ""), figures)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------ identity
def _diff_under_bars(f, g):
    """Largest normalised |f - g| per quantity over the rows, against the forces bars (normalisers from f itself)."""
    bad = []
    for k in ("contact_bit", "contact_mask", "status"):
        if not np.array_equal(f[k], g[k]):
            bad.append(k)
    sq = np.maximum(1.0, np.abs(f["qacc"]).max(axis=1)); sf = np.maximum(1.0, np.abs(f["qfrc_constraint"]).max(axis=1))
    sa = np.maximum(1.0, np.abs(f["qfrc_actuator"]).max(axis=1))
    d = dict(qacc=(np.abs(f["qacc"] - g["qacc"]).max(axis=1) / sq).max(), qfrc_constraint=(np.abs(f["qfrc_constraint"] - g["qfrc_constraint"]).max(axis=1) / sf).max(),
             qfrc_actuator=(np.abs(f["qfrc_actuator"] - g["qfrc_actuator"]).max(axis=1) / sa).max(),
             contact_force=(np.abs(f["contact_force"] - g["contact_force"]).max(axis=(1, 2)) / sf).max(),
             geometry=max(float(np.abs(f[k] - g[k]).max()) for k in ("contact_frame", "contact_pos", "contact_dist")))
    bars = dict(qacc=BAR_QACC, qfrc_constraint=BAR_QFRC_CONSTRAINT, qfrc_actuator=BAR_QFRC_ACTUATOR, contact_force=BAR_CONTACT_FORCE, geometry=1e-12)
    return bad + [(k, v, bars[k]) for k, v in d.items() if not v <= bars[k]], d


# tests/test_forward_cpu.py checks that these rows launch every k_forward object the Makefile compiles.
IDENTITY_ROWS = [(a, m) for a in ASSETS for m in ("plain", "bound", "params", "params+bound")] + [("solo_arm", "ranges")]


@pytest.mark.parametrize("asset,mode", IDENTITY_ROWS)
def test_every_input_none_is_forces(asset, mode):
    """On a stepped handle holding every cell, forward() computes what forces() computes: the default, the applied-force, the
    parameter and the combined build of both link classes; per-env parameters explicit (different per env) and in ranges mode."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    n = len(labels)
    dev = _device(cm, qpos, qvel, ctrl, warm)
    if "params" in mode:
        k = np.arange(n) % 3
        dev.set_env_params(cube_mass=cm.desc.cube_mass * (1.0 + 0.5 * k), cube_friction=0.5 + 0.2 * k, cube_frictionloss=0.01 * k, kp_scale=1.0 + 0.15 * k)
    if mode == "ranges":
        dev.set_env_param_ranges(cube_mass=(0.5 * cm.desc.cube_mass, 2.0 * cm.desc.cube_mass), cube_friction=(0.4, 1.2), kp_scale=(0.8, 1.3))
        dev.k_reset()
        dev.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, step=np.zeros(n, dtype=np.int32))
        p = dev.get_env_params()["cube_mass"].cpu().numpy()
        assert len(np.unique(p)) == n
    if "bound" in mode:
        dev.bind_applied_force(_t(AO.draw_test_forces(cm, n)))
    act = np.random.default_rng(5).uniform(-0.2, 0.2, (n, cm.act_dim)).astype(np.float32)
    dev.step_flat(torch.from_numpy(act).cuda())
    want, got = dev.forces(), dev.forward()
    dev.k_close()
    assert not want["status"].any() and want["contact_mask"].ne(0).any()
    same = _same(want, got)
    bad, d = _diff_under_bars(_host(want), _host(got))
    print("\n%s %s: forward() vs forces(): %s; largest normalised differences %s"
          % (asset, mode, "bytes equal" if not same else "fields that differ: %s" % same, "  ".join("%s %.1e" % kv for kv in d.items())))
    assert not bad, bad
    if IDENTITY_BYTES_EQUAL:
        assert not same, same


# ------------------------------------------------------------------------------------------------------- bit-exact within the kernel
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_rows_are_independent_of_their_place_and_their_neighbours(asset):
    """Rows permuted give outputs permuted; a row repeated five times gives five identical rows; overrides on handle A give the bits
    of no overrides on handle B, whose state was written with set_state_tensors (warm start and ctrl included)."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    n = len(labels)
    rows = _rows(asset, warm=True)
    tau = _t(AO.draw_test_forces(cm, n))
    a = _fresh(cm, 2)
    envs = torch.arange(n, dtype=torch.int32, device="cuda") % 2
    f = a.forward(envs=envs, qfrc_applied=tau, **rows)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    g = a.forward(envs=envs[perm], qfrc_applied=tau[perm], **{k: v[perm].contiguous() for k, v in rows.items()})
    assert not f["status"].any() and _same(f, g, rows_f=perm) == []
    e = labels.index("G2")
    five = torch.full((5,), e, dtype=torch.int64, device="cuda")
    h = a.forward(envs=envs[five], qfrc_applied=tau[five], **{k: v[five].contiguous() for k, v in rows.items()})
    assert _same(f, h, rows_f=five) == [] and h["contact_mask"][0] != 0
    # the same rows as the stored state of a handle of n envs, no overrides; and as overrides on a handle that stores something else
    b = _fresh(cm, n, seed=4)
    b.set_state_tensors(qpos=rows["qpos"], qvel=rows["qvel"], ctrl=rows["ctrl"], warm=rows["warm"])
    stored = b.forward()
    c = _fresh(cm, n, seed=5)
    over = c.forward(**rows)
    plain = a.forward(envs=envs, **rows)
    assert _same(stored, over) == [] and _same(stored, plain) == []
    b.bind_applied_force(tau)
    assert _same(b.forward(), f) == [] and _same(b.forward(qfrc_applied=tau), f) == []
    assert _same(b.forward(qfrc_applied=torch.zeros_like(tau)), stored) == []          # a given row replaces the bound one
    for d in (a, b, c):
        d.k_close()


# --------------------------------------------------------------------------------------------------------------- per-env parameters
@pytest.mark.parametrize("asset", ASSETS)
def test_a_row_takes_the_parameters_of_the_env_it_names(asset):
    """A 2-env handle with cube mass x 2, friction 0.5, friction loss 0 and kp scale 1.3 on env 1 only; the same grasp row is sent
    once per env (and twice more, interleaved): each matches the oracle of its own model, and the two differ."""
    from gym_kmanip_amd.model import env_param_defaults, with_env_params
    from oracle.oracle import Oracle
    cm, qpos, qvel, ctrl, _, labels = _cells(asset)
    p = _params(cm)
    base = env_param_defaults(cm)
    cmp_ = with_env_params(cm, **p)
    dev = _fresh(cm, 2)
    dev.set_env_params(**{k: np.array([base[k], p[k]]) for k in p})
    figures, bad = [], []
    for cell in ("G1", "G2"):
        e = labels.index(cell)
        rep = lambda x: _t(np.tile(x[e], (4, 1)))
        f = _host(dev.forward(envs=[0, 1, 1, 0], qpos=rep(qpos), qvel=rep(qvel), ctrl=rep(ctrl), warm=_t(np.zeros((4, cm.nv)))))
        o0 = FW.row(cm, Oracle(cm, 1), qpos[e], qvel[e], ctrl[e])
        o1 = FW.row(cmp_, Oracle(cmp_, 1), qpos[e], qvel[e], ctrl[e])
        for r, (m, o) in enumerate(((cm, o0), (cmp_, o1), (cmp_, o1), (cm, o0))):
            bad += _compare(m, f, r, o, (cell, "row %d" % r), figures)
        assert np.array_equal(f["qacc"][0], f["qacc"][3]) and np.array_equal(f["qacc"][1], f["qacc"][2])
        assert np.abs(f["qacc"][0] - f["qacc"][1]).max() > 1e-3 and not np.array_equal(f["qfrc_actuator"][0], f["qfrc_actuator"][1])
    dev.k_close()
    _report(asset + ", env 1 with parameters", figures)
    assert not bad, bad


# -------------------------------------------------------------------------------------------------------------------- launch shapes
@pytest.mark.parametrize("asset,counts", [("solo_arm", (1, 3, 5, 47)), ("dual_arm", (1, 3, 72))])
def test_launch_shapes_leave_the_tails_alone(asset, counts):
    """Four rows per wave (single arm) and two (two-arm models): 1, 3, 5 rows and every cell, outputs over-allocated by four rows
    of a sentinel that must survive; every row equals the same row of the largest call, bit for bit."""
    torch = _torch()
    cm, qpos, qvel, ctrl, _, labels = _cells(asset)
    rows = _rows(asset)
    dev = _fresh(cm, 2)
    full = dev.forward(envs=np.arange(len(labels)) % 2, **rows)
    assert len(labels) == counts[-1]
    for n in counts:
        store = {k: torch.full((n + 4,) + tuple(v.shape[1:]), 77, dtype=v.dtype, device="cuda") for k, v in full.items()}
        out = dev.forward(envs=np.arange(n) % 2, out={k: v[:n] for k, v in store.items()}, **{k: v[:n] for k, v in rows.items()})
        assert sorted(out) == sorted(full)
        for k, v in store.items():
            assert torch.equal(v[:n], full[k][:n]), (n, k)
            assert (v[n:] == 77).all(), (n, k)
    three = {k: v[:3] for k, v in rows.items()}
    only = dev.forward(envs=[1, 0, 1], fields=["qacc"], **three)
    assert list(only) == ["qacc"] and torch.equal(only["qacc"], dev.forward(envs=[1, 0, 1], **three)["qacc"])
    empty = dev.forward(envs=torch.zeros((0,), dtype=torch.int32, device="cuda"))
    assert tuple(empty["qacc"].shape) == (0, cm.nv)
    with pytest.raises(ValueError):
        dev.forward(fields=["nonsense"])
    dev.k_close()


def test_three_rows_naming_the_last_envs_of_a_large_handle():
    """A 64-env handle after a few steps, rows naming envs 61, 0 and 63 with nothing else given: the rows of the all-env call."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    dev = env_hip.make("KManipSoloArm", num_envs=64, seed=2)
    dev.k_reset()
    for _ in range(3):
        dev.step_flat(dev.sample_action())
    full = dev.forward()
    f = dev.forward(envs=[61, 0, 63])
    pick = torch.tensor([61, 0, 63], device="cuda")
    dev.k_close()
    assert tuple(f["qacc"].shape) == (3, dev.cm.nv) and not full["status"].any()
    assert _same(full, f, rows_f=pick) == []
    assert not torch.equal(f["qacc"][0], f["qacc"][2])


# ---------------------------------------------------------------------------------------------------------------------------- status
def test_bad_rows_get_their_status_and_zeros_and_harm_nobody():
    torch = _torch()
    cm, qpos, qvel, ctrl, _, labels = _cells("solo_arm")
    n = len(labels)
    rows = dict(_rows("solo_arm", warm=True), qfrc_applied=_t(AO.draw_test_forces(cm, n)))
    dev = _fresh(cm, 2)
    assert dev.state_index_errors() == 0
    envs = np.arange(n) % 2
    clean = dev.forward(envs=envs, **rows)
    assert not clean["status"].any()

    def check(g, e, status):
        assert g["status"][e] == status and int(g["status"].ne(0).sum()) == 1, (e, status, g["status"])
        assert (g["contact_bit"][e] == -1).all() and g["contact_mask"][e] == 0
        for key in FLOAT_FIELDS:
            assert not g[key][e].any(), key
        keep = torch.arange(n, device="cuda") != e
        assert _same(clean, g, rows_f=keep, rows_g=keep) == []
    e = 5
    for name in rows:
        for value in (float("nan"), float("inf")):
            bad = dict(rows)
            bad[name] = rows[name].clone()
            bad[name][e, -1 if name == "qpos" else 2] = value
            check(dev.forward(envs=envs, **bad), e, 1)
    # without the force rows (the default build) as well
    plain = {k: v for k, v in rows.items() if k != "qfrc_applied"}
    clean = dev.forward(envs=envs, **plain)
    bad = dict(plain, ctrl=plain["ctrl"].clone())
    bad["ctrl"][e, 0] = float("nan")
    check(dev.forward(envs=envs, **bad), e, 1)
    # indices outside the handle: status 2, never an address
    for e, idx in ((0, -1), (7, 2), (n - 1, 2 ** 31 - 1), (3, -2 ** 31)):
        ie = envs.copy()
        ie[e] = idx
        check(dev.forward(envs=_t(ie, np.int32), **plain), e, 2)
    assert dev.state_index_errors() == 0
    # a stored non-finite value reaches the rows that use it, and only those
    q = dev.state_tensors()["qpos"]
    q[1, 0] = float("nan")
    dev.set_state_tensors(qpos=q)
    g = dev.forward(envs=[0, 1, 1, 0], qvel=plain["qvel"][:4])
    assert g["status"].tolist() == [0, 1, 1, 0]
    assert not dev.forward(envs=[0, 1, 1, 0], qpos=plain["qpos"][:4])["status"].any()
    dev.k_close()


# ------------------------------------------------------------------------------------------------------------------ handle read-only
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """Two identical handles, three steps; one calls forward -- identity rows, overriding rows, more rows than envs, with and without
    a force -- before each.  State, counters, obs, reward, done and diagnostics bit for bit."""
    torch = _torch()
    cm, qpos, qvel, ctrl, warm, labels = _cells(asset)
    n = len(labels)
    a, b = _device(cm, qpos, qvel, ctrl, warm), _device(cm, qpos, qvel, ctrl, warm)
    rows = _rows(asset)
    tau = _t(AO.draw_test_forces(cm, n))
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)
    for k in range(3):
        before = a.state_tensors()
        diag = a.get_diag()
        a.forward()
        a.forward(**rows)
        a.forward(envs=np.arange(2 * n)[::-1] % n, qvel=torch.cat([rows["qvel"], rows["qvel"]]), qfrc_applied=torch.cat([tau, tau]))
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), k
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), k
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), k
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
        assert torch.equal(a.sim_time, b.sim_time)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_diag(), b.get_diag())), k
    a.k_close(); b.k_close()


# -------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.lib import KForcesDev, KForwardIn, KManipError
    pgs = env_hip.KManipEnvHip(R.model("solo_arm", "pgs"), num_envs=4, seed=0)
    pgs.k_reset()
    with pytest.raises(KManipError, match="contact forces need the Newton solver"):
        pgs.forward()
    pgs.step_flat(torch.zeros((4, pgs.cm.act_dim), dtype=torch.float32, device="cuda"))
    assert not pgs.done.cpu().numpy().any()
    pgs.k_close()
    dev = _fresh(R.model("solo_arm"), 4)
    cm = dev.cm
    good = dev.forward()
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    with pytest.raises(KManipError, match="more rows than envs"):
        dev.forward(qvel=z(5, cm.nv))
    for kw in (dict(qpos=z(4, cm.nq, dtype=torch.float32)), dict(qvel=z(4, cm.nv + 1)), dict(ctrl=z(4, cm.nu, device="cpu")),
               dict(warm=z(4, cm.nv, 1)), dict(qfrc_applied=z(8, cm.nv)[::2]), dict(qpos=z(4, cm.nq), qvel=z(3, cm.nv)),
               dict(envs=[0, 1], qpos=z(3, cm.nq)), dict(qpos=np.zeros((4, cm.nq))), dict(out={"qacc": z(5, cm.nv)}),
               dict(out={"status": z(4, dtype=torch.int32)})):
        with pytest.raises(KManipError):
            dev.forward(**kw)
    L, fi, fd = dev.L, KForwardIn(), KForcesDev()
    assert L.kmanip_forward(dev.h, None, 4, C.byref(fd), None) != 0 and b"KForwardIn pointer is NULL" in L.kmanip_last_error(dev.h)
    assert L.kmanip_forward(dev.h, C.byref(fi), 4, None, None) != 0 and b"KForcesDev pointer is NULL" in L.kmanip_last_error(dev.h)
    assert L.kmanip_forward(None, C.byref(fi), 4, C.byref(fd), None) != 0
    assert L.kmanip_forward(dev.h, C.byref(fi), -1, C.byref(fd), None) != 0 and b"negative" in L.kmanip_last_error(dev.h)
    assert L.kmanip_forward(dev.h, C.byref(fi), 5, C.byref(fd), None) != 0
    assert L.kmanip_forward(dev.h, C.byref(fi), 4, C.byref(fd), None) == 0          # every field NULL: succeeds, does nothing
    assert L.kmanip_forward(dev.h, C.byref(fi), 0, C.byref(fd), None) == 0
    assert _same(good, dev.forward()) == []
    dev.step_flat(z(4, cm.act_dim, dtype=torch.float32))
    assert not dev.done.cpu().numpy().any()
    dev.k_close()


# ----------------------------------------------------------------------------------------------------------------------- derivatives
# one cell of each family of regime_states: grasp, pinch, limit, force limit, impact, free cube.  The single arm reaches no
# two-arm pinch (regime_states.UNREACHABLE): its one-finger push G3 stands in that place.
FD_CELLS = {"solo_arm": ("G1", "G3", "L1", "F1", "C2", "C1"), "dual_arm": ("P1", "L1", "C2"), "torso": ("P1", "L1", "C2")}


class _Recorder:
    """forward_fd's view of a handle -- .cm and .forward -- that keeps the rows of every call."""

    def __init__(self, dev):
        self.dev, self.cm, self.calls = dev, dev.cm, []

    def forward(self, **kw):
        self.calls.append({k: None if v is None else v.cpu().numpy() for k, v in kw.items() if k not in ("fields", "out")})
        return self.dev.forward(**kw)


@pytest.mark.parametrize("asset", ASSETS)
def test_finite_differences_against_the_oracles(asset):
    """forward_fd on the device against forward_fd on OracleForward, all blocks of qacc and qfrc_constraint, under
    bar x normaliser / eps; both sides were handed bit-equal rows (the warm start aside: each side's own nominal qacc), and the
    contact mask of every perturbed row is the same on both."""
    torch = _torch()
    from gym_kmanip_amd.derivatives import forward_fd
    cm, qpos, qvel, ctrl, _, labels = _cells(asset)
    pick = [labels.index(c) for c in FD_CELLS[asset]]
    n, nv = len(pick), cm.nv
    dec = [FO.cell_decodes(asset)[1][e] for e in pick]
    envs = np.arange(n) % 2
    ref_env = FW.OracleForward(cm, 2)
    ref = forward_fd(ref_env, envs=torch.from_numpy(envs), qpos=torch.from_numpy(qpos[pick]), qvel=torch.from_numpy(qvel[pick]),
                     ctrl=torch.from_numpy(ctrl[pick]), eps=EPS)
    dev = _fresh(cm, 2)
    rec = _Recorder(dev)
    got = forward_fd(rec, envs=_t(envs, np.int32), qpos=_t(qpos[pick]), qvel=_t(qvel[pick]), ctrl=_t(ctrl[pick]), eps=EPS)
    dev.k_close()
    assert len(rec.calls) == len(ref_env.calls) == 2 and len(rec.calls[1]["qpos"]) == 2 * (3 * nv + cm.nu) * n > 2
    for mine, theirs in zip(rec.calls, ref_env.calls):
        for k in ("envs", "qpos", "qvel", "ctrl", "qfrc_applied"):
            assert np.array_equal(mine[k], theirs[k]), k
    assert not got["status"].any() and not got["status_fd"].any() and not ref["status_fd"].any()
    assert torch.equal(got["contact_mask_fd"].cpu(), ref["contact_mask_fd"])
    bad, worst = [], {}
    for r, o in enumerate(dec):
        bq, bf = fd_bars(o)
        sq, sf, _ = FO.scales(o)
        for key in ("dqpos", "dqvel", "dctrl", "dfrc"):
            for q, bar, s in (("qacc", bq, sq), ("qfrc_constraint", bf, sf)):
                name = "d%s_%s" % (q, key)
                d = float((got[name][r].cpu() - ref[name][r]).abs().max())
                worst[name] = max(worst.get(name, 0.0), d * EPS / s)
                if not d <= bar:
                    bad.append((labels[pick[r]], name, d, bar))
    print("\n%s: worst |device - oracle| of every block x eps / normaliser (bars %.0e, %.0e): %s"
          % (asset, BAR_QACC, BAR_QFRC_CONSTRAINT, "  ".join("%s %.1e" % kv for kv in worst.items())))
    assert not bad, bad
    assert float(got["dqacc_dfrc"].abs().max()) > 1.0 and float(got["dqacc_dqpos"].abs().max()) > 1.0


def test_normal_by_bit_and_finger_force_take_their_rows_from_the_result():
    """Nine rows from a 2-env handle: [9, 32] and [9, 2], the oracle's normal forces at the bits."""
    cm, qpos, qvel, ctrl, _, labels = _cells("solo_arm")
    dec = FO.cell_decodes("solo_arm")[1]
    dev = _fresh(cm, 2)
    f = dev.forward(envs=np.arange(9) % 2, **{k: v[:9] for k, v in _rows("solo_arm").items()})
    by_bit, finger = dev.normal_by_bit(f).cpu().numpy(), dev.finger_force(f).cpu().numpy()
    dev.k_close()
    assert by_bit.shape == (9, 32) and finger.shape == (9, 2) and np.array_equal(finger, by_bit[:, 8:10]) and finger.max() > 1.0
    for e in range(9):
        want = np.zeros(32)
        for b, c in dec[e]["contacts"].items():
            want[b] = c["force"][0]
        assert np.abs(by_bit[e] - want).max() / FO.scales(dec[e])[1] <= BAR_CONTACT_FORCE and not (by_bit[e][want == 0] != 0).any()


# --------------------------------------------------------------------------------------------------------------------------- example
def test_the_example_reports_a_finite_gap(capsys):
    from gym_kmanip_amd.examples import forward_derivatives
    out = forward_derivatives.main([])
    print(capsys.readouterr().out)
    assert out["num_envs"] == 64 and out["rows_ok"] == 64
    assert math.isfinite(out["worst_rel_gap"]) and math.isfinite(out["worst_rel_gap_same_contacts"])
