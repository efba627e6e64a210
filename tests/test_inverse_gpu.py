"""kmanip_inverse against the inverse reference (run with -m gpu on an MI355X).

One handle per asset holds every regime cell's copies (tests/tools/regime_states.py: 47 envs for the single arm, 72 for the two-arm
models -- not a multiple of the 4 / 2 envs a wave holds).  Every field kmanip_inverse writes is compared with
tests/tools/inverse_oracle.py at each of a cell's eleven test accelerations, contact by contact through the mask bit, under the bars
of tests/test_inverse_cpu.py (1000 x the reference's own figures).  Then: per-env parameters, a PGS handle, the forward/inverse
residual of the device's own solve, the round trip through bind_applied_force, the state override, the handle left untouched, the
launch shapes, the status byte and the validation of the caller's tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import force_oracle as FO  # noqa: E402
import inverse_oracle as IO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
from test_inverse_cpu import (BAR_CONTACT_FORCE, BAR_FWDINV, BAR_QFRC_CONSTRAINT, BAR_QFRC_INVERSE, BAR_ROUNDTRIP,  # noqa: E402
                              ROUND_TRIP_SCALES, round_trip_indices)

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
FLOAT_FIELDS = ("qfrc_inverse", "qfrc_constraint", "contact_force")
PARAMS = dict(cube_mass=2.0, cube_friction=0.5, cube_frictionloss=0.0, kp_scale=1.3)      # (cube_mass: a factor of the model's)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_WARM = {}


def _warm(asset, c):
    from oracle.oracle import Oracle
    if asset not in _WARM:
        cm = R.model(asset)
        _WARM[asset] = R.warm_start(cm, Oracle(cm, 1), c["qpos"], c["qvel"], c["ctrl"])
    return _WARM[asset]


def _device(cm, c, warm, n=None):
    from gym_kmanip_amd import env_hip
    n = len(c["qpos"]) if n is None else n
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=0)
    dev.k_reset()
    dev.set_state(qpos=c["qpos"][:n], qvel=c["qvel"][:n], ctrl=c["ctrl"][:n], warm=warm[:n], step=np.zeros(n, dtype=np.int32))
    return dev


def _dev_t(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def _host(f):
    out = {k: v.cpu().numpy() for k, v in f.items()}
    if "contact_mask" in out:
        out["contact_mask"] = out["contact_mask"].view(np.uint32)
    return out


def _slot_kind_ok(nlink, slot, bit):
    nss = 2 * (nlink // 10)
    return bit < 8 if slot < 4 else (8 <= bit < 20 if slot < 4 + nss else bit >= 20)


def _compare(cm, f, e, o, what, figures):
    """Every field of env e of an inverse() result (host arrays) against the reference o.  Appends the normalised differences to
    `figures` and returns the list of violations."""
    si, sf = IO.scales(o)
    if f["status"][e] != 0:
        return [(what, "status", int(f["status"][e]))]
    if int(f["contact_mask"][e]) != o["mask"]:
        return [(what, "mask", hex(int(f["contact_mask"][e])), hex(o["mask"]))]
    bits = f["contact_bit"][e]
    used = [int(b) for b in bits if b >= 0]
    if sorted(used) != FO.mask_bits(o["mask"]):
        return [(what, "contact_bit", used, FO.mask_bits(o["mask"]))]
    bad = []
    d = dict(qfrc_inverse=float(np.abs(f["qfrc_inverse"][e] - o["qfrc_inverse"]).max()) / si,
             qfrc_constraint=float(np.abs(f["qfrc_constraint"][e] - o["qfrc_constraint"]).max()) / sf, contact_force=0.0)
    for s, b in enumerate(bits):
        if b < 0:                                            # an empty slot: every field zero
            if np.any(f["contact_force"][e, s] != 0):
                bad.append((what, "empty slot not zero", s))
            continue
        if not _slot_kind_ok(cm.nlink, s, int(b)):
            bad.append((what, "bit in a slot of another kind", s, int(b)))
        d["contact_force"] = max(d["contact_force"], float(np.abs(f["contact_force"][e, s] - o["contacts"][int(b)]).max()) / sf)
    figures.append((what, d))
    bars = dict(qfrc_inverse=BAR_QFRC_INVERSE, qfrc_constraint=BAR_QFRC_CONSTRAINT, contact_force=BAR_CONTACT_FORCE)
    return bad + [(what, k, v, bars[k]) for k, v in d.items() if not v <= bars[k]]


def _report(tag, figures):
    worst = {}
    for what, d in figures:
        for k, v in d.items():
            if v >= worst.get(k, (-1.0, None))[0]:
                worst[k] = (v, what)
    print("\n%s: worst normalised |device - reference|: %s" % (tag, "  ".join("%s %.1e %s" % (k, v, w) for k, (v, w) in worst.items())))


def _parity(tag, dev, c):
    """Every cell x every test acceleration of the handle against c["ref"]; returns the device results (device tensors) per k."""
    figures, bad, results = [], [], []
    for k in range(IO.N_ACCELS):
        inv = dev.inverse(_dev_t(c["qacc"][:, k]))
        results.append(inv)
        f = _host(inv)
        for e in range(len(c["labels"])):
            bad += _compare(c["cm"], f, e, c["ref"][e][k], (c["labels"][e], e, k), figures)
    _report(tag, figures)
    assert not bad, bad[:20]
    return results


@pytest.mark.parametrize("asset", ASSETS)
def test_parity_with_the_reference_on_every_cell_and_acceleration(asset):
    """Worst normalised differences measured on an MI355X: qfrc_inverse 1.6e-11, qfrc_constraint 1.6e-11,
    contact force 1.1e-11 (bars 3e-8, 2e-8, 7e-9)."""
    c = IO.cell_inverses(asset)
    dev = _device(c["cm"], c, _warm(asset, c))
    results = _parity(asset, dev, c)
    by_bit, finger = dev.normal_by_bit(results[0]).cpu().numpy(), dev.finger_force(results[0]).cpu().numpy()
    dev.k_close()
    for e, per_cell in enumerate(c["ref"]):
        want = np.zeros(32)
        for b, F in per_cell[0]["contacts"].items():
            want[b] = F[0]
        assert np.abs(by_bit[e] - want).max() / IO.scales(per_cell[0])[1] <= BAR_CONTACT_FORCE and not (by_bit[e][want == 0] != 0).any(), e
    assert finger.shape == (len(c["labels"]), 2 * (c["cm"].nlink // 10)) and np.array_equal(finger, by_bit[:, 8:8 + finger.shape[1]])
    f0 = _host(results[0])
    assert max((b >= 0).sum() for b in f0["contact_bit"]) >= (7 if c["cm"].nlink == 10 else 8)
    assert f0["contact_force"][:, :, 0].max() > 30.0


@pytest.mark.parametrize("asset", ASSETS)
def test_per_env_parameters_on_the_device(asset):
    """set_env_params (cube mass x 2, friction 0.5, friction loss 0, kp scale 1.3: those of tests/test_forces_gpu.py) against the
    reference on the with_env_params model, every cell x every test acceleration.  Measured on an MI355X: qfrc_inverse 8.3e-11,
    qfrc_constraint 8.3e-11, contact force 5.6e-11."""
    base = R.model(asset)
    p = dict(PARAMS, cube_mass=PARAMS["cube_mass"] * base.desc.cube_mass)
    c = IO.cell_inverses(asset, p)
    dev = _device(base, c, _warm(asset, c))
    dev.set_env_params(**p)
    _parity(asset + " with parameters", dev, c)
    dev.k_close()


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_a_pgs_handle_returns_the_bits_of_a_newton_handle(asset):
    torch = _torch()
    c = IO.cell_inverses(asset)
    warm = _warm(asset, c)
    newton, pgs = _device(c["cm"], c, warm), _device(R.model(asset, "pgs"), c, warm)
    assert pgs.cm.desc.solver != newton.cm.desc.solver
    for k in (0, 1, 3, 6, 9):
        a = _dev_t(c["qacc"][:, k])
        x, y = newton.inverse(a), pgs.inverse(a)
        assert all(torch.equal(x[key], y[key]) for key in x), k
    if asset == "solo_arm":
        _parity(asset + " on a PGS handle", pgs, c)
    newton.k_close(); pgs.k_close()


def _fwdinv(dev, tau):
    """Per-env forward/inverse residual of the handle's current state, normalised by max(1, max|qfrc_actuator|, max|M a + bias|)."""
    torch = _torch()
    from gym_kmanip_amd import applied
    f = dev.forces()
    inv = dev.inverse(f["qacc"])
    assert not f["status"].any() and not inv["status"].any()
    res = applied.fwdinv_residual(f, inv, tau)
    scale = torch.maximum(f["qfrc_actuator"].abs().amax(dim=1), (inv["qfrc_inverse"] + inv["qfrc_constraint"]).abs().amax(dim=1)).clamp(min=1.0)
    return (res / scale).cpu().numpy()


@pytest.mark.parametrize("asset", ASSETS)
def test_forward_inverse_residual_of_the_device_solve(asset):
    """fwdinv_residual(forces(), inverse(forces()["qacc"])) on every cell, without an applied force and with the test forces of
    tests/tools/applied_oracle.py bound; the bar is 1000 x the reference's own residual (tests/test_inverse_cpu.py): 9e-10.
    Measured on an MI355X, worst per asset without / with the test forces: SoloArm 1.57e-12 / 8.85e-13,
    DualArm 1.20e-12 / 1.77e-12, Torso 1.20e-12 / 4.94e-13."""
    c = IO.cell_inverses(asset)
    dev = _device(c["cm"], c, _warm(asset, c))
    free = _fwdinv(dev, None)
    tau = _dev_t(AO.draw_test_forces(c["cm"], len(c["labels"])))
    dev.bind_applied_force(tau)
    forced = _fwdinv(dev, tau)
    dev.bind_applied_force(None)
    dev.k_close()
    for tag, r in (("no applied force", free), ("test forces bound", forced)):
        e = int(np.argmax(r))
        print("\n%s, %s: worst forward/inverse residual %.2e (%s, env %d); bar %.0e" % (asset, tag, r[e], c["labels"][e], e, BAR_FWDINV))
    assert free.max() <= BAR_FWDINV and forced.max() <= BAR_FWDINV, (free.max(), forced.max())


@pytest.mark.parametrize("asset", ASSETS)
def test_round_trip_through_the_applied_force(asset):
    """inverse(a), bind_applied_force(from_inverse(..)), forces()["qacc"] == a for a = a* + s z, s in {1, 30}: the bars are 1000 x the
    reference's round-trip errors, per s (3e-10 and 3e-2: at s = 30 the reference's own solver is the limit, tests/test_inverse_cpu.py).
    Measured on an MI355X, worst over the assets: s = 1 5.45e-14, s = 30 9.12e-13."""
    torch = _torch()
    from gym_kmanip_amd import applied
    c = IO.cell_inverses(asset)
    dev = _device(c["cm"], c, _warm(asset, c))
    f0 = dev.forces(fields=["qfrc_actuator"])
    worst = {s: (0.0, -1, -1) for s in ROUND_TRIP_SCALES}
    for s in ROUND_TRIP_SCALES:
        for k in round_trip_indices(s):
            a = _dev_t(c["qacc"][:, k])
            inv = dev.inverse(a, fields=["qfrc_inverse", "status"])
            dev.bind_applied_force(applied.from_inverse(inv, f0))
            f = dev.forces(fields=["qacc", "status"])
            dev.bind_applied_force(None)
            assert not inv["status"].any() and not f["status"].any(), (s, k)
            r = ((f["qacc"] - a).abs().amax(dim=1) / a.abs().amax(dim=1).clamp(min=1.0)).cpu().numpy()
            e = int(np.argmax(r))
            if r[e] >= worst[s][0]:
                worst[s] = (float(r[e]), e, k)
    dev.k_close()
    print("\n%s: round trip, worst per scale: %s" % (asset, "  ".join("s=%g %.2e (%s, env %d, k %d; bar %.0e)" % (
        s, worst[s][0], c["labels"][worst[s][1]], worst[s][1], worst[s][2], BAR_ROUNDTRIP[s]) for s in ROUND_TRIP_SCALES)))
    for s in ROUND_TRIP_SCALES:
        assert worst[s][0] <= BAR_ROUNDTRIP[s], (s, worst[s])


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_state_override_is_set_state_tensors_then_the_call(asset):
    torch = _torch()
    from gym_kmanip_amd import env_hip
    c = IO.cell_inverses(asset)
    n = len(c["labels"])
    a_dev = env_hip.KManipEnvHip(c["cm"], num_envs=n, seed=0)       # handle A keeps its reset state
    b_dev = env_hip.KManipEnvHip(c["cm"], num_envs=n, seed=0)
    a_dev.k_reset(); b_dev.k_reset()
    qpos, qvel, qacc = _dev_t(c["qpos"]), _dev_t(c["qvel"]), _dev_t(c["qacc"][:, 3])
    before = a_dev.state_tensors()
    over = a_dev.inverse(qacc, qpos=qpos, qvel=qvel)
    after = a_dev.state_tensors()
    assert all(torch.equal(before[key], after[key]) for key in before)
    b_dev.set_state_tensors(qpos=qpos, qvel=qvel)
    want = b_dev.inverse(qacc)
    assert all(torch.equal(over[key], want[key]) for key in want)
    assert not want["status"].any() and want["contact_mask"].any()
    # one field alone: qpos from the caller, qvel the handle's
    b_dev.set_state_tensors(qvel=before["qvel"])
    half, want_half = a_dev.inverse(qacc, qpos=qpos), b_dev.inverse(qacc)
    assert all(torch.equal(half[key], want_half[key]) for key in half)
    assert not torch.equal(half["qfrc_inverse"], over["qfrc_inverse"])
    # the handle's own state passed explicitly
    st = b_dev.state_tensors()
    own = b_dev.inverse(qacc, qpos=st["qpos"], qvel=st["qvel"])
    assert all(torch.equal(own[key], want_half[key]) for key in own)
    a_dev.k_close(); b_dev.k_close()


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """Two identical handles, three steps; one calls inverse before each.  State, warm start, counters, obs, reward, done and
    diagnostics bit for bit."""
    torch = _torch()
    c = IO.cell_inverses(asset)
    warm = _warm(asset, c)
    a, b = _device(c["cm"], c, warm), _device(c["cm"], c, warm)
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, len(c["labels"]), c["cm"].act_dim)).astype(np.float32)
    for k in range(3):
        before = a.state_tensors()
        diag = a.get_diag()
        a.inverse(_dev_t(c["qacc"][:, 2 + k]))
        a.inverse(_dev_t(c["qacc"][:, 5 + k]), qpos=_dev_t(c["qpos"][::-1]), qvel=_dev_t(c["qvel"][::-1]))
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


@pytest.mark.parametrize("asset,sizes", [("solo_arm", (1, 3, 5, 47)), ("dual_arm", (1, 3, 72))])
def test_launch_shapes(asset, sizes):
    """Handles of 1, 3, 5 envs (four envs per wave) / 1, 3 (two per wave): each env's rows are the bits of the same state's rows in
    the full batch; the tensors are over-allocated and the rows beyond num_envs stay as they were."""
    torch = _torch()
    c = IO.cell_inverses(asset)
    warm = _warm(asset, c)
    k = 4
    full_n = len(c["labels"])
    assert sizes[-1] == full_n
    from gym_kmanip_amd.model import contact_slots
    nv, nc = c["cm"].nv, contact_slots(c["cm"].nlink)
    layout = dict(qfrc_inverse=((nv,), torch.float64), qfrc_constraint=((nv,), torch.float64), contact_force=((nc, 4), torch.float64),
                  contact_bit=((nc,), torch.int32), contact_mask=((), torch.int32), status=((), torch.uint8))
    full = None
    for n in reversed(sizes):
        dev = _device(c["cm"], c, warm, n)
        big = {name: torch.full((n + 3,) + shp, 77, dtype=dt, device="cuda") for name, (shp, dt) in layout.items()}
        got = dev.inverse(_dev_t(c["qacc"][:n, k]), out={name: t[:n] for name, t in big.items()})
        dev.k_close()
        if full is None:
            full = {name: t.clone() for name, t in got.items()}
            assert not full["status"].any()
        for name, t in big.items():
            assert torch.equal(t[:n], full[name][:n]), (n, name)
            assert (t[n:] == 77).all(), (n, name)


def test_status_of_a_non_finite_env():
    """A NaN in one env's qacc, or in its qpos (the handle's, and the caller's): status 1 there, zeros and contact_bit -1; its
    wave-mates' rows are the bits of a clean run."""
    torch = _torch()
    c = IO.cell_inverses("solo_arm")
    n = len(c["labels"])
    dev = _device(c["cm"], c, _warm("solo_arm", c))
    qacc = _dev_t(c["qacc"][:, 2])
    clean = dev.inverse(qacc)
    assert not clean["status"].any()

    def check(g, e, tag):
        assert g["status"][e] == 1 and g["status"].sum() == 1, tag
        assert (g["contact_bit"][e] == -1).all() and g["contact_mask"][e] == 0, tag
        for key in FLOAT_FIELDS:
            assert not g[key][e].any(), (tag, key)
        keep = torch.arange(n, device=g["status"].device) != e
        for key in g:
            assert torch.equal(g[key][keep], clean[key][keep]), (tag, key)
    e = 5                                                    # (not the first env of its wave)
    bad = qacc.clone()
    bad[e, 3] = float("nan")
    check(dev.inverse(bad), e, "qacc")
    bad = qacc.clone()
    bad[e, c["cm"].nv - 1] = float("inf")
    check(dev.inverse(bad), e, "qacc inf")
    qn = _dev_t(c["qpos"])
    qn[e + 1, 0] = float("nan")
    check(dev.inverse(qacc, qpos=qn), e + 1, "qpos of the caller")
    vn = _dev_t(c["qvel"])
    vn[e, 2] = float("nan")
    check(dev.inverse(qacc, qvel=vn), e, "qvel of the caller")
    host = c["qpos"].copy()
    host[e, 0] = np.nan
    dev.set_state(qpos=host)
    check(dev.inverse(qacc), e, "qpos of the handle")
    dev.k_close()


def test_example_reports_the_residual_and_holds_a_pressed_cube():
    """examples/inverse_dynamics.py.  residual: the device's forward/inverse residual over a rollout stays at its solver's stopping
    point -- solver_tolerance = 1e-8 is a bound on the scaled gradient norm, gradient = residual / (meaninertia nv); 1e-6 leaves the
    scale's two digits.  hold: without the binding the pressed cube and the unsupported arm accelerate with more than 1 m/s^2 (gravity
    alone is 9.81); with it, |qacc| is below 1e-6 and the state moves a thousand times less."""
    from gym_kmanip_amd.examples import inverse_dynamics
    r = inverse_dynamics.main(["--mode", "residual", "--num-envs", "64", "--steps", "6"])
    print(r)
    assert 0 <= r["fwdinv_residual_max"] <= 1e-6 and r["fwdinv_applied_l2"] <= 1e-6 and r["fwdinv_constraint_l2"] <= 1e-6
    h = inverse_dynamics.main(["--mode", "hold", "--num-envs", "16", "--steps", "4"])
    print(h)
    assert h["qacc_max_without"] > 1.0 and h["qacc_max_with"] <= 1e-6
    assert h["qpos_drift_with"] <= 1e-3 * h["qpos_drift_without"]


def test_validation_and_refusals():
    """_check_buf rejects a wrong shape, dtype, device or a non-contiguous tensor before the library is called; `fields` / `out`
    select what is computed; the C entry refuses NULL arguments and leaves the handle usable."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.lib import KInverseDev, KInverseIn, KManipError
    dev = env_hip.KManipEnvHip(R.model("solo_arm"), num_envs=6, seed=0)
    dev.k_reset()
    nv, nq = dev.cm.nv, dev.cm.nq
    qacc = torch.zeros((6, nv), dtype=torch.float64, device="cuda")
    full = dev.inverse(qacc)
    assert set(full) == {"qfrc_inverse", "qfrc_constraint", "contact_force", "contact_bit", "contact_mask", "status"}
    calls = []
    real = dev.L.kmanip_inverse

    class Spy:                                               # (counts the calls that reach the library)
        def __getattr__(self, name):
            if name == "kmanip_inverse":
                return lambda *a: (calls.append(1), real(*a))[1]
            return getattr(dev_L, name)
    dev_L, dev.L = dev.L, Spy()
    wide = torch.zeros((6, 2 * nv), dtype=torch.float64, device="cuda")
    for tag, kw in (("shape", dict(qacc=torch.zeros((5, nv), dtype=torch.float64, device="cuda"))),
                    ("dtype", dict(qacc=qacc.float())),
                    ("device", dict(qacc=qacc.cpu())),
                    ("layout", dict(qacc=wide[:, ::2])),
                    ("not a tensor", dict(qacc=np.zeros((6, nv)))),
                    ("missing", dict(qacc=None)),
                    ("qpos shape", dict(qacc=qacc, qpos=torch.zeros((6, nv), dtype=torch.float64, device="cuda"))),
                    ("qvel dtype", dict(qacc=qacc, qvel=torch.zeros((6, nv), dtype=torch.float32, device="cuda"))),
                    ("qpos device", dict(qacc=qacc, qpos=torch.zeros((6, nq), dtype=torch.float64))),
                    ("out shape", dict(qacc=qacc, out={"qfrc_inverse": torch.zeros((6, nv + 1), dtype=torch.float64, device="cuda")})),
                    ("out dtype", dict(qacc=qacc, out={"status": torch.zeros((6,), dtype=torch.int32, device="cuda")})),
                    ("out layout", dict(qacc=qacc, out={"qfrc_constraint": wide[:, ::2]}))):
        with pytest.raises(KManipError):
            dev.inverse(**kw)
        assert not calls, tag
    with pytest.raises(ValueError):
        dev.inverse(qacc, fields=["qacc"])
    assert not calls
    only = dev.inverse(qacc, fields=["qfrc_inverse"])
    assert list(only) == ["qfrc_inverse"] and torch.equal(only["qfrc_inverse"], full["qfrc_inverse"]) and len(calls) == 1
    again = dev.inverse(qacc, out={"status": torch.full_like(full["status"], 7), "contact_bit": torch.zeros_like(full["contact_bit"])})
    assert torch.equal(again["contact_bit"], full["contact_bit"]) and not again["status"].any()
    dev.L = dev_L
    # the C entry
    iv, od = KInverseIn(), KInverseDev()
    assert dev.L.kmanip_inverse(None, C.byref(iv), C.byref(od), None) != 0
    assert dev.L.kmanip_inverse(dev.h, None, C.byref(od), None) != 0 and b"KInverseIn pointer is NULL" in dev.L.kmanip_last_error(dev.h)
    assert dev.L.kmanip_inverse(dev.h, C.byref(iv), None, None) != 0 and b"KInverseDev pointer is NULL" in dev.L.kmanip_last_error(dev.h)
    assert dev.L.kmanip_inverse(dev.h, C.byref(iv), C.byref(od), None) != 0 and b"qacc is NULL" in dev.L.kmanip_last_error(dev.h)
    iv.qacc = qacc.data_ptr()
    assert dev.L.kmanip_inverse(dev.h, C.byref(iv), C.byref(od), None) == 0          # every output NULL: succeeds, does nothing
    assert all(torch.equal(v, full[k]) for k, v in dev.inverse(qacc).items())
    dev.k_close()
