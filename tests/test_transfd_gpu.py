"""kmanip_transition_fd on the device (run with -m gpu on an MI355X): KManipEnvHip.transition_fd, the fused derivatives.transition_fd.

The rows are the six cells per asset of rollout_oracle.FD_CELLS -- the smallest rows that reach contact, grasp, pinch, limit and
force-limit states -- on handles of 2 envs (envs = arange(6) % 2): more rows than envs, 6 x ncol pairs, not a multiple of the pairs a
wave holds.  Against the oracle the bars are tests/test_rollout_cpu.py's BAR_FD as they stand.  Against derivatives.transition_fd on the
same handle the perturbed inputs are the same bytes and the sub-step source is the same, so the nominal rows and the masks are
compared byte for byte, and so are the joint, cube-position and qvel rows of every block behind FUSED_BYTES_EQUAL -- see there for
what the device showed and what is asserted in its place; BAR_FD is asserted first either way.  The three cube-rotation rows pass
through atan2, whose two implementations are each within 2 ulp, so differ by up to 4, and one multiply and one divide follow:
16 * 2^-52 * |entry|.  Everything that compares the kernel with itself is bit for bit.
What the device showed: DESIGN.md section 31."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu

ASSETS = mujoco_pin.ASSETS
ALL = ("qpos", "qvel", "ctrl", "qfrc_applied")
# (asset, solver, mode) of the comparison with derivatives.transition_fd on the same handle, nsub = 1: plain, a given force
# (differentiated as well), env 1 with parameters of its own, both -- and a BOUND force in place of a given one.
# tests/test_transfd_cpu.py checks that these rows launch every k_transfd object the Makefile compiles.
HANDLE_ROWS = ([(a, s, m) for a in ("solo_arm", "dual_arm") for s in ("newton", "pgs") for m in ("plain", "forced", "params", "params+forced")]
               + [("solo_arm", "newton", "bound")])
# The fused call against derivatives.transition_fd's own blocks on the same handle, byte for byte on the joint, cube-position and
# qvel rows.  The first measurement on an MI355X did NOT show it: entries of every block differed by one unit
# in the last place, 1.00 x 2^-52 |entry| at the most.  The cause is the last operation alone: torch on the device divides a tensor
# by a Python number as a multiplication by its reciprocal, where the kernel -- and torch on the CPU, hence the oracle's reference --
# divides.  So the flag is off and BAR_FD is the fallback the blocks are held to, with two checks that are tighter and follow from
# the arithmetic: (a) RECIPROCAL_ULPS on those rows -- x * fl(1 / d) carries two roundings, x / d one, each within 2^-53 relative:
# 1.5 x 2^-52 |entry| apart at the most, rounded up to 2; (b) QUOTIENT_BYTES_EQUAL: the perturbed states the Python's second launch
# returned, differenced by its own torch operations and then DIVIDED (by a tensor: an IEEE division), are the fused bytes.
FUSED_BYTES_EQUAL = False
QUOTIENT_BYTES_EQUAL = True
RECIPROCAL_ULPS = 2.0          # in units of 2^-52 |entry|
ROT_ULPS = 16.0                # likewise: the three cube-rotation rows (the module docstring)
_ROWS = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _t(x, dtype=None):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _fresh(cm, n, seed=0):
    from gym_kmanip_amd import env_hip
    dev = env_hip.KManipEnvHip(cm, num_envs=n, seed=seed)
    dev.k_reset()
    return dev


def _rows(asset, solver="newton"):
    """(cm, the FD_CELLS rows as device tensors, [6, nv] test forces) of the asset under the solver's default model, built once."""
    if (asset, solver) not in _ROWS:
        cm = R.model(asset, solver)
        rows = RO.fd_rows(asset, cm)
        _ROWS[(asset, solver)] = (cm, rows, np.ascontiguousarray(RO.step_forces(cm, len(rows["qpos"]), 1)[:, 0]))
    cm, rows, tau = _ROWS[(asset, solver)]
    return cm, {k: _t(v) for k, v in rows.items()}, _t(tau)


NOMINAL = ("qpos", "qvel", "qacc_warm", "contact_mask", "status")
BLOCKS = ("A", "B", "dnext_dfrc", "dnext_dqpos", "dnext_dqvel")


def _bytes_differ(f, g, keys=None):
    """Names of the fields (default: every one of f) whose bytes differ."""
    torch = _torch()
    return [k for k in (f if keys is None else keys) if not torch.equal(f[k], g[k])]


class _Recorder:
    """derivatives.transition_fd's view of a handle -- .cm and .rollout -- that keeps what every launch returned."""

    def __init__(self, dev):
        self.dev, self.cm, self.outs = dev, dev.cm, []

    def rollout(self, **kw):
        self.outs.append(self.dev.rollout(**kw))
        return self.outs[-1]


def _divided(cm, pert, n, ncol, eps=1e-6):
    """[n, ncol, 2 nv]: derivatives.transition_fd's quotients from the perturbed rows its second launch returned, in its own torch
    operations but for the last: the numerators are divided by a TENSOR holding 2.0 * eps, an IEEE division on the device."""
    torch = _torch()
    from gym_kmanip_amd.derivatives import tangent_diff
    q, v = pert["qpos"][:, 0], pert["qvel"][:, 0].reshape(ncol, 2, n, cm.nv)
    dq = torch.stack([tangent_diff(cm, q[(2 * k) * n:(2 * k + 1) * n], q[(2 * k + 1) * n:(2 * k + 2) * n]) for k in range(ncol)])
    num = torch.cat([dq, v[:, 0] - v[:, 1]], dim=2)
    return (num / torch.full_like(num, 2.0 * eps)).permute(1, 0, 2)


def _against_the_python(tag, cm, got, ref, exact=NOMINAL + ("contact_mask_fd", "status_fd"), pert=None):
    """A fused result against derivatives.transition_fd's of the same rows on the same handle (the module docstring's rules);
    `exact`: the fields compared byte for byte besides the blocks; `pert`: what the Python's second launch returned."""
    torch = _torch()
    from test_rollout_cpu import BAR_FD
    assert _bytes_differ(ref, got, exact) == [], tag
    nl, nv = cm.nlink, cm.nv
    rot = torch.zeros(2 * nv, dtype=torch.bool, device="cuda")
    rot[nl + 3:nl + 6] = True
    if "A" in ref:
        dist = RO.fd_dist(RO.fd_blocks(ref, nv), RO.fd_blocks(got, nv))
        bad = [(k, float(v.max())) for k, v in dist.items() if not (v <= BAR_FD[1][k]).all()]
        assert not bad, (tag, bad)
    worst, bad = {}, []
    for k in BLOCKS:
        if k not in ref:
            assert k not in got, (tag, k)
            continue
        a, b = got[k], ref[k]
        assert a.shape == b.shape, (tag, k)
        d = (a - b).abs() / b.abs().clamp(min=1e-300) / 2.0 ** -52
        worst[k] = (float(d[:, ~rot].max()), float(d[:, rot].max()))
        if FUSED_BYTES_EQUAL and not torch.equal(a[:, ~rot], b[:, ~rot]):
            bad.append((k, "bytes"))
        if not (worst[k][0] <= RECIPROCAL_ULPS and worst[k][1] <= ROT_ULPS):
            bad.append((k, "units"))
    same = None
    if pert is not None:
        want = _divided(cm, pert, int(got["deriv_t"].shape[0]), int(got["deriv_t"].shape[1]))
        same = torch.equal(want[:, :, ~rot], got["deriv_t"][:, :, ~rot])
    print("%s: worst |fused - python| in units of 2^-52 |entry|, joint / cube-position / qvel rows and rotation rows: %s; the Python's own "
          "numerators divided on the device give the fused bytes on the first kind: %s" % (tag, "  ".join("%s %.2f / %.2f" % ((k,) + v) for k, v in worst.items()), same))
    assert not bad, (tag, bad, worst)
    if pert is not None and QUOTIENT_BYTES_EQUAL:
        assert same, tag


# ------------------------------------------------------------------------------------------------------------ 1. against the oracles
@pytest.mark.parametrize("nsub", [1, None], ids=["mj_step", "control_step"])
@pytest.mark.parametrize("asset", ASSETS)
def test_fused_transition_fd_against_the_oracles(asset, nsub):
    """KManipEnvHip.transition_fd against transition_fd over OracleRollout on the FD_CELLS rows, the model compiled at FD_TOLERANCE,
    one mj_step and one control step: every block within BAR_FD, the contact masks of the nominal and of all perturbed rows equal,
    every status 0."""
    torch = _torch()
    from test_rollout_cpu import BAR_FD, SPREAD_FD
    cm, rows, _, ref = RO.fd_reference(asset, nsub)
    n, nv = len(rows["qpos"]), cm.nv
    dev = _fresh(cm, 2)
    got = dev.transition_fd(nsub=nsub, **{k: _t(v) for k, v in rows.items()})
    torch.cuda.synchronize()
    dev.k_close()
    assert tuple(got["deriv_t"].shape) == (n, 2 * nv + cm.nu, 2 * nv) and got["A"].data_ptr() == got["deriv_t"].data_ptr()
    assert not got["status"].any() and not got["status_fd"].any() and not got["status_cols"].any() and not ref["status_fd"].any()
    assert torch.equal(got["contact_mask_fd"].cpu(), ref["contact_mask_fd"]) and torch.equal(got["contact_mask"].cpu(), ref["contact_mask"])
    dist = RO.fd_dist(RO.fd_blocks(ref, nv), RO.fd_blocks(got, nv))
    print("\n%s, nsub %s: worst normalised |fused - oracle| per block (the reference's spread; the bar): %s"
          % (asset, nsub or "the model's", "  ".join("%s %.1e in %s (%.1e; %.0e)" % (k, v.max(), RO.FD_CELLS[asset][int(v.argmax())], SPREAD_FD[nsub][k], BAR_FD[nsub][k])
                                                     for k, v in dist.items())))
    bad = [(k, RO.FD_CELLS[asset][e], float(v[e]), BAR_FD[nsub][k]) for k, v in dist.items() for e in range(n) if not v[e] <= BAR_FD[nsub][k]]
    assert not bad, bad
    assert float(got["A"].abs().max()) > 1.0 and float(got["B"].abs().max()) > 1e-3


# ------------------------------------------------------------------------------- 2. against derivatives.transition_fd on the handle
@pytest.mark.parametrize("asset,solver,mode", HANDLE_ROWS)
def test_fused_against_the_python_on_the_same_handle(asset, solver, mode):
    """KManipEnvHip.transition_fd against derivatives.transition_fd on the same handle of 2 envs, the FD_CELLS rows, nsub = 1, on the
    rows that launch every k_transfd object: nominal outputs, contact_mask_fd and status_fd byte for byte, the blocks as
    _against_the_python and the flags above say."""
    torch = _torch()
    from gym_kmanip_amd.derivatives import transition_fd
    cm, rows, tau = _rows(asset, solver)
    dev = _fresh(cm, 2)
    if "params" in mode:
        dev.set_env_params(**RO.env_params(cm)[0])
    kw = dict(rows, nsub=1)
    if "forced" in mode:
        kw.update(qfrc_applied=tau, wrt=ALL)
    if mode == "bound":
        dev.new_applied_force().copy_(tau[:2])
    rec = _Recorder(dev)
    ref = transition_fd(rec, **kw)
    got = dev.transition_fd(**kw)
    assert len(rec.outs) == 2 and not ref["status"].any() and not ref["status_fd"].any() and float(ref["A"].abs().max()) > 1.0
    _against_the_python("\n%s %s %s" % (asset, solver, mode), cm, got, ref, pert=rec.outs[1])
    if "forced" in mode:
        assert float(got["dnext_dfrc"].abs().max()) > 1e-6
    dev.k_close()


def test_trajectory_fd_fused_against_the_python_on_the_device():
    """ilqr.trajectory_fd(fused=True) against fused=False on KManipSoloArmQPos, 4 envs, horizon 4: the rows it passes are held by the
    comparison above."""
    torch = _torch()
    from gym_kmanip_amd import env_hip, ilqr
    env = env_hip.make("KManipSoloArmQPos", num_envs=4, seed=3)
    env.k_reset()
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    ctrl = st["ctrl"][:, None, :].repeat(1, 4, 1)
    a = ilqr.trajectory_fd(env, None, st["qpos"], st["qvel"], st["warm"], ctrl)
    b = ilqr.trajectory_fd(env, None, st["qpos"], st["qvel"], st["warm"], ctrl, fused=True)
    assert _bytes_differ(a, b, ("qpos", "qvel", "warm", "status", "status_fd")) == [] and not a["status_fd"].any()
    cm = env.cm
    flat = lambda d: {k: d[k].reshape((16,) + tuple(d[k].shape[2:])) for k in ("A", "B")}
    _against_the_python("\ntrajectory_fd", cm, flat(b), flat(a), exact=())
    env.k_close()


# --------------------------------------------------------------------------------------------- 3. the kernel against itself, bit for bit
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_kernel_against_itself_bit_for_bit(asset):
    """Two sub-steps, every input differentiated, a force given: the same bytes with the rows reversed, each row alone, on a handle
    of 5 envs under a repeated index, for every subset of wrt (masks in the caller's column order), for a differentiated force
    nobody gave against explicit zeros, without contact_mask_fd, and with the warm-start base given against the nominal row's."""
    torch = _torch()
    cm, rows, tau = _rows(asset)
    n, nv = 6, cm.nv
    dev = _fresh(cm, 2)
    kw = dict(rows, nsub=2, wrt=ALL, qfrc_applied=tau)
    full = dev.transition_fd(**kw)
    assert not full["status"].any() and not full["status_fd"].any()
    raw = NOMINAL + ("deriv_t", "status_cols", "contact_mask_fd")
    # rows reversed
    rev = dev.transition_fd(**{k: (v.flip(0).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    assert [k for k in raw if not torch.equal(rev[k].flip(-1 if k == "contact_mask_fd" else 0), full[k])] == []
    # each row alone, n = 1
    for e in (0, 3, 5):
        one = dev.transition_fd(**{k: (v[e:e + 1].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        assert [k for k in raw if not torch.equal(one[k], full[k][..., e:e + 1] if k == "contact_mask_fd" else full[k][e:e + 1])] == [], e
    # a handle of 5 envs, a repeated index: envs 3 and 1 hold nothing the rows use (every field is given)
    big = _fresh(cm, 5)
    idx = _t(np.array([3, 1, 3, 3, 1, 3], np.int32))
    assert _bytes_differ(full, big.transition_fd(**dict(kw, envs=idx)), raw) == []
    big.k_close()
    # subsets of wrt give the bytes of their blocks
    part = dev.transition_fd(**dict(kw, wrt=("ctrl",)))
    assert torch.equal(part["B"], full["B"]) and part["deriv_t"].shape[1] == cm.nu and _bytes_differ(full, part, NOMINAL) == []
    part = dev.transition_fd(**dict(kw, wrt=("qpos",)))
    assert torch.equal(part["dnext_dqpos"], full["A"][:, :, :nv]) and "A" not in part
    part = dev.transition_fd(**dict(kw, wrt=("qfrc_applied", "ctrl")))
    assert torch.equal(part["dnext_dfrc"], full["dnext_dfrc"]) and torch.equal(part["B"], full["B"])
    # ... and the masks' columns follow the caller's order
    m, c0 = full["contact_mask_fd"], 2 * nv
    assert torch.equal(part["contact_mask_fd"], torch.cat([m[c0 + cm.nu:], m[c0:c0 + cm.nu]]))
    # a differentiated force nobody gave is rows of zeros
    zero = dev.transition_fd(**dict(kw, qfrc_applied=torch.zeros_like(tau), wrt=("qfrc_applied",)))
    none = dev.transition_fd(**dict(kw, qfrc_applied=None, wrt=("qfrc_applied",)))
    assert _bytes_differ(zero, none, ("deriv_t", "status_cols", "contact_mask_fd", "contact_mask", "status")) == []
    print("\n%s: nominal rows of the plain build against the force build under zero force differ in %s" % (asset, _bytes_differ(zero, none, NOMINAL) or "nothing"))
    # with and without contact_mask_fd
    lean = dev.transition_fd(out={"status_cols": torch.empty((n, full["deriv_t"].shape[1]), dtype=torch.uint8, device="cuda")}, **kw)
    assert "contact_mask_fd" not in lean and "contact_mask" not in lean and _bytes_differ(lean, full, ("deriv_t", "status_cols", "A", "B")) == []
    # warm given against None: the base is then the nominal row's qacc_warm after the step
    nom = dev.transition_fd(**dict(kw, wrt=()))
    assert set(nom) == set(NOMINAL) and _bytes_differ(nom, full) == []
    st = dev.state_tensors()
    st["warm"][:] = rows["warm"][:2]
    dev.set_state_tensors(warm=st["warm"])
    two = {k: (v[:2].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    stored = dev.transition_fd(**dict(two, warm=None))                              # nominal rows: the stored warm start, the same bytes
    given = dev.transition_fd(**dict(two, warm=stored["qacc_warm"], warm_offset=1.0))
    again = dev.transition_fd(**dict(two, warm=rows["warm"][:2].contiguous()))
    assert _bytes_differ(again, stored, NOMINAL) == []
    # (given: nominal rows from another warm start, but the perturbed rows' base is the one `stored` used)
    assert _bytes_differ(given, stored, ("status_cols", "contact_mask_fd")) == [] and torch.equal(given["deriv_t"], stored["deriv_t"])
    dev.k_close()


# ------------------------------------------------------------------------------------------------------------ 4. status and refusals
def test_bad_rows_get_their_status_and_zero_columns_and_harm_nobody():
    torch = _torch()
    cm, rows, tau = _rows("solo_arm")
    n, e = 6, 3
    dev = _fresh(cm, 2)
    raw = NOMINAL + ("deriv_t", "status_cols", "contact_mask_fd")
    for kw in (dict(rows, nsub=1), dict(rows, nsub=1, qfrc_applied=tau, wrt=ALL)):
        clean = dev.transition_fd(**kw)
        assert not clean["status"].any() and not clean["status_cols"].any()
        keep = torch.arange(n, device="cuda") != e

        def check(g, status):
            assert g["status"].tolist() == [0] * e + [status] + [0] * (n - e - 1)
            assert bool((g["status_cols"][e] == status).all()) and not g["status_cols"][keep].any() and int(g["status_fd"][e]) == status
            assert not g["deriv_t"][e].any() and not g["contact_mask_fd"][:, :, e].any() and not g["A"][e].any()
            for k in raw:
                a, b = (g[k], clean[k]) if k != "contact_mask_fd" else (g[k].permute(2, 0, 1), clean[k].permute(2, 0, 1))
                assert torch.equal(a[keep], b[keep]), k
        # indices outside the handle, in the middle of the rows: status 2, never an address
        for idx in (2, -1, 2 ** 31 - 1, -2 ** 31):
            ie = rows["envs"].cpu().numpy().copy()
            ie[e] = idx
            check(dev.transition_fd(**dict(kw, envs=_t(ie, np.int32))), 2)
        assert dev.state_index_errors() == 0
        for name, at in (("qpos", (e, -1)), ("qvel", (e, 3)), ("ctrl", (e, 0))):
            bad = dict(kw)
            bad[name] = kw[name].clone()
            bad[name][at] = float("nan")
            check(dev.transition_fd(**bad), 1)
    dev.k_close()


def test_refusals_launch_nothing_and_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd.lib import KManipError, KTransFdDev, KTransFdIn
    dev = _fresh(R.model("solo_arm"), 4)
    cm, L = dev.cm, dev.L
    ncol = 2 * cm.nv + cm.nu
    good = dev.transition_fd()
    assert not good["status"].any() and not good["status_fd"].any() and tuple(good["A"].shape) == (4, 2 * cm.nv, 2 * cm.nv)
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    with pytest.raises(KManipError, match="more rows than envs"):
        dev.transition_fd(qvel=z(5, cm.nv))
    with pytest.raises(KManipError, match="negative"):
        dev.transition_fd(nsub=-1)
    with pytest.raises(KManipError, match="eps"):
        dev.transition_fd(eps=0.0)
    for kw in (dict(qpos=z(4, cm.nq, dtype=torch.float32)), dict(ctrl=z(4, cm.nu, device="cpu")), dict(ctrl=z(4, 2, cm.nu)), dict(envs=[0, 1], qpos=z(3, cm.nq)),
               dict(out={"deriv_t": z(4, 2 * cm.nv, ncol)}), dict(out={"status_cols": z(4, ncol)})):
        with pytest.raises(KManipError):
            dev.transition_fd(**kw)
    for kw in (dict(wrt=("qpos", "nonsense")), dict(wrt=("qpos", "qpos")), dict(out={"nonsense": z(4)})):
        with pytest.raises(ValueError):
            dev.transition_fd(**kw)
    # the C ABI's own refusals: nonzero, last_error set, nothing launched -- the outputs keep their sentinel
    sent = dict(qpos=torch.full((4, cm.nq), 77.0, dtype=torch.float64, device="cuda"), qacc_warm=torch.full((4, cm.nv), 77.0, dtype=torch.float64, device="cuda"),
                status=torch.full((4,), 77, dtype=torch.uint8, device="cuda"), deriv_t=torch.full((4, ncol, 2 * cm.nv), 77.0, dtype=torch.float64, device="cuda"),
                status_cols=torch.full((4, ncol), 77, dtype=torch.uint8, device="cuda"), contact_mask_fd=torch.full((4, ncol, 2), 77, dtype=torch.int32, device="cuda"))

    def fout(**drop):
        o = KTransFdDev()
        for k, v in sent.items():
            if k not in drop:
                setattr(o, k, v.data_ptr())
        return o

    def fin(**kw):
        i = KTransFdIn()
        i.wrt, i.eps, i.warm_offset = 7, 1e-6, 1.0
        for k, v in kw.items():
            setattr(i, k, v)
        return i
    ok, fo = fin(), fout()
    index = torch.zeros(4, dtype=torch.int32, device="cuda")          # (a refused call reads none of it)
    refused = ((None, ok, 4, 0, fo, b""), (dev.h, None, 4, 0, fo, b"kmanip_transition_fd: the KTransFdIn pointer is NULL"),
               (dev.h, ok, 4, 0, None, b"kmanip_transition_fd: the KTransFdDev pointer is NULL"), (dev.h, ok, -1, 0, fo, b"n is negative"),
               (dev.h, ok, 4, -1, fo, b"kmanip_transition_fd: nsub is negative"), (dev.h, ok, 5, 0, fo, b"more rows than envs"),
               (dev.h, fin(wrt=16), 4, 0, fo, b"wrt has bits outside"), (dev.h, fin(wrt=-1), 4, 0, fo, b"wrt has bits outside"),
               (dev.h, fin(eps=0.0), 4, 0, fo, b"eps is not a finite positive"), (dev.h, fin(eps=-1e-6), 4, 0, fo, b"eps is not a finite positive"),
               (dev.h, fin(eps=float("nan")), 4, 0, fo, b"eps is not a finite positive"), (dev.h, fin(eps=float("inf")), 4, 0, fo, b"eps is not a finite positive"),
               (dev.h, fin(warm_offset=float("nan")), 4, 0, fo, b"warm_offset is not finite"), (dev.h, fin(warm_offset=float("-inf")), 4, 0, fo, b"warm_offset is not finite"),
               (dev.h, ok, 4, 0, fout(deriv_t=1), b"KTransFdDev::deriv_t is NULL"), (dev.h, ok, 4, 0, fout(qacc_warm=1), b"KTransFdDev::qacc_warm, which is NULL"),
               (dev.h, fin(wrt=15, env_index=index.data_ptr()), 2 ** 31 // (2 * (3 * cm.nv + cm.nu)) + 1, 0, fo, b"more than an int counts"))
    for h, i, n, nsub, o, msg in refused:
        rc = L.kmanip_transition_fd(h, None if i is None else C.byref(i), n, nsub, None if o is None else C.byref(o), None)
        err = L.kmanip_last_error(h)
        assert rc != 0 and (err == msg if msg.startswith(b"kmanip_") else msg in err), (n, nsub, msg, err)
    assert L.kmanip_transition_fd(dev.h, C.byref(ok), 0, 0, C.byref(fo), None) == 0                         # n == 0: succeeds and does nothing
    assert L.kmanip_transition_fd(dev.h, C.byref(fin(wrt=0)), 4, 0, C.byref(KTransFdDev()), None) == 0      # nothing asked for
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in sent.values())
    # wrt == 0: the nominal launch only
    assert L.kmanip_transition_fd(dev.h, C.byref(fin(wrt=0)), 4, 0, C.byref(fo), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(sent["qpos"], good["qpos"]) and not sent["status"].any() and bool((sent["deriv_t"] == 77).all()) and bool((sent["status_cols"] == 77).all())
    # the handle works afterwards
    assert L.kmanip_transition_fd(dev.h, C.byref(ok), 4, 0, C.byref(fo), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(sent["deriv_t"], good["deriv_t"]) and not sent["status_cols"].any()
    assert torch.equal(sent["contact_mask_fd"], good["contact_mask_fd"].permute(2, 0, 1))
    empty = dev.transition_fd(envs=torch.zeros((0,), dtype=torch.int32, device="cuda"))
    assert tuple(empty["qpos"].shape) == (0, cm.nq) and "A" not in empty
    dev.step_flat(z(4, cm.act_dim, dtype=torch.float32))
    assert not dev.done.cpu().numpy().any()
    dev.k_close()


# ----------------------------------------------------------------------------------------------------------------- 5. handle read-only
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_handle_is_read_only(asset):
    """Two identical handles holding six cells, three steps; one calls transition_fd -- stored rows, overriding rows, more rows than
    envs with a differentiated force -- before each.  State, diagnostics and sample_action before and after equal; the next
    step_flat gives the bytes of the twin that never made the call."""
    torch = _torch()
    from test_forces_gpu import _device
    cm, rows, tau = _rows(asset)
    host = {k: v.cpu().numpy() for k, v in rows.items()}
    n = 6
    a, b = (_device(cm, host["qpos"], host["qvel"], host["ctrl"], host["warm"]) for _ in range(2))
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)
    for k in range(3):
        before, diag, sample = a.state_tensors(), a.get_diag(), a.sample_action().clone()
        a.transition_fd()
        a.transition_fd(qpos=rows["qpos"], qvel=rows["qvel"], ctrl=rows["ctrl"], warm=rows["warm"], nsub=3)
        a.transition_fd(envs=np.arange(2 * n)[::-1] % n, qvel=torch.cat([rows["qvel"], rows["qvel"]]), qfrc_applied=torch.cat([tau, tau]), nsub=2, wrt=ALL)
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), k
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), k
        assert torch.equal(sample, a.sample_action()), k
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), k
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
        assert torch.equal(a.sim_time, b.sim_time)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_diag(), b.get_diag())), k
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. iLQR
def test_ilqr_fused_on_the_device_and_the_example(capsys):
    """KManipSoloArmQPos, 4 envs, horizon 4, 2 iterations, 3 alphas, --fused: the accepted cost never increases and every env's is
    lower after the first iteration."""
    import math
    from gym_kmanip_amd.examples import ilqr_reach
    out = ilqr_reach.main(["--num-envs", "4", "--horizon", "4", "--iters", "2", "--alphas", "1.0", "0.5", "0.25", "--fused"])
    print(capsys.readouterr().out)
    cost = np.asarray(out["cost_per_env"])
    assert out["fused"] is True and cost.shape == (3, 4) and np.isfinite(cost).all()
    assert (np.diff(cost, axis=0) <= 0).all() and (cost[1] < cost[0]).all()
    assert out["rows_per_line_search"] == 12 and out["feedback_launches"] == 2 and all(math.isfinite(c) for c in out["cost"])
