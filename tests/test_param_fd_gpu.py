"""kmanip_param_fd on the device (run with -m gpu on an MI355X): KManipEnvHip.param_fd, and gym_kmanip_amd.sysid on top of it.

The rows are the six cells per asset of rollout_oracle.FD_CELLS on handles of 2 envs (envs = arange(6) % 2): more rows than envs,
6 x npar pairs, not a multiple of the pairs a wave holds.  Against the oracle (tests/tools/paramfd_oracle.py) the bars are
tests/test_param_fd_cpu.py's BAR_P as they stand.  Against KManipEnvHip.rollout on the same handle with set_env_params at plus and at
minus the sub-step source and the derived constants are the same, so the perturbed rows' masks are compared byte for byte, and so are
the joint, cube-position and qvel rows of the quotient once the numerators are DIVIDED by a tensor on the device (torch divides by a
Python number through its reciprocal: tests/test_transfd_gpu.py); the three cube-rotation rows pass through atan2 and are held within
test_transfd_gpu.ROT_ULPS, as argued there.  Everything that compares the kernel with itself is bit for bit.
What the device showed: DESIGN.md section 42."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import paramfd_oracle as PO  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu

# (asset, solver, mode) of the comparison with rollout on the same handle: env 1 with parameters of its own, the same with a given
# force -- and a handle that never had parameters with a BOUND force.  tests/test_param_fd_cpu.py checks that these rows launch every
# k_paramfd object the Makefile compiles.
HANDLE_ROWS = ([(a, s, m) for a in ("solo_arm", "dual_arm") for s in ("newton", "pgs") for m in ("params", "params+forced")]
               + [("solo_arm", "newton", "bound")])
# the joint, cube-position and qvel rows of the quotient against the handle's own rollouts, byte for byte
ROLLOUT_BYTES_EQUAL = True
EPS = 1e-4
RAW = ("deriv_t", "status_cols", "contact_mask_fd")
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


def _two_env_params(cm):
    """{name: [2] device tensor}: env 0 the compiled model's values, env 1 the check values (every one above 0)."""
    from gym_kmanip_amd.model import ENV_PARAMS, env_param_defaults
    base, true = env_param_defaults(cm), PO.true_params(cm)
    return {name: _t(np.array([base[name], true[name]])) for name in ENV_PARAMS}


def _bytes_differ(f, g, keys):
    torch = _torch()
    return [k for k in keys if not torch.equal(f[k], g[k])]


# ------------------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("nsub", [1, None], ids=["mj_step", "control_step"])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_param_fd_against_the_reference(asset, nsub):
    """KManipEnvHip.param_fd against paramfd_oracle.reference on the FD_CELLS rows at the check values, one mj_step and one control
    step: both column kinds within BAR_P, the contact masks of all perturbed rows equal, every column's status 0."""
    torch = _torch()
    from test_param_fd_cpu import BAR_P, SPREAD_P
    from gym_kmanip_amd.model import ENV_PARAMS
    cm, rows, p, ref = PO.reference(asset, nsub)
    n, nv = len(rows["qpos"]), cm.nv
    dev = _fresh(cm, 2)
    got = dev.param_fd(nsub=nsub, params=_t(p), **{k: _t(v) for k, v in rows.items()})
    torch.cuda.synchronize()
    dev.k_close()
    assert tuple(got["deriv_t"].shape) == (n, 4, 2 * nv) and tuple(got["P"].shape) == (n, 2 * nv, 4) and got["P"].data_ptr() == got["deriv_t"].data_ptr()
    assert got["wrt"] == ENV_PARAMS and not got["status_cols"].any() and not got["status_fd"].any() and not ref["status_cols"].any()
    assert np.array_equal(got["contact_mask_fd"].permute(2, 0, 1).cpu().numpy(), ref["contact_mask_fd"])
    dist = RO.fd_dist(PO.blocks(ref["deriv_t"], nv), PO.blocks(got["deriv_t"].cpu().numpy(), nv))
    print("\n%s, nsub %s: worst normalised |device - oracle| per column kind (the reference's spread; the bar): %s"
          % (asset, nsub or "the model's", "  ".join("%s %.1e in %s (%.1e; %.0e)" % (k, v.max(), RO.FD_CELLS[asset][int(v.argmax())], SPREAD_P[nsub][k], BAR_P[nsub][k])
                                                     for k, v in dist.items())))
    bad = [(k, RO.FD_CELLS[asset][e], float(v[e]), BAR_P[nsub][k]) for k, v in dist.items() for e in range(n) if not v[e] <= BAR_P[nsub][k]]
    assert not bad, bad
    assert float(got["deriv_t"].abs().max()) > 0.1


# ----------------------------------------------------------------------------------------- 2. against rollout on the same handle
def _quotients_from_rollouts(dev, cm, rows, tau, base, nsub):
    """(deriv_t [n, 4, 2 nv], contact_mask_fd [4, 2, n]) assembled from the handle's own kernels: per parameter set_env_params at plus and
    at minus (every env's own p_k +- fl(EPS p_k)), one rollout of the rows each from warm + 1, derivatives.tangent_diff, and a division by
    a TENSOR holding fl(2.0 * e).  The handle's parameters are put back."""
    torch = _torch()
    from gym_kmanip_amd.derivatives import tangent_diff
    from gym_kmanip_amd.model import ENV_PARAMS
    envs = rows["envs"].long()
    cols, masks = [], []
    for name in ENV_PARAMS:
        p = base[name]
        e = p * EPS
        ends = []
        for val in (p + e, p - e):
            dev.set_env_params(**dict(base, **{name: val}))
            ends.append(dev.rollout(envs=rows["envs"], qpos=rows["qpos"], qvel=rows["qvel"], ctrl=rows["ctrl"], warm=rows["warm"] + 1.0,
                                    qfrc_applied=tau, nstep=1, nsub=nsub, fields=("qpos", "qvel", "contact_mask", "status")))
            assert not ends[-1]["status"].any()
        num = torch.cat([tangent_diff(cm, ends[0]["qpos"][:, 0], ends[1]["qpos"][:, 0]), ends[0]["qvel"][:, 0] - ends[1]["qvel"][:, 0]], dim=1)
        cols.append(num / (2.0 * e)[envs][:, None].expand_as(num).contiguous())
        masks.append(torch.stack([ends[0]["contact_mask"][:, 0], ends[1]["contact_mask"][:, 0]]))
    dev.set_env_params(**base)
    return torch.stack(cols, dim=1), torch.stack(masks)


@pytest.mark.parametrize("asset,solver,mode", HANDLE_ROWS)
def test_param_fd_against_rollout_on_the_same_handle(asset, solver, mode):
    """KManipEnvHip.param_fd (params None: the handle's own) against the quotient assembled from set_env_params and two rollout calls per
    parameter on the same handle of 2 envs, the FD_CELLS rows, nsub = 1, on the rows that launch every k_paramfd object: the masks
    byte for byte, the joint, cube-position and qvel rows byte for byte (ROLLOUT_BYTES_EQUAL), the rotation rows within ROT_ULPS; the
    handle's parameters are the ones it had."""
    torch = _torch()
    from test_transfd_gpu import ROT_ULPS
    from gym_kmanip_amd.model import ENV_PARAMS, env_param_defaults
    cm, rows, tau = _rows(asset, solver)
    dev = _fresh(cm, 2)
    had = "params" in mode
    base = _two_env_params(cm) if had else {k: _t(np.full(2, v)) for k, v in env_param_defaults(cm).items()}
    if had:
        dev.set_env_params(**base)
    if mode == "bound":
        dev.new_applied_force().copy_(tau[:2])
    given = tau if "forced" in mode else None
    got = dev.param_fd(nsub=1, qfrc_applied=given, **rows)
    assert not got["status_cols"].any() and got["wrt"] == ENV_PARAMS and float(got["deriv_t"].abs().max()) > 0.1
    want, masks = _quotients_from_rollouts(dev, cm, rows, given, base, 1)
    if had:
        now = dev.get_env_params()
        assert all(torch.equal(now[k], base[k]) for k in ENV_PARAMS)
    else:
        dev.clear_env_params()
    assert torch.equal(got["contact_mask_fd"], masks), (asset, solver, mode)
    nl, nv = cm.nlink, cm.nv
    rot = torch.zeros(2 * nv, dtype=torch.bool, device="cuda")
    rot[nl + 3:nl + 6] = True
    a, b = got["deriv_t"], want
    d = (a - b).abs() / b.abs().clamp(min=1e-300) / 2.0 ** -52
    worst = (float(d[:, :, ~rot].max()), float(d[:, :, rot].max()))
    same = torch.equal(a[:, :, ~rot], b[:, :, ~rot])
    print("\n%s %s %s: worst |param_fd - rollouts| in units of 2^-52 |entry|, joint / cube-position / qvel rows and rotation rows: %.2f / %.2f; "
          "byte equality of the first kind: %s" % (asset, solver, mode, worst[0], worst[1], same))
    assert worst[1] <= ROT_ULPS, worst
    if ROLLOUT_BYTES_EQUAL:
        assert same, worst
    # the call again after the handle went through plus and minus: the same bytes
    again = dev.param_fd(nsub=1, qfrc_applied=given, **rows)
    assert _bytes_differ(got, again, RAW) == []
    dev.k_close()


# --------------------------------------------------------------------------------------------- 3. the kernel against itself, bit for bit
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_kernel_against_itself_bit_for_bit(asset):
    """Two sub-steps.  params given as rows against the same values set on the handle; a handle that never had parameters against one
    given the model's defaults, as rows and with set_env_params; a column's bytes whatever n, the row's place and wrt's other bits;
    with and without contact_mask_fd; relative against the same absolute steps."""
    torch = _torch()
    from gym_kmanip_amd.model import ENV_PARAMS, env_param_defaults
    cm, rows, tau = _rows(asset)
    n = 6
    # ---- a handle with parameters: None against rows
    dev = _fresh(cm, 2)
    base = _two_env_params(cm)
    dev.set_env_params(**base)
    kw = dict(rows, nsub=2)
    full = dev.param_fd(**kw)
    assert not full["status_cols"].any()
    as_rows = torch.stack([base[name][rows["envs"].long()] for name in ENV_PARAMS], dim=1).contiguous()
    plain = _fresh(cm, 2)                                                  # (a handle that never had parameters is handed them as rows)
    for h in (dev, plain):
        assert _bytes_differ(full, h.param_fd(params=as_rows, **kw), RAW) == []
        assert _bytes_differ(full, h.param_fd(params={name: as_rows[:, k] for k, name in enumerate(ENV_PARAMS)}, **kw), RAW) == []
    assert _bytes_differ(full, dev.param_fd(params={"kp_scale": as_rows[:, 3]}, **kw), RAW) == []      # unnamed: the env's own
    # ---- a handle that never had parameters: None = the compiled model's values, by value
    dflt = env_param_defaults(cm)
    none = plain.param_fd(qfrc_applied=tau, **kw)
    assert not none["status_cols"].any() and plain._ep_active is False
    rows_d = torch.tensor([[dflt[name] for name in ENV_PARAMS]] * n, dtype=torch.float64, device="cuda")
    assert _bytes_differ(none, plain.param_fd(params=rows_d, qfrc_applied=tau, **kw), RAW) == []
    given = _fresh(cm, 2)
    given.set_env_params(**dflt)
    assert _bytes_differ(none, given.param_fd(qfrc_applied=tau, **kw), RAW) == []
    given.k_close()
    # ---- rows reversed, each row alone, a handle of 5 envs under a repeated index
    flip = lambda v: v.flip(0).contiguous() if isinstance(v, torch.Tensor) else v
    rev = plain.param_fd(params=flip(as_rows), **{k: flip(v) for k, v in kw.items()})
    assert [k for k in RAW if not torch.equal(rev[k].flip(-1 if k == "contact_mask_fd" else 0), full[k])] == []
    for e in (0, 3, 5):
        one = plain.param_fd(params=as_rows[e:e + 1].contiguous(), **{k: (v[e:e + 1].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        assert [k for k in RAW if not torch.equal(one[k], full[k][..., e:e + 1] if k == "contact_mask_fd" else full[k][e:e + 1])] == [], e
    big = _fresh(cm, 5)
    assert _bytes_differ(full, big.param_fd(params=as_rows, **dict(kw, envs=_t(np.array([3, 1, 3, 3, 1, 3], np.int32)))), RAW) == []
    big.k_close()
    # ---- every subset of wrt gives the bytes of its columns, in ENV_PARAMS order whatever the caller's
    for sub in (("kp_scale",), ("cube_frictionloss", "cube_mass"), ("cube_friction", "kp_scale", "cube_frictionloss"), "cube_mass"):
        part = dev.param_fd(wrt=sub, **kw)
        cols = [k for k, name in enumerate(ENV_PARAMS) if name in ((sub,) if isinstance(sub, str) else sub)]
        assert part["wrt"] == tuple(ENV_PARAMS[k] for k in cols)
        assert torch.equal(part["deriv_t"], full["deriv_t"][:, cols]) and torch.equal(part["status_cols"], full["status_cols"][:, cols])
        assert torch.equal(part["contact_mask_fd"], full["contact_mask_fd"][cols]), sub
    none_wrt = dev.param_fd(wrt=(), **kw)
    assert tuple(none_wrt["deriv_t"].shape) == (n, 0, 2 * cm.nv) and none_wrt["wrt"] == ()
    # ---- with and without contact_mask_fd; relative against the same steps given absolute
    lean = dev.param_fd(out={"status_cols": torch.empty((n, 4), dtype=torch.uint8, device="cuda")}, **kw)
    assert "contact_mask_fd" not in lean and _bytes_differ(lean, full, ("deriv_t", "status_cols")) == []
    one_env = {k: (v[1:2].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}          # (row 1: env 1)
    absolute = dev.param_fd(relative=False, eps={name: float(base[name][1]) * EPS for name in ENV_PARAMS}, **one_env)
    assert [k for k in RAW if not torch.equal(absolute[k], full[k][..., 1:2] if k == "contact_mask_fd" else full[k][1:2])] == []
    dev.k_close(); plain.k_close()


# ------------------------------------------------------------------------------------------------------------ 4. status and refusals
def test_bad_rows_get_their_status_and_zero_columns_and_harm_nobody():
    """In the middle of the rows: an index outside the handle (2), a NaN state, ctrl, warm start or force (1), a friction loss of 0, a
    parameter outside its domain and a perturbed mass below 0 (3): zero columns, zero masks, the other rows' bytes those of the same
    call without the bad entry."""
    torch = _torch()
    cm, rows, tau = _rows("solo_arm")
    n, e = 6, 3
    dev = _fresh(cm, 2)
    dev.set_env_params(**PO.true_params(cm))             # (both envs hold what the rows are given: params None means the same values)
    par = _t(PO.fd_params(cm, n))
    keep = torch.arange(n, device="cuda") != e
    absolute = dict(relative=False, eps={"cube_mass": 1e-3, "cube_friction": 1e-4, "cube_frictionloss": 1e-3, "kp_scale": 1e-4})
    for kw in (dict(rows, nsub=1, params=par), dict(rows, nsub=1, params=par, qfrc_applied=tau)):

        def check(status, cols=slice(None), **bad):
            clean, g = dev.param_fd(**kw) if not set(bad) & set(absolute) else dev.param_fd(**dict(kw, **absolute)), dev.param_fd(**dict(kw, **bad))
            assert not clean["status_cols"].any()
            hit = torch.zeros((n, 4), dtype=torch.bool, device="cuda")
            hit[e, cols] = True
            assert bool((g["status_cols"][hit] == status).all()) and not g["status_cols"][~hit].any() and int(g["status_fd"][e]) == status
            assert not g["deriv_t"][hit].any() and not g["contact_mask_fd"].permute(2, 0, 1)[hit].any() and not g["P"].transpose(1, 2)[hit].any()
            assert bool(g["deriv_t"][e][~hit[e]].any()) or bool(hit[e].all())          # the row's other columns are derivatives
            for k in RAW:
                a, b = (g[k], clean[k]) if k != "contact_mask_fd" else (g[k].permute(2, 0, 1), clean[k].permute(2, 0, 1))
                assert torch.equal(a[keep], b[keep]), k
        for idx in (2, -1, 2 ** 31 - 1, -2 ** 31):
            ie = rows["envs"].cpu().numpy().copy()
            ie[e] = idx
            check(2, envs=_t(ie, np.int32))
            check(2, envs=_t(ie, np.int32), params=None)                                # (the env's own parameters are not read either)
        assert dev.state_index_errors() == 0
        for name, at in (("qpos", (e, -1)), ("qvel", (e, 3)), ("ctrl", (e, 0)), ("warm", (e, 2))) + ((("qfrc_applied", (e, 1)),) if "qfrc_applied" in kw else ()):
            t = kw[name].clone()
            t[at] = float("nan")
            check(1, **{name: t})
        p3 = par.clone()
        p3[e, 2] = 0.0                                   # a friction loss of 0: that column alone (relative: e = 0)
        check(3, [2], params=p3)
        check(3, [2], params=p3, **absolute)             # (absolute: minus < 0)
        p3 = par.clone()
        p3[e, 1] = float("nan")                          # a parameter outside its domain: the row's every column
        check(3, params=p3)
        p3[e, 1] = -0.5
        check(3, params=p3)
        p3 = par.clone()
        p3[e, 0] = 1e-4                                  # an absolute step larger than the mass: a negative perturbed mass
        check(3, [0], params=p3, **absolute)
    dev.k_close()


def test_refusals_launch_nothing_and_leave_the_outputs_untouched():
    torch = _torch()
    from gym_kmanip_amd.lib import KManipError, KParamFdDev, KParamFdIn
    dev = _fresh(R.model("solo_arm"), 4)
    cm, L = dev.cm, dev.L
    good = dev.param_fd()
    assert not good["status_cols"].any() and tuple(good["P"].shape) == (4, 2 * cm.nv, 4)
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    with pytest.raises(KManipError, match="more rows than envs"):
        dev.param_fd(qvel=z(5, cm.nv))
    with pytest.raises(KManipError, match="negative"):
        dev.param_fd(nsub=-1)
    with pytest.raises(KManipError, match="eps"):
        dev.param_fd(eps=0.0)
    for kw in (dict(qpos=z(4, cm.nq, dtype=torch.float32)), dict(ctrl=z(4, cm.nu, device="cpu")), dict(params=z(4, 3)), dict(params=z(3, 4)),
               dict(out={"deriv_t": z(4, 2 * cm.nv, 4)}), dict(out={"status_cols": z(4, 4)})):
        with pytest.raises(KManipError):
            dev.param_fd(**kw)
    for kw in (dict(wrt=("kp_scale", "nonsense")), dict(wrt=("kp_scale", "kp_scale")), dict(out={"nonsense": z(4)}), dict(params={"nonsense": 1.0})):
        with pytest.raises(ValueError):
            dev.param_fd(**kw)
    # the C ABI's own refusals: nonzero, last_error set, nothing launched -- the outputs keep their sentinel
    sent = dict(deriv_t=torch.full((4, 4, 2 * cm.nv), 77.0, dtype=torch.float64, device="cuda"),
                status_cols=torch.full((4, 4), 77, dtype=torch.uint8, device="cuda"), contact_mask_fd=torch.full((4, 4, 2), 77, dtype=torch.int32, device="cuda"))

    def fout(**drop):
        o = KParamFdDev()
        for k, v in sent.items():
            if k not in drop:
                setattr(o, k, v.data_ptr())
        return o

    def fin(eps=None, **kw):
        i = KParamFdIn()
        i.wrt, i.eps_relative, i.warm_offset = 15, 1, 1.0
        for k in range(4):
            i.eps[k] = 1e-4
        for k, v in (eps or {}).items():
            i.eps[k] = v
        for k, v in kw.items():
            setattr(i, k, v)
        return i
    ok, fo = fin(), fout()
    index = torch.zeros(4, dtype=torch.int32, device="cuda")          # (a refused call reads none of it)
    nan, inf = float("nan"), float("inf")
    refused = ((None, ok, 4, 0, fo, b""), (dev.h, None, 4, 0, fo, b"kmanip_param_fd: the KParamFdIn pointer is NULL"),
               (dev.h, ok, 4, 0, None, b"kmanip_param_fd: the KParamFdDev pointer is NULL"), (dev.h, ok, -1, 0, fo, b"n is negative"),
               (dev.h, ok, 4, -1, fo, b"kmanip_param_fd: nsub is negative"), (dev.h, ok, 5, 0, fo, b"more rows than envs"),
               (dev.h, fin(wrt=16), 4, 0, fo, b"wrt has bits outside"), (dev.h, fin(wrt=-1), 4, 0, fo, b"wrt has bits outside"),
               (dev.h, fin(eps={0: 0.0}), 4, 0, fo, b"eps[0] of a selected parameter"), (dev.h, fin(eps={1: -1e-4}), 4, 0, fo, b"eps[1] of a selected parameter"),
               (dev.h, fin(eps={2: nan}), 4, 0, fo, b"eps[2] of a selected parameter"), (dev.h, fin(eps={3: inf}), 4, 0, fo, b"eps[3] of a selected parameter"),
               (dev.h, fin(warm_offset=nan), 4, 0, fo, b"warm_offset is not finite"), (dev.h, fin(warm_offset=-inf), 4, 0, fo, b"warm_offset is not finite"),
               (dev.h, ok, 4, 0, fout(deriv_t=1), b"KParamFdDev::deriv_t is NULL"),
               (dev.h, fin(env_index=index.data_ptr()), 2 ** 31 // 8 + 1, 0, fo, b"more than an int counts"))
    for h, i, n, nsub, o, msg in refused:
        rc = L.kmanip_param_fd(h, None if i is None else C.byref(i), n, nsub, None if o is None else C.byref(o), None)
        err = L.kmanip_last_error(h)
        assert rc != 0 and (err == msg if msg.startswith(b"kmanip_") else msg in err), (n, nsub, msg, err)
    assert L.kmanip_param_fd(dev.h, C.byref(ok), 0, 0, C.byref(fo), None) == 0                              # n == 0: succeeds and does nothing
    assert L.kmanip_param_fd(dev.h, C.byref(fin(wrt=0)), 4, 0, C.byref(fo), None) == 0                      # wrt == 0 likewise
    assert L.kmanip_param_fd(dev.h, C.byref(fin(wrt=0)), 4, 0, C.byref(KParamFdDev()), None) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in sent.values())
    # the eps of a parameter that is not selected is not read
    assert L.kmanip_param_fd(dev.h, C.byref(fin(wrt=8, eps={0: nan, 1: -1.0, 2: 0.0})), 4, 0, C.byref(fo), None) == 0
    torch.cuda.synchronize()
    flat = sent["deriv_t"].reshape(-1, 2 * cm.nv)                        # (one column per row: the first four runs of 2 nv doubles)
    assert torch.equal(flat[:4], good["deriv_t"][:, 3]) and bool((flat[4:] == 77).all()) and not sent["status_cols"].reshape(-1)[:4].any()
    # the handle works afterwards
    assert L.kmanip_param_fd(dev.h, C.byref(ok), 4, 0, C.byref(fo), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(sent["deriv_t"], good["deriv_t"]) and not sent["status_cols"].any()
    assert torch.equal(sent["contact_mask_fd"], good["contact_mask_fd"].permute(2, 0, 1))
    empty = dev.param_fd(envs=torch.zeros((0,), dtype=torch.int32, device="cuda"))
    assert tuple(empty["deriv_t"].shape) == (0, 4, 2 * cm.nv) and tuple(empty["P"].shape) == (0, 2 * cm.nv, 4)
    dev.step_flat(z(4, cm.act_dim, dtype=torch.float32))
    assert not dev.done.cpu().numpy().any()
    dev.k_close()


# ----------------------------------------------------------------------------------------------------------------- 5. handle read-only
@pytest.mark.parametrize("mode", ["plain", "params"])
def test_the_handle_is_read_only(mode):
    """Two identical handles holding six cells, three steps; one calls param_fd -- stored rows, overriding rows, more rows than envs with
    a force and parameters as rows -- before each.  State, parameters, diagnostics and sample_action before and after equal; the next
    step_flat gives the bytes of the twin that never made the call -- also on a handle without parameters, whose steps stay the
    default kernels'."""
    torch = _torch()
    from test_forces_gpu import _device
    from gym_kmanip_amd.model import ENV_PARAMS
    cm, rows, tau = _rows("solo_arm")
    host = {k: v.cpu().numpy() for k, v in rows.items()}
    n = 6
    a, b = (_device(cm, host["qpos"], host["qvel"], host["ctrl"], host["warm"]) for _ in range(2))
    if mode == "params":
        vals = {name: _t(np.linspace(1.0, 1.5, n) * v) for name, v in PO.true_params(cm).items()}
        a.set_env_params(**vals); b.set_env_params(**vals)
    par = _t(PO.fd_params(cm, 2 * n))
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, n, cm.act_dim)).astype(np.float32)
    for k in range(3):
        before, params, diag, sample = a.state_tensors(), a.get_env_params(), a.get_diag(), a.sample_action().clone()
        a.param_fd()
        a.param_fd(qpos=rows["qpos"], qvel=rows["qvel"], ctrl=rows["ctrl"], warm=rows["warm"], nsub=3, wrt=("kp_scale", "cube_mass"))
        a.param_fd(envs=np.arange(2 * n)[::-1] % n, qvel=torch.cat([rows["qvel"], rows["qvel"]]), qfrc_applied=torch.cat([tau, tau]), params=par, nsub=2)
        after, params_after = a.state_tensors(), a.get_env_params()
        assert all(torch.equal(before[key], after[key]) for key in before), k
        assert all(torch.equal(params[key], params_after[key]) for key in ENV_PARAMS) and a._ep_active is (mode == "params"), k
        assert all(np.array_equal(x, y) for x, y in zip(diag, a.get_diag())), k
        assert torch.equal(sample, a.sample_action()), k
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), k
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------------------------------ 6. sysid
class _Linear:
    """tests/test_param_fd_cpu.py's linear loss on device tensors."""

    def __init__(self, cm, w):
        from test_param_fd_cpu import _LinearCost
        self._c = _LinearCost(cm, w)
        self.total, self.derivatives = self._c.total, self._c.derivatives


def test_rollout_param_grad_on_the_device_against_the_centred_loss_difference():
    """KManipSoloArmQPos, 2 envs stepped four times from reset with parameters of their own, T = 4 control steps, a linear loss:
    rollout_param_grad(device=True, fused=True) -- kmanip_transition_fd, kmanip_adjoint, kmanip_param_fd -- against the centred
    difference of the loss at h = 1e-4 through set_env_params and rollout, each parameter's entry times the parameter and normalised
    by the env's largest.  The plain path (device=False, fused=False) is held to tests/test_param_fd_cpu.py's BAR_GRAD, and that is
    the bar of the device path too; the two paths differ by no more than the same bar."""
    torch = _torch()
    from test_param_fd_cpu import BAR_GRAD
    from gym_kmanip_amd import env_hip, sysid
    from gym_kmanip_amd.model import ENV_PARAMS
    env = env_hip.make("KManipSoloArmQPos", num_envs=2, seed=3)
    env.k_reset()
    base = {k: _t(np.array([v, 1.1 * v])) for k, v in PO.true_params(env.cm).items()}
    env.set_env_params(**base)
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    T, cm = 4, env.cm
    ctrl = st["ctrl"][:, None, :].repeat(1, T, 1)
    w = _t(np.random.default_rng(5).standard_normal((2, T + 1, 2 * cm.nv)))
    cost = _Linear(cm, w)
    plain = sysid.rollout_param_grad(env, None, st["qpos"], st["qvel"], st["warm"], ctrl, cost)
    fused = sysid.rollout_param_grad(env, None, st["qpos"], st["qvel"], st["warm"], ctrl, cost, fused=True, device=True)
    for g in (plain, fused):
        assert not g["status"].any() and not g["status_fd"].any() and not g["status_param"].any() and g["wrt"] == ENV_PARAMS
    idx = torch.arange(2, dtype=torch.int32, device="cuda")

    def loss(params):
        env.set_env_params(**params)
        r = env.rollout(envs=idx, qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl, fields=("qpos", "qvel", "status"))
        assert not r["status"].any()
        return cost.total(torch.cat([st["qpos"][:, None], r["qpos"]], 1), torch.cat([st["qvel"][:, None], r["qvel"]], 1), ctrl)
    h = 1e-4
    cd = torch.stack([(loss(dict(base, **{k: base[k] * (1 + h)})) - loss(dict(base, **{k: base[k] * (1 - h)}))) / (2 * h) for k in ENV_PARAMS], dim=1)
    env.set_env_params(**base)
    pv = torch.stack([base[k] for k in ENV_PARAMS], dim=1)
    scale = cd.abs().max(dim=1, keepdim=True).values
    assert bool((scale > 1e-6).all())
    err = {name: float(((g["grad_params"] * pv - cd).abs() / scale).max()) for name, g in (("plain", plain), ("device", fused))}
    apart = float(((fused["grad_params"] - plain["grad_params"]).abs() * pv / scale).max())
    print("\nrollout_param_grad against the centred difference: plain %.2e, fused + device %.2e (bar %.0e); the two paths %.2e apart; p dL/dp %s"
          % (err["plain"], err["device"], BAR_GRAD, apart, (plain["grad_params"] * pv).tolist()))
    assert err["plain"] <= BAR_GRAD and err["device"] <= BAR_GRAD and apart <= BAR_GRAD
    env.k_close()


def test_identify_recovers_kp_scale_on_the_device(capsys):
    """The example's loop on two handles of 2 envs, kp_scale alone (observable from the arm without any contact), fused, 5 iterations:
    both envs' hidden values within 1e-6 relative, the loss never rises, the real handle untouched, the model handle holding the
    estimate."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.examples import system_identification as ex
    real, model = (env_hip.make("KManipSoloArmQPos", num_envs=2, seed=3) for _ in range(2))
    real.k_reset(); model.k_reset()
    hidden = _t(np.array([1.2, 0.85]))
    real.set_env_params(kp_scale=hidden)
    st = model.state_tensors()
    ctrl = ex.sweep_controls(model.cm, st, 4)
    res = ex.identify_log(real, model, st, ctrl, wrt=("kp_scale",), iters=5, fused=True, device_adjoint=True)
    print(capsys.readouterr().out)
    err = res["error"]["kp_scale"]
    print("identify on the device: kp_scale %s, relative error %s, loss %s" % (res["params"]["kp_scale"].tolist(), err.tolist(), res["loss"].tolist()))
    assert float(err.max()) <= 1e-6 and int(res["status"].max()) == 0 and bool(res["observable"].all())
    assert bool((res["loss"][1:] <= res["loss"][:-1]).all()) and tuple(res["grad_params"].shape) == (2, 1)
    assert torch.equal(real.get_env_params()["kp_scale"], hidden) and torch.equal(model.get_env_params()["kp_scale"], res["params"]["kp_scale"])
    with pytest.raises(ValueError, match="ranges mode"):
        model.set_env_param_ranges(kp_scale=(0.9, 1.1))
        from gym_kmanip_amd import sysid
        sysid.identify(model, [0, 1], st["qpos"], st["qvel"], st["warm"], ctrl, res["hidden"]["kp_scale"], res["hidden"]["kp_scale"], iters=1)
    real.k_close(); model.k_close()
