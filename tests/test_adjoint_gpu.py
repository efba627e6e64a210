"""kmanip_adjoint on the device (run with -m gpu on an MI355X): KManipEnvHip.adjoint, derivatives.adjoint_pass in one launch, and
grad.rollout_grad over it.

Handles of 2 envs, KManipSoloArm and KManipDualArm: one per size class (nx, nu) = (32, 10), (52, 20); the problems are not envs, so
3 problems run on a handle of 2.  Against adjoint_reference's longdouble restatement on its family the bar is
tests/test_adjoint_cpu.py's BAR as it stands; on real step Jacobians the bar is 1000 x the distance between torch's adjoint_pass and
its twin on A (1 + 1e-15), measured in the test.  Everything that compares the kernel with itself is bit for bit.  What the device
showed: DESIGN.md section 41."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import adjoint_reference as AR  # noqa: E402
import regime_states as R  # noqa: E402
from test_adjoint_cpu import BAR, N_PROBLEMS, gaps, reference  # noqa: E402

pytestmark = pytest.mark.gpu

ASSET_OF = {(32, 10): "solo_arm", (52, 20): "dual_arm"}
OUT = ("lam", "mu")
_DEV = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _t(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def _handle(cls):
    """The class's handle of 2 envs, made once and shared (adjoint only reads it)."""
    if cls not in _DEV:
        from gym_kmanip_amd import env_hip
        dev = env_hip.KManipEnvHip(R.model(ASSET_OF[cls]), num_envs=2, seed=0)
        dev.k_reset()
        assert (2 * dev.cm.nv, dev.cm.nu) == cls
        _DEV[cls] = dev
    return _DEV[cls]


def _family(cls, T, m, closed=True):
    """(the family's arrays on the device, the longdouble reference) of test_adjoint_cpu.reference."""
    f, ref = reference(cls[0], cls[1], T, m, closed)
    return {name: None if v is None else _t(v) for name, v in f.items()}, ref


def _deriv_t(d, extra=0):
    """transition_fd's buffer of the family's A and B: [n, T, nx + nu + extra, nx], the extra columns (qfrc_applied's place) NaN."""
    torch = _torch()
    parts = [d["A"].transpose(2, 3), d["B"].transpose(2, 3)]
    if extra:
        parts.append(torch.full(tuple(d["A"].shape[:2]) + (extra, int(d["A"].shape[3])), float("nan"), dtype=torch.float64, device="cuda"))
    return torch.cat(parts, dim=2).contiguous()


def _run(dev, d, m, gains=True, **kw):
    return dev.adjoint(d["gx"], kw.pop("gu", d["gu"]), A=d["A"], B=d["B"], gains=d["gains"] if gains else None, m=m, **kw)


def _equal(a, b, rows=None):
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    return all(_torch().equal(pick(a[name]), pick(b[name])) for name in OUT)


def _host(res):
    return dict(lam=res["lam"].cpu().numpy(), mu=res["mu"].cpu().numpy())


# ------------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("cls", AR.CLASSES)
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("m", [1, 3])
def test_the_device_meets_the_bar_against_the_longdouble_restatement(cls, T, m):
    """The family, 3 problems of m vectors, open and closed loop: lam and mu within BAR of the longdouble restatement, relative to
    the row's largest entry, through dense A / B and through the strided deriv_t, whose bytes are the dense path's."""
    torch = _torch()
    dev = _handle(cls)
    for closed in (False, True):
        d, ref = _family(cls, T, m, closed)
        res = _run(dev, d, m, gains=closed)
        strided = dev.adjoint(d["gx"], d["gu"], deriv_t=_deriv_t(d), gains_t=d["gains"].transpose(2, 3).contiguous() if closed else None, m=m)
        g, gs = gaps(_host(res), ref), gaps(_host(strided), ref)
        print("\n%s T %d m %d %s: gap to the longdouble restatement lam %.2e mu %.2e; through deriv_t lam %.2e mu %.2e (bar %.0e)"
              % (cls, T, m, "closed" if closed else "open", g["lam"], g["mu"], gs["lam"], gs["mu"], BAR))
        assert tuple(res["lam"].shape) == (N_PROBLEMS * m, T + 1, cls[0]) and tuple(res["mu"].shape) == (N_PROBLEMS * m, T, cls[1])
        assert torch.equal(res["lam"][:, T], d["gx"][:, T])
        for name in OUT:
            assert g[name] <= BAR and gs[name] <= BAR, (name, closed, g[name], gs[name])
        assert _equal(res, strided)


# ----------------------------------------------------------------------------------------------------------- 2. real derivatives
def test_on_real_step_jacobians_the_device_is_as_close_to_torch_as_torch_is_to_itself():
    """KManipSoloArmQPos, 2 envs, horizon 3, trajectory_fd(fused=True) and ilqr_reach's cost: the device on deriv_t against
    derivatives.adjoint_pass on the A, B views of the same buffer, gx = lx and gu = lu, open loop and under gains of scale 0.1.  The
    bar is the reference's own: adjoint_pass against its twin on A (1 + 1e-15), per quantity relative to the row's largest entry,
    times 1000."""
    torch = _torch()
    from gym_kmanip_amd import env_hip, ilqr
    from gym_kmanip_amd.derivatives import adjoint_pass
    env = env_hip.make("KManipSoloArmQPos", num_envs=2, seed=3)
    cm, n, T = env.cm, 2, 3
    env.k_reset()
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64, device="cuda").repeat(cm.nlink)[:cm.nlink]
    goal = st["qpos"].clone()
    goal[:, :cm.nlink] += 0.1 * sign
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64, device="cuda")
    wq[:cm.nlink] = 10.0
    wq[cm.nv:cm.nv + cm.nlink] = 0.01
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((n, cm.nv), dtype=torch.float64, device="cuda"), wq,
                              torch.full((cm.nu,), 1e-3, dtype=torch.float64, device="cuda"), 10.0 * wq)
    ctrl = st["ctrl"][:, None, :].repeat(1, T, 1)
    fd = ilqr.trajectory_fd(env, None, st["qpos"], st["qvel"], st["warm"], ctrl, fused=True)
    assert tuple(fd["deriv_t"].shape) == (n, T, 2 * cm.nv + cm.nu, 2 * cm.nv) and not fd["status"].any() and not fd["status_fd"].any()
    lx, lu = cost.derivatives(fd["qpos"], fd["qvel"], ctrl)[:2]
    K = _t(0.1 * np.random.default_rng(4).standard_normal((n, T, cm.nu, 2 * cm.nv)))
    rel = lambda a, b: float(((a - b).abs().reshape(n, -1).amax(dim=1) / b.abs().reshape(n, -1).amax(dim=1)).max())
    for gains in (None, K):
        want = dict(zip(OUT, adjoint_pass(fd["A"], fd["B"], lx, lu, gains)))
        twin = dict(zip(OUT, adjoint_pass(fd["A"] * (1.0 + 1e-15), fd["B"], lx, lu, gains)))
        got = env.adjoint(lx, lu, deriv_t=fd["deriv_t"], gains=gains)
        for name in OUT:
            spread, gap = rel(twin[name], want[name]), rel(got[name], want[name])
            print("\nreal Jacobians, %s %s: torch against its twin %.3e, the device against torch %.3e (bar %.3e); largest |%s| %.3e"
                  % ("closed" if gains is not None else "open", name, spread, gap, 1000.0 * spread, name, float(want[name].abs().max())))
            assert gap <= 1000.0 * spread, (name, gap, spread)
    env.k_close()


# ------------------------------------------------------------------------------------------------------- 3. bit for bit against itself
@pytest.mark.parametrize("cls", AR.CLASSES)
def test_the_kernel_agrees_with_itself_bit_for_bit(cls):
    """T = 5, m = 3, closed loop: each problem alone is its rows of the batch; the problems reversed give the rows reversed; row j of
    m = 3 is the m = 1 run of that vector; nx + 3 vectors -- two workgroups a problem -- give the rows of single runs; deriv_t with
    NaN columns after ctrl's (qfrc_applied's place: skipped by the stride) equals the dense path; zero gains give the open-loop
    bytes; no gu equals a gu of zeros; lam and mu of steps 3 .. 4 equal those of the T = 2 problem made of these two steps; outputs
    the caller hands in are the ones filled, and asking for one of the two changes nothing in it."""
    torch = _torch()
    dev = _handle(cls)
    nx, nu = cls
    n, m, T = N_PROBLEMS, 3, 5
    d, _ = _family(cls, T, m)
    full = _run(dev, d, m)
    rows = lambda t, e: t[e * m:(e + 1) * m]
    for e in range(n):
        one = dev.adjoint(rows(d["gx"], e).contiguous(), rows(d["gu"], e).contiguous(), A=d["A"][e:e + 1].contiguous(), B=d["B"][e:e + 1].contiguous(),
                          gains=d["gains"][e:e + 1].contiguous(), m=m)
        assert all(torch.equal(one[name], rows(full[name], e)) for name in OUT), e
        for j in range(m):
            r = e * m + j
            single = dev.adjoint(d["gx"][r:r + 1].contiguous(), d["gu"][r:r + 1].contiguous(), A=d["A"][e:e + 1].contiguous(),
                                 B=d["B"][e:e + 1].contiguous(), gains=d["gains"][e:e + 1].contiguous(), m=1)
            assert all(torch.equal(single[name][0], full[name][r]) for name in OUT), (e, j)
    flip_rows = lambda t: t.reshape((n, m) + tuple(t.shape[1:])).flip(0).reshape(t.shape).contiguous()
    rev = dev.adjoint(flip_rows(d["gx"]), flip_rows(d["gu"]), A=d["A"].flip(0).contiguous(), B=d["B"].flip(0).contiguous(),
                      gains=d["gains"].flip(0).contiguous(), m=m)
    assert all(torch.equal(flip_rows(rev[name]), full[name]) for name in OUT)
    # more vectors than one workgroup carries: vector j of problem e is row (e, j % 3) of the family, every one its single run's bytes
    big = nx + 3
    pick = torch.tensor([e * m + j % m for e in range(n) for j in range(big)], device="cuda")
    many = dev.adjoint(d["gx"][pick].contiguous(), d["gu"][pick].contiguous(), A=d["A"], B=d["B"], gains=d["gains"], m=big)
    assert all(torch.equal(many[name], full[name][pick]) for name in OUT)
    wide = dev.adjoint(d["gx"], d["gu"], deriv_t=_deriv_t(d, extra=nx // 2), gains=d["gains"], m=m)
    assert _equal(wide, full) and bool(torch.isfinite(wide["lam"]).all())
    open_loop = _run(dev, d, m, gains=False)
    assert not _equal(open_loop, full)
    assert _equal(dev.adjoint(d["gx"], d["gu"], A=d["A"], B=d["B"], gains=torch.zeros_like(d["gains"]), m=m), open_loop)
    for gains in (False, True):
        assert _equal(_run(dev, d, m, gains=gains, gu=None), _run(dev, d, m, gains=gains, gu=torch.zeros_like(d["gu"])))
    tail = dev.adjoint(d["gx"][:, 3:6].contiguous(), d["gu"][:, 3:5].contiguous(), A=d["A"][:, 3:5].contiguous(), B=d["B"][:, 3:5].contiguous(),
                       gains=d["gains"][:, 3:5].contiguous(), m=m)
    assert torch.equal(tail["mu"], full["mu"][:, 3:5]) and torch.equal(tail["lam"], full["lam"][:, 3:6])
    mine = {"lam": torch.full_like(full["lam"], 77.0), "mu": torch.full_like(full["mu"], 77.0)}
    res = _run(dev, d, m, out=mine)
    assert res["lam"].data_ptr() == mine["lam"].data_ptr() and _equal(res, full)
    for name in OUT:
        part = _run(dev, d, m, out={name: torch.full_like(full[name], 77.0)})
        assert set(part) == {name} and torch.equal(part[name], full[name])


@pytest.mark.parametrize("cls", AR.CLASSES)
def test_a_nan_stays_in_its_row(cls):
    """A NaN in gx of one row, at the final state and at step 1 (open and closed loop): that row's lam from there down and its mu are
    NaN, and every other row's bytes -- the other vectors of the same problem included -- are those of the clean run.  A NaN in
    A reaches every row of its problem and no other problem."""
    torch = _torch()
    dev = _handle(cls)
    n, m, T = N_PROBLEMS, 3, 5
    d, _ = _family(cls, T, m)
    others = [r for r in range(n * m) if r != 4]
    for closed in (False, True):
        good = _run(dev, d, m, gains=closed)
        for step in (T, 1):
            bad = dict(d, gx=d["gx"].clone())
            bad["gx"][4, step, 2] = float("nan")
            res = _run(dev, bad, m, gains=closed)
            assert _equal(res, good, rows=others), (closed, step)
            assert bool(torch.isnan(res["lam"][4, 0]).all()) and bool(torch.isnan(res["mu"][4, 0]).all())
            assert torch.equal(res["lam"][4, step + 1:], good["lam"][4, step + 1:]) and torch.equal(res["mu"][4, step:], good["mu"][4, step:])
        bad = dict(d, A=d["A"].clone())
        bad["A"][1, 2, 3, 4] = float("nan")
        res = _run(dev, bad, m, gains=closed)
        assert _equal(res, good, rows=[0, 1, 2, 6, 7, 8]) and bool(torch.isnan(res["lam"][3:6, 0]).any(dim=1).all())


# ------------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing_and_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd.lib import KAdjointDev, KAdjointIn, KManipError
    cls = AR.CLASSES[0]
    nx, nu = cls
    dev = _handle(cls)
    L = dev.L
    n, m, T = N_PROBLEMS, 3, 2
    d, _ = _family(cls, T, m)
    good = _run(dev, d, m)
    a_t, b_t, g_t = d["A"].transpose(2, 3).contiguous(), d["B"].transpose(2, 3).contiguous(), d["gains"].transpose(2, 3).contiguous()
    sent = dict(lam=torch.full((n * m, T + 1, nx), 77.0, dtype=torch.float64, device="cuda"), mu=torch.full((n * m, T, nu), 77.0, dtype=torch.float64, device="cuda"))
    fo = KAdjointDev()
    for name, v in sent.items():
        setattr(fo, name, v.data_ptr())
    ptr = dict(a_t=a_t.data_ptr(), b_t=b_t.data_ptr(), gx=d["gx"].data_ptr())

    def fin(**kw):
        i = KAdjointIn()
        i.gu, i.gain_t = d["gu"].data_ptr(), g_t.data_ptr()
        for name, v in dict(ptr, **kw).items():
            setattr(i, name, v)
        return i
    ok = fin()
    refused = [(None, ok, n, T, m, fo, b""), (dev.h, None, n, T, m, fo, b"kmanip_adjoint: the KAdjointIn pointer is NULL"),
               (dev.h, ok, n, T, m, None, b"kmanip_adjoint: the KAdjointDev pointer is NULL"), (dev.h, ok, -1, T, m, fo, b"kmanip_adjoint: n is negative"),
               (dev.h, ok, n, -1, m, fo, b"kmanip_adjoint: T is negative"), (dev.h, ok, n, T, -1, fo, b"kmanip_adjoint: m is negative"),
               (dev.h, fin(a_stride=nx * nx - 1), n, T, m, fo, b"a_stride is smaller"), (dev.h, fin(b_stride=1), n, T, m, fo, b"b_stride is smaller"),
               (dev.h, fin(a_stride=-8), n, T, m, fo, b"a_stride is smaller"), (dev.h, ok, 2 ** 16, 2 ** 15, 1, fo, b"more than an int counts"),
               (dev.h, ok, 2 ** 16, 1, 2 ** 16, fo, b"more than an int counts"), (dev.h, ok, 2 ** 11, 2 ** 11, 2 ** 11, fo, b"more than an int counts")]
    refused += [(dev.h, fin(**{name: None}), n, T, m, fo, ("KAdjointIn::%s is NULL" % name).encode()) for name in ptr]
    for h, i, nn, tt, mm, o, msg in refused:
        rc = L.kmanip_adjoint(h, None if i is None else C.byref(i), nn, tt, mm, None if o is None else C.byref(o), None)
        err = L.kmanip_last_error(h)
        assert rc != 0 and (err == msg if msg.startswith(b"kmanip_") else msg in err), (nn, tt, mm, msg, err)
    for nn, tt, mm in ((0, T, m), (n, 0, m), (n, T, 0)):          # no problems, no steps, no vectors: succeeds, launches nothing
        assert L.kmanip_adjoint(dev.h, C.byref(ok), nn, tt, mm, C.byref(fo), None) == 0
    assert L.kmanip_adjoint(dev.h, C.byref(ok), n, T, m, C.byref(KAdjointDev()), None) == 0          # nothing asked for
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in sent.values())
    # the wrapper's own checks
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    for kw in (dict(A=d["A"]), dict(A=d["A"], B=d["B"], deriv_t=z(n, T, nx + nu, nx)), dict(), dict(deriv_t=z(n, T, nx + nu, nx + 1)),
               dict(deriv_t=z(n, T, nx + nu - 1, nx)), dict(deriv_t=z(n, T, nx + nu, nx, dtype=torch.float32)), dict(A=d["A"], B=z(n, T, nx, nu, device="cpu")),
               dict(A=d["A"], B=d["B"], gu=z(n * m, T, nu + 1)), dict(A=d["A"], B=d["B"], gains=d["gains"], gains_t=g_t),
               dict(A=d["A"], B=d["B"], gains=z(n, T, nx, nu)), dict(A=d["A"], B=d["B"], gains_t=z(n, T, nu, nx)), dict(A=d["A"], B=d["B"], m=0),
               dict(A=d["A"], B=d["B"], m=2), dict(A=d["A"], B=d["B"], out={"lam": z(n * m, T, nx)})):
        with pytest.raises(KManipError):
            dev.adjoint(d["gx"], **dict(dict(m=m), **kw))
    with pytest.raises(ValueError):
        dev.adjoint(d["gx"], A=d["A"], B=d["B"], m=m, out={"nonsense": z(n)})
    empty = dev.adjoint(z(0, T + 1, nx), A=z(0, T, nx, nx), B=z(0, T, nx, nu), m=m)
    assert tuple(empty["lam"].shape) == (0, T + 1, nx) and tuple(empty["mu"].shape) == (0, T, nu)
    still = dev.adjoint(d["gx"][:, :1].contiguous(), A=z(n, 0, nx, nx), B=z(n, 0, nx, nu), m=m)          # T = 0: lam[T] = gx[T] is all there is
    assert torch.equal(still["lam"], d["gx"][:, :1]) and tuple(still["mu"].shape) == (n * m, 0, nu)
    # the handle works afterwards, through the same structs
    assert L.kmanip_adjoint(dev.h, C.byref(ok), n, T, m, C.byref(fo), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(sent["lam"], good["lam"]) and torch.equal(sent["mu"], good["mu"])
    dev.step_flat(z(2, dev.cm.act_dim, dtype=torch.float32))
    assert not dev.done.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------------------- 5. handle read-only
def test_the_handle_is_read_only():
    """Two handles made alike, three steps; one calls adjoint before each.  Its state tensors before and after are equal, and the next
    step_flat gives the bytes of the twin that never made the call."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    cls = AR.CLASSES[0]
    cm = R.model(ASSET_OF[cls])
    a, b = (env_hip.KManipEnvHip(cm, num_envs=2, seed=5) for _ in range(2))
    a.k_reset(); b.k_reset()
    d, _ = _family(cls, 2, 3)
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, 2, cm.act_dim)).astype(np.float32)
    for k in range(3):
        before = a.state_tensors()
        _run(a, d, 3)
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), k
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), k
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------------------------ 6. rollout_grad
def test_rollout_grad_on_the_device_is_the_centred_difference_of_the_cost():
    """KManipSoloArmQPos, 2 envs stepped 4 times from reset, horizon 4, ilqr_reach's cost: grad_ctrl . d of
    rollout_grad(device=True, fused=True) against the centred difference of the cost of env.rollout along d (default_rng(1),
    h = 1e-6), per env.  The bar is 10 x what rollout_grad(device=False, fused=False) shows against the same difference, and that
    reference path is itself below 1e-3.  Closed loop (gains of scale 0.1, none on the cube's rotation) both paths make the same
    feedback launch and agree to 1e-9 of the largest entry: the fused and the unfused linearisation run the same arithmetic per row
    (DESIGN.md section 31), and a quotient by 2e-6 of states rounded at 1e-16 carries 1e-10 an entry before the sweep's sums."""
    torch = _torch()
    from gym_kmanip_amd import env_hip, grad, ilqr
    env = env_hip.make("KManipSoloArmQPos", num_envs=2, seed=3)
    cm, n, T, h = env.cm, 2, 4, 1e-6
    env.k_reset()
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64, device="cuda").repeat(cm.nlink)[:cm.nlink]
    goal = st["qpos"].clone()
    goal[:, :cm.nlink] += 0.1 * sign
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64, device="cuda")
    wq[:cm.nlink] = 10.0
    wq[cm.nv:cm.nv + cm.nlink] = 0.01
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((n, cm.nv), dtype=torch.float64, device="cuda"), wq,
                              torch.full((cm.nu,), 1e-3, dtype=torch.float64, device="cuda"), 10.0 * wq)
    ctrl = st["ctrl"][:, None, :].repeat(1, T, 1)
    args = (env, None, st["qpos"], st["qvel"], st["warm"])

    def J(u):
        r = env.rollout(qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=u, fields=("qpos", "qvel", "status"))
        assert not r["status"].any()
        return cost.total(torch.cat([st["qpos"][:, None], r["qpos"]], dim=1), torch.cat([st["qvel"][:, None], r["qvel"]], dim=1), u)
    d = _t(np.random.default_rng(1).standard_normal((n, T, cm.nu)))
    fd = (J(ctrl + h * d) - J(ctrl - h * d)) / (2 * h)
    ref = grad.rollout_grad(*args, ctrl, cost)
    got = grad.rollout_grad(*args, ctrl, cost, fused=True, device=True)
    assert not got["status"].any() and not got["status_fd"].any() and torch.equal(got["cost"], J(ctrl)) and torch.equal(ref["cost"], got["cost"])
    err_ref = ((ref["grad_ctrl"] * d).sum(dim=(1, 2)) - fd).abs() / fd.abs()
    err_got = ((got["grad_ctrl"] * d).sum(dim=(1, 2)) - fd).abs() / fd.abs()
    print("\nrollout_grad against the centred difference %s: torch unfused %s, device fused %s" % (fd.tolist(), err_ref.tolist(), err_got.tolist()))
    assert bool((err_ref < 1e-3).all()), err_ref
    assert bool((err_got <= 10.0 * err_ref).all()), (err_got, err_ref)
    # closed loop
    K = _t(0.1 * np.random.default_rng(4).standard_normal((n, T, cm.nu, 2 * cm.nv)))
    K[:, :, :, cm.nlink + 3:cm.nlink + 6] = 0.0          # (no gain on the cube's rotation: nothing is approximated)
    pol = dict(gains=K, qpos_ref=ref["qpos"][:, :-1].contiguous(), qvel_ref=(ref["qvel"][:, :-1] + 0.01).contiguous())
    a = grad.rollout_grad(*args, ctrl, cost, **pol)
    b = grad.rollout_grad(*args, ctrl, cost, **pol, fused=True, device=True)
    assert not b["status"].any() and float((b["ctrl"] - ctrl).abs().max()) > 1e-5 and torch.equal(a["ctrl"], b["ctrl"])
    for name in ("grad_ctrl", "grad_x0", "grad_gains"):
        gap = float((a[name] - b[name]).abs().max() / a[name].abs().max())
        print("closed loop, %s: device fused against torch unfused %.3e" % (name, gap))
        assert gap <= 1e-9, (name, gap)
    env.k_close()
