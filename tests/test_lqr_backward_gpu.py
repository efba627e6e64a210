"""kmanip_lqr_backward on the device (run with -m gpu on an MI355X): KManipEnvHip.lqr_backward, ilqr.backward_pass in one launch.

Handles of 2 envs, KManipSoloArm and KManipDualArm: one per size class (nx, nu) = (32, 10), (52, 20); the problems are not envs, so
3 problems run on a handle of 2.  Against riccati_reference's longdouble restatement on its well-conditioned family the bar is
tests/test_lqr_backward_cpu.py's BAR as it stands; on real step Jacobians the bar is 1000 x the distance between torch's
backward_pass and its twin on A (1 + 1e-15), measured in the test.  Everything that compares the kernel with itself is bit for bit.
What the device showed: DESIGN.md section 37."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import regime_states as R  # noqa: E402
import riccati_reference as RR  # noqa: E402
from test_lqr_backward_cpu import BAR, N_PROBLEMS, gaps, reference  # noqa: E402

pytestmark = pytest.mark.gpu

ASSET_OF = {(32, 10): "solo_arm", (52, 20): "dual_arm"}
OUT = ("k", "gains_t", "dV", "status", "fail_step")
_DEV = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _t(x, dtype=None):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _handle(cls):
    """The class's handle of 2 envs, made once and shared (lqr_backward only reads it)."""
    if cls not in _DEV:
        from gym_kmanip_amd import env_hip
        dev = env_hip.KManipEnvHip(R.model(ASSET_OF[cls]), num_envs=2, seed=0)
        dev.k_reset()
        assert (2 * dev.cm.nv, dev.cm.nu) == cls
        _DEV[cls] = dev
    return _DEV[cls]


def _family(cls, T, reg=0.0):
    """(the family's arrays on the device, as NumPy, the longdouble reference) of test_lqr_backward_cpu.reference."""
    f, ref = reference(cls[0], cls[1], T, reg)
    return {name: _t(v) for name, v in f.items()}, f, ref


def _run(dev, d, **kw):
    return dev.lqr_backward(d["lx"], d["lu"], d["lxx"], d["luu"], A=d["A"], B=d["B"], **kw)


def _same(a, b, names=OUT, rows=None):
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    return [name for name in names if not _torch().equal(pick(a[name]), pick(b[name]))]


def _host(res):
    return dict(k=res["k"].cpu().numpy(), K=res["K"].cpu().numpy(), dV=res["dV"].cpu().numpy())


# ------------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("cls", RR.CLASSES)
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("reg", [0.0, 0.3])
def test_the_device_meets_the_bar_against_the_longdouble_restatement(cls, T, reg):
    """The family, 3 problems: k, K and dV within BAR of the longdouble restatement, relative to the problem's largest entry, with
    lxx / luu per problem and with problem 0's shared by all; every status 0 and fail_step -1; K is the transposed view of gains_t."""
    dev = _handle(cls)
    d, f, ref = _family(cls, T, reg)
    res = _run(dev, d, reg=reg)
    g = gaps(_host(res), ref)
    shared = dict(f, lxx=f["lxx"][0], luu=f["luu"][0])
    ref_s = RR.batch(**shared, reg=reg, dtype=np.longdouble)
    res_s = _run(dev, dict(d, lxx=d["lxx"][0].contiguous(), luu=d["luu"][0].contiguous()), reg=reg)
    g_s = gaps(_host(res_s), ref_s)
    print("\n%s T %d reg %.1f: gap to the longdouble restatement k %.2e K %.2e dV %.2e; shared lxx / luu k %.2e K %.2e dV %.2e (bar %.0e)"
          % (cls, T, reg, g["k"], g["K"], g["dV"], g_s["k"], g_s["K"], g_s["dV"], BAR))
    for r in (res, res_s):
        assert not r["status"].any() and bool((r["fail_step"] == -1).all())
        assert tuple(r["gains_t"].shape) == (N_PROBLEMS, T, cls[0], cls[1]) and r["gains_t"].is_contiguous()
        assert r["K"].data_ptr() == r["gains_t"].data_ptr() and tuple(r["K"].shape) == (N_PROBLEMS, T, cls[1], cls[0])
    assert not ref_s["status"].any()
    for name in ("k", "K", "dV"):
        assert g[name] <= BAR and g_s[name] <= BAR, (name, g[name], g_s[name])


# ----------------------------------------------------------------------------------------------------------- 2. real derivatives
def test_on_real_step_jacobians_the_device_is_as_close_to_torch_as_torch_is_to_itself():
    """KManipSoloArmQPos, 2 envs, horizon 3, trajectory_fd(fused=True) and ilqr_reach's cost: the device on deriv_t against
    ilqr.backward_pass on the A, B views of the same buffer.  The bar is the reference's own: backward_pass against its twin on
    A (1 + 1e-15), per quantity relative to its largest entry, times 1000."""
    torch = _torch()
    from gym_kmanip_amd import env_hip, ilqr
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
    assert tuple(fd["deriv_t"].shape) == (n, T, 2 * cm.nv + cm.nu, 2 * cm.nv) and fd["deriv_t"].data_ptr() == fd["A"].data_ptr()
    assert not fd["status"].any() and not fd["status_fd"].any()
    ls = cost.derivatives(fd["qpos"], fd["qvel"], ctrl)
    reg = 1e-6
    want = dict(zip(("k", "K", "dV"), ilqr.backward_pass(fd["A"], fd["B"], *ls, reg=reg)))
    twin = dict(zip(("k", "K", "dV"), ilqr.backward_pass(fd["A"] * (1.0 + 1e-15), fd["B"], *ls, reg=reg)))
    got = env.lqr_backward(*ls, deriv_t=fd["deriv_t"], reg=reg)
    assert not got["status"].any()
    rel = lambda a, b: float(((a - b).abs().reshape(n, -1).amax(dim=1) / b.abs().reshape(n, -1).amax(dim=1)).max())
    for name in ("k", "K", "dV"):
        spread, gap = rel(twin[name], want[name]), rel(got[name], want[name])
        print("\nreal Jacobians, %s: torch against its twin %.3e, the device against torch %.3e (bar %.3e); largest |%s| %.3e"
              % (name, spread, gap, 1000.0 * spread, name, float(want[name].abs().max())))
        assert gap <= 1000.0 * spread, (name, gap, spread)
    env.k_close()


# ------------------------------------------------------------------------------------------------------- 3. bit for bit against itself
@pytest.mark.parametrize("cls", RR.CLASSES)
def test_the_kernel_agrees_with_itself_bit_for_bit(cls):
    """T = 5, reg 0.3: each problem alone is its row of the batch; the problems reversed give the rows reversed; deriv_t read in
    place (strided blocks) equals A and B through their transposed dense copies; shared lxx / luu equal three private copies;
    reg left out equals a tensor of zeros, a number equals the tensor filled with it; k and K of steps 3 .. 4 equal those of the
    T = 2 problem made of these two steps and the final cost."""
    torch = _torch()
    dev = _handle(cls)
    d, _, _ = _family(cls, 5)
    full = _run(dev, d, reg=0.3)
    assert not full["status"].any()
    for e in range(N_PROBLEMS):
        one = _run(dev, {name: v[e:e + 1].contiguous() for name, v in d.items()}, reg=0.3)
        assert all(torch.equal(one[name][0], full[name][e]) for name in OUT), e
    rev = _run(dev, {name: v.flip(0).contiguous() for name, v in d.items()}, reg=torch.full((N_PROBLEMS,), 0.3, dtype=torch.float64, device="cuda"))
    assert all(torch.equal(rev[name].flip(0), full[name]) for name in OUT)
    deriv_t = torch.cat([d["A"].transpose(2, 3), d["B"].transpose(2, 3)], dim=2).contiguous()
    assert _same(dev.lqr_backward(d["lx"], d["lu"], d["lxx"], d["luu"], deriv_t=deriv_t, reg=0.3), full) == []
    sh = dict(d, lxx=d["lxx"][1].contiguous(), luu=d["luu"][1].contiguous())
    private = dict(d, lxx=d["lxx"][1][None].repeat(N_PROBLEMS, 1, 1, 1), luu=d["luu"][1][None].repeat(N_PROBLEMS, 1, 1, 1))
    assert _same(_run(dev, sh, reg=0.3), _run(dev, private, reg=0.3)) == []
    assert _same(_run(dev, d), _run(dev, d, reg=torch.zeros(N_PROBLEMS, dtype=torch.float64, device="cuda"))) == []
    tail = dict(A=d["A"][:, 3:5], B=d["B"][:, 3:5], lx=d["lx"][:, 3:6], lu=d["lu"][:, 3:5], lxx=d["lxx"][:, 3:6], luu=d["luu"][:, 3:5])
    two = _run(dev, {name: v.contiguous() for name, v in tail.items()}, reg=0.3)
    assert torch.equal(two["k"], full["k"][:, 3:5]) and torch.equal(two["gains_t"], full["gains_t"][:, 3:5]) and not two["status"].any()
    # outputs the caller hands in are the ones filled
    mine = {"k": torch.full_like(full["k"], 77.0), "status": torch.full((N_PROBLEMS,), 77, dtype=torch.uint8, device="cuda")}
    res = _run(dev, d, reg=0.3, out=mine)
    assert res["k"].data_ptr() == mine["k"].data_ptr() and _same(res, full) == []


# ------------------------------------------------------------------------------------------------------------------------ 4. status
@pytest.mark.parametrize("cls", RR.CLASSES)
def test_a_failed_problem_is_zeros_and_its_neighbours_are_untouched(cls):
    """luu = -I at step 2 of the middle problem.  T = 3: step 2 is the first solved and Quu there is indefinite -- status 1, fail_step
    2.  T = 5: the family's B' Vxx B outweighs the -I at step 2 and the spoilt Vxx fails step 0 (tests/test_lqr_backward_cpu.py:
    the restatement's figures) -- status 1, fail_step 0, with four steps already written.  A NaN in a_t at step 0 (it reaches Qux,
    not Quu): fail_step 0.  An inf in b_t at step 1: fail_step 1.  Each time ALL of the problem's k, gains_t and dV are zeros over
    a sentinel fill, and the neighbours' bytes are those of the run without the bad problem."""
    torch = _torch()
    dev = _handle(cls)
    nu = cls[1]
    cases = []
    for T, step in ((3, 2), (5, 0)):
        d, f, _ = _family(cls, T)
        bad = dict(d, luu=d["luu"].clone())
        bad["luu"][1, 2] = -torch.eye(nu, dtype=torch.float64, device="cuda")
        want = dict(f, luu=f["luu"].copy())
        want["luu"][1, 2] = -np.eye(nu)
        assert RR.batch(**want, dtype=np.longdouble)["fail_step"].tolist() == [-1, step, -1]
        cases.append((d, bad, step))
    d, _, _ = _family(cls, 5)
    nan = dict(d, A=d["A"].clone())
    nan["A"][1, 0, 3, 4] = float("nan")
    inf = dict(d, B=d["B"].clone())
    inf["B"][1, 1, 5, 2] = float("inf")
    cases += [(d, nan, 0), (d, inf, 1)]
    for d, bad, step in cases:
        good = _run(dev, d)
        n, T = int(d["lu"].shape[0]), int(d["lu"].shape[1])
        fill = {"k": torch.full((n, T, nu), 77.0, dtype=torch.float64, device="cuda"),
                "gain_t": torch.full((n, T, cls[0], nu), 77.0, dtype=torch.float64, device="cuda"),
                "dv": torch.full((n, 2), 77.0, dtype=torch.float64, device="cuda"),
                "status": torch.full((n,), 77, dtype=torch.uint8, device="cuda"), "fail_step": torch.full((n,), 77, dtype=torch.int32, device="cuda")}
        res = _run(dev, bad, out=fill)
        assert res["status"].tolist() == [0, 1, 0] and res["fail_step"].tolist() == [-1, step, -1], (T, step)
        assert not res["k"][1].any() and not res["gains_t"][1].any() and not res["dV"][1].any()
        assert _same(res, good, rows=[0, 2]) == []
        # through deriv_t as well: the strided read
        deriv_t = torch.cat([bad["A"].transpose(2, 3), bad["B"].transpose(2, 3)], dim=2).contiguous()
        assert _same(dev.lqr_backward(bad["lx"], bad["lu"], bad["lxx"], bad["luu"], deriv_t=deriv_t), res) == []


def test_refusals_launch_nothing_and_leave_the_handle_usable():
    torch = _torch()
    from gym_kmanip_amd.lib import KLqrDev, KLqrIn, KManipError
    cls = RR.CLASSES[0]
    nx, nu = cls
    dev = _handle(cls)
    L = dev.L
    d, _, _ = _family(cls, 2)
    good = _run(dev, d)
    n, T = N_PROBLEMS, 2
    a_t, b_t = d["A"].transpose(2, 3).contiguous(), d["B"].transpose(2, 3).contiguous()
    sent = dict(k=torch.full((n, T, nu), 77.0, dtype=torch.float64, device="cuda"), gain_t=torch.full((n, T, nx, nu), 77.0, dtype=torch.float64, device="cuda"),
                dv=torch.full((n, 2), 77.0, dtype=torch.float64, device="cuda"), status=torch.full((n,), 77, dtype=torch.uint8, device="cuda"),
                fail_step=torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    fo = KLqrDev()
    for name, v in sent.items():
        setattr(fo, name, v.data_ptr())
    ptr = dict(a_t=a_t.data_ptr(), b_t=b_t.data_ptr(), lx=d["lx"].data_ptr(), lu=d["lu"].data_ptr(), lxx=d["lxx"].data_ptr(), luu=d["luu"].data_ptr())

    def fin(**kw):
        i = KLqrIn()
        i.lxx_per_env = i.luu_per_env = 1
        for name, v in dict(ptr, **kw).items():
            setattr(i, name, v)
        return i
    ok = fin()
    refused = [(None, ok, n, T, fo, b""), (dev.h, None, n, T, fo, b"kmanip_lqr_backward: the KLqrIn pointer is NULL"),
               (dev.h, ok, n, T, None, b"kmanip_lqr_backward: the KLqrDev pointer is NULL"), (dev.h, ok, -1, T, fo, b"kmanip_lqr_backward: n is negative"),
               (dev.h, ok, n, -1, fo, b"kmanip_lqr_backward: T is negative"),
               (dev.h, fin(a_stride=nx * nx - 1), n, T, fo, b"a_stride is smaller"), (dev.h, fin(b_stride=1), n, T, fo, b"b_stride is smaller"),
               (dev.h, fin(a_stride=-8), n, T, fo, b"a_stride is smaller"), (dev.h, ok, 2 ** 16, 2 ** 15, fo, b"more than an int counts")]
    refused += [(dev.h, fin(**{name: None}), n, T, fo, ("KLqrIn::%s is NULL" % name).encode()) for name in ptr]
    for h, i, nn, tt, o, msg in refused:
        rc = L.kmanip_lqr_backward(h, None if i is None else C.byref(i), nn, tt, None if o is None else C.byref(o), None)
        err = L.kmanip_last_error(h)
        assert rc != 0 and (err == msg if msg.startswith(b"kmanip_") else msg in err), (nn, tt, msg, err)
    assert L.kmanip_lqr_backward(dev.h, C.byref(ok), 0, T, C.byref(fo), None) == 0          # no problems, no steps: succeeds, launches nothing
    assert L.kmanip_lqr_backward(dev.h, C.byref(ok), n, 0, C.byref(fo), None) == 0
    assert L.kmanip_lqr_backward(dev.h, C.byref(ok), n, T, C.byref(KLqrDev()), None) == 0  # nothing asked for
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in sent.values())
    # the wrapper's own checks
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    for kw in (dict(A=d["A"]), dict(A=d["A"], B=d["B"], deriv_t=z(n, T, nx + nu, nx)), dict(), dict(deriv_t=z(n, T, nx + nu, nx + 1)),
               dict(deriv_t=z(n, T, nx + nu, nx, dtype=torch.float32)), dict(A=d["A"], B=z(n, T, nx, nu, device="cpu")), dict(A=d["A"], B=d["B"], reg=z(n + 1)),
               dict(A=d["A"], B=d["B"], out={"k": z(n, T, nu + 1)})):
        with pytest.raises(KManipError):
            dev.lqr_backward(d["lx"], d["lu"], d["lxx"], d["luu"], **kw)
    with pytest.raises(KManipError):
        dev.lqr_backward(d["lx"], d["lu"], d["lxx"][:, :-1].contiguous(), d["luu"], A=d["A"], B=d["B"])
    with pytest.raises(ValueError):
        dev.lqr_backward(d["lx"], d["lu"], d["lxx"], d["luu"], A=d["A"], B=d["B"], out={"nonsense": z(n)})
    empty = dev.lqr_backward(z(0, T + 1, nx), z(0, T, nu), d["lxx"][0].contiguous(), d["luu"][0].contiguous(), A=z(0, T, nx, nx), B=z(0, T, nx, nu))
    assert tuple(empty["k"].shape) == (0, T, nu) and tuple(empty["K"].shape) == (0, T, nu, nx)
    # the handle works afterwards, through the same structs
    assert L.kmanip_lqr_backward(dev.h, C.byref(ok), n, T, C.byref(fo), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(sent["k"], good["k"]) and torch.equal(sent["gain_t"], good["gains_t"]) and torch.equal(sent["dv"], good["dV"])
    assert not sent["status"].any() and bool((sent["fail_step"] == -1).all())
    dev.step_flat(z(2, dev.cm.act_dim, dtype=torch.float32))
    assert not dev.done.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------------------- 5. handle read-only
@pytest.mark.parametrize("cls", RR.CLASSES)
def test_the_handle_is_read_only(cls):
    """Two handles made alike, three steps; one calls lqr_backward before each (a good batch and one with a failing problem).  Its
    state tensors before and after are equal, and the next step_flat gives the bytes of the twin that never made the call."""
    torch = _torch()
    from gym_kmanip_amd import env_hip
    cm = R.model(ASSET_OF[cls])
    a, b = (env_hip.KManipEnvHip(cm, num_envs=2, seed=5) for _ in range(2))
    a.k_reset(); b.k_reset()
    d, _, _ = _family(cls, 2)
    bad = dict(d, luu=-100.0 * d["luu"])             # (far below what B' Vxx B adds: every problem fails at its first step)
    acts = np.random.default_rng(6).uniform(-0.2, 0.2, (3, 2, cm.act_dim)).astype(np.float32)
    for k in range(3):
        before = a.state_tensors()
        assert not _run(a, d, reg=0.3)["status"].any() and bool(_run(a, bad)["status"].all())
        after = a.state_tensors()
        assert all(torch.equal(before[key], after[key]) for key in before), k
        act = torch.from_numpy(acts[k]).cuda()
        a.step_flat(act); b.step_flat(act)
        sa, sb = a.state_tensors(), b.state_tensors()
        assert all(torch.equal(sa[key], sb[key]) for key in sa), k
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
    a.k_close(); b.k_close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. iLQR
def test_ilqr_device_backward_on_the_device_and_the_example(capsys):
    """KManipSoloArmQPos, 4 envs, horizon 4, 2 iterations, 3 alphas, --fused --device-backward: the assertions of the fused test, and
    no backward pass failed."""
    import math
    from gym_kmanip_amd.examples import ilqr_reach
    out = ilqr_reach.main(["--num-envs", "4", "--horizon", "4", "--iters", "2", "--alphas", "1.0", "0.5", "0.25", "--fused", "--device-backward"])
    print(capsys.readouterr().out)
    cost = np.asarray(out["cost_per_env"])
    assert out["fused"] is True and out["device_backward"] is True and cost.shape == (3, 4) and np.isfinite(cost).all()
    assert (np.diff(cost, axis=0) <= 0).all() and (cost[1] < cost[0]).all()
    assert out["rows_per_line_search"] == 12 and out["feedback_launches"] == 2 and all(math.isfinite(c) for c in out["cost"])
    assert out["backward_failures"] == 0
