"""kmanip_adjoint and gym_kmanip_amd/grad.py on the CPU: the bar the references set for the device tests,
derivatives.adjoint_pass against the explicit product form, rollout_grad / diff_rollout / rollout_jacobian over the CPU stand-in
(tests/tools/adjoint_reference.py OracleAdjoint) against centred differences of the cost, the built library's two k_adjoint kernels
and the binding against the header."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import adjoint_reference as AR  # noqa: E402
import build_matrix as BM  # noqa: E402
import feedback_oracle as FO  # noqa: E402
from test_lqr_backward_cpu import _problem  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------------ the bar
# derivatives.adjoint_pass (torch float64) and adjoint_reference.adjoint in float64 against adjoint in longdouble on
# adjoint_reference.family (riccati_reference.family's A and B; gx, gu, gains from seed 23): both classes, T in {1, 2, 5, 12}, 3
# problems, m in {1, 3}, open and closed loop; per row the largest difference divided by the largest |lam|, |mu| of the row.
# Measured here and committed: the worst over everything,
SPREAD = {"lam": 2.1e-15, "mu": 1.2e-15}
# (torch's; the float64 restatement's: 1.9e-15, 1.2e-15.)  The bar of tests/test_adjoint_gpu.py is 1000 x the worst of them, one digit
# up -- tests/test_lqr_backward_cpu.py's rule: the device sums in another order and contracts to FMAs but computes the same sums.
BAR = 3e-12
T_SET, M_SET, N_PROBLEMS = (1, 2, 5, 12), (1, 3), 3
_REF = {}

# rollout_grad / diff_rollout against a centred difference of the cost (h = 1e-6, one direction from default_rng(1)) on the CPU
# oracle, cell 20 of the solo_arm regime cells (C1: the cube in flight, no contact), relative error |fd - g . d| / |fd|.  Measured
# here and committed (this run: 1.45e-6, 8.2e-8, 5.4e-9 -- the first three constants are the figures measured when the sweep was designed, with
# another draw of dK --, 1.01e-7, 3.3e-8); the tests' bar is 10 x each.
FD_H = 1e-6
FD_ERR = {"open ctrl": 1.4e-6, "closed ctrl": 8e-8, "closed K": 2.7e-7, "diff ctrl": 1.1e-7, "diff qpos0": 3.4e-8}


def reference(nx, nu, T, m, closed, n=N_PROBLEMS):
    """(the family's arrays, adjoint_reference.batch of them in longdouble): computed once per argument set, shared by the tests."""
    key = (nx, nu, T, m, closed, n)
    if key not in _REF:
        f = AR.family(nx, nu, T, n, m)
        if not closed:
            f = dict(f, gains=None)
        _REF[key] = (f, AR.batch(**f, m=m, dtype=np.longdouble))
    return _REF[key]


def gaps(got, ref):
    """{lam, mu: the worst over the rows of max |got - ref| / max |ref|}; got float64 arrays, ref longdouble."""
    out = {}
    for name in ("lam", "mu"):
        rows = len(ref[name])
        d = np.abs(np.asarray(got[name]).astype(np.longdouble) - ref[name]).reshape(rows, -1).max(axis=1)
        out[name] = float((d / np.abs(ref[name]).reshape(rows, -1).max(axis=1)).max())
    return out


def test_the_references_agree_far_inside_the_bar_they_set():
    """The spread is measured again and printed; torch's adjoint_pass and the float64 restatement both stay a hundred times inside
    the committed bar (ten times the committed spread: BLAS builds sum in different orders), and the bar is the committed
    spread's: 1000 x its worst, one digit up."""
    import torch
    from gym_kmanip_amd.derivatives import adjoint_pass
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs a longdouble wider than float64"
    worst = {"torch": dict.fromkeys(SPREAD, 0.0), "float64": dict.fromkeys(SPREAD, 0.0)}
    for nx, nu in AR.CLASSES:
        for T in T_SET:
            for m in M_SET:
                for closed in (False, True):
                    f, ref = reference(nx, nu, T, m, closed)
                    r64 = AR.batch(**f, m=m)
                    t = {name: None if v is None else torch.from_numpy(v) for name, v in f.items()}
                    lam, mu = adjoint_pass(t["A"], t["B"], t["gx"], t["gu"], t["gains"], m)
                    assert tuple(lam.shape) == (N_PROBLEMS * m, T + 1, nx) and tuple(mu.shape) == (N_PROBLEMS * m, T, nu)
                    for tag, got in (("torch", dict(lam=lam.numpy(), mu=mu.numpy())), ("float64", r64)):
                        for name, g in gaps(got, ref).items():
                            worst[tag][name] = max(worst[tag][name], g)
    print("\nspread against the longdouble restatement: %s" % worst)
    for tag in worst:
        for name in SPREAD:
            assert worst[tag][name] <= BAR / 100.0, (tag, name, worst[tag][name])
    top = max(SPREAD.values())
    assert BAR >= 1000.0 * top and BAR <= 2000.0 * top


def test_adjoint_pass_is_the_explicit_product_form():
    """T = 2, both classes, m = 3: open loop lam[0] = gx_0 + A_0' gx_1 + A_0' A_1' gx_2 and mu[t] = gu_t + B_t' lam[t+1]; closed loop
    the same with A_t + B_t K_t in place of A_t and gx_t + K_t' gu_t in place of gx_t (t < T).  gu = None is gu = 0, bit for bit;
    m vectors at once are the m single runs to the bar (BLAS sums by shape)."""
    import torch
    from gym_kmanip_amd.derivatives import adjoint_pass
    for nx, nu in AR.CLASSES:
        f, _ = reference(nx, nu, 2, 3, True)
        A, B, gx, gu, K = (torch.from_numpy(f[name]) for name in ("A", "B", "gx", "gu", "gains"))
        n, m = N_PROBLEMS, 3
        rel = lambda a, b: float(((a - b).abs().reshape(a.shape[0], -1).amax(dim=1) / b.abs().reshape(b.shape[0], -1).amax(dim=1)).max())
        for gains in (None, K):
            lam, mu = adjoint_pass(A, B, gx, gu, gains, m)
            for e in range(n):
                Ac = [A[e, t] if gains is None else A[e, t] + B[e, t] @ K[e, t] for t in range(2)]
                for j in range(m):
                    r = e * m + j
                    g = [gx[r, t] if gains is None else gx[r, t] + K[e, t].T @ gu[r, t] for t in range(2)] + [gx[r, 2]]
                    want = g[0] + Ac[0].T @ g[1] + Ac[0].T @ (Ac[1].T @ g[2])
                    assert rel(lam[r, 0][None], want[None]) <= BAR, (nx, e, j)
                    for t in range(2):
                        assert rel(mu[r, t][None], (gu[r, t] + B[e, t].T @ lam[r, t + 1])[None]) <= BAR
                    one = adjoint_pass(A[e:e + 1], B[e:e + 1], gx[r:r + 1], gu[r:r + 1], None if gains is None else K[e:e + 1], 1)
                    assert rel(one[0], lam[r:r + 1]) <= BAR and rel(one[1], mu[r:r + 1]) <= BAR
            a, b = adjoint_pass(A, B, gx, None, gains, m), adjoint_pass(A, B, gx, torch.zeros_like(gu), gains, m)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        adjoint_pass(A, B, gx[:-1], gu, None, 3)


# ------------------------------------------------------------------------------------------------------ over the CPU stand-in
_CASE = {}


def _case(T=4):
    """test_ilqr_cpu's problem: cell 20 of the solo_arm regime cells (C1, the cube in flight), one env, horizon T, a joint-space goal
    0.1 rad away; the fixed policy of feedback_oracle (s = 0.3) about the cell's state."""
    import torch
    if T not in _CASE:
        cm, cost, p = _problem(n=1, T=T)
        K, qr, vr = FO.fixed_policy(cm, p["qpos0"].numpy(), p["qvel0"].numpy(), nstep=T, s=0.3)
        pol = dict(gains=torch.from_numpy(K), qpos_ref=torch.from_numpy(qr), qvel_ref=torch.from_numpy(vr))
        _CASE[T] = (cm, cost, p, pol)
    return _CASE[T]


def _open_cost(env, cost, p, ctrl=None, qpos0=None):
    import torch
    ctrl = p["ctrl"] if ctrl is None else ctrl
    q0 = p["qpos0"] if qpos0 is None else qpos0
    r = env.rollout(envs=p["envs"], qpos=q0, qvel=p["qvel0"], warm=p["warm0"], ctrl=ctrl, fields=("qpos", "qvel", "status"))
    assert not r["status"].any()
    return r, cost.total(torch.cat([q0[:, None], r["qpos"]], dim=1), torch.cat([p["qvel0"][:, None], r["qvel"]], dim=1), ctrl)


def _closed_cost(env, cost, p, pol, ctrl=None, gains=None):
    import torch
    r = env.rollout_feedback(envs=p["envs"], qpos=p["qpos0"], qvel=p["qvel0"], warm=p["warm0"], ctrl=p["ctrl"] if ctrl is None else ctrl,
                             **dict(pol, gains=pol["gains"] if gains is None else gains), fields=("qpos", "qvel", "ctrl", "status"))
    assert not r["status"].any()
    return cost.total(torch.cat([p["qpos0"][:, None], r["qpos"]], dim=1), torch.cat([p["qvel0"][:, None], r["qvel"]], dim=1), r["ctrl"])


def _check(tag, fd, g):
    err = abs(fd - g) / abs(fd)
    print("%s: centred difference %.9e, adjoint %.9e, relative error %.2e (committed %.1e, bar 10 x)" % (tag, fd, g, err, FD_ERR[tag]))
    assert err <= 10.0 * FD_ERR[tag], (tag, err)


def test_rollout_grad_is_the_centred_difference_of_the_cost_open_loop():
    """Cell 20, T = 4: grad_ctrl . d against the centred difference of cost.total along d (default_rng(1), h = 1e-6); the call makes
    trajectory_fd's three rollout calls (its nominal trajectory, then transition_fd's two) and no feedback call; cost, ctrl and the
    trajectory are the plain rollout's; grad_x0 is lam[:, 0]."""
    import torch
    from gym_kmanip_amd import grad, ilqr
    cm, cost, p, _ = _case()
    env = AR.OracleAdjoint(cm, 2)
    g = grad.rollout_grad(env, cost=cost, **p)
    assert len(env.calls) == 3 and [c["nstep"] for c in env.calls] == [4, 1, 1] and env.fb_calls == [] and env.adjoint_calls == []
    base = AR.OracleAdjoint(cm, 2)
    ilqr.trajectory_fd(base, p["envs"], p["qpos0"], p["qvel0"], p["warm0"], p["ctrl"])
    assert len(base.calls) == len(env.calls)
    assert not g["status"].any() and not g["status_fd"].any() and "grad_gains" not in g
    assert tuple(g["grad_ctrl"].shape) == (1, 4, cm.nu) and tuple(g["grad_x0"].shape) == (1, 2 * cm.nv) and tuple(g["lam"].shape) == (1, 5, 2 * cm.nv)
    assert torch.equal(g["grad_x0"], g["lam"][:, 0]) and torch.equal(g["ctrl"], p["ctrl"])
    r, J = _open_cost(env, cost, p)
    assert torch.equal(g["cost"], J) and torch.equal(g["qpos"][:, 1:], r["qpos"])
    d = torch.from_numpy(np.random.default_rng(1).standard_normal(tuple(p["ctrl"].shape)))
    fd = float((_open_cost(env, cost, p, p["ctrl"] + FD_H * d)[1] - _open_cost(env, cost, p, p["ctrl"] - FD_H * d)[1]) / (2 * FD_H))
    print()
    _check("open ctrl", fd, float((g["grad_ctrl"] * d).sum()))


def test_rollout_grad_is_the_centred_difference_of_the_cost_closed_loop():
    """The same problem under feedback_oracle.fixed_policy(s = 0.3): ONE rollout_feedback call, then trajectory_fd's three rollout
    calls on the recorded controls, which replay the closed-loop trajectory bit for bit; grad_ctrl . d and grad_gains . dK against
    the centred differences of the closed-loop cost along d (ctrl) and dK (the gains), both from default_rng(1).  gains_t gives
    the same result as gains."""
    import torch
    from gym_kmanip_amd import grad
    cm, cost, p, pol = _case()
    env = AR.OracleAdjoint(cm, 2)
    g = grad.rollout_grad(env, cost=cost, **p, **pol)
    assert len(env.fb_calls) == 1 and len(env.calls) == 3 and env.fb_calls[0]["n"] == 1 and env.fb_calls[0]["nstep"] == 4
    assert not g["status"].any() and not g["status_fd"].any() and tuple(g["grad_gains"].shape) == (1, 4, cm.nu, 2 * cm.nv)
    fb = env.rollout_feedback(envs=p["envs"], qpos=p["qpos0"], qvel=p["qvel0"], warm=p["warm0"], ctrl=p["ctrl"], **pol)
    assert torch.equal(g["ctrl"], fb["ctrl"]) and torch.equal(g["qpos"][:, 1:], fb["qpos"]) and torch.equal(g["qvel"][:, 1:], fb["qvel"])
    assert float((g["ctrl"] - p["ctrl"]).abs().max()) > 1e-4          # (the policy acts)
    assert torch.equal(g["cost"], _closed_cost(env, cost, p, pol))
    g_t = grad.rollout_grad(env, cost=cost, **p, gains_t=pol["gains"].transpose(2, 3).contiguous(), qpos_ref=pol["qpos_ref"], qvel_ref=pol["qvel_ref"])
    assert all(torch.equal(g[name], g_t[name]) for name in ("cost", "grad_ctrl", "grad_x0", "grad_gains"))
    d = torch.from_numpy(np.random.default_rng(1).standard_normal(tuple(p["ctrl"].shape)))
    dK = torch.from_numpy(np.random.default_rng(1).standard_normal(tuple(pol["gains"].shape)))
    fd = float((_closed_cost(env, cost, p, pol, ctrl=p["ctrl"] + FD_H * d) - _closed_cost(env, cost, p, pol, ctrl=p["ctrl"] - FD_H * d)) / (2 * FD_H))
    print()
    _check("closed ctrl", fd, float((g["grad_ctrl"] * d).sum()))
    fd = float((_closed_cost(env, cost, p, pol, gains=pol["gains"] + FD_H * dK) - _closed_cost(env, cost, p, pol, gains=pol["gains"] - FD_H * dK)) / (2 * FD_H))
    _check("closed K", fd, float((g["grad_gains"] * dK).sum()))
    with pytest.raises(ValueError):
        grad.rollout_grad(env, cost=cost, **p, gains=pol["gains"])


def test_the_device_switch_routes_to_the_adjoint_entry():
    """rollout_grad(device=True) over the stand-in: one env.adjoint call with A and B (not fused: no deriv_t), gx = lx, gu = lu,
    m = 1, open loop without gains and closed loop with them; the gradients are device=False's to the bar."""
    import torch
    from gym_kmanip_amd import grad
    cm, cost, p, pol = _case(T=2)
    pol = {name: v[:, :2].contiguous() for name, v in pol.items()}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    for kw in ({}, pol):
        env = AR.OracleAdjoint(cm, 2)
        want = grad.rollout_grad(env, cost=cost, **p, **kw)
        assert env.adjoint_calls == []
        got = grad.rollout_grad(env, cost=cost, **p, **kw, device=True)
        assert len(env.adjoint_calls) == 1
        call = env.adjoint_calls[0]
        assert set(call["kwargs"]) == {"A", "B", "gains", "gains_t", "m"} and call["kwargs"]["m"] == 1 and call["kwargs"]["gains_t"] is None
        assert (call["kwargs"]["gains"] is None) == (not kw) and len(call["args"]) == 2
        lx, lu = cost.derivatives(got["qpos"], got["qvel"], got["ctrl"])[:2]
        assert torch.equal(call["args"][0], lx) and torch.equal(call["args"][1], lu)
        assert torch.equal(got["lam"], call["lam"]) and torch.equal(got["grad_ctrl"], call["mu"])
        for name in ("grad_ctrl", "grad_x0") + (("grad_gains",) if kw else ()):
            assert rel(got[name], want[name]) <= BAR, name


def _tangent_move(cm, qpos, d, h):
    """qpos [1, nq] moved by h d along the tangent vector d [nv]: joints and cube position += h d, the quaternion multiplied on the
    right by exp(h d_rot / 2)."""
    import torch
    nl = cm.nlink
    out = qpos.clone()
    out[0, :nl + 3] += h * d[:nl + 3]
    r = h * d[nl + 3:]
    ang = float(r.norm())
    w1 = np.cos(0.5 * ang)
    x1, y1, z1 = ((np.sin(0.5 * ang) / ang if ang > 0 else 0.5) * r).tolist()
    w0, x0, y0, z0 = qpos[0, nl + 3:].tolist()
    out[0, nl + 3:] = torch.tensor([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                                    w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1], dtype=qpos.dtype)
    return out


def test_diff_rollout_carries_backward_through_the_quaternion():
    """T = 2, a loss linear in every entry of qpos and qvel after every step (fixed coefficients from default_rng(2): the cube's
    quaternion entries included): loss.backward() through diff_rollout gives ctrl.grad, qvel0.grad and qpos0.grad; warm0 gets none.
    ctrl.grad . d and qpos0.grad, mapped to the tangent, . d_tan against centred differences of the loss (h = 1e-6), the qpos0
    direction taken in the tangent space: the joints more than 10 h inside their range, the cube's position and a rotation about the cube's
    own axes (the cell's two finger joints sit ON their upper limit, where the step has a kink and a centred difference is a secant
    across it: measured 2.0 against 20.3 one-sided at h = 1e-6).  The quaternion part of
    qpos0.grad is the minimal one: orthogonal to the quaternion.  rollout_jacobian's m = nx sweep equals nx sweeps of m = 1."""
    import torch
    from gym_kmanip_amd import grad, ilqr
    from gym_kmanip_amd.derivatives import adjoint_pass
    cm, _, p, _ = _case(T=2)
    nl = cm.nlink
    rng = np.random.default_rng(2)
    cq, cv = torch.from_numpy(rng.standard_normal((2, cm.nq))), torch.from_numpy(rng.standard_normal((2, cm.nv)))
    env = AR.OracleAdjoint(cm, 2)

    def loss_of(ctrl, qpos0):
        r = env.rollout(envs=p["envs"], qpos=qpos0, qvel=p["qvel0"], warm=p["warm0"], ctrl=ctrl, fields=("qpos", "qvel", "status"))
        assert not r["status"].any()
        return float((cq * r["qpos"]).sum() + (cv * r["qvel"]).sum())
    ctrl, q0, v0, w0 = (p[name].clone().requires_grad_(True) for name in ("ctrl", "qpos0", "qvel0", "warm0"))
    info = {}
    q, v = grad.diff_rollout(env, p["envs"], q0, v0, w0, ctrl, info=info)
    assert tuple(q.shape) == (1, 2, cm.nq) and tuple(v.shape) == (1, 2, cm.nv) and not info["status"].any() and not info["status_fd"].any()
    loss = (cq * q).sum() + (cv * v).sum()
    assert float(loss.detach()) == loss_of(p["ctrl"], p["qpos0"])
    loss.backward()
    assert w0.grad is None and tuple(ctrl.grad.shape) == tuple(ctrl.shape) and tuple(v0.grad.shape) == tuple(v0.shape)
    quat = p["qpos0"][0, nl + 3:]
    assert abs(float((q0.grad[0, nl + 3:] * quat).sum())) <= 1e-12 * float(q0.grad[0, nl + 3:].norm())
    d = torch.from_numpy(np.random.default_rng(1).standard_normal(tuple(ctrl.shape)))
    fd = (loss_of(p["ctrl"] + FD_H * d, p["qpos0"]) - loss_of(p["ctrl"] - FD_H * d, p["qpos0"])) / (2 * FD_H)
    print()
    _check("diff ctrl", fd, float((ctrl.grad * d).sum()))
    dt = torch.from_numpy(np.random.default_rng(1).standard_normal(cm.nv))
    rng_j = torch.tensor([[cm.desc.jnt_range[i][0], cm.desc.jnt_range[i][1]] for i in range(nl)], dtype=torch.float64)
    inside = (p["qpos0"][0, :nl] > rng_j[:, 0] + 10 * FD_H) & (p["qpos0"][0, :nl] < rng_j[:, 1] - 10 * FD_H)      # (the fingers: 1.1e-10 below)
    assert inside.tolist() == [True] * 8 + [False] * 2
    dt[:nl] = torch.where(inside, dt[:nl], torch.zeros_like(dt[:nl]))
    fd = (loss_of(p["ctrl"], _tangent_move(cm, p["qpos0"], dt, FD_H)) - loss_of(p["ctrl"], _tangent_move(cm, p["qpos0"], dt, -FD_H))) / (2 * FD_H)
    g_tan = grad.ambient_to_tangent(cm, p["qpos0"], q0.grad)
    assert float(g_tan[0, nl + 3:].abs().max()) > 1e-3                  # (the rotation part is there to be tested)
    _check("diff qpos0", fd, float((g_tan[0] * dt).sum()))
    # the tangent round trip, and the Jacobian's columns
    back = grad.ambient_to_tangent(cm, p["qpos0"], grad.tangent_to_ambient(cm, p["qpos0"], g_tan))
    assert float((back - g_tan).abs().max()) <= 1e-14 * float(g_tan.abs().max())
    jac = grad.rollout_jacobian(env, p["envs"], p["qpos0"], p["qvel0"], p["warm0"], p["ctrl"])
    nx = 2 * cm.nv
    assert tuple(jac["dxT_du"].shape) == (1, nx, 2, cm.nu) and tuple(jac["dxT_dx0"].shape) == (1, nx, nx)
    fdj = ilqr.trajectory_fd(env, p["envs"], p["qpos0"], p["qvel0"], p["warm0"], p["ctrl"])
    worst = 0.0
    for j in range(nx):
        gx = torch.zeros((1, 3, nx), dtype=torch.float64)
        gx[0, 2, j] = 1.0
        lam, mu = adjoint_pass(fdj["A"], fdj["B"], gx)
        worst = max(worst, float((mu[0] - jac["dxT_du"][0, j]).abs().max()), float((lam[0, 0] - jac["dxT_dx0"][0, j]).abs().max()))
    scale = float(jac["dxT_dx0"].abs().max())
    print("rollout_jacobian: m = nx against nx sweeps of m = 1, largest difference %.2e of %.2e" % (worst, scale))
    assert worst <= BAR * scale
    assert float((jac["dxT_dx0"][0] - fdj["A"][0, 1] @ fdj["A"][0, 0]).abs().max()) <= BAR * scale


# ------------------------------------------------------------------------------------------------------------------ the library
def test_the_library_holds_one_adjoint_kernel_per_class_without_scratch():
    """Parsed from the .so (no GPU): one k_adjoint per (nx, nu) class, no scratch, the LDS plan of kmanip_adjoint.hip within the 160 KB
    of a CU; the header declares the entry and its structs, the binding lists their fields in the header's order with the C
    compiler's layout, and the symbol is among the exports."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, "k_adjoint")
    assert sorted(r.args for r in rows) == sorted(AR.CLASSES)
    for r in rows:
        nx, nu = r.args
        assert r.scratch == 0 and r.lds <= 160 * 1024 and r.vgpr + r.agpr <= 512, r
        # two buffers of [nx + nu][nx | 1] and of [nx][nu | 1], the two lam buffers of nx vectors, and mu
        assert r.lds == 8 * (2 * (nx + nu) * (nx | 1) + 2 * nx * (nu | 1) + 2 * nx * nx + nx * nu), r
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for name, cls in (("KAdjointIn", klib.KAdjointIn), ("KAdjointDev", klib.KAdjointDev)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for t, star, names in re.findall(r"(\w+)\s*(\*?)\s*([\w, ]+);", body):
            fields += [(t, star, nm.strip()) for nm in names.split(",")]
        assert [f for _, _, f in fields] == [n for n, _ in cls._fields_], name
        assert [C.c_void_p if star else ctype[t] for t, star, _ in fields] == [t for _, t in cls._fields_], name
    assert (klib.KAdjointIn.a_stride.offset, klib.KAdjointIn.gx.offset, klib.KAdjointIn.gain_t.offset, C.sizeof(klib.KAdjointIn)) == (16, 32, 48, 56)
    assert C.sizeof(klib.KAdjointDev) == 16
    assert "KMANIP_API int kmanip_adjoint(KHandle h, const KAdjointIn* in, int n, int T, int m, const KAdjointDev* out, void* stream);" in hdr
    assert "kmanip_adjoint" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_adjoint.argtypes == [C.c_void_p, C.POINTER(klib.KAdjointIn), C.c_int, C.c_int, C.c_int, C.POINTER(klib.KAdjointDev), C.c_void_p]
    assert set(env_hip.KManipEnvHip._ADJOINT_FIELDS) == {n for n, _ in klib.KAdjointDev._fields_}


# ------------------------------------------------------------------------------------------------------------------ the example
@pytest.mark.parametrize("closed_loop", [False, True])
def test_the_example_descends_on_the_stand_in(closed_loop):
    """examples/gradient_reach.descend on the CPU stand-in with kinematics_at (site_cost_reference.OracleSite): cell 20, horizon 2,
    4 Adam steps of 0.003 rad on ctrl towards a site target: every cost is finite, every status 0, and each iterate is cheaper than the one
    before; closed loop the rollouts after the first go through rollout_feedback."""
    import torch
    import site_cost_reference as SC
    from gym_kmanip_amd.examples import gradient_reach
    cm, _, p, _ = _case(T=2)
    env = SC.OracleSite(cm, 2)
    st = dict(qpos=p["qpos0"], qvel=p["qvel0"], warm=p["warm0"], ctrl=p["ctrl"][:, 0].contiguous())
    out = gradient_reach.descend(env, st, horizon=2, iters=4, lr=0.003, closed_loop=closed_loop)
    J = out["cost"][:, 0].numpy()
    print("\ngradient_reach on the stand-in%s: cost per iteration %s" % (", closed loop" if closed_loop else "", J.tolist()))
    assert J.shape == (5,) and np.isfinite(J).all() and (np.diff(J) < 0).all() and int(out["status"].max()) == 0
    assert len(env.fb_calls) == (4 if closed_loop else 0) and tuple(out["ctrl"].shape) == (1, 2, cm.nu)
    assert torch.equal(st["ctrl"], p["ctrl"][:, 0])
