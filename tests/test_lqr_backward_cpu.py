"""kmanip_lqr_backward on the CPU: the bar the references set for the device tests, the built library's two
k_lqr_backward kernels and the binding against the header, and ilqr's device_backward / K_t switches over a stand-in
(tests/tools/riccati_reference.py OracleLqr) whose lqr_backward is the float64 restatement."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import build_matrix as BM  # noqa: E402
import riccati_reference as RR  # noqa: E402
import rollout_oracle as RO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------------ the bar
# ilqr.backward_pass (torch float64, LU) and riccati_reference.riccati in float64 (Cholesky) against riccati in longdouble on
# riccati_reference.family (seed 17): both classes, T in {1, 2, 5, 12}, 3 problems, reg in {0, 0.3}; per problem the largest
# difference divided by the largest |k|, |K|, |dV| of the problem.  Measured here and committed: the worst over everything,
SPREAD = {"k": 1.3e-15, "K": 1.9e-15, "dV": 4.7e-16}
# (torch's; the float64 restatement's: 1.1e-15, 1.6e-15, 3.9e-16.)  The bar of tests/test_lqr_backward_gpu.py is 1000 x the worst of
# them, one digit up -- section 27's margin: the device sums in another order and contracts to FMAs but solves the same problem.
BAR = 2e-12
T_SET, REGS, N_PROBLEMS = (1, 2, 5, 12), (0.0, 0.3), 3
_REF = {}


def reference(nx, nu, T, reg, n=N_PROBLEMS):
    """(the family's arrays, riccati_reference.batch of them in longdouble): computed once per argument set, shared by the tests."""
    key = (nx, nu, T, reg, n)
    if key not in _REF:
        f = RR.family(nx, nu, T, n)
        _REF[key] = (f, RR.batch(**f, reg=reg, dtype=np.longdouble))
    return _REF[key]


def gaps(got, ref):
    """{k, K, dV: the worst over the problems of max |got - ref| / max |ref|}; got float64 arrays, ref longdouble."""
    out = {}
    for name in ("k", "K", "dV"):
        n = len(ref[name])
        d = np.abs(np.asarray(got[name]).astype(np.longdouble) - ref[name]).reshape(n, -1).max(axis=1)
        out[name] = float((d / np.abs(ref[name]).reshape(n, -1).max(axis=1)).max())
    return out


def test_the_references_agree_far_inside_the_bar_they_set():
    """The spread is measured again and printed; torch's backward_pass and the float64 restatement both stay a hundred times inside
    the committed bar (ten times the committed spread: BLAS builds sum in different orders), no problem of the family fails, and
    the bar is the committed spread's: 1000 x its worst, one digit up."""
    import torch
    from gym_kmanip_amd import ilqr
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs a longdouble wider than float64"
    worst = {"torch": dict.fromkeys(SPREAD, 0.0), "float64": dict.fromkeys(SPREAD, 0.0)}
    for nx, nu in RR.CLASSES:
        for T in T_SET:
            for reg in REGS:
                f, ref = reference(nx, nu, T, reg)
                assert not ref["status"].any() and (ref["fail_step"] == -1).all()
                r64 = RR.batch(**f, reg=reg)
                assert not r64["status"].any()
                tk, tK, tdV = ilqr.backward_pass(*(torch.from_numpy(f[name]) for name in ("A", "B", "lx", "lu", "lxx", "luu")), reg=reg)
                for tag, got in (("torch", dict(k=tk.numpy(), K=tK.numpy(), dV=tdV.numpy())), ("float64", r64)):
                    for name, g in gaps(got, ref).items():
                        worst[tag][name] = max(worst[tag][name], g)
    print("\nspread against the longdouble restatement: %s" % worst)
    for tag in worst:
        for name in SPREAD:
            assert worst[tag][name] <= BAR / 100.0, (tag, name, worst[tag][name])
    top = max(SPREAD.values())
    assert BAR >= 1000.0 * top and BAR <= 2000.0 * top


# ------------------------------------------------------------------------------------------------------------------ the library
def _lqr_table():
    """The k_lqr_backward kernels of the built library; args = (NX, NU)."""
    from gym_kmanip_amd import lib as klib
    return BM.kernels(klib.LIB_PATH, "k_lqr_backward")


def test_the_library_holds_one_lqr_kernel_per_class_without_scratch():
    """Parsed from the .so (no GPU): one k_lqr_backward per (nx, nu) class, no scratch, LDS within the 160 KB of a CU, at most 512
    registers a lane (a 256-thread workgroup has one wave per SIMD); the header declares the entry and its structs, the binding
    lists their fields in the header's order with the C compiler's layout, and the symbol is among the exports."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    rows = _lqr_table()
    assert sorted(r.args for r in rows) == sorted(RR.CLASSES)
    for r in rows:
        nx, nu = r.args
        assert r.scratch == 0 and r.lds <= 160 * 1024 and r.vgpr + r.agpr <= 512, r
        # the plan of kmanip_lqr.hip: three [nx][nx | 1] matrices, two [nu][nx | 1], Y / K, Quu and its factor, the vectors, the flag
        lx, lu = nx | 1, nu | 1
        assert r.lds == 8 * (3 * nx * lx + 2 * nu * lx + max(nx * lu, nu * lx) + 2 * nu * lu + 2 * nx + 4 * nu) + 8, r
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for name, cls in (("KLqrIn", klib.KLqrIn), ("KLqrDev", klib.KLqrDev)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for t, star, names in re.findall(r"(\w+)\s*(\*?)\s*([\w, ]+);", body):
            fields += [(t, star, nm.strip()) for nm in names.split(",")]
        assert [f for _, _, f in fields] == [n for n, _ in cls._fields_], name
        assert [C.c_void_p if star else ctype[t] for t, star, _ in fields] == [t for _, t in cls._fields_], name
    assert (klib.KLqrIn.a_stride.offset, klib.KLqrIn.lx.offset, klib.KLqrIn.lxx_per_env.offset, klib.KLqrIn.reg.offset, C.sizeof(klib.KLqrIn)) == (16, 32, 64, 72, 80)
    assert C.sizeof(klib.KLqrDev) == 40
    assert "KMANIP_API int kmanip_lqr_backward(KHandle h, const KLqrIn* in, int n, int T, const KLqrDev* out, void* stream);" in hdr
    assert "kmanip_lqr_backward" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_lqr_backward.argtypes == [C.c_void_p, C.POINTER(klib.KLqrIn), C.c_int, C.c_int, C.POINTER(klib.KLqrDev), C.c_void_p]
    assert set(env_hip.KManipEnvHip._LQR_FIELDS) == {n for n, _ in klib.KLqrDev._fields_}


# ------------------------------------------------------------------------------------------------------ the restatement's own rules
def test_the_restatement_fails_a_problem_the_way_the_device_does():
    """luu = -I at step 2 of the middle problem: status 1, zeros, and fail_step 2 at T = 3, where step 2 is the first one solved (the
    smallest eigenvalue of Quu there is -0.5); at T = 5 the family's B' Vxx B outweighs the -I at step 2 (Quu stays positive
    definite, smallest eigenvalue 0.67) and the spoilt Vxx makes step 0 fail (-0.71): fail_step 0, with four steps already
    written.  A NaN in A at step 0: fail_step 0.  The neighbours are the unspoilt run's, bit for bit.  The stand-in reads deriv_t
    as the device does: the same result as A and B, bit for bit."""
    import torch
    nx, nu = RR.CLASSES[0]
    for T, step in ((3, 2), (5, 0)):
        f, _ = reference(nx, nu, T, 0.0)
        good = RR.batch(**f)
        bad = {name: v.copy() for name, v in f.items()}
        bad["luu"][1, 2] = -np.eye(nu)
        r = RR.batch(**bad)
        assert r["status"].tolist() == [0, 1, 0] and r["fail_step"].tolist() == [-1, step, -1]
        assert not r["k"][1].any() and not r["K"][1].any() and not r["dV"][1].any()
        assert all(np.array_equal(r[name][[0, 2]], good[name][[0, 2]]) for name in ("k", "K", "dV"))
    bad = {name: v.copy() for name, v in f.items()}
    bad["A"][1, 0, 3, 4] = np.nan
    r = RR.batch(**bad)
    assert r["status"].tolist() == [0, 1, 0] and r["fail_step"].tolist() == [-1, 0, -1] and not r["K"][1].any()
    t = {name: torch.from_numpy(v) for name, v in f.items()}
    deriv_t = torch.cat([t["A"].transpose(2, 3), t["B"].transpose(2, 3)], dim=2).contiguous()
    a = RR.lqr_backward(t["lx"], t["lu"], t["lxx"], t["luu"], A=t["A"], B=t["B"], reg=torch.full((3,), 0.3, dtype=torch.float64))
    b = RR.lqr_backward(t["lx"], t["lu"], t["lxx"], t["luu"], deriv_t=deriv_t, reg=0.3)
    assert set(a) == {"k", "gains_t", "K", "dV", "status", "fail_step"} and all(torch.equal(a[name], b[name]) for name in a)
    assert tuple(a["gains_t"].shape) == (3, 5, nx, nu) and a["gains_t"].is_contiguous() and a["K"].data_ptr() == a["gains_t"].data_ptr()


# ------------------------------------------------------------------------------------------------------ the loop over the stand-in
class _SpoiltCost:
    """A QuadraticCost whose derivatives hand env `env` luu = -I at step `step` (luu then comes per env)."""

    def __init__(self, cost, env, step):
        self.cost, self.env, self.step, self.total = cost, env, step, cost.total

    def derivatives(self, qpos, qvel, ctrl):
        import torch
        lx, lu, lxx, luu = self.cost.derivatives(qpos, qvel, ctrl)
        luu = luu[None].repeat(int(ctrl.shape[0]), 1, 1, 1)
        luu[self.env, self.step] = -torch.eye(luu.shape[-1], dtype=luu.dtype)
        return lx, lu, lxx, luu


def _problem(n=3, T=3):
    """ilqr_reach's problem on the contact-free SoloArm cell of tests/test_ilqr_cpu.py, n envs with a goal each."""
    import torch
    from gym_kmanip_amd import ilqr
    run = RO.cell_runs("solo_arm")
    cm, rows = run["cm"], run["rows"]
    e = 20
    q0, v0, w0, c0 = (torch.from_numpy(rows[name][e:e + 1].copy()).repeat(n, 1) for name in ("qpos", "qvel", "warm", "ctrl"))
    goal = q0.clone()
    goal[:, :cm.nlink] += torch.tensor([0.1, -0.06, 0.08], dtype=torch.float64)[:n, None]
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64)
    wq[:cm.nlink] = 10.0
    wq[cm.nv:cm.nv + cm.nlink] = 0.01
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((n, cm.nv), dtype=torch.float64), wq, torch.full((cm.nu,), 1e-3, dtype=torch.float64), 10.0 * wq)
    return cm, cost, dict(envs=[0, 1, 0][:n], qpos0=q0, qvel0=v0, warm0=w0, ctrl=c0[:, None].repeat(1, T, 1))


def test_ilqr_device_backward_over_the_stand_in():
    """ilqr(device_backward=True) on three envs, horizon 3, 2 iterations: the accepted cost never increases and is lower after the first
    iteration; lqr_backward was called once per iteration with A and B (not fused: no deriv_t) and the line search got its
    transposed gains; with every status 0 the last pass's k and K are ilqr.backward_pass's on the same inputs to the bar.  Then
    env 1 is handed luu = -I at step 1: status 1 in every iteration, never accepted, its controls kept, its reg multiplied; the
    other envs' results are those of the unspoilt run, bit for bit.  device_backward=False never calls lqr_backward."""
    import torch
    from gym_kmanip_amd import ilqr
    cm, cost, p = _problem()
    env = RR.OracleLqr(cm, 2)
    res = ilqr.ilqr(env, cost=cost, iters=2, alphas=(1.0, 0.5, 0.25), **p, device_backward=True)
    J = res["cost"].numpy()
    print("\niLQR over the stand-in, device_backward: cost per iteration %s" % J.tolist())
    assert J.shape == (3, 3) and np.isfinite(J).all() and (np.diff(J, axis=0) <= 0).all() and (J[1] < J[0]).all()
    assert len(env.lqr_calls) == 2 and not res["backward_status"].any() and tuple(res["backward_status"].shape) == (2, 3)
    assert all("deriv_t" not in c["kwargs"] and set(c["kwargs"]) == {"A", "B", "reg"} for c in env.lqr_calls)
    assert len(env.fb_calls) == 2
    for fb, call in zip(env.fb_calls, env.lqr_calls):
        assert np.array_equal(fb["gains"], call["K"].numpy())
    last = env.lqr_calls[-1]
    assert torch.equal(res["k"], last["k"]) and torch.equal(res["K"], last["K"])
    k, K, dV = ilqr.backward_pass(last["kwargs"]["A"], last["kwargs"]["B"], *last["args"], reg=last["kwargs"]["reg"])
    for name, got, want in (("k", res["k"], k), ("K", res["K"], K), ("dV", last["dV"], dV)):
        gap = float(((got - want).abs().reshape(3, -1).max(dim=1).values / want.abs().reshape(3, -1).max(dim=1).values).max())
        print("last pass, stand-in against backward_pass: %s %.3e" % (name, gap))
        assert gap <= BAR, (name, gap)
    # the spoilt env
    env2 = RR.OracleLqr(cm, 2)
    res2 = ilqr.ilqr(env2, cost=_SpoiltCost(cost, 1, 1), iters=2, alphas=(1.0, 0.5, 0.25), **p, device_backward=True)
    assert res2["backward_status"].tolist() == [[0, 1, 0]] * 2 and [c["fail_step"].tolist() for c in env2.lqr_calls] == [[-1, 1, -1]] * 2
    assert not res2["accepted"][:, 1].any() and torch.equal(res2["ctrl"][1], p["ctrl"][1]) and torch.equal(res2["cost"][:, 1], res2["cost"][0, 1].repeat(3))
    assert float(res2["reg"][1]) == 1e-6 * 10.0 * 10.0 and not res2["k"][1].any() and not res2["K"][1].any()
    keep = [0, 2]
    for name in ("ctrl", "reg", "k", "K"):
        assert torch.equal(res2[name][keep], res[name][keep]), name
    assert torch.equal(res2["cost"][:, keep], res["cost"][:, keep]) and torch.equal(res2["accepted"][:, keep], res["accepted"][:, keep])
    # the default: torch's pass, the stand-in's method untouched
    env3 = RR.OracleLqr(cm, 2)
    res3 = ilqr.ilqr(env3, cost=cost, iters=1, alphas=(1.0, 0.5, 0.25), **p)
    assert env3.lqr_calls == [] and "backward_status" not in res3


def test_forward_pass_takes_the_transposed_gains():
    """forward_pass(K_t=...) hands rollout_feedback gains_t in place of gains: the stand-in sees the same gains and returns the same
    rows, bit for bit."""
    import torch
    from gym_kmanip_amd import ilqr
    cm, cost, p = _problem(n=2, T=2)
    env = RR.OracleLqr(cm, 2)
    fd = ilqr.trajectory_fd(env, p["envs"], p["qpos0"], p["qvel0"], p["warm0"], p["ctrl"])
    assert "deriv_t" not in fd
    bp = env.lqr_backward(*cost.derivatives(fd["qpos"], fd["qvel"], p["ctrl"]), A=fd["A"], B=fd["B"], reg=1e-6)
    args = (env, p["envs"], p["qpos0"], p["qvel0"], p["warm0"], p["ctrl"], bp["k"])
    rest = (fd["qpos"][:, :-1], fd["qvel"][:, :-1], cost, (1.0, 0.5))
    a = ilqr.forward_pass(*args, bp["K"], *rest)
    b = ilqr.forward_pass(*args, None, *rest, K_t=bp["gains_t"])
    assert np.array_equal(env.fb_calls[0]["gains"], env.fb_calls[1]["gains"])
    assert torch.equal(a["cost"], b["cost"]) and torch.equal(a["ctrl"], b["ctrl"]) and torch.equal(a["best"], b["best"])
    assert all(torch.equal(a["rows"][name], b["rows"][name]) for name in a["rows"])
