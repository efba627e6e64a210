"""kmanip_tangent on the CPU: the bar the references set for the device tests, derivatives.tangent_pass against a
longdouble restatement, against sysid.param_sensitivity and in duality with adjoint_pass; the built library's two k_tangent kernels
and the binding against the header."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import adjoint_reference as AR  # noqa: E402
import build_matrix as BM  # noqa: E402
from tangent_reference import N_PROBLEMS, family, gaps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The NumPy float64 restatement against the longdouble one on the family below, both classes, T in {1, 2, 5}, m in {1, 3}, open and
# closed loop, 3 problems; per (problem, column) the largest difference divided by the largest entry (test_adjoint_cpu.py's rel), H and
# g per problem.  Measured here and committed: the worst over everything,
SPREAD = {"S": 6.9e-16, "du_acted": 4.9e-16, "H": 7.0e-16, "g": 1.3e-14}
# (torch's tangent_pass and gauss_newton_products: 8.4e-16, 9.8e-16, 7.9e-16, 1.8e-14.  g is a signed sum over (T + 1) nx products,
# taken relative to a problem's largest |g[a]|: at m = 1 that is the cancelled sum itself.)  The bars of tests/test_tangent_gpu.py:
# 1000 x the worst, one digit up (sections 37 / 41's rule) -- S and du_acted share BAR, the sums of products of S have BAR_GN.
BAR, BAR_GN = 7e-13, 2e-11
T_SET, M_SET = (1, 2, 5), (1, 3)
_REF = {}


def sweep(A, B, src, du, s0, K, r, W, dtype):
    """The recursion of include/kmanip.h KTangentIn and its Gauss-Newton terms over n problems in `dtype`, every product a NumPy matmul:
    A [n, T, nx, nx], B [n, T, nx, nu], src [n, T, nx, m], du [n, T, nu, m], s0 [n, nx, m], K [n, T, nu, nx] (None: zeros / open)."""
    c = lambda x: None if x is None else np.asarray(x, dtype=dtype)
    A, B, src, du, s0, K, r, W = (c(x) for x in (A, B, src, du, s0, K, r, W))
    n, T, nx, nu = B.shape
    m = next(x.shape[-1] for x in (src, du, s0) if x is not None)
    S, acted = np.zeros((n, T + 1, nx, m), dtype=dtype), np.zeros((n, T, nu, m), dtype=dtype)
    if s0 is not None:
        S[:, 0] = s0
    with np.errstate(all="ignore"):
        for t in range(T):
            u = (K[:, t] @ S[:, t] if K is not None else 0) + (du[:, t] if du is not None else 0)
            acted[:, t] = u
            S[:, t + 1] = A[:, t] @ S[:, t] + B[:, t] @ acted[:, t] + (src[:, t] if src is not None else 0)
        y = S if W is None else W @ S
        H = np.einsum("ntja,ntjb->nab", S, y)
        g = None if r is None else np.einsum("ntja,ntj->na", y, r)
    return dict(S=S, du_acted=acted, H=H, g=g)


def reference(nx, nu, T, m, closed, n=N_PROBLEMS):
    """(the family's arrays, their longdouble sweep): computed once per argument set, shared by the tests of both files."""
    key = (nx, nu, T, m, closed, n)
    if key not in _REF:
        f = family(nx, nu, T, m, closed, n)
        _REF[key] = (f, sweep(**f, dtype=np.longdouble))
    return _REF[key]


def test_tangent_pass_and_the_float64_restatement_stay_far_inside_the_bar_they_set():
    """The spread is measured again and printed; torch's tangent_pass (with gauss_newton_products) and the float64 restatement stay a
    hundred times inside the bars, and the bars are the committed spread's: 1000 x its worst, one digit up."""
    import torch
    from gym_kmanip_amd.derivatives import gauss_newton_products, tangent_pass
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs a longdouble wider than float64"
    worst = {"torch": dict.fromkeys(SPREAD, 0.0), "float64": dict.fromkeys(SPREAD, 0.0)}
    for nx, nu in AR.CLASSES:
        for T in T_SET:
            for m in M_SET:
                for closed in (False, True):
                    f, ref = reference(nx, nu, T, m, closed)
                    t = {k: None if v is None else torch.from_numpy(v) for k, v in f.items()}
                    S, acted = tangent_pass(t["A"], t["B"], t["src"], t["du"], t["s0"], t["K"])
                    H, g = gauss_newton_products(S, t["r"], t["W"])
                    assert tuple(S.shape) == (N_PROBLEMS, T + 1, nx, m) and tuple(acted.shape) == (N_PROBLEMS, T, nu, m)
                    for tag, got in (("torch", dict(S=S, du_acted=acted, H=H, g=g)), ("float64", sweep(**f, dtype=np.float64))):
                        for name, v in gaps(got, ref).items():
                            worst[tag][name] = max(worst[tag][name], v)
    print("\nspread against the longdouble restatement: %s" % worst)
    for tag in worst:
        for name in SPREAD:
            assert worst[tag][name] <= (BAR if name in ("S", "du_acted") else BAR_GN) / 100.0, (tag, name, worst[tag][name])
    for bar, top in ((BAR, max(SPREAD["S"], SPREAD["du_acted"])), (BAR_GN, max(SPREAD["H"], SPREAD["g"]))):
        assert 1000.0 * top <= bar <= 2000.0 * top


@pytest.mark.parametrize("cls", AR.CLASSES)
def test_tangent_pass_is_param_sensitivity_and_the_dual_of_adjoint_pass(cls):
    """T = 5, m = 3: with src = P and nothing else tangent_pass is sysid.param_sensitivity, open loop and under gains, to the bar.
    Duality on the same A, B, K with gx from adjoint_reference.family and no gu: sum_t gx_t . s_t = lam_0 . s0 + sum_t mu_t . dU_t +
    sum_t lam_{t+1} . src_t per (problem, column), the gap relative to the sum of the terms' absolute values."""
    import torch
    from gym_kmanip_amd.derivatives import adjoint_pass, tangent_pass
    from gym_kmanip_amd.sysid import param_sensitivity
    nx, nu = cls
    T, m, n = 5, 3, N_PROBLEMS
    adj = AR.family(nx, nu, T, n, m)
    gx = torch.from_numpy(adj["gx"]).reshape((n, m) + adj["gx"].shape[1:])
    for closed in (False, True):
        f, _ = reference(nx, nu, T, m, closed)
        t = {k: None if v is None else torch.from_numpy(v) for k, v in f.items()}
        S = tangent_pass(t["A"], t["B"], src=t["src"], gains=t["K"])[0]
        want = param_sensitivity(t["A"], t["src"], B=t["B"] if closed else None, gains=t["K"])
        assert gaps(dict(S=S), dict(S=want.numpy().astype(np.longdouble)), ("S",))["S"] <= BAR
        S, _ = tangent_pass(t["A"], t["B"], t["src"], t["du"], t["s0"], t["K"])
        lam, mu = (x.reshape((n, m) + tuple(x.shape[1:])) for x in adjoint_pass(t["A"], t["B"], gx.flatten(0, 1), None, t["K"], m))
        lhs = torch.einsum("natj,ntja->na", gx, S)
        terms = [torch.einsum("naj,nja->na", lam[:, :, 0], t["s0"]), torch.einsum("nati,ntia->na", mu, t["du"]),
                 torch.einsum("natj,ntja->na", lam[:, :, 1:], t["src"])]
        gap = float(((lhs - sum(terms)).abs() / (lhs.abs() + sum(x.abs() for x in terms))).max())
        print("\n%s %s: duality gap %.2e" % (cls, "closed" if closed else "open", gap))
        assert gap <= BAR


def test_the_library_holds_one_tangent_kernel_per_class_without_scratch():
    """Parsed from the .so (no GPU): one k_tangent per class, no scratch, kmanip_tangent.hip's LDS plan within a CU's 160 KB; the binding
    has the C compiler's layout of the header's structs, and the symbol is among the exports."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, "k_tangent")
    assert sorted(r.args for r in rows) == sorted(AR.CLASSES)
    mc = klib.KM_TANGENT_MC
    for r in rows:
        nx, nu = r.args
        assert r.scratch == 0 and r.lds <= 160 * 1024 and r.vgpr + r.agpr <= 512, r
        assert r.lds == 8 * (2 * (nx + nu) * nx + 2 * nx * nu + nx * nx + 5 * mc * (nx | 1) + 2 * mc * (nu | 1) + 3 * nx), r
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    assert "#define KM_TANGENT_MC %d " % mc in hdr
    assert (C.sizeof(klib.KTangentIn), C.sizeof(klib.KTangentDev), klib.KTangentIn.src_stride.offset) == (88, 32, 48)
    assert "KMANIP_API int kmanip_tangent(KHandle h, const KTangentIn* in, int n, int T, int m, const KTangentDev* out, void* stream);" in hdr
    assert "kmanip_tangent" in klib.EXPORTS
    assert klib.load().kmanip_tangent.argtypes == [C.c_void_p, C.POINTER(klib.KTangentIn), C.c_int, C.c_int, C.c_int, C.POINTER(klib.KTangentDev), C.c_void_p]
    assert {dev for dev, _, _ in env_hip.KManipEnvHip._TANGENT_FIELDS.values()} == {nm for nm, _ in klib.KTangentDev._fields_}
