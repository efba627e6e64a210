"""kmanip_tangent on the device (run with -m gpu on an MI355X): KManipEnvHip.tangent, derivatives.tangent_pass and its Gauss-Newton
terms in one launch, and sysid.identify / the adjoint's duality over it.

Handles of 2 envs, KManipSoloArm and KManipDualArm: one per size class; the problems are not envs.  Against test_tangent_cpu's
longdouble restatement the bars are its BAR (S, du_acted) and BAR_GN (H, g) as they stand.  Everything that compares the kernel with
itself is bit for bit.  What the device showed: DESIGN.md section 43."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import adjoint_reference as AR  # noqa: E402
import regime_states as R  # noqa: E402
from test_tangent_cpu import BAR, BAR_GN, N_PROBLEMS, gaps, reference, sweep  # noqa: E402

pytestmark = pytest.mark.gpu

ASSET_OF = {(32, 10): "solo_arm", (52, 20): "dual_arm"}
_DEV = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _t(x):
    return None if x is None else _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def _handle(cls):
    """The class's handle of 2 envs, made once and shared (tangent only reads it)."""
    if cls not in _DEV:
        from gym_kmanip_amd import env_hip
        _DEV[cls] = env_hip.KManipEnvHip(R.model(ASSET_OF[cls]), num_envs=2, seed=0)
        _DEV[cls].k_reset()
        assert (2 * _DEV[cls].cm.nv, _DEV[cls].cm.nu) == cls
    return _DEV[cls]


def _family(cls, T, m, closed=True, n=N_PROBLEMS):
    f, ref = reference(cls[0], cls[1], T, m, closed, n)
    return {k: _t(v) for k, v in f.items()}, f, ref


def _run(dev, d, fields=("S", "du_acted"), **kw):
    a = dict(A=d["A"], B=d["B"], src=d["src"], du=d["du"], s0=d["s0"], gains=d["K"], fields=fields)
    return dev.tangent(**dict(a, **kw))


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _equal(a, b, names=None):
    return all(_torch().equal(a[k], b[k]) for k in (names or a))


@pytest.mark.parametrize("cls", AR.CLASSES)
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("m", [1, 3, 19])
def test_the_device_meets_the_bar_against_the_longdouble_restatement(cls, T, m):
    """3 problems of m columns (19: two workgroups a problem), open and closed loop, every input given through dense A / B; then s0
    alone (src and dU NULL) through a deriv_t with NaN columns after ctrl's and gains_t.  S and du_acted within BAR."""
    torch = _torch()
    dev = _handle(cls)
    nx, nu = cls
    for closed in (False, True):
        d, f, ref = _family(cls, T, m, closed)
        g = gaps(_host(_run(dev, d)), ref, ("S", "du_acted"))
        wide = torch.cat([d["A"].transpose(2, 3), d["B"].transpose(2, 3), torch.full((N_PROBLEMS, T, 5, nx), float("nan"), dtype=torch.float64, device="cuda")], dim=2).contiguous()
        lone = dev.tangent(deriv_t=wide, s0=d["s0"], gains_t=d["K"].transpose(2, 3).contiguous() if closed else None, fields=("S", "du_acted"))
        gl = gaps(_host(lone), sweep(f["A"], f["B"], None, None, f["s0"], f["K"], None, None, np.longdouble), ("S",))
        print("\n%s T %d m %d %s: S %.2e du_acted %.2e; s0 alone through deriv_t: S %.2e (bar %.0e)" % (cls, T, m, "closed" if closed else "open", g["S"], g["du_acted"], gl["S"], BAR))
        assert g["S"] <= BAR and g["du_acted"] <= BAR and gl["S"] <= BAR
        assert closed or not bool(lone["du_acted"].any())


@pytest.mark.parametrize("cls", AR.CLASSES)
@pytest.mark.parametrize("m", [1, 3, 16])
def test_the_gauss_newton_terms_meet_their_bar_and_are_symmetric_bit_for_bit(cls, m):
    """T = 5, closed loop, n in {1, 3}, W NULL and a full symmetric positive-definite W: H and g within BAR_GN, H == H' bitwise, and
    the same bytes whether S is written or not."""
    torch = _torch()
    dev = _handle(cls)
    for n in (1, 3):
        d, f, _ = _family(cls, 5, m, True, n)
        for W in (None, "W"):
            ref = sweep(**dict(f, W=None if W is None else f["W"]), dtype=np.longdouble)
            kw = dict(resid=d["r"], weight=None if W is None else d["W"])
            res = _run(dev, d, fields=("H", "g"), **kw)
            g = gaps(_host(res), ref, ("H", "g"))
            print("\n%s m %d n %d W %s: H %.2e g %.2e (bar %.0e)" % (cls, m, n, W, g["H"], g["g"], BAR_GN))
            assert g["H"] <= BAR_GN and g["g"] <= BAR_GN
            assert torch.equal(res["H"], res["H"].transpose(1, 2))
            both = _run(dev, d, fields=("S", "H", "g"), **kw)
            assert _equal(res, both, ("H", "g")) and torch.equal(both["S"], _run(dev, d, fields=("S",))["S"])
            assert torch.equal(_run(dev, d, fields=("H",), weight=kw["weight"])["H"], res["H"])          # (H alone needs no resid)


@pytest.mark.parametrize("cls", AR.CLASSES)
def test_the_kernel_agrees_with_itself_bit_for_bit(cls):
    """T = 5, m = 3, closed loop, with H and g: column j is its m = 1 run; a problem alone is its rows among three, and the problems
    reversed give the rows reversed; zero gains give the open-loop values; NULL src / dU / s0 equal zeros of them."""
    torch = _torch()
    dev = _handle(cls)
    n, m, T = N_PROBLEMS, 3, 5
    d, _, _ = _family(cls, T, m)
    F = ("S", "du_acted", "H", "g")
    full = _run(dev, d, fields=F, resid=d["r"], weight=d["W"])
    cut = lambda e, j: dict(A=d["A"][e], B=d["B"][e], src=d["src"][e][..., j].contiguous(), du=d["du"][e][..., j].contiguous(),
                            s0=d["s0"][e][..., j].contiguous(), gains=d["K"][e], resid=d["r"][e], weight=d["W"], fields=F)
    for e in range(n):
        es = slice(e, e + 1)
        one = dev.tangent(**cut(es, slice(None)))
        assert all(torch.equal(one[k][0], full[k][e]) for k in F), e
        for j in range(m):
            col = dev.tangent(**cut(es, slice(j, j + 1)))
            assert torch.equal(col["S"][0, ..., 0], full["S"][e, ..., j]) and torch.equal(col["du_acted"][0, ..., 0], full["du_acted"][e, ..., j])
            assert torch.equal(col["H"][0, 0, 0], full["H"][e, j, j]) and torch.equal(col["g"][0, 0], full["g"][e, j])
    rev = dev.tangent(**{k: v.flip(0).contiguous() if k not in ("weight", "fields") else v for k, v in cut(slice(None), slice(None)).items()})
    assert all(torch.equal(rev[k].flip(0), full[k]) for k in F)
    z = torch.zeros_like
    open_loop = _run(dev, d, gains=None)
    assert not _equal(open_loop, _run(dev, d)) and _equal(_run(dev, d, gains=z(d["K"])), open_loop)
    for gains in (None, d["K"]):
        assert _equal(_run(dev, d, gains=gains, src=None, du=None, s0=None, m=m), _run(dev, d, gains=gains, src=z(d["src"]), du=z(d["du"]), s0=z(d["s0"])))
        assert _equal(_run(dev, d, gains=gains, du=None), _run(dev, d, gains=gains, du=z(d["du"])))


@pytest.mark.parametrize("cls", AR.CLASSES)
def test_a_nan_stays_in_its_column(cls):
    """A NaN in src of column 1 of problem 1 at step 1 (open and closed loop): that column of S from step 2 on, row and column 1 of
    that problem's H and its g[1] are NaN; every other value is the clean run's."""
    torch = _torch()
    dev = _handle(cls)
    d, _, _ = _family(cls, 5, 3)
    for gains in (None, d["K"]):
        kw = dict(fields=("S", "H", "g"), resid=d["r"], weight=d["W"], gains=gains)
        good = _run(dev, d, **kw)
        src = d["src"].clone()
        src[1, 1, 2, 1] = float("nan")
        bad = _run(dev, d, src=src, **kw)
        hit = {k: torch.zeros_like(good[k], dtype=torch.bool) for k in good}
        hit["S"][1, 2:, :, 1] = True
        hit["H"][1, 1, :] = hit["H"][1, :, 1] = hit["g"][1, 1] = True
        for k in good:
            assert torch.equal(bad[k][~hit[k]], good[k][~hit[k]]) and bool(torch.isnan(bad[k][hit[k]]).reshape(-1, 1).any(dim=1).any()), k
        assert bool(torch.isnan(bad["S"][1, 2:, :, 1]).any(dim=1).all()) and bool(torch.isnan(bad["H"][1, 1, :]).all()) and bool(torch.isnan(bad["g"][1, 1]))


def test_refusals_launch_nothing_and_the_handle_is_only_read():
    torch = _torch()
    from gym_kmanip_amd.lib import KManipError, KTangentDev, KTangentIn
    cls = AR.CLASSES[0]
    nx, nu = cls
    dev = _handle(cls)
    L = dev.L
    n, m, T = N_PROBLEMS, 3, 2
    d, _, _ = _family(cls, T, m)
    before = dev.state_tensors()
    good = _run(dev, d, fields=("S", "du_acted", "H", "g"), resid=d["r"])
    keep = dict(a_t=d["A"].transpose(2, 3).contiguous(), b_t=d["B"].transpose(2, 3).contiguous(), gain_t=d["K"].transpose(2, 3).contiguous(),
                src_t=d["src"].transpose(2, 3).contiguous(), du_t=d["du"].transpose(2, 3).contiguous(), s0_t=d["s0"].transpose(1, 2).contiguous(), r=d["r"])
    shapes = dict(s_t=(n, T + 1, m, nx), du_acted_t=(n, T, m, nu), h=(n, m, m), g=(n, m))
    sent = {k: torch.full(s, 77.0, dtype=torch.float64, device="cuda") for k, s in shapes.items()}

    def fo(*names):
        o = KTangentDev()
        for k in names or sent:
            setattr(o, k, sent[k].data_ptr())
        return o

    def fin(**kw):
        i = KTangentIn()
        for k, v in dict({k: v.data_ptr() for k, v in keep.items()}, **kw).items():
            setattr(i, k, v)
        return i
    ok, all_out = fin(), fo()
    refused = [(None, ok, n, T, m, all_out, b""), (dev.h, None, n, T, m, all_out, b"the KTangentIn pointer is NULL"), (dev.h, ok, n, T, m, None, b"the KTangentDev pointer is NULL"),
               (dev.h, ok, -1, T, m, all_out, b"n is negative"), (dev.h, ok, n, -1, m, all_out, b"T is negative"), (dev.h, ok, n, T, -1, all_out, b"m is negative"),
               (dev.h, fin(a_t=None), n, T, m, all_out, b"a_t is NULL"), (dev.h, fin(b_t=None), n, T, m, all_out, b"b_t is NULL"),
               (dev.h, fin(a_stride=nx * nx - 1), n, T, m, all_out, b"a_stride is smaller"), (dev.h, fin(b_stride=1), n, T, m, all_out, b"b_stride is smaller"),
               (dev.h, fin(src_stride=m * nx - 1), n, T, m, all_out, b"src_stride is smaller"), (dev.h, ok, 2 ** 11, 2 ** 11, 2 ** 11, fo("s_t"), b"more than an int counts"),
               (dev.h, ok, n, T, 17, fo("h"), b"m <= KM_TANGENT_MC"), (dev.h, ok, n, T, 17, fo("s_t", "g"), b"m <= KM_TANGENT_MC"), (dev.h, fin(r=None), n, T, m, fo("g"), b"KTangentIn::r is NULL")]
    for h, i, nn, tt, mm, o, msg in refused:
        rc = L.kmanip_tangent(h, None if i is None else C.byref(i), nn, tt, mm, None if o is None else C.byref(o), None)
        assert rc != 0 and msg in L.kmanip_last_error(h), (nn, tt, mm, msg, L.kmanip_last_error(h))
    for nn, tt, mm in ((0, T, m), (n, 0, m), (n, T, 0)):          # no problems, no steps, no columns: succeeds, launches nothing
        assert L.kmanip_tangent(dev.h, C.byref(ok), nn, tt, mm, C.byref(all_out), None) == 0
    assert L.kmanip_tangent(dev.h, C.byref(ok), n, T, m, C.byref(KTangentDev()), None) == 0          # nothing asked for
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in sent.values())
    with pytest.raises(KManipError):
        _run(dev, d, fields=("g",))          # (the wrapper refuses g without resid before the C entry does)
    # the handle works afterwards, through the same structs, and was never written
    assert L.kmanip_tangent(dev.h, C.byref(ok), n, T, m, C.byref(all_out), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(sent["s_t"].transpose(2, 3), good["S"]) and torch.equal(sent["h"], good["H"]) and torch.equal(sent["g"], good["g"])
    after = dev.state_tensors()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_duality_with_the_adjoint_on_real_jacobians_and_identify_on_the_device(capsys):
    """KManipSoloArmQPos, 2 envs, T = 3, trajectory_fd(fused=True): sum_t gx_t . s_t = lam_0 . s0 + sum_t mu_t . dU_t + sum_t lam_{t+1} .
    src_t between env.tangent and env.adjoint on deriv_t, open loop and under gains, the gap relative to the sum of the terms'
    absolute values within BAR.  Then the kp_scale case of test_param_fd_gpu.py through identify(device_sensitivity=True): parameters
    within BAR_GN relative and the loss history within BAR_GN times the first loss of the default path's."""
    torch = _torch()
    from gym_kmanip_amd import env_hip, ilqr
    from gym_kmanip_amd.examples import system_identification as ex
    env = env_hip.make("KManipSoloArmQPos", num_envs=2, seed=3)
    cm, n, T, m = env.cm, 2, 3, 3
    nx, nu = 2 * cm.nv, cm.nu
    env.k_reset()
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    fd = ilqr.trajectory_fd(env, None, st["qpos"], st["qvel"], st["warm"], st["ctrl"][:, None, :].repeat(1, T, 1), fused=True)
    assert not fd["status"].any() and not fd["status_fd"].any()
    rng = np.random.default_rng(4)
    K, gx = _t(0.1 * rng.standard_normal((n, T, nu, nx))), _t(rng.standard_normal((n, m, T + 1, nx)))
    src, du, s0 = (_t(0.1 * rng.standard_normal(s)) for s in ((n, T, nx, m), (n, T, nu, m), (n, nx, m)))
    for gains in (None, K):
        S = env.tangent(deriv_t=fd["deriv_t"], src=src, du=du, s0=s0, gains=gains)["S"]
        adj = env.adjoint(gx.flatten(0, 1), deriv_t=fd["deriv_t"], gains=gains, m=m)
        lam, mu = adj["lam"].reshape(n, m, T + 1, nx), adj["mu"].reshape(n, m, T, nu)
        lhs = torch.einsum("natj,ntja->na", gx, S)
        terms = [torch.einsum("naj,nja->na", lam[:, :, 0], s0), torch.einsum("nati,ntia->na", mu, du), torch.einsum("natj,ntja->na", lam[:, :, 1:], src)]
        gap = float(((lhs - sum(terms)).abs() / (lhs.abs() + sum(x.abs() for x in terms))).max())
        print("\nreal Jacobians, %s: duality gap %.2e (bar %.0e)" % ("closed" if gains is not None else "open", gap, BAR))
        assert gap <= BAR
    env.k_close()
    real = env_hip.make("KManipSoloArmQPos", num_envs=2, seed=3)
    real.k_reset()
    real.set_env_params(kp_scale=_t(np.array([1.2, 0.85])))
    res = []
    for device in (False, True):
        model = env_hip.make("KManipSoloArmQPos", num_envs=2, seed=3)
        model.k_reset()
        st = model.state_tensors()
        res.append(ex.identify_log(real, model, st, ex.sweep_controls(model.cm, st, 4), wrt=("kp_scale",), iters=5, fused=True, device_sensitivity=device))
        model.k_close()
    real.k_close()
    print(capsys.readouterr().out)
    a, b = res
    dp = float((b["params"]["kp_scale"] / a["params"]["kp_scale"] - 1.0).abs().max())
    dl = float((b["loss"] - a["loss"]).abs().max() / a["loss"][0].max())
    ds = float((b["singular_values"] / a["singular_values"] - 1.0).abs().max())
    print("identify, device sensitivity against the default path: params %.2e, loss %.2e of the first loss, singular values %.2e" % (dp, dl, ds))
    assert dp <= BAR_GN and dl <= BAR_GN and ds <= BAR_GN and float(b["error"]["kp_scale"].max()) <= 1e-6 and torch.equal(a["accepted"], b["accepted"])
