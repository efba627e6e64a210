"""kmanip_param_fd and gym_kmanip_amd.sysid on the CPU: the reference's own spread and the bars the device test
takes from it, the status rules on the stand-in, the parameter gradient against a centred difference of the loss, the sensitivity
recursion against the adjoint form, identify on a grasp (all four parameters) and on a cube in flight (an unobservable direction),
the example's loop, and the build: the eight k_paramfd objects and the binding against the header."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import build_matrix as BM  # noqa: E402
import paramfd_oracle as PO  # noqa: E402
import rollout_oracle as RO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = ("solo_arm", "dual_arm")

# ------------------------------------------------------------------------------------------------- the bars of the device's derivatives
# paramfd_oracle.reference on rollout_oracle.FD_CELLS (the check values of the parameters, relative eps 1e-4, warm_offset 1, the default
# solver tolerance): the worst spread of each column kind under qvel (1 + 1e-15) over the two assets (rollout_oracle.fd_dist: per cell,
# normalised by max(1, max|block|)), measured here and committed; the bar of tests/test_param_fd_gpu.py is 1000 x that, one digit up --
# tests/test_rollout_cpu.py's rule and its margin.  Keys: nsub (None = the model's 10 sub-steps).
SPREAD_P = {1: {"P_qpos": 3.470e-11, "P_qvel": 2.401e-09}, None: {"P_qpos": 1.319e-10, "P_qvel": 1.201e-09}}
BAR_P = {1: {"P_qpos": 4e-8, "P_qvel": 3e-6}, None: {"P_qpos": 2e-7, "P_qvel": 2e-6}}


@pytest.mark.parametrize("nsub", [1, None], ids=["mj_step", "control_step"])
def test_the_parameter_derivative_bars_are_1000_times_the_references_own_spread(nsub):
    from test_forces_cpu import _round_up_one_digit
    worst = {k: 0.0 for k in PO.KINDS}
    for asset in ASSETS:
        cm, rows, p, d = PO.reference(asset, nsub)
        t = PO.reference(asset, nsub, twin=True)[3]
        assert len(rows["qpos"]) == 6 and cm.desc.solver_tolerance == 1e-8 and d["deriv_t"].shape == (6, 4, 2 * cm.nv)
        assert not d["status_cols"].any() and not t["status_cols"].any()
        assert np.array_equal(d["contact_mask_fd"], t["contact_mask_fd"])
        size = np.abs(d["deriv_t"]).reshape(6, -1).max(axis=1)
        assert (size > 0.01).all() and (size < 100.0).all(), size                   # every cell has a derivative worth comparing
        for k, v in RO.fd_dist(PO.blocks(d["deriv_t"], cm.nv), PO.blocks(t["deriv_t"], cm.nv)).items():
            worst[k] = max(worst[k], float(v.max()))
    print("\nnsub %s: spread of the reference's P under qvel (1 + 1e-15): %s" % (nsub, "  ".join("%s %.3e" % kv for kv in worst.items())))
    for k in PO.KINDS:
        assert 1000.0 * worst[k] <= BAR_P[nsub][k], (k, worst[k])
        assert BAR_P[nsub][k] == pytest.approx(_round_up_one_digit(1000.0 * SPREAD_P[nsub][k]), rel=1e-12), k


# ----------------------------------------------------------------------------------------------------------- statuses on the stand-in
def test_the_stand_in_refuses_values_outside_the_domain_with_status_3():
    """A friction loss of 0 (relative: e = 0; absolute: minus < 0), a perturbed mass below 0, a NaN parameter: status 3, zero columns, no
    step; a bad index: status 2 on every column; a NaN state: status 1; the other rows and columns are derivatives."""
    import torch
    cm, rows, p, ref = PO.reference("solo_arm", 1)
    env = PO.OracleParamFd(cm, 2)
    t = {k: torch.from_numpy(v[:4].copy()) for k, v in rows.items()}
    par = torch.from_numpy(p[:4].copy())
    par[1, 2] = 0.0                                      # row 1: friction loss 0
    par[3, 1] = float("nan")                             # row 3: a NaN friction -- every column of the row
    t["envs"][2] = 7                                     # row 2: a bad index
    d = env.param_fd(params=par, nsub=1, **t)
    st = d["status_cols"].numpy()
    assert st.tolist() == [[0, 0, 0, 0], [0, 0, 3, 0], [2, 2, 2, 2], [3, 3, 3, 3]]
    assert d["status_fd"].tolist() == [0, 3, 2, 3] and d["wrt"] == ("cube_mass", "cube_friction", "cube_frictionloss", "kp_scale")
    assert tuple(d["P"].shape) == (4, 2 * cm.nv, 4) and tuple(d["contact_mask_fd"].shape) == (4, 2, 4)
    D = d["deriv_t"].numpy()
    assert not D[st != 0].any() and not d["contact_mask_fd"].permute(2, 0, 1).numpy()[st != 0].any()
    assert np.array_equal(D[0], ref["deriv_t"][0]) and np.abs(D[1][[0, 1, 3]]).max() > 0
    # absolute steps: a mass step larger than the mass, a friction-loss step at 0
    a = env.param_fd(params=par[:2], nsub=1, eps={"cube_mass": 1.0, "cube_frictionloss": 1e-3}, relative=False, wrt=("cube_frictionloss", "cube_mass"),
                     **{k: v[:2] for k, v in t.items()})
    assert a["wrt"] == ("cube_mass", "cube_frictionloss") and a["status_cols"].tolist() == [[3, 0], [3, 3]]
    # a NaN velocity: the rows stop
    t2 = {k: v[:2].clone() for k, v in t.items()}
    t2["qvel"][1, 0] = float("nan")
    b = env.param_fd(nsub=1, wrt="kp_scale", **t2)
    assert b["status_cols"].tolist() == [[0], [1]] and not b["deriv_t"][1].any()


# ------------------------------------------------------------------------------------------------------ gradients and sensitivities
GRAD_CELLS = ("C2", "G1", "G3")
T, NSUB = 3, 2
# the worst |sum_t lam_{t+1}' P_t - centred difference of the loss at h = 1e-4| over the three cells, each parameter's entry times the
# parameter (a relative change) and normalised by the cell's largest such entry: measured here and committed; the bar is 1000 x that, one
# digit up, by the rule above.  (The centred difference itself is no better than h^2 times the loss's third derivative.)
SPREAD_GRAD = 1.64e-8
BAR_GRAD = 2e-5
_CASE = {}


def _case(cell):
    """One FD cell of solo_arm as an identification problem: (cm, dict of [1, ..] CPU tensors q0, v0, w0, ctrl [1, T, nu])."""
    import torch
    if cell not in _CASE:
        cm = RO.fd_model("solo_arm", 1e-8)
        rows = RO.fd_rows("solo_arm", cm)
        i = RO.FD_CELLS["solo_arm"].index(cell)
        q0, v0, w0, c0 = (torch.from_numpy(rows[k][i:i + 1].copy()) for k in ("qpos", "qvel", "warm", "ctrl"))
        _CASE[cell] = (cm, dict(q0=q0, v0=v0, w0=w0, ctrl=c0[:, None].repeat(1, T, 1)))
    return _CASE[cell]


class _LinearCost:
    """sum_t w_t' [tangent_diff(qpos_t, ref_t) ; qvel_t]: linear in the state's tangent about the trajectory `ref` it is first used on."""

    def __init__(self, cm, w):
        self.cm, self.w, self.ref = cm, w, None

    def _x(self, qpos, qvel):
        import torch
        from gym_kmanip_amd.derivatives import tangent_diff
        if self.ref is None:
            self.ref = qpos.clone()
        n, L = qpos.shape[:2]
        dq = tangent_diff(self.cm, qpos.reshape(n * L, -1), self.ref.reshape(n * L, -1)).reshape(n, L, -1)
        return torch.cat([dq, qvel], dim=2)

    def total(self, qpos, qvel, ctrl):
        return (self._x(qpos, qvel) * self.w).sum(dim=(1, 2))

    def derivatives(self, qpos, qvel, ctrl):
        import torch
        self._x(qpos, qvel)
        return self.w.clone(), torch.zeros_like(ctrl), None, None


def _loss_at(cm, c, cost, params):
    import torch
    env = PO.OracleParamFd(cm, 1)
    env.set_env_params(**params)
    r = env.rollout(envs=torch.zeros(1, dtype=torch.int32), qpos=c["q0"], qvel=c["v0"], warm=c["w0"], ctrl=c["ctrl"], nsub=NSUB,
                    fields=("qpos", "qvel", "status"))
    assert not r["status"].any()
    return float(cost.total(torch.cat([c["q0"][:, None], r["qpos"]], 1), torch.cat([c["v0"][:, None], r["qvel"]], 1), c["ctrl"])[0])


def test_param_grad_matches_a_centred_difference_of_the_loss_and_the_forward_sensitivity():
    """rollout_param_grad on the stand-in at the check values, a linear loss with default_rng(5) weights, cells C2, G1 and G3, T = 3 steps
    of 2 sub-steps: grad_params against (loss(p_k (1 + h)) - loss(p_k (1 - h))) / (2 h p_k), h = 1e-4, within BAR_GRAD; and against
    sum_t w_t' S_t of param_sensitivity -- the same products summed in the other order -- within 1e-12 of the largest entry."""
    import torch
    from gym_kmanip_amd import sysid
    from gym_kmanip_amd.model import ENV_PARAMS
    h, worst, worst_fwd = 1e-4, 0.0, 0.0
    for cell in GRAD_CELLS:
        cm, c = _case(cell)
        w = torch.from_numpy(np.random.default_rng(5).standard_normal((1, T + 1, 2 * cm.nv)))
        cost = _LinearCost(cm, w)
        p0 = PO.true_params(cm)
        env = PO.OracleParamFd(cm, 1)
        env.set_env_params(**p0)
        g = sysid.rollout_param_grad(env, [0], c["q0"], c["v0"], c["w0"], c["ctrl"], cost, nsub=NSUB)
        assert env.param_fd_calls == 1 and not g["status"].any() and not g["status_fd"].any() and not g["status_param"].any()
        assert g["wrt"] == ENV_PARAMS and tuple(g["P"].shape) == (1, T, 2 * cm.nv, 4) and tuple(g["grad_params"].shape) == (1, 4)
        pv = np.array([p0[k] for k in ENV_PARAMS])
        grad = g["grad_params"][0].numpy() * pv
        fd = np.array([(_loss_at(cm, c, cost, dict(p0, **{k: p0[k] * (1 + h)})) - _loss_at(cm, c, cost, dict(p0, **{k: p0[k] * (1 - h)}))) / (2 * h)
                       for k in ENV_PARAMS])
        err = float(np.abs(grad - fd).max() / np.abs(fd).max())
        # the forward form: the same A and P
        S = sysid.param_sensitivity(g["A"], g["P"])
        fwd = torch.einsum("ntx,ntxp->np", w, S)[0].numpy() * pv
        err_fwd = float(np.abs(grad - fwd).max() / np.abs(grad).max())
        print("\ncell %s: grad p %s  centred difference %s  relative %.2e  forward form %.2e" % (cell, grad, fd, err, err_fwd))
        assert np.abs(fd).max() > 1e-6
        worst, worst_fwd = max(worst, err), max(worst_fwd, err_fwd)
    print("worst: %.3e against the centred difference, %.3e against the forward form" % (worst, worst_fwd))
    from test_forces_cpu import _round_up_one_digit
    assert 1000.0 * worst <= BAR_GRAD and worst_fwd <= 1e-12
    assert BAR_GRAD == pytest.approx(_round_up_one_digit(1000.0 * SPREAD_GRAD), rel=1e-12)


def test_param_sensitivity_under_gains_and_its_refusals():
    """S_0 = 0, S_1 = P_0, S_2 = (A_1 + B_1 K_1) P_0 + P_1 on random blocks; B without gains is refused."""
    import torch
    from gym_kmanip_amd import sysid
    rng = np.random.default_rng(0)
    A, B, K, P = (torch.from_numpy(rng.standard_normal(s)) for s in ((2, 2, 6, 6), (2, 2, 6, 3), (2, 2, 3, 6), (2, 2, 6, 4)))
    S = sysid.param_sensitivity(A, P, B=B, gains=K)
    assert tuple(S.shape) == (2, 3, 6, 4) and not S[:, 0].any() and torch.equal(S[:, 1], P[:, 0])
    assert torch.allclose(S[:, 2], (A[:, 1] + B[:, 1] @ K[:, 1]) @ P[:, 0] + P[:, 1], rtol=0, atol=1e-13)
    assert torch.equal(sysid.param_sensitivity(A, P)[:, 2], A[:, 1] @ P[:, 0] + P[:, 1])
    with pytest.raises(ValueError):
        sysid.param_sensitivity(A, P, B=B)
    lam = torch.from_numpy(rng.standard_normal((2, 3, 6)))
    assert torch.allclose(sysid.param_grad(lam, P), (P.transpose(2, 3) @ lam[:, 1:, :, None]).sum(dim=1)[:, :, 0], rtol=0, atol=1e-13)


def test_tracking_cost_is_the_quadratic_costs_sibling():
    """total = 1/2 sum residual' Q residual; lx = Q residual; zero at the observed trajectory; a diagonal and a full Q agree."""
    import torch
    from gym_kmanip_amd import sysid
    cm, c = _case("G1")
    rng = np.random.default_rng(1)
    qo = c["q0"][:, None].repeat(1, 2, 1)
    vo = c["v0"][:, None].repeat(1, 2, 1)
    q = qo.clone()
    q[:, :, :cm.nlink + 3] += torch.from_numpy(1e-2 * rng.standard_normal((1, 2, cm.nlink + 3)))
    v = vo + torch.from_numpy(1e-2 * rng.standard_normal((1, 2, cm.nv)))
    Q = torch.from_numpy(rng.uniform(0.5, 2.0, 2 * cm.nv))
    cost, full = sysid.TrackingCost(cm, qo, vo, Q), sysid.TrackingCost(cm, qo, vo, torch.diag(Q))
    r = cost.residual(q, v)
    assert tuple(r.shape) == (1, 2, 2 * cm.nv) and torch.allclose(r[:, :, :cm.nlink + 3], q[:, :, :cm.nlink + 3] - qo[:, :, :cm.nlink + 3], rtol=0, atol=1e-16)
    assert not cost.residual(qo, vo).any() and float(cost.total(qo, vo)[0]) == 0.0
    assert float(cost.total(q, v)[0]) == pytest.approx(0.5 * float((r * r * Q).sum()), rel=1e-14)
    ctrl = c["ctrl"][:, :1]
    lx, lu, lxx, luu = cost.derivatives(q, v, ctrl)
    assert torch.allclose(lx, r * Q, rtol=0, atol=1e-16) and not lu.any() and not luu.any() and tuple(lxx.shape) == (2, 2 * cm.nv, 2 * cm.nv)
    assert torch.equal(full.total(q, v), cost.total(q, v)) and torch.equal(full.derivatives(q, v, ctrl)[0], lx)


# ------------------------------------------------------------------------------------------------------------------------- identify
_IDENT = {}


def _identified(cell, iters=8):
    """identify on the stand-in from the model's defaults, the data noise-free from the check values: (cm, result, calls per iteration)."""
    import torch
    from gym_kmanip_amd import sysid
    if cell not in _IDENT:
        cm, c = _case(cell)
        real = PO.OracleParamFd(cm, 1)
        real.set_env_params(**PO.true_params(cm))
        obs = real.rollout(envs=torch.zeros(1, dtype=torch.int32), qpos=c["q0"], qvel=c["v0"], warm=c["w0"], ctrl=c["ctrl"], nsub=NSUB,
                           fields=("qpos", "qvel"))
        qo, vo = torch.cat([c["q0"][:, None], obs["qpos"]], 1), torch.cat([c["v0"][:, None], obs["qvel"]], 1)
        env = PO.OracleParamFd(cm, 1)
        seen = []
        res = sysid.identify(env, [0], c["q0"], c["v0"], c["w0"], c["ctrl"], qo, vo, iters=iters, nsub=NSUB,
                             callback=lambda it, p, loss, sv: seen.append((it, p.numpy().copy(), float(loss[0]))))
        _IDENT[cell] = (cm, res, env, seen)
    return _IDENT[cell]


def test_identify_recovers_all_four_parameters_of_a_grasp():
    """Cell G1, T = 3, nsub = 2, from the model's defaults: all four parameters within 1e-6 relative in at most 8 iterations (the
    first iterate that is within 1e-6 is printed); the handle holds the estimate; one param_fd call per linearisation."""
    from gym_kmanip_amd.model import ENV_PARAMS
    cm, res, env, seen = _identified("G1")
    tp = PO.true_params(cm)
    true = np.array([tp[k] for k in ENV_PARAMS])
    err = {k: abs(float(res["params"][k][0]) / tp[k] - 1.0) for k in ENV_PARAMS}
    first = next((it for it, p, _ in seen if np.abs(p[0] / true - 1.0).max() <= 1e-6), None)
    print("\nidentify on G1: relative errors %s, within 1e-6 from iteration %s, loss %s" % (err, first, res["loss"][:, 0].tolist()))
    assert first is not None and first <= 8 and max(err.values()) <= 1e-6
    assert int(res["status"].max()) == 0 and res["wrt"] == ENV_PARAMS and tuple(res["loss"].shape) == (9, 1) and tuple(res["accepted"].shape) == (8, 1)
    assert (np.diff(res["loss"][:, 0].numpy()) <= 0).all()                              # a step is taken only if the loss falls
    assert env.param_fd_calls == 9 and all(float(env.get_env_params()[k][0]) == float(res["params"][k][0]) for k in ENV_PARAMS)
    sv = res["singular_values"][0].numpy()
    assert sv.shape == (4,) and (np.diff(sv) <= 0).all() and sv[-1] > 1e-3 * sv[0]     # every direction is observable in a grasp


def test_identify_shows_the_unobservable_direction_of_a_cube_in_flight():
    """Cell C2: the smallest singular value of the scaled Jacobian is below 1e-6 of the largest -- only a combination of the cube's mass
    and friction loss shows in flight; friction and kp_scale are recovered, the loss falls to rounding."""
    cm, res, env, seen = _identified("C2")
    tp = PO.true_params(cm)
    sv = res["singular_values"][0].numpy()
    err = {k: abs(float(res["params"][k][0]) / tp[k] - 1.0) for k in tp}
    print("\nidentify on C2: singular values %s, relative errors %s, loss %.3e" % (sv, err, float(res["loss"][-1, 0])))
    assert sv[-1] < 1e-6 * sv[0]
    assert err["cube_friction"] <= 1e-6 and err["kp_scale"] <= 1e-6 and float(res["loss"][-1, 0]) < 1e-20


def test_identify_refuses_ranges_mode_and_repeated_envs():
    import torch
    from gym_kmanip_amd import sysid
    cm, c = _case("G1")
    env = PO.OracleParamFd(cm, 2)
    two = {k: v.repeat(2, *([1] * (v.dim() - 1))) for k, v in c.items()}
    obs = (two["q0"][:, None].repeat(1, T + 1, 1), two["v0"][:, None].repeat(1, T + 1, 1))
    with pytest.raises(ValueError, match="different envs"):
        sysid.identify(env, [0, 0], two["q0"], two["v0"], two["w0"], two["ctrl"], *obs, iters=1, nsub=NSUB)
    env._ep_ranges = (np.zeros(4), np.ones(4))
    with pytest.raises(ValueError, match="ranges mode"):
        sysid.identify(env, [0, 1], two["q0"], two["v0"], two["w0"], two["ctrl"], *obs, iters=1, nsub=NSUB)
    assert env.param_fd_calls == 0 and len(env.calls) == 0
    with pytest.raises(ValueError):
        sysid.identify(PO.OracleParamFd(cm, 2), [0, 1], two["q0"], two["v0"], two["w0"], two["ctrl"], *obs, wrt=("mass",), iters=1)


def test_the_examples_loop_runs_on_the_stand_in():
    """examples/system_identification.identify_log with kp_scale alone on cell G3, 4 iterations: the hidden value is recovered, the
    record names it, and the lines it prints carry the parameters, the loss and the singular values of every iteration."""
    import torch
    from gym_kmanip_amd.examples import system_identification as ex
    cm, c = _case("G3")
    real, model = PO.OracleParamFd(cm, 1), PO.OracleParamFd(cm, 1)
    real.set_env_params(kp_scale=1.2)
    lines = []
    st = dict(qpos=c["q0"], qvel=c["v0"], warm=c["w0"])
    res = ex.identify_log(real, model, st, c["ctrl"], wrt=("kp_scale",), iters=4, nsub=NSUB, verbose=lines.append)
    assert res["wrt"] == ("kp_scale",) and float(res["error"]["kp_scale"][0]) <= 1e-6 and bool(res["observable"][0])
    assert float(res["hidden"]["kp_scale"][0]) == 1.2 and int(res["status"].max()) == 0
    assert sum("singular values" in ln and "kp_scale" in ln and "loss" in ln for ln in lines) == 5
    assert "recovered kp_scale" in lines[-1] and "NOT recovered" not in lines[-1]
    assert float(real.get_env_params()["kp_scale"][0]) == 1.2                          # the real handle was only read


# ---------------------------------------------------------------------------------------------------------------------- the build
def test_param_fd_binding_matches_the_header():
    """lib.KParamFdIn / KParamFdDev list the header's fields in the header's order with the header's types and the C compiler's layout;
    the first six inputs are KRolloutIn's; the prototype is in the header, the symbol bound with the right argument types and listed
    among the exports; the version string is still 0.40."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    for name, cls in (("KParamFdIn", klib.KParamFdIn), ("KParamFdDev", klib.KParamFdDev)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(\w+)\s*(\*?)\s*(\w+)\s*(\[KM_EP_N\])?\s*;", body)
        assert [f for _, _, f, _ in fields] == [n for n, _ in cls._fields_], name
        want = [C.c_void_p if star else (ctype[t] * 4 if arr else ctype[t]) for t, star, _, arr in fields]
        assert want == [t for _, t in cls._fields_], name
    assert klib.KParamFdIn._fields_[:6] == klib.KRolloutIn._fields_[:6]
    assert [n for n, _ in klib.KParamFdIn._fields_[6:]] == ["params", "wrt", "eps", "eps_relative", "warm_offset"]
    # seven pointers, the mask, four bytes of padding, four doubles, the flag, four bytes of padding, a double: the LP64 layout
    I = klib.KParamFdIn
    assert (I.params.offset, I.wrt.offset, I.eps.offset, I.eps_relative.offset, I.warm_offset.offset, C.sizeof(I)) == (48, 56, 64, 96, 104, 112)
    assert C.sizeof(klib.KParamFdDev) == 24
    assert re.search(r"enum \{ KM_EP_CUBE_MASS = 0,.*KM_EP_N = 4 \};", hdr)
    assert "KMANIP_API int kmanip_param_fd(KHandle h, const KParamFdIn* in, int n, int nsub, const KParamFdDev* out, void* stream);" in hdr
    assert "kmanip_param_fd" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_param_fd.argtypes == [C.c_void_p, C.POINTER(klib.KParamFdIn), C.c_int, C.c_int, C.POINTER(klib.KParamFdDev), C.c_void_p]
    assert set(env_hip.KManipEnvHip._PARAMFD_FIELDS) == {n for n, _ in klib.KParamFdDev._fields_}
    assert " 0.40 " in L.kmanip_version().decode()


def test_the_eight_param_fd_objects_are_built_and_run_without_scratch():
    """The Makefile lists eight k_paramfd objects -- both classes, both solvers, the _ep_ and _ep_frc_ builds and no other -- and the
    built library holds exactly their kernels: 64 / G lane groups per wave, no scratch, registers within the 512 of a single-wave
    workgroup, and the LDS of the k_transfd sibling (the same workspace, model image and exchange array)."""
    from gym_kmanip_amd import lib as klib
    objs = BM.objects(BM.MAKEFILE, "paramfd")
    assert sorted(tuple(o[1:]) for o in objs) == sorted((nl, g, s, True, frc) for nl, g in ((10, 16), (20, 32)) for s in (0, 1) for frc in (False, True))
    rows = BM.kernels(klib.LIB_PATH, r"k_paramfd\w*")
    assert sorted((r.base, r.args[0], r.args[2]) for r in rows) == sorted((nm, nl, s) for nm in ("k_paramfd_ep", "k_paramfd_ep_frc") for nl in (10, 20) for s in (0, 1))
    sib = {(r.base.replace("k_transfd", "k_paramfd"), r.args[0], r.args[2]): r for r in BM.kernels(klib.LIB_PATH, r"k_transfd_ep\w*")}
    for r in rows:
        nl, g, solver, epb = r.args
        assert (g, epb) == ((16, 4) if nl == 10 else (32, 2)), r
        assert r.scratch == 0 and r.vgpr <= 512 and r.lds == sib[(r.base, nl, solver)].lds, r


def covered(handle_rows):
    """The (NL, G, SOLVER, ep, frc) objects the device test's rows launch (kmanip_dispatch.hip: always a parameter build; the force
    build while the call gives a force or one is bound)."""
    import regime_states as R
    out = set()
    for asset, solver, mode in handle_rows:
        cls = (10, 16) if R.model(asset).nlink <= 10 else (20, 32)
        out.add(cls + ({"pgs": 0, "newton": 1}[solver], True, "forced" in mode or "bound" in mode))
    return out


def test_every_compiled_param_fd_object_has_a_row():
    from test_param_fd_gpu import HANDLE_ROWS
    have = covered(HANDLE_ROWS)
    assert [tuple(o[1:]) for o in BM.objects(BM.MAKEFILE, "paramfd") if tuple(o[1:]) not in have] == []
