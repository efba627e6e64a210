"""kmanip_site_cost and kmanip_kinematics_rows on the CPU (no GPU): the bar of tests/test_site_cost_gpu.py, the cost's definition
(ilqr.site_cost_rows, what ilqr.SiteCost(device=False) evaluates) against finite differences and against J'WJ, the bindings, the
library's new kernels and the planner loop on the oracle's stand-in (tests/tools/site_cost_reference.py).

THE BAR.  Over the input family of site_cost_reference (the regime cells of the three assets, both follow_cube values), cost, lx and
lxx of two double-precision evaluations -- torch's site_cost_rows through the stand-in's kinematics_at, and restate(dtype=float64) --
are compared with restate in np.longdouble from the same geometry, each output relative to the row's largest entry of that output.
The worst figure is the reference's own rounding spread; BAR_SITE_COST is 1000 x it, rounded up to one digit, never below 1e-12
(the rule of DESIGN.md sections 19, 37 and 39)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import kin_oracle as KO  # noqa: E402
import mujoco_pin  # noqa: E402
import site_cost_reference as SR  # noqa: E402

ASSETS = mujoco_pin.ASSETS
OUTPUTS = ("cost", "lx", "lxx")
# the worst relative distance of the two double evaluations from the longdouble restatement, measured by
# test_the_bar_is_a_thousand_times_the_references_spread
SPREAD_SITE_COST = 2.9e-15
BAR_SITE_COST = 3e-12
# central differences of the cost with h = 1e-6, relative to the row's max |lx|: truncation h^2 |d3 cost| / 6 with third derivatives
# within 1e3 x max |lx| (the weights times products of Jacobian entries of order one and their derivatives) ~ 2e-10; round-off
# 2^-53 cost / h with cost / max |lx| below 10 (|e| against a Jacobian column of order one) ~ 2e-9.  The bar is 50 x their sum.
FD_H = 1e-6
BAR_FD = 1e-7
# The reach of examples/ilqr_site_reach.plan on the stand-in (2 envs, horizon 3, 2 iterations, seed 3): the median site-to-target
# distance after the plan over the one before it, measured by test_ilqr_with_a_site_cost_on_the_stand_in, and the fraction asserted
# there and on the device: the measured one with the margin resolved_rate_reach took (0.23 measured, 0.6 asserted), at most 1.
REACH_MEASURED = {("KManipSoloArmQPos", False): 0.009, ("KManipSoloArmQPos", True): 0.322,
                  ("KManipDualArmQPos", False): 0.011, ("KManipDualArmQPos", True): 0.685}
REACH_ASSERTED = {k: min(1.0, v * 0.6 / 0.23) for k, v in REACH_MEASURED.items()}


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


_ENVS = {}


def _stand_in(cm):
    if id(cm) not in _ENVS:
        _ENVS[id(cm)] = SR.OracleSite(cm, 2)
    return _ENVS[id(cm)]


def _rows(fam, qpos=None, target_pos=None, target_quat="family", weight=None, want_derivatives=True):
    """ilqr.site_cost_rows over the family's rows on the stand-in (every row names env 0), as NumPy."""
    import torch
    from gym_kmanip_amd import ilqr
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    q = fam["qpos"] if qpos is None else qpos
    n = len(q)
    tq = fam["target_quat"] if isinstance(target_quat, str) else target_quat
    r = ilqr.site_cost_rows(_stand_in(fam["cm"]), torch.zeros(n, dtype=torch.int32), t(q), t(fam["qvel"][:n]),
                            t(fam["target_pos"] if target_pos is None else target_pos), t(tq), t(fam["weight"] if weight is None else weight),
                            fam["follow"], want_derivatives)
    return {k: v.numpy() for k, v in r.items()}


def worst_relative(got, fam):
    """{output: (worst over the rows of max |got - ref| / max |ref|, row)} against the family's longdouble reference."""
    out = {}
    for k in OUTPUTS:
        figs = [SR.relative(got[k][e], fam["ref"][e][k]) for e in range(len(fam["ref"]))]
        e = int(np.argmax(figs))
        out[k] = (figs[e], e)
    return out


def test_the_family_keeps_every_state_and_deals_every_weight_pattern():
    for asset in ASSETS:
        for follow in (False, True):
            fam = SR.family(asset, follow)
            assert fam["kept"].all() and len(fam["kept"]) in (47, 72), (asset, follow)
            d = fam["cm"].desc
            for a in range(2):
                if d.arm_present[a]:
                    seen = {tuple(w) for w in fam["weight"][:, a]}
                    assert seen == {(p, r) for p in SR.WEIGHTS for r in SR.WEIGHTS}, (asset, a)       # all zeros and rotation only among them
            ang = np.array([[np.linalg.norm(np.asarray(r["resid"][a, 3:], dtype=np.float64)) for a in range(2)] for r in fam["ref"]])
            assert ang.max() < SR.MAX_EROT


def test_the_bar_is_a_thousand_times_the_references_spread():
    worst = 0.0
    for asset in ASSETS:
        for follow in (False, True):
            fam = SR.family(asset, follow)
            n = len(fam["ref"])
            torch_rows = _rows(fam)
            assert not torch_rows["status"].any()
            f64 = [SR.restate(fam["cm"], fam["geo"][e], fam["qpos"][e], fam["target_pos"][e], fam["target_quat"][e], fam["weight"][e],
                              fam["follow"], dtype=np.float64) for e in range(n)]
            for name, got in (("torch", torch_rows), ("float64", {k: [r[k] for r in f64] for k in OUTPUTS})):
                w = worst_relative(got, fam)
                print("\n%s follow %d, %s vs longdouble: %s" % (asset, follow, name, "  ".join("%s %.1e (row %d)" % ((k,) + w[k]) for k in OUTPUTS)))
                worst = max(worst, max(v for v, _ in w.values()))
    print("worst spread %.2e" % worst)
    assert 1000.0 * worst <= BAR_SITE_COST
    assert BAR_SITE_COST == pytest.approx(max(1e-12, _round_up_one_digit(1000.0 * SPREAD_SITE_COST)), rel=1e-12)
    assert worst > 0.5 * SPREAD_SITE_COST                      # ... and the recorded spread not far above what is measured


@pytest.mark.parametrize("asset", ASSETS)
def test_lx_is_the_central_difference_of_the_cost(asset):
    """Every tangent column through derivatives.tangent_perturb, h = 1e-6; the cube's position columns with follow_cube on (they are
    exact zeros without it), the cube's rotation columns exactly 0."""
    import torch
    from gym_kmanip_amd.derivatives import tangent_perturb
    worst = 0.0
    for follow in (False, True):
        fam = SR.family(asset, follow)
        cm = fam["cm"]
        nl, nv = cm.nlink, cm.nv
        lx = _rows(fam)["lx"]
        assert not lx[:, nv:].any() and not lx[:, nl + 3:nv].any()
        assert (not lx[:, nl:nl + 3].any()) != follow
        scale = np.where(np.abs(lx).max(axis=1) > 0, np.abs(lx).max(axis=1), 1.0)
        q = torch.from_numpy(fam["qpos"].copy())
        for col in range(nv):
            c = [_rows(fam, qpos=tangent_perturb(cm, q, col, s * FD_H).numpy(), want_derivatives=False)["cost"] for s in (1.0, -1.0)]
            fd = (c[0] - c[1]) / (2 * FD_H)
            if col >= nl + 3:
                assert not fd.any(), col
            worst = max(worst, float((np.abs(fd - lx[:, col]) / scale).max()))
    print("\n%s: lx vs central differences of the cost (h = %g), worst relative to max |lx| over all columns: %.1e" % (asset, FD_H, worst))
    assert worst <= BAR_FD


@pytest.mark.parametrize("asset", ASSETS)
def test_lxx_is_jtwj_and_the_derivative_of_lx_at_a_zero_residual(asset):
    import torch
    from gym_kmanip_amd.derivatives import tangent_perturb
    import regime_states as R
    for follow in (False, True):
        fam = SR.family(asset, follow)
        cm = fam["cm"]
        d, nl, nv = cm.desc, cm.nlink, cm.nv
        lxx = _rows(fam)["lxx"]
        for e, o in enumerate(fam["geo"]):
            H = np.zeros((2 * nv, 2 * nv))
            for a in range(2):
                if d.arm_present[a]:
                    Jp, Jr = o["site_jacp"][a].copy(), o["site_jacr"][a]
                    if follow:
                        Jp[:, nl:nl + 3] = -np.eye(3)
                    H[:nv, :nv] += fam["weight"][e, a, 0] * Jp.T @ Jp + fam["weight"][e, a, 1] * Jr.T @ Jr
            scale = max(np.abs(H).max(), 1e-300)
            assert np.abs(lxx[e] - H).max() <= BAR_SITE_COST * scale if H.any() else not lxx[e].any(), e
            assert np.abs(lxx[e] - lxx[e].T).max() <= BAR_SITE_COST * scale
            assert np.linalg.eigvalsh(0.5 * (lxx[e] + lxx[e].T)).min() >= -BAR_SITE_COST * scale * 2 * nv
            assert not lxx[e, nv:].any() and not lxx[e, :, nv:].any() and not lxx[e, nl + 3:nv].any()
        # e = 0: the target is the site's own pose, Gauss-Newton is exact there
        tp = np.stack([o["site_xpos"] for o in fam["geo"]]) - (fam["qpos"][:, None, nl:nl + 3] if follow else 0.0)
        tq = np.zeros((len(tp), 2, 4)); tq[:, :, 0] = 1.0
        for e, o in enumerate(fam["geo"]):
            for a in range(2):
                if d.arm_present[a]:
                    tq[e, a] = R.mat2quat(o["site_xmat"][a].reshape(3, 3))
        base = _rows(fam, target_pos=tp, target_quat=tq)
        assert np.abs(base["cost"]).max() < 1e-25
        scale = np.where(np.abs(base["lxx"]).max(axis=(1, 2)) > 0, np.abs(base["lxx"]).max(axis=(1, 2)), 1.0)
        q = torch.from_numpy(fam["qpos"].copy())
        worst = 0.0
        for col in range(nv):
            g = [_rows(fam, qpos=tangent_perturb(cm, q, col, s * FD_H).numpy(), target_pos=tp, target_quat=tq)["lx"] for s in (1.0, -1.0)]
            fd = (g[0] - g[1]) / (2 * FD_H)
            worst = max(worst, float((np.abs(fd - base["lxx"][:, col]).max(axis=1) / scale).max()))
        print("\n%s follow %d: lxx vs central differences of lx at e = 0, worst relative to max |lxx|: %.1e" % (asset, follow, worst))
        assert worst <= BAR_FD


def _header_fields(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kmanip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"[\*\s](\w+)\s*(?:\[\w+\])?;", body), hdr


def test_the_bindings_match_the_header():
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    for name, want in (("KKinRowsIn", ["env_index", "qpos", "qvel"]),
                       ("KSiteCostIn", ["env_index", "qpos", "target_pos", "target_quat", "weight", "follow_cube"]),
                       ("KSiteCostDev", ["cost", "lx", "lxx", "site_xpos", "resid", "status"])):
        fields, hdr = _header_fields(name)
        assert fields == [n for n, _ in getattr(klib, name)._fields_] == want, name
    assert all(t is C.c_void_p for _, t in klib.KKinRowsIn._fields_ + klib.KSiteCostDev._fields_ + klib.KSiteCostIn._fields_[:-1])
    assert klib.KSiteCostIn._fields_[-1][1] is C.c_int32 * 2 and "#define KM_MAX_ARMS 2" in re.sub(r"[ \t]+", " ", hdr)
    assert list(env_hip.KManipEnvHip._SITE_COST_FIELDS) == [n for n, _ in klib.KSiteCostDev._fields_]
    assert "KMANIP_API int kmanip_kinematics_rows(KHandle h, const KKinRowsIn* in, int n, const KKinDev* out, void* stream);" in hdr
    assert "KMANIP_API int kmanip_site_cost(KHandle h, const KSiteCostIn* in, int n, const KSiteCostDev* out, void* stream);" in hdr
    assert "kmanip_kinematics_rows" in klib.EXPORTS and "kmanip_site_cost" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_kinematics_rows.argtypes == [C.c_void_p, C.POINTER(klib.KKinRowsIn), C.c_int, C.POINTER(klib.KKinDev), C.c_void_p]
    assert L.kmanip_site_cost.argtypes == [C.c_void_p, C.POINTER(klib.KSiteCostIn), C.c_int, C.POINTER(klib.KSiteCostDev), C.c_void_p]
    assert b"0.40" in L.kmanip_version()
    assert len(klib.KKinDev._fields_) == 10


# ------------------------------------------------------------------------------------------------------ the library's new kernels
def covered(rows):
    """The (NL, G, ep) sitekin objects that a GPU file's (asset, mode) rows launch (kmanip_dispatch.hip: the 10-link class for
    nlink <= 10, the parameter build while the handle has per-env parameters)."""
    import regime_states as R
    return {((10, 16) if R.model(asset).nlink <= 10 else (20, 32)) + ("params" in mode,) for asset, mode in rows}


def missing_rows(makefile_path, rows):
    import build_matrix as BM
    have = covered(rows)
    return [(o.NL, o.G, o.ep) for o in BM.objects(makefile_path, "sitekin") if (o.NL, o.G, o.ep) not in have]


def test_shipped_row_kernels_run_without_scratch_and_every_object_has_a_row(tmp_path):
    """k_kinrows* / k_sitecost* of the built library (parsed from the .so: no GPU): four variants each, none spills, no LDS beyond the
    k_kinematics sibling's; and every sitekin object `make print-objs` lists is launched by a row of both GPU files."""
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    from test_kinematics_rows_gpu import LAUNCH_ROWS as KIN_ROWS
    from test_site_cost_gpu import LAUNCH_ROWS as COST_ROWS
    kin = {(r.base, r.args[0]): r for r in BM.kernels(klib.LIB_PATH, r"k_kinematics\w*")}
    for base in ("k_kinrows", "k_sitecost"):
        rows = BM.kernels(klib.LIB_PATH, base + r"\w*")
        assert sorted((r.base,) + r.args for r in rows) == [(base, 10, 16, 4), (base, 20, 32, 2), (base + "_ep", 10, 16, 4), (base + "_ep", 20, 32, 2)]
        for r in rows:
            sib = kin[("k_kinematics" + r.base[len(base):], r.args[0])]
            assert r.scratch == 0 and r.vgpr <= 512 and r.lds <= sib.lds, (r, sib)
    objs = BM.objects(BM.MAKEFILE, "sitekin")
    assert sorted((o.NL, o.G, o.solver, o.ep, o.frc) for o in objs) == [(10, 16, None, False, False), (10, 16, None, True, False),
                                                                        (20, 32, None, False, False), (20, 32, None, True, False)]
    for rows in (KIN_ROWS, COST_ROWS):
        assert missing_rows(BM.MAKEFILE, rows) == []
        assert missing_rows(BM.MAKEFILE, [r for r in rows if "params" not in r[1]]) == [(10, 16, True), (20, 32, True)]
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    assert missing_rows(more, KIN_ROWS) == [(30, 64, False), (30, 64, True)]


# ------------------------------------------------------------------------------------------------------------------- the planner
def _reset_states(env_id, n, seed=3):
    import torch
    from gym_kmanip_amd.model import compile_model
    from oracle.oracle import Oracle
    cm = compile_model(env_id)
    orc = Oracle(cm, n, seed=seed)
    orc.reset()
    s = orc.get_state()
    return cm, {k: torch.from_numpy(s[i].copy()) for i, k in enumerate(("qpos", "qvel", "ctrl", "warm"))}


@pytest.mark.parametrize("env_id,cube", sorted(REACH_MEASURED))
def test_ilqr_with_a_site_cost_on_the_stand_in(env_id, cube):
    """examples/ilqr_site_reach.plan -- SumCost(QuadraticCost, SiteCost(device=False)), the torch backward pass -- on the stand-in: 2
    envs, horizon 3, 2 iterations.  The accepted costs never increase and the median site-to-target distance ends below
    REACH_ASSERTED x its start (measured: REACH_MEASURED)."""
    from gym_kmanip_amd.examples import ilqr_site_reach as EX
    cm, st = _reset_states(env_id, 2)
    out = EX.plan(SR.OracleSite(cm, 2), st, horizon=3, iters=2, cube=cube)
    J = out["res"]["cost"].numpy()
    ratio = out["end"] / out["start"]
    print("\n%s cube %d: mean cost %s, median distance %.4f -> %.4f m (%.3f x; asserted %.3f x)"
          % (env_id, cube, out["cost"], out["start"], out["end"], ratio, REACH_ASSERTED[(env_id, cube)]))
    assert J.shape == (3, 2) and np.isfinite(J).all() and (np.diff(J, axis=0) <= 0).all() and (J[-1] < J[0]).all()
    assert ratio < REACH_ASSERTED[(env_id, cube)]
    assert abs(ratio - REACH_MEASURED[(env_id, cube)]) <= 0.05 * REACH_MEASURED[(env_id, cube)] + 5e-4      # the recorded figure is this run's


def test_boxed_ilqr_with_a_site_cost_and_the_quadratic_cost_alone():
    """The same loop control-limited (one box for both envs, 0.05 around their initial ctrl): every control of the plan in the box, the
    history never increasing, the distance falling.  And QuadraticCost alone through SumCost: ilqr's result bit for bit."""
    import torch
    from gym_kmanip_amd import ilqr
    from gym_kmanip_amd.examples import ilqr_site_reach as EX
    cm, st = _reset_states("KManipSoloArmQPos", 2)
    box = dict(ctrl_lo=st["ctrl"].min(dim=0).values - 0.05, ctrl_hi=st["ctrl"].max(dim=0).values + 0.05)
    out = EX.plan(SR.boxed_stand_in(cm, 2), st, horizon=3, iters=2, box=box)
    J, u = out["res"]["cost"].numpy(), out["res"]["ctrl"]
    print("\nboxed: mean cost %s, median distance %.4f -> %.4f m" % (out["cost"], out["start"], out["end"]))
    assert (np.diff(J, axis=0) <= 0).all() and out["end"] < out["start"]
    assert bool(((u >= box["ctrl_lo"]) & (u <= box["ctrl_hi"])).all()) and "clamped" in out["res"] and bool(out["res"]["clamped"].any())
    goal = st["qpos"].clone()
    goal[:, :cm.nlink] += 0.1
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64)
    wq[:cm.nlink], wq[cm.nv:cm.nv + cm.nlink] = 10.0, 0.01
    quad = ilqr.QuadraticCost(cm, goal, torch.zeros((2, cm.nv), dtype=torch.float64), wq, torch.full((cm.nu,), 1e-3, dtype=torch.float64), 10.0 * wq)
    guess = st["ctrl"][:, None].repeat(1, 3, 1)
    runs = [ilqr.ilqr(SR.OracleSite(cm, 2), None, st["qpos"], st["qvel"], st["warm"], guess, c, iters=2) for c in (quad, ilqr.SumCost(quad))]
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in ("ctrl", "cost", "accepted", "k", "K", "reg"))
    assert bool((runs[0]["cost"][-1] < runs[0]["cost"][0]).all())
    # a per-problem lxx goes through the shapes a shared one does
    lx, lu, lxx, luu = ilqr.SumCost(quad, ilqr.SiteCost(SR.OracleSite(cm, 2), out["target_pos"])).derivatives(
        st["qpos"][:, None].repeat(1, 4, 1), st["qvel"][:, None].repeat(1, 4, 1), guess)
    assert tuple(lxx.shape) == (2, 4, 2 * cm.nv, 2 * cm.nv) and tuple(luu.shape) == (3, cm.nu, cm.nu) and tuple(lx.shape) == (2, 4, 2 * cm.nv)


def test_site_cost_spreads_a_target_trajectory_and_the_final_weights_over_the_rows():
    """SiteCost with targets to track [n0, T + 1, arms, 3] (one slot per present arm), per-arm weights and final weights, 2 n0 rows (a
    line search's): total and lx are site_cost_rows' with row a n0 + e on entry e, the last state under the final weights."""
    import torch
    from gym_kmanip_amd import ilqr
    fam = SR.family("dual_arm", False)
    cm = fam["cm"]
    env = _stand_in(cm)
    n0, T = 2, 2
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    q = t(fam["qpos"][:2 * n0 * (T + 1)]).reshape(2 * n0, T + 1, -1)
    v = t(fam["qvel"][:2 * n0 * (T + 1)]).reshape(2 * n0, T + 1, -1)
    tp = t(fam["target_pos"][:n0 * (T + 1)]).reshape(n0, T + 1, 2, 3)
    tq = t(fam["target_quat"][:n0 * (T + 1)]).reshape(n0, T + 1, 2, 4)
    cost = ilqr.SiteCost(env, tp, tq, w_pos=[2.0, 3.0], w_rot=0.5, wf_pos=[20.0, 30.0], wf_rot=[0.0, 1.5])
    u = torch.zeros((2 * n0, T, cm.nu), dtype=torch.float64)
    lx, lu, lxx, luu = cost.derivatives(q, v, u)
    total = cost.total(q, v, u)
    assert tuple(lxx.shape) == (2 * n0, T + 1, 2 * cm.nv, 2 * cm.nv) and not lu.any() and not luu.any()
    for r in range(2 * n0):
        e, c = r % n0, 0.0
        for s in range(T + 1):
            w = torch.tensor([[2.0, 0.5], [3.0, 0.5]] if s < T else [[20.0, 0.0], [30.0, 1.5]], dtype=torch.float64)
            one = ilqr.site_cost_rows(env, torch.tensor([e], dtype=torch.int32), q[r, s:s + 1], v[r, s:s + 1], tp[e, s:s + 1], tq[e, s:s + 1],
                                      w[None], (False, False))
            c = c + float(one["cost"][0])
            assert torch.equal(one["lx"][0], lx[r, s]) and torch.equal(one["lxx"][0], lxx[r, s]), (r, s)
        assert abs(c - float(total[r])) <= 1e-12 * c
    bad = q.clone()                                        # (q shares the cells' memory)
    bad[1, 1, 0] = float("nan")
    assert torch.isinf(cost.total(bad, v, u)).tolist() == [False, True, False, False]
