"""Control-limited iLQR on the CPU: the bar the references set for tests/test_lqr_box_gpu.py, the box family's
coverage, every step's QP against the KKT conditions and SciPy's BVLS, the two new entries in the header, the binding and the built
library, and ilqr.ilqr(ctrl_lo=, ctrl_hi=) over a stand-in (tests/tools/boxqp_reference.py OracleLqrBox)."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import boxqp_reference as BQ  # noqa: E402
import build_matrix as BM  # noqa: E402
import riccati_reference as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------------ the bar
# ilqr.backward_pass_box (torch float64) and boxqp_reference.riccati_box in float64 against riccati_box in longdouble on
# boxqp_reference.family (seed 17): both classes, T in {1, 2, 5, 12}, 3 problems, reg in {0, 0.3}; per problem the largest difference
# divided by the largest |k|, |K|, |dV| of the problem.  Measured here and committed: the worst over everything,
SPREAD = {"k": 4.1e-15, "K": 2.1e-15, "dV": 3.9e-16}
# (torch's; the float64 restatement's: 2.9e-15, 1.4e-15, 3.7e-16.)  The bar of tests/test_lqr_box_gpu.py is 1000 x the worst of them,
# one digit up -- section 37's derivation.  The masks and the QP's step counts must be equal exactly.
BAR = 5e-12
BAR_37 = 2e-12                       # section 37's, for the pass with an infinite box against the unconstrained one
T_SET, REGS, N_PROBLEMS = (1, 2, 5, 12), (0.0, 0.3), 3
NAMES = ("A", "B", "lx", "lu", "lxx", "luu", "u", "lo", "hi")


def gaps(got, ref):
    """{k, K, dV: the worst over the problems of max |got - ref| / max |ref|}; got float64 arrays, ref longdouble.  A problem whose
    reference is all zeros (every actuator clamped at d = 0) must be zeros."""
    out = {}
    for name in ("k", "K", "dV"):
        n = len(ref[name])
        d = np.abs(np.asarray(got[name]).astype(np.longdouble) - ref[name]).reshape(n, -1).max(axis=1)
        top = np.abs(ref[name]).reshape(n, -1).max(axis=1)
        assert not d[top == 0].any(), name
        out[name] = float((d[top > 0] / top[top > 0]).max(initial=0))
    return out


def torch_pass(g, reg):
    """ilqr.backward_pass_box on the family's arrays: (dict(k, K, dV) as NumPy, clamped, info)."""
    import torch
    from gym_kmanip_amd import ilqr
    info = {}
    k, K, dV, c = ilqr.backward_pass_box(*(torch.from_numpy(g[name]) for name in NAMES), reg=reg, info=info)
    return dict(k=k.numpy(), K=K.numpy(), dV=dV.numpy()), c.numpy(), info


def test_the_references_agree_far_inside_the_bar_they_set():
    """The spread is measured again and printed; torch's backward_pass_box and the float64 restatement stay a hundred times inside
    the committed bar, their masks and step counts are the longdouble restatement's exactly, no problem fails, every margin of the
    family holds, and the bar is the committed spread's: 1000 x its worst, one digit up."""
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs a longdouble wider than float64"
    worst = {"torch": dict.fromkeys(SPREAD, 0.0), "float64": dict.fromkeys(SPREAD, 0.0)}
    for nx, nu in RR.CLASSES:
        for T in T_SET:
            for reg in REGS:
                g, ref, _ = BQ.family(nx, nu, T, N_PROBLEMS, reg)
                assert not ref["status"].any() and (ref["fail_step"] == -1).all() and min(ref["margins"].values()) > BQ.MARGIN
                r64 = BQ.batch(**g, reg=reg)
                got, c, info = torch_pass(g, reg)
                assert not r64["status"].any() and not info["status"].any()
                assert np.array_equal(r64["clamped"], ref["clamped"]) and np.array_equal(c, ref["clamped"])
                assert np.array_equal(r64["qp_iters"], ref["qp_iters"]) and np.array_equal(info["qp_iters"].numpy(), ref["qp_iters"])
                for tag, res in (("torch", got), ("float64", r64)):
                    for name, gap in gaps(res, ref).items():
                        worst[tag][name] = max(worst[tag][name], gap)
    print("\nspread against the longdouble restatement: %s" % worst)
    for tag in worst:
        for name in SPREAD:
            assert worst[tag][name] <= BAR / 100.0, (tag, name, worst[tag][name])
    top = max(SPREAD.values())
    assert BAR >= 1000.0 * top and BAR <= 2000.0 * top


def test_the_family_shows_every_pattern_and_every_qp_is_the_kkt_point_bvls_finds():
    """Per class, over the family, by the longdouble reference's own masks: a step with nothing clamped, one clamped low, one
    clamped high, a step with every actuator clamped, a problem whose clamped set changes between steps.  Every step's k is feasible,
    has g = 0 on the free coordinates, g >= 0 at a lower and g <= 0 at an upper bound (to 1e-12 of max |Qu|: the reference's own
    rounding is 1e-19), and is the minimiser scipy.optimize.lsq_linear(method="bvls") finds on the factor of H, which shares no
    code with it (to 1e-9 of the largest |d|: BVLS solves its free block by lstsq in float64)."""
    for nx, nu in RR.CLASSES:
        seen = dict.fromkeys(("none", "low", "high", "all", "change"), 0)
        worst = dict(feas=0.0, free=0.0, clamped=0.0, bvls=0.0)
        for T in T_SET:
            for reg in REGS:
                _, ref, _ = BQ.family(nx, nu, T, N_PROBLEMS, reg)
                for e in range(N_PROBLEMS):
                    masks = [int(m) for m in ref["clamped"][e]]
                    seen["change"] += len(set(masks)) > 1
                    for t in range(T):
                        H, q, bl, bh = ref["qps"][e][t]
                        d = ref["k"][e, t]
                        c = np.array([(masks[t] >> i) & 1 for i in range(nu)], dtype=bool)
                        seen["none"] += masks[t] == 0
                        seen["all"] += masks[t] == (1 << nu) - 1
                        seen["low"] += bool((c & (d == bl)).any())
                        seen["high"] += bool((c & (d == bh)).any())
                        for name, v in BQ.kkt(H, q, bl, bh, d, c).items():
                            worst[name] = max(worst[name], v)
                        x = BQ.bvls(H, q, bl, bh)
                        worst["bvls"] = max(worst["bvls"], float(np.abs(x - d.astype(np.float64)).max() / max(np.abs(x).max(), 1e-300)))
                    assert not ref["K"][e][np.array([[(m >> i) & 1 for i in range(nu)] for m in masks], dtype=bool)].any()
        print("\n(%d, %d): steps by pattern %s; worst KKT residuals and distance to BVLS %s" % (nx, nu, seen, worst))
        assert all(seen.values()), seen
        assert worst["feas"] == 0.0 and worst["free"] <= 1e-12 and worst["clamped"] == 0.0 and worst["bvls"] <= 1e-9, worst


def test_with_an_infinite_box_the_pass_is_the_unconstrained_one():
    """backward_pass_box with lo = -inf, hi = +inf against backward_pass: within section 37's 2e-12, nothing clamped, one QP step."""
    import torch
    from gym_kmanip_amd import ilqr
    for nx, nu in RR.CLASSES:
        for T, reg in ((1, 0.0), (5, 0.3)):
            f = {name: torch.from_numpy(v) for name, v in RR.family(nx, nu, T, N_PROBLEMS).items()}
            want = dict(zip(("k", "K", "dV"), ilqr.backward_pass(*(f[name] for name in NAMES[:6]), reg=reg)))
            inf = torch.full((nu,), float("inf"), dtype=torch.float64)
            info = {}
            k, K, dV, c = ilqr.backward_pass_box(*(f[name] for name in NAMES[:6]), torch.zeros_like(f["lu"]), -inf, inf, reg=reg, info=info)
            assert not c.any() and not info["status"].any() and bool((info["qp_iters"] == 1).all())
            for name, got in (("k", k), ("K", K), ("dV", dV)):
                gap = float(((got - want[name]).abs().reshape(N_PROBLEMS, -1).amax(dim=1) / want[name].abs().reshape(N_PROBLEMS, -1).amax(dim=1)).max())
                assert gap <= BAR_37, (name, gap)


def test_the_restatement_and_torch_classify_failures_alike():
    """An indefinite free block (luu = -I at the first step solved), lo > hi and a NaN bound give status 1, fail_step T - 1 and
    zeros, in the restatement and in torch's pass; the neighbours are untouched."""
    nx, nu = RR.CLASSES[0]
    g, ref, _ = BQ.family(nx, nu, 2, N_PROBLEMS, 0.0)
    good, _, _ = torch_pass(g, 0.0)
    for spoil in ("luu", "lo>hi", "nan"):
        bad = {name: v.copy() for name, v in g.items()}
        if spoil == "luu":
            bad["luu"][1, 1] = -np.eye(nu)
            bad["lo"][1], bad["hi"][1] = -np.inf, np.inf
        elif spoil == "lo>hi":
            bad["lo"][1, 3] = bad["hi"][1, 3] + 1.0
        else:
            bad["hi"][1, 2] = np.nan
        r = BQ.batch(**bad)
        got, c, info = torch_pass(bad, 0.0)
        for st, fs, res, cl in ((r["status"], r["fail_step"], r, r["clamped"]), (info["status"].numpy(), info["fail_step"].numpy(), got, c)):
            assert st.tolist() == [0, 1, 0] and fs.tolist() == [-1, 1, -1], spoil
            assert not res["k"][1].any() and not res["K"][1].any() and not res["dV"][1].any() and not cl[1].any()
        assert all(np.array_equal(got[name][[0, 2]], good[name][[0, 2]]) for name in ("k", "K", "dV"))


# ------------------------------------------------------------------------------------------------------------------ the library
def _fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for t, star, names in re.findall(r"(\w+)\s*(\*?)\s*([\w, ]+);", body):
        out += [(t, star, nm.strip()) for nm in names.split(",")]
    return out


def test_the_library_holds_the_box_kernels_and_the_binding_follows_the_header():
    """Parsed from the .so (no GPU): one k_lqr_backward_box per (nx, nu) class without scratch, LDS within the 160 KB of a CU; as many
    k_boxfb kernels as the Makefile has boxfb objects, none with more scratch than its k_feedback sibling; the header declares both
    entries, the bindings list their structs' fields in the header's order, and both symbols are exported and bound."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, "k_lqr_backward_box")
    assert sorted(r.args for r in rows) == sorted(RR.CLASSES)
    for r in rows:
        nx, nu = r.args
        lx, lu = nx | 1, nu | 1
        assert r.scratch == 0 and r.agpr <= r.vgpr <= 512, r          # (vgpr: the unified count, the AGPRs in it)
        assert r.lds == 8 * (3 * nx * lx + 2 * nu * lx + max(nx * lu, nu * lx) + 2 * nu * lu + 2 * nx + 4 * nu) + 16 <= 160 * 1024, r
    objs = BM.objects(BM.MAKEFILE, "boxfb")
    assert sorted(tuple(o[1:]) for o in objs) == sorted(tuple(o[1:]) for o in BM.objects(BM.MAKEFILE, "feedback")) and len(objs) == 16
    box = {(k.base.replace("k_boxfb", ""), k.args): k for k in BM.kernels(klib.LIB_PATH, r"k_boxfb\w*")}
    sib = {(k.base.replace("k_feedback", ""), k.args): k for k in BM.kernels(klib.LIB_PATH, r"k_feedback\w*")}
    assert len(box) == len(objs) and set(box) == set(sib)
    for key, k in box.items():
        assert k.scratch <= sib[key].scratch and k.lds == sib[key].lds, (k, sib[key])
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "KLqrIn": klib.KLqrIn, "KLqrDev": klib.KLqrDev}
    for name, cls in (("KLqrBoxIn", klib.KLqrBoxIn), ("KLqrBoxDev", klib.KLqrBoxDev), ("KFeedbackBoxIn", klib.KFeedbackBoxIn)):
        fields = _fields(hdr, name)
        assert [f for _, _, f in fields] == [n for n, _ in cls._fields_], name
        assert [C.c_void_p if star else ctype[t] for t, star, _ in fields] == [t for _, t in cls._fields_], name
    assert [f for _, _, f in _fields(hdr, "KFeedbackBoxIn")][:14] == [f for _, _, f in _fields(hdr, "KFeedbackIn")]
    assert (klib.KLqrBoxIn.u.offset, klib.KLqrBoxIn.box_per_env.offset, C.sizeof(klib.KLqrBoxIn)) == (80, 104, 112)
    assert (klib.KLqrBoxDev.clamped.offset, C.sizeof(klib.KLqrBoxDev)) == (40, 56)
    assert (klib.KFeedbackBoxIn.lo.offset, C.sizeof(klib.KFeedbackBoxIn)) == (C.sizeof(klib.KFeedbackIn), C.sizeof(klib.KFeedbackIn) + 24)
    assert "KMANIP_API int kmanip_lqr_backward_box(KHandle h, const KLqrBoxIn* in, int n, int T, const KLqrBoxDev* out, void* stream);" in hdr
    assert ("KMANIP_API int kmanip_feedback_box(KHandle h, const KFeedbackBoxIn* in, int n, int nstep, int nsub, const KFeedbackDev* out, "
            "void* stream);") in hdr
    assert "kmanip_lqr_backward_box" in klib.EXPORTS and "kmanip_feedback_box" in klib.EXPORTS
    L = klib.load()
    vp = C.c_void_p
    assert L.kmanip_lqr_backward_box.argtypes == [vp, C.POINTER(klib.KLqrBoxIn), C.c_int, C.c_int, C.POINTER(klib.KLqrBoxDev), vp]
    assert L.kmanip_feedback_box.argtypes == [vp, C.POINTER(klib.KFeedbackBoxIn), C.c_int, C.c_int, C.c_int, C.POINTER(klib.KFeedbackDev), vp]
    assert set(env_hip.KManipEnvHip._LQR_BOX_FIELDS) == {n for n, _ in klib.KLqrDev._fields_} | {"clamped", "qp_iters"}


def test_every_compiled_boxfb_object_has_a_parity_row(tmp_path):
    """The guard of tests/test_feedback_cpu.py for the kmanip_boxfb_* objects: each runs a row of tests/test_feedback_box_gpu.py's
    PARITY_ROWS, and the guard fails for a variant without one."""
    from test_feedback_box_gpu import PARITY_ROWS
    from test_feedback_cpu import covered
    missing = lambda makefile, rows: [tuple(o[1:]) for o in BM.objects(makefile, "boxfb") if tuple(o[1:]) not in covered(rows)]
    assert missing(BM.MAKEFILE, PARITY_ROWS) == []
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    assert sorted(missing(more, PARITY_ROWS)) == [(30, 64, s, ep, frc) for s in (0, 1) for ep in (False, True) for frc in (False, True)]
    assert (10, 16, 0, False, True) in missing(BM.MAKEFILE, [r for r in PARITY_ROWS if not (r[1] == "pgs" and "forced" in r[2])])


# ------------------------------------------------------------------------------------------------------ the loop over the stand-in
def test_ilqr_with_a_box_over_the_stand_in():
    """ilqr(ctrl_lo, ctrl_hi) on KManipSoloArmQPos's contact-free cell, 2 envs, horizon 3, 2 iterations, a box of half-width 0.02 about
    the initial ctrl (the unconstrained plan moves ctrl by more than 0.05): every ctrl applied lies inside the box, the box binds
    (the last pass has clamped actuators, some applied ctrl sits on a bound), the accepted cost never increases and falls in the
    first iteration, with torch's pass and with the stand-in's lqr_backward_box (device_backward).  Without a
    box the result is today's bit for bit: no box call is made and the stand-in's unboxed path is the parent's."""
    import torch
    from gym_kmanip_amd import ilqr
    from test_lqr_backward_cpu import _problem
    cm, cost, p = _problem(n=2, T=3)
    free = ilqr.ilqr(BQ.OracleLqrBox(cm, 2), cost=cost, iters=2, alphas=(1.0, 0.5, 0.25), **p)
    plain = ilqr.ilqr(RR.OracleLqr(cm, 2), cost=cost, iters=2, alphas=(1.0, 0.5, 0.25), **p)
    assert set(free) == set(plain) and all(torch.equal(free[name], plain[name]) for name in free)
    assert float((free["ctrl"] - p["ctrl"]).abs().max()) > 0.05
    lo, hi = p["ctrl"][0, 0] - 0.02, p["ctrl"][0, 0] + 0.02
    res = {}
    for device_backward in (False, True):
        env = BQ.OracleLqrBox(cm, 2)
        r = res[device_backward] = ilqr.ilqr(env, cost=cost, iters=2, alphas=(1.0, 0.5, 0.25), **p, ctrl_lo=lo, ctrl_hi=hi,
                                             device_backward=device_backward)
        J = r["cost"].numpy()
        print("\nboxed iLQR over the stand-in (device_backward %s): cost per iteration %s" % (device_backward, J.tolist()))
        assert np.isfinite(J).all() and (np.diff(J, axis=0) <= 0).all() and (J[1] < J[0]).all()
        assert not r["backward_status"].any() and len(env.box_calls) == (2 if device_backward else 0) and len(env.fb_calls) == 2
        for fb in env.fb_calls:
            assert fb["ctrl"] is not None
        assert bool(((r["ctrl"] >= lo) & (r["ctrl"] <= hi)).all())
        assert bool(((r["ctrl"] == lo) | (r["ctrl"] == hi)).any()) and bool(r["clamped"].any())
    print("the two boxed plans differ by %.3e (accept decisions are discrete: no bar)" % float((res[True]["ctrl"] - res[False]["ctrl"]).abs().max()))
