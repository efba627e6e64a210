"""The kernels' FP64 math and quaternion helpers on the CPU: the fixture tests/golden/math_edges.npz is what
tests/tools/math_reference.py generates and holds every edge it names; the host twin of kmanip_math.hpp (the header unmodified,
the two hardware estimates replaced by 24-bit seeds; tests/tools/math_twin.cpp) meets the device's bars and runs clean under
-fsanitize=undefined; the NumPy restatements of the quaternion helpers measure what the device's bars are ten times of; SciPy's
Rotation agrees with the references; the probe is declared and bound.  tests/test_math_gpu.py is the device's half."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_kmanip_amd import lib as klib

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import math_reference as MR  # noqa: E402

CSRC = os.path.join(ROOT, "gym_kmanip_amd", "csrc")
TWIN_FNS = {"km_sincos": "sincos", "km_atan2": "atan2", "km_sqrt": "sqrt", "km_rcp": "rcp"}


@pytest.fixture(scope="module")
def fx():
    return MR.load()


def test_fixture_is_what_the_generator_writes(fx):
    pytest.importorskip("mpmath")
    new = MR.generate()
    assert sorted(new) == sorted(fx)
    for k, v in new.items():
        assert v.dtype == fx[k].dtype and v.shape == fx[k].shape, k
        assert np.array_equal(v, fx[k]) if v.dtype.kind in "US" else v.tobytes() == fx[k].tobytes(), k
    assert os.path.getsize(MR.FIXTURE) < (1 << 20)


def test_fixture_holds_every_edge(fx):
    """At least 16 rows of every case of mat2quat, of both sides of every threshold and of all eight octants of km_atan2: a
    regenerated fixture cannot lose an edge unnoticed.  Every set is half edges, half seeded random rows."""
    count = lambda s, *t: int(MR.tag_mask(fx, s, *t).sum())
    edges = ~MR.tag_mask(fx, "mat2quat", "random")
    cases = MR.mat2quat_case(fx["mat2quat_in"][edges])
    assert all((cases == c).sum() >= 16 for c in range(4)), np.bincount(cases)
    for t in ("trace_positive", "trace_negative", "tie_m0_m4", "tie_m0_m8", "tie_m4_m8", "pi_exact", "pi_minus_1e-8", "chain10"):
        assert count("mat2quat", t) >= 16, t
    m = fx["mat2quat_in"]
    tr = m[:, 0] + m[:, 4] + m[:, 8]
    assert (tr[MR.tag_mask(fx, "mat2quat", "trace_positive")] > 0).all() and (tr[MR.tag_mask(fx, "mat2quat", "trace_negative")] < 0).all()
    assert np.abs(tr[MR.tag_mask(fx, "mat2quat", "trace_positive", "trace_negative")]).min() < 1e-11
    for t, (i, j) in (("tie_m0_m4", (0, 4)), ("tie_m0_m8", (0, 8)), ("tie_m4_m8", (4, 8))):
        rows = m[MR.tag_mask(fx, "mat2quat", t)]
        assert (rows[:, i] == rows[:, j]).all() and (tr[MR.tag_mask(fx, "mat2quat", t)] <= 0).all(), t
    # km_atan2: the diagonal and the tan(pi/8) seam, both sides, in every octant
    a = fx["atan2_in"]
    octant = (a[:, 0] < 0) * 4 + (a[:, 1] < 0) * 2 + (np.abs(a[:, 0]) > np.abs(a[:, 1]))
    for t in ("diagonal", "seam"):
        sel = MR.tag_mask(fx, "atan2", t)
        mn, mx = np.minimum(np.abs(a[:, 0]), np.abs(a[:, 1])), np.maximum(np.abs(a[:, 0]), np.abs(a[:, 1]))
        big = mn > MR.TAN_PI_8 * mx                       # km_atan2's own test
        for o in range(8):
            if t == "seam":
                assert (sel & (octant == o) & big).sum() >= 16 and (sel & (octant == o) & ~big).sum() >= 16, (t, o)
        for o in (0, 2, 4, 6):                            # |y| <= |x| on one side of the diagonal, |y| > |x| on the other
            assert (sel & (octant == o)).sum() >= 16 and (sel & (octant == o + 1)).sum() >= 16, (t, o)
        assert len(np.unique(np.frexp(mx[sel])[1])) >= 40, t
    for t in ("one_zero", "ratio_1e-300", "domain_end"):
        assert count("atan2", t) >= 16, t
    assert count("atan2", "signed_zero") == 5
    mxd = np.maximum(np.abs(a[:, 0]), np.abs(a[:, 1]))
    assert ((mxd >= MR.ATAN2_MIN) & (mxd <= MR.ATAN2_MAX) | (mxd == 0)).all() and mxd.min() == 0 and mxd.max() == MR.ATAN2_MAX
    assert (mxd == MR.ATAN2_MIN).sum() >= 16
    # km_sincos
    for t in ("kpi2_small", "kpi2_large", "tie", "tiny", "domain_end"):
        assert count("sincos", t) >= 16, t
    x = fx["sincos_in"][:, 0]
    assert np.abs(x).max() == MR.SINCOS_MAX and (np.abs(x) == 2.0 ** -1074).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    # the MJ_MINVAL^2 threshold of normalize3_fast / normalize4_fast, the quaternion sweep
    for s in ("norm3", "norm4"):
        s2 = (fx[s + "_in"] ** 2).sum(1)
        for t, below in (("below_minval", True), ("above_minval", False)):
            sel = MR.tag_mask(fx, s, t)
            assert sel.sum() >= 16 and ((s2[sel] < MR.MINVAL2) == below).all(), (s, t)
            assert (np.abs(s2[sel] / MR.MINVAL2 - 1) < 1e-9).sum() >= 4, (s, t)
    for t in ("zero", "tiny", "underflow", "small", "switch_below", "switch_above", "mid", "below_pi", "pi", "wrap", "antipodal", "equal"):
        assert count("quatpair", t) >= 16, t
    ang = 2 * np.arctan2(fx["sub_quat_sc_hi"][:, 3], fx["sub_quat_sc_hi"][:, 4])        # the references' own half angles
    for t, below in (("switch_below", True), ("switch_above", False)):
        sel = MR.tag_mask(fx, "quatpair", t)
        assert ((0.5 * ang[sel] < MR.HALF_SWITCH) == below).sum() >= 16 and (np.abs(0.5 * ang[sel] / MR.HALF_SWITCH - 1) < 1e-9).sum() >= 16, t
    assert len(fx["sub_quat_alt_rows"]) >= 16 and MR.tag_mask(fx, "quatpair", "pi")[fx["sub_quat_alt_rows"]].all()
    for t in ("zero", "tiny", "dt_w", "pi", "large"):
        assert count("axang", t) >= 16, t
    for t in ("power_of_two", "binade", "perfect_square", "negative"):
        assert count("scalar", t) >= 16, t
    e = np.frexp(fx["scalar_in"][MR.tag_mask(fx, "scalar", "power_of_two"), 0])[1]
    assert e.min() <= -299 and e.max() >= 300
    for s in MR.FN_SET.values():
        assert 2 * count(s, "random") == len(fx[s + "_tag"]), s


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """The two builds of the host twin: {"plain": path, "ubsan": path}."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("math_twin")
    os.makedirs(d / "shim" / "hip")
    (d / "shim" / "hip" / "hip_runtime.h").write_text("/* the host twin needs nothing of the HIP runtime */\n")
    out = {}
    for name, flags in (("plain", []), ("ubsan", ["-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all"])):
        out[name] = str(d / ("math_twin_" + name))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags
                              + ["-I", str(d / "shim"), "-I", CSRC, os.path.join(ROOT, "tests", "tools", "math_twin.cpp"), "-o", out[name]])
    out["dir"] = d
    return out


def _run_twin(exe, d, fn, rows):
    rows = np.ascontiguousarray(rows, np.float64)
    src, dst = str(d / (fn + ".in")), str(d / (fn + ".out"))
    rows.tofile(src)
    r = subprocess.run([exe, TWIN_FNS[fn], str(len(rows)), src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(dst, np.float64).reshape(len(rows), -1)


@pytest.mark.parametrize("fn", sorted(TWIN_FNS))
def test_host_twin_meets_the_device_bars(fx, twin, fn):
    """Everything of kmanip_math.hpp but the two hardware estimates, held to the bars of the device test over the whole fixture.
    Measured (worst): km_sincos 0.57 / 0.66 ulp inside |x| <= pi/4, 0.90 / 0.92 x 2^-53 elsewhere (relative there: 1781 ulp, next
    to a zero of the sine: not bounded); km_atan2 2.19 ulp; km_sqrt 0.50, perfect squares exact; km_rcp 0.50."""
    got = _run_twin(twin["plain"], twin["dir"], fn, fx[MR.FN_SET[fn] + "_in"])
    assert MR.report("host twin " + fn, MR.scalar_figures(fx, fn, got)) == []


@pytest.mark.parametrize("fn", sorted(TWIN_FNS))
def test_host_twin_under_ubsan(fx, twin, fn):
    """The same program built with -fsanitize=undefined,float-cast-overflow (no recovery) over the in-domain rows -- all of the
    fixture's: the (int)k of km_sincos is in range up to the stated 2^17 -- and the same bytes as the plain build."""
    rows = fx[MR.FN_SET[fn] + "_in"]
    a = _run_twin(twin["ubsan"], twin["dir"], fn, rows)
    b = _run_twin(twin["plain"], twin["dir"], fn, rows)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("fn", sorted(MR.NP_FN))
def test_numpy_restatement_sets_the_device_bar(fx, fn):
    """The host-side restatement of each quaternion helper (IEEE sqrt / divide, libm's atan2 / sincos) against the 50-digit
    reference: C_HOST records its worst error, the device gets ten times that (C_DEVICE)."""
    u = MR.quat_units(fx, fn, MR.NP_FN[fn](fx[MR.FN_SET[fn] + "_in"]))
    print("NumPy %s: worst %.3f x 2^-53 x scale at row %d (recorded %.2f)" % (fn, u.max(), int(u.argmax()), MR.C_HOST[fn]))
    assert 0.5 * MR.C_HOST[fn] <= u.max() <= 1.25 * MR.C_HOST[fn]          # (libm's last bit differs between machines; the recorded figure is this one's)
    assert MR.C_DEVICE[fn] == 10.0 * MR.C_HOST[fn]


def test_references_agree_with_scipy_rotation(fx):
    """The second, independent part of the references (SciPy need not exist next to the GPU, so it runs here): quat2mat of
    mat2quat's reference gives the matrix back and is +-Rotation.from_matrix's quaternion; the log maps are Rotation's rotation
    vectors of the relative rotation; sub_quat_sc's pair satisfies tan(|res| / 2) = sn / ac."""
    R = pytest.importorskip("scipy.spatial.transform").Rotation
    m, q = fx["mat2quat_in"], fx["mat2quat_hi"]
    # the inputs are orthonormal to rounding (1e-15 after a chain of ten products); the pi - 1e-8 rows lose half the digits of the
    # small component in any formula that reads it off the matrix, which is all the matrix holds of it
    assert np.abs(MR.np_quat2mat(q) - m).max() < 1e-14
    qs = R.from_matrix(m.reshape(-1, 3, 3)).as_quat()[:, [3, 0, 1, 2]]
    assert np.minimum(np.abs(qs - q).max(1), np.abs(qs + q).max(1)).max() < 1e-8
    assert np.median(np.minimum(np.abs(qs - q).max(1), np.abs(qs + q).max(1))) < 1e-15
    p = fx["quatpair_in"]
    ok = ~MR.tag_mask(fx, "quatpair", "zero", "tiny", "underflow", "pi", "antipodal", "equal")     # (below MJ_MINVAL mju_subQuat's axis is (1, 0, 0) by rule)
    rel = (R.from_quat(p[:, [5, 6, 7, 4]]).inv() * R.from_quat(p[:, [1, 2, 3, 0]])).as_rotvec()
    assert np.abs(rel - fx["sub_quat_hi"])[ok].max() < 1e-14
    assert np.abs(-rel - fx["quat_log_diff_hi"])[ok].max() < 1e-14
    r5 = fx["sub_quat_sc_hi"]
    half = 0.5 * np.sqrt((r5[:, :3] ** 2).sum(1))
    assert np.abs(np.arctan2(r5[:, 3], r5[:, 4]) - half).max() < 1e-15                # (tan itself is 1e8 at pi - 1e-8, 1e16 at pi)
    assert (fx["quat_log_diff_hi"][MR.tag_mask(fx, "quatpair", "equal")] == 0).all()


def test_probe_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "kmanip_debug.h")).read()
    assert "KMANIP_API int kmanip_dbg_math(KHandle h, int fn, int n, const double* in_dev, int in_cols, double* out_dev, int out_cols, void* stream);" in hdr
    assert "kmanip_dbg_math" in klib.DEBUG_EXPORTS and set(klib.MATH_FNS) == set(MR.FN_SET)
    names = hdr.split("enum {")[1].split("}")[0].replace("= 0", "").replace(",", " ").split()
    order = ["KM_MATH_SINCOS", "KM_MATH_ATAN2", "KM_MATH_SQRT", "KM_MATH_RCP", "KM_MATH_FRCP", "KM_MATH_RSQRT_NR", "KM_MATH_NORMALIZE3", "KM_MATH_NORMALIZE4",
             "KM_MATH_AXIS_ANGLE", "KM_MATH_MAT2QUAT", "KM_MATH_SUB_QUAT", "KM_MATH_SUB_QUAT_SC", "KM_MATH_QUAT_LOG_DIFF", "KM_MATH_NFN"]
    assert names == order
    assert [v[0] for v in klib.MATH_FNS.values()] == list(range(13))
    s = MR.load()
    for fn, (_, ic, oc) in klib.MATH_FNS.items():       # the fixture's columns are the binding's
        assert s[MR.FN_SET[fn] + "_in"].shape[1] == ic and s[fn + "_hi"].shape[1] == oc, fn
    if not os.path.exists(klib.LIB_PATH):
        klib.build()
    L = klib.load()
    assert L.kmanip_dbg_math.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    assert L.kmanip_dbg_math(None, 0, 0, None, 1, None, 2, None) != 0 and b"kmanip_dbg_math: null handle" in L.kmanip_last_error(None)


@pytest.fixture(scope="module")
def oracle_rows():
    """{env: (sweep, res [R, 6 + 2 n], jac [R, 6 + 2 n, n])} of Oracle.ik_res / ik_jac on subquat_jac's sweep, computed once."""
    pytest.importorskip("mpmath")
    import subquat_jac as SJ
    from oracle.oracle import Oracle
    out = {}
    for env in SJ.ENVS:
        sw = SJ.sweep(env)
        o = Oracle(sw["cm"], 1)
        args = [(SJ.ARM, q, q[sw["mask"]], q, gp, gq) for q, gp, gq in zip(sw["qpos"], sw["goal_pos"], sw["goal_quat"])]
        out[env] = (sw, np.array([o.ik_res(*a) for a in args]), np.array([o.ik_jac(*a) for a in args]))
    return out


def test_oracle_orientation_rows_on_the_subquat_sweep(oracle_rows):
    """Rows 3 to 5 of the oracle's ik_res / ik_jac against the 50-digit composition -rad Da(r) (site_xmat^T axis_j) with NumpyArm's
    site frame and axes, over 8 poses x the rotation sweep per asset: the host-side measurement C_HOST_JAC / C_HOST_RES that the
    device's bars are ten times of.  At the `half < 6e-8` switch the coefficient 1 - h / tan h is dropped: the rows below it show
    the whole expected jump (h^2 / 3 <= 1.2e-15) more than the rows above it (subquat_jac.jac_figures: the difference of the two
    shares, so that an offset common to both sides -- a site frame that is orthonormal to a few ulp only -- cancels)."""
    import subquat_jac as SJ
    worst_j, worst_r = 0.0, 0.0
    for env, (sw, res, jac) in oracle_rows.items():
        f = SJ.jac_figures(sw, res, jac)
        e = SJ.res_figures(sw, res)
        print("oracle %s: ik_jac rows 3-5 worst %.2f x 2^-53 rad (%s), ik_res rows 3-5 worst %.2f; below the switch %d rows show %.3f of the jump %.3g, above it %d rows %.3f"
              % (env, f["worst"].max(), sw["tag"][f["worst"].argmax()], e.max(), f["below"], f["share_below"], f["jump"], f["above"], f["share_above"]))
        assert f["below"] >= 16 and f["above"] >= 16
        assert 0.8 < f["share_below"] - f["share_above"] < 1.2
        assert 1.0e-15 < f["jump"] <= 1.2e-15
        worst_j, worst_r = max(worst_j, f["worst"].max()), max(worst_r, e.max())
    assert 0.5 * SJ.C_HOST_JAC <= worst_j <= 1.25 * SJ.C_HOST_JAC and 0.5 * SJ.C_HOST_RES <= worst_r <= 1.25 * SJ.C_HOST_RES


def test_header_constants_are_the_doubles_of_their_definitions():
    """The named constants of kmanip_math.hpp -- 2/pi, the two parts of pi/2, pi/4, pi/2, pi and the tan(pi/8) seam of km_atan2 -- are
    the doubles nearest their 50-digit values.  (A seam off by 1e-9 changes no result by a measurable amount: both branches of
    km_atan2 agree to 1e-18 there, so the bars above cannot see it; this does.)"""
    import re
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    text = open(os.path.join(CSRC, "kmanip_math.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.split("\n"))
    literals = {float(v) for v in re.findall(r"(?<![\w.])\d+\.\d+(?:e[+-]?\d+)?", code)}
    hi = float(mp.pi / 2)
    want = {"2/pi": float(2 / mp.pi), "pi/2 (high part)": hi, "pi/2 (low part)": float(mp.pi / 2 - mp.mpf(hi)), "pi/4": float(mp.pi / 4), "pi": float(mp.pi),
            "tan(pi/8)": float(mp.tan(mp.pi / 8))}
    assert [name for name, v in want.items() if v not in literals] == []
    assert MR.TAN_PI_8 == want["tan(pi/8)"]
