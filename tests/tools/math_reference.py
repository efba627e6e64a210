"""The 50-digit reference of the kernels' FP64 math and quaternion helpers and the inputs they are held to.

    python tests/tools/math_reference.py        writes tests/golden/math_edges.npz

The fixture holds, per input SET (sincos, atan2, scalar, norm3, norm4, axang, mat2quat, quatpair):
    <set>_in    float64 [n, columns]   the arguments, one row per call
    <set>_tag   uint8 [n]              which edge the row was built for, an index into <set>_tags; the last tag, "random", is
                                       the seeded random half of the set (as many rows as the edges)
and per FUNCTION (FN_SET: the set it reads; lib.MATH_FNS: its columns)
    <fn>_hi     float64 [n, results]   the reference rounded to double
    <fn>_lo     float32 [n, results]   (reference - hi) in spacings of the doubles at |hi|, within +-1/2: a double-double tail, enough
                                       to read an error off to 2^-24 ulp
computed with mpmath at 50 digits FROM THE ROWS' DOUBLES, so that the test on the device needs neither mpmath nor a long double.
A reference states the helper's own semantics (the MJ_MINVAL test of mju_normalize3, the wrap of mju_subQuat, mat2quat's case by
the same comparisons), in exact arithmetic; rows where a comparison would fall differently in exact and in double arithmetic are not
generated (asserted below), except the wrap at an angle of pi, whose rows carry both answers (<fn>_alt_*).

The module also restates each helper in NumPy float64 (np_*): the host-side measurement that fixes the device's bar (10 x its
worst error), and reads the errors (err_units)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "math_edges.npz")
SEED = 20260
MINVAL2 = 1e-15 * 1e-15            # MJ_MINVAL * MJ_MINVAL as the device evaluates it (one rounded product)
TAN_PI_8 = 4.14213562373095048802e-01
SINCOS_MAX = 131072.0              # the domain kmanip_math.hpp states for km_sincos: |x| <= 2^17
ATAN2_MIN, ATAN2_MAX = 1e-300, 1e300   # ... for km_atan2: max(|y|, |x|) in this range, or both zero
HALF_SWITCH = 6e-8                 # coop_eval: below this half angle the mjd_subQuat coefficient is taken as 0

FN_SET = {"km_sincos": "sincos", "km_atan2": "atan2", "km_sqrt": "scalar", "km_rcp": "scalar", "frcp": "scalar", "rsqrt_nr": "scalar",
          "normalize3_fast": "norm3", "normalize4_fast": "norm4", "axis_angle2quat": "axang", "mat2quat": "mat2quat",
          "sub_quat": "quatpair", "sub_quat_sc": "quatpair", "quat_log_diff": "quatpair"}
# the powers k of the angles 1.2e-7 (1 +- 2^-k) on both sides of the switch (thetas(); tests/tools/subquat_jac.py sweeps the same list)
SWITCH_K = (4, 8, 16, 24, 32, 40, 50, 52)


def thetas():
    """[(tag, theta)] of the rotation sweep: qa = qb (x) exp(theta n / 2)."""
    pi = float(np.pi)
    out = [("zero", 0.0), ("tiny", 1e-300), ("underflow", 1e-160), ("tiny", 1e-16), ("small", 1e-8)]
    out += [("switch_below", 2 * HALF_SWITCH * (1 - 2.0 ** -k)) for k in SWITCH_K]
    out += [("switch_above", 2 * HALF_SWITCH * (1 + 2.0 ** -k)) for k in SWITCH_K]
    out += [("mid", 1e-3), ("mid", 1.0), ("below_pi", pi - 1e-8), ("pi", pi), ("wrap", pi + 1e-8), ("wrap", 2 * pi - 1e-8)]
    return out


# ------------------------------------------------------------------------------------------------------------ reading errors
def err_units(got, hi, lo, unit):
    """(got - reference) / unit, elementwise: got - hi is exact wherever the two are within a factor of two (and huge otherwise)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.abs((np.asarray(got, np.float64) - hi) - lo.astype(np.float64) * np.spacing(np.abs(hi))) / unit


def ulp_of(hi):
    """The spacing of the doubles at |hi| (tools/libm_check.hip's unit)."""
    return np.spacing(np.abs(hi))


def quat_units(fx, fn, got):
    """The bar of the quaternion helpers, per row: the worst |got - reference| over the row's components in units of 2^-53 * scale;
    scale is 1 for the components of unit vectors and quaternions (and sin, |cos| of the half angle), max(|r|, 1) for a log map r,
    the value itself for the norm normalize3_fast returns.  A row at an angle of pi passes on either branch of the wrap."""
    hi, lo = fx[fn + "_hi"], fx[fn + "_lo"]
    scale = np.ones_like(hi)
    if fn in ("sub_quat", "sub_quat_sc", "quat_log_diff"):
        scale[:, :3] = np.maximum(np.sqrt((hi[:, :3] ** 2).sum(1)), 1.0)[:, None]
    if fn == "normalize3_fast":
        scale[:, 3] = np.where(hi[:, 3] > 0, hi[:, 3], 2.0 ** -1021)        # (a zero norm is returned exactly)
    u = np.nan_to_num(err_units(got, hi, lo, 2.0 ** -53 * scale), nan=np.inf).max(1)
    if fn + "_alt_rows" in fx:
        at = fx[fn + "_alt_rows"]
        ua = np.nan_to_num(err_units(np.asarray(got)[at], fx[fn + "_alt_hi"], fx[fn + "_alt_lo"], 2.0 ** -53 * scale[at]), nan=np.inf).max(1)
        u[at] = np.minimum(u[at], ua)
    return u


# what the NumPy float64 restatements below measure with quat_units over the whole fixture (tests/test_math_cpu.py asserts they still
# do); the device's bar is 10 x these
C_HOST = {"normalize3_fast": 1.62, "normalize4_fast": 1.43, "axis_angle2quat": 0.90, "mat2quat": 1.85, "sub_quat": 6.10, "sub_quat_sc": 6.10,
          "quat_log_diff": 6.65}
C_DEVICE = {fn: 10.0 * c for fn, c in C_HOST.items()}


def scalar_figures(fx, fn, got):
    """[(what, figure, bar)] of km_sincos / km_atan2 / km_sqrt / km_rcp / frcp / rsqrt_nr on their set: a figure passes below its bar
    (at a bar of 0: when it is 0); bar None = reported only.  The bars are tools/libm_check.hip's exit criteria (4 ulp; 2 for the
    square root, the reciprocals with it), an ulp being the spacing of the doubles at the reference."""
    sname = FN_SET[fn]
    x, hi, lo = fx[sname + "_in"], fx[fn + "_hi"], fx[fn + "_lo"]
    got = np.asarray(got, np.float64).reshape(hi.shape)
    worst = lambda e, m: float(np.nan_to_num(e[m], nan=np.inf).max()) if m.any() else 0.0
    rel = err_units(got, hi, lo, ulp_of(hi))
    if fn == "km_sincos":
        small = np.abs(x[:, 0]) <= float(np.pi) / 4           # the reduction index is 0
        ab = err_units(got, hi, lo, 2.0 ** -53)
        return [("sin, |x| <= pi/4: relative error in ulp", worst(rel[:, 0], small), 4.0), ("cos, |x| <= pi/4: relative error in ulp", worst(rel[:, 1], small), 4.0),
                ("sin elsewhere: absolute error in 2^-53", worst(ab[:, 0], ~small), 4.0), ("cos elsewhere: absolute error in 2^-53", worst(ab[:, 1], ~small), 4.0),
                ("sin elsewhere: relative error in ulp", worst(rel[:, 0], ~small), None), ("cos elsewhere: relative error in ulp", worst(rel[:, 1], ~small), None)]
    if fn == "km_atan2":
        return [("relative error in ulp, %s" % t, worst(rel[:, 0], tag_mask(fx, sname, t)), 4.0) for t in fx[sname + "_tags"]]
    dom = ~tag_mask(fx, sname, "special") & (np.ones(len(x), bool) if fn in ("km_rcp", "frcp") else ~tag_mask(fx, sname, "negative"))
    out = [("relative error in ulp", worst(rel[:, 0], dom), 2.0)]
    if fn == "km_sqrt":
        zero = x[:, 0] <= 0
        out += [("perfect squares: error in ulp", worst(rel[:, 0], tag_mask(fx, sname, "perfect_square")), 0.0),
                ("|result| at 0, -0 and negative arguments", worst(np.abs(got[:, 0]), zero), 0.0),
                ("subnormal arguments (outside the domain): relative error in ulp", worst(rel[:, 0], tag_mask(fx, sname, "special") & ~zero), None)]
    return out


def report(title, figures):
    """Prints every figure, then returns the ones that miss their bar."""
    for what, v, bar in figures:
        print("%s: %s %.4g%s" % (title, what, v, "" if bar is None else " (bar %g)" % bar))
    return [(what, v, bar) for what, v, bar in figures if bar is not None and not (v == 0 if bar == 0 else v < bar)]


# ------------------------------------------------------------------------------------------------ NumPy float64 restatements
def np_normalize3(v):
    v = np.array(v, np.float64)
    s = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    n = np.sqrt(s)
    small = s < MINVAL2
    with np.errstate(invalid="ignore", divide="ignore"):
        u = v / n[:, None]
    u[small] = (1.0, 0.0, 0.0)
    return np.concatenate([u, n[:, None]], 1)


def np_normalize4(q):
    q = np.array(q, np.float64)
    s = (q * q).sum(1)
    small = s < MINVAL2
    with np.errstate(invalid="ignore", divide="ignore"):
        u = q / np.sqrt(s)[:, None]
    u[small] = (1.0, 0.0, 0.0, 0.0)
    return u


def np_axis_angle(a):
    a = np.asarray(a, np.float64)
    h = 0.5 * a[:, 3]
    q = np.concatenate([np.cos(h)[:, None], a[:, :3] * np.sin(h)[:, None]], 1)
    q[a[:, 3] == 0] = (1.0, 0.0, 0.0, 0.0)
    return q


def mat2quat_case(m):
    """The case mat2quat takes, by its own comparisons in double arithmetic; m [n, 9]."""
    m = np.asarray(m, np.float64)
    tr = m[:, 0] + m[:, 4] + m[:, 8]
    return np.where(tr > 0, 0, np.where((m[:, 0] > m[:, 4]) & (m[:, 0] > m[:, 8]), 1, np.where(m[:, 4] > m[:, 8], 2, 3)))


def np_mat2quat(m):
    """mju_mat2Quat as MuJoCo writes it (one square root per case, divisions), then mju_normalize4."""
    m = np.asarray(m, np.float64)
    cs = mat2quat_case(m)
    q = np.zeros((len(m), 4))
    for i, (c, r) in enumerate(zip(cs, m)):
        if c == 0:
            q0 = 0.5 * np.sqrt(1 + r[0] + r[4] + r[8]); k = 0.25 / q0
            q[i] = (q0, k * (r[7] - r[5]), k * (r[2] - r[6]), k * (r[3] - r[1]))
        elif c == 1:
            q1 = 0.5 * np.sqrt(1 + r[0] - r[4] - r[8]); k = 0.25 / q1
            q[i] = (k * (r[7] - r[5]), q1, k * (r[1] + r[3]), k * (r[2] + r[6]))
        elif c == 2:
            q2 = 0.5 * np.sqrt(1 - r[0] + r[4] - r[8]); k = 0.25 / q2
            q[i] = (k * (r[2] - r[6]), k * (r[1] + r[3]), q2, k * (r[5] + r[7]))
        else:
            q3 = 0.5 * np.sqrt(1 - r[0] - r[4] + r[8]); k = 0.25 / q3
            q[i] = (k * (r[3] - r[1]), k * (r[2] + r[6]), k * (r[5] + r[7]), q3)
    return np_normalize4(q)


def np_qmul(a, b):
    w = a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2] - a[:, 3] * b[:, 3]
    x = a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2]
    y = a[:, 0] * b[:, 2] - a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1]
    z = a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1] + a[:, 3] * b[:, 0]
    return np.stack([w, x, y, z], 1)


def np_sub_quat_sc(p):
    """mju_subQuat(qa = p[:, :4], qb = p[:, 4:]) and sin, |cos| of half the angle: [n, 5]."""
    p = np.asarray(p, np.float64)
    qd = np_qmul(p[:, 4:] * np.array([1.0, -1.0, -1.0, -1.0]), p[:, :4])
    u = np_normalize3(qd[:, 1:])
    speed = 2 * np.arctan2(u[:, 3], qd[:, 0])
    speed = np.where(speed > np.pi, speed - 2 * np.pi, speed)
    return np.concatenate([u[:, :3] * speed[:, None], u[:, 3:4], np.abs(qd[:, 0:1])], 1)


def np_quat_log_diff(p):
    """derivatives.tangent_diff's rotation part: the body-frame log of conj(a = p[:, :4]) (x) (b = p[:, 4:])."""
    p = np.asarray(p, np.float64)
    qd = np_qmul(p[:, :4] * np.array([1.0, -1.0, -1.0, -1.0]), p[:, 4:])
    s = np.sqrt((qd[:, 1:] ** 2).sum(1))
    ang = 2 * np.arctan2(s, qd[:, 0])
    ang = np.where(ang > np.pi, ang - 2 * np.pi, ang)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(s > 0, ang / s, 2.0 / np.where(qd[:, 0] != 0, qd[:, 0], 1.0))
    return qd[:, 1:] * k[:, None]


def np_quat2mat(q):
    w, x, y, z = (np.asarray(q, np.float64)[..., i] for i in range(4))
    return np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)


NP_FN = {"normalize3_fast": np_normalize3, "normalize4_fast": np_normalize4, "axis_angle2quat": np_axis_angle, "mat2quat": np_mat2quat,
         "sub_quat": lambda p: np_sub_quat_sc(p)[:, :3], "sub_quat_sc": np_sub_quat_sc, "quat_log_diff": np_quat_log_diff}


# -------------------------------------------------------------------------------------------------------------- the inputs
def _steps(x, k):
    """The double k ulps from x (k of either sign)."""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


# The inputs are built from Generator.uniform / integers / choice, IEEE operations (+ - * / sqrt) and mpmath only -- no libm or SIMD
# sin / cos / pow, whose last bit differs between machines: the committed file is reproducible to the byte.
def _unit(rng, n, d):
    """n seeded unit vectors: uniform draws from the cube, kept inside the ball (and off its centre), normalised."""
    out = []
    while len(out) < n:
        v = rng.uniform(-1.0, 1.0, d)
        s = float((v * v).sum())
        if 0.01 < s <= 1.0:
            out.append(v / np.sqrt(s))
    return np.array(out).reshape(n, d)


def _pow(mp, base, e):
    """base ** e elementwise, correctly rounded."""
    return np.array([float(mp.power(base, mp.mpf(float(v)))) for v in np.ravel(e)]).reshape(np.shape(e))


class _Set:
    def __init__(self):
        self.rows, self.tags, self.names = [], [], []

    def add(self, tag, rows):
        rows = np.atleast_2d(np.asarray(rows, np.float64))
        if tag not in self.names:
            self.names.append(tag)
        self.rows.append(rows)
        self.tags += [self.names.index(tag)] * len(rows)

    def n(self):
        return len(self.tags)

    def done(self):
        return np.concatenate(self.rows, 0), np.asarray(self.tags, np.uint8), np.asarray(self.names)


def _sincos_inputs(mp, rng):
    S = _Set()
    near = lambda k: float(mp.mpf(k) * mp.pi / 2)
    ks = list(range(-64, 65))
    S.add("kpi2_small", [[_steps(near(k), d)] for k in ks for d in range(-3, 4)])
    big = rng.integers(65, 64001, 120) * rng.choice([-1, 1], 120)
    S.add("kpi2_large", [[_steps(near(int(k)), d)] for k in big for d in range(-3, 4)])
    S.add("kpi2_large", [[-92133.487751827866]])           # the worst relative error a host emulation found
    S.add("tie", [[_steps(float((mp.mpf(k) + mp.mpf(1) / 2) * mp.pi / 2), d)] for k in ks for d in (-1, 0, 1)])
    S.add("zero", [[0.0], [-0.0]])
    tiny = [2.0 ** -1074, 2.0 ** -1060, 2.0 ** -1023, 2.0 ** -1022] + [2.0 ** -e for e in range(20, 1021, 20)]
    S.add("tiny", [[s * t] for t in tiny for s in (1.0, -1.0)])
    top = int(mp.floor(mp.mpf(SINCOS_MAX) / (mp.pi / 2)))
    S.add("domain_end", [[s * _steps(SINCOS_MAX, -d)] for d in range(4) for s in (1.0, -1.0)])
    S.add("domain_end", [[s * _steps(near(top - j), d)] for j in range(4) for d in range(-3, 4) for s in (1.0, -1.0)])
    n = S.n()
    q = float(np.pi) / 4                                   # a third each: the reduction index 0, a few turns, the whole 1e5
    S.add("random", np.concatenate([rng.uniform(-q, q, n // 3), rng.uniform(-7, 7, n // 3), rng.uniform(-1e5, 1e5, n - 2 * (n // 3))])[:, None])
    return S


def _atan2_inputs(mp, rng):
    S = _Set()
    signs = [(sy, sx) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]
    for e in range(-20, 20):                                # 40 binades of the larger magnitude
        mx = float(rng.uniform(1.0, 2.0)) * 2.0 ** e
        for name, mn0 in (("diagonal", mx), ("seam", TAN_PI_8 * mx)):
            for d in (-4, -2, -1, 0, 1, 2, 4):
                mn = _steps(mn0, d)
                for sy, sx in signs:                        # the four quadrants, the smaller magnitude in y and in x: eight octants
                    S.add(name, [[sy * mn, sx * mx], [sy * mx, sx * mn]])
    mags = [1e-300, 1e-150, 1e-8, 0.3, 1.0, 7.0, 1e5, 1e150, 1e300]
    S.add("one_zero", [[s * m, 0.0] for m in mags for s in (1.0, -1.0)] + [[0.0, s * m] for m in mags for s in (1.0, -1.0)])
    S.add("ratio_1e-300", [[sy * 1e-300 * m, sx * m] for m in (1e-8, 1.0, 1e5) for sy, sx in signs]
          + [[sy * m, sx * 1e-300 * m] for m in (1e-8, 1.0, 1e5) for sy, sx in signs])
    S.add("signed_zero", [[0.0, -1.0], [-0.0, -1.0], [0.0, 0.0], [0.0, 1.0], [-0.0, 1.0]])
    for m in (ATAN2_MIN, ATAN2_MAX):                        # both ends of the stated domain, every branch
        for mn in (0.0, 1e-3 * m, _steps(TAN_PI_8 * m, -2), _steps(TAN_PI_8 * m, 2), 0.9 * m, m):
            S.add("domain_end", [[sy * mn, sx * m] for sy, sx in signs] + [[sy * m, sx * mn] for sy, sx in signs])
    n = S.n()
    r = np.stack([rng.uniform(-7, 7, n), rng.uniform(-7, 7, n)], 1)
    r[::2] *= _pow(mp, 10, rng.uniform(-8, 0, (len(r[::2]), 2)))  # tools/libm_check.hip's mix: plain and tiny magnitudes
    S.add("random", r)
    return S


def _scalar_inputs(mp, rng):
    S = _Set()
    for e in range(-300, 301, 3):
        p = 2.0 ** e
        S.add("power_of_two", [[p], [_steps(p, 1)], [_steps(p, -1)]])
        S.add("binade", [[p * float(rng.uniform(1.0, 2.0))], [p * float(rng.uniform(1.0, 2.0))]])
    sq = [float(i * i) for i in range(1, 129)] + [float(i * i) * 4.0 ** int(k) for i, k in zip(rng.integers(3, 2 ** 26, 128), rng.integers(-140, 120, 128))]
    S.add("perfect_square", [[v] for v in sq])
    S.add("negative", [[-float(v)] for v in _pow(mp, 2, rng.uniform(-300, 300, 64))])      # km_rcp, frcp only
    S.add("special", [[0.0], [-0.0], [-1.5], [2.0 ** -1074], [1e-310]])              # km_sqrt only: 0, 0, 0 and whatever a subnormal gives
    n = S.n()
    S.add("random", _pow(mp, 2, rng.uniform(-300, 300, n))[:, None])
    return S


def _norm_inputs(mp, rng, d):
    S = _Set()
    u = _unit(rng, 64, d)
    for k, row in zip(list(range(4, 36)) * 2, u):
        S.add("below_minval", [row * np.sqrt(MINVAL2 * (1 - 2.0 ** -k))])
    for k, row in zip(list(range(4, 36)) * 2, _unit(rng, 64, d)):
        S.add("above_minval", [row * np.sqrt(MINVAL2 * (1 + 2.0 ** -k))])
    S.add("below_minval", [np.zeros(d)] + [row * float("1e-%d" % e) for row, e in zip(_unit(rng, 15, d), range(20, 140, 8))])
    S.add("scale", [row * e for row, e in zip(_unit(rng, 32, d), _pow(mp, 10, np.arange(32) * 0.75 - 12))])
    S.add("unit", _unit(rng, 32, d))
    S.add("axis", np.eye(d)[np.arange(16) % d] * rng.choice([-1.0, 1.0], 16)[:, None] * _pow(mp, 10, rng.uniform(-3, 3, 16))[:, None])
    n = S.n()
    S.add("random", _unit(rng, n, d) * _pow(mp, 10, rng.uniform(-6, 6, n))[:, None])
    return S


def _axang_inputs(mp, rng):
    S = _Set()
    for name, a in (("zero", 0.0), ("tiny", 1e-300), ("dt_w", 0.06), ("pi", float(np.pi)), ("large", 4e4)):
        S.add(name, np.concatenate([_unit(rng, 16, 3), np.full((16, 1), a)], 1))
        if a:
            S.add(name, np.concatenate([_unit(rng, 16, 3), np.full((16, 1), -a)], 1))
    n = S.n()
    S.add("random", np.concatenate([_unit(rng, n, 3), rng.uniform(-7, 7, (n, 1))], 1))
    return S


def _rot_np(mp, axis, angle):
    """The rotation matrix of a unit axis and an angle in float64 (through the quaternion: orthonormal to rounding only)."""
    axis = np.asarray(axis, np.float64)
    h = mp.mpf(float(angle)) / 2
    return np_quat2mat(np.concatenate([[float(mp.cos(h))], float(mp.sin(h)) * axis]))


def _mat2quat_inputs(mp, rng):
    S = _Set()
    S.add("case0", [_rot_np(mp, a, t) for a, t in zip(_unit(rng, 24, 3), rng.uniform(-1.8, 1.8, 24))])
    for c in (1, 2, 3):                                     # a large angle about an axis near x / y / z
        ax = _unit(rng, 24, 3) * 0.3
        ax[:, c - 1] = 1.0
        ax /= np.sqrt((ax * ax).sum(1))[:, None]
        S.add("case%d" % c, [_rot_np(mp, a, t) for a, t in zip(ax, rng.uniform(2.4, 3.1, 24))])
    th0 = 2 * float(np.pi) / 3                              # the trace 1 + 2 cos(angle) changes sign at 2 pi / 3
    for name, sg in (("trace_positive", -1.0), ("trace_negative", 1.0)):
        S.add(name, [_rot_np(mp, a, th0 + sg * d) for d in (1e-3, 1e-6, 1e-9, 1e-12) for a in _unit(rng, 6, 3)])
    for name, (i, j, k) in (("tie_m0_m4", (0, 1, 2)), ("tie_m0_m8", (0, 2, 1)), ("tie_m4_m8", (1, 2, 0))):
        for t in range(24):                                 # axis components i and j equal: the two diagonal entries tie; forced to the bit
            a, c = rng.uniform(0.2, 0.9), rng.uniform(-0.9, 0.9)
            ax = np.zeros(3); ax[i] = a; ax[j] = a; ax[k] = c
            m = _rot_np(mp, ax / np.sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), rng.uniform(2.2, 3.1))
            m[4 * j] = m[4 * i]
            S.add(name, [m])
    S.add("pi_exact", [np.diag(d).ravel() for d in ([1.0, -1, -1], [-1.0, 1, -1], [-1.0, -1, 1])])
    S.add("pi_exact", [(2 * np.outer(a, a) - np.eye(3)).ravel() for a in _unit(rng, 21, 3)])
    S.add("pi_minus_1e-8", [_rot_np(mp, a, float(np.pi) - 1e-8) for a in list(np.eye(3)) + list(_unit(rng, 21, 3))])
    chain = []
    for _ in range(32):                                     # the product of a 10-link chain's joint rotations, as FK forms it
        m = np.eye(3)
        for a, t in zip(_unit(rng, 10, 3), rng.uniform(-2.5, 2.5, 10)):
            r = _rot_np(mp, a, t).reshape(3, 3)
            m = np.array([[m[i, 0] * r[0, j] + m[i, 1] * r[1, j] + m[i, 2] * r[2, j] for j in range(3)] for i in range(3)])   # (no BLAS: its summation order is the machine's)
        chain.append(m.ravel())
    S.add("chain10", chain)
    n = S.n()
    S.add("random", [np_quat2mat(q) for q in _unit(rng, n, 4)])
    return S


def quat_exp_mul(mp, qb, axis, theta):
    """qb (x) exp(theta axis / 2) at working precision, rounded to doubles."""
    h = mp.mpf(theta) / 2
    e = [mp.cos(h)] + [mp.sin(h) * mp.mpf(float(a)) for a in axis]
    b = [mp.mpf(float(v)) for v in qb]
    return np.array([float(v) for v in _qmul_mp(b, e)])


EXACT_QB = [np.eye(4)[i] * s for i in range(4) for s in (1.0, -1.0)]    # products with these are exact: a tiny angle survives the rounding of qa


def _quatpair_inputs(mp, rng):
    S = _Set()
    for tag, th in thetas():
        for t in range(24):
            n = _unit(rng, 1, 3)[0]
            qb = EXACT_QB[t % 8] if th < 1e-6 else _unit(rng, 1, 4)[0]
            S.add(tag, [np.concatenate([quat_exp_mul(mp, qb, n, th), qb])])
    qb = _unit(rng, 16, 4)
    S.add("antipodal", np.concatenate([-qb, qb], 1))
    qb = _unit(rng, 16, 4)
    S.add("equal", np.concatenate([qb, qb], 1))
    n = S.n()
    S.add("random", np.concatenate([_unit(rng, n, 4), _unit(rng, n, 4)], 1))
    return S


# ---------------------------------------------------------------------------------------------------------- the references
def _qmul_mp(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def _normalize_mp(mp, v):
    """(unit vector, norm) with mju_normalize's MJ_MINVAL rule; the comparison must fall the same way in double arithmetic."""
    s = sum(x * x for x in v)
    sd = float(s)
    assert abs(sd - MINVAL2) > 1e-12 * MINVAL2 or sd == 0, "a row sits on the MJ_MINVAL threshold to rounding"
    n = mp.sqrt(s)
    if s < mp.mpf(MINVAL2):
        return [mp.mpf(1)] + [mp.mpf(0)] * (len(v) - 1), n
    return [x / n for x in v], n


def _log_mp(mp, w, vec, minval_rule):
    """The wrapped body-frame log of the quaternion (w, vec), and its other branch where the angle is pi to 1e-12 (else None).
    minval_rule: mju_subQuat's axis (mju_normalize3: (1, 0, 0) below MJ_MINVAL); without it the limit 2 vec / w (quat_log_diff)."""
    if minval_rule:
        ax, sn = _normalize_mp(mp, vec)
    else:
        sn = mp.sqrt(sum(x * x for x in vec))
        if sn == 0:
            return [2 * x / (w if w != 0 else 1) for x in vec], None, sn
        ax = [x / sn for x in vec]
    speed = 2 * mp.atan2(sn, w)
    other = None
    if abs(speed - mp.pi) < mp.mpf(10) ** -12:
        other = speed - 2 * mp.pi if speed <= mp.pi else speed
    if speed > mp.pi:
        speed -= 2 * mp.pi
    return [a * speed for a in ax], (None if other is None else [a * other for a in ax]), sn


def _reference_rows(mp, fn, rows):
    """[n][results] mpf (and [n][results] of the other branch at the wrap, or None) of function fn on the rows' doubles."""
    F = mp.mpf
    out, alt = [], []
    for row in rows:
        a = [F(float(v)) for v in row]
        o = None
        if fn == "km_sincos":
            r = [mp.sin(a[0]), mp.cos(a[0])]
        elif fn == "km_atan2":
            r = [mp.atan2(a[0], a[1]) if (a[0] != 0 or a[1] != 0) else F(0)]
            if a[0] == 0 and a[1] < 0:
                r = [+mp.pi]                              # (-pi, pi]: y = -0 is 0
        elif fn == "km_sqrt":
            r = [mp.sqrt(a[0]) if a[0] > 0 else F(0)]
        elif fn in ("km_rcp", "frcp"):
            r = [1 / a[0] if a[0] != 0 else F(0)]
        elif fn == "rsqrt_nr":
            r = [1 / mp.sqrt(a[0]) if a[0] > 0 else F(0)]
        elif fn == "normalize3_fast":
            u, n = _normalize_mp(mp, a)
            r = u + [n]
        elif fn == "normalize4_fast":
            r = _normalize_mp(mp, a)[0]
        elif fn == "axis_angle2quat":
            h = a[3] / 2
            r = [mp.cos(h)] + [x * mp.sin(h) for x in a[:3]]
        elif fn == "mat2quat":
            cs = int(mat2quat_case(np.asarray(row)[None])[0])
            tr = a[0] + a[4] + a[8]
            exact = 0 if tr > 0 else (1 if (a[0] > a[4] and a[0] > a[8]) else (2 if a[4] > a[8] else 3))
            assert cs == exact, "mat2quat's case differs between double and exact arithmetic on a fixture row"
            arg = 1 + [tr, a[0] - a[4] - a[8], -a[0] + a[4] - a[8], -a[0] - a[4] + a[8]][cs]
            q = mp.sqrt(arg) / 2
            s = 1 / (4 * q)
            d75, d26, d31 = s * (a[7] - a[5]), s * (a[2] - a[6]), s * (a[3] - a[1])
            s13, s26, s57 = s * (a[1] + a[3]), s * (a[2] + a[6]), s * (a[5] + a[7])
            r = _normalize_mp(mp, [[q, d75, d26, d31], [d75, q, s13, s26], [d26, s13, q, s57], [d31, s26, s57, q]][cs])[0]
        elif fn in ("sub_quat", "sub_quat_sc"):
            qd = _qmul_mp([a[4], -a[5], -a[6], -a[7]], a[:4])
            r, o, sn = _log_mp(mp, qd[0], qd[1:], True)
            if fn == "sub_quat_sc":
                r = r + [sn, abs(qd[0])]
                o = None if o is None else o + [sn, abs(qd[0])]
        elif fn == "quat_log_diff":
            qd = _qmul_mp([a[0], -a[1], -a[2], -a[3]], a[4:])
            r, o, _ = _log_mp(mp, qd[0], qd[1:], False)
        else:
            raise KeyError(fn)
        out.append(r)
        alt.append(o)
    return out, alt


def _split(mp, vals):
    hi = np.array([[float(v) for v in r] for r in vals], np.float64).reshape(len(vals), -1)
    sp = np.spacing(np.abs(hi))
    lo = np.array([[float((v - mp.mpf(h)) / mp.mpf(u)) for v, h, u in zip(r, hr, ur)] for r, hr, ur in zip(vals, hi.tolist(), sp.tolist())], np.float64)
    return hi, lo.reshape(hi.shape).astype(np.float32)


def generate():
    """Every array of the fixture, {name: array}: deterministic (seeded inputs, 50-digit arithmetic)."""
    import mpmath
    mp = mpmath.mp
    mp.dps = 50
    makers = {"sincos": _sincos_inputs, "atan2": _atan2_inputs, "scalar": _scalar_inputs, "norm3": lambda m, r: _norm_inputs(m, r, 3),
              "norm4": lambda m, r: _norm_inputs(m, r, 4), "axang": _axang_inputs, "mat2quat": _mat2quat_inputs, "quatpair": _quatpair_inputs}
    # a generator per set: a set that gains a row leaves the others' draws alone
    sets = {name: make(mp, np.random.default_rng([SEED, i])) for i, (name, make) in enumerate(makers.items())}
    out = {}
    for name, S in sets.items():
        rows, tag, names = S.done()
        assert names[-1] == "random" and 2 * (tag == len(names) - 1).sum() == len(tag), name
        out[name + "_in"], out[name + "_tag"], out[name + "_tags"] = rows, tag, names
    for fn, sname in FN_SET.items():
        vals, alt = _reference_rows(mp, fn, out[sname + "_in"])
        out[fn + "_hi"], out[fn + "_lo"] = _split(mp, vals)
        at = [i for i, o in enumerate(alt) if o is not None]
        if fn in ("sub_quat", "sub_quat_sc", "quat_log_diff"):      # the rows at an angle of pi: the wrap's other branch
            out[fn + "_alt_rows"] = np.asarray(at, np.int32)
            out[fn + "_alt_hi"], out[fn + "_alt_lo"] = _split(mp, [alt[i] for i in at])
    return out


def load(path=FIXTURE):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def tag_mask(fx, sname, *tags):
    """The rows of a set that carry one of the tags."""
    names = list(fx[sname + "_tags"])
    return np.isin(fx[sname + "_tag"], [names.index(t) for t in tags])


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(FIXTURE, **arrays)
    print("%s: %d bytes, rows per set %s" % (FIXTURE, os.path.getsize(FIXTURE), {k[:-3]: len(v) for k, v in arrays.items() if k.endswith("_in")}))
    sys.exit(0 if os.path.getsize(FIXTURE) < (1 << 20) else 1)
