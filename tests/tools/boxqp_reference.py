"""The backward pass of control-limited DDP restated in NumPy: the reference of kmanip_lqr_backward_box and of ilqr.backward_pass_box
(DESIGN.md section 39).  oracle/ and riccati_reference.py stay as they are.

box_qp(...)           ONE box QP, the iteration of include/kmanip.h KLqrBoxIn in the dtype of its arguments (np.float64 or np.longdouble),
                      scalar NumPy with riccati_reference's hand-written Cholesky and triangular solves.  It also returns the three
                      margins of its discrete decisions (see MARGIN).
riccati_box(...)      ONE problem: riccati_reference.riccati with that QP in the solve's place, the device's failure rules.
bvls(...)             the INDEPENDENT solution of a QP, sharing no code with box_qp: scipy.optimize.lsq_linear(method="bvls") on the
                      Cholesky factor of H (0.5 d'H d + q'd = 0.5 |R d + R^-T q|^2 + const for H = R'R).
kkt(...)              the KKT residuals of a candidate d: infeasibility, |g| on the free coordinates, the wrong-signed part of g on
                      the clamped ones, relative to max |q|.
family(...)           THE BOX FAMILY: riccati_reference.family (seed 17) plus, from default_rng(seed + 1000 + attempt), per problem e a
                      base half-width BASE[e % 3] (wide, middling, narrow: nothing clamps / some clamp / everything clamps), per
                      actuator w = base (0.5 + U(0, 1)), a centre c ~ 0.3 N(0, 1), lo = c - w, hi = c + w, and u ~ c + 0.9 w U(-1, 1)
                      per step.  The draw is repeated (attempt 0, 1, ..) until riccati_box in longdouble finds every margin above
                      MARGIN at every step of every problem: the decisions are discrete, and the margin keeps a 1e-12 difference
                      from flipping one.  No case is dropped and none is exempted.
OracleLqrBox          riccati_reference.OracleLqr whose rollout_feedback clamps (ctrl_lo / ctrl_hi) and which offers lqr_backward_box."""
import numpy as np

import riccati_reference as RR

ITERS, TRIALS, ARMIJO, STEP = 100, 100, 0.1, 0.6      # the paper's constants (ilqr.BOXQP_*, kmanip_lqr_box.hip)
MARGIN = 1e-6
BASE = (4.0, 0.4, 0.02)


def box_qp(H, q, bl, bh):
    """(d, c bool [nu], L the factor for c, iters, status, margins): margins = dict(mult: the smallest multiplier |g_i| on a clamped
    coordinate of the result / max |q|; free: the smallest distance of a free coordinate of the result to a bound / the box's width
    there; armijo: the smallest |ratio - 0.1| over all line-search trials) -- inf where there is nothing to measure."""
    dt = H.dtype.type
    nu = len(q)
    marg = dict(mult=np.inf, free=np.inf, armijo=np.inf)
    c = np.zeros(nu, dtype=bool)
    L = np.eye(nu, dtype=H.dtype)
    if not (bl <= bh).all():
        return np.zeros_like(q), c, L, 0, 1, marg
    clip = lambda x: np.where(x < bl, bl, np.where(x > bh, bh, x))
    value = lambda x: x @ (dt(0.5) * (H @ x) + q)
    d = clip(np.zeros_like(q))
    v = value(d)
    moved, cf, it, status, g = True, None, 0, 0, q
    with np.errstate(all="ignore"):
        while True:
            g = q + H @ d
            c = ((d == bl) & (g > 0)) | ((d == bh) & (g < 0))
            if not moved and cf is not None and (c == cf).all():
                break
            if it == ITERS:
                status = 3
                break
            if cf is None or (c != cf).any():
                Hr = np.where(c[:, None] | c[None, :], np.eye(nu, dtype=H.dtype), H)
                L, ok = RR.cholesky(Hr)
                if not ok:
                    status = 1
                    break
                cf = c.copy()
            if c.all():
                break
            s = RR.chol_solve(L, np.where(c, dt(0), -g)[:, None])[:, 0]
            s = np.where(c, dt(0), s)
            sg = s @ g
            if not np.isfinite(sg):
                status = 1
                break
            if not sg < 0:
                break
            a, found = dt(1), False
            for _ in range(TRIALS):
                y = d + a * s
                xc = clip(y)
                vc = value(xc)
                ratio = (vc - v) / (a * sg)
                if np.isfinite(ratio):
                    marg["armijo"] = min(marg["armijo"], float(abs(ratio - dt(ARMIJO))))
                if ratio >= ARMIJO:
                    found = True
                    break
                a = a * dt(STEP)
            if not found:
                status = 3
                break
            moved = bool((xc != y).any()) or a != 1
            d, v = xc, vc
            it += 1
    if status == 0 and not np.isfinite(d).all():
        status = 1
    if status == 0:
        scale = float(np.abs(q).max())
        if c.any():
            marg["mult"] = float(np.abs(g[c]).min()) / scale
        fin = ~c & np.isfinite(bl) & np.isfinite(bh)
        if fin.any():
            marg["free"] = float((np.minimum(d - bl, bh - d)[fin] / (bh - bl)[fin]).min())
    return d, c, L, it, status, marg


def riccati_box(A, B, lx, lu, lxx, luu, u, lo, hi, reg=0.0, dtype=np.float64):
    """One problem: riccati_reference.riccati's arguments, u [T, nu], lo / hi [nu].  Returns a dict: k [T, nu], K [T, nu, nx], dV [2] in
    `dtype`; clamped [T] int64 (bit i: actuator i clamped), qp_iters [T], status, fail_step; margins (the worst over the steps);
    qps: per step (H, q, bl, bh) as the QP saw them."""
    A, B, lx, lu, lxx, luu, u, lo, hi = (np.asarray(x, dtype=dtype) for x in (A, B, lx, lu, lxx, luu, u, lo, hi))
    reg = dtype(reg)
    T, nx, nu = B.shape
    k, K, dV = np.zeros((T, nu), dtype=dtype), np.zeros((T, nu, nx), dtype=dtype), np.zeros(2, dtype=dtype)
    clamped, iters = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    marg = dict(mult=np.inf, free=np.inf, armijo=np.inf)
    qps = [None] * T
    failed = lambda st, t: dict(k=np.zeros_like(k), K=np.zeros_like(K), dV=np.zeros_like(dV), clamped=np.zeros_like(clamped),
                                qp_iters=np.zeros_like(iters), status=st, fail_step=t, margins=marg, qps=qps)
    Vx, Vxx = lx[T], lxx[T]
    half = dtype(0.5)
    for t in range(T - 1, -1, -1):
        with np.errstate(all="ignore"):
            At, Bt = A[t], B[t]
            Qx, Qu = lx[t] + At.T @ Vx, lu[t] + Bt.T @ Vx
            W = Vxx @ At
            Qxx, Qux, Quu = lxx[t] + At.T @ W, Bt.T @ W, luu[t] + Bt.T @ (Vxx @ Bt)
            H, bl, bh = Quu + reg * np.eye(nu, dtype=dtype), lo - u[t], hi - u[t]
        qps[t] = (H, Qu, bl, bh)
        kt, c, L, it, st, m = box_qp(H, Qu, bl, bh)
        if st:
            return failed(st, t)
        marg = {name: min(marg[name], m[name]) for name in marg}
        with np.errstate(all="ignore"):
            Kt = -RR.chol_solve(L, np.where(c[:, None], dtype(0), Qux))
            Kt = np.where(c[:, None], dtype(0), Kt)
            if not np.isfinite(Kt).all():
                return failed(1, t)
            Vx = Qx + Kt.T @ (Quu @ kt + Qu) + Qux.T @ kt
            Vxx = Qxx + Kt.T @ (Quu @ Kt) + Kt.T @ Qux + Qux.T @ Kt
            Vxx = half * (Vxx + Vxx.T)
            dV[0] += kt @ Qu
            dV[1] += half * (kt @ (Quu @ kt))
        k[t], K[t], iters[t] = kt, Kt, it
        clamped[t] = int(sum(1 << i for i in range(nu) if c[i]))
    return dict(k=k, K=K, dV=dV, clamped=clamped, qp_iters=iters, status=0, fail_step=-1, margins=marg, qps=qps)


def batch(A, B, lx, lu, lxx, luu, u, lo, hi, reg=0.0, dtype=np.float64):
    """riccati_box over the n problems (lxx / luu / lo / hi with or without the leading problem dimension; reg a number or [n])."""
    n = len(B)
    reg = np.broadcast_to(np.asarray(reg, dtype=np.float64).reshape(-1), (n,))
    lo, hi = (np.broadcast_to(np.asarray(x), (n, B.shape[3])) for x in (lo, hi))
    rows = [riccati_box(A[e], B[e], lx[e], lu[e], lxx[e] if lxx.ndim == 4 else lxx, luu[e] if luu.ndim == 4 else luu, u[e], lo[e], hi[e],
                        reg[e], dtype) for e in range(n)]
    out = {name: np.stack([r[name] for r in rows]) for name in ("k", "K", "dV", "clamped", "qp_iters")}
    out.update(status=np.array([r["status"] for r in rows], dtype=np.uint8), fail_step=np.array([r["fail_step"] for r in rows], dtype=np.int32),
               margins={name: min(r["margins"][name] for r in rows) for name in ("mult", "free", "armijo")}, qps=[r["qps"] for r in rows])
    return out


def bvls(H, q, bl, bh):
    """The minimiser by SciPy's bounded-variable least squares on the factor of H: float64, nothing of box_qp."""
    import scipy.linalg
    import scipy.optimize
    H, q = np.asarray(H, dtype=np.float64), np.asarray(q, dtype=np.float64)
    R = scipy.linalg.cholesky(0.5 * (H + H.T), lower=False)
    rhs = -scipy.linalg.solve_triangular(R, q, trans="T", lower=False)
    res = scipy.optimize.lsq_linear(R, rhs, bounds=(np.asarray(bl, dtype=np.float64), np.asarray(bh, dtype=np.float64)), method="bvls",
                                    tol=1e-15, max_iter=1000)
    return res.x


def kkt(H, q, bl, bh, d, c):
    """dict(feas, free, clamped): the KKT residuals of d with the clamped set c, relative to max |q| (feas: to the box's scale)."""
    g = q + H @ d
    scale = float(np.abs(q).max())
    low, high = c & (d == bl), c & (d == bh)
    assert (low | high)[c].all(), "a clamped coordinate is not on a bound"
    wrong = np.concatenate([np.maximum(-g[low], 0), np.maximum(g[high], 0), [0]])
    return dict(feas=float(np.maximum(np.maximum(bl - d, d - bh), 0).max()), free=float(np.abs(g[~c]).max(initial=0)) / scale,
                clamped=float(wrong.max()) / scale)


_FAMILY = {}


def family(nx, nu, T, n, reg=0.0, seed=RR.SEED):
    """(arrays, the longdouble batch of them): riccati_reference.family's dict plus u [n, T, nu], lo, hi [n, nu] -- the module header's
    box family for this (class, T, n, reg), redrawn until every margin of the longdouble reference exceeds MARGIN; computed once per
    argument set and shared."""
    key = (nx, nu, T, n, reg, seed)
    if key not in _FAMILY:
        f = RR.family(nx, nu, T, n, seed)
        for attempt in range(50):
            rng = np.random.default_rng(seed + 1000 + attempt)
            w = np.stack([BASE[e % 3] * (0.5 + rng.random(nu)) for e in range(n)])
            c = 0.3 * rng.standard_normal((n, nu))
            u = c[:, None, :] + 0.9 * w[:, None, :] * rng.uniform(-1, 1, (n, T, nu))
            g = dict(f, u=u, lo=c - w, hi=c + w)
            ref = batch(**g, reg=reg, dtype=np.longdouble)
            if not ref["status"].any() and min(ref["margins"].values()) > MARGIN:
                break
        else:
            raise AssertionError("no draw of the box family met the margins")
        _FAMILY[key] = (g, ref, attempt)
    return _FAMILY[key]


def lqr_backward_box(lx, lu, lxx, luu, u, lo, hi, A=None, B=None, deriv_t=None, reg=0.0, out=None):
    """KManipEnvHip.lqr_backward_box's signature and result on CPU tensors, the float64 restatement per problem."""
    import torch
    assert out is None and ((deriv_t is None) != (A is None and B is None)) and ((A is None) == (B is None))
    np_ = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
    if deriv_t is not None:
        d = np_(deriv_t)
        nx = d.shape[3]
        A, B = d[:, :, :nx].transpose(0, 1, 3, 2), d[:, :, nx:].transpose(0, 1, 3, 2)
    else:
        A, B = np_(A), np_(B)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    nu = B.shape[3]
    lo = np.full(nu, -np.inf) if lo is None else np_(lo)
    hi = np.full(nu, np.inf) if hi is None else np_(hi)
    r = batch(A, B, np_(lx), np_(lu), np_(lxx), np_(luu), np_(u), lo, hi, np_(reg))
    gains_t = torch.from_numpy(np.ascontiguousarray(r["K"].transpose(0, 1, 3, 2)))
    return {"k": torch.from_numpy(r["k"]), "gains_t": gains_t, "K": gains_t.transpose(2, 3), "dV": torch.from_numpy(r["dV"]),
            "status": torch.from_numpy(r["status"]), "fail_step": torch.from_numpy(r["fail_step"]),
            "clamped": torch.from_numpy(r["clamped"].astype(np.int32)), "qp_iters": torch.from_numpy(r["qp_iters"].astype(np.int32))}


class OracleLqrBox(RR.OracleLqr):
    """OracleLqr plus KManipEnvHip.lqr_backward_box, and rollout_feedback(ctrl_lo=, ctrl_hi=): the clamp after the finite-u test, the
    clamped u acting and recorded, a box with lo <= hi false giving status 1 and no step.  Box calls are kept in .box_calls."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.box_calls = []
        self._box = None

    def lqr_backward_box(self, *a, **kw):
        res = lqr_backward_box(*a, **kw)
        self.box_calls.append(dict(res, args=a, kwargs=kw))
        return res

    def rollout_feedback(self, *a, ctrl_lo=None, ctrl_hi=None, **kw):
        import torch
        if ctrl_lo is None and ctrl_hi is None:
            return super().rollout_feedback(*a, **kw)
        np_ = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
        nu = self.cm.nu
        self._box = (np.full(nu, -np.inf) if ctrl_lo is None else np_(ctrl_lo), np.full(nu, np.inf) if ctrl_hi is None else np_(ctrl_hi))
        try:
            return super().rollout_feedback(*a, **kw)
        finally:
            self._box = None

    def _step(self, m, orc, q, v, u, w, tau, nsub):
        """OracleFeedback hands its unclamped u here and records the array it handed: clamped in place, the clamped u acts and is
        what the record shows.  (One box for all rows, or row g's: the stand-in is only run with a shared box or one row per
        trajectory in trajectory order.)"""
        if self._box is not None:
            lo, hi = self._box
            if lo.ndim == 2:
                raise NotImplementedError("the stand-in takes one box for all rows")
            if not (lo <= hi).all():
                return q, v, w, True
            np.copyto(u, np.minimum(np.maximum(u, lo), hi))
        return super()._step(m, orc, q, v, u, w, tau, nsub)
