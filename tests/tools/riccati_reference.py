"""The backward pass of iLQR restated in NumPy: the reference of kmanip_lqr_backward.  oracle/ stays as it is.

riccati(...)          ONE problem, the recursion of include/kmanip.h KLqrIn in the dtype the caller chooses (np.float64 or
                      np.longdouble), every product a NumPy matmul in that dtype, the solve a hand-written Cholesky factorisation
                      (lower triangle, column by column, the pivot tested before its root) and two triangular solves, with the
                      device's rules: a pivot that is not > 0 or not finite at step t, or an entry of the step's k or K that is not
                      finite, stops the problem -- status 1, fail_step t, k, K and dV all zeros.
family(...)           THE WELL-CONDITIONED TEST FAMILY, rng = default_rng(seed), per problem and in this order: for t = 0 .. T-1
                      A_t = I + 0.4 N / sqrt(nx) and B_t = N / sqrt(nx) (N: standard normal draws of the matrix's shape), then lxx
                      [T + 1] = M M' / nx + I (M [nx, nx] normal), luu [T] = M M' / nu + I (M [nu, nu]), lx [T + 1, nx] and lu [T, nu]
                      standard normal.
lqr_backward(...)     the stand-in of KManipEnvHip.lqr_backward on CPU tensors: riccati per problem in float64.
OracleLqr             feedback_oracle.OracleFeedback with that method, so that ilqr.ilqr(device_backward=True) runs without a GPU."""
import numpy as np

import feedback_oracle as FO

CLASSES = ((32, 10), (52, 20))       # (nx, nu): KManipSoloArm; KManipDualArm and KManipTorso
SEED = 17


def cholesky(a):
    """(L, ok): the lower factor of the symmetric a from its lower triangle, in a's dtype; ok False as soon as a pivot is not > 0 or
    not finite (L is then unfinished)."""
    n = a.shape[0]
    L = np.zeros_like(a)
    for j in range(n):
        with np.errstate(all="ignore"):
            s = a[j:, j] - L[j:, :j] @ L[j, :j]
        if not (s[0] > 0 and np.isfinite(s[0])):
            return L, False
        d = np.sqrt(s[0])
        L[j, j] = d
        L[j + 1:, j] = s[1:] / d
    return L, True


def chol_solve(L, b):
    """x with L L' x = b (b [n, m]): forward, then back, row by row."""
    n = L.shape[0]
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def riccati(A, B, lx, lu, lxx, luu, reg=0.0, dtype=np.float64):
    """One problem: A [T, nx, nx], B [T, nx, nu], lx [T + 1, nx], lu [T, nu], lxx [T + 1, nx, nx], luu [T, nu, nu], reg a number.
    Returns (k [T, nu], K [T, nu, nx], dV [2], status, fail_step) in `dtype`."""
    A, B, lx, lu, lxx, luu = (np.asarray(x, dtype=dtype) for x in (A, B, lx, lu, lxx, luu))
    reg = dtype(reg)
    T, nx, nu = B.shape
    k, K, dV = np.zeros((T, nu), dtype=dtype), np.zeros((T, nu, nx), dtype=dtype), np.zeros(2, dtype=dtype)
    Vx, Vxx = lx[T], lxx[T]
    half = dtype(0.5)
    for t in range(T - 1, -1, -1):
        with np.errstate(all="ignore"):
            At, Bt = A[t], B[t]
            Qx, Qu = lx[t] + At.T @ Vx, lu[t] + Bt.T @ Vx
            W = Vxx @ At
            Qxx, Qux, Quu = lxx[t] + At.T @ W, Bt.T @ W, luu[t] + Bt.T @ (Vxx @ Bt)
        L, ok = cholesky(Quu + reg * np.eye(nu, dtype=dtype))
        if not ok:
            return np.zeros_like(k), np.zeros_like(K), np.zeros_like(dV), 1, t
        with np.errstate(all="ignore"):
            sol = -chol_solve(L, np.concatenate([Qu[:, None], Qux], axis=1))
            kt, Kt = sol[:, 0], sol[:, 1:]
            if not np.isfinite(sol).all():
                return np.zeros_like(k), np.zeros_like(K), np.zeros_like(dV), 1, t
            Vx = Qx + Kt.T @ (Quu @ kt + Qu) + Qux.T @ kt
            Vxx = Qxx + Kt.T @ (Quu @ Kt) + Kt.T @ Qux + Qux.T @ Kt
            Vxx = half * (Vxx + Vxx.T)
            dV[0] += kt @ Qu
            dV[1] += half * (kt @ (Quu @ kt))
        k[t], K[t] = kt, Kt
    return k, K, dV, 0, -1


def family(nx, nu, T, n, seed=SEED):
    """dict of float64 arrays A [n, T, nx, nx], B [n, T, nx, nu], lx [n, T + 1, nx], lu [n, T, nu], lxx [n, T + 1, nx, nx], luu
    [n, T, nu, nu]: the module header's family."""
    rng = np.random.default_rng(seed)
    out = {name: [] for name in ("A", "B", "lx", "lu", "lxx", "luu")}
    for _ in range(n):
        A, B = np.zeros((T, nx, nx)), np.zeros((T, nx, nu))
        for t in range(T):
            A[t] = np.eye(nx) + 0.4 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
            B[t] = rng.standard_normal((nx, nu)) / np.sqrt(nx)
        M = rng.standard_normal((T + 1, nx, nx))
        lxx = M @ M.transpose(0, 2, 1) / nx + np.eye(nx)
        M = rng.standard_normal((T, nu, nu))
        luu = M @ M.transpose(0, 2, 1) / nu + np.eye(nu)
        lx, lu = rng.standard_normal((T + 1, nx)), rng.standard_normal((T, nu))
        for name, v in (("A", A), ("B", B), ("lx", lx), ("lu", lu), ("lxx", lxx), ("luu", luu)):
            out[name].append(v)
    return {name: np.stack(v) for name, v in out.items()}


def batch(A, B, lx, lu, lxx, luu, reg=0.0, dtype=np.float64):
    """riccati over the n problems of arrays with a leading problem dimension (lxx / luu with or without it; reg a number or [n]).
    Returns dict(k [n, T, nu], K [n, T, nu, nx], dV [n, 2], status [n] uint8, fail_step [n] int32)."""
    n = len(B)
    reg = np.broadcast_to(np.asarray(reg, dtype=np.float64).reshape(-1), (n,))
    rows = [riccati(A[e], B[e], lx[e], lu[e], lxx[e] if lxx.ndim == 4 else lxx, luu[e] if luu.ndim == 4 else luu, reg[e], dtype) for e in range(n)]
    return dict(k=np.stack([r[0] for r in rows]), K=np.stack([r[1] for r in rows]), dV=np.stack([r[2] for r in rows]),
                status=np.array([r[3] for r in rows], dtype=np.uint8), fail_step=np.array([r[4] for r in rows], dtype=np.int32))


def lqr_backward(lx, lu, lxx, luu, A=None, B=None, deriv_t=None, reg=0.0, out=None):
    """KManipEnvHip.lqr_backward's signature and result on CPU tensors, float64 restatement per problem."""
    import torch
    assert out is None and ((deriv_t is None) != (A is None and B is None)) and ((A is None) == (B is None))
    np_ = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
    if deriv_t is not None:
        d = np_(deriv_t)
        nx = d.shape[3]
        A, B = d[:, :, :nx].transpose(0, 1, 3, 2), d[:, :, nx:].transpose(0, 1, 3, 2)
    else:
        A, B = np_(A), np_(B)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)      # (one memory layout whichever way they came: BLAS sums by layout)
    r = batch(A, B, np_(lx), np_(lu), np_(lxx), np_(luu), np_(reg))
    gains_t = torch.from_numpy(np.ascontiguousarray(r["K"].transpose(0, 1, 3, 2)))
    return {"k": torch.from_numpy(r["k"]), "gains_t": gains_t, "K": gains_t.transpose(2, 3), "dV": torch.from_numpy(r["dV"]),
            "status": torch.from_numpy(r["status"]), "fail_step": torch.from_numpy(r["fail_step"])}


class OracleLqr(FO.OracleFeedback):
    """OracleFeedback plus KManipEnvHip.lqr_backward; every call's result is kept in .lqr_calls."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lqr_calls = []

    def lqr_backward(self, *a, **kw):
        res = lqr_backward(*a, **kw)
        self.lqr_calls.append(dict(res, args=a, kwargs=kw))
        return res
