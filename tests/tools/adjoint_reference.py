"""The adjoint sweep of a rollout restated in NumPy: the reference of kmanip_adjoint.  oracle/ and
riccati_reference.py stay as they are.

adjoint(...)          ONE problem with its m cotangent vectors, the recursion of include/kmanip.h KAdjointIn in the dtype the caller
                      chooses (np.float64 or np.longdouble), every product a NumPy matmul in that dtype: lam[T] = gx[T], then
                      mu[t] = gu[t] + B_t' lam[t+1], lam[t] = gx[t] + A_t' lam[t+1] + K_t' mu[t], the direct term added last.
family(...)           riccati_reference.family's A and B (imported, the same seed and draws) and, from default_rng(SEED) in this
                      order, gx [n m, T + 1, nx] and gu [n m, T, nu] standard normal, gains [n, T, nu, nx] = 0.1 N(0, 1).
batch(...)            adjoint over the n problems.
adjoint_rows(...)     the stand-in of KManipEnvHip.adjoint on CPU tensors: the float64 restatement per problem.
OracleAdjoint         feedback_oracle.OracleFeedback with that method, so that grad.rollout_grad(device=True) runs without a GPU."""
import numpy as np

import feedback_oracle as FO
import riccati_reference as RR

CLASSES = RR.CLASSES
SEED = 23
GAIN_SCALE = 0.1


def adjoint(A, B, gx, gu=None, gains=None, dtype=np.float64):
    """One problem: A [T, nx, nx], B [T, nx, nu], gx [m, T + 1, nx], gu [m, T, nu] or None, gains [T, nu, nx] or None.  Returns
    (lam [m, T + 1, nx], mu [m, T, nu]) in `dtype`."""
    A, B, gx = (np.asarray(x, dtype=dtype) for x in (A, B, gx))
    gu = None if gu is None else np.asarray(gu, dtype=dtype)
    K = None if gains is None else np.asarray(gains, dtype=dtype)
    T, nx, nu = B.shape
    m = gx.shape[0]
    lam, mu = np.zeros((m, T + 1, nx), dtype=dtype), np.zeros((m, T, nu), dtype=dtype)
    lam[:, T] = gx[:, T]
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            nxt = lam[:, t + 1]
            u = nxt @ B[t]
            if gu is not None:
                u = u + gu[:, t]
            s = nxt @ A[t]
            if K is not None:
                s = s + u @ K[t]
            mu[:, t], lam[:, t] = u, s + gx[:, t]
    return lam, mu


def family(nx, nu, T, n, m, seed=SEED):
    """dict of float64 arrays A [n, T, nx, nx], B [n, T, nx, nu] (riccati_reference.family's), gx [n m, T + 1, nx], gu [n m, T, nu],
    gains [n, T, nu, nx]: the module header's family."""
    f = RR.family(nx, nu, T, n)
    rng = np.random.default_rng(seed)
    gx = rng.standard_normal((n * m, T + 1, nx))
    gu = rng.standard_normal((n * m, T, nu))
    gains = GAIN_SCALE * rng.standard_normal((n, T, nu, nx))
    return dict(A=f["A"], B=f["B"], gx=gx, gu=gu, gains=gains)


def batch(A, B, gx, gu=None, gains=None, m=1, dtype=np.float64):
    """adjoint over the n problems of arrays with a leading problem dimension; gx / gu have n m rows, row e m + j vector j of
    problem e.  Returns dict(lam [n m, T + 1, nx], mu [n m, T, nu])."""
    n = len(B)
    rows = [adjoint(A[e], B[e], gx[e * m:(e + 1) * m], None if gu is None else gu[e * m:(e + 1) * m],
                    None if gains is None else gains[e], dtype) for e in range(n)]
    T, nx, nu = B.shape[1:]
    if n == 0:
        return dict(lam=np.zeros((0, T + 1, nx), dtype=dtype), mu=np.zeros((0, T, nu), dtype=dtype))
    return dict(lam=np.concatenate([r[0] for r in rows]), mu=np.concatenate([r[1] for r in rows]))


def adjoint_rows(gx, gu=None, A=None, B=None, deriv_t=None, gains=None, gains_t=None, m=1, out=None, nu=None):
    """KManipEnvHip.adjoint's signature and result on CPU tensors, float64 restatement per problem (nu: the model's, for a deriv_t
    with columns after ctrl's; default: none after them)."""
    import torch
    assert out is None and ((deriv_t is None) != (A is None and B is None)) and ((A is None) == (B is None))
    assert gains is None or gains_t is None
    np_ = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64))
    if deriv_t is not None:
        d = np_(deriv_t)
        nx = d.shape[3]
        nu = d.shape[2] - nx if nu is None else nu
        A, B = d[:, :, :nx].transpose(0, 1, 3, 2), d[:, :, nx:nx + nu].transpose(0, 1, 3, 2)
    else:
        A, B = np_(A), np_(B)
    K = np_(gains) if gains is not None else (None if gains_t is None else np.swapaxes(np_(gains_t), -1, -2))
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    r = batch(A, B, np_(gx), np_(gu), None if K is None else np.ascontiguousarray(K), int(m))
    return {"lam": torch.from_numpy(r["lam"]), "mu": torch.from_numpy(r["mu"])}


class OracleAdjoint(FO.OracleFeedback):
    """OracleFeedback plus KManipEnvHip.adjoint; every call's result is kept in .adjoint_calls."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.adjoint_calls = []

    def adjoint(self, *a, **kw):
        res = adjoint_rows(*a, nu=self.cm.nu, **kw)
        self.adjoint_calls.append(dict(res, args=a, kwargs=kw))
        return res
