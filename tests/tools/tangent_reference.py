"""The inputs of kmanip_tangent's tests and of tangent_cost.py, and the distance they are judged by.  The
restatement of the recursion itself is tests/test_tangent_cpu.py's sweep."""
import numpy as np

import adjoint_reference as AR

N_PROBLEMS, SCALE = 3, 0.1


def family(nx, nu, T, m, closed, n=N_PROBLEMS):
    """adjoint_reference.family's A, B and gains; from default_rng(23) in this order src, du, s0 at scale 0.1, then r standard normal and
    the symmetric positive-definite W = M M' / nx + I."""
    f = AR.family(nx, nu, T, n, m)
    rng = np.random.default_rng(23)
    src, du, s0 = (SCALE * rng.standard_normal(s) for s in ((n, T, nx, m), (n, T, nu, m), (n, nx, m)))
    r, M = rng.standard_normal((n, T + 1, nx)), rng.standard_normal((nx, nx))
    return dict(A=f["A"], B=f["B"], src=src, du=du, s0=s0, K=f["gains"] if closed else None, r=r, W=M @ M.T / nx + np.eye(nx))


def gaps(got, ref, names=("S", "du_acted", "H", "g")):
    """{name: the worst over the rows of max |got - ref| / max |ref|}: a row is a (problem, column) of S and du_acted, a problem of H, g."""
    out = {}
    for name in names:
        a, b = np.asarray(got[name]).astype(np.longdouble), ref[name]
        if name in ("S", "du_acted"):
            a, b = np.moveaxis(a, 3, 1), np.moveaxis(b, 3, 1)
            a, b = a.reshape(a.shape[0] * a.shape[1], -1), b.reshape(b.shape[0] * b.shape[1], -1)
        else:
            a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
        out[name] = float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())
    return out
