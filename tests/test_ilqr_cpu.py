"""gym_kmanip_amd.ilqr on the CPU: the backward pass against a NumPy restatement and against the discrete LQR gain, the cost's
derivatives against finite differences, and the whole loop driven through the oracle stand-in (tests/tools/feedback_oracle.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import feedback_oracle as FO  # noqa: E402
import rollout_oracle as RO  # noqa: E402


def _riccati_numpy(A, B, lx, lu, lxx, luu, reg):
    """The recursion of ilqr.backward_pass for one problem, written with explicit inverses."""
    T = len(B)
    Vx, Vxx = lx[T], lxx[T]
    k, K = [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        Qx, Qu = lx[t] + A[t].T @ Vx, lu[t] + B[t].T @ Vx
        Qxx, Quu, Qux = lxx[t] + A[t].T @ Vxx @ A[t], luu[t] + B[t].T @ Vxx @ B[t], B[t].T @ Vxx @ A[t]
        inv = np.linalg.inv(Quu + reg * np.eye(len(Qu)))
        k[t], K[t] = -inv @ Qu, -inv @ Qux
        Vx = Qx + K[t].T @ Quu @ k[t] + K[t].T @ Qu + Qux.T @ k[t]
        Vxx = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qux + Qux.T @ K[t]
        Vxx = 0.5 * (Vxx + Vxx.T)
    return np.stack(k), np.stack(K)


def test_backward_pass_is_the_riccati_recursion():
    """Random (A, B, Q, R) and random cost gradients, 5 problems, horizon 6, two regularisations: k and K equal the NumPy
    restatement's to 1e-10 of their size."""
    import torch
    from gym_kmanip_amd.ilqr import backward_pass
    rng = np.random.default_rng(11)
    n, T, nx, nu = 5, 6, 7, 3
    A = rng.standard_normal((n, T, nx, nx)) * 0.4 + np.eye(nx)
    B = rng.standard_normal((n, T, nx, nu))
    sq = lambda m: m @ np.swapaxes(m, -1, -2)
    lxx = sq(rng.standard_normal((n, T + 1, nx, nx))) + np.eye(nx)
    luu = sq(rng.standard_normal((n, T, nu, nu))) + np.eye(nu)
    lx, lu = rng.standard_normal((n, T + 1, nx)), rng.standard_normal((n, T, nu))
    for reg in (0.0, 0.3):
        k, K, dV = backward_pass(*(torch.from_numpy(x) for x in (A, B, lx, lu, lxx, luu)), reg=reg)
        assert tuple(k.shape) == (n, T, nu) and tuple(K.shape) == (n, T, nu, nx) and tuple(dV.shape) == (n, 2)
        for e in range(n):
            kn, Kn = _riccati_numpy(A[e], B[e], lx[e], lu[e], lxx[e], luu[e], reg)
            assert np.abs(k[e].numpy() - kn).max() <= 1e-10 * np.abs(kn).max() and np.abs(K[e].numpy() - Kn).max() <= 1e-10 * np.abs(Kn).max()
        # the expected reduction of a full step: minus (dV1 + dV2), positive for a positive definite problem without regularisation
        if reg == 0.0:
            assert bool((-(dV[:, 0] + dV[:, 1]) > 0).all())
    # per-env regularisation and cost Hessians shared by the batch (no leading dimension)
    regs = np.array([0.0, 0.1, 0.2, 0.3, 0.4])
    k, K, _ = backward_pass(*(torch.from_numpy(x) for x in (A, B, lx, lu, lxx[0], luu[0])), reg=torch.from_numpy(regs))
    for e in range(n):
        kn, Kn = _riccati_numpy(A[e], B[e], lx[e], lu[e], lxx[0], luu[0], regs[e])
        assert np.abs(k[e].numpy() - kn).max() <= 1e-10 * np.abs(kn).max() and np.abs(K[e].numpy() - Kn).max() <= 1e-10 * np.abs(Kn).max()


def test_a_long_horizon_gives_the_discrete_lqr_gain():
    """A time-invariant stable system (spectral radius 0.9), horizon 400, no gradients: K_0 of the backward pass against the gain of
    the Riccati map's fixed point, iterated in NumPy until P moves by less than 1e-13 of its size.
    THE BAR.  The backward pass IS that iteration, started from Qf = Q and run 400 times; the map contracts, so after 400 steps it is
    no further from the fixed point than the NumPy iterate was when its step fell below the residual r (it took fewer than 400).  A
    change dP of P moves the gain by at most |d K / d P| |dP| <= c r |K|, with c the conditioning of the solve, bounded here by
    cond(R + B' P B) (|A| |B| |P| / |B' P A| is of order one for this system); both sides also carry the rounding of 400 steps,
    400 x 2^-53 x cond.  The bar is (r + 400 x 2^-53) x cond(R + B' P B) x 10 relative to |K|, stated and printed."""
    import torch
    from gym_kmanip_amd.ilqr import backward_pass
    rng = np.random.default_rng(2)
    nx, nu, T = 6, 2, 400
    A = rng.standard_normal((nx, nx))
    A *= 0.9 / np.abs(np.linalg.eigvals(A)).max()
    B = rng.standard_normal((nx, nu))
    Q, Rm = np.eye(nx), 0.1 * np.eye(nu)
    P, resid, its = Q.copy(), 1.0, 0
    while resid > 1e-13 and its < T:
        G = np.linalg.solve(Rm + B.T @ P @ B, B.T @ P @ A)
        Pn = Q + A.T @ P @ A - (B.T @ P @ A).T @ G
        Pn = 0.5 * (Pn + Pn.T)
        resid, P, its = np.abs(Pn - P).max() / np.abs(Pn).max(), Pn, its + 1
    assert resid <= 1e-13 and its < T
    K_lqr = -np.linalg.solve(Rm + B.T @ P @ B, B.T @ P @ A)
    t = lambda x, *lead: torch.from_numpy(np.broadcast_to(x, lead + x.shape).copy())
    k, K, dV = backward_pass(t(A, 1, T), t(B, 1, T), torch.zeros((1, T + 1, nx), dtype=torch.float64), torch.zeros((1, T, nu), dtype=torch.float64),
                             t(Q, T + 1), t(Rm, T), reg=0.0)
    bar = (resid + T * 2.0 ** -53) * np.linalg.cond(Rm + B.T @ P @ B) * 10.0
    gap = np.abs(K[0, 0].numpy() - K_lqr).max() / np.abs(K_lqr).max()
    print("\nLQR: fixed point after %d iterations (residual %.1e); |K_0 - K_lqr| / |K_lqr| = %.2e, bar %.2e" % (its, resid, gap, bar))
    assert gap <= bar and not k.any() and not dV.any()
    assert np.abs(np.linalg.eigvals(A + B @ K_lqr)).max() < 0.9


def test_quadratic_cost_derivatives_are_its_finite_differences():
    """lx and lu of QuadraticCost against centred differences of its total along tangent_perturb's columns (joints, cube position,
    velocities, controls: where dx is linear in the state the quadratic is differenced exactly up to the rounding of the totals,
    2^-53 x cost / eps; the bar is 1000 x that)."""
    import torch
    import regime_states as R
    from gym_kmanip_amd.derivatives import tangent_perturb
    from gym_kmanip_amd.ilqr import QuadraticCost
    cm = R.model("solo_arm")
    qpos, qvel, ctrl, _ = R.cells("solo_arm")
    rng = np.random.default_rng(4)
    n, T, nv, nu, nl = 2, 2, cm.nv, cm.nu, cm.nlink
    q = torch.from_numpy(qpos[:n * (T + 1)].reshape(n, T + 1, -1).copy())
    v = torch.from_numpy(qvel[:n * (T + 1)].reshape(n, T + 1, -1).copy())
    u = torch.from_numpy(ctrl[:n * T].reshape(n, T, -1).copy())
    M = rng.standard_normal((2 * nv, 2 * nv))
    cost = QuadraticCost(cm, torch.from_numpy(qpos[40:42].copy()), torch.from_numpy(qvel[40:42].copy()), torch.from_numpy(M @ M.T),
                         torch.from_numpy(rng.uniform(0.1, 1.0, nu)), torch.from_numpy(rng.uniform(0.1, 1.0, 2 * nv)))
    lx, lu, lxx, luu = cost.derivatives(q, v, u)
    assert tuple(lx.shape) == (n, T + 1, 2 * nv) and tuple(lu.shape) == (n, T, nu) and tuple(lxx.shape) == (T + 1, 2 * nv, 2 * nv) and tuple(luu.shape) == (T, nu, nu)
    eps = 1e-6
    bar = 1000.0 * 2.0 ** -53 * float(cost.total(q, v, u).max()) / eps
    for t in (0, T):
        for col in (0, nl + 1, nv + 2, nv + nl + 4):
            def moved(sign):
                q2, v2 = q.clone(), v.clone()
                if col < nv:
                    q2[:, t] = tangent_perturb(cm, q[:, t], col, sign * eps)
                else:
                    v2[:, t, col - nv] += sign * eps
                return cost.total(q2, v2, u)
            fd = (moved(1.0) - moved(-1.0)) / (2 * eps)
            assert float((fd - lx[:, t, col]).abs().max()) <= bar, (t, col)
    u2 = u.clone(); u2[:, 1, 3] += eps
    u3 = u.clone(); u3[:, 1, 3] -= eps
    assert float(((cost.total(q, v, u2) - cost.total(q, v, u3)) / (2 * eps) - lu[:, 1, 3]).abs().max()) <= bar


def test_ilqr_through_the_oracle_lowers_the_cost_with_one_feedback_call_per_iteration():
    """One contact-free SoloArm cell (row 20: C1, the cube in flight, no contact over the horizon), horizon 4, 2 iterations, 3
    alphas, a joint-space goal 0.1 rad away: the accepted costs never increase, the first iteration lowers the cost, and every
    forward pass is ONE rollout_feedback call of n x 3 rows whose references are the nominal states BEFORE each step."""
    import torch
    import regime_states as R
    from gym_kmanip_amd import ilqr
    run = RO.cell_runs("solo_arm")
    cm, rows = run["cm"], run["rows"]
    e, T, n = 20, 4, 1
    assert run["labels"][e] == "C1" and not run["ref"]["contact_mask"][e].any()
    q0, v0, w0, c0 = (torch.from_numpy(rows[k][e:e + 1].copy()) for k in ("qpos", "qvel", "warm", "ctrl"))
    goal = q0.clone()
    goal[:, :cm.nlink] += 0.1
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64)
    wq[:cm.nlink] = 10.0
    wq[cm.nv:cm.nv + cm.nlink] = 0.01
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((n, cm.nv), dtype=torch.float64), wq, torch.full((cm.nu,), 1e-3, dtype=torch.float64), 10.0 * wq)
    env = FO.OracleFeedback(cm, 2)
    res = ilqr.ilqr(env, [0], q0, v0, w0, c0[:, None].repeat(1, T, 1), cost, iters=2, alphas=(1.0, 0.5, 0.25))
    J = res["cost"].numpy()
    print("\niLQR on the oracle: cost per iteration %s, accepted %s" % (J[:, 0].tolist(), res["accepted"][:, 0].tolist()))
    assert J.shape == (3, 1) and np.isfinite(J).all() and (np.diff(J, axis=0) <= 0).all() and J[1, 0] < J[0, 0]
    assert len(env.fb_calls) == 2 and all(c["n"] == n * 3 and c["nstep"] == T for c in env.fb_calls)
    assert len(env.calls) == 2 * 3 and [c["nstep"] for c in env.calls] == [T, 1, 1] * 2          # rollout, then transition_fd's two launches
    assert len(env.calls[1]["qpos"]) == n * T and len(env.calls[2]["qpos"]) == 2 * (2 * cm.nv + cm.nu) * n * T
    fb = env.fb_calls[0]
    assert fb["gain_index"].tolist() == [0, 0, 0] and fb["gains"].shape == (n, T, cm.nu, 2 * cm.nv)
    # the references are x_0 .. x_{T-1} of the nominal rollout: the initial row, then its records 0 .. T-2
    nominal = env.rollout(envs=[0], qpos=q0, qvel=v0, warm=w0, ctrl=c0[:, None].repeat(1, T, 1))
    assert np.array_equal(fb["qpos_ref"][0, 0], q0.numpy()[0]) and np.array_equal(fb["qpos_ref"][0, 1:], nominal["qpos"].numpy()[0, :-1])
    assert np.array_equal(fb["qvel_ref"][0, 1:], nominal["qvel"].numpy()[0, :-1])
    # the open-loop terms are the nominal ctrl + alpha k, alpha-major
    guess = c0.numpy()[:, None]
    assert np.allclose(fb["ctrl"][0] - guess[0], 2.0 * (fb["ctrl"][1] - guess[0]), rtol=0, atol=1e-12) and np.abs(fb["ctrl"][2] - guess[0]).max() > 1e-6
    assert tuple(res["ctrl"].shape) == (n, T, cm.nu) and tuple(res["K"].shape) == (n, T, cm.nu, 2 * cm.nv)
