#!/usr/bin/env python3
"""Cost of KManipEnvHip.lqr_backward (kmanip_lqr_backward) beside ilqr.backward_pass, the torch loop it replaces, and where an iLQR
iteration spends its time, measured with HIP events in one process on one GPU:

    timeout 600 python tests/tools/lqr_cost.py [--reps 30] [--out profiles/lqr_backward_cost.txt]

After WARM untimed rounds, `--reps` rounds; a round times each phase as ONE call sequence between two events of its own, the phases
interleaved round by round so that clock and box drift hit all of them alike.  Reported: mean / median / min / max in us.
1. THE SPLIT: one fused ilqr.ilqr iteration of examples/ilqr_reach.py's problem (KManipSoloArmQPos, 8 envs, horizon 8, 3 alphas) cut
   into its five phases, each timed on the inputs the phase before it left: the nominal rollout; transition_fd (with the torch glue
   that builds its rows and views); the cost's derivatives; the backward pass, torch's and the device's; the forward pass with the
   cost of its rows, fed K and fed gains_t.  Then the whole iteration, device_backward off and on.
2. THE PASSES ALONE on riccati_reference.family at (n, T): KManipSoloArm (8, 8), (64, 32), (4096, 8); KManipDualArm (8, 8), (64, 32).
   The condition reported per shape is transfd_cost.py's: the device's max below torch's min.
The yardstick is ilqr.backward_pass at the same commit.  There is no absolute bar."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM = 3
HORIZON, NENV, ALPHAS = 8, 8, (1.0, 0.5, 0.25)
SHAPES = (("KManipSoloArm", ((8, 8), (64, 32), (4096, 8))), ("KManipDualArm", ((8, 8), (64, 32))))


def _timed(phases, reps):
    import torch
    t = {name: [] for name, _ in phases}
    for k in range(WARM + reps):
        for name, f in phases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            b.synchronize()
            if k >= WARM:
                t[name].append(a.elapsed_time(b) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import riccati_reference as RR
    from gym_kmanip_amd import env_hip, ilqr
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def report(tag, phases, t):
        for name, _ in phases:
            emit("%-26s %-34s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f"
                 % (tag, name, statistics.fmean(t[name]), statistics.median(t[name]), min(t[name]), max(t[name])))

    # ---- 1. the split of one fused iteration
    env = env_hip.make("KManipSoloArmQPos", num_envs=NENV, seed=3)
    cm, dev = env.cm, env.device
    env.k_reset()
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    goal = st["qpos"].clone()
    goal[:, :cm.nlink] += 0.1 * torch.tensor([1.0, -1.0], dtype=torch.float64, device=dev).repeat(cm.nlink)[:cm.nlink]
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64, device=dev)
    wq[:cm.nlink] = 10.0
    wq[cm.nv:cm.nv + cm.nlink] = 0.01
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((NENV, cm.nv), dtype=torch.float64, device=dev), wq, torch.full((cm.nu,), 1e-3, dtype=torch.float64, device=dev), 10.0 * wq)
    ctrl = st["ctrl"][:, None, :].repeat(1, HORIZON, 1)
    q0, v0, w0 = st["qpos"], st["qvel"], st["warm"]
    n, T, nx = NENV, HORIZON, 2 * cm.nv
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    reg = torch.full((n,), 1e-6, dtype=torch.float64, device=dev)
    s = {}

    def p_rollout():
        s["roll"] = env.rollout(envs=idx, qpos=q0, qvel=v0, warm=w0, ctrl=ctrl, fields=("qpos", "qvel", "qacc_warm", "status"))

    def p_transfd():                                   # ilqr.trajectory_fd after its rollout, line for line
        roll = s["roll"]
        qs, vs, ws = ilqr._start_states(q0, roll["qpos"]), ilqr._start_states(v0, roll["qvel"]), ilqr._start_states(w0, roll["qacc_warm"])
        flat = lambda t: t.reshape(n * T, t.shape[-1]).contiguous()
        d = env.transition_fd(envs=idx.repeat_interleave(T), qpos=flat(qs), qvel=flat(vs), ctrl=flat(ctrl), warm=flat(ws), qfrc_applied=None, nsub=None, eps=1e-6)
        s["fd"] = {"A": d["A"].reshape(n, T, nx, nx), "B": d["B"].reshape(n, T, nx, cm.nu), "deriv_t": d["deriv_t"].reshape(n, T, nx + cm.nu, nx),
                   "qpos": torch.cat([q0[:, None], roll["qpos"]], dim=1), "qvel": torch.cat([v0[:, None], roll["qvel"]], dim=1),
                   "status_fd": torch.maximum(d["status"], d["status_fd"]).reshape(n, T).max(dim=1).values}

    def p_cost():
        s["ls"] = cost.derivatives(s["fd"]["qpos"], s["fd"]["qvel"], ctrl)

    def p_back_torch():
        s["k"], s["K"], _ = ilqr.backward_pass(s["fd"]["A"], s["fd"]["B"], *s["ls"], reg=reg)

    def p_back_dev():
        s["bp"] = env.lqr_backward(*s["ls"], deriv_t=s["fd"]["deriv_t"], reg=reg)

    def forward(k, K, K_t):
        fd = s["fd"]
        return ilqr.forward_pass(env, None, q0, v0, w0, ctrl, k, K, fd["qpos"][:, :-1], fd["qvel"][:, :-1], cost, ALPHAS, K_t=K_t)

    phases = [("1 rollout", p_rollout), ("2 transition_fd", p_transfd), ("3 cost derivatives", p_cost), ("4 backward_pass (torch)", p_back_torch),
              ("4 lqr_backward (device)", p_back_dev), ("5 forward_pass + cost, K", lambda: forward(s["k"], s["K"], None)),
              ("5 forward_pass + cost, gains_t", lambda: forward(s["bp"]["k"], None, s["bp"]["gains_t"])),
              ("whole iteration, fused", lambda: ilqr.ilqr(env, None, q0, v0, w0, ctrl, cost, iters=1, alphas=ALPHAS, fused=True)),
              ("whole iteration, fused + device", lambda: ilqr.ilqr(env, None, q0, v0, w0, ctrl, cost, iters=1, alphas=ALPHAS, fused=True, device_backward=True))]
    t = _timed(phases, args.reps)
    a = ilqr.ilqr(env, None, q0, v0, w0, ctrl, cost, iters=1, alphas=ALPHAS, fused=True)
    b = ilqr.ilqr(env, None, q0, v0, w0, ctrl, cost, iters=1, alphas=ALPHAS, fused=True, device_backward=True)
    emit("# library %s; KManipSoloArmQPos, %d envs, horizon %d, %d alphas: one fused ilqr.ilqr iteration in phases, %d timed rounds after %d warm-up "
         "rounds; mean cost after it %.6f (torch backward pass) / %.6f (device), statuses nonzero %d; largest |K device - K torch| / largest |K| in the last round %.3e"
         % (env.L.kmanip_version().decode(), n, T, len(ALPHAS), args.reps, WARM, float(a["cost"][-1].mean()), float(b["cost"][-1].mean()),
            int(b["backward_status"].ne(0).sum()), float((s["bp"]["K"] - s["K"]).abs().max() / s["K"].abs().max())))
    report("iLQR 8 x 8", phases, t)
    env.k_close()

    # ---- 2. the passes alone
    for env_id, shapes in SHAPES:
        env = env_hip.make(env_id, num_envs=2, seed=1)
        nx, nu = 2 * env.cm.nv, env.cm.nu
        for n, T in shapes:
            f = RR.family(nx, nu, T, n)
            d = {name: torch.from_numpy(np.ascontiguousarray(v)).to(env.device) for name, v in f.items()}
            deriv_t = torch.cat([d["A"].transpose(2, 3), d["B"].transpose(2, 3)], dim=2).contiguous()
            ls = (d["lx"], d["lu"], d["lxx"], d["luu"])
            out = {}
            phases = [("backward_pass (torch)", lambda: out.update(torch=ilqr.backward_pass(d["A"], d["B"], *ls, reg=0.3))),
                      ("lqr_backward (device, deriv_t)", lambda: out.update(dev=env.lqr_backward(*ls, deriv_t=deriv_t, reg=0.3))),
                      ("lqr_backward (device, A and B)", lambda: out.update(dev_ab=env.lqr_backward(*ls, A=d["A"], B=d["B"], reg=0.3)))]
            t = _timed(phases, args.reps)
            tag = "%s %d x %d" % (env_id, n, T)
            emit("# %s (nx %d, nu %d): statuses nonzero %d; largest |K device - K torch| / largest |K| %.3e"
                 % (tag, nx, nu, int(out["dev"]["status"].ne(0).sum()), float((out["dev"]["K"] - out["torch"][1]).abs().max() / out["torch"][1].abs().max())))
            report(tag, phases, t)
            p1, p2 = t[phases[0][0]], t[phases[1][0]]
            emit("%-26s device / torch = %.4f   condition (device max < torch min): %s" % (tag, statistics.fmean(p2) / statistics.fmean(p1), "met" if max(p2) < min(p1) else "NOT met"))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
