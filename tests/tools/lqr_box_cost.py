#!/usr/bin/env python3
"""What the control-limited backward pass and the clamped line search cost: needs an MI355X.

    python tests/tools/lqr_box_cost.py [--reps 30] [--out profiles/lqr_box_cost.txt]

lqr_cost.py's method: HIP events around each phase, the phases interleaved round by round, WARM warm-up rounds, then mean (min - max)
in us over --reps rounds, one process.
1. THE PASSES on riccati_reference.family at (n, T): KManipSoloArm (8, 8), (64, 32); KManipDualArm (8, 8).  u = 0 and the box
   [-w, w], w the 2/3 quantile of |k| of the unconstrained pass, so that the box binds on roughly a third of the (problem, step,
   actuator) entries; the share the device's masks show is printed.  Timed: ilqr.backward_pass_box (torch), KManipEnvHip.lqr_backward_box
   and, on the same problems, KManipEnvHip.lqr_backward.  The condition is transfd_cost.py's: the device's max below torch's min.
   Reported without a bar: the ratio to lqr_backward and the mean qp_iters.
2. THE LINE SEARCH: rollout_feedback on examples/ilqr_reach.py's problem (KManipSoloArmQPos, 8 envs, horizon 8, 3 alphas: 24 rows)
   under the gains of one backward pass, without a box and clamped to the model's ctrlrange.  Reported without a bar."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("KManipSoloArm", ((8, 8), (64, 32))), ("KManipDualArm", ((8, 8),)))
HORIZON, NENV, ALPHAS = 8, 8, (1.0, 0.5, 0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import riccati_reference as RR
    from lqr_cost import WARM, _timed
    from gym_kmanip_amd import env_hip, ilqr
    from gym_kmanip_amd.model import ctrl_range
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def report(tag, phases, t):
        for name, _ in phases:
            emit("%-24s %-34s mean %9.1f us  (min %9.1f - max %9.1f)" % (tag, name, statistics.fmean(t[name]), min(t[name]), max(t[name])))

    emit("# HIP events, phases interleaved, %d timed rounds after %d warm-up rounds, one process" % (args.reps, WARM))
    for env_id, shapes in SHAPES:
        env = env_hip.make(env_id, num_envs=2, seed=1)
        if env_id == SHAPES[0][0]:
            emit("# library %s" % env.L.kmanip_version().decode())
        nx, nu = 2 * env.cm.nv, env.cm.nu
        for n, T in shapes:
            f = RR.family(nx, nu, T, n)
            d = {name: torch.from_numpy(np.ascontiguousarray(v)).to(env.device) for name, v in f.items()}
            deriv_t = torch.cat([d["A"].transpose(2, 3), d["B"].transpose(2, 3)], dim=2).contiguous()
            ls = (d["lx"], d["lu"], d["lxx"], d["luu"])
            free = env.lqr_backward(*ls, deriv_t=deriv_t, reg=0.3)
            w = torch.quantile(free["k"].abs().flatten(), 2.0 / 3.0)
            u, lo, hi = torch.zeros_like(d["lu"]), torch.full((nu,), -float(w), dtype=torch.float64, device=env.device), torch.full((nu,), float(w), dtype=torch.float64, device=env.device)
            out = {}
            phases = [("backward_pass_box (torch)", lambda: out.update(torch=ilqr.backward_pass_box(d["A"], d["B"], *ls, u, lo, hi, reg=0.3))),
                      ("lqr_backward_box (device)", lambda: out.update(dev=env.lqr_backward_box(*ls, u, lo, hi, deriv_t=deriv_t, reg=0.3))),
                      ("lqr_backward (device)", lambda: out.update(plain=env.lqr_backward(*ls, deriv_t=deriv_t, reg=0.3)))]
            t = _timed(phases, args.reps)
            tag = "%s %d x %d" % (env_id, n, T)
            bits = (out["dev"]["clamped"][..., None].long() >> torch.arange(nu, device=env.device)) & 1
            emit("# %s (nx %d, nu %d), half-width %.4f: share of entries on a bound %.3f; mean qp_iters %.2f (max %d); statuses nonzero %d; masks equal "
                 "torch's: %s; largest |K device - K torch| / largest |K| %.3e"
                 % (tag, nx, nu, float(w), float(bits.double().mean()), float(out["dev"]["qp_iters"].double().mean()), int(out["dev"]["qp_iters"].max()),
                    int(out["dev"]["status"].ne(0).sum()), bool(torch.equal(out["dev"]["clamped"], out["torch"][3])),
                    float((out["dev"]["K"] - out["torch"][1]).abs().max() / out["torch"][1].abs().max())))
            report(tag, phases, t)
            p1, p2, p3 = (t[name] for name, _ in phases)
            emit("%-24s device / torch = %.4f   condition (device max < torch min): %s   box / lqr_backward = %.2f"
                 % (tag, statistics.fmean(p2) / statistics.fmean(p1), "met" if max(p2) < min(p1) else "NOT met", statistics.fmean(p2) / statistics.fmean(p3)))
        env.k_close()

    # ---- 2. the line search, with and without the clamp
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
    fd = ilqr.trajectory_fd(env, None, st["qpos"], st["qvel"], st["warm"], ctrl, fused=True)
    bp = env.lqr_backward(*cost.derivatives(fd["qpos"], fd["qvel"], ctrl), deriv_t=fd["deriv_t"], reg=1e-6)
    lo, hi = ctrl_range(cm, dev)
    args_fp = (env, None, st["qpos"], st["qvel"], st["warm"], ctrl, bp["k"], None, fd["qpos"][:, :-1], fd["qvel"][:, :-1], cost, ALPHAS)
    out = {}
    phases = [("forward_pass, kmanip_feedback", lambda: out.update(a=ilqr.forward_pass(*args_fp, K_t=bp["gains_t"]))),
              ("forward_pass, kmanip_feedback_box", lambda: out.update(b=ilqr.forward_pass(*args_fp, K_t=bp["gains_t"], ctrl_lo=lo, ctrl_hi=hi)))]
    t = _timed(phases, args.reps)
    on = (out["b"]["rows"]["ctrl"] == lo) | (out["b"]["rows"]["ctrl"] == hi)
    emit("# KManipSoloArmQPos, %d envs, horizon %d, %d alphas (%d rows): the line search with its cost; ctrlrange binds on %.3f of the clamped launch's entries"
         % (NENV, HORIZON, len(ALPHAS), NENV * len(ALPHAS), float(on.double().mean())))
    report("line search 8 x 8", phases, t)
    env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
