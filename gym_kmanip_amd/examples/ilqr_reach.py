#!/usr/bin/env python3
"""iLQR in ctrl space to a joint-space goal (gym_kmanip_amd.ilqr): every env plans for itself from the state its handle holds.

    python -m gym_kmanip_amd.examples.ilqr_reach [--env KManipSoloArmQPos] [--num-envs 8] [--horizon 8] [--iters 5] [--alphas 1 0.5 0.25] [--fused] [--device-backward] [--box ctrlrange|FLOAT]

The goal of env e is its own joint configuration moved by `--reach` radians on every joint (signs alternate); the cost weighs the
joints' distance to it, the joint velocities and the servo targets' distance from the goal, and leaves the cube alone.  Per
iteration the device sees three calls whatever the horizon: the nominal rollout, transition_fd over all num_envs x horizon steps as
rows, and ONE rollout_feedback launch that runs the backward pass's time-varying policy closed loop for every step size at once
(num_envs x len(alphas) rows sharing num_envs gain trajectories).  With --fused the linearisation is KManipEnvHip.transition_fd, the rows perturbed and differenced inside the kernel, in place of
derivatives.transition_fd's torch arithmetic around two rollout launches; with --device-backward the backward pass is
KManipEnvHip.lqr_backward, one launch, in place of ilqr.backward_pass's torch loop over the steps.  The handle itself takes no step.  Printed: the mean cost per
iteration, then the record as JSON.  With --box the plan is control-limited: `ctrlrange` plans inside the
model's own servo range, a number inside that half-width around each env's initial ctrl (a trust region); the backward pass solves a
box QP per step (KManipEnvHip.lqr_backward_box with --device-backward, else ilqr.backward_pass_box), the line search clamps the
policy's output, and the share of (env, step, actuator) entries of the plan that sit on a bound is printed.  Both, --fused as well."""
import argparse
import json

from gym_kmanip_amd import env_hip, ilqr
from gym_kmanip_amd.model import ctrl_range


class _Count:
    """The env as ilqr sees it -- .cm, .rollout, .transition_fd, .lqr_backward, .rollout_feedback -- counting the feedback launches and
    their rows."""

    def __init__(self, env):
        self.env, self.cm, self.rows = env, env.cm, []
        self.rollout, self.transition_fd, self.lqr_backward = env.rollout, env.transition_fd, env.lqr_backward
        self.lqr_backward_box = env.lqr_backward_box

    def rollout_feedback(self, **kw):
        self.rows.append(int(kw["ctrl"].shape[0]))
        return self.env.rollout_feedback(**kw)


def main(argv=None):
    """Returns the printed record as a dict; "cost" is the mean over the envs of the accepted cost, entry 0 the initial guess's."""
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArmQPos")
    ap.add_argument("--num-envs", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--alphas", type=float, nargs="+", default=[1.0, 0.5, 0.25])
    ap.add_argument("--reach", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--fused", action="store_true", help="linearise with KManipEnvHip.transition_fd (kmanip_transition_fd)")
    ap.add_argument("--device-backward", action="store_true", help="the backward pass in one launch: KManipEnvHip.lqr_backward (kmanip_lqr_backward)")
    ap.add_argument("--box", default=None, help="plan inside a box on ctrl: `ctrlrange` (the model's) or a half-width around the initial ctrl")
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    cm, n, T = env.cm, args.num_envs, args.horizon
    dev = env.device
    env.k_reset()
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    # the goal: the joints moved, the cube wherever it is (its columns carry no weight)
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64, device=dev).repeat(cm.nlink)[:cm.nlink]
    goal = st["qpos"].clone()
    goal[:, :cm.nlink] += args.reach * sign
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64, device=dev)
    wq[:cm.nlink] = 10.0
    wq[cm.nv:cm.nv + cm.nlink] = 0.01
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((n, cm.nv), dtype=torch.float64, device=dev), wq,
                              torch.full((cm.nu,), 1e-3, dtype=torch.float64, device=dev), 10.0 * wq)
    guess = st["ctrl"][:, None, :].repeat(1, T, 1)
    box = {}
    if args.box == "ctrlrange":
        box = dict(zip(("ctrl_lo", "ctrl_hi"), ctrl_range(cm, dev)))
    elif args.box is not None:
        box = dict(ctrl_lo=st["ctrl"] - float(args.box), ctrl_hi=st["ctrl"] + float(args.box))
    counted = _Count(env)
    res = ilqr.ilqr(counted, None, st["qpos"], st["qvel"], st["warm"], guess, cost, iters=args.iters, alphas=args.alphas, fused=args.fused,
                    device_backward=args.device_backward, **box)
    after = env.state_tensors()
    assert all(torch.equal(st[k], after[k]) for k in st)                                 # the handle was only read
    per_env = res["cost"].cpu()
    for it, c in enumerate(per_env.mean(dim=1).tolist()):
        print("iteration %d: mean cost %.6f" % (it, c))
    out = {"env": args.env, "num_envs": n, "horizon": T, "alphas": list(args.alphas), "fused": bool(args.fused), "device_backward": bool(args.device_backward),
           "backward_failures": int(res["backward_status"].ne(0).sum()) if "backward_status" in res else 0, "cost": per_env.mean(dim=1).tolist(),
           "cost_per_env": per_env.tolist(), "accepted": res["accepted"].cpu().tolist(), "feedback_launches": len(counted.rows),
           "rows_per_line_search": counted.rows[0] if counted.rows else 0, "first_ctrl_moved_by": float((res["ctrl"][:, 0] - st["ctrl"]).abs().max())}
    if box:
        lo, hi = (box[k].reshape(-1, 1, cm.nu) for k in ("ctrl_lo", "ctrl_hi"))
        on = (res["ctrl"] == lo) | (res["ctrl"] == hi)
        out.update(box=args.box, box_share=float(on.double().mean()), inside_box=bool(((res["ctrl"] >= lo) & (res["ctrl"] <= hi)).all()))
        print("on a bound: %.1f %% of the plan's (env, step, actuator) entries" % (100.0 * out["box_share"]))
    print(json.dumps(out))
    env.k_close()
    return out


if __name__ == "__main__":
    main()
