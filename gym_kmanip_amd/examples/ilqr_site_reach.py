#!/usr/bin/env python3
"""iLQR in ctrl space to a task-space goal (gym_kmanip_amd.ilqr.SiteCost): every env plans to put its end-effector site(s) at a point.

    python -m gym_kmanip_amd.examples.ilqr_site_reach [--env KManipSoloArmQPos|KManipDualArmQPos] [--num-envs 8] [--horizon 8] [--iters 5]
        [--cube] [--device-cost] [--fused] [--device-backward] [--box ctrlrange|FLOAT]

The target of each present arm is a Cartesian goal, its site's position at the start plus an offset drawn uniformly in +-5 cm per
axis, or -- with --cube -- the cube itself: SiteCost(follow_cube=True) with a zero offset, a target that moves with the state.  The
cost is SumCost(QuadraticCost with velocity and control weights only, SiteCost): nothing is said in joint space about where the arm
should go.  --device-cost evaluates the site cost, its gradient and Gauss-Newton Hessian in one kmanip_site_cost launch per call
 in place of kinematics_at and torch arithmetic; --fused, --device-backward and --box are ilqr_reach's.  Printed:
the mean cost per iteration, the median site-to-target distance at the start and at the end of the plan, then the record as JSON.
plan() is the loop itself on any env with ilqr's methods and kinematics_at: tests run it on the CPU oracle's stand-in."""
import argparse
import json

import numpy as np

from gym_kmanip_amd import ilqr

W_POS, WF_POS, W_VEL, W_CTRL = 200.0, 2000.0, 0.01, 1e-4


def _present(cm):
    return [a for a in range(2) if cm.desc.arm_present[a]]


def site_distance(env, qpos, qvel, target_pos, follow_cube):
    """[n, arms]: the distance of each present arm's site to its target at the states qpos [n, nq] (one kinematics_at call)."""
    import torch
    cm = env.cm
    n = int(qpos.shape[0])
    k = env.kinematics_at(envs=torch.arange(n, dtype=torch.int32, device=qpos.device), qpos=qpos.contiguous(), qvel=qvel.contiguous(),
                          fields=("site_xpos", "status"))
    goal = target_pos + (qpos[:, None, cm.nlink:cm.nlink + 3] if follow_cube else 0.0)
    return (k["site_xpos"] - goal).norm(dim=-1)[:, _present(cm)]


def plan(env, st, horizon=8, iters=5, alphas=(1.0, 0.5, 0.25), cube=False, device_cost=False, fused=False, device_backward=False, box=None,
         seed=3):
    """The example's loop from the states st (qpos, qvel, warm, ctrl: [n, ..] tensors; problem e is env e).  Returns dict(res: ilqr's
    result, cost: the mean accepted cost per iteration, start, end: the median site-to-target distance before the plan and after its
    controls are rolled out, target_pos [n, 2, 3])."""
    import torch
    cm = env.cm
    n, T = int(st["qpos"].shape[0]), horizon
    dev, f64 = st["qpos"].device, torch.float64
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    if cube:
        target = torch.zeros((n, 2, 3), dtype=f64, device=dev)
    else:
        sx = env.kinematics_at(envs=idx, qpos=st["qpos"], qvel=st["qvel"], fields=("site_xpos", "status"))["site_xpos"]
        target = sx + torch.from_numpy(np.random.default_rng(seed).uniform(-0.05, 0.05, (n, 2, 3))).to(dev)
    wq = torch.zeros(2 * cm.nv, dtype=f64, device=dev)
    wq[cm.nv:cm.nv + cm.nlink] = W_VEL
    smooth = ilqr.QuadraticCost(cm, st["qpos"], torch.zeros((n, cm.nv), dtype=f64, device=dev), wq,
                                torch.full((cm.nu,), W_CTRL, dtype=f64, device=dev), wq)
    site = ilqr.SiteCost(env, target, w_pos=W_POS, wf_pos=WF_POS, follow_cube=cube, device=device_cost)
    cost = ilqr.SumCost(smooth, site)
    guess = st["ctrl"][:, None, :].repeat(1, T, 1)
    res = ilqr.ilqr(env, None, st["qpos"], st["qvel"], st["warm"], guess, cost, iters=iters, alphas=alphas, fused=fused,
                    device_backward=device_backward, **(box or {}))
    roll = env.rollout(envs=idx, qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=res["ctrl"], fields=("qpos", "qvel", "status"))
    start = site_distance(env, st["qpos"], st["qvel"], target, cube)
    end = site_distance(env, roll["qpos"][:, -1], roll["qvel"][:, -1], target, cube)
    return {"res": res, "cost": res["cost"].mean(dim=1).tolist(), "start": float(start.median()), "end": float(end.median()),
            "target_pos": target}


def main(argv=None):
    """Returns the printed record as a dict: "cost" the mean accepted cost per iteration (entry 0 the initial guess's), "start" and
    "end" the median site-to-target distance before and after the plan."""
    import torch
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.model import ctrl_range
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArmQPos", choices=["KManipSoloArmQPos", "KManipDualArmQPos"])
    ap.add_argument("--num-envs", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--alphas", type=float, nargs="+", default=[1.0, 0.5, 0.25])
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--cube", action="store_true", help="the target is the cube's position (follow_cube, zero offset)")
    ap.add_argument("--device-cost", action="store_true", help="the site cost and its derivatives in one launch: KManipEnvHip.site_cost (kmanip_site_cost)")
    ap.add_argument("--fused", action="store_true", help="linearise with KManipEnvHip.transition_fd (kmanip_transition_fd)")
    ap.add_argument("--device-backward", action="store_true", help="the backward pass in one launch: KManipEnvHip.lqr_backward (kmanip_lqr_backward)")
    ap.add_argument("--box", default=None, help="plan inside a box on ctrl: `ctrlrange` (the model's) or a half-width around the initial ctrl")
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    env.k_reset()
    st = env.state_tensors()
    box = None
    if args.box == "ctrlrange":
        box = dict(zip(("ctrl_lo", "ctrl_hi"), ctrl_range(env.cm, env.device)))
    elif args.box is not None:
        box = dict(ctrl_lo=st["ctrl"] - float(args.box), ctrl_hi=st["ctrl"] + float(args.box))
    out = plan(env, st, horizon=args.horizon, iters=args.iters, alphas=args.alphas, cube=args.cube, device_cost=args.device_cost,
               fused=args.fused, device_backward=args.device_backward, box=box, seed=args.seed)
    after = env.state_tensors()
    assert all(torch.equal(st[k], after[k]) for k in st)                                 # the handle was only read
    for it, c in enumerate(out["cost"]):
        print("iteration %d: mean cost %.6f" % (it, c))
    print("median site-to-target distance: %.4f -> %.4f m" % (out["start"], out["end"]))
    rec = {"env": args.env, "num_envs": args.num_envs, "horizon": args.horizon, "cube": bool(args.cube), "device_cost": bool(args.device_cost),
           "fused": bool(args.fused), "device_backward": bool(args.device_backward), "box": args.box, "cost": out["cost"],
           "accepted": out["res"]["accepted"].cpu().tolist(), "start": out["start"], "end": out["end"]}
    print(json.dumps(rec))
    env.k_close()
    return rec


if __name__ == "__main__":
    main()
