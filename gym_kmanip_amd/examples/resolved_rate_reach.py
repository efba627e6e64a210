#!/usr/bin/env python3
"""Resolved-rate reaching with the device's own Jacobians (KManipEnvHip.kinematics): every hand moves its end-effector site to a
goal a few centimetres away, the controller written in torch on the tensors kmanip_kinematics returns.  Nothing crosses PCIe inside
the loop.

    python -m gym_kmanip_amd.examples.resolved_rate_reach [--env KManipSoloArmQPos] [--num-envs 256] [--steps 24] [--seed 3]

For a *QPos id (joint-delta actions).  The goal is each site's reset position plus an offset drawn uniformly in +-5 cm per axis.
Per arm and step, with Jp the site's 3 x k position Jacobian on the arm's arm_q_id columns:

    dq = Jp^T (Jp Jp^T + 1e-4 I)^-1 (goal - site_xpos),    action = clip(dq / q_pos_delta, -1, 1),    grip 0

(damped least squares: the step that moves the site straight at the goal, bounded near singular poses).  Prints the median
site-to-goal distance at the start and at the end.
"""
import argparse
import json

from gym_kmanip_amd import env_hip

DAMPING = 1e-4


def arm_columns(cm):
    """[(arm, action slice, dof ids)] of the arms the id's joint-delta keys drive."""
    out = []
    for a, (key, ids) in enumerate((("q_pos_r", cm.spec.q_id_r_mask), ("q_pos_l", cm.spec.q_id_l_mask))):
        if key in cm.act_slices:
            out.append((a, cm.act_slices[key], list(ids)))
    return out


def solve3(A, b):
    """x of A x = b for batched 3 x 3 systems [n, 3, 3], [n, 3] by the adjugate (cross products of the rows): plain tensor
    arithmetic, no solver library."""
    import torch
    r0, r1, r2 = A[:, 0], A[:, 1], A[:, 2]
    c0, c1, c2 = torch.cross(r1, r2, dim=-1), torch.cross(r2, r0, dim=-1), torch.cross(r0, r1, dim=-1)
    det = (r0 * c0).sum(-1, keepdim=True)
    return (c0 * b[:, 0:1] + c1 * b[:, 1:2] + c2 * b[:, 2:3]) / det


def resolved_rate_action(env, k, goal, act=None):
    """The action above for every env, from a kinematics() result with site_xpos and site_jacp; goal [n, 2, 3]."""
    import torch
    cm = env.cm
    if act is None:
        act = torch.zeros((env.num_envs, cm.act_dim), dtype=torch.float32, device=goal.device)
    eye = DAMPING * torch.eye(3, dtype=torch.float64, device=goal.device)
    for a, sl, ids in arm_columns(cm):
        Jp = k["site_jacp"][:, a][:, :, ids]
        y = solve3(Jp @ Jp.transpose(1, 2) + eye, goal[:, a] - k["site_xpos"][:, a])
        dq = (Jp.transpose(1, 2) @ y.unsqueeze(-1)).squeeze(-1)
        act[:, sl] = (dq / cm.desc.q_pos_delta).clamp(-1.0, 1.0).to(torch.float32)
    return act


def median_distance(env, k, goal):
    arms = [a for a, _, _ in arm_columns(env.cm)]
    return float((k["site_xpos"][:, arms] - goal[:, arms]).norm(dim=-1).median())


def main(argv=None):
    """Returns {"start": median site-to-goal distance after the reset, "end": after the last step} in metres."""
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArmQPos")
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    if not arm_columns(env.cm):
        raise SystemExit("%s has no joint-delta action key (q_pos_r / q_pos_l): use a *QPos id" % args.env)
    env.k_reset()
    k = env.kinematics(fields=("site_xpos", "site_jacp"))
    gen = torch.Generator().manual_seed(args.seed)
    offset = (torch.rand((args.num_envs, 2, 3), generator=gen, dtype=torch.float64) - 0.5) * 0.1
    goal = k["site_xpos"] + offset.to(k["site_xpos"].device)
    start = median_distance(env, k, goal)
    act = None
    for _ in range(args.steps):
        act = resolved_rate_action(env, k, goal, act)
        env.step_flat(act)
        env.kinematics(out=k)
    out = {"start": start, "end": median_distance(env, k, goal)}
    print(json.dumps({"env": args.env, "num_envs": args.num_envs, "steps": args.steps, "median_distance_start_m": round(out["start"], 5),
                      "median_distance_end_m": round(out["end"], 5)}))
    env.k_close()
    return out


if __name__ == "__main__":
    main()
