#!/usr/bin/env python3
"""Applied forces (KManipEnvHip.bind_applied_force: MuJoCo's data.qfrc_applied) in two uses.  Nothing crosses PCIe inside either loop.

    python -m gym_kmanip_amd.examples.applied_forces --mode gravity [--env KManipSoloArmQPos] [--num-envs 256] [--steps 8]
    python -m gym_kmanip_amd.examples.applied_forces --mode push [--every 4] [--newtons 1.0] [--steps 32] [--seed 3]

--mode gravity   gravity (and Coriolis) compensation on a *QPos id with zero actions.  A zero action re-targets every position servo
                 at the joint's current position, so the servos hold nothing and the arm sinks under its own weight.  Every step
                 the joint columns of kinematics()["qfrc_bias"] are copied into the bound tensor: the applied force cancels the
                 bias force and the arm stays.  Prints the arm's largest joint drift from the home pose with and without the
                 binding.
--mode push      disturbance: in one step of every `every` the cube of every env gets a horizontal force of `newtons` in a random
                 direction (applied.cube_wrench); in the other steps the tensor is zero.  Prints the median horizontal cube
                 displacement with and without the pushes.
"""
import argparse
import json
import math

from gym_kmanip_amd import applied, env_hip


def gravity_drift(env, steps, compensate):
    """Largest |qpos - home| over the arm joints after `steps` zero-action steps from a reset."""
    import torch
    cm = env.cm
    nl = cm.nlink
    env.k_reset()
    home = env.state_tensors()["qpos"][:, :nl].clone()
    act = torch.zeros((env.num_envs, cm.act_dim), dtype=torch.float32, device=env.device)
    tau = env.new_applied_force() if compensate else env.bind_applied_force(None)
    k = None
    for _ in range(steps):
        if compensate:
            k = env.kinematics(out=k, fields=("qfrc_bias",))
            tau[:, :nl] = k["qfrc_bias"][:, :nl]
        env.step_flat(act)
    drift = (env.state_tensors()["qpos"][:, :nl] - home).abs().max()
    env.bind_applied_force(None)
    return float(drift)


def push_displacement(env, steps, every, newtons, seed, push):
    """Median horizontal distance of the cube from its spawn position after `steps` zero-action steps."""
    import torch
    cm = env.cm
    nl = cm.nlink
    env.k_reset()
    start = env.state_tensors()["qpos"][:, nl:nl + 2].clone()
    act = torch.zeros((env.num_envs, cm.act_dim), dtype=torch.float32, device=env.device)
    tau = env.new_applied_force()
    gen = torch.Generator(device=env.device).manual_seed(seed)
    force = torch.zeros((env.num_envs, 3), dtype=torch.float64, device=env.device)
    state = None
    for k in range(steps):
        tau.zero_()
        if push and k % every == 0:
            phi = torch.rand((env.num_envs,), generator=gen, dtype=torch.float64, device=env.device) * (2.0 * math.pi)
            force[:, 0] = newtons * torch.cos(phi)
            force[:, 1] = newtons * torch.sin(phi)
            state = env.state_tensors(out=state)
            applied.cube_wrench(cm, state["qpos"], force=force, out=tau)
        env.step_flat(act)
    moved = (env.state_tensors()["qpos"][:, nl:nl + 2] - start).norm(dim=1).median()
    env.bind_applied_force(None)
    return float(moved)


def main(argv=None):
    """Returns {"without": ..., "with": ...}: the drift in rad (gravity) or the displacement in metres (push)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("gravity", "push"), default="gravity")
    ap.add_argument("--env", default="KManipSoloArmQPos")
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--newtons", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed, auto_reset=False)
    if args.mode == "gravity":
        if not ("q_pos_r" in env.cm.act_slices or "q_pos_l" in env.cm.act_slices):
            raise SystemExit("%s has no joint-delta action key (q_pos_r / q_pos_l): use a *QPos id" % args.env)
        steps = 8 if args.steps is None else args.steps
        out = {"without": gravity_drift(env, steps, False), "with": gravity_drift(env, steps, True)}
        print(json.dumps({"mode": "gravity", "env": args.env, "num_envs": args.num_envs, "steps": steps,
                          "arm_drift_rad_without": out["without"], "arm_drift_rad_with": out["with"]}))
    else:
        steps = 32 if args.steps is None else args.steps
        out = {"without": push_displacement(env, steps, args.every, args.newtons, args.seed, False),
               "with": push_displacement(env, steps, args.every, args.newtons, args.seed, True)}
        print(json.dumps({"mode": "push", "env": args.env, "num_envs": args.num_envs, "steps": steps, "every": args.every,
                          "newtons": args.newtons, "cube_displacement_m_without": round(out["without"], 6),
                          "cube_displacement_m_with": round(out["with"], 6)}))
    env.k_close()
    return out


if __name__ == "__main__":
    main()
