#!/usr/bin/env python3
"""An on-policy rollout buffer with a learned policy evaluated on the device between steps.

    python -m gym_kmanip_amd.examples.actor_rollout [--env KManipSoloArm] [--num-envs 4096] [--steps 256] [--hidden 64 64] [--torch]

A random tanh actor (gym_kmanip_amd.actor.Actor) and a critic of the same shape drive every env for `steps` control steps through
KManipEnvHip.collect: per step one kmanip_actor launch for the policy, one for the critic and one kmanip_step, all on one stream with
no host synchronisation; the noise of every action is a function of (seed, env, episode, step).  Printed: env steps per second over
the whole buffer (one synchronisation at the end) and the mean reward.  With --torch the same parameters run as a torch float32
program between step_flat calls (Actor.torch_eval; its noise comes from torch's global generator), for comparison."""
import argparse
import json
import time

from gym_kmanip_amd import env_hip
from gym_kmanip_amd.actor import Actor


def main(argv=None):
    """Returns the printed record as a dict."""
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArm")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--hidden", type=int, nargs=2, default=(64, 64))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--torch", action="store_true", help="the same policy as a torch module between step_flat calls")
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    env.k_reset()
    actor = Actor(env, hidden=tuple(args.hidden), activation="tanh", seed=args.seed)
    critic = Actor(env, hidden=tuple(args.hidden), activation="tanh", out_dim=1, seed=args.seed + 1)
    actor.log_std.fill_(-0.5)
    T, n = args.steps, args.num_envs
    if args.torch:
        reward = torch.empty((T, n), dtype=torch.float64, device=env.device)
        obs = env.observe()[0]
        actor.torch_eval(obs), critic.torch_eval(obs)           # (the BLAS library's start-up outside the clock)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            act, _, _ = actor.torch_eval(obs)
            critic.torch_eval(obs)
            obs, rew, _ = env.step_flat(act)
            reward[t].copy_(rew)
    else:
        buf = env.collect(actor, 2, critic=critic)              # (allocations and first launches outside the clock)
        buf = {k: torch.empty((T + v.shape[0] - 2,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device) for k, v in buf.items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reward = env.collect(actor, T, critic=critic, out=buf)["reward"]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = {"env": args.env, "num_envs": n, "steps": T, "policy": "torch" if args.torch else "kmanip_actor", "hidden": list(args.hidden),
           "env_steps_per_s": round(T * n / dt, 1), "mean_reward": float(reward.mean())}
    print(json.dumps(rec))
    env.k_close()
    return rec


if __name__ == "__main__":
    main()
