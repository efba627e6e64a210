#!/usr/bin/env python3
"""Domain randomisation on the device: every env of one SoloArm handle gets its own cube mass, cube friction, cube friction loss
and servo stiffness, redrawn at each of its resets (kmanip_set_env_param_ranges; the auto-reset inside the step draws them, the
host never sees the episode boundary).  Steps the batch with sampled actions (kmanip_sample_action) with and without ranges on
the same handle and prints env steps/s of both.

    python -m gym_kmanip_amd.examples.domain_randomization [--env KManipSoloArm] [--num-envs 4096] [--steps 256] [--warmup 32]
                                                           [--chunk K]   (K control steps per launch: kmanip_step_chunk)
"""
import argparse
import json
import time

from gym_kmanip_amd import env_hip


def _rate(env, steps, warmup, chunk=1):
    import torch
    acts = torch.empty((chunk, env.num_envs, env.cm.act_dim), dtype=torch.float32, device=env.device)
    env.k_reset()
    nw, ns = -(-warmup // chunk), -(-steps // chunk)
    for k in range(nw + ns):
        if k == nw:
            torch.cuda.synchronize(env.device)
            t0 = time.perf_counter()
        for j in range(chunk):
            env.sample_action(acts[j], ahead=j)
        if chunk == 1:
            env.step_flat(acts[0])
        else:
            env.step_chunk(acts)
    torch.cuda.synchronize(env.device)
    return env.num_envs * ns * chunk / (time.perf_counter() - t0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArm")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=1)
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    d = env.cm.desc
    ranges = {"cube_mass": (0.5 * d.cube_mass, 2.0 * d.cube_mass), "cube_friction": (0.3, 1.5),
              "cube_frictionloss": (0.0, 2.0 * d.cube_frictionloss), "kp_scale": (0.5, 1.5)}
    off = _rate(env, args.steps, args.warmup, args.chunk)
    env.set_env_param_ranges(**ranges)
    on = _rate(env, args.steps, args.warmup, args.chunk)
    p = {k: v.float() for k, v in env.get_env_params().items()}
    env.clear_env_params()
    off2 = _rate(env, args.steps, args.warmup, args.chunk)
    print(json.dumps({"env": args.env, "num_envs": args.num_envs, "steps": args.steps, "chunk": args.chunk,
                      "env_steps_per_s_ranges_off": round(0.5 * (off + off2)), "env_steps_per_s_ranges_on": round(on),
                      "ratio_on_off": round(on / (0.5 * (off + off2)), 4),
                      "drawn": {k: [round(float(v.min()), 4), round(float(v.max()), 4)] for k, v in p.items()}}))
    env.k_close()


if __name__ == "__main__":
    main()
