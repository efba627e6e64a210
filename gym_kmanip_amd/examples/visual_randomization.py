#!/usr/bin/env python3
"""Visual domain randomisation on the device: every env of one *Vision handle renders its camera set with its own cube, table,
robot and background colours, light terms and camera offset, redrawn for each episode (kmanip_set_visual_param_ranges; the render
kernels evaluate the draw from the episode counter).  Steps the batch with sampled actions and renders the id's cameras behind
the steps (pipeline.RenderBehind), with ranges off and then on for the same handle, and prints env steps/s of both.

    python -m gym_kmanip_amd.examples.visual_randomization [--env KManipSoloArmVision] [--num-envs 2048] [--steps 128]
                                                           [--warmup 16] [--save frames.npz]
"""
import argparse
import json
import time

import numpy as np

from gym_kmanip_amd import env_hip
from gym_kmanip_amd.pipeline import RenderBehind

RANGES = {"cube_rgb": (0.3, 1.0), "table_rgb": (0.05, 0.6), "robot_rgb": (0.3, 0.9), "background_rgb": (0.0, 0.4),
          "ambient": (0.2, 0.6), "headlight": (0.2, 0.6), "directional": (0.5, 1.5), "camera_offset": (-0.03, 0.03)}


def _rate(env, rb, steps, warmup):
    import torch
    act = torch.empty((env.num_envs, env.cm.act_dim), dtype=torch.float32, device=env.device)
    env.k_reset()
    for k in range(warmup + steps):
        if k == warmup:
            torch.cuda.synchronize(env.device)
            t0 = time.perf_counter()
        env.sample_action(act)
        env.step_flat(act)
        rb.after_step()
    torch.cuda.synchronize(env.device)
    return env.num_envs * steps / (time.perf_counter() - t0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArmVision")
    ap.add_argument("--num-envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="write the last images of a few envs (ranges off and on) to this .npz")
    args = ap.parse_args(argv)
    import torch
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    rb = RenderBehind(env)
    off = _rate(env, rb, args.steps, args.warmup)
    torch.cuda.synchronize(env.device)
    keep = min(4, env.num_envs)
    frames = {"off/" + k: v[:keep].cpu().numpy() for k, v in rb.images(rb.k - 1).items()}
    env.set_visual_param_ranges(**RANGES)
    on = _rate(env, rb, args.steps, args.warmup)
    torch.cuda.synchronize(env.device)
    frames.update({"on/" + k: v[:keep].cpu().numpy() for k, v in rb.images(rb.k - 1).items()})
    drawn = {k: [round(float(v.min()), 4), round(float(v.max()), 4)] for k, v in env.get_visual_params().items()}
    env.clear_visual_params()
    if args.save:
        np.savez_compressed(args.save, **frames)
    print(json.dumps({"env": args.env, "num_envs": args.num_envs, "steps": args.steps, "cameras": env.cm.cameras,
                      "env_steps_per_s_ranges_off": round(off), "env_steps_per_s_ranges_on": round(on),
                      "ratio_on_off": round(on / off, 4), "drawn": drawn}))
    env.k_close()


if __name__ == "__main__":
    main()
