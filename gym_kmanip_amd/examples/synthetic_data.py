#!/usr/bin/env python3
"""Scripted data generation on the device -- the reference's examples/2_synthetic_data.py (random action with `eer_pos`
overwritten by the unit vector from the right end effector to the cube) for a whole batch, without the host in the loop:
the policy is a kernel (`kmanip_scripted_action`), the step takes its device action matrix, the logger's rings are device
tensors.  A *Vision id also logs its camera frames (the reference's log_h5py.cam / step): the heuristic acts on the state, so
the frames of step t are rendered BEHIND the steps (pipeline.RenderBehind: a qpos snapshot and a second stream) and reach the
logger while step t + 1 runs -- `--render-in-sequence` renders them before the next step instead.  `--segmentation` logs the
per-pixel class labels of every frame next to it (`observations/segmentation/<camera>`), rendered by the frames' own launch.
`--links` draws the arm links as capsules in the frames and the labels (KManipEnvHip.set_render_links).
`--points` (any id) logs one world-frame point cloud of the right gripper camera per step (KManipEnvHip.render_points: float32
[h, w, 3], the back-projection of the camera's depth image; with `--links` the capsules are in it) for the logged envs, one
`points_grip_r_<episode>.npy` [steps, envs, h, w, 3] per episode next to the episode files.

    python -m gym_kmanip_amd.examples.synthetic_data [--env KManipSoloArm] [--num-envs 4096] [--episodes 10] [--log-envs 0 1 2 3]
                                                     [--segmentation] [--links] [--points]
"""
import argparse
import os
import time

import numpy as np

from gym_kmanip_amd import env_hip
from gym_kmanip_amd.episode_log import EpisodeLogger
from gym_kmanip_amd.model import MAX_EPISODE_STEPS


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArm")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--log-envs", type=int, nargs="*", default=[0, 1, 2, 3])
    ap.add_argument("--log-dir", default=os.path.join(os.getcwd(), "data", "sim_synth"))
    ap.add_argument("--render-in-sequence", action="store_true", help="*Vision ids: render every step's frames before the next step starts")
    ap.add_argument("--segmentation", action="store_true", help="*Vision ids: also log uint8 class labels per pixel (KM_SEG_*)")
    ap.add_argument("--links", action="store_true", help="*Vision ids: draw the arm links as capsules in the frames and labels (set_render_links)")
    ap.add_argument("--points", action="store_true", help="log a world-frame point cloud of the right gripper camera per step (render_points)")
    args = ap.parse_args(argv)
    import torch
    os.makedirs(args.log_dir, exist_ok=True)
    env = env_hip.make(args.env, num_envs=args.num_envs, auto_reset=False)
    if args.links and (env.cm.cameras or args.points):
        env.set_render_links(True)                                               # the frames and labels show the arm, not only the finger tips
        env.set_depth_links(args.points)                                         # ... and so does the point cloud's depth ray cast
    q = env.cm.nlink
    log = EpisodeLogger(args.log_dir, args.num_envs, q, env.cm.act_dim, device=env.obs.device, env_ids=args.log_envs,
                        info={"sim": True, "env": args.env, "policy": "toward-cube heuristic"})
    from gym_kmanip_amd.model import CAMERAS
    from gym_kmanip_amd.pipeline import RenderBehind
    for name in env.cm.cameras:                                                  # (none unless the id is a *Vision one)
        log.cam(CAMERAS[name], labels=args.segmentation)
    pts = ("grip_r", CAMERAS["grip_r"].h, CAMERAS["grip_r"].w, "world") if args.points else None
    sel = torch.as_tensor(args.log_envs, dtype=torch.long, device=env.obs.device)
    pts_ring = torch.zeros((MAX_EPISODE_STEPS, len(args.log_envs), pts[1], pts[2], 3), dtype=torch.float32, device=env.obs.device) if pts else None
    behind = (RenderBehind(env, segmentation=args.segmentation, points=pts)
              if ((env.cm.cameras or pts) and not args.render_in_sequence) else None)

    def late(due):                                                               # the frames (and the point cloud) of an earlier step
        imgs = behind.images(due[0])
        if env.cm.cameras:
            log.late_images(due[1], imgs)
        if pts:
            pts_ring[due[1]].copy_(imgs["points"].index_select(0, sel))
    gen = torch.Generator(device=env.obs.device); gen.manual_seed(0)
    t0 = time.time()
    closest = None
    for ep in range(args.episodes):
        env.k_reset()
        due = None                                                               # (step index of the renderer, row of the logger)
        for _ in range(MAX_EPISODE_STEPS):
            act = torch.rand((args.num_envs, env.cm.act_dim), generator=gen, device=env.obs.device) * 2 - 1    # action_space.sample()
            env.scripted_action(act)                                                                           # eer_pos <- unit(cube - eer)
            env.step_flat(act)
            if behind is not None:
                k = behind.after_step()                                          # this step's frames: rendering from now on
                if due is not None:
                    late(due)                                                    # the previous step's frames have had a whole step
                due = (k, log.step(act, env.obs[:, :q], env.obs[:, q:2 * q], images_later=bool(env.cm.cameras)))
            else:
                t = log.step(act, env.obs[:, :q], env.obs[:, q:2 * q], images=env.render_cameras(segmentation=args.segmentation) if env.cm.cameras else None)
                if pts:
                    pts_ring[t].copy_(env.render_points(*pts[:3], frame=pts[3]).index_select(0, sel))
        if due is not None:
            late(due)
        paths = log.end_episode()
        if pts:
            np.save(os.path.join(args.log_dir, "points_grip_r_%04d.npy" % ep), pts_ring.cpu().numpy())
        closest = float(env.reward.max())
    torch.cuda.synchronize()
    dt = time.time() - t0
    n = args.episodes * MAX_EPISODE_STEPS * args.num_envs
    print(f"{n} env steps in {dt:.2f} s ({n / dt:.0f} env steps/s incl. logging); best final reward {closest:.3f}; last files: {paths[:2]}")
    env.k_close()
    return args.log_dir


if __name__ == "__main__":
    main()
