#!/usr/bin/env python3
"""Cost of the point-cloud render against the depth render (profiles/points_cost.txt is this tool's output),
measured with HIP events in one process on one GPU:

    python tests/tools/points_cost.py [--reps 40]

Two shapes -- KManipSoloArm, 2048 envs x 64 x 64 on grip_r (BASELINE config 5's image) and 256 envs x 480 x 640 on head -- each
with the depth flag off (the scene without capsules) and on (the default capsule list).  Per shape and flag, after WARM launches,
`--reps` launches of each of: render_depth (the kernels of the parent commit, untouched), render_points in the camera frame, in the
world frame, and in the world frame with depth_out; every launch between two events of its own, the phases interleaved launch by
launch so that clock and box drift hit all of them alike.  Also timed the same way: a plain fill (Tensor.zero_) of the points buffer
(12 bytes per pixel), the store traffic the depth render does not have.  The report: median / min / max per phase in us, the ratio
to render_depth, and the difference to render_depth next to the fill."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 4
SHAPES = [("grip_r", 2048, 64, 64), ("head", 256, 480, 640)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip
    for cam, n, h, w in SHAPES:
        env = env_hip.make("KManipSoloArm", num_envs=n, seed=1)
        env.k_reset()
        for _ in range(args.steps):
            env.step_flat(env.sample_action())
        env.set_render_links(True)
        depth = torch.empty((n, h, w), dtype=torch.float32, device=env.device)
        xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device=env.device)
        phases = [("render_depth", lambda: env.render_depth(cam, h, w, out=depth)),
                  ("render_points camera", lambda: env.render_points(cam, h, w, frame="camera", out=xyz)),
                  ("render_points world", lambda: env.render_points(cam, h, w, frame="world", out=xyz)),
                  ("render_points world + depth_out", lambda: env.render_points(cam, h, w, frame="world", out=xyz, depth_out=depth)),
                  ("fill of the points buffer", lambda: xyz.zero_())]
        print("# library %s, KManipSoloArm, %s, %d envs x %d x %d, %d capsules, %d timed launches per phase after %d warm-up launches"
              % (env.L.kmanip_version().decode(), cam, n, h, w, len(env.get_render_links()), args.reps, WARM))
        for on in (False, True):
            env.set_depth_links(on)
            t = {name: [] for name, _ in phases}
            for k in range(WARM + args.reps):
                for name, f in phases:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); f(); b.record()
                    b.synchronize()
                    if k >= WARM:
                        t[name].append(a.elapsed_time(b) * 1e3)
            med = {name: statistics.median(v) for name, v in t.items()}
            base, fill = med["render_depth"], med["fill of the points buffer"]
            for name, _ in phases:
                extra = "" if name in ("render_depth", "fill of the points buffer") else "  x %.2f of render_depth, + %.1f us (fill %.1f us)" % (
                    med[name] / base, med[name] - base, fill)
                print("%-7s links %-3s %-34s median %8.1f us  min %8.1f  max %8.1f%s"
                      % (cam, "on" if on else "off", name, med[name], min(t[name]), max(t[name]), extra))
            gb = 12.0 * n * h * w / 1e9
            print("%-7s links %-3s points buffer %.3f GB: fill at %.2f TB/s" % (cam, "on" if on else "off", gb, gb / fill * 1e3))
        env.k_close()
        del depth, xyz


if __name__ == "__main__":
    main()
