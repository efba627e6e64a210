#!/usr/bin/env python3
"""Cost of a bound applied force (kmanip_bind_applied_force), measured with HIP events in one process on one GPU:

    python tests/tools/applied_force_cost.py [--steps 100] [--out <file>]

KManipSoloArm at 4096 envs and KManipDualArm at 8192 envs, after a reset and 12 sampled steps.  ONE handle, the buffer unbound and
bound in alternation, three blocks of `--steps` sampled steps each way after WARM untimed steps.  The bound buffer holds zeros, which
change no bit of the step (tests/test_applied_force_gpu.py): both modes walk the same trajectory, so the blocks differ only in the
kernel that runs (k_step / k_step_frc) and its nv doubles per env of extra reads.  Every step is ONE step_flat call between two events
of its own (the kernel, the event pair of about 5 us and what of the wrapper's checks the GPU waits for); a block's wall time is taken
around the whole block with a synchronisation at each end.  Reported per block: env steps / s from the wall time and the mean / median
step interval in us; then the ratio bound / unbound of the three-block means.  There is no pass bar: nobody had measured this before."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 20
BLOCKS = 3
CONFIGS = (("KManipSoloArm", 4096), ("KManipDualArm", 8192))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for env_id, n in CONFIGS:
        env = env_hip.make(env_id, num_envs=n, seed=1)
        env.k_reset()
        zeros = torch.zeros((n, env.cm.nv), dtype=torch.float64, device=env.device)
        act = env.sample_action()
        for _ in range(12 + WARM):
            env.step_flat(env.sample_action(act))
        emit("# library %s, %s, %d envs, %d blocks of %d steps per mode after %d warm-up steps"
             % (env.L.kmanip_version().decode(), env_id, n, BLOCKS, args.steps, WARM))
        mean = {"unbound": [], "bound": []}
        for blk in range(BLOCKS):
            for mode in ("unbound", "bound"):
                env.bind_applied_force(zeros if mode == "bound" else None)
                env.step_flat(env.sample_action(act))                    # (the first launch of the other kernel: untimed)
                ev = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    env.sample_action(act)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); env.step_flat(act); b.record()
                    ev.append((a, b))
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                us = [a.elapsed_time(b) * 1e3 for a, b in ev]
                mean[mode].append(statistics.fmean(us))
                emit("%-14s block %d %-8s %10.0f env steps/s   step interval mean %8.1f us  median %8.1f  min %8.1f  max %8.1f"
                     % (env_id, blk, mode, n * args.steps / wall, statistics.fmean(us), statistics.median(us), min(us), max(us)))
        u, b = statistics.fmean(mean["unbound"]), statistics.fmean(mean["bound"])
        emit("%-14s step interval bound / unbound = %.4f   (unbound blocks' own spread: %.4f)"
             % (env_id, b / u, (max(mean["unbound"]) - min(mean["unbound"])) / u))
        assert not zeros.any()
        env.bind_applied_force(None)
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
