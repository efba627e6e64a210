#!/usr/bin/env python3
"""Cost of kmanip_kinematics beside kmanip_observe, kmanip_forces and kmanip_step, measured with HIP events
in one process on one GPU:

    python tests/tools/kinematics_cost.py [--reps 100] [--out <file>]

KManipSoloArm at 4096 envs and KManipDualArm at 8192 envs, after a reset and 12 sampled steps.  After WARM untimed rounds, `--reps`
rounds; every round takes one sampled step first (untimed: the states stay those of a natural rollout) and then times each phase
as ONE call between two events of its own -- kinematics with every field, kinematics with the two fields the Gymnasium shell asks
for, observe, forces with every field, step -- interleaved round by round so that clock and box drift hit all of them alike.  An
interval holds the call as the stream sees it: the kernel, the event pair (about 5 us) and what of the Python wrapper's checks the
GPU has to wait for.  Reported: mean / median / min / max in us and the ratios kinematics / step, / forces and / observe.  There is
no pass bar: nobody had measured this before."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 10
CONFIGS = (("KManipSoloArm", 4096), ("KManipDualArm", 8192))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
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
        for _ in range(12):
            env.step_flat(env.sample_action())
        act = env.sample_action()
        full = env.kinematics()
        shell = env.kinematics(fields=("site_xpos", "site_xmat"))
        forces = env.forces()
        phases = [("kmanip_kinematics, every field", lambda: env.kinematics(out=full)),
                  ("kmanip_kinematics, 2 fields", lambda: env.kinematics(out=shell)),
                  ("kmanip_observe", lambda: env.observe()),
                  ("kmanip_forces, every field", lambda: env.forces(out=forces)),
                  ("kmanip_step", lambda: env.step_flat(act))]
        t = {name: [] for name, _ in phases}
        for k in range(WARM + args.reps):
            env.step_flat(env.sample_action())
            env.sample_action(act)
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        assert not full["status"].any()
        nbytes = sum(v.numel() * v.element_size() for v in full.values())
        emit("# library %s, %s, %d envs, %d timed rounds after %d warm-up rounds, %.1f MB written per full call"
             % (env.L.kmanip_version().decode(), env_id, n, args.reps, WARM, nbytes / 1e6))
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-14s %-32s mean %8.1f us  median %8.1f  min %8.1f  max %8.1f"
                 % (env_id, name, mean[name], statistics.median(t[name]), min(t[name]), max(t[name])))
        kin = mean["kmanip_kinematics, every field"]
        emit("%-14s kinematics / step = %.3f   kinematics / forces = %.2f   kinematics / observe = %.1f   2 fields / observe = %.1f"
             % (env_id, kin / mean["kmanip_step"], kin / mean["kmanip_forces, every field"], kin / mean["kmanip_observe"],
                mean["kmanip_kinematics, 2 fields"] / mean["kmanip_observe"]))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
