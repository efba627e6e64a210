#!/usr/bin/env python3
"""Cost of kmanip_forces beside kmanip_observe and kmanip_step, measured with HIP events in one process on
one GPU:

    python tests/tools/forces_cost.py [--reps 100] [--out <file>]

KManipSoloArm at 4096 envs and KManipDualArm at 8192 envs, after a reset and 12 sampled steps.  After WARM untimed rounds, `--reps`
rounds; every round takes one sampled step first (untimed: the states stay those of a natural rollout) and then times each phase
as ONE call between two events of its own -- forces with every field, forces with the three fields the Gymnasium shell asks for,
observe, step -- interleaved round by round so that clock and box drift hit all of them alike.  An interval holds the call as the
stream sees it: the kernel, the event pair (about 5 us) and what of the Python wrapper's checks the GPU has to wait for; for
kernel times run this tool under a kernel trace, in a run of its own.  Reported: mean / median / min / max in us and the ratios
forces / step and forces / observe.  There is no pass bar: nobody had measured this before."""
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
        full = env.forces()
        shell = env.forces(fields=("contact_force", "contact_bit", "qfrc_actuator"))
        phases = [("kmanip_forces, every field", lambda: env.forces(out=full)),
                  ("kmanip_forces, 3 fields", lambda: env.forces(out=shell)),
                  ("kmanip_observe", lambda: env.observe()),
                  ("kmanip_step", lambda: env.step_flat(act))]
        t = {name: [] for name, _ in phases}
        contacts = 0.0
        for k in range(WARM + args.reps):
            env.step_flat(env.sample_action())
            env.sample_action(act)
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
            if k >= WARM:
                contacts += float((full["contact_bit"] >= 0).sum()) / n
        assert not full["status"].any()
        emit("# library %s, %s, %d envs, %d timed rounds after %d warm-up rounds, %.2f contacts per env on average"
             % (env.L.kmanip_version().decode(), env_id, n, args.reps, WARM, contacts / args.reps))
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-14s %-28s mean %8.1f us  median %8.1f  min %8.1f  max %8.1f"
                 % (env_id, name, mean[name], statistics.median(t[name]), min(t[name]), max(t[name])))
        emit("%-14s forces / step = %.3f   forces / observe = %.1f" % (env_id, mean["kmanip_forces, every field"] / mean["kmanip_step"],
                                                                      mean["kmanip_forces, every field"] / mean["kmanip_observe"]))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
