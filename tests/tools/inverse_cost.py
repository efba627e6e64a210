#!/usr/bin/env python3
"""Cost of kmanip_inverse beside kmanip_forces, kmanip_observe and kmanip_step, measured with HIP events in one
process on one GPU:

    python tests/tools/inverse_cost.py [--reps 100] [--out <file>]

KManipSoloArm at 4096 envs and KManipDualArm at 8192 envs, after a reset and 12 sampled steps.  After WARM untimed rounds, `--reps`
rounds; every round takes one sampled step first (untimed: the states stay those of a natural rollout) and then times each phase
as ONE call between two events of its own -- inverse with every field at the forward solution's qacc, inverse with qfrc_inverse
alone, inverse with the state passed by the caller, forces with every field, observe, step -- interleaved round by round so that
clock and box drift hit all of them alike.  An interval holds the call as the stream sees it: the kernel, the event pair (about
5 us) and what of the Python wrapper's checks the GPU has to wait for.  Reported: mean / median / min / max in us and the ratios
inverse / forces, inverse / step and inverse / observe.  There is no pass bar: nobody had measured this before."""
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
        qacc = full["qacc"]
        st = env.state_tensors()
        inv = env.inverse(qacc)
        one = env.inverse(qacc, fields=("qfrc_inverse",))
        phases = [("kmanip_inverse, every field", lambda: env.inverse(qacc, out=inv)),
                  ("kmanip_inverse, qfrc_inverse", lambda: env.inverse(qacc, out=one)),
                  ("kmanip_inverse, caller's state", lambda: env.inverse(qacc, qpos=st["qpos"], qvel=st["qvel"], out=inv)),
                  ("kmanip_forces, every field", lambda: env.forces(out=full)),
                  ("kmanip_observe", lambda: env.observe()),
                  ("kmanip_step", lambda: env.step_flat(act))]
        t = {name: [] for name, _ in phases}
        for k in range(WARM + args.reps):
            env.step_flat(env.sample_action())
            env.sample_action(act)
            env.state_tensors(out=st)
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        assert not full["status"].any() and not inv["status"].any()
        emit("# library %s, %s, %d envs, %d timed rounds after %d warm-up rounds" % (env.L.kmanip_version().decode(), env_id, n, args.reps, WARM))
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-14s %-32s mean %8.1f us  median %8.1f  min %8.1f  max %8.1f"
                 % (env_id, name, mean[name], statistics.median(t[name]), min(t[name]), max(t[name])))
        m = mean["kmanip_inverse, every field"]
        emit("%-14s inverse / forces = %.3f   inverse / step = %.3f   inverse / observe = %.2f"
             % (env_id, m / mean["kmanip_forces, every field"], m / mean["kmanip_step"], m / mean["kmanip_observe"]))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
