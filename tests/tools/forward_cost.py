#!/usr/bin/env python3
"""Cost of kmanip_forward beside kmanip_forces and kmanip_step, measured with HIP events in one process on one
GPU:

    python tests/tools/forward_cost.py [--reps 100] [--out profiles/forward_cost.txt]

KManipSoloArm at 4096 envs and KManipDualArm at 8192 envs, after a reset and 12 sampled steps.  After WARM untimed rounds, `--reps`
rounds; every round takes one sampled step first (untimed: the states stay those of a natural rollout) and then times each phase
as ONE call between two events of its own -- forces; forward with identity rows (every input None); forward with identity rows
and every input given (the state read back, the warm start, a zero force: the applied-force build); forward with 8 x num_envs rows
(the state tiled eight times, env index given); forward_fd for the first 64 envs, all blocks (two forward launches and the torch
kernels that build the rows and the quotients); step -- interleaved round by round so that clock and box drift hit all of them
alike.  An interval holds the call as the stream sees it: the kernels, the event pair (about 5 us) and what of the Python wrapper's
checks the GPU has to wait for.  Reported: mean / median / min / max in us and the ratios to forces in the same run.  There is no
pass bar."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 10
CONFIGS = (("KManipSoloArm", 4096), ("KManipDualArm", 8192))
FD_ENVS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.derivatives import forward_fd
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for env_id, n in CONFIGS:
        env = env_hip.make(env_id, num_envs=n, seed=1)
        cm = env.cm
        env.k_reset()
        for _ in range(12):
            env.step_flat(env.sample_action())
        act = env.sample_action()
        full = env.forces()
        fwd = env.forward()
        st = env.state_tensors()
        zero = torch.zeros((n, cm.nv), dtype=torch.float64, device=env.device)
        idx8 = torch.arange(n, dtype=torch.int32, device=env.device).repeat(8)
        big = {k: st[k].repeat(8, 1) for k in ("qpos", "qvel", "ctrl", "warm")}
        out8 = env.forward(envs=idx8, **big)
        fd_idx = torch.arange(FD_ENVS, dtype=torch.int32, device=env.device)
        fd_rows = lambda: {k: st[k][:FD_ENVS] for k in ("qpos", "qvel", "ctrl")}
        phases = [("kmanip_forces", lambda: env.forces(out=full)),
                  ("kmanip_forward, identity rows", lambda: env.forward(out=fwd)),
                  ("kmanip_forward, every input given", lambda: env.forward(qpos=st["qpos"], qvel=st["qvel"], ctrl=st["ctrl"], warm=st["warm"],
                                                                             qfrc_applied=zero, out=fwd)),
                  ("kmanip_forward, 8 x num_envs rows", lambda: env.forward(envs=idx8, out=out8, **big)),
                  ("forward_fd, %d envs, all blocks" % FD_ENVS, lambda: forward_fd(env, envs=fd_idx, **fd_rows())),
                  ("kmanip_step", lambda: env.step_flat(act))]
        t = {name: [] for name, _ in phases}
        for k in range(WARM + args.reps):
            env.step_flat(env.sample_action())
            env.sample_action(act)
            env.state_tensors(out=st)
            for key in big:
                big[key].copy_(st[key].repeat(8, 1))
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        assert not full["status"].any() and not fwd["status"].any() and not out8["status"].any()
        emit("# library %s, %s, %d envs, %d timed rounds after %d warm-up rounds" % (env.L.kmanip_version().decode(), env_id, n, args.reps, WARM))
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-14s %-36s mean %8.1f us  median %8.1f  min %8.1f  max %8.1f"
                 % (env_id, name, mean[name], statistics.median(t[name]), min(t[name]), max(t[name])))
        m = mean["kmanip_forces"]
        emit("%-14s identity / forces = %.3f   every input given / forces = %.3f   8 x rows / forces = %.2f   forward_fd / forces = %.2f   "
             "forces / step = %.3f" % (env_id, mean["kmanip_forward, identity rows"] / m, mean["kmanip_forward, every input given"] / m,
                                     mean["kmanip_forward, 8 x num_envs rows"] / m, mean["forward_fd, %d envs, all blocks" % FD_ENVS] / m,
                                     m / mean["kmanip_step"]))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
