#!/usr/bin/env python3
"""Cost of kmanip_forward_fd beside the torch forward_fd it fuses and beside its floor, measured with HIP
events in one process on one GPU, tests/tools/forward_cost.py's protocol:

    python tests/tools/forward_fd_cost.py [--reps 100] [--out profiles/forward_fd_cost.txt]

KManipSoloArm at 4096 envs and KManipDualArm at 8192 envs, after a reset and 12 sampled steps; the rows are the first 64 envs' states,
all four `wrt` blocks, the default `of`.  After WARM untimed rounds, `--reps` rounds; every round takes one sampled step first
(untimed) and then times each phase as ONE call between two events of its own, interleaved round by round:
  torch    derivatives.forward_fd: two forward launches and the torch kernels that build the rows and the quotients
  fused    KManipEnvHip.forward_fd: one library call, two launches
  floor    what the simulator alone costs: forward over the 64 rows, then forward over 2 ncol 64 PREBUILT rows into preallocated
           outputs -- no perturbation, no quotient, but the perturbed rows read from and their outputs written to memory
Reported: mean (min - max) in us.  THE CONDITION: the fused call's max is below the torch path's min in the same run (exit status 1
otherwise).  Reported only: whether the fused mean lies within the floor's min - max."""
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
    lines, ok = [], True

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for env_id, n in CONFIGS:
        env = env_hip.make(env_id, num_envs=n, seed=1)
        cm = env.cm
        env.k_reset()
        for _ in range(12):
            env.step_flat(env.sample_action())
        st = env.state_tensors()
        idx = torch.arange(FD_ENVS, dtype=torch.int32, device=env.device)
        reps = 2 * (3 * cm.nv + cm.nu)
        rows = lambda: {k: st[k][:FD_ENVS] for k in ("qpos", "qvel", "ctrl")}
        fields = ("qacc", "qfrc_constraint", "contact_mask", "status")
        nominal = env.forward(envs=idx, fields=fields, **rows())
        big = dict({k: v.repeat(reps, 1) for k, v in rows().items()}, warm=(nominal["qacc"] + 1.0).repeat(reps, 1),
                   qfrc_applied=torch.zeros((reps * FD_ENVS, cm.nv), dtype=torch.float64, device=env.device))
        big_idx = idx.repeat(reps)
        pert = env.forward(envs=big_idx, fields=fields, **big)

        def floor():
            env.forward(envs=idx, out=nominal, **rows())
            env.forward(envs=big_idx, out=pert, **big)

        phases = [("torch", lambda: forward_fd(env, envs=idx, **rows())), ("fused", lambda: env.forward_fd(envs=idx, **rows())), ("floor", floor)]
        t = {name: [] for name, _ in phases}
        for k in range(WARM + args.reps):
            env.step_flat(env.sample_action())
            env.state_tensors(out=st)
            for key in ("qpos", "qvel", "ctrl"):
                big[key].copy_(st[key][:FD_ENVS].repeat(reps, 1))
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        emit("# library %s, %s, %d envs, rows = the first %d envs, %d column pairs a row, %d timed rounds after %d warm-up rounds"
             % (env.L.kmanip_version().decode(), env_id, n, FD_ENVS, reps // 2, args.reps, WARM))
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-14s %-6s mean %8.1f us  (%8.1f - %8.1f)" % (env_id, name, mean[name], min(t[name]), max(t[name])))
        cond = max(t["fused"]) < min(t["torch"])
        ok = ok and cond
        emit("%-14s torch / fused = %.2f   fused / floor = %.2f   fused max < torch min: %s   fused mean within the floor's min - max: %s"
             % (env_id, mean["torch"] / mean["fused"], mean["fused"] / mean["floor"], cond, min(t["floor"]) <= mean["fused"] <= max(t["floor"])))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
