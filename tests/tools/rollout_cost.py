#!/usr/bin/env python3
"""Cost of kmanip_rollout beside kmanip_step, measured with HIP events in one process on one GPU:

    python tests/tools/rollout_cost.py [--reps 50] [--out profiles/rollout_cost.txt]

KManipSoloArm at 4096 envs and KManipDualArm at 8192 envs, after a reset and 12 sampled steps.  After WARM untimed rounds, `--reps`
rounds; every round takes one sampled step first (untimed: the states stay those of a natural rollout) and then times each phase
as ONE call between two events of its own -- step; rollout of n = num_envs identity rows (every input None) for 1 step and for 8
steps of the model's sub-steps, with and without contact mask and reward (the trailing pass); the same 8 steps with every input
given and ctrl per step; 8 x num_envs rows for 1 step; 1 step of a single sub-step (MuJoCo's mj_step); transition_fd for the
first 64 envs (two rollout launches and the torch kernels that build the rows and the quotients) -- interleaved round by round so
that clock and box drift hit all of them alike.  An interval holds the call as the stream sees it: the kernels, the event pair
(about 5 us) and what of the Python wrapper's checks the GPU has to wait for.  Reported: mean / median / min / max in us and the
cost of a rollout step relative to kmanip_step in the same run.  There is no pass bar and no expected figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 5
CONFIGS = (("KManipSoloArm", 4096), ("KManipDualArm", 8192))
FD_ENVS = 64
NSTEP = 8
STATE = ("qpos", "qvel", "qacc_warm", "status", "steps_done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.derivatives import transition_fd
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
        st = env.state_tensors()
        one = env.rollout(nstep=1)
        many = env.rollout(nstep=NSTEP)
        lean = env.rollout(nstep=NSTEP, fields=STATE)
        sub1 = env.rollout(nstep=1, nsub=1)
        ctrl = st["ctrl"].unsqueeze(1).repeat(1, NSTEP, 1).contiguous()
        idx8 = torch.arange(n, dtype=torch.int32, device=env.device).repeat(8)
        big = {k: st[k].repeat(8, 1) for k in ("qpos", "qvel", "ctrl", "warm")}
        out8 = env.rollout(envs=idx8, nstep=1, **big)
        fd_idx = torch.arange(FD_ENVS, dtype=torch.int32, device=env.device)
        fd_rows = lambda: {k: st[k][:FD_ENVS] for k in ("qpos", "qvel", "ctrl", "warm")}
        phases = [("kmanip_step", lambda: env.step_flat(act)),
                  ("rollout, n rows, 1 step", lambda: env.rollout(nstep=1, out=one)),
                  ("rollout, n rows, %d steps" % NSTEP, lambda: env.rollout(nstep=NSTEP, out=many)),
                  ("rollout, n rows, %d steps, states only" % NSTEP, lambda: env.rollout(nstep=NSTEP, out=lean)),
                  ("rollout, n rows, %d steps, inputs given" % NSTEP, lambda: env.rollout(qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl, out=many)),
                  ("rollout, 8 n rows, 1 step", lambda: env.rollout(envs=idx8, nstep=1, out=out8, **big)),
                  ("rollout, n rows, 1 step of 1 sub-step", lambda: env.rollout(nstep=1, nsub=1, out=sub1)),
                  ("transition_fd, %d envs" % FD_ENVS, lambda: transition_fd(env, envs=fd_idx, **fd_rows()))]
        t = {name: [] for name, _ in phases}
        for k in range(WARM + args.reps):
            env.step_flat(env.sample_action())
            env.sample_action(act)
            env.state_tensors(out=st)
            ctrl.copy_(st["ctrl"].unsqueeze(1).expand(-1, NSTEP, -1))
            for key in big:
                big[key].copy_(st[key].repeat(8, 1))
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        emit("# library %s, %s, %d envs, %d timed rounds after %d warm-up rounds; rows that stopped early in the last round: %d of %d"
             % (env.L.kmanip_version().decode(), env_id, n, args.reps, WARM, int(many["status"].ne(0).sum()), n))
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-14s %-40s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f"
                 % (env_id, name, mean[name], statistics.median(t[name]), min(t[name]), max(t[name])))
        m = mean["kmanip_step"]
        emit("%-14s 1 step / kmanip_step = %.3f   %d steps / (%d x kmanip_step) = %.3f   states only / with mask and reward = %.3f   "
             "8 n rows / n rows = %.2f   1 sub-step / 1 step = %.3f"
             % (env_id, mean["rollout, n rows, 1 step"] / m, NSTEP, NSTEP, mean["rollout, n rows, %d steps" % NSTEP] / (NSTEP * m),
                mean["rollout, n rows, %d steps, states only" % NSTEP] / mean["rollout, n rows, %d steps" % NSTEP],
                mean["rollout, 8 n rows, 1 step"] / mean["rollout, n rows, 1 step"],
                mean["rollout, n rows, 1 step of 1 sub-step"] / mean["rollout, n rows, 1 step"]))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
