#!/usr/bin/env python3
"""Cost of kmanip_feedback beside kmanip_rollout and beside the path it replaces, measured with HIP events in
one process on one GPU:

    python tests/tools/feedback_cost.py [--reps 30] [--out profiles/feedback_cost.txt]

KManipSoloArm at 4096 rows and KManipDualArm at 8192 rows (row r = env r), after a reset and 12 sampled steps; 8 steps of the model's
sub-steps, states only (no trailing pass), ctrl per step, a gain trajectory per row: the references are the states of the open-loop
rollout before each step moved by 1e-2, the gains those of tests/tools/feedback_oracle.py's fixed set.  After WARM untimed rounds,
`--reps` rounds; every round takes one sampled step first (untimed) and then times each phase as ONE call sequence between two
events of its own, interleaved round by round so that clock and box drift hit all of them alike:
  rollout            one rollout() launch of 8 steps, open loop
  rollout_feedback   one rollout_feedback() launch of 8 steps, the policy evaluated on the device (transposed gains given)
  eight launches     the path this replaces: eight one-step rollout() launches fed qpos / qvel / qacc_warm, with tangent_diff, the
                     matvec and the add in torch between each pair
  eight launches, open loop   the same eight launches without the torch policy (what the launches alone cost)
Reported: mean / median / min / max in us and the ratios.  There is no pass bar and no expected figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 3
CONFIGS = (("KManipSoloArm", 4096), ("KManipDualArm", 8192))
NSTEP = 8
STATE = ("qpos", "qvel", "qacc_warm", "status", "steps_done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import numpy as np
    import torch
    import feedback_oracle as FO
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.derivatives import tangent_diff
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
        st = env.state_tensors()
        ctrl = st["ctrl"].unsqueeze(1).repeat(1, NSTEP, 1).contiguous()
        # one gain trajectory per row: the fixed set's gains for 64 trajectories, tiled
        K64 = FO.fixed_policy(cm, np.zeros((64, cm.nq)) + np.eye(cm.nq)[cm.nlink + 3], np.zeros((64, cm.nv)), NSTEP)[0]
        gains_t = torch.from_numpy(K64).to(env.device).repeat(n // 64, 1, 1, 1).transpose(-1, -2).contiguous()
        gains = gains_t.transpose(-1, -2).contiguous()
        open_out = env.rollout(nstep=NSTEP, fields=STATE)
        fb_out = env.rollout_feedback(ctrl=ctrl, gains_t=gains_t, qpos_ref=open_out["qpos"], qvel_ref=open_out["qvel"], fields=STATE + ("ctrl",))
        one_out = env.rollout(nstep=1, fields=STATE)
        qref, vref = torch.empty_like(open_out["qpos"]), torch.empty_like(open_out["qvel"])

        def eight(policy):
            q, v, w = st["qpos"], st["qvel"], st["warm"]
            for t in range(NSTEP):
                u = ctrl[:, t]
                if policy:
                    dx = torch.cat([tangent_diff(cm, q, qref[:, t]), v - vref[:, t]], dim=1)
                    u = u + (gains[:, t] @ dx[:, :, None])[:, :, 0]
                env.rollout(qpos=q, qvel=v, warm=w, ctrl=u.contiguous(), nstep=1, out=one_out)
                q, v, w = (one_out[k][:, 0].clone() for k in ("qpos", "qvel", "qacc_warm"))

        phases = [("rollout, %d steps" % NSTEP, lambda: env.rollout(qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl, out=open_out)),
                  ("rollout_feedback, %d steps" % NSTEP, lambda: env.rollout_feedback(qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl, gains_t=gains_t,
                                                                                      qpos_ref=qref, qvel_ref=vref, out=fb_out)),
                  ("eight launches + torch policy", lambda: eight(True)),
                  ("eight launches, open loop", lambda: eight(False))]
        t = {name: [] for name, _ in phases}
        for k in range(WARM + args.reps):
            env.step_flat(env.sample_action())
            env.state_tensors(out=st)
            ctrl.copy_(st["ctrl"].unsqueeze(1).expand(-1, NSTEP, -1))
            env.rollout(qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl, out=open_out)
            qref[:, 0], vref[:, 0] = st["qpos"], st["qvel"]
            qref[:, 1:], vref[:, 1:] = open_out["qpos"][:, :-1], open_out["qvel"][:, :-1]
            qref[:, :, :cm.nlink + 3] += 1e-2
            vref += 1e-2
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        moved = float((fb_out["ctrl"] - ctrl).abs().max())
        emit("# library %s, %s, %d rows, %d timed rounds after %d warm-up rounds; rows that stopped early in the last round: %d of %d; "
             "largest |u - ctrl| in the last round %.3f" % (env.L.kmanip_version().decode(), env_id, n, args.reps, WARM, int(fb_out["status"].ne(0).sum()), n, moved))
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-14s %-32s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f"
                 % (env_id, name, mean[name], statistics.median(t[name]), min(t[name]), max(t[name])))
        names = [name for name, _ in phases]
        emit("%-14s rollout_feedback / rollout = %.3f   rollout_feedback / (eight launches + torch policy) = %.3f   "
             "eight launches open loop / rollout = %.3f" % (env_id, mean[names[1]] / mean[names[0]], mean[names[1]] / mean[names[2]], mean[names[3]] / mean[names[0]]))
        env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
