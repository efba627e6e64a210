#!/usr/bin/env python3
"""Cost of KManipEnvHip.transition_fd (kmanip_transition_fd) beside the path it replaces and beside the floor of its launches
(DESIGN.md section 31), measured with HIP events in one process on one GPU:

    python tests/tools/transfd_cost.py [--reps 30] [--out profiles/transfd_cost.txt]

KManipSoloArm and KManipDualArm on 64 envs, after a reset and 12 sampled steps, the default wrt (qpos, qvel, ctrl), the model's
sub-steps, two cases: the 64 stored states as rows, and 64 x 8 rows -- the start-of-step states of an 8-step rollout under the stored
ctrl, what ilqr.trajectory_fd passes for a horizon of 8.  After WARM untimed rounds, `--reps` rounds; every round takes one sampled
step first (untimed) and then times each phase as ONE call sequence between two events of its own, interleaved round by round so that
clock and box drift hit all of them alike:
  derivatives.transition_fd    the path replaced: two rollout() launches with torch arithmetic before, between and after them
  KManipEnvHip.transition_fd   the fused call: the nominal launch and the kernel that perturbs, steps and differences
  two rollout launches         the floor: rollout(nstep = 1) of the n rows, then of the 2 ncol n perturbed rows, prebuilt (untimed)
Then one iteration of ilqr.ilqr on examples/ilqr_reach.py's problem (KManipSoloArmQPos, 8 envs, horizon 8, 3 alphas), with and without
fused=True, timed the same way.  Reported: mean / median / min / max in us and the ratios.  There is no absolute bar."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 3
ENVS = ("KManipSoloArm", "KManipDualArm")
N, HORIZON = 64, 8
FIELDS = ("qpos", "qvel", "qacc_warm", "contact_mask", "status")


class _Keep:
    """derivatives.transition_fd's view of a handle -- .cm and .rollout -- that keeps the arguments of every call."""

    def __init__(self, env):
        self.env, self.cm, self.calls = env, env.cm, []

    def rollout(self, **kw):
        self.calls.append(kw)
        return self.env.rollout(**kw)


def _timed(phases, reps, before_round):
    import torch
    t = {name: [] for name, _ in phases}
    for k in range(WARM + reps):
        before_round()
        for name, f in phases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            b.synchronize()
            if k >= WARM:
                t[name].append(a.elapsed_time(b) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip, ilqr
    from gym_kmanip_amd.derivatives import transition_fd
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def report(tag, phases, t):
        mean = {name: statistics.fmean(v) for name, v in t.items()}
        for name, _ in phases:
            emit("%-28s %-28s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f" % (tag, name, mean[name], statistics.median(t[name]), min(t[name]), max(t[name])))
        return mean

    for env_id in ENVS:
        env = env_hip.make(env_id, num_envs=N, seed=1)
        cm = env.cm
        env.k_reset()
        for _ in range(12):
            env.step_flat(env.sample_action())
        idx = torch.arange(N, dtype=torch.int32, device=env.device)
        for case, T in (("%d rows" % N, 1), ("%d x %d rows" % (N, HORIZON), HORIZON)):
            rows, floor = {}, {}

            def new_rows():
                """A sampled step, then the rows of the case and the prebuilt perturbed rows of the floor (all untimed)."""
                env.step_flat(env.sample_action())
                st = env.state_tensors()
                rows.update(envs=idx, qpos=st["qpos"], qvel=st["qvel"], ctrl=st["ctrl"], warm=st["warm"])
                if T > 1:
                    roll = env.rollout(nstep=T, fields=("qpos", "qvel", "qacc_warm"))
                    start = lambda first, rec: torch.cat([first[:, None], rec[:, :-1]], dim=1).reshape(N * T, -1).contiguous()
                    rows.update(envs=idx.repeat_interleave(T), qpos=start(st["qpos"], roll["qpos"]), qvel=start(st["qvel"], roll["qvel"]),
                                warm=start(st["warm"], roll["qacc_warm"]), ctrl=st["ctrl"].repeat_interleave(T, dim=0))
                keep = _Keep(env)
                transition_fd(keep, **rows)
                floor["calls"] = keep.calls

            def two_launches():
                for kw in floor["calls"]:
                    env.rollout(**kw)

            phases = [("derivatives.transition_fd", lambda: transition_fd(env, **rows)),
                      ("KManipEnvHip.transition_fd", lambda: env.transition_fd(**rows)),
                      ("two rollout launches", two_launches)]
            t = _timed(phases, args.reps, new_rows)
            a, b = transition_fd(env, **rows), env.transition_fd(**rows)
            n, ncol = int(rows["qpos"].shape[0]), 2 * cm.nv + cm.nu
            emit("# library %s, %s, %s (%d perturbed rows), %d timed rounds after %d warm-up rounds; rows or columns with a nonzero status in the last round: "
                 "%d; largest |fused - python| over A and B in the last round %.3e" % (env.L.kmanip_version().decode(), env_id, case, 2 * ncol * n, args.reps, WARM,
                                                                                      int(b["status"].ne(0).sum() + b["status_cols"].ne(0).sum()),
                                                                                      max(float((a[k] - b[k]).abs().max()) for k in ("A", "B"))))
            mean = report("%s, %s" % (env_id, case), phases, t)
            p1, p2, p3 = (t[name] for name, _ in phases)
            emit("%-28s fused / python = %.3f   fused / floor = %.3f   condition (fused max < python min): %s   fused mean within the floor's min .. max: %s"
                 % ("%s, %s" % (env_id, case), mean[phases[1][0]] / mean[phases[0][0]], mean[phases[1][0]] / mean[phases[2][0]],
                    "met" if max(p2) < min(p1) else "NOT met", "yes" if min(p3) <= mean[phases[1][0]] <= max(p3) else "no"))
        env.k_close()

    # one iLQR iteration of examples/ilqr_reach.py's problem
    env = env_hip.make("KManipSoloArmQPos", num_envs=8, seed=3)
    cm, dev = env.cm, env.device
    env.k_reset()
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    goal = st["qpos"].clone()
    goal[:, :cm.nlink] += 0.1 * torch.tensor([1.0, -1.0], dtype=torch.float64, device=dev).repeat(cm.nlink)[:cm.nlink]
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64, device=dev)
    wq[:cm.nlink] = 10.0
    wq[cm.nv:cm.nv + cm.nlink] = 0.01
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((8, cm.nv), dtype=torch.float64, device=dev), wq, torch.full((cm.nu,), 1e-3, dtype=torch.float64, device=dev), 10.0 * wq)
    guess = st["ctrl"][:, None, :].repeat(1, HORIZON, 1)
    one = lambda fused: ilqr.ilqr(env, None, st["qpos"], st["qvel"], st["warm"], guess, cost, iters=1, fused=fused)
    phases = [("ilqr iteration", lambda: one(False)), ("ilqr iteration, fused", lambda: one(True))]
    t = _timed(phases, args.reps, lambda: None)
    emit("# KManipSoloArmQPos, 8 envs, horizon %d, 3 alphas: one ilqr.ilqr iteration; cost after it %.6f / %.6f (fused)"
         % (HORIZON, float(one(False)["cost"][-1].mean()), float(one(True)["cost"][-1].mean())))
    mean = report("KManipSoloArmQPos, 8 x %d" % HORIZON, phases, t)
    emit("%-28s fused / python = %.3f" % ("KManipSoloArmQPos, 8 x %d" % HORIZON, mean[phases[1][0]] / mean[phases[0][0]]))
    env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
