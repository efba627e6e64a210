#!/usr/bin/env python3
"""Cost of KManipEnvHip.site_cost (kmanip_site_cost) beside ilqr.SiteCost(device=False), the kinematics_at launch plus torch
arithmetic it replaces, measured by lqr_cost.py's method -- HIP events in one process on one GPU:

    timeout 600 python tests/tools/site_cost_cost.py [--reps 30] [--out profiles/site_cost.txt]

After WARM untimed rounds, `--reps` rounds; a round times each phase as ONE call sequence between two events of its own, the phases
interleaved round by round.  Reported: mean / median / min / max in us.  Per shape (n envs x horizon T): KManipSoloArmQPos 8 x 8 and
64 x 32, KManipDualArmQPos 8 x 8 --
1. COST DERIVATIVES: cost.derivatives of SumCost(QuadraticCost, SiteCost) on a nominal trajectory, the phase an iLQR iteration spends
   on them: device=False (one kinematics_at launch + torch) against device=True (one launch).
2. LINE SEARCH: cost.total on the 3 n trajectories of a line search with 3 alphas, likewise.
The condition reported per shape and phase is section 37's: the device's max below torch's min.
3. THE WHOLE ITERATION at 8 x 8, fused with the device backward pass, without and with the device cost, for the record.
Last, the new kernels' resource lines (tools/kernel_resources.py).  The yardstick is device=False at the same commit."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM = 3
ALPHAS = (1.0, 0.5, 0.25)
SHAPES = (("KManipSoloArmQPos", 8, 8), ("KManipSoloArmQPos", 64, 32), ("KManipDualArmQPos", 8, 8))


def _timed(phases, reps):
    import torch
    t = {name: [] for name, _ in phases}
    for k in range(WARM + reps):
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
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import torch
    import kernel_resources
    from gym_kmanip_amd import env_hip, ilqr
    from gym_kmanip_amd import lib as klib
    from gym_kmanip_amd.examples import ilqr_site_reach as EX
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def report(tag, phases, t):
        for name, _ in phases:
            emit("%-28s %-40s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f"
                 % (tag, name, statistics.fmean(t[name]), statistics.median(t[name]), min(t[name]), max(t[name])))

    def condition(tag, what, t, dev_name, torch_name):
        d, h = t[dev_name], t[torch_name]
        emit("%-28s %s: device / torch = %.4f   condition (device max < torch min): %s"
             % (tag, what, statistics.fmean(d) / statistics.fmean(h), "met" if max(d) < min(h) else "NOT met"))

    first = True
    for env_id, n, T in SHAPES:
        env = env_hip.make(env_id, num_envs=n, seed=3)
        cm, dev = env.cm, env.device
        env.k_reset()
        st = env.state_tensors()
        idx = torch.arange(n, dtype=torch.int32, device=dev)
        sx = env.kinematics_at(envs=idx, fields=("site_xpos",))["site_xpos"]
        target = sx + torch.from_numpy(np.random.default_rng(3).uniform(-0.05, 0.05, (n, 2, 3))).to(dev)
        quat = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev).expand(n, 2, 4).contiguous()
        wq = torch.zeros(2 * cm.nv, dtype=torch.float64, device=dev)
        wq[cm.nv:cm.nv + cm.nlink] = EX.W_VEL
        smooth = ilqr.QuadraticCost(cm, st["qpos"], torch.zeros((n, cm.nv), dtype=torch.float64, device=dev), wq,
                                    torch.full((cm.nu,), EX.W_CTRL, dtype=torch.float64, device=dev), wq)
        costs = {d: ilqr.SumCost(smooth, ilqr.SiteCost(env, target, quat, w_pos=EX.W_POS, w_rot=1.0, wf_pos=EX.WF_POS, device=d)) for d in (False, True)}
        ctrl = st["ctrl"][:, None, :].repeat(1, T, 1)
        roll = env.rollout(envs=idx, qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl, fields=("qpos", "qvel", "status"))
        q = torch.cat([st["qpos"][:, None], roll["qpos"]], dim=1)
        v = torch.cat([st["qvel"][:, None], roll["qvel"]], dim=1)
        na = len(ALPHAS)
        q3, v3, u3 = q.repeat(na, 1, 1), v.repeat(na, 1, 1), ctrl.repeat(na, 1, 1)
        out = {}
        phases = [("cost derivatives, device=False", lambda: out.update(dt=costs[False].derivatives(q, v, ctrl))),
                  ("cost derivatives, device=True", lambda: out.update(dd=costs[True].derivatives(q, v, ctrl))),
                  ("line-search total, device=False", lambda: out.update(tt=costs[False].total(q3, v3, u3))),
                  ("line-search total, device=True", lambda: out.update(td=costs[True].total(q3, v3, u3)))]
        t = _timed(phases, args.reps)
        tag = "%s %d x %d" % (env_id.replace("KManip", "").replace("QPos", ""), n, T)
        if first:
            emit("# library %s; %d timed rounds after %d warm-up rounds; SumCost(QuadraticCost, SiteCost with position and rotation weights), %d alphas"
                 % (env.L.kmanip_version().decode(), args.reps, WARM, na))
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
        emit("# %s (nx %d): rows %d / %d; device against torch in the last round: lx %.1e  lxx %.1e  total %.1e (relative to the largest entry)"
             % (tag, 2 * cm.nv, n * (T + 1), na * n * (T + 1), rel(out["dd"][0], out["dt"][0]), rel(out["dd"][2], out["dt"][2]), rel(out["td"], out["tt"])))
        report(tag, phases, t)
        condition(tag, "cost derivatives", t, phases[1][0], phases[0][0])
        condition(tag, "line-search total", t, phases[3][0], phases[2][0])
        if first:
            whole = [("whole iteration, torch cost", lambda: ilqr.ilqr(env, None, st["qpos"], st["qvel"], st["warm"], ctrl, costs[False], iters=1, alphas=ALPHAS,
                                                                     fused=True, device_backward=True)),
                     ("whole iteration, device cost", lambda: ilqr.ilqr(env, None, st["qpos"], st["qvel"], st["warm"], ctrl, costs[True], iters=1, alphas=ALPHAS,
                                                                      fused=True, device_backward=True))]
            report(tag, whole, _timed(whole, args.reps))
            first = False
        env.k_close()
    emit("# resources of the new kernels (tools/kernel_resources.py)")
    for k in kernel_resources.kernels(klib.LIB_PATH, "k_kinrows|k_sitecost"):
        emit("%-60s vgpr %s agpr %s sgpr %s scratch %s lds %s" % ((k.name[:60],) + k[1:]))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
