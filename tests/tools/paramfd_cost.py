#!/usr/bin/env python3
"""Cost of KManipEnvHip.param_fd (kmanip_param_fd) beside the same quotient assembled from set_env_params, two rollout calls per
parameter and torch arithmetic on the same handle, and of one sysid.identify iteration split by call, measured
with HIP events in one process on one GPU:

    timeout 600 python tests/tools/paramfd_cost.py [--reps 30] [--out profiles/param_fd_cost.txt]

lqr_cost.py's method: after WARM untimed rounds, `--reps` rounds; a round times each variant as ONE call between two events of its
own, the variants interleaved round by round so that clock and box drift hit all of them alike.  Reported: mean / median / min / max
in us -- the spread is the min .. max column.  The rows are the 64 envs of a KManipSoloArmQPos handle with parameters of their own,
four control steps after reset; 4 parameters; one control step (the model's 10 sub-steps) per row.  The identify iteration is 64
problems of 8 steps: its calls are timed one by one, in the order identify makes them.  There is no threshold: what was measured is
recorded, whichever way it came out."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM = 3
N, T = 64, 8
EPS = 1e-4


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
    import numpy as np
    import torch
    from gym_kmanip_amd import env_hip, sysid
    from gym_kmanip_amd.derivatives import tangent_diff
    from gym_kmanip_amd.ilqr import trajectory_fd
    from gym_kmanip_amd.model import ENV_PARAMS, env_param_defaults
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    env = env_hip.make("KManipSoloArmQPos", num_envs=N, seed=1)
    env.k_reset()
    cm = env.cm
    dflt = env_param_defaults(cm)
    spread = torch.from_numpy(np.linspace(1.0, 1.5, N)).to(env.device)
    base = {name: spread * (dflt[name] if name != "cube_mass" else 1.5 * dflt[name]) for name in ENV_PARAMS}
    env.set_env_params(**base)
    for _ in range(4):
        env.step_flat(env.sample_action())
    st = env.state_tensors()
    idx = torch.arange(N, dtype=torch.int32, device=env.device)
    emit("# library %s; KManipSoloArmQPos, %d rows x %d parameters, one control step; %d timed rounds after %d warm-up rounds, variants "
         "interleaved; us per call" % (env.L.kmanip_version().decode(), N, len(ENV_PARAMS), args.reps, WARM))
    out = {}

    def assembled():
        cols = []
        for name in ENV_PARAMS:
            p = base[name]
            e = p * EPS
            ends = []
            for val in (p + e, p - e):
                env.set_env_params(**dict(base, **{name: val}))
                ends.append(env.rollout(envs=idx, qpos=st["qpos"], qvel=st["qvel"], ctrl=st["ctrl"], warm=st["warm"] + 1.0, nstep=1,
                                        fields=("qpos", "qvel", "status")))
            num = torch.cat([tangent_diff(cm, ends[0]["qpos"][:, 0], ends[1]["qpos"][:, 0]), ends[0]["qvel"][:, 0] - ends[1]["qvel"][:, 0]], dim=1)
            cols.append(num / (2.0 * e)[:, None].expand_as(num).contiguous())
        env.set_env_params(**base)
        out["assembled"] = torch.stack(cols, dim=1)
    phases = [("param_fd (one launch)", lambda: out.update(fused=env.param_fd(envs=idx, qpos=st["qpos"], qvel=st["qvel"], ctrl=st["ctrl"], warm=st["warm"])["deriv_t"])),
              ("set_env_params + 8 rollouts + torch", assembled)]
    t = _timed(phases, args.reps)
    a, b = out["fused"], out["assembled"]
    emit("# largest |param_fd - assembled| / largest |entry| %.3e; bytes equal: %s" % (float((a - b).abs().max() / b.abs().max()), torch.equal(a, b)))
    for name, _ in phases:
        emit("%-40s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f" % (name, statistics.fmean(t[name]), statistics.median(t[name]), min(t[name]), max(t[name])))
    p1, p2 = t[phases[1][0]], t[phases[0][0]]
    emit("param_fd / assembled = %.4f   param_fd max < assembled min: %s" % (statistics.fmean(p2) / statistics.fmean(p1), "yes" if max(p2) < min(p1) else "NO"))
    # ---- one identify iteration, call by call
    ctrl = st["ctrl"][:, None, :].repeat(1, T, 1)
    cost = sysid.TrackingCost(cm, torch.cat([st["qpos"][:, None]] * (T + 1), dim=1), torch.cat([st["qvel"][:, None]] * (T + 1), dim=1),
                              torch.ones(2 * cm.nv, dtype=torch.float64, device=env.device))
    s = {}
    pv = torch.stack([base[k] for k in ENV_PARAMS], dim=1)

    def solve():
        S = sysid.param_sensitivity(s["fd"]["A"], s["P"])
        J, half = sysid._scaled_jacobian(cost, S, pv)
        r = (cost.residual(s["fd"]["qpos"], s["fd"]["qvel"]) @ half.transpose(0, 1)).reshape(N, -1)
        H = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[:, :, None])[:, :, 0]
        dg = torch.diagonal(H, dim1=1, dim2=2)
        s["d"] = -torch.linalg.solve(H + torch.diag_embed(0.1 * torch.where(dg > 0, dg, torch.ones_like(dg))), g)
        s["sv"] = torch.linalg.svdvals(J)
    for fused in (False, True):
        phases = [("trajectory_fd%s" % (" (fused)" if fused else ""), lambda: s.update(fd=trajectory_fd(env, idx, st["qpos"], st["qvel"], st["warm"], ctrl, fused=fused))),
                  ("trajectory_param_fd (one param_fd call)", lambda: s.update(P=sysid.trajectory_param_fd(env, s["fd"], idx, ctrl))),
                  ("sensitivity, J, step, singular values (torch)", solve),
                  ("set_env_params (the candidate)", lambda: env.set_env_params(**base)),
                  ("rollout (the candidate's loss)", lambda: s.update(roll=env.rollout(envs=idx, qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl,
                                                                                        fields=("qpos", "qvel", "status"))))]
        t = _timed(phases, args.reps)
        emit("# one identify iteration, %d problems of %d steps%s" % (N, T, ", fused" if fused else ""))
        for name, _ in phases:
            emit("%-48s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f" % (name, statistics.fmean(t[name]), statistics.median(t[name]), min(t[name]), max(t[name])))
        emit("%-48s mean %9.1f us" % ("the iteration", sum(statistics.fmean(t[name]) for name, _ in phases)))
    env.k_close()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from gym_kmanip_amd import lib as klib
    for k in kr.kernels(klib.LIB_PATH):
        if "k_paramfd" in k.name or "k_transfd_ep" in k.name:
            emit("# %-110s vgpr %s agpr %s sgpr %s scratch %s lds %s" % ((k.name,) + tuple(k[1:])))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
