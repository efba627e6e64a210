#!/usr/bin/env python3
"""Cost of KManipEnvHip.adjoint (kmanip_adjoint) beside derivatives.adjoint_pass, the torch loop it replaces,
measured with HIP events in one process on one GPU:

    timeout 600 python tests/tools/adjoint_cost.py [--reps 30] [--out profiles/adjoint_cost.txt]

lqr_cost.py's method: after WARM untimed rounds, `--reps` rounds; a round times each variant as ONE call between two events of its
own, the variants interleaved round by round so that clock and box drift hit all of them alike.  Reported: mean / median / min / max
in us -- the spread is the min .. max column.  The tensors are adjoint_reference.family's at 8 problems of 8 steps, both classes
(KManipSoloArm: nx 32, nu 10; KManipDualArm: nx 52, nu 20), m = 1 (a gradient) and m = nx (a sensitivity Jacobian), open and closed
loop; the device reads the same A and B through deriv_t, the layout transition_fd leaves them in, and the same gx, gu and gains.
The yardstick is derivatives.adjoint_pass at the same commit on the same device.  There is no threshold: what was measured is
recorded, whichever way it came out."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM = 3
N, T = 8, 8
ENVS = ("KManipSoloArm", "KManipDualArm")


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
    import adjoint_reference as AR
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.derivatives import adjoint_pass
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    first = True
    for env_id in ENVS:
        env = env_hip.make(env_id, num_envs=2, seed=1)
        nx, nu = 2 * env.cm.nv, env.cm.nu
        if first:
            emit("# library %s; %d problems of %d steps, %d timed rounds after %d warm-up rounds, variants interleaved; us per call"
                 % (env.L.kmanip_version().decode(), N, T, args.reps, WARM))
            first = False
        for m in (1, nx):
            f = AR.family(nx, nu, T, N, m)
            d = {name: torch.from_numpy(np.ascontiguousarray(v)).to(env.device) for name, v in f.items()}
            deriv_t = torch.cat([d["A"].transpose(2, 3), d["B"].transpose(2, 3)], dim=2).contiguous()
            gains_t = d["gains"].transpose(2, 3).contiguous()
            out = {}
            phases = [("adjoint_pass (torch), open", lambda: out.update(t_open=adjoint_pass(d["A"], d["B"], d["gx"], d["gu"], None, m))),
                      ("adjoint (device), open", lambda: out.update(d_open=env.adjoint(d["gx"], d["gu"], deriv_t=deriv_t, m=m))),
                      ("adjoint_pass (torch), closed", lambda: out.update(t_closed=adjoint_pass(d["A"], d["B"], d["gx"], d["gu"], d["gains"], m))),
                      ("adjoint (device), closed", lambda: out.update(d_closed=env.adjoint(d["gx"], d["gu"], deriv_t=deriv_t, gains_t=gains_t, m=m)))]
            t = _timed(phases, args.reps)
            tag = "%s %d x %d, m %d" % (env_id, N, T, m)
            gap = max(float((out["d_" + k]["lam"] - out["t_" + k][0]).abs().max() / out["t_" + k][0].abs().max()) for k in ("open", "closed"))
            emit("# %s (nx %d, nu %d): largest |lam device - lam torch| / largest |lam| %.3e" % (tag, nx, nu, gap))
            for name, _ in phases:
                emit("%-30s %-30s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f"
                     % (tag, name, statistics.fmean(t[name]), statistics.median(t[name]), min(t[name]), max(t[name])))
            for k in ("open", "closed"):
                p1, p2 = t["adjoint_pass (torch), " + k], t["adjoint (device), " + k]
                emit("%-30s %-6s device / torch = %.4f   device max < torch min: %s"
                     % (tag, k, statistics.fmean(p2) / statistics.fmean(p1), "yes" if max(p2) < min(p1) else "NO"))
        env.k_close()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from gym_kmanip_amd import lib as klib
    for k in kr.kernels(klib.LIB_PATH):
        if "k_adjoint" in k.name:
            emit("# %-60s vgpr %s agpr %s sgpr %s scratch %s lds %s" % ((k.name,) + tuple(k[1:])))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
