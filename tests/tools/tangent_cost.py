#!/usr/bin/env python3
"""Cost of KManipEnvHip.tangent (kmanip_tangent) beside the torch code it replaces, measured with HIP events
in one process on one GPU:

    timeout 900 python tests/tools/tangent_cost.py [--reps 30] [--out profiles/tangent_cost.txt]

lqr_cost.py's method (section 37): after WARM untimed rounds, `--reps` rounds; a round times each variant as ONE call between two
events of its own, the variants interleaved round by round.  Reported: mean (min - max) in us.
  1. tangent against derivatives.tangent_pass on the same tensors: tangent_reference.family at 8 problems of 8 steps, both classes,
     m in {1, 4, 16}, open and closed loop, every input given; the device reads A and B through deriv_t.
  2. H and g from the kernel (S not written) against sysid.param_sensitivity + _scaled_jacobian + the two matmuls in torch: 64
     KManipSoloArm problems of 8 steps, m = 4, src alone.
  3. One sysid.identify iteration on 64 KManipSoloArmQPos problems of 8 steps in its parts -- state linearisation (plain and fused),
     param_fd, the torch sensitivity recursion, J and the products (apart and together), the batched SVD, the device's H and g -- and whole, for plain,
     fused, and fused + device_sensitivity (no callback: neither S nor the SVD before the last iterate).
There is no threshold: what was measured is recorded, whichever way it came out."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM = 3
N, T = 8, 8


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
    import tangent_reference as TC
    from gym_kmanip_amd import env_hip, ilqr, sysid
    from gym_kmanip_amd.derivatives import tangent_pass
    from gym_kmanip_amd.examples import system_identification as ex
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def table(tag, t, pairs):
        for name in t:
            emit("%-34s %-44s mean %9.1f us (%9.1f - %9.1f)" % (tag, name, statistics.fmean(t[name]), min(t[name]), max(t[name])))
        for dev, ref in pairs:
            emit("%-34s %s / %s = %.4f   device max < torch min: %s" % (tag, dev, ref, statistics.fmean(t[dev]) / statistics.fmean(t[ref]),
                                                                        "yes" if max(t[dev]) < min(t[ref]) else "NO"))
    # ---- 1. the sweep
    for k, env_id in enumerate(("KManipSoloArm", "KManipDualArm")):
        env = env_hip.make(env_id, num_envs=2, seed=1)
        nx, nu = 2 * env.cm.nv, env.cm.nu
        if k == 0:
            emit("# library %s; %d timed rounds after %d warm-up rounds, variants interleaved; us per call, mean (min - max)"
                 % (env.L.kmanip_version().decode(), args.reps, WARM))
        for m in (1, 4, 16):
            d = {name: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(env.device) for name, v in TC.family(nx, nu, T, m, True, N).items()}
            deriv_t = torch.cat([d["A"].transpose(2, 3), d["B"].transpose(2, 3)], dim=2).contiguous()
            gains_t = d["K"].transpose(2, 3).contiguous()
            out = {}
            dev = lambda g: env.tangent(deriv_t=deriv_t, src=d["src"], du=d["du"], s0=d["s0"], gains_t=g, fields=("S", "du_acted"))
            phases = [("tangent_pass (torch), open", lambda: out.update(t_open=tangent_pass(d["A"], d["B"], d["src"], d["du"], d["s0"], None))),
                      ("tangent (device), open", lambda: out.update(d_open=dev(None))),
                      ("tangent_pass (torch), closed", lambda: out.update(t_closed=tangent_pass(d["A"], d["B"], d["src"], d["du"], d["s0"], d["K"]))),
                      ("tangent (device), closed", lambda: out.update(d_closed=dev(gains_t)))]
            t = _timed(phases, args.reps)
            tag = "%s %d x %d, m %d" % (env_id, N, T, m)
            gap = max(float((out["d_" + c]["S"] - out["t_" + c][0]).abs().max() / out["t_" + c][0].abs().max()) for c in ("open", "closed"))
            emit("# %s (nx %d, nu %d): largest |S device - S torch| / largest |S| %.3e" % (tag, nx, nu, gap))
            table(tag, t, [("tangent (device), " + c, "tangent_pass (torch), " + c) for c in ("open", "closed")])
        if k == 0:
            # ---- 2. the Gauss-Newton terms, 64 problems, m = 4
            n2, m = 64, 4
            d = {name: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(env.device) for name, v in TC.family(nx, nu, T, m, False, n2).items()}
            deriv_t = torch.cat([d["A"].transpose(2, 3), d["B"].transpose(2, 3)], dim=2).contiguous()
            P = d["src"].transpose(2, 3).contiguous().transpose(2, 3)          # (param_fd's layout: passed by pointer)
            cost = sysid.TrackingCost(env.cm, None, None, torch.ones(nx, dtype=torch.float64, device=env.device))
            scale = torch.ones((n2, m), dtype=torch.float64, device=env.device)
            r = d["r"]
            out = {}

            def torch_terms():
                J, half = sysid._scaled_jacobian(cost, sysid.param_sensitivity(d["A"], P), scale)
                rw = (r @ half.transpose(0, 1)).reshape(n2, -1)
                out.update(tH=J.transpose(1, 2) @ J, tg=(J.transpose(1, 2) @ rw[:, :, None])[:, :, 0])
            phases = [("param_sensitivity + J + J'J, J'r (torch)", torch_terms),
                      ("tangent H, g (device)", lambda: out.update(env.tangent(deriv_t=deriv_t, src=P, resid=r, weight=cost.Q, fields=("H", "g"))))]
            t = _timed(phases, args.reps)
            tag = "%s %d x %d, m %d" % (env_id, n2, T, m)
            emit("# %s: largest |H device - H torch| / largest |H| %.3e, g %.3e" % (tag, float((out["H"] - out["tH"]).abs().max() / out["tH"].abs().max()),
                                                                                  float((out["g"] - out["tg"]).abs().max() / out["tg"].abs().max())))
            table(tag, t, [("tangent H, g (device)", "param_sensitivity + J + J'J, J'r (torch)")])
        env.k_close()
    # ---- 3. one identify iteration, 64 problems of 8 steps
    n3 = 64
    real, model = (env_hip.make("KManipSoloArmQPos", num_envs=n3, seed=3) for _ in range(2))
    real.k_reset(); model.k_reset()
    real.set_env_params(**{name: torch.from_numpy(v).to(real.device) for name, v in ex.hidden_params(real.cm, n3).items()})
    st = ex.contact_states(model, model.state_tensors())
    ctrl = ex.sweep_controls(model.cm, st, T)
    idx = torch.arange(n3, dtype=torch.int32, device=ctrl.device)
    qo, vo, _ = ex.log_trajectory(real, idx, st, ctrl)
    start = {k: v.clone() for k, v in model.get_env_params().items()}
    cost = sysid.TrackingCost(model.cm, qo, vo, torch.ones(2 * model.cm.nv, dtype=torch.float64, device=ctrl.device))
    fd = ilqr.trajectory_fd(model, idx, st["qpos"], st["qvel"], st["warm"], ctrl, fused=True)
    P = sysid.trajectory_param_fd(model, fd, idx, ctrl)
    scale = torch.stack([start[k][:n3] for k in start], dim=1)
    keep = {}

    def whole(**kw):
        model.set_env_params(**start)
        sysid.identify(model, idx, st["qpos"], st["qvel"], st["warm"], ctrl, qo, vo, iters=1, **kw)
    phases = [("state linearisation, plain", lambda: ilqr.trajectory_fd(model, idx, st["qpos"], st["qvel"], st["warm"], ctrl)),
              ("state linearisation, fused", lambda: ilqr.trajectory_fd(model, idx, st["qpos"], st["qvel"], st["warm"], ctrl, fused=True)),
              ("parameter derivative (param_fd)", lambda: sysid.trajectory_param_fd(model, fd, idx, ctrl)),
              ("sensitivity recursion (torch)", lambda: keep.update(S=sysid.param_sensitivity(fd["A"], P))),
              ("J, J'J, J'r and the solve (torch)", lambda: keep.update(J=_step(torch, sysid, cost, keep["S"], scale, fd))),
              ("recursion + J, J'J, J'r and the solve (torch)", lambda: _step(torch, sysid, cost, sysid.param_sensitivity(fd["A"], P), scale, fd)),
              ("batched svdvals(J) (torch)", lambda: torch.linalg.svdvals(keep["J"])),
              ("H, g (device) + scaling + the solve", lambda: _step_dev(torch, sysid, model, cost, P, scale, fd)),
              ("2 linearisations + 1 step, plain", lambda: whole()), ("2 linearisations + 1 step, fused", lambda: whole(fused=True)),
              ("2 linearisations + 1 step, fused + device", lambda: whole(fused=True, device_sensitivity=True))]
    t = _timed(phases, args.reps)
    table("identify %d x %d, 4 parameters" % (n3, T), t, [("H, g (device) + scaling + the solve", "recursion + J, J'J, J'r and the solve (torch)"),
                                                         ("2 linearisations + 1 step, fused + device", "2 linearisations + 1 step, fused")])
    real.k_close(); model.k_close()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from gym_kmanip_amd import lib as klib
    for k in kr.kernels(klib.LIB_PATH):
        if "k_tangent" in k.name:
            emit("# %-60s vgpr %s agpr %s sgpr %s scratch %s lds %s" % ((k.name,) + tuple(k[1:])))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


def _solve(torch, H, g):
    dg = torch.diagonal(H, dim1=1, dim2=2)
    return -torch.linalg.solve(H + torch.diag_embed(0.1 * torch.where(dg > 0, dg, torch.ones_like(dg))), g)


def _step(torch, sysid, cost, S, scale, fd):
    """identify's torch step from S: J, r, J'J, J'r and the damped solve.  Returns J."""
    J, half = sysid._scaled_jacobian(cost, S, scale)
    r = (cost.residual(fd["qpos"], fd["qvel"]) @ half.transpose(0, 1)).reshape(J.shape[0], -1)
    _solve(torch, J.transpose(1, 2) @ J, (J.transpose(1, 2) @ r[:, :, None])[:, :, 0])
    return J


def _step_dev(torch, sysid, model, cost, P, scale, fd):
    """identify's device step: gauss_newton_terms, the scaling and the damped solve."""
    H, g, _ = sysid.gauss_newton_terms(model, fd, P, cost)
    _solve(torch, H * (scale[:, :, None] * scale[:, None, :]), g * scale)


if __name__ == "__main__":
    sys.exit(main())
