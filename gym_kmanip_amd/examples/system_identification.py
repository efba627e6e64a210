#!/usr/bin/env python3
"""System identification (gym_kmanip_amd.sysid.identify): the per-env physics parameters of a "real" handle recovered from one logged
trajectory per env by a second handle that starts at the model's defaults.

    python -m gym_kmanip_amd.examples.system_identification [--num-envs 4] [--horizon 6] [--iters 8] [--wrt kp_scale cube_mass ...]
        [--fused] [--device-adjoint] [--no-contact]

The task is KManipSoloArmQPos.  The real handle gets hidden parameters (per env: the check values of DESIGN.md section 42 spread by a
few per cent) and is stepped open loop with a control sequence; the states it passes through are the log.  The second handle then
runs sysid.identify: per iteration one rollout and its linearisation (ilqr.trajectory_fd; --fused: kmanip_transition_fd), ONE
KManipEnvHip.param_fd call (kmanip_param_fd: d x_{t+1} / d p at every step), the sensitivity recursion and a damped Gauss-Newton step
whose candidate is written with set_env_params and judged by one more rollout.  Printed per iteration: the parameters, the loss and
the singular values of the scaled Jacobian, per env; then what was and was not recovered, then the record as JSON.
THE START STATES put the cube at the gripper's site, between the fingers, and the controls close the gripper while the arm sweeps:
contact with the arm is what makes the cube's parameters observable (every singular value then stands well above RATIO); from the
model's defaults the default eight iterations do not always reach the hidden values on such a start, and the example prints which did.  --no-contact leaves the cube where the reset spawned it: the
arm alone shows kp_scale and nothing else, and the example says so -- a singular value below RATIO times the largest marks a
direction in parameter space that this log does not determine.
--device-adjoint also prints the gradient of the tracking loss in the parameters at the start (sysid.rollout_param_grad with the
adjoint sweep in one launch, kmanip_adjoint).
identify_log() is the loop itself on any env with rollout, param_fd and set_env_params: tests run it on the CPU oracle's stand-in."""
import argparse
import json

from gym_kmanip_amd import sysid
from gym_kmanip_amd.model import ENV_PARAMS

RATIO = 1e-6        # a singular value below RATIO x the largest: the direction is not observable from the log
RECOVERED = 1e-4    # a parameter within this relative distance of the hidden value counts as recovered


def log_trajectory(env, envs, st, ctrl, nsub=None):
    """(qpos_obs [n, T + 1, nq], qvel_obs [n, T + 1, nv]): the states x_0 .. x_T env passes through under ctrl [n, T, nu] from st."""
    import torch
    roll = env.rollout(envs=envs, qpos=st["qpos"], qvel=st["qvel"], warm=st["warm"], ctrl=ctrl, nsub=nsub, fields=("qpos", "qvel", "status"))
    return torch.cat([st["qpos"][:, None], roll["qpos"]], dim=1), torch.cat([st["qvel"][:, None], roll["qvel"]], dim=1), roll["status"]


def identify_log(real, model, st, ctrl, wrt=ENV_PARAMS, iters=8, nsub=None, fused=False, device_adjoint=False, verbose=print):
    """The example's loop: `real` (a handle with hidden parameters) logs the trajectory of ctrl [n, T, nu] from the states st (qpos,
    qvel, warm: [n, ..] tensors; problem e is env e of both handles), `model` identifies `wrt` from it.  Returns sysid.identify's dict
    plus hidden {name: [n]}, error {name: [n]} (relative), observable [n] bool (the smallest singular value against RATIO) and, with
    device_adjoint, grad_params [n, npar] at the start."""
    import torch
    n = int(ctrl.shape[0])
    envs = torch.arange(n, dtype=torch.int32, device=ctrl.device)
    qpos_obs, qvel_obs, status = log_trajectory(real, envs, st, ctrl, nsub)
    extra = {}
    if device_adjoint:
        cost = sysid.TrackingCost(model.cm, qpos_obs, qvel_obs, torch.ones(2 * model.cm.nv, dtype=ctrl.dtype, device=ctrl.device))
        g = sysid.rollout_param_grad(model, envs, st["qpos"], st["qvel"], st["warm"], ctrl, cost, wrt=wrt, nsub=nsub, fused=fused, device=True)
        extra["grad_params"] = g["grad_params"]
        verbose("start: loss %s  d loss / d p (%s) %s" % (g["cost"].tolist(), ", ".join(g["wrt"]), g["grad_params"].tolist()))

    def show(it, p, loss, sv):
        for e in range(n):
            verbose("iteration %d env %d: %s  loss %.3e  singular values %s" % (
                it, e, "  ".join("%s %.6g" % (name, v) for name, v in zip(order, p[e].tolist())), float(loss[e]),
                " ".join("%.2e" % s for s in sv[e].tolist())))

    order = tuple(name for name in ENV_PARAMS if name in wrt)
    res = sysid.identify(model, envs, st["qpos"], st["qvel"], st["warm"], ctrl, qpos_obs, qvel_obs, wrt=order, iters=iters, nsub=nsub,
                         fused=fused, callback=show)
    hidden = {name: v[envs.long()] for name, v in real.get_env_params().items()}
    res.update(extra, hidden=hidden, status=torch.maximum(res["status"], status.to(res["status"].device)),
               error={name: (res["params"][name] / hidden[name].to(res["params"][name].device) - 1.0).abs() for name in ENV_PARAMS},
               observable=res["singular_values"][:, -1] > RATIO * res["singular_values"][:, 0])
    for e in range(n):
        got = [name for name in order if float(res["error"][name][e]) <= RECOVERED]
        lost = [name for name in order if name not in got]
        verbose("env %d: recovered %s%s%s" % (e, ", ".join(got) or "nothing", "; NOT recovered: " + ", ".join(lost) if lost else "",
                                              "" if bool(res["observable"][e]) else
                                              "  (smallest singular value %.1e of the largest: a direction in parameter space this log does not determine)"
                                              % float(res["singular_values"][e, -1] / res["singular_values"][e, 0])))
    return res


def hidden_params(cm, n):
    """{name: [n]}: the check values (1.5 x the model's cube mass, friction 0.7, friction loss 0.02, kp_scale 1.2), env e's scaled by 1 + 0.03 e."""
    import numpy as np
    spread = 1.0 + 0.03 * np.arange(n)
    base = {"cube_mass": 1.5 * cm.desc.cube_mass, "cube_friction": 0.7, "cube_frictionloss": 0.02, "kp_scale": 1.2}
    return {name: base[name] * spread for name in ENV_PARAMS}


def contact_states(env, st):
    """st with every env's cube at rest at its gripper site, between the fingers."""
    import torch
    cm = env.cm
    n = int(st["qpos"].shape[0])
    idx = torch.arange(n, dtype=torch.int32, device=st["qpos"].device)
    arm = next(a for a in range(2) if cm.desc.arm_present[a])
    site = env.kinematics_at(envs=idx, qpos=st["qpos"], qvel=st["qvel"], fields=("site_xpos", "status"))["site_xpos"][:, arm]
    out = {k: v.clone() for k, v in st.items()}
    out["qpos"][:, cm.nlink:cm.nlink + 3] = site
    out["qvel"][:, cm.nlink:] = 0.0
    return out


def sweep_controls(cm, st, horizon, close=0.02, swing=0.05):
    """ctrl [n, T, nu]: from the stored ctrl, the gripper joints close by `close` rad a step while the other joints swing by `swing` rad."""
    import math
    import torch
    ctrl = st["ctrl"][:, None, :].repeat(1, horizon, 1)
    arm = next(a for a in range(2) if cm.desc.arm_present[a])
    grip = [int(cm.desc.arm_grip_id[arm][k]) for k in range(2)] if cm.desc.arm_has_grip[arm] else []
    for t in range(horizon):
        for j in range(cm.nu):
            ctrl[:, t, j] += -close * (t + 1) if j in grip else swing * math.sin(0.7 * (t + 1) + j)
    return ctrl


def main(argv=None):
    """Returns the printed record as a dict."""
    import torch
    from gym_kmanip_amd import env_hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4)
    ap.add_argument("--horizon", type=int, default=6)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--wrt", nargs="+", default=list(ENV_PARAMS), choices=ENV_PARAMS, help="the parameters to identify")
    ap.add_argument("--fused", action="store_true", help="linearise with KManipEnvHip.transition_fd (kmanip_transition_fd)")
    ap.add_argument("--device-adjoint", action="store_true", help="print the loss's parameter gradient from KManipEnvHip.adjoint (kmanip_adjoint)")
    ap.add_argument("--no-contact", action="store_true", help="leave the cube where the reset spawned it: only kp_scale is observable")
    args = ap.parse_args(argv)
    real = env_hip.make("KManipSoloArmQPos", num_envs=args.num_envs, seed=args.seed)
    model = env_hip.make("KManipSoloArmQPos", num_envs=args.num_envs, seed=args.seed)
    real.k_reset()
    model.k_reset()
    hidden = hidden_params(real.cm, args.num_envs)
    real.set_env_params(**{name: torch.from_numpy(v).to(real.device) for name, v in hidden.items()})
    st = model.state_tensors()
    if not args.no_contact:
        st = contact_states(model, st)
    ctrl = sweep_controls(model.cm, st, args.horizon)
    res = identify_log(real, model, st, ctrl, wrt=args.wrt, iters=args.iters, fused=args.fused, device_adjoint=args.device_adjoint)
    rec = {"env": "KManipSoloArmQPos", "num_envs": args.num_envs, "horizon": args.horizon, "iters": args.iters, "wrt": list(res["wrt"]),
           "fused": bool(args.fused), "device_adjoint": bool(args.device_adjoint), "contact": not args.no_contact,
           "hidden": {k: v.tolist() for k, v in hidden.items()}, "params": {k: v.cpu().tolist() for k, v in res["params"].items()},
           "error": {k: v.cpu().tolist() for k, v in res["error"].items()}, "loss": res["loss"].cpu().tolist(),
           "singular_values": res["singular_values"].cpu().tolist(), "observable": res["observable"].cpu().tolist(),
           "status": int(res["status"].max()) if args.num_envs else 0}
    print(json.dumps(rec))
    real.k_close()
    model.k_close()
    return rec


if __name__ == "__main__":
    main()
