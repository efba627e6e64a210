#!/usr/bin/env python3
"""Inverse dynamics (KManipEnvHip.inverse: MuJoCo's mj_inverse / data.qfrc_inverse) in two uses.  Nothing crosses PCIe inside either loop.

    python -m gym_kmanip_amd.examples.inverse_dynamics --mode residual [--env KManipSoloArm] [--num-envs 256] [--steps 16]
    python -m gym_kmanip_amd.examples.inverse_dynamics --mode hold [--env KManipSoloArmQPos] [--press 0.002] [--steps 8]

--mode residual  the forward/inverse comparison of MuJoCo's mj_compareFwdInv over a short rollout of sampled actions: after every
                 step, forces() solves the forward problem and inverse() is evaluated at its qacc.  At the exact solution
                 qfrc_inverse = qfrc_actuator + qfrc_applied and the two constraint forces agree; what is left is how far the
                 solver stopped from it.  Prints, over all envs and steps, the largest L2 norm of the constraint-force discrepancy
                 and of the applied-force discrepancy (mj_compareFwdInv's two figures), and applied.fwdinv_residual's largest
                 component.
--mode hold      computed-torque holding on a *QPos id: the cube is pressed `press` metres into the table, everything at rest.  A
                 zero action re-targets every servo at the joint's current position, so without help the arm sinks and the table
                 pushes the cube out.  Requesting qacc = 0 from inverse() and binding applied.from_inverse gives the force that
                 compensates gravity AND the contacts: forces()["qacc"] drops to the solver's tolerance and the state stays where
                 it is over `steps` zero-action steps.  Prints max |qacc| and the largest drift of qpos with and without the
                 binding.
"""
import argparse
import json

from gym_kmanip_amd import applied, env_hip


def residual_rollout(env, steps):
    """(constraint-force discrepancy, applied-force discrepancy, fwdinv_residual): each the largest over envs and steps."""
    import torch
    env.k_reset()
    worst = torch.zeros((3,), dtype=torch.float64, device=env.device)
    f = inv = None
    for _ in range(steps):
        env.step_flat(env.sample_action())
        f = env.forces(out=f, fields=("qacc", "qfrc_constraint", "qfrc_actuator", "status"))
        inv = env.inverse(f["qacc"], out=inv, fields=("qfrc_inverse", "qfrc_constraint", "status"))
        ok = ((f["status"] == 0) & (inv["status"] == 0)).to(torch.float64)
        now = torch.stack([((f["qfrc_constraint"] - inv["qfrc_constraint"]).norm(dim=1) * ok).max(),
                           (applied.from_inverse(inv, f).norm(dim=1) * ok).max(),
                           (applied.fwdinv_residual(f, inv) * ok).max()])
        worst = torch.maximum(worst, now)
    return tuple(float(x) for x in worst)


def hold(env, press, steps, compensate):
    """(max |qacc| of the pressed state, largest |qpos - start| after `steps` zero-action steps)."""
    import torch
    cm = env.cm
    nl = cm.nlink
    env.k_reset()
    st = env.state_tensors()
    st["qpos"][:, nl + 2] = cm.desc.table_z + cm.desc.cube_half[2] - press          # the cube's four lower corners `press` into the table
    st["qvel"].zero_()
    env.set_state_tensors(qpos=st["qpos"], qvel=st["qvel"])
    start = st["qpos"].clone()
    act = torch.zeros((env.num_envs, cm.act_dim), dtype=torch.float32, device=env.device)
    zero = torch.zeros((env.num_envs, cm.nv), dtype=torch.float64, device=env.device)
    tau = env.new_applied_force() if compensate else env.bind_applied_force(None)
    qacc = None
    for k in range(steps + 1):
        if compensate:
            # the servo forces of the state do not depend on the applied force: read them with the current binding
            tau.copy_(applied.from_inverse(env.inverse(zero, fields=("qfrc_inverse",)), env.forces(fields=("qfrc_actuator",))))
        if k == 0:
            qacc = float(env.forces(fields=("qacc",))["qacc"].abs().max())
        if k < steps:
            env.step_flat(act)
    drift = float((env.state_tensors()["qpos"] - start).abs().max())
    env.bind_applied_force(None)
    return qacc, drift


def main(argv=None):
    """Returns the printed record as a dict."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("residual", "hold"), default="residual")
    ap.add_argument("--env", default=None)
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--press", type=float, default=0.002)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args(argv)
    if args.mode == "residual":
        env_id = args.env or "KManipSoloArm"
        steps = 16 if args.steps is None else args.steps
        env = env_hip.make(env_id, num_envs=args.num_envs, seed=args.seed)
        dc, da, r = residual_rollout(env, steps)
        out = {"mode": "residual", "env": env_id, "num_envs": args.num_envs, "steps": steps, "fwdinv_constraint_l2": dc,
               "fwdinv_applied_l2": da, "fwdinv_residual_max": r, "solver_tolerance": env.cm.desc.solver_tolerance}
    else:
        env_id = args.env or "KManipSoloArmQPos"
        steps = 8 if args.steps is None else args.steps
        env = env_hip.make(env_id, num_envs=args.num_envs, seed=args.seed, auto_reset=False)
        if not ("q_pos_r" in env.cm.act_slices or "q_pos_l" in env.cm.act_slices):
            raise SystemExit("%s has no joint-delta action key (q_pos_r / q_pos_l): use a *QPos id" % env_id)
        a0, d0 = hold(env, args.press, steps, False)
        a1, d1 = hold(env, args.press, steps, True)
        out = {"mode": "hold", "env": env_id, "num_envs": args.num_envs, "steps": steps, "press_m": args.press,
               "qacc_max_without": a0, "qacc_max_with": a1, "qpos_drift_without": d0, "qpos_drift_with": d1}
    print(json.dumps(out))
    env.k_close()
    return out


if __name__ == "__main__":
    main()
