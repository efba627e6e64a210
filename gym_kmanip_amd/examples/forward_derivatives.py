#!/usr/bin/env python3
"""Linearise the forward dynamics with finite differences (gym_kmanip_amd.derivatives.forward_fd over KManipEnvHip.forward) and test
the linear model on a small step.  Nothing crosses PCIe until the figures are printed.

    python -m gym_kmanip_amd.examples.forward_derivatives [--env KManipSoloArm] [--num-envs 64] [--steps 8] [--scale 1e-4]

After `steps` steps of the scripted policy the envs' states are read on the device, forward_fd gives qacc and its derivatives with
respect to ctrl and the applied force at those states (two forward() launches: the nominal rows, then all perturbed rows), and a
random dctrl (|.| <= scale rad) and dfrc (|.| <= scale N) are drawn.  forward() at the perturbed inputs is compared with the linear
prediction  qacc + dqacc_dctrl dctrl + dqacc_dfrc dfrc.  Printed: the worst gap over all envs relative to the size of the change
the step caused (max |qacc(perturbed) - qacc|), and the worst over the envs whose contact mask did not change.  The dynamics are
piecewise smooth (a contact opening, a friction-loss row saturating, a servo reaching its clamp), so an env that crosses a kink
inside the step shows a gap of order one: the derivative there is a secant, and no bar is attached to the figure."""
import argparse
import json

from gym_kmanip_amd import env_hip
from gym_kmanip_amd.derivatives import forward_fd


def main(argv=None):
    """Returns the printed record as a dict; "worst_rel_gap" is the worst linear-prediction gap."""
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArm")
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--scale", type=float, default=1e-4)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    cm, n = env.cm, args.num_envs
    env.k_reset()
    gen = torch.Generator(device=env.device).manual_seed(args.seed)
    for _ in range(args.steps):
        env.step_flat(env.scripted_action(generator=gen))
    st = env.state_tensors()
    d = forward_fd(env, qpos=st["qpos"], qvel=st["qvel"], ctrl=st["ctrl"], eps=args.eps, wrt=("ctrl", "qfrc_applied"))
    dctrl = (torch.rand((n, cm.nu), dtype=torch.float64, device=env.device, generator=gen) * 2 - 1) * args.scale
    dfrc = (torch.rand((n, cm.nv), dtype=torch.float64, device=env.device, generator=gen) * 2 - 1) * args.scale
    lin = d["qacc"] + torch.bmm(d["dqacc_dctrl"], dctrl[:, :, None])[:, :, 0] + torch.bmm(d["dqacc_dfrc"], dfrc[:, :, None])[:, :, 0]
    f = env.forward(qpos=st["qpos"], qvel=st["qvel"], ctrl=st["ctrl"] + dctrl, warm=d["qacc"], qfrc_applied=dfrc,
                    fields=("qacc", "contact_mask", "status"))
    f0 = env.forward(qpos=st["qpos"], qvel=st["qvel"], ctrl=st["ctrl"], warm=d["qacc"], fields=("contact_mask",))
    ok = (f["status"] == 0) & (d["status"] == 0) & (d["status_fd"] == 0)
    change = (f["qacc"] - d["qacc"]).abs().amax(dim=1)
    rel = (f["qacc"] - lin).abs().amax(dim=1) / change.clamp(min=1e-300)
    rel = torch.where(ok, rel, torch.zeros_like(rel))
    same = ok & (f["contact_mask"] == f0["contact_mask"])
    out = {"env": args.env, "num_envs": n, "steps": args.steps, "scale": args.scale, "eps": args.eps, "rows_ok": int(ok.sum()),
           "rows_same_contacts": int(same.sum()), "worst_rel_gap": float(rel.max()),
           "worst_rel_gap_same_contacts": float(torch.where(same, rel, torch.zeros_like(rel)).max()),
           "median_rel_gap": float(rel.median()), "max_qacc_change": float(change.max())}
    print(json.dumps(out))
    env.k_close()
    return out


if __name__ == "__main__":
    main()
