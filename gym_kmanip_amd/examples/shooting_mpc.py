#!/usr/bin/env python3
"""Random-shooting MPC on the device (pipeline.BranchRollouts): at every control step each real env is copied into K candidate
envs (kmanip_copy_envs), the candidates run H sampled actions in one launch (kmanip_step_chunk), and the real env takes the first
action of the candidate with the largest summed reward.  Nothing crosses PCIe inside the loop; the state never leaves the device.

    python -m gym_kmanip_amd.examples.shooting_mpc [--env KManipSoloArm] [--num-envs 256] [--k 16] [--horizon 4] [--steps 32]

A candidate computes exactly what the real env computes with the same actions, so the reward the real env gets at every control
step IS the chosen candidate's predicted first-step reward, bit for bit (main() returns both; the test compares them) -- while no
reset falls inside the horizon: candidates reset to their own cube spawns (BranchRollouts: the reset caveat), so returns are
masked from a candidate's first done byte on.
"""
import argparse
import json

from gym_kmanip_amd import env_hip
from gym_kmanip_amd.pipeline import BranchRollouts


def main(argv=None):
    """Returns {"mean_return": per control step, the mean over the envs of the chosen candidates' predicted returns,
    "realised": [steps, n] and "predicted": [steps, n] float64 host arrays of the real envs' rewards and the chosen candidates'
    first-step rewards}."""
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArm")
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    plan = BranchRollouts(env, args.k)
    env.k_reset()
    realised, predicted, mean_return = [], [], []
    for t in range(args.steps):
        plan.branch()
        acts = plan.sample_actions(args.horizon)
        reward, done = plan.rollout(acts)
        # a candidate's steps after its first done byte belong to another episode (its own spawn): they do not count
        alive = (done != 0).cumsum(0) - (done != 0).long() == 0
        returns = torch.where(alive, reward, torch.zeros_like(reward)).sum(0)
        j, chosen = plan.best(returns)
        env.step_flat(chosen[0].contiguous())
        predicted.append(reward[0, plan.rows, j].clone())
        realised.append(env.reward.clone())
        mean_return.append(returns[plan.rows, j].mean())
    out = {"mean_return": torch.stack(mean_return).cpu().numpy(), "realised": torch.stack(realised).cpu().numpy(),
           "predicted": torch.stack(predicted).cpu().numpy()}
    print(json.dumps({"env": args.env, "num_envs": args.num_envs, "k": args.k, "horizon": args.horizon, "steps": args.steps,
                      "mean_return": [round(float(x), 6) for x in out["mean_return"]]}))
    plan.close()
    env.k_close()
    return out


if __name__ == "__main__":
    main()
