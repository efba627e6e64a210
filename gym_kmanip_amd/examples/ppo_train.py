#!/usr/bin/env python3
"""A few iterations of PPO with every piece of arithmetic in the library.

    python -m gym_kmanip_amd.examples.ppo_train [--env KManipSoloArm] [--num-envs 1024] [--iterations 5] [--steps 16] [--hidden 64 64]
                                                [--normalize-obs] [--normalize-reward]

gym_kmanip_amd.ppo.PPO: per iteration KManipEnvHip.collect (policy, critic and step back to back), gae (kmanip_gae: advantages and
returns), and per epoch and minibatch actor_grad + actor_adam for the policy and for the critic (kmanip_actor_grad, kmanip_actor_adam:
the clipped surrogate and the squared error, gradient clipping, Adam, both packed weight copies rewritten in the same pass).
--normalize-obs and --normalize-reward add the running statistics of gym_kmanip_amd.normalize (kmanip_obs_stats, kmanip_reward_scale).  Nothing
synchronises inside an iteration; the printed record is read back once per iteration: the mean reward of the rollout and the losses
of the first and the last update."""
import argparse
import json

from gym_kmanip_amd import env_hip
from gym_kmanip_amd.actor import Actor
from gym_kmanip_amd.ppo import PPO


def main(argv=None):
    """Returns the printed records as a list of dicts."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="KManipSoloArm")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--hidden", type=int, nargs=2, default=(64, 64))
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--normalize-obs", action="store_true")
    ap.add_argument("--normalize-reward", action="store_true")
    args = ap.parse_args(argv)
    env = env_hip.make(args.env, num_envs=args.num_envs, seed=args.seed)
    env.k_reset()
    actor = Actor(env, hidden=tuple(args.hidden), seed=args.seed)
    critic = Actor(env, hidden=tuple(args.hidden), out_dim=1, seed=args.seed + 1)
    actor.log_std.fill_(-0.5)
    ppo = PPO(env, actor, critic, nsteps=args.steps, lr=args.lr, seed=args.seed, normalize_obs=args.normalize_obs,
              normalize_reward=args.normalize_reward)
    recs = []
    for it in range(args.iterations):
        r = ppo.iterate()
        recs.append({"iteration": it, "mean_reward": float(r["reward"]), "policy_loss": [float(r["policy_loss"][0, 0]), float(r["policy_loss"][-1, -1])],
                     "value_loss": [float(r["value_loss"][0, 0]), float(r["value_loss"][-1, -1])], "adv_std": float(r["adv_stats"][1])})
        print(json.dumps(recs[-1]))
    env.k_close()
    return recs


if __name__ == "__main__":
    main()
