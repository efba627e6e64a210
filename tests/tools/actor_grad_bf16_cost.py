#!/usr/bin/env python3
"""Cost of kmanip_actor_grad_bf16 beside kmanip_actor_grad, measured with HIP events in one process on one GPU:

    python tests/tools/actor_grad_bf16_cost.py [--reps 50] [--out profiles/actor_grad_bf16_cost.txt]

Section 46's four points: the PPO head on n = 4096 and n = 65536 records, the networks 27 -> 64 -> 64 -> 7 and 27 -> 256 -> 256 -> 7,
tanh, with an observation normaliser; raw and logp_old come from the bf16 policy.  After WARM untimed rounds, `--reps` rounds; every
round times each call between two events of its own, the two precisions interleaved round by round so that clock and box drift hit
both alike.  An interval holds the call as the stream sees it: its three launches, the event pair and what of the Python wrapper the
GPU has to wait for.  Reported: mean (min - max), and whether the bf16 max is below the float32 min.  There is no pass bar."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, CLIP = 10, 0.2
NETS, ROWS = ((64, 64), (256, 256)), (4096, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.actor import Actor
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    env = env_hip.make("KManipSoloArm", num_envs=64, seed=1)
    dev, gen = env.device, torch.Generator().manual_seed(1)
    emit("# library %s, PPO head, %d timed rounds after %d warm-up rounds" % (env.L.kmanip_version().decode(), args.reps, WARM))
    for hidden in NETS:
        for n in ROWS:
            actor = Actor(env, hidden=hidden, activation="tanh", in_dim=27, out_dim=7)
            actor.log_std.fill_(-0.5)
            obs = torch.randn((n, 27), generator=gen, dtype=torch.float64).to(dev)
            actor.obs_mean, actor.obs_inv_std = obs.mean(0), 1.0 / (obs.std(0) + 1e-3)
            mean = env.actor_eval(actor, obs, envs=torch.zeros(n, dtype=torch.int32, device=dev), deterministic=True, precision="bf16")["mean"]
            raw = mean + math.exp(-0.5) * torch.randn((n, 7), generator=gen).to(dev)
            z = (raw - mean) / math.exp(-0.5)
            logp_old = (-0.5 * z * z + 0.5 - 0.5 * math.log(2 * math.pi)).sum(-1).double() + 0.1 * torch.randn((n,), generator=gen, dtype=torch.float64).to(dev)
            ppo = dict(raw=raw, logp_old=logp_old, adv=torch.randn((n,), generator=gen).to(dev), clip=CLIP)
            outs = {p: env.actor_grad(actor, obs, ppo=ppo, set_grad=False, precision=p) for p in ("bf16", "f32")}
            apart = max(float((outs["bf16"][k] - outs["f32"][k]).abs().max() / outs["f32"][k].abs().max()) for k in ("w0", "b0", "w1", "b1", "w2", "b2", "log_std"))
            names = {"bf16": "kmanip_actor_grad_bf16", "f32": "kmanip_actor_grad"}
            t = {p: [] for p in names}
            for k in range(WARM + args.reps):
                for p in names:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); env.actor_grad(actor, obs, ppo=ppo, out=outs[p], set_grad=False, precision=p); b.record()
                    b.synchronize()
                    if k >= WARM:
                        t[p].append(a.elapsed_time(b) * 1e3)
            tag = "27 -> %d -> %d -> 7, n = %5d" % (hidden + (n,))
            for p, name in names.items():
                emit("%-32s %-24s mean %9.1f us  (min %9.1f - max %9.1f)" % (tag, name, statistics.fmean(t[p]), min(t[p]), max(t[p])))
            emit("%-32s bf16 max %s float32 min; mean float32 / mean bf16 = %.2f; the two gradients are %.1e of a tensor's largest entry apart"
                 % (tag, "below" if max(t["bf16"]) < min(t["f32"]) else "NOT below", statistics.fmean(t["f32"]) / statistics.fmean(t["bf16"]), apart))
    env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
