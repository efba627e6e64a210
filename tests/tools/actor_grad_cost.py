#!/usr/bin/env python3
"""Cost of kmanip_actor_grad beside torch float32 forward plus autograd backward of the same loss on Actor's tensors (DESIGN.md
section 46), measured with HIP events in one process on one GPU:

    python tests/tools/actor_grad_cost.py [--reps 50] [--out profiles/actor_grad_cost.txt]

The PPO head on n = 4096 and n = 65536 records (random observations, raw = mean + noise, rho near 1 so that most rows are active), the
networks 27 -> 64 -> 64 -> 7 and 27 -> 256 -> 256 -> 7, tanh, with an observation normaliser.  After WARM untimed rounds, `--reps`
rounds; every round times each phase as ONE call between two events of its own -- actor_grad into given tensors (three launches);
the torch program (cast, normalise, three addmm, two tanh, the clipped surrogate, backward(), which leaves .grad on the seven
parameters) -- interleaved round by round so that clock and box drift hit both alike.  An interval holds the call as the stream
sees it: the kernels, the event pair and what of the Python wrapper the GPU has to wait for.  Reported: mean (min - max).  There is no
pass bar; the condition the project quotes a speed-up under is kernel max below torch min within one run."""
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
            mean = env.actor_eval(actor, obs, envs=torch.zeros(n, dtype=torch.int32, device=dev), deterministic=True)["mean"]
            raw = mean + math.exp(-0.5) * torch.randn((n, 7), generator=gen).to(dev)
            z = (raw - mean) / math.exp(-0.5)
            logp_old = (-0.5 * z * z + 0.5 - 0.5 * math.log(2 * math.pi)).sum(-1).double() + 0.1 * torch.randn((n,), generator=gen, dtype=torch.float64).to(dev)
            ppo = dict(raw=raw, logp_old=logp_old, adv=torch.randn((n,), generator=gen).to(dev), clip=CLIP)
            out = env.actor_grad(actor, obs, ppo=ppo, set_grad=False)
            leaves = [p.clone().requires_grad_() for p in actor.parameters()]
            lp32, om, oi = logp_old.float(), actor.obs_mean.float(), actor.obs_inv_std.float()

            def torch_grad():
                w0, b0, w1, b1, w2, b2, ls = leaves
                for p in leaves:
                    p.grad = None
                x = (obs.to(torch.float32) - om) * oi
                m = torch.addmm(b2, torch.tanh(torch.addmm(b1, torch.tanh(torch.addmm(b0, x, w0.T)), w1.T)), w2.T)
                u = (raw - m) / ls.exp()
                rho = ((-0.5 * u * u - ls - 0.5 * math.log(2 * math.pi)).sum(-1) - lp32).exp()
                (-torch.minimum(rho * ppo["adv"], rho.clamp(1 - CLIP, 1 + CLIP) * ppo["adv"])).mean().backward()

            torch_grad()
            agree = max(float((out[k] - p.grad).abs().max() / p.grad.abs().max()) for k, p in zip(("w0", "b0", "w1", "b1", "w2", "b2", "log_std"), leaves))
            phases = [("kmanip_actor_grad", lambda: env.actor_grad(actor, obs, ppo=ppo, out=out, set_grad=False)), ("torch float32 autograd", torch_grad)]
            t = {name: [] for name, _ in phases}
            for k in range(WARM + args.reps):
                for name, f in phases:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); f(); b.record()
                    b.synchronize()
                    if k >= WARM:
                        t[name].append(a.elapsed_time(b) * 1e3)
            tag = "27 -> %d -> %d -> 7, n = %5d" % (hidden + (n,))
            for name, _ in phases:
                emit("%-32s %-24s mean %9.1f us  (min %9.1f - max %9.1f)" % (tag, name, statistics.fmean(t[name]), min(t[name]), max(t[name])))
            emit("%-32s kernel max %s torch min; mean torch / mean kernel = %.2f; worst relative difference of the two gradients %.1e"
                 % (tag, "below" if max(t["kmanip_actor_grad"]) < min(t["torch float32 autograd"]) else "NOT below",
                    statistics.fmean(t["torch float32 autograd"]) / statistics.fmean(t["kmanip_actor_grad"]), agree))
    env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
