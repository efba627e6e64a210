#!/usr/bin/env python3
"""Cost of kmanip_gae and kmanip_actor_adam beside the torch arithmetic they replace, measured with HIP events
in one process on one GPU:

    python tests/tools/ppo_update_cost.py [--reps 50] [--out profiles/ppo_update_cost.txt]

KManipSoloArm at 4096 envs; a collect() buffer of 64 steps; the networks 27 -> 64 -> 64 -> act_dim and 27 -> 256 -> 256 -> act_dim.
After WARM untimed rounds, `--reps` rounds; every round times each phase as ONE call between two events of its own, interleaved round
by round so that clock and box drift hit all alike:
  kmanip_gae                 env.gae into given tensors (normalised): two launches
  torch GAE                  the reverse-time loop over the 64 steps in float32 torch, then (adv - mean) / (std + 1e-8)
  kmanip_actor_adam          env.actor_adam with clipping: two launches, both packed buffers rewritten
  torch clip + Adam + repack clip_grad_norm_, torch.optim.Adam.step(), Actor.repack()
GAE does not depend on the network: it is timed once.  An interval holds the call as the stream sees it: the kernels, the event pair
(about 5 us) and what of the Python wrapper the GPU has to wait for.  Reported: mean (min - max).  There is no pass bar; the condition
the project quotes a speed-up under is the library call's max below the torch path's min within one run."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, T, N = 10, 64, 4096
NETS = ((64, 64), (256, 256))
GAMMA, LAM = 0.99, 0.95


def timed(torch, phases, reps):
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

    def report(tag, t, ours, theirs):
        for name in (ours, theirs):
            emit("%-22s %-28s mean %8.1f us  (min %8.1f - max %8.1f)" % (tag, name, statistics.fmean(t[name]), min(t[name]), max(t[name])))
        emit("%-22s library max %s torch min; mean torch / mean library = %.2f"
             % (tag, "below" if max(t[ours]) < min(t[theirs]) else "NOT below", statistics.fmean(t[theirs]) / statistics.fmean(t[ours])))

    env = env_hip.make("KManipSoloArm", num_envs=N, seed=1)
    env.k_reset()
    emit("# library %s, KManipSoloArm, %d envs, T = %d, %d timed rounds after %d warm-up rounds" % (env.L.kmanip_version().decode(), N, T, args.reps, WARM))
    buf = env.collect(Actor(env, hidden=(64, 64)), T, critic=Actor(env, hidden=(64, 64), out_dim=1, seed=1))
    out = env.gae(buf, GAMMA, LAM)

    def torch_gae():
        reward, value, live = buf["reward"].float(), buf["value"], (buf["done"] == 0).float()
        adv, carry = torch.empty_like(reward), torch.zeros_like(reward[0])
        for t in range(T - 1, -1, -1):
            delta = reward[t] + GAMMA * value[t + 1] * live[t] - value[t]
            carry = delta + GAMMA * LAM * live[t] * carry
            adv[t] = carry
        ret = adv + value[:-1]
        return (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8), ret

    t = timed(torch, [("kmanip_gae", lambda: env.gae(buf, GAMMA, LAM, out=out)), ("torch GAE", torch_gae)], args.reps)
    report("T = %d, N = %d" % (T, N), t, "kmanip_gae", "torch GAE")
    for hidden in NETS:
        ours, theirs = Actor(env, hidden=hidden, seed=2), Actor(env, hidden=hidden, seed=2)
        gen = torch.Generator().manual_seed(3)
        grads = {nm: torch.randn(p.shape, generator=gen).to(env.device) for nm, p in zip(("w0", "b0", "w1", "b1", "w2", "b2", "log_std"), ours.parameters())}
        for p, g in zip(theirs.parameters(), grads.values()):
            p.grad = g.clone()
        opt = torch.optim.Adam(theirs.parameters(), lr=3e-4)

        def torch_update():
            torch.nn.utils.clip_grad_norm_(theirs.parameters(), 0.5)
            opt.step()
            theirs.repack()

        t = timed(torch, [("kmanip_actor_adam", lambda: env.actor_adam(ours, 3e-4, max_grad_norm=0.5, grads=grads)),
                          ("torch clip + Adam + repack", torch_update)], args.reps)
        report("27 -> %d -> %d -> %d" % (hidden + (ours.out_dim,)), t, "kmanip_actor_adam", "torch clip + Adam + repack")
    env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
