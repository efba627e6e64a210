#!/usr/bin/env python3
"""Cost of kmanip_actor_bf16 beside kmanip_actor, and of collect in both precisions beside the hand loop with the torch policy
(DESIGN.md section 49), measured with HIP events in one process on one GPU:

    python tests/tools/actor_bf16_cost.py [--reps 100] [--out profiles/actor_bf16_cost.txt]

KManipSoloArm at 4096 envs, after a reset and 12 sampled steps; the networks 27 -> 256 -> 256 -> act_dim and 27 -> 64 -> 64 -> act_dim,
tanh, with an observation normaliser.  After WARM untimed rounds, `--reps` rounds; every round times each call -- actor_eval with the
head into given tensors, precision "f32" and "bf16" -- as ONE call between two events of its own, interleaved round by round so that
clock and box drift hit both alike.  An interval holds the call as the stream sees it: the kernel, the event pair (about 5 us) and
what of the Python wrapper the GPU has to wait for.  Then, at 256 x 256, ROLL rounds of a STEPS-step rollout, again interleaved:
collect in both precisions (policy, kmanip_step; no critic) against the hand loop of Actor.torch_eval and step_flat, wall clock around
one synchronisation, in env steps per second.  Reported: mean (min - max), and the bf16 mean's distance from the float32 call's.
There is no pass bar; the condition the project quotes a speed-up under is bf16 max below float32 min within one run."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ROLL, STEPS, N = 10, 5, 64, 4096
NETS = ((256, 256), (64, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
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

    env = env_hip.make("KManipSoloArm", num_envs=N, seed=1)
    env.k_reset()
    for _ in range(12):
        env.step_flat(env.sample_action())
    obs = env.obs.clone()
    emit("# library %s, KManipSoloArm, %d envs, %d timed rounds after %d warm-up rounds" % (env.L.kmanip_version().decode(), N, args.reps, WARM))
    for hidden in NETS:
        actor = Actor(env, hidden=hidden, activation="tanh")
        actor.log_std.fill_(-0.5)
        actor.obs_mean, actor.obs_inv_std = obs.mean(0), 1.0 / (obs.std(0) + 1e-3)
        actor.repack_bf16()
        outs = {p: env.actor_eval(actor, obs, precision=p) for p in ("f32", "bf16")}
        names = {"f32": "kmanip_actor", "bf16": "kmanip_actor_bf16"}
        t = {p: [] for p in names}
        for k in range(WARM + args.reps):
            for p in names:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); env.actor_eval(actor, obs, out=outs[p], precision=p); b.record()
                b.synchronize()
                if k >= WARM:
                    t[p].append(a.elapsed_time(b) * 1e3)
        tag = "27 -> %d -> %d -> %d" % (hidden + (actor.out_dim,))
        for p, name in names.items():
            emit("%-22s %-22s mean %8.1f us  (min %8.1f - max %8.1f)" % (tag, name, statistics.fmean(t[p]), min(t[p]), max(t[p])))
        emit("%-22s bf16 max %s float32 min; mean float32 / mean bf16 = %.2f; worst |mean bf16 - mean float32| %.3e"
             % (tag, "below" if max(t["bf16"]) < min(t["f32"]) else "NOT below", statistics.fmean(t["f32"]) / statistics.fmean(t["bf16"]),
                float((outs["bf16"]["mean"] - outs["f32"]["mean"]).abs().max())))
        if hidden != NETS[0]:
            continue
        buf = env.collect(actor, STEPS)

        def hand_loop():
            o = env.observe()[0]
            for _ in range(STEPS):
                o = env.step_flat(actor.torch_eval(o)[0])[0]

        rolls = [("collect, f32", lambda: env.collect(actor, STEPS, out=buf)), ("collect, bf16", lambda: env.collect(actor, STEPS, out=buf, precision="bf16")),
                 ("hand loop, torch policy", hand_loop)]
        r = {name: [] for name, _ in rolls}
        for k in range(1 + ROLL):
            for name, f in rolls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                if k >= 1:
                    r[name].append(STEPS * N / (time.perf_counter() - t0))
        for name, _ in rolls:
            emit("%-22s %-24s mean %10.0f env steps/s  (min %10.0f - max %10.0f), %d rollouts of %d steps"
                 % (tag, name, statistics.fmean(r[name]), min(r[name]), max(r[name]), ROLL, STEPS))
    env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
