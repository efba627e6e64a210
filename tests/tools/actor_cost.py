#!/usr/bin/env python3
"""Cost of kmanip_actor beside the same policy as a torch float32 program, and of collect beside the hand loop with the torch policy
(DESIGN.md section 45), measured with HIP events in one process on one GPU:

    python tests/tools/actor_cost.py [--reps 100] [--out profiles/actor_cost.txt]

KManipSoloArm at 4096 envs, after a reset and 12 sampled steps; the networks 27 -> 256 -> 256 -> act_dim and 27 -> 64 -> 64 -> act_dim,
tanh, with an observation normaliser.  After WARM untimed rounds, `--reps` rounds; every round times each phase as ONE call between
two events of its own -- kmanip_actor with the head (actor_eval into given tensors); Actor.torch_eval (cast, normalise, three addmm,
two tanh, randn, clamp, log-probability) -- interleaved round by round so that clock and box drift hit both alike.  An interval holds
the call as the stream sees it: the kernels, the event pair (about 5 us) and what of the Python wrapper the GPU has to wait for.
Then, per network, ROLL rounds of a STEPS-step rollout, again interleaved: collect (policy, kmanip_step; no critic) against the hand
loop of torch_eval and step_flat, wall clock around one synchronisation, in env steps per second.  Reported: mean (min - max).  There
is no pass bar; the condition the project quotes a speed-up under is kernel max below torch min within one run."""
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
        out = env.actor_eval(actor, obs)
        phases = [("kmanip_actor", lambda: env.actor_eval(actor, obs, out=out)), ("torch float32 policy", lambda: actor.torch_eval(obs))]
        t = {name: [] for name, _ in phases}
        for k in range(WARM + args.reps):
            for name, f in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        tag = "27 -> %d -> %d -> %d" % (hidden + (actor.out_dim,))
        for name, _ in phases:
            emit("%-22s %-22s mean %8.1f us  (min %8.1f - max %8.1f)" % (tag, name, statistics.fmean(t[name]), min(t[name]), max(t[name])))
        emit("%-22s kernel max %s torch min; mean torch / mean kernel = %.2f"
             % (tag, "below" if max(t["kmanip_actor"]) < min(t["torch float32 policy"]) else "NOT below",
                statistics.fmean(t["torch float32 policy"]) / statistics.fmean(t["kmanip_actor"])))
        buf = env.collect(actor, STEPS)

        def hand_loop():
            o = env.observe()[0]
            for _ in range(STEPS):
                o = env.step_flat(actor.torch_eval(o)[0])[0]

        rolls = [("collect", lambda: env.collect(actor, STEPS, out=buf)), ("hand loop, torch policy", hand_loop)]
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
