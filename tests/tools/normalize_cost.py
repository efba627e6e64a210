#!/usr/bin/env python3
"""Cost of kmanip_obs_stats and kmanip_reward_scale beside the torch float64 arithmetic they replace, measured
with HIP events in one process on one GPU:

    python tests/tools/normalize_cost.py [--reps 50] [--out profiles/normalize_cost.txt]

KManipSoloArm at 4096 envs; a collect() buffer of 64 steps (obs_dim 27).  After WARM untimed rounds, `--reps` rounds; every round times
each phase as ONE call between two events of its own, interleaved round by round so that clock and box drift hit all alike:
  kmanip_obs_stats        ObsStats.update(buf["obs"][:T]): two launches
  torch obs statistics    mean and var (unbiased=False) over the T N rows, Chan's merge into a running (count, mean, M2), inv_std
  kmanip_reward_scale     RewardScale.update(buf): two launches
  torch reward scaling    the forward loop over the T steps (G = gamma G + r, collected, G cut where done), mean and var of the
                          returns, the merge, reward / sqrt(var + eps)
An interval holds the call as the stream sees it: the kernels, the event pair (about 5 us) and what of the Python wrapper the GPU has
to wait for.  Reported: mean (min - max), and for the obs call the bytes it has to read over the mean interval -- an END-TO-END rate
of a two-launch call, not k_obs_stats' share of the memory system's peak.  There is no pass bar; the condition the project quotes a
speed-up under is the library call's max below the torch path's min within one run."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, T, N = 10, 64, 4096
GAMMA, EPS = 0.99, 1e-8


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
    from gym_kmanip_amd.normalize import ObsStats, RewardScale
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def report(tag, t, ours, theirs):
        for name in (ours, theirs):
            emit("%-22s %-24s mean %8.1f us  (min %8.1f - max %8.1f)" % (tag, name, statistics.fmean(t[name]), min(t[name]), max(t[name])))
        emit("%-22s library max %s torch min; mean torch / mean library = %.2f"
             % (tag, "below" if max(t[ours]) < min(t[theirs]) else "NOT below", statistics.fmean(t[theirs]) / statistics.fmean(t[ours])))

    env = env_hip.make("KManipSoloArm", num_envs=N, seed=1)
    env.k_reset()
    emit("# library %s, KManipSoloArm, %d envs, T = %d, %d timed rounds after %d warm-up rounds" % (env.L.kmanip_version().decode(), N, T, args.reps, WARM))
    buf = env.collect(Actor(env, hidden=(64, 64)), T, critic=Actor(env, hidden=(64, 64), out_dim=1, seed=1))
    obs, dim = buf["obs"][:T], env.cm.obs_dim
    stats, scale = ObsStats(env), RewardScale(env, GAMMA, EPS)
    run = {"n": 0.0, "mean": torch.zeros(dim, dtype=torch.float64, device=env.device), "M2": torch.zeros(dim, dtype=torch.float64, device=env.device)}
    ret = {"n": 0.0, "mean": torch.zeros((), dtype=torch.float64, device=env.device), "M2": torch.zeros((), dtype=torch.float64, device=env.device),
           "G": torch.zeros(N, dtype=torch.float64, device=env.device)}

    def merge(s, x, axis):
        R, mb = float(x.numel() // max(s["mean"].numel(), 1)), x.mean(axis)
        M2b = x.var(axis, unbiased=False) * R
        n, delta = s["n"] + R, mb - s["mean"]
        s["mean"], s["M2"], s["n"] = s["mean"] + delta * (R / n), s["M2"] + M2b + delta * delta * (s["n"] * R / n), n
        return s["M2"] / n

    def torch_obs():
        return run["mean"], 1.0 / torch.sqrt(merge(run, obs.reshape(-1, dim), 0) + EPS)

    def torch_reward():
        G, every, live = ret["G"], torch.empty_like(buf["reward"]), buf["done"] == 0
        for t in range(T):
            G = GAMMA * G + buf["reward"][t]
            every[t] = G
            G = G * live[t]
        ret["G"] = G
        return buf["reward"] / torch.sqrt(merge(ret, every.reshape(-1), 0) + EPS)

    t = timed(torch, [("kmanip_obs_stats", lambda: stats.update(obs)), ("torch obs statistics", torch_obs),
                      ("kmanip_reward_scale", lambda: scale.update(buf)), ("torch reward scaling", torch_reward)], args.reps)
    report("obs [%d, %d]" % (T * N, dim), t, "kmanip_obs_stats", "torch obs statistics")
    nbytes = 8 * T * N * dim
    emit("%-22s reads %.1f MB: %.0f GB/s over the mean interval, %.0f GB/s over the shortest (end to end: two launches and an event pair)"
         % ("", nbytes / 1e6, nbytes / statistics.fmean(t["kmanip_obs_stats"]) / 1e3, nbytes / min(t["kmanip_obs_stats"]) / 1e3))
    report("reward [%d, %d]" % (T, N), t, "kmanip_reward_scale", "torch reward scaling")
    env.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
