#!/usr/bin/env python3
"""Cost of the device-state paths (profiles/state_dev_cost.txt is this tool's output), measured with HIP events
in one process on one GPU:

    python tests/tools/state_dev_cost.py [--reps 100] [--out profiles/state_dev_cost.txt]

For KManipSoloArm and KManipTorso, on a 4096-env handle after a reset and 12 sampled steps:
  state_tensors / set_state_tensors of the whole handle (NULL index, preallocated tensors);
  copy_envs_from another 4096-env handle: identity, 64 sources 64 times each, one source 4096 times; a same-handle reversal
  (two launches through the staging copy);
  one kmanip_step of the handle (sampled actions drawn outside the timed interval);
  the host route to the same result, get_state + set_state (kmanip_get_state / kmanip_set_state: device-wide synchronisation,
  PCIe both ways, CPU transposes), by the wall clock around a synchronised call pair.
After WARM untimed rounds, `--reps` rounds; in every round each device phase is ONE call between two events of its own, the phases
interleaved round by round so that clock and box drift hit all of them alike.  What such an interval holds is the CALL as the
stream sees it: the kernel plus the event pair (about 5 us) plus whatever of the Python wrapper's argument checks and the launch
the GPU has to wait for -- for kernels of a few microseconds that is most of it.  So the figures are call costs, an upper bound of
the kernel times, and the column computed from them is named "per call", not a memory rate; kernel times come from a kernel trace
of this same tool (rocprofv3 --kernel-trace --stats -- python tests/tools/state_dev_cost.py), a run of its own.  Reported: median /
min / max in us, the bytes the path reads plus writes and bytes per call time, the ratio of the host route to the device path, and
the one condition: a whole-handle copy must take less time than one step of that handle in the same run (call overhead counts
against the copy, so the condition is met with room when it is met here)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 10
N = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip
    lines, ok = [], True

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for env_id in ("KManipSoloArm", "KManipTorso"):
        env = env_hip.make(env_id, num_envs=N, seed=1)
        other = env_hip.make(env_id, num_envs=N, seed=2, env_id_offset=N)
        for e in (env, other):
            e.k_reset()
            for _ in range(12):
                e.step_flat(e.sample_action())
        cm = env.cm
        row_bytes = 8 * (cm.nq + 2 * cm.nv + cm.nu) + 4          # the four float64 fields and the step counter
        T = env.state_tensors()
        act = env.sample_action()
        dev = env.device
        ident = torch.arange(N, dtype=torch.int32, device=dev)
        src64 = ident % 64
        src1 = torch.zeros(N, dtype=torch.int32, device=dev)
        rev = torch.flip(ident, [0])
        env.copy_envs_from(env, src_envs=ident, dst_envs=ident)  # (allocates the staging copy: the one call that synchronises)
        # bytes read + written: state_tensors also carries the episode counter
        phases = [("kmanip_step", lambda: env.step_flat(act), None),
                  ("state_tensors, whole handle", lambda: env.state_tensors(out=T), 2 * N * (row_bytes + 4)),
                  ("set_state_tensors, whole handle", lambda: env.set_state_tensors(**T), 2 * N * (row_bytes + 4)),
                  ("copy_envs 4096 -> 4096 identity", lambda: env.copy_envs_from(other, env_params=False), 2 * N * row_bytes),
                  ("copy_envs 64 -> 4096 (each 64 x)", lambda: env.copy_envs_from(other, src_envs=src64, env_params=False), N * row_bytes + 64 * row_bytes),
                  ("copy_envs 1 -> 4096", lambda: env.copy_envs_from(other, src_envs=src1, env_params=False), N * row_bytes + row_bytes),
                  ("copy_envs same handle, reversed", lambda: env.copy_envs_from(env, src_envs=rev, dst_envs=ident, env_params=False), 4 * N * row_bytes)]
        t = {name: [] for name, _, _ in phases}
        for k in range(WARM + args.reps):
            # every round starts from a state of a natural rollout: `other` takes one step and the handle becomes its copy (the
            # broadcast copies below leave every env alike, which is no state to time a step on)
            other.step_flat(other.sample_action())
            env.copy_envs_from(other, episode=True, env_params=False)
            env.sample_action(act)
            for name, f, _ in phases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                b.synchronize()
                if k >= WARM:
                    t[name].append(a.elapsed_time(b) * 1e3)
        host = []
        for k in range(2 + args.host_reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            st = env.get_state()
            env.set_state(*st)
            torch.cuda.synchronize(dev)
            if k >= 2:
                host.append((time.perf_counter() - t0) * 1e6)
        emit("# library %s, %s, %d envs (nq %d nv %d nu %d: %d state bytes per env), %d timed rounds after %d warm-up rounds"
             % (env.L.kmanip_version().decode(), env_id, N, cm.nq, cm.nv, cm.nu, row_bytes, args.reps, WARM))
        med = {name: statistics.median(v) for name, v in t.items()}
        for name, _, nbytes in phases:
            rate = "" if nbytes is None else "  %6.2f MB moved, %7.1f GB/s per call (overheads included)" % (nbytes / 1e6, nbytes / med[name] / 1e3)
            emit("%-14s %-34s median %8.1f us  min %8.1f  max %8.1f%s" % (env_id, name, med[name], min(t[name]), max(t[name]), rate))
        hm = statistics.median(host)
        dev_pair = med["state_tensors, whole handle"] + med["set_state_tensors, whole handle"]
        emit("%-14s %-34s median %8.1f us  min %8.1f  max %8.1f  (wall clock, %d calls): x %.0f of state_tensors + set_state_tensors (%.1f us)"
             % (env_id, "host get_state + set_state", hm, min(host), max(host), args.host_reps, hm / dev_pair, dev_pair))
        ratio = med["copy_envs 4096 -> 4096 identity"] / med["kmanip_step"]
        good = ratio < 1.0
        ok = ok and good
        emit("%-14s whole-handle copy_envs / kmanip_step = %.3f  (condition: < 1)  %s" % (env_id, ratio, "OK" if good else "FAILED"))
        env.k_close(); other.k_close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
