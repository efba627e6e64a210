#!/usr/bin/env python3
"""Cost of the depth render with link capsules (profiles/depth_links_cost.txt is this tool's output),
measured with rocprofv3 --kernel-trace --stats (no counters, no other tracing) on one GPU box:

    python tests/tools/depth_links_cost.py collect --out OUT

One profiled child process under a time limit: `run` -- KManipSoloArm, 2048 envs, a short step loop, the default capsule list,
then per camera (grip_r: BASELINE config 5's image, several whole-image capsule rectangles; head: far fewer rectangles over a
pixel) at 64 x 64 two phases of WARM + `--reps` back-to-back render_depth launches: the depth flag off (k_render_depth<true, false>,
the parent's code) and on (k_render_depth_links<true, false>).  The report: per phase the kernel, its launches, median / min / max
of the last `--reps`, and per camera the ratio of the two medians -- both kernels from the SAME run."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 4
CAMS = ("grip_r", "head")
PHASES = [(cam, on) for cam in CAMS for on in (False, True)]
KERNEL = {False: "k_render_depth<true, false>", True: "k_render_depth_links<true, false>"}


def run(args):
    sys.path.insert(0, ROOT)
    import torch
    from gym_kmanip_amd import env_hip
    env = env_hip.make("KManipSoloArm", num_envs=args.envs, seed=1)
    env.k_reset()
    for _ in range(args.steps):
        env.step_flat(env.sample_action())
    env.set_render_links(True)
    out = env.render_depth("grip_r", 64, 64)
    torch.cuda.synchronize()
    nearer = {}
    for cam, on in PHASES:
        env.set_depth_links(on)
        for _ in range(WARM + args.reps):
            env.render_depth(cam, 64, 64, out=out)
        torch.cuda.synchronize()
        if not on:
            base = out.clone()
        else:
            nearer[cam] = float((out < base).float().mean())
    print("depth_links_cost: library %s, %d envs, %d capsules, 64 x 64, %d timed launches per phase, capsule pixels %s"
          % (env.L.kmanip_version().decode(), args.envs, len(env.get_render_links()), args.reps,
             ", ".join("%s %.1f %%" % (c, 100 * nearer[c]) for c in CAMS)))
    env.k_close()


def launches(d):
    """(start, kernel name, duration in us) of every depth render launch in the *kernel_trace.csv files under d, by start time."""
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            name = (r.get("Kernel_Name") or r.get("Name") or "").split("(")[0].replace("void ", "")
            if name.startswith("k_render_depth"):
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    return sorted(rows)


def report(d, reps):
    rows = launches(d)[1:]                               # (the first launch allocated the buffer)
    per = WARM + reps
    assert len(rows) == per * len(PHASES), "expected %d depth launches, found %d" % (per * len(PHASES) + 1, len(rows) + 1)
    med = {}
    for i, (cam, on) in enumerate(PHASES):
        ph = rows[i * per:(i + 1) * per]
        assert all(r[1].startswith(KERNEL[on][:-1]) for r in ph), (cam, on, sorted({r[1] for r in ph}))
        v = [r[2] for r in ph[-reps:]]
        med[(cam, on)] = statistics.median(v)
        print("%-7s flag %-3s %-36s n %3d  median %7.1f us  min %7.1f  max %7.1f" % (cam, "on" if on else "off", KERNEL[on], len(v), med[(cam, on)], min(v), max(v)))
    for cam in CAMS:
        print("%-7s k_render_depth_links / k_render_depth = %.2f  (%.1f us / %.1f us)"
              % (cam, med[(cam, True)] / med[(cam, False)], med[(cam, True)], med[(cam, False)]))


def collect(args):
    d = os.path.abspath(args.out)
    cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt",
           "--", sys.executable, os.path.abspath(__file__), "run", "--reps", str(args.reps), "--envs", str(args.envs)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    said = [l for l in p.stdout.splitlines() if l.startswith("depth_links_cost:")]
    if p.returncode != 0 or not said:
        print(p.stdout[-2000:], p.stderr[-4000:], sep="\n")
        sys.exit("depth_links_cost: the profiled run ended with status %d" % p.returncode)
    print("# " + said[-1].split(": ", 1)[1])
    report(d, args.reps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    c = sub.add_parser("collect")
    c.add_argument("--out", required=True)
    c.add_argument("--limit", type=int, default=240, help="seconds for the profiled process")
    s = sub.add_parser("stats")
    s.add_argument("dir")
    for q in (r, c, s):
        q.add_argument("--reps", type=int, default=40)
    for q in (r, c):
        q.add_argument("--envs", type=int, default=2048)
    r.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    {"run": run, "collect": collect, "stats": lambda a: report(a.dir, a.reps)}[a.cmd](a)
