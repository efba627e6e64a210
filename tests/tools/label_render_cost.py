#!/usr/bin/env python3
"""Cost of the label render (profiles/label_render_cost.txt is this tool's output), measured with
rocprofv3 --kernel-trace --stats on one GPU box:

    python tests/tools/label_render_cost.py collect --parent-tree PARENT --out OUT [--alternations 3] [--links]

PARENT is a built checkout of the parent commit.  Per alternation four profiled child processes, each under a time limit, the
first failure ends the collection: (a) PARENT's `run --mode rgb`, then this tree's (b) `--mode rgb`, (c) `--mode both`, (d)
`--mode seg`.  Then the report: per process and render kernel the launches / median / min / max, and (a) .. (d) over the
alternations with the ratios section 13 holds them to.

`run`: KManipSoloArmVision, 2048 envs, a short step loop, then the id's head + grip_r jobs rendered `--reps` times back to back,
one launch each -- MODE rgb: render_cameras() (k_render_rgb; the only mode the parent can run), both:
render_cameras(segmentation=True) (k_render_labels writing RGB + labels), seg: kmanip_render_labels_multi without RGB buffers.
--tree: the checkout whose package and library run (default: the one this file is in).
--links: set_render_links(True) before the warm-up, the model's default capsule list: every mode then launches
k_render_links, rgb and both its <false, true>, seg its <false, false>; `collect --links` passes the switch to every `run`.
`stats`: the per-kernel lines for directories collected earlier.  The warm-up launches are left out: the last `--reps` launches
of a kernel count."""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM = 4
RUNS = (("a", "rgb", "k_render_rgb<false>"), ("b", "rgb", "k_render_rgb<false>"), ("c", "both", "k_render_labels<false, true>"),
        ("d", "seg", "k_render_labels<false, false>"))
LINK_KERNEL = {"rgb": "k_render_links<false, true>", "both": "k_render_links<false, true>", "seg": "k_render_links<false, false>"}


def run(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.model import CAMERAS, KM_CAM_INDEX
    env = env_hip.make("KManipSoloArmVision", num_envs=args.envs, seed=1)
    env.k_reset()
    for _ in range(args.steps):
        env.step_flat(env.sample_action())
    names = list(env.cm.cameras)
    if args.mode == "rgb":
        out = env.render_cameras()
        call = lambda: env.render_cameras(out=out)
    elif args.mode == "both":
        out = env.render_cameras(segmentation=True)
        call = lambda: env.render_cameras(out=out, segmentation=True)
    else:
        n = len(names)
        seg = [torch.empty((args.envs, CAMERAS[c].h, CAMERAS[c].w), dtype=torch.uint8, device=env.device) for c in names]
        ci = (C.c_int32 * n)(*[KM_CAM_INDEX[c] for c in names])
        hh = (C.c_int32 * n)(*[CAMERAS[c].h for c in names])
        ww = (C.c_int32 * n)(*[CAMERAS[c].w for c in names])
        ps = (C.c_void_p * n)(*[b.data_ptr() for b in seg])
        call = lambda: env._check(env.L.kmanip_render_labels_multi(env.h, n, ci, hh, ww, None, ps, env._stream()), "kmanip_render_labels_multi")
    if args.links:
        env.set_render_links(True)
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        call()
    torch.cuda.synchronize()
    print("label_render_cost: library %s, mode %s%s, %d envs, cameras %s, %d timed launches"
          % (env.L.kmanip_version().decode(), args.mode, " with link capsules" if args.links else "", args.envs, names, args.reps))
    env.k_close()


def kernel_times(d, reps):
    """kernel name -> durations in us of its last `reps` launches, from every *kernel_trace.csv under d."""
    per = {}
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            name = (r.get("Kernel_Name") or r.get("Name") or "").split("(")[0].replace("void ", "")
            if "render" in name:
                per.setdefault(name, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    return {k: [t for _, t in sorted(v)[-reps:]] for k, v in per.items()}


def line(tag, name, v):
    return "%-6s %-44s n %3d  median %7.1f us  min %7.1f  max %7.1f" % (tag, name[:44], len(v), statistics.median(v), min(v), max(v))


def stats(args):
    for d in args.dirs:
        for name, v in sorted(kernel_times(d, args.reps).items()):
            print(line(os.path.basename(d.rstrip("/")), name, v))


def collect(args):
    med = {tag: [] for tag, _, _ in RUNS}
    for i in range(1, args.alternations + 1):
        for tag, mode, kernel in RUNS:
            d = os.path.join(os.path.abspath(args.out), "%d%s" % (i, tag))
            tree = os.path.abspath(args.parent_tree) if tag == "a" else ROOT
            cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt",
                   "--", sys.executable, os.path.abspath(__file__), "run", "--mode", mode, "--tree", tree, "--reps", str(args.reps)] + (["--links"] if args.links else [])
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=tree)
            said = [l for l in p.stdout.splitlines() if l.startswith("label_render_cost:")]
            if p.returncode != 0 or not said:
                print(p.stdout[-2000:], p.stderr[-4000:], sep="\n")
                sys.exit("label_render_cost: run %d%s ended with status %d; nothing more is started" % (i, tag, p.returncode))
            print("# %d%s %s: %s" % (i, tag, "parent commit" if tag == "a" else "this commit", said[-1].split(": ", 1)[1]), flush=True)
            per = kernel_times(d, args.reps)
            for name, v in sorted(per.items()):
                print(line("%d%s" % (i, tag), name, v), flush=True)
            med[tag].append(statistics.median(per[LINK_KERNEL[mode] if args.links else kernel]))
    a, b, c, d = (med[t] for t in "abcd")
    if args.links:
        print("\n(with link capsules: every line below is k_render_links, (a) and (b) its RGB-only launch)")
    print("\n(a) parent k_render_rgb            medians %s us: median %.1f, spread %.1f .. %.1f" % (["%.1f" % x for x in a], statistics.median(a), min(a), max(a)))
    print("(b) this commit's k_render_rgb     medians %s us: median %.1f, (b) / (a) %.3f" % (["%.1f" % x for x in b], statistics.median(b), statistics.median(b) / statistics.median(a)))
    print("(c) k_render_labels RGB + labels   medians %s us: median %.1f, (c) / (a) %.3f   [4/3 = 1.333; two launches = 2]" % (["%.1f" % x for x in c], statistics.median(c), statistics.median(c) / statistics.median(a)))
    print("(d) k_render_labels labels only    medians %s us: median %.1f, (d) / (a) %.3f" % (["%.1f" % x for x in d], statistics.median(d), statistics.median(d) / statistics.median(a)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--mode", choices=["rgb", "both", "seg"], default="rgb")
    r.add_argument("--tree", default=ROOT)
    r.add_argument("--envs", type=int, default=2048)
    r.add_argument("--steps", type=int, default=20)
    r.add_argument("--reps", type=int, default=40)
    r.add_argument("--links", action="store_true", help="set_render_links(True) before the warm-up")
    c = sub.add_parser("collect")
    c.add_argument("--parent-tree", required=True)
    c.add_argument("--out", required=True)
    c.add_argument("--alternations", type=int, default=3)
    c.add_argument("--reps", type=int, default=40)
    c.add_argument("--limit", type=int, default=240, help="seconds per profiled process")
    c.add_argument("--links", action="store_true", help="every run with --links")
    s = sub.add_parser("stats")
    s.add_argument("dirs", nargs="+")
    s.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    {"run": run, "collect": collect, "stats": stats}[a.cmd](a)
