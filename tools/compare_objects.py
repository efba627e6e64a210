#!/usr/bin/env python3
"""Compare the device code of two builds object by object: the tools/disasm.py listing of every *.o of two csrc directories, the
line that names the file dropped.  One row per object: SHA-256 of the first side's listing, SHA-256 of the second side's, the
listing's length, and "same" or the number of differing lines.  Exit status 1 if any object differs or exists on one side only.
Usage: tools/compare_objects.py <parent csrc> <head csrc> [objects ...]      (both built, e.g. the parent in a `git worktree`)"""
import glob, hashlib, os, subprocess, sys, tempfile

DISASM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "disasm.py")


def listing(obj, tmp):
    """Every code object of `obj`, disassembled: the lines without the one that carries the file name."""
    for f in glob.glob(os.path.join(tmp, "x.*")):
        os.remove(f)
    subprocess.run([sys.executable, DISASM, obj, os.path.join(tmp, "x")], check=True, capture_output=True)
    return [l for s in sorted(glob.glob(os.path.join(tmp, "x.*.s"))) for l in open(s).read().split("\n") if "file format" not in l]


def main(argv):
    a_dir, b_dir = argv[1:3]
    names = argv[3:] or sorted({os.path.basename(p) for d in (a_dir, b_dir) for p in glob.glob(os.path.join(d, "*.o"))})
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            pa, pb = os.path.join(a_dir, n), os.path.join(b_dir, n)
            if not (os.path.exists(pa) and os.path.exists(pb)):
                print("%-34s on one side only" % n)
                bad += 1
                continue
            a, b = listing(pa, tmp), listing(pb, tmp)
            ha, hb = (hashlib.sha256("\n".join(x).encode()).hexdigest() for x in (a, b))
            diff = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
            bad += diff != 0
            print("%-34s %s %s %6d lines  %s" % (n, ha, hb, len(a), "same" if not diff else "DIFFERENT: %d lines" % diff), flush=True)
    print("%d objects, %d different" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
