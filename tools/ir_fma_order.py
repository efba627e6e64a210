#!/usr/bin/env python3
"""Which product of a * b + c * d does the compiler fuse?  Compare two builds of one kernel in the optimised LLVM IR.

With -ffp-contract=fast the back end turns `fadd (fmul a, b), (fmul c, d)` into fma(a, b, rnd(c * d)): the FIRST operand's product is
fused, the second is rounded on its own.  Addition commutes, so the optimiser may swap the operands -- and does, when the code around an
expression moves (values arriving from a lane gather instead of an LDS load, a loop unrolled differently).  The result then differs in
its last bit although no source expression changed.  An ISA listing does not show it (the same mul + fma pair either way); the IR does:
every fmul carries the line and column of ITS product, so for each fadd / fsub of two products this tool says whether they still stand
in source order.

  hipcc -O3 ... -S -emit-llvm --cuda-device-only -gline-tables-only kmanip_dyn.hip -o new.ll      (the flags of csrc/Makefile; old.ll
                                                                                                   the same from the other tree)
  tools/ir_fma_order.py <kernel-symbol-substring> old.ll new.ll

prints, per inlined-at chain (innermost three functions), the sums of two products whose count in source order / swapped order differs
between the two files.  No line of output: every such sum kept its pairing.  Expressions written with __builtin_fma (the *_pinned
helpers of kmanip_dyn_tree.hpp) are no fadd of products any more and drop out of both columns."""
import collections
import re
import sys


def load(path, fn):
    """(instruction lines of the first function whose `define` line contains fn, {metadata id: (kind, text)})"""
    md, body, inside, done = {}, [], False, False
    with open(path) as f:
        for ln in f:
            if not done and ln.startswith("define") and fn in ln:
                inside = True
                continue
            if inside:
                if ln.startswith("}"):
                    inside, done = False, True
                    continue
                body.append(ln)
            elif ln.startswith("!"):
                m = re.match(r"!(\d+) = (?:distinct )?!(\w+)\((.*)\)", ln)
                if m:
                    md[m.group(1)] = (m.group(2), m.group(3))
    return body, md


def scope_name(md, sid):
    for _ in range(20):
        if sid not in md:
            break
        kind, txt = md[sid]
        if kind == "DISubprogram":
            m = re.search(r'name: "([^"]+)"', txt)
            return m.group(1) if m else "?"
        m = re.search(r"scope: !(\d+)", txt)
        if not m:
            break
        sid = m.group(1)
    return "?"


def chain(md, did, depth=3):
    """function names of a !dbg location, innermost first, following inlinedAt"""
    out = []
    while did and did in md and len(out) < depth:
        kind, txt = md[did]
        if kind != "DILocation":
            break
        sc = re.search(r"scope: !(\d+)", txt)
        ia = re.search(r"inlinedAt: !(\d+)", txt)
        out.append(scope_name(md, sc.group(1)) if sc else "?")
        did = ia.group(1) if ia else None
    return tuple(out)


def line_col(md, did):
    if not did or did not in md or md[did][0] != "DILocation":
        return None
    txt = md[did][1]
    line = re.search(r"line: (\d+)", txt)
    col = re.search(r"column: (\d+)", txt)
    return (int(line.group(1)) if line else 0, int(col.group(1)) if col else 0)


SUM = re.compile(r"\s+(%[\w.]+) = (fadd|fsub) ([\w ]*?)double (%[\w.]+|[-\w.+]+), (%[\w.]+|[-\w.+]+)(?:, !dbg !(\d+))?")


def product_sums(path, fn):
    body, md = load(path, fn)
    defs = {}
    for ln in body:
        m = re.match(r"\s+(%[\w.]+) = (\w+)", ln)
        if m:
            defs[m.group(1)] = (m.group(2), ln)
    out = collections.Counter()
    for ln in body:
        m = SUM.match(ln)
        if not m:
            continue
        a, b = m.group(4), m.group(5)
        if a in defs and b in defs and defs[a][0] == "fmul" and defs[b][0] == "fmul":
            da, db = (re.search(r"!dbg !(\d+)", defs[v][1]) for v in (a, b))
            la, lb = (line_col(md, d.group(1)) if d else None for d in (da, db))
            order = "unknown" if (la is None or lb is None or la == lb) else ("source" if la < lb else "swapped")
            out[(m.group(2), order, chain(md, m.group(6)))] += 1
    return out


def main():
    fn, old, new = sys.argv[1:4]
    a, b = product_sums(old, fn), product_sums(new, fn)
    if not a or not b:
        sys.exit("no sums of two products found: is %r part of a `define` line of both files, built with -gline-tables-only?" % fn)
    tot = collections.Counter()
    for tag, c in (("old", a), ("new", b)):
        for k, v in c.items():
            tot[(tag, k[1])] += v
    print("sums of two products:  " + "  ".join("%s %s %d" % (t, o, tot[(t, o)]) for t in ("old", "new") for o in ("source", "swapped", "unknown")))
    n = 0
    for k in sorted(set(a) | set(b), key=str):
        if a[k] != b[k]:
            print("%-5s %-8s old %4d new %4d   %s" % (k[0], k[1], a[k], b[k], " < ".join(k[2])))
            n += 1
    print("%d (operation, order, inlined-at chain) classes differ" % n)


if __name__ == "__main__":
    main()
