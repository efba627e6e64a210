"""What the library is built from and what it holds, for the CPU guards and the kernel resource tests.

objects(makefile)        the per-variant objects `make print-objs` lists: what make builds, not a reading of the Makefile's text
kernels(lib, base)       the kernels of the built library by base name, with their template arguments and resource figures"""
import collections
import functools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MAKEFILE = os.path.join(ROOT, "gym_kmanip_amd", "csrc", "Makefile")

# solver is None for the units without one (their kernels are the Newton class's); ep / frc: the per-env parameter / applied-force build
Obj = collections.namedtuple("Obj", "unit NL G solver ep frc")
# base: the kernel's name without mangling or arguments; args: its leading integer and bool template arguments, in order
Kernel = collections.namedtuple("Kernel", "base args vgpr agpr sgpr scratch lds")


def objects(makefile_path=MAKEFILE, unit=None):
    """The per-variant objects of `make -f makefile_path print-objs` (every object whose name carries a number), all of them or one
    unit's, in link order.  The single-build objects (kmanip_api.o, ...) carry none and are left out; a numbered name that does not
    read as kmanip_<unit>[_ep][_frc]_<NL>_<G>[_<solver>].o is an error."""
    out = subprocess.run(["make", "--no-print-directory", "-f", os.path.abspath(makefile_path), "print-objs"], capture_output=True, text=True,
                         check=True).stdout
    objs = []
    for name in out.split():
        if not re.search(r"\d", name):
            continue
        m = re.fullmatch(r"kmanip_([a-z]+)(_ep)?(_frc)?_(\d+)_(\d+)(?:_(\d))?\.o", name)
        if not m:
            raise ValueError("cannot read the per-variant object name %r" % name)
        u, ep, frc, nl, g, s = m.groups()
        objs.append(Obj(u, int(nl), int(g), None if s is None else int(s), bool(ep), bool(frc)))
    assert len(set(objs)) == len(objs), "an object is listed twice"
    return [o for o in objs if unit is None or o.unit == unit]


def copy_with_class(dst_path, cls, makefile_path=MAKEFILE):
    """A copy of the Makefile at dst_path whose class list has one class more ("30_64"): every unit then has objects of that class."""
    lines = open(makefile_path).read().split("\n")
    at = [i for i, ln in enumerate(lines) if ln.startswith("CLASSES :=")]
    assert len(at) == 1, "the Makefile has one CLASSES line"
    lines[at[0]] += " " + cls
    with open(dst_path, "w") as f:
        f.write("\n".join(lines))
    return str(dst_path)


def _decode(mangled):
    """(base name, leading integer and bool template arguments) of a kernel's symbol:
    _Z[N<len><namespace>...]<len><base>[I(Li<int>E | Lb<0|1>E)...<other arguments>E]...; a symbol that is not mangled (extern "C") is
    its own base name."""
    if not mangled.startswith("_Z"):
        return mangled, ()
    nested = mangled.startswith("_ZN")
    base, rest = None, mangled[3 if nested else 2:]
    while base is None or nested:                     # (a nested name ends at its template arguments or its closing E, never at a digit)
        m = re.match(r"\d+", rest)
        if not m:
            break
        n = int(m.group())
        base, rest = rest[m.end():m.end() + n], rest[m.end() + n:]
    if base is None:
        raise ValueError("cannot read the name of %r" % mangled)
    t = re.match(r"I((?:L[ib]n?\d+E)*)", rest)
    args = re.findall(r"L([ib])(n?\d+)E", t.group(1)) if t else []
    return base, tuple(bool(int(v)) if k == "b" else int(v.replace("n", "-")) for k, v in args)


@functools.lru_cache(maxsize=None)
def _table(lib_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    return tuple(Kernel(*_decode(k.name), *(int(x) for x in k[1:])) for k in kr.kernels(lib_path))


def kernels(lib_path, base=".*"):
    """The kernels of the built library whose base name matches the pattern `base` in full (k_step does not match k_step_frc).  The
    library is read once per process and path."""
    return [k for k in _table(os.path.abspath(lib_path)) if re.fullmatch(base, k.base)]
