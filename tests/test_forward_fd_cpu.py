"""kmanip_forward_fd on the CPU: the binding against the header, the built library's eight k_fwdfd kernels, and derivatives.forward_fd's
`of` and `fused` switches over the oracle stand-in.  No tolerance is set here."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import build_matrix as BM  # noqa: E402
import forward_oracle as FW  # noqa: E402
import regime_states as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_fd_binding_matches_the_header():
    """Fields, order, types and bits are the header's; the prototype is declared, bound, listed and exported; the version is still 0.40."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    for name, cls in (("KForwardFdIn", klib.KForwardFdIn), ("KForwardFdDev", klib.KForwardFdDev)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = re.findall(r"(\w+)\s*(\*?)\s*(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert [(f, C.c_void_p if star else ctype[t]) for t, star, f in fields] == cls._fields_, name
    fi = klib.KForwardFdIn
    assert fi._fields_[:6] == klib.KForwardIn._fields_ and (fi.wrt.offset, fi.of.offset, fi.eps.offset, fi.warm_offset.offset, C.sizeof(fi)) == (48, 52, 56, 64, 72)      # LP64
    bits = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define KM_OF_(\w+)\s+(\d+)", hdr)}
    assert bits == klib.KM_OF and list(klib.KM_OF) == ["qacc", "qfrc_constraint", "qfrc_actuator", "contact_force"]
    assert "KMANIP_API int kmanip_forward_fd(KHandle h, const KForwardFdIn* in, int n, const KForwardFdDev* out, void* stream);" in hdr
    assert "kmanip_forward_fd" in klib.EXPORTS and "kmanip_*" in open(os.path.join(ROOT, "gym_kmanip_amd", "csrc", "exports.map")).read()
    L = klib.load()
    assert L.kmanip_forward_fd.argtypes == [C.c_void_p, C.POINTER(fi), C.c_int, C.POINTER(klib.KForwardFdDev), C.c_void_p]
    assert set(env_hip.KManipEnvHip._FWDFD_FIELDS) == {n for n, _ in klib.KForwardFdDev._fields_}
    assert " 0.40 " in L.kmanip_version().decode()


def test_shipped_forward_fd_kernels_run_without_scratch():
    """The eight k_fwdfd variants of the built library (parsed from the .so: no GPU): none spills, and the exchange in registers costs
    neither LDS nor registers -- the k_forward sibling's LDS to the byte, no more registers than it."""
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, r"k_fwdfd\w*")
    names = ("k_fwdfd", "k_fwdfd_ep", "k_fwdfd_frc", "k_fwdfd_ep_frc")
    assert sorted((r.base, r.args[0]) for r in rows) == sorted((nm, nl) for nm in names for nl in (10, 20))
    assert len(BM.objects(BM.MAKEFILE, "fwdfd")) == 8
    sib = {(r.base.replace("k_forward", "k_fwdfd"), r.args[0]): r for r in BM.kernels(klib.LIB_PATH, r"k_forward\w*")}
    for r in rows:
        s = sib[(r.base, r.args[0])]
        assert r.args[1:] == ((16, 4) if r.args[0] == 10 else (32, 2)), r
        assert r.scratch == 0 and r.vgpr <= s.vgpr <= 512 and r.lds == s.lds, (r, s)


def test_forward_fd_of_and_fused_over_the_oracle():
    """Two SoloArm cells, a grasp and a free cube, differentiated in ctrl.  The default `of` returns the keys forward_fd had before
    `of` existed, and every block is the quotient of the perturbed rows its second launch was handed, as it always formed it.  All
    four leave those bytes alone and add the new blocks: a grasping finger's normal force answers ctrl, a free cube has no sphere
    contact to differentiate.  fused=True hands the caller's arguments to env.forward_fd and returns its result."""
    import torch
    from gym_kmanip_amd.derivatives import OF, forward_fd
    from gym_kmanip_amd.model import contact_slots
    cm = R.model("solo_arm")
    qpos, qvel, ctrl, labels = R.cells("solo_arm")
    pick = [labels.index("G1"), labels.index("C1")]
    rows = {k: torch.from_numpy(x[pick].copy()) for k, x in (("qpos", qpos), ("qvel", qvel), ("ctrl", ctrl))}
    env = FW.OracleForward(cm, 2)
    d = forward_fd(env, wrt=("ctrl",), **rows)
    assert sorted(d) == ["contact_mask_fd", "dqacc_dctrl", "dqfrc_constraint_dctrl", "qacc", "qfrc_constraint", "status", "status_fd"]
    pert = env.forward(**{k: None if v is None else torch.from_numpy(v) for k, v in env.calls[1].items()})
    for key in ("qacc", "qfrc_constraint"):
        v = pert[key].reshape(cm.nu, 2, 2, cm.nv)
        assert torch.equal(d["d%s_dctrl" % key], ((v[:, 0] - v[:, 1]) / (2.0 * 1e-6)).permute(1, 2, 0).contiguous()), key
    full = forward_fd(env, wrt=("ctrl",), of=OF, **rows)
    assert all(torch.equal(d[k], full[k]) for k in d)
    assert tuple(full["dqfrc_actuator_dctrl"].shape) == (2, cm.nu, cm.nu) and tuple(full["dcontact_force_dctrl"].shape) == (2, contact_slots(cm.nlink), 4, cm.nu)
    assert float(full["dcontact_force_dctrl"][0, 4:, 0].abs().max()) > 1.0 and not full["dcontact_force_dctrl"][1, 4:].any()
    assert float(full["dqfrc_actuator_dctrl"][0].diagonal().abs().max()) > 1.0
    seen = {}
    env.forward_fd = lambda **kw: seen.update(kw) or "the method's result"
    assert forward_fd(env, wrt=("ctrl",), of=("contact_force",), fused=True, eps=1e-5, **rows) == "the method's result"
    assert seen["wrt"] == ("ctrl",) and seen["of"] == ("contact_force",) and seen["eps"] == 1e-5 and seen["qpos"] is rows["qpos"]
