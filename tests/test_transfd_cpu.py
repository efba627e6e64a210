"""kmanip_transition_fd on the CPU: the binding against the header, the built library's sixteen k_transfd kernels, the guard that the
device tests launch every compiled transfd object, and ilqr.trajectory_fd's fused switch over a stand-in.

Nothing is measured here and no tolerance is set: the device tests take tests/test_rollout_cpu.py's BAR_FD as it stands."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import build_matrix as BM  # noqa: E402
import feedback_oracle as FO  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the binding
def test_transfd_binding_matches_the_header():
    """lib.KTransFdIn / KTransFdDev list the header's fields in the header's order with the header's types and the C compiler's
    offsets; the first six inputs are KRolloutIn's; the KM_WRT_* bits are the header's; the prototype is in the header, the symbol
    bound with the right argument types, listed among the exports and exported; the version string is still 0.40."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    for name, cls in (("KTransFdIn", klib.KTransFdIn), ("KTransFdDev", klib.KTransFdDev)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(\w+)\s*(\*?)\s*(\w+)\s*;", body)
        assert [f for _, _, f in fields] == [n for n, _ in cls._fields_], name
        assert [C.c_void_p if star else ctype[t] for t, star, _ in fields] == [t for _, t in cls._fields_], name
    assert klib.KTransFdIn._fields_[:6] == klib.KRolloutIn._fields_[:6]
    assert [n for n, _ in klib.KTransFdIn._fields_[6:]] == ["wrt", "eps", "warm_offset"]
    # six pointers, the mask, four bytes of padding, two doubles: the layout of the C struct on the LP64 target
    assert (klib.KTransFdIn.wrt.offset, klib.KTransFdIn.eps.offset, klib.KTransFdIn.warm_offset.offset, C.sizeof(klib.KTransFdIn)) == (48, 56, 64, 72)
    assert [n for n, _ in klib.KTransFdDev._fields_] == ["qpos", "qvel", "qacc_warm", "contact_mask", "status", "deriv_t", "status_cols", "contact_mask_fd"]
    assert C.sizeof(klib.KTransFdDev) == 64
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define KM_WRT_(\w+)\s+(\d+)", hdr)}
    assert bits == {"QPOS": 1, "QVEL": 2, "CTRL": 4, "FRC": 8}
    assert klib.KM_WRT == {"qpos": 1, "qvel": 2, "ctrl": 4, "qfrc_applied": 8} and list(klib.KM_WRT) == ["qpos", "qvel", "ctrl", "qfrc_applied"]
    assert "KMANIP_API int kmanip_transition_fd(KHandle h, const KTransFdIn* in, int n, int nsub, const KTransFdDev* out, void* stream);" in hdr
    assert "kmanip_transition_fd" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_transition_fd.argtypes == [C.c_void_p, C.POINTER(klib.KTransFdIn), C.c_int, C.c_int, C.POINTER(klib.KTransFdDev), C.c_void_p]
    assert set(env_hip.KManipEnvHip._TRANSFD_FIELDS) == {n for n, _ in klib.KTransFdDev._fields_}
    assert " 0.40 " in L.kmanip_version().decode()


def _transfd_table():
    """The k_transfd* kernels of the built library; args = (NL, G, SOLVER, lane groups per wave)."""
    from gym_kmanip_amd import lib as klib
    return BM.kernels(klib.LIB_PATH, r"k_transfd\w*")


def test_shipped_transfd_kernels_run_without_scratch():
    """The sixteen k_transfd variants of the built library (parsed from the .so: no GPU): one per (class, solver) in each of the four
    builds, 64 / G lane groups per wave, none spills, registers within the 512 of a single-wave workgroup and no more than the
    k_feedback sibling's; the LDS is the k_rollout sibling's plus the exchange array -- per lane group qpos, qvel and one more
    8 bytes for the status."""
    from test_feedback_cpu import _feedback_table
    from test_rollout_cpu import _rollout_table
    rows = _transfd_table()
    names = ("k_transfd", "k_transfd_ep", "k_transfd_frc", "k_transfd_ep_frc")
    assert sorted((r.base, r.args[0], r.args[2]) for r in rows) == sorted((nm, nl, s) for nm in names for nl in (10, 20) for s in (0, 1))
    lds = {(r.base.replace("k_rollout", "k_transfd"), r.args[0], r.args[2]): r.lds for r in _rollout_table()}
    vgpr = {(r.base.replace("k_feedback", "k_transfd"), r.args[0], r.args[2]): r.vgpr for r in _feedback_table()}
    for r in rows:
        nl, g, solver, epb = r.args
        key = (r.base, nl, solver)
        assert (g, epb) == ((16, 4) if nl == 10 else (32, 2)), r
        assert r.scratch == 0 and r.vgpr <= 512 and r.vgpr <= vgpr[key], r
        assert r.lds == lds[key] + epb * ((nl + 7) + (nl + 6) + 1) * 8, r


# ------------------------------------------------------------------------------------------ every compiled object runs a parity row
def covered(handle_rows):
    """The (NL, G, SOLVER, ep, frc) objects the device's comparison with derivatives.transition_fd launches (kmanip_dispatch.hip: the
    10-link class for nlink <= 10, the parameter build while the handle has per-env parameters, the force build while the call
    gives a force, one is bound or a force is differentiated)."""
    from test_rollout_cpu import SOLVER_OF
    out = set()
    for asset, solver, mode in handle_rows:
        cls = (10, 16) if R.model(asset).nlink <= 10 else (20, 32)
        out.add(cls + (SOLVER_OF[solver], "params" in mode, "forced" in mode or "bound" in mode))
    return out


def missing_rows(makefile_path, handle_rows):
    have = covered(handle_rows)
    return [tuple(o[1:]) for o in BM.objects(makefile_path, "transfd") if tuple(o[1:]) not in have]


def test_every_compiled_transfd_object_has_a_row():
    from test_transfd_gpu import HANDLE_ROWS
    objs = BM.objects(BM.MAKEFILE, "transfd")
    assert sorted({o[1:4] for o in objs}) == sorted([(10, 16, 1), (10, 16, 0), (20, 32, 1), (20, 32, 0)])
    assert missing_rows(BM.MAKEFILE, HANDLE_ROWS) == []
    assert len(_transfd_table()) == len(objs)          # the objects the Makefile links are the ones the library holds


def test_the_guard_fails_for_a_transfd_variant_without_a_row(tmp_path):
    from test_transfd_gpu import HANDLE_ROWS
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    assert sorted(missing_rows(more, HANDLE_ROWS)) == [(30, 64, s, ep, frc) for s in (0, 1) for ep in (False, True) for frc in (False, True)]
    rows = [r for r in HANDLE_ROWS if not (r[1] == "pgs" and ("forced" in r[2] or "bound" in r[2]))]
    miss = missing_rows(BM.MAKEFILE, rows)
    assert (10, 16, 0, False, True) in miss and (20, 32, 0, True, True) in miss


# --------------------------------------------------------------------------------------------------------- the switch in ilqr.py
class _Fused:
    """OracleFeedback with the method KManipEnvHip has: .transition_fd is derivatives.transition_fd on the same stand-in."""

    def __init__(self, env):
        self.env, self.cm, self.fused_calls = env, env.cm, 0
        self.rollout, self.rollout_feedback = env.rollout, env.rollout_feedback

    def transition_fd(self, **kw):
        from gym_kmanip_amd.derivatives import transition_fd
        self.fused_calls += 1
        return transition_fd(self.env, **kw)


def test_trajectory_fd_fused_calls_the_envs_method_and_gives_the_same_result():
    """trajectory_fd(fused=True) hands env.transition_fd the rows fused=False hands derivatives.transition_fd: over a stand-in whose
    method IS derivatives.transition_fd the two results are equal bit for bit, and the method was called once; fused=False never
    calls it.  ilqr(fused=True) reaches it once per iteration."""
    import torch
    from gym_kmanip_amd import ilqr
    run = RO.cell_runs("solo_arm")
    cm, rows = run["cm"], run["rows"]
    e, T = 20, 2
    q0, v0, w0, c0 = (torch.from_numpy(rows[k][e:e + 1].copy()) for k in ("qpos", "qvel", "warm", "ctrl"))
    ctrl = c0[:, None].repeat(1, T, 1)
    env = _Fused(FO.OracleFeedback(cm, 2))
    plain = ilqr.trajectory_fd(env, [0], q0, v0, w0, ctrl, nsub=1)
    assert env.fused_calls == 0
    fused = ilqr.trajectory_fd(env, [0], q0, v0, w0, ctrl, nsub=1, fused=True)
    assert env.fused_calls == 1
    assert set(plain) == set(fused) and all(torch.equal(plain[k], fused[k]) for k in plain)
    assert tuple(fused["A"].shape) == (1, T, 2 * cm.nv, 2 * cm.nv) and tuple(fused["B"].shape) == (1, T, 2 * cm.nv, cm.nu)
    goal = q0.clone()
    goal[:, :cm.nlink] += 0.1
    wq = torch.zeros(2 * cm.nv, dtype=torch.float64)
    wq[:cm.nlink] = 10.0
    cost = ilqr.QuadraticCost(cm, goal, torch.zeros((1, cm.nv), dtype=torch.float64), wq, torch.full((cm.nu,), 1e-3, dtype=torch.float64), 10.0 * wq)
    res = ilqr.ilqr(env, [0], q0, v0, w0, ctrl, cost, iters=1, alphas=(1.0,), nsub=1, fused=True)
    assert env.fused_calls == 2 and np.isfinite(res["cost"].numpy()).all()
