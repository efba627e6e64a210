"""kmanip_feedback on the CPU: the binding, the built library's sixteen k_feedback kernels, the reference's own checks
(tests/tools/feedback_oracle.py OracleFeedback) and the guard that the device tests launch every compiled feedback object.

No tolerance of the device's state parity is invented here: the bars are test_gpu_parity's (qpos 1e-7, qvel 1e-5, reward 1e-6), and the
reference's own spread under qvel (1 + 1e-15) must stay ten times below them on every cell under the fixed gains.  The bar of the
recorded ctrl is 1000 x the reference's own spread of u, one digit up (DESIGN.md section 27's rule), derived and re-asserted here."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import build_matrix as BM  # noqa: E402
import feedback_oracle as FO  # noqa: E402
import mujoco_pin  # noqa: E402
import regime_states as R  # noqa: E402
import rollout_oracle as RO  # noqa: E402
from test_forward_cpu import QUALIFYING  # noqa: E402
from test_gpu_parity import TOL_Q, TOL_R, TOL_V  # noqa: E402

ASSETS = mujoco_pin.ASSETS
SOLVERS = ("newton", "pgs")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = {"qpos": TOL_Q, "qvel": TOL_V, "reward": TOL_R}
# the worst spread of the recorded u between the reference and its qvel (1 + 1e-15) twin over every cell of the three assets, both
# solvers, 3 steps of the model's sub-steps under the fixed gains (values of size <= 5), measured by the test below and committed; the
# device's bar is 1000 x that, one digit up
SPREAD_U = 4.708e-14
BAR_U = 5e-11


# ------------------------------------------------------------------------------------------------------------------ the binding
def test_feedback_binding_matches_the_header():
    """lib.KFeedbackIn / KFeedbackDev list the header's fields in the header's order, begin with KRolloutIn's / KRolloutDev's; the
    prototype is in the header, the symbol bound with the right argument types, listed among the exports and exported."""
    import ctypes as C
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    for name, cls in (("KFeedbackIn", klib.KFeedbackIn), ("KFeedbackDev", klib.KFeedbackDev)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(\*?)\s*(\w+)\s*;", body)
        assert [f for _, f in fields] == [n for n, _ in cls._fields_], name
        assert [C.c_void_p if star else C.c_int32 for star, _ in fields] == [t for _, t in cls._fields_], name
    assert klib.KFeedbackIn._fields_[:8] == klib.KRolloutIn._fields_ and klib.KFeedbackDev._fields_[:7] == klib.KRolloutDev._fields_
    assert [n for n, _ in klib.KFeedbackIn._fields_[8:]] == ["gain_index", "qpos_ref", "qvel_ref", "gain_t", "ng", "gain_per_step"]
    assert [n for n, _ in klib.KFeedbackDev._fields_[7:]] == ["ctrl"]
    assert ("KMANIP_API int kmanip_feedback(KHandle h, const KFeedbackIn* in, int n, int nstep, int nsub, const KFeedbackDev* out, void* stream);"
            in hdr)
    assert "kmanip_feedback" in klib.EXPORTS
    L = klib.load()
    assert L.kmanip_feedback.argtypes == [C.c_void_p, C.POINTER(klib.KFeedbackIn), C.c_int, C.c_int, C.c_int, C.POINTER(klib.KFeedbackDev), C.c_void_p]
    assert set(env_hip.KManipEnvHip._FEEDBACK_FIELDS) == {n for n, _ in klib.KFeedbackDev._fields_} == set(FO.FIELDS)
    assert " 0.40 " in L.kmanip_version().decode()


def _feedback_table():
    """The k_feedback* kernels of the built library; args = (NL, G, SOLVER, rows per wave)."""
    from gym_kmanip_amd import lib as klib
    return BM.kernels(klib.LIB_PATH, r"k_feedback\w*")


def test_shipped_feedback_kernels_run_without_scratch():
    """The sixteen k_feedback variants of the built library (parsed from the .so: no GPU): one per (class, solver) in each of the four
    builds, 64 / G rows per wave, none spills, registers within the 512 of a single-wave workgroup; the LDS is the k_rollout
    sibling's plus the dx array [rows per wave][2 nv] of doubles."""
    from test_rollout_cpu import _rollout_table
    rows = _feedback_table()
    names = ("k_feedback", "k_feedback_ep", "k_feedback_frc", "k_feedback_ep_frc")
    assert sorted((r.base, r.args[0], r.args[2]) for r in rows) == sorted((nm, nl, s) for nm in names for nl in (10, 20) for s in (0, 1))
    sibling = {(r.base.replace("k_rollout", "k_feedback"), r.args[0], r.args[2]): r.lds for r in _rollout_table()}
    for r in rows:
        nl, g, solver, epb = r.args
        assert (g, epb) == ((16, 4) if nl == 10 else (32, 2)), r
        assert r.scratch == 0 and r.vgpr <= 512, r
        assert r.lds == sibling[(r.base, nl, solver)] + epb * 2 * (nl + 6) * 8, r


# ---------------------------------------------------------------------------------------------------- the reference's own identities
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_zero_gains_and_a_reference_on_the_trajectory_are_the_open_loop_rollout(asset, solver):
    """Equalities of OracleFeedback against OracleRollout.rollout of the same rows (the shared open-loop run): (a) gains = 0 under
    the perturbed references; (b) the fixed gains, finite and non-zero, with the references on the row's own open-loop trajectory --
    x_0 the row itself, x_t record t - 1: the state BEFORE step t -- so that every dx is exactly zero.  ctrl out is ctrl in."""
    run = FO.cell_runs(asset, solver)
    cm, rows, pol, ol = run["cm"], run["rows"], run["policy"], run["open"]
    n = len(run["labels"])
    env = FO.OracleFeedback(cm, 2)
    zero = env.rollout_feedback(nstep=FO.NSTEP, **rows, **dict(pol, gains=np.zeros_like(pol["gains"])))
    qr = np.concatenate([rows["qpos"][:, None], ol["qpos"][:, :-1]], axis=1)
    vr = np.concatenate([rows["qvel"][:, None], ol["qvel"][:, :-1]], axis=1)
    assert np.abs(pol["gains"]).min() > 0 and np.isfinite(pol["gains"]).all()
    on = env.rollout_feedback(nstep=FO.NSTEP, **rows, gains=pol["gains"], qpos_ref=qr, qvel_ref=vr)
    for got in (zero, on):
        for k in RO.FIELDS:
            assert np.array_equal(got[k], ol[k]), k
        assert np.array_equal(got["ctrl"], np.repeat(rows["ctrl"][:, None], FO.NSTEP, axis=1))
    # the off-by-one reference (record t as the reference of step t) is NOT the open-loop run: the identity can tell
    off = env.rollout_feedback(nstep=FO.NSTEP, **{k: v[:4] for k, v in rows.items()}, gains=pol["gains"][:4], qpos_ref=ol["qpos"][:4], qvel_ref=ol["qvel"][:4])
    assert not np.array_equal(off["ctrl"], zero["ctrl"][:4])
    assert len(env.fb_calls) == 3 and env.fb_calls[0]["n"] == n and not env.calls


def test_oracle_feedback_status_rules_and_shared_trajectories():
    """The stand-in's own semantics, which the device tests rely on: held gains are the same gain every step, a shared trajectory
    is a private copy, gains_t is the transpose, a non-finite reference or gain entry at step t stops the row with steps_done = t
    and zeros from there on, an entry no row names changes nothing, a gain index outside 0 .. ng-1 gives status 2."""
    run = FO.cell_runs("solo_arm")
    cm, pol = run["cm"], run["policy"]
    rows = {k: v[:4] for k, v in run["rows"].items()}
    env = FO.OracleFeedback(cm, 2)
    p4 = {k: v[:4] for k, v in pol.items()}
    ref = env.rollout_feedback(nstep=3, nsub=1, **rows, **p4)
    assert not ref["status"].any() and np.abs(ref["ctrl"] - rows["ctrl"][:, None]).max() > 0.1
    t_ = env.rollout_feedback(nstep=3, nsub=1, **rows, gains_t=np.ascontiguousarray(np.swapaxes(p4["gains"], -1, -2)), qpos_ref=p4["qpos_ref"], qvel_ref=p4["qvel_ref"])
    assert all(np.array_equal(ref[k], t_[k]) for k in ref)
    held = env.rollout_feedback(nstep=3, nsub=1, **rows, **{k: v[:, 0] for k, v in p4.items()})
    rep = env.rollout_feedback(nstep=3, nsub=1, **rows, **{k: np.repeat(v[:, :1], 3, axis=1) for k, v in p4.items()})
    assert all(np.array_equal(held[k], rep[k]) for k in held) and not np.array_equal(held["ctrl"], ref["ctrl"])
    shared = env.rollout_feedback(nstep=3, nsub=1, gain_index=np.array([1, 1, 0, 3], np.int32), **rows, **p4)
    private = env.rollout_feedback(nstep=3, nsub=1, **rows, **{k: v[[1, 1, 0, 3]] for k, v in p4.items()})
    assert all(np.array_equal(shared[k], private[k]) for k in shared)
    for name, at, done in (("gains", (2, 1, 3, 5), 1), ("qpos_ref", (2, 0, cm.nq - 1), 0), ("qvel_ref", (2, 2, 0), 2)):
        bad = {k: v.copy() for k, v in p4.items()}
        bad[name][at] = np.nan
        g = env.rollout_feedback(nstep=3, nsub=1, **rows, **bad)
        assert g["status"].tolist() == [0, 0, 1, 0] and g["steps_done"].tolist() == [3, 3, done, 3]
        assert not g["ctrl"][2, done:].any() and not g["qpos"][2, done:].any() and np.array_equal(g["ctrl"][2, :done], ref["ctrl"][2, :done])
        same = env.rollout_feedback(nstep=3, nsub=1, gain_index=np.array([0, 1, 3, 3], np.int32), **rows, **bad)
        assert not same["status"].any()
    g = env.rollout_feedback(nstep=3, nsub=1, gain_index=np.array([0, 4, -1, 3], np.int32), **rows, **p4)
    assert g["status"].tolist() == [0, 2, 2, 0] and not g["ctrl"][1:3].any() and np.array_equal(g["ctrl"][3], ref["ctrl"][3])


# ------------------------------------------------------------------------------------------------------- the reference's own spread
def _cellwise(d, labels):
    out = {}
    for c, v in zip(labels, d):
        out[c] = max(out.get(c, 0.0), float(v))
    return out


def spreads(run, keys):
    rows = run["twin_rows"]
    labels = [run["labels"][e] for e in rows]
    return {k: _cellwise(np.abs(run["twin"][k] - run["ref"][k][rows]).reshape(len(rows), -1).max(axis=1), labels) for k in keys}


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("asset", ASSETS)
def test_the_references_own_spread_under_the_fixed_gains(asset, solver):
    """OracleFeedback at qvel and at qvel (1 + 1e-15) under the fixed gains (s = 1), every cell, 3 steps of the model's sub-steps: no
    row stops, the gains matter (|u - ctrl| above 1 somewhere), and the run FAILS if ten times any cell's spread exceeds its state
    bar or 1000 times its spread of u exceeds BAR_U (no cell is left out)."""
    run = FO.cell_runs(asset, solver)
    n = len(run["labels"])
    assert n == QUALIFYING[asset] and len(run["twin_rows"]) == n and run["cm"].desc.n_sub_steps == 10
    assert not run["ref"]["status"].any() and (run["ref"]["steps_done"] == FO.NSTEP).all() and not run["twin"]["status"].any()
    assert np.abs(run["ref"]["ctrl"] - run["rows"]["ctrl"][:, None]).max() > 1.0 and np.abs(run["ref"]["ctrl"]).max() <= 5.0
    sp = spreads(run, list(BARS) + ["ctrl"])
    print("\n%s %s: the reference's own spread per cell over 3 steps under the fixed gains" % (asset, solver))
    for c in dict.fromkeys(run["labels"]):
        print("  %-5s %s" % (c, "  ".join("%s %.1e" % (k, sp[k][c]) for k in sp)))
    print("  worst u spread %.3e" % max(sp["ctrl"].values()))
    broken = [(c, k, s) for k, bar in BARS.items() for c, s in sp[k].items() if not 10.0 * s <= bar]
    broken += [(c, "ctrl", s) for c, s in sp["ctrl"].items() if not (s <= SPREAD_U and 1000.0 * s <= BAR_U)]
    assert not broken, broken


def test_the_ctrl_bar_is_1000_times_the_committed_spread_one_digit_up():
    from test_forces_cpu import _round_up_one_digit
    assert BAR_U == pytest.approx(_round_up_one_digit(1000.0 * SPREAD_U), rel=1e-12)


# ------------------------------------------------------------------------------------------ every compiled object runs a parity row
def covered(parity_rows):
    """The (NL, G, SOLVER, ep, frc) objects the device's parity runs launch (kmanip_dispatch.hip: the 10-link class for nlink <= 10,
    the parameter build while the handle has per-env parameters, the force build while the call gives a force)."""
    from test_rollout_cpu import SOLVER_OF
    out = set()
    for asset, solver, mode, _ in parity_rows:
        cls = (10, 16) if R.model(asset).nlink <= 10 else (20, 32)
        out.add(cls + (SOLVER_OF[solver], "params" in mode, "forced" in mode))
    return out


def missing_rows(makefile_path, parity_rows):
    have = covered(parity_rows)
    return [tuple(o[1:]) for o in BM.objects(makefile_path, "feedback") if tuple(o[1:]) not in have]


def test_every_compiled_feedback_object_has_a_parity_row():
    from test_feedback_gpu import PARITY_ROWS
    objs = BM.objects(BM.MAKEFILE, "feedback")
    assert sorted({o[1:4] for o in objs}) == sorted([(10, 16, 1), (10, 16, 0), (20, 32, 1), (20, 32, 0)])
    assert missing_rows(BM.MAKEFILE, PARITY_ROWS) == []
    assert len(_feedback_table()) == len(objs)          # the objects the Makefile links are the ones the library holds


def test_the_guard_fails_for_a_feedback_variant_without_a_row(tmp_path):
    from test_feedback_gpu import PARITY_ROWS
    more = BM.copy_with_class(tmp_path / "Makefile", "30_64")
    assert sorted(missing_rows(more, PARITY_ROWS)) == [(30, 64, s, ep, frc) for s in (0, 1) for ep in (False, True) for frc in (False, True)]
    rows = [r for r in PARITY_ROWS if not (r[1] == "pgs" and "forced" in r[2])]
    miss = missing_rows(BM.MAKEFILE, rows)
    assert (10, 16, 0, False, True) in miss and (20, 32, 0, True, True) in miss


# ------------------------------------------------------------------------------------------------------- one source, two kernels
def test_the_feedback_objects_are_the_rollout_source_with_one_more_macro():
    """k_feedback is kmanip_rollout.hip compiled with -DKM_VAR_FB=1 and nothing else: make's dry run (nothing
    is compiled) gives the feedback object and its rollout sibling the same command line but for that flag and the object's name."""
    import subprocess
    csrc = os.path.dirname(BM.MAKEFILE)
    objs = {"feedback": "kmanip_feedback_ep_frc_20_32_0.o", "rollout": "kmanip_rollout_ep_frc_20_32_0.o"}
    lines = {}
    for kind, obj in objs.items():
        out = subprocess.run(["make", "-n", "-B", obj], cwd=csrc, check=True, capture_output=True, text=True).stdout
        cmds = [ln.split() for ln in out.splitlines() if " -c " in ln and "-o %s" % obj in ln]
        assert len(cmds) == 1, out
        lines[kind] = cmds[0]
    for kind, cmd in lines.items():
        assert cmd[cmd.index("-c") + 1] == "kmanip_rollout.hip", cmd
        assert cmd[cmd.index("-o") + 1] == objs[kind], cmd
        assert cmd.count("-DKM_VAR_FB=1") == (1 if kind == "feedback" else 0), cmd
        assert not [a for a in cmd if a.startswith("-DKM_VAR_FB") and a != "-DKM_VAR_FB=1"], cmd
    bare = {kind: [a for a in cmd if a not in ("-DKM_VAR_FB=1", objs[kind])] for kind, cmd in lines.items()}
    assert bare["feedback"] == bare["rollout"]
    assert not os.path.exists(os.path.join(csrc, "kmanip_feedback.hip"))
