"""kmanip_feedback_box on the device (run with -m gpu on an MI355X): rollout_feedback(ctrl_lo=, ctrl_hi=), the closed-loop rollout with
the policy's output clamped to a box.

Four regime cells of tests/tools/regime_states.py as caller rows on handles of 2 envs, 3 steps, the fixed gains of
tests/tools/feedback_oracle.py, every build of the kernel (PARITY_ROWS; tests/test_lqr_box_cpu.py checks that they launch every
kmanip_boxfb_* object).  kmanip_feedback itself is the yardstick: with infinite bounds, and wherever the policy stays inside the box,
the bytes are its own; where the box binds, the recorded ctrl is the clip of the policy torch evaluates on the recorded states, to
tests/test_feedback_cpu.py's BAR_U."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import feedback_oracle as FO  # noqa: E402
import rollout_oracle as RO  # noqa: E402
from test_rollout_gpu import _dev_rows, _fresh, _same, _t, _torch  # noqa: E402

pytestmark = pytest.mark.gpu

NSTEP, NROWS = FO.NSTEP, 4
# (asset, solver, mode, nsub): the plain build at the model's 10 sub-steps, the forced / per-env-parameter builds at one (the runs
# tests/tools/feedback_oracle.py keeps for them)
PARITY_ROWS = [(a, s, m, None if m == "plain" else 1) for a in ("solo_arm", "dual_arm") for s in ("newton", "pgs")
               for m in ("plain", "forced", "params", "params+forced")]
HALF = 0.3                       # the binding box: [-HALF, HALF] cut to the model's ctrlrange


def _setup(asset, solver, mode, nsub):
    """(cm, the handle, rollout_feedback's keyword arguments for NROWS cells spread over the regime cells)."""
    run = FO.cell_runs(asset, solver, mode, nsub)
    cm = run["cm"]
    pick = np.linspace(0, len(run["labels"]) - 1, NROWS).astype(int)
    dev = _fresh(cm, 2)
    if "params" in mode:
        dev.set_env_params(**RO.env_params(cm)[0])
    kw = _dev_rows({k: np.ascontiguousarray(v[pick]) for k, v in run["rows"].items()})
    kw.update({k: _t(np.ascontiguousarray(v[pick])) for k, v in run["policy"].items()}, nsub=nsub, nstep=NSTEP)
    return cm, dev, kw


def _box(cm):
    from gym_kmanip_amd.model import ctrl_range
    lo, hi = ctrl_range(cm, "cuda")
    return lo.clamp(min=-HALF), hi.clamp(max=HALF)


@pytest.mark.parametrize("asset,solver,mode,nsub", PARITY_ROWS)
def test_the_clamped_rollout_against_kmanip_feedback(asset, solver, mode, nsub):
    """(a) infinite bounds, given as tensors or one side None, and a box no policy output reaches: every output byte is
    rollout_feedback's; (b) a box inside ctrlrange that binds: every recorded ctrl lies in it, equals the clip of ctrl + K dx evaluated
    by torch on the recorded states to BAR_U, and a row's records are the unboxed launch's bytes up to the first step whose policy
    leaves the box; (c) the handle is only read."""
    torch = _torch()
    from gym_kmanip_amd.derivatives import tangent_diff
    from test_feedback_cpu import BAR_U
    cm, dev, kw = _setup(asset, solver, mode, nsub)
    before = dev.state_tensors()
    plain = dev.rollout_feedback(**kw)
    assert not plain["status"].any()
    inf = torch.full((cm.nu,), float("inf"), dtype=torch.float64, device="cuda")
    for box in (dict(ctrl_lo=-inf, ctrl_hi=inf), dict(ctrl_lo=-inf), dict(ctrl_hi=inf.repeat(NROWS, 1)), dict(ctrl_lo=torch.full_like(inf, -100.0), ctrl_hi=torch.full_like(inf, 100.0))):
        assert _same(plain, dev.rollout_feedback(**kw, **box)) == [], sorted(box)
    lo, hi = _box(cm)
    got = dev.rollout_feedback(**kw, ctrl_lo=lo, ctrl_hi=hi)
    assert not got["status"].any() and bool((got["steps_done"] == NSTEP).all())
    u = got["ctrl"]
    on = (u == lo) | (u == hi)
    assert bool(((u >= lo) & (u <= hi)).all()) and bool(on.any()) and not bool(on.all())
    # the unclamped policy on the recorded states: the state before step t is the row, then record t - 1
    q = torch.cat([kw["qpos"][:, None], got["qpos"][:, :-1]], dim=1)
    v = torch.cat([kw["qvel"][:, None], got["qvel"][:, :-1]], dim=1)
    dq = tangent_diff(cm, q.reshape(NROWS * NSTEP, -1), kw["qpos_ref"].reshape(NROWS * NSTEP, -1)).reshape(NROWS, NSTEP, -1)
    dx = torch.cat([dq, v - kw["qvel_ref"]], dim=2)
    open_loop = kw["ctrl"][:, None] if kw["ctrl"].dim() == 2 else kw["ctrl"]
    want = (open_loop + (kw["gains"] @ dx[..., None])[..., 0]).clamp(min=lo, max=hi)
    gap = float((u - want).abs().max())
    print("\n%s %s %s: %.0f %% of the recorded ctrl on a bound; worst |device - clip(torch's policy)| %.2e (bar %.0e)"
          % (asset, solver, mode, 100.0 * float(on.double().mean()), gap, BAR_U))
    assert gap <= BAR_U
    # up to the first step whose unclamped policy leaves the box a row is the unboxed launch's, bit for bit: under the binding box, and
    # under the box spanned by the rows' own step-0 outputs, which no row leaves before step 1 (a u ON a bound is left alone)
    late = dev.rollout_feedback(**kw, ctrl_lo=plain["ctrl"][:, 0].amin(dim=0), ctrl_hi=plain["ctrl"][:, 0].amax(dim=0))
    for tag, res, blo, bhi in (("the binding box", got, lo, hi), ("the step-0 span", late, plain["ctrl"][:, 0].amin(dim=0), plain["ctrl"][:, 0].amax(dim=0))):
        out = ((plain["ctrl"] < blo) | (plain["ctrl"] > bhi)).any(dim=2)
        first = torch.where(out.any(dim=1), out.int().argmax(dim=1), torch.full((NROWS,), NSTEP, device="cuda"))
        for r in range(NROWS):
            t = int(first[r])
            for name in ("qpos", "qvel", "qacc_warm", "contact_mask", "reward", "ctrl"):
                assert torch.equal(res[name][r, :t], plain[name][r, :t]), (tag, r, name)
            if t < NSTEP:
                assert not torch.equal(res["ctrl"][r, t], plain["ctrl"][r, t]), (tag, r)
        print("  %s: steps kept bit for bit before a row's first clamp %s of %d each" % (tag, first.tolist(), NSTEP))
        assert tag == "the binding box" or int(first.min()) >= 1
    after = dev.state_tensors()
    assert all(torch.equal(before[k], after[k]) for k in before)
    dev.k_close()


@pytest.mark.parametrize("solver", ["newton", "pgs"])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_an_empty_or_nan_box_stops_the_row_before_its_first_step(asset, solver):
    """A box per gain trajectory: trajectory 1 has lo > hi at one actuator, trajectory 2 a NaN bound -- status 1, steps_done 0 and
    zero records for the rows that follow them; rows 0 and 3 are the launch with the sound box, bit for bit.  One shared box with lo >
    hi stops every row.  A missing gain is refused as in rollout_feedback."""
    torch = _torch()
    from gym_kmanip_amd import lib as klib
    cm, dev, kw = _setup(asset, solver, "plain", None)
    lo, hi = _box(cm)
    good = dev.rollout_feedback(**kw, ctrl_lo=lo, ctrl_hi=hi)
    blo, bhi = lo.repeat(NROWS, 1), hi.repeat(NROWS, 1)
    blo[1, cm.nu - 1] = bhi[1, cm.nu - 1] + 0.5
    bhi[2, 0] = float("nan")
    got = dev.rollout_feedback(**kw, ctrl_lo=blo, ctrl_hi=bhi)
    assert got["status"].tolist() == [0, 1, 1, 0] and got["steps_done"].tolist() == [NSTEP, 0, 0, NSTEP]
    for name in ("qpos", "qvel", "qacc_warm", "contact_mask", "reward", "ctrl"):
        assert not got[name][1:3].any(), name
    keep = torch.tensor([0, 3], device="cuda")
    assert _same(got, good, rows_f=keep, rows_g=keep) == []
    allbad = dev.rollout_feedback(**kw, ctrl_lo=hi + 1.0, ctrl_hi=hi)
    assert bool((allbad["status"] == 1).all()) and not allbad["steps_done"].any() and not allbad["ctrl"].any()
    with pytest.raises(klib.KManipError):
        dev.rollout_feedback(**dict(kw, gains=None), ctrl_lo=lo, ctrl_hi=hi)
    dev.k_close()
