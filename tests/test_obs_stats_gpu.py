"""kmanip_obs_stats on the device (run with -m gpu on an MI355X): normalize.ObsStats.update against its longdouble two-pass reference at
test_normalize_cpu's BAR, on that file's cases: the row counts that leave a ragged pass, a ragged unroll and a ragged last block at
dims 1, 27, 49 and 64, and three successive folds against the two-pass over their concatenation.  What the device showed: DESIGN.md
section 51."""
import ctypes as C

import numpy as np
import pytest

from test_actor_gpu import _make, _torch
from test_normalize_cpu import DIMS, EPS, close, obs_rows, row_cases

pytestmark = pytest.mark.gpu
_ENV = []


def _env():
    if not _ENV:
        _ENV.append(_make("KManipSoloArm"))
    return _ENV[0]


@pytest.mark.parametrize("dim,sizes", [(d, s) for d in DIMS for s in row_cases(d)], ids=str)
def test_the_folded_moments_match_the_two_pass_reference(dim, sizes):
    from gym_kmanip_amd.normalize import ObsStats
    torch, env = _torch(), _env()
    a, b, seen = ObsStats(env, dim, EPS), ObsStats(env, dim, EPS), []
    for k, n in enumerate(sizes):
        seen.append(obs_rows(dim, n, k))
        x = torch.from_numpy(seen[-1]).to(env.device)
        a.update(x)
        b.update(x.view(1, n, dim))                                                # every leading row, whatever the leading shape
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("state", "mean", "inv_std"))      # equal states, the same call: the same bytes
    state, mean, inv_std = (getattr(a, k).cpu().numpy() for k in ("state", "mean", "inv_std"))
    assert state[0] == sum(sizes) and np.array_equal(state[1:1 + dim], mean)
    for name, got, want in zip(("mean", "M2 / n", "inv_std"), (mean, state[1 + dim:] / state[0], inv_std), a.reference(np.concatenate(seen))):
        ok, err = close(got, want)
        print("\ndim %d rows %s %s: worst relative error %.2e" % (dim, sizes, name, err))
        assert ok, (name, err)
    assert dim < 3 or inv_std[-1] == 1.0 / np.sqrt(EPS)                            # the constant column


def test_no_rows_leave_the_state_and_still_write_the_vectors():
    from gym_kmanip_amd.normalize import ObsStats
    torch, env = _torch(), _env()
    s = ObsStats(env, 27, EPS)
    s.mean.fill_(5.0), s.inv_std.fill_(5.0)
    s.update(torch.empty((0, 27), dtype=torch.float64, device=env.device))
    assert not s.state.any() and not s.mean.any() and bool((s.inv_std == 1.0).all())      # an empty state: no normalisation
    s.update(torch.from_numpy(obs_rows(27, 10)).to(env.device))
    keep = [t.clone() for t in (s.state, s.mean, s.inv_std)]
    s.mean.fill_(5.0), s.inv_std.fill_(5.0)
    s.update(torch.empty((0, 27), dtype=torch.float64, device=env.device))
    assert all(torch.equal(k, t) for k, t in zip(keep, (s.state, s.mean, s.inv_std)))


@pytest.mark.parametrize("bad", ["handle", "in", "obs", "state", "workspace", "dim 0", "dim 65", "rows", "eps 0", "eps nan", "odd obs", "odd state",
                                 "odd workspace", "odd mean", "odd inv_std"])
def test_obs_stats_refuses(bad):
    from gym_kmanip_amd import lib as klib
    torch, env = _torch(), _env()
    t = {k: torch.zeros((64,), dtype=torch.float64, device=env.device) for k in ("obs", "state", "workspace", "mean", "inv_std")}
    ptr = {k: None if k == bad else v.data_ptr() + (4 if bad == "odd " + k else 0) for k, v in t.items()}
    oi = klib.KObsStatsIn(obs=ptr["obs"], n_rows=-1 if bad == "rows" else 2, dim={"dim 0": 0, "dim 65": 65}.get(bad, 27),
                          eps={"eps 0": 0.0, "eps nan": float("nan")}.get(bad, EPS))
    h = None if bad == "handle" else env.h
    rc = env.L.kmanip_obs_stats(h, None if bad == "in" else C.byref(oi), C.c_void_p(ptr["state"]), C.c_void_p(ptr["workspace"]), C.c_void_p(ptr["mean"]),
                                C.c_void_p(ptr["inv_std"]), env._stream())
    assert rc != 0 and b"kmanip_obs_stats" in env.L.kmanip_last_error(h)
    torch.cuda.synchronize()
    assert not any(bool(v.any()) for v in t.values())
