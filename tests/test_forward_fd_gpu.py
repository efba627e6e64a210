"""kmanip_forward_fd on the device (run with -m gpu on an MI355X), handles of 2 envs.  The bars against the oracle: test_forward_cpu's
fd_bars and, for qfrc_actuator and contact_force, the same rule (test_forces_cpu's bar x force_oracle.scales' normaliser / eps; the
oracle's own spreads, 4.9e-16 and 1.27e-12, x 1000 stay within it).  Against the torch path the blocks lie within RECIPROCAL_ULPS:
torch on the device divides by a Python number as x * fl(1 / d), the kernel divides.  Derivations and figures: DESIGN.md section 44."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import applied_oracle as AO  # noqa: E402
import force_oracle as FO  # noqa: E402
import forward_oracle as FW  # noqa: E402
import regime_states as R  # noqa: E402
from test_forces_cpu import BAR_CONTACT_FORCE, BAR_QFRC_ACTUATOR  # noqa: E402
from test_forces_gpu import _cells  # noqa: E402
from test_forward_cpu import EPS, fd_bars  # noqa: E402
from test_forward_gpu import FD_CELLS, _fresh, _params, _t, _torch  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ("qpos", "qvel", "ctrl", "qfrc_applied")
OF = ("qacc", "qfrc_constraint", "qfrc_actuator", "contact_force")
BLOCK = dict(zip(ALL, ("dqpos", "dqvel", "dctrl", "dfrc")))
RECIPROCAL_ULPS = 2.0          # in units of 2^-52 |entry|


def _rows(asset, forced=False, n=None):
    """(cm, the first n FD_CELLS rows of the asset as forward_fd's keyword arguments, envs = arange % 2, their cells)."""
    cm, qpos, qvel, ctrl, _, labels = _cells(asset)
    pick = [labels.index(c) for c in FD_CELLS[asset]][:n]
    kw = dict(envs=_t(np.arange(len(pick)) % 2, np.int32), qpos=_t(qpos[pick]), qvel=_t(qvel[pick]), ctrl=_t(ctrl[pick]))
    if forced:
        kw.update(qfrc_applied=_t(AO.draw_test_forces(cm, len(labels))[pick]), wrt=ALL)
    return cm, kw, pick


@pytest.mark.parametrize("asset", sorted(FD_CELLS))
def test_fused_forward_fd_against_the_oracle(asset):
    torch = _torch()
    from gym_kmanip_amd.derivatives import forward_fd
    cm, kw, pick = _rows(asset)
    ref = forward_fd(FW.OracleForward(cm, 2), of=OF, eps=EPS, **{k: v.cpu() for k, v in kw.items()})
    dev = _fresh(cm, 2)
    got = dev.forward_fd(of=OF, eps=EPS, **kw)
    assert not got["status"].any() and not got["status_cols"].any() and not got["status_fd"].any() and not ref["status_fd"].any()
    assert torch.equal(got["contact_mask_fd"].cpu(), ref["contact_mask_fd"])
    bad, worst = [], {}
    for r, e in enumerate(pick):
        o = FO.cell_decodes(asset)[1][e]
        sq, sf, sa = FO.scales(o)
        bars = fd_bars(o) + (BAR_QFRC_ACTUATOR * sa / EPS, BAR_CONTACT_FORCE * sf / EPS)
        for key, s, bar in zip(OF, (sq, sf, sa, sf), bars):
            for blk in BLOCK.values():
                name = "d%s_%s" % (key, blk)
                d = float((got[name][r].cpu() - ref[name][r]).abs().max())
                worst[key] = max(worst.get(key, 0.0), d * EPS / s)
                if not d <= bar:
                    bad.append((FD_CELLS[asset][r], name, d, bar))
    print("\n%s: worst |fused - oracle| x eps / normaliser per output over all blocks: %s" % (asset, "  ".join("%s %.1e" % kv for kv in worst.items())))
    assert not bad and float(got["dcontact_force_dqpos"].abs().max()) > 1.0 and float(got["dqfrc_actuator_dctrl"].abs().max()) > 1.0, bad
    dev.k_close()


# one row per size class and build: together they launch all eight k_fwdfd objects
@pytest.mark.parametrize("mode", ["plain", "forced", "params", "params+forced"])
@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_fused_against_the_python_on_the_same_handle(asset, mode):
    torch = _torch()
    from gym_kmanip_amd.derivatives import forward_fd
    cm, kw, _ = _rows(asset, forced="forced" in mode)
    kw.setdefault("wrt", ALL[:3])
    dev = _fresh(cm, 2)
    if "params" in mode:
        dev.set_env_params(**_params(cm))
    ref, got = forward_fd(dev, of=OF, **kw), dev.forward_fd(of=OF, **kw)
    assert not ref["status"].any() and not ref["status_fd"].any() and float(ref["dqacc_dqpos"].abs().max()) > 1.0
    assert [k for k in OF + ("status", "status_fd", "contact_mask_fd") if not torch.equal(ref[k], got[k])] == []
    worst = {}
    for blk in ("d%s_%s" % (key, BLOCK[name]) for key in OF for name in kw["wrt"]):
        assert got[blk].shape == ref[blk].shape, blk
        worst[blk] = float(((got[blk] - ref[blk]).abs() / ref[blk].abs().clamp(min=1e-300)).max()) / 2.0 ** -52
    print("\n%s %s: worst |fused - python| in units of 2^-52 |entry|: %s" % (asset, mode, "  ".join("%s %.2f" % kv for kv in worst.items())))
    assert max(worst.values()) <= RECIPROCAL_ULPS, worst
    dev.k_close()


@pytest.mark.parametrize("asset", ["solo_arm", "dual_arm"])
def test_the_kernel_against_itself_bit_for_bit(asset):
    """Rows reversed, each row alone, every row naming env 1, every single-name `wrt` and every subset of `of` against the full call."""
    torch = _torch()
    cm, kw, _ = _rows(asset, forced=True, n=3)
    kw["warm"] = torch.zeros((3, cm.nv), dtype=torch.float64, device="cuda")
    dev = _fresh(cm, 2)
    full = dev.forward_fd(of=OF, **kw)
    assert not full["status_cols"].any() and full["deriv_t"].abs().max() > 1.0
    same = lambda g, f=full: all(torch.equal(g[k], f[k]) for k in ("deriv_t", "status_cols", "qacc", "contact_force"))
    take = lambda f: {k: (f(v) if hasattr(v, "shape") else v) for k, v in kw.items()}
    rev = {k: v.flip(2 if k == "contact_mask_fd" else 0) for k, v in dev.forward_fd(of=OF, **take(lambda v: v.flip(0).contiguous())).items()}
    assert same(rev) and torch.equal(rev["contact_mask_fd"], full["contact_mask_fd"])
    for r in range(3):
        assert same(dev.forward_fd(of=OF, **take(lambda v: v[r:r + 1])), {k: v[r:r + 1] for k, v in full.items()}), r
    assert same(dev.forward_fd(of=OF, **dict(kw, envs=[1, 1, 1])))
    c = 0
    for name, w in zip(ALL, (cm.nv, cm.nv, cm.nu, cm.nv)):
        sub = dev.forward_fd(of=OF, **dict(kw, wrt=(name,)))
        assert all(torch.equal(sub[k], full[k][:, c:c + w]) for k in ("deriv_t", "status_cols")), name
        assert torch.equal(sub["contact_mask_fd"], full["contact_mask_fd"][c:c + w]), name
        c += w
    edges = np.cumsum([0, cm.nv, cm.nv, cm.nu, 4 * full["contact_force"].shape[1]])
    run = {key: torch.arange(edges[i], edges[i + 1], device="cuda") for i, key in enumerate(OF)}
    for of in (s for k in range(1, 4) for s in itertools.combinations(OF, k)):
        sub = dev.forward_fd(of=of[::-1], **kw)
        assert torch.equal(sub["deriv_t"], full["deriv_t"][:, :, torch.cat([run[key] for key in of])]), of
    dev.k_close()


def test_bad_rows_get_their_status_and_zero_columns_and_harm_nobody():
    torch = _torch()
    cm, kw, _ = _rows("solo_arm")
    dev = _fresh(cm, 2)
    clean = dev.forward_fd(of=OF, **kw)
    n = clean["deriv_t"].shape[0]
    keep = torch.arange(n, device="cuda") != 2
    nan = dict(kw, ctrl=kw["ctrl"].clone())
    nan["ctrl"][2, 1] = float("nan")
    cases = [(1, nan)] + [(2, dict(kw, envs=torch.where(keep, kw["envs"], torch.full_like(kw["envs"], idx)))) for idx in (2, -1, 2 ** 31 - 1, -2 ** 31)]
    for status, bad in cases:
        g = dev.forward_fd(of=OF, **bad)
        assert (g["status_cols"][2] == status).all() and not g["status_cols"][keep].any() and g["status"].tolist() == [0, 0, status] + [0] * (n - 3)
        assert not g["deriv_t"][2].any() and not g["contact_mask_fd"][:, :, 2].any() and not g["qacc"][2].any()
        assert [k for k in ("deriv_t", "qacc", "contact_force") if not torch.equal(g[k][keep], clean[k][keep])] == []
        assert torch.equal(g["contact_mask_fd"][:, :, keep], clean["contact_mask_fd"][:, :, keep])
    assert dev.state_index_errors() == 0
    dev.k_close()


def test_refusals_leave_the_outputs_untouched_and_the_handle_as_it_was():
    torch = _torch()
    from gym_kmanip_amd import env_hip
    from gym_kmanip_amd.lib import KForwardFdDev, KForwardFdIn
    dev = _fresh(R.model("solo_arm"), 2)
    pgs = env_hip.KManipEnvHip(R.model("solo_arm", "pgs"), num_envs=2, seed=0)
    pgs.k_reset()
    cm, n, ncol = dev.cm, 2, 3 * dev.cm.nv + dev.cm.nu
    bufs = {"qacc": ((n, cm.nv), torch.float64), "deriv_t": ((n, ncol, 2 * cm.nv), torch.float64), "status_cols": ((n, ncol), torch.uint8)}
    bufs = {k: torch.full(s, 7, dtype=dt, device="cuda") for k, (s, dt) in bufs.items()}
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    untouched = lambda: torch.cuda.synchronize() or all(bool((t == 7).all()) for t in bufs.values())

    def call(h=dev, n=n, drop=(), **fields):
        fi, fd = KForwardFdIn(), KForwardFdDev()
        fi.wrt, fi.of, fi.eps, fi.warm_offset = 15, 3, 1e-6, 1.0
        for k, v in fields.items():
            setattr(fi, k, v)
        for k, t in bufs.items():
            setattr(fd, k, None if k in drop else t.data_ptr())
        return h.L.kmanip_forward_fd(h.h, C.byref(fi), n, C.byref(fd), None), h.L.kmanip_last_error(h.h)

    before, too_many = dev.state_tensors(), dict(n=2 ** 31 - 1, env_index=idx.data_ptr())
    for kw in ([dict(eps=v) for v in (0.0, -1e-6, float("nan"), float("inf"))] + [dict(warm_offset=v) for v in (float("nan"), float("-inf"))]
               + [dict(of=0), dict(of=16), dict(wrt=16), dict(drop=("deriv_t",)), dict(drop=("qacc",)), dict(n=-1), dict(n=3), dict(h=pgs), too_many]):
        rc, err = call(**kw)
        assert rc != 0 and err and untouched(), kw
    assert b"Newton" in call(h=pgs)[1] and b"int counts" in call(**too_many)[1]
    assert call(n=0, eps=0.0, of=0)[0] == 0 and call(h=pgs, n=0)[0] == 0 and untouched()
    assert call()[0] == 0 and not untouched()
    assert not bufs["status_cols"].any() and bufs["deriv_t"].abs().max() > 1.0 and torch.isfinite(bufs["deriv_t"]).all()
    assert all(torch.equal(v, dev.state_tensors()[k]) for k, v in before.items())
    dev.step_flat(torch.zeros((2, cm.act_dim), dtype=torch.float32, device="cuda"))
    assert not dev.done.cpu().numpy().any()
    dev.k_close(), pgs.k_close()
