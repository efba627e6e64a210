"""kmanip_actor_grad on the CPU: the bar the float32 arithmetic sets for the device test, the binding against
the header with the two size formulas, and the built library's kernels.  CASES, `inputs` and ROWS are the device test's as well."""
import ctypes as C
import os
import re

import numpy as np

from test_actor_cpu import ACTIVATIONS, BM, ROOT, mean_of, network

CASES = [(27, (16, 16), 7), (47, (64, 32), 14), (27, (80, 48), 1), (64, (256, 256), 16)]
HEADS = ["given", "mse", "ppo"]
NREC, CLIP = 33, 0.2
ROWS = [list(range(3)), list(range(17)), None, [(7 * r + 3) % NREC for r in range(300)]]      # 300 rows: two K-splits of 160
RHO = [0.7, 1.4, 0.95, 1.1]      # by row: below 1 - CLIP, above 1 + CLIP, inside twice; the advantage's sign changes every four rows
# The worst max|g32 - g64| / max|g64| over every gradient tensor of CASES x ACTIVATIONS x HEADS x ROWS: a NumPy float32 program of
# include/kmanip.h's formulas against the float64 one, on the same float32 weights and float32-rounded inputs.  Measured here and
# committed; the device's bar is 8 x that, the project's margin: MFMA's K order against BLAS's, tanhf's ulps.
SPREAD = 7.5e-6
BAR = 8 * SPREAD


def inputs(net, in_dim, out_dim, activation):
    """The records of a case: obs, g, target, and PPO's raw, logp_old, adv with the float64 rho of record i at RHO[i % 4]."""
    rng = np.random.default_rng(in_dim + out_dim)
    obs = rng.normal(0.0, 1.0, (NREC, in_dim))
    mean = mean_of(net, obs, activation, np.float64)
    sd = np.exp(net["log_std"].astype(np.float64)).astype(np.float32).astype(np.float64)
    raw = (mean + sd * rng.normal(0.0, 1.0, mean.shape)).astype(np.float32)
    u = (raw - mean) / sd
    logp = (-0.5 * u * u - net["log_std"] - 0.5 * np.log(2.0 * np.pi)).sum(-1)
    i = np.arange(NREC)
    return dict(obs=obs, g=rng.normal(0.0, 1.0, mean.shape).astype(np.float32), target=(mean + rng.normal(0.0, 1.0, mean.shape)).astype(np.float32),
                raw=raw, logp_old=logp - np.log(np.array(RHO)[i % 4]), adv=(rng.uniform(0.5, 1.5, NREC) * np.where(i // 4 % 2, -1.0, 1.0)).astype(np.float32))


def grads_of(net, rec, activation, head, rows, dtype, rowsum=None):
    """include/kmanip.h's gradients in `dtype`: the head in float64 on the dtype's mean, the GEMMs in dtype.  rowsum(a, b=None): the
    sum over the rows of a[n, p] (b given: of the outer products a[r] b[r]) -- None: NumPy's own, a.sum(0) and a.T @ b."""
    rowsum = rowsum or (lambda a, b=None: a.sum(0) if b is None else a.T @ b)
    rows = np.arange(NREC) if rows is None else np.array(rows)
    f = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0))
    df = (lambda h: 1 - h * h) if activation == "tanh" else (lambda h: (h > 0).astype(dtype))
    w = {k: net[k].astype(dtype) for k in ("w0", "b0", "w1", "b1", "w2", "b2")}
    x = ((rec["obs"][rows] - net["obs_mean"]) * net["obs_inv_std"]).astype(np.float32).astype(dtype)
    h1 = f(x @ w["w0"].T + w["b0"])
    h2 = f(h1 @ w["w1"].T + w["b1"])
    mean, scale, out = (h2 @ w["w2"].T + w["b2"]).astype(np.float64), 1.0 / len(rows), {}
    if head == "given":
        gm = scale * rec["g"][rows]
    elif head == "mse":
        gm = scale * (mean - rec["target"][rows])
    else:
        sd = np.exp(net["log_std"].astype(np.float64)).astype(np.float32).astype(np.float64)
        u = (rec["raw"][rows] - mean) / sd
        rho = np.exp((-0.5 * u * u - net["log_std"] - 0.5 * np.log(2.0 * np.pi)).sum(-1) - rec["logp_old"][rows])
        adv = rec["adv"][rows].astype(np.float64)
        coef = np.where(rho * adv <= np.clip(rho, 1 - CLIP, 1 + CLIP) * adv, -scale * adv * rho, 0.0)[:, None]
        gm, out["log_std"] = coef * u / sd, rowsum((coef * (u * u - 1)).astype(dtype))
    dz = gm.astype(dtype)
    for l, h in ((2, h2), (1, h1), (0, x)):
        out["w%d" % l], out["b%d" % l] = rowsum(dz, h), rowsum(dz)
        dz = (dz @ w["w%d" % l]) * df(h) if l else None
    return out


def test_the_float32_spread_sets_the_device_bar():
    worst = 0.0
    for in_dim, hidden, od in CASES:
        net = network(in_dim, hidden, od)
        for a in ACTIVATIONS:
            rec = inputs(net, in_dim, od, a)
            for head in HEADS:
                for rows in ROWS:
                    g32, g64 = grads_of(net, rec, a, head, rows, np.float32), grads_of(net, rec, a, head, rows, np.float64)
                    worst = max(worst, max(float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64))
    print("\nworst max|g32 - g64| / max|g64| over the gradient tensors: %.3e" % worst)
    assert worst <= 2 * SPREAD and BAR == 8 * SPREAD      # (another BLAS orders its sums differently: a factor, not a digit)


def test_the_binding_has_the_headers_layout_and_the_sizes_their_formulas():
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    for name in ("KActorGradIn", "KActorGradDev"):
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
        names = [nm for nm, _ in getattr(klib, name)._fields_]
        at = [re.search(r"[ *]%s[,;]" % nm, body).start() for nm in names]
        assert at == sorted(at), name
    assert [nm for nm, _ in klib.KActorGradIn._fields_] == ["head", "n_records", "idx", "obs", "obs_mean", "obs_inv_std", "log_std", "g", "target", "raw",
                                                            "logp_old", "adv", "clip", "scale"]
    assert (C.sizeof(klib.KActorGradIn), C.sizeof(klib.KActorGradDev), klib.KActorGradIn.clip.offset, klib.KActorGradDev.status.offset) == (104, 80, 88, 72)
    assert all("#define KM_AGRAD_%s %d" % (k, v) in re.sub(" +", " ", hdr) for k, v in (("GIVEN", 0), ("MSE", 1), ("PPO_CLIP", 2)))
    new = {"kmanip_actor_grad", "kmanip_actor_grad_pack", "kmanip_actor_grad_packed_floats", "kmanip_actor_grad_workspace_floats"}
    assert new <= set(klib.EXPORTS) and all("KMANIP_API" in ln for ln in hdr.splitlines() if any(" %s(" % s in ln for s in new))
    L = klib.load()
    for in_dim, hidden, od in CASES + [(1, (16, 16), 1), (64, (80, 144), 16), (33, (256, 16), 1)]:
        d = klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, 0)
        assert L.kmanip_actor_grad_packed_floats(C.byref(d)) == klib.actor_grad_packed_floats(in_dim, hidden, od)
        for n in (0, 1, 16, 17, 256, 257, 300, 4096, 16400, 65536):
            assert L.kmanip_actor_grad_workspace_floats(C.byref(d), n) == klib.actor_grad_workspace_floats(in_dim, hidden, od, n) > 0
    assert klib.actor_grad_packed_floats(27, (64, 64), 7) == (4 * 4 + 4 * 4) * 256 + (4 + 4) * 16
    assert klib.actor_grad_splits(300) == (304, 2, 160) and klib.actor_grad_splits(65536) == (65536, 64, 1024) and klib.actor_grad_splits(0)[1] == 0
    assert klib.actor_grad_workspace_floats(27, (64, 64), 7, 33) == 16 * (2 + 8 + 8 + 2) * 48 + 256 * (8 + 16 + 4) + 16 * 10
    for in_dim, hidden, od, a in [(0, (64, 64), 7, 0), (65, (64, 64), 7, 0), (27, (8, 64), 7, 0), (27, (64, 272), 7, 0), (27, (64, 40), 7, 0),
                                  (27, (64, 64), 17, 0), (27, (64, 64), 7, 2)]:
        d = klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, a)
        assert L.kmanip_actor_grad_packed_floats(C.byref(d)) == 0 and L.kmanip_actor_grad_workspace_floats(C.byref(d), 33) == 0
    assert L.kmanip_actor_grad_workspace_floats(C.byref(klib.KActorDesc(27, (C.c_int32 * 2)(64, 64), 7, 0)), -1) == 0


def test_the_library_holds_the_gradient_kernels_without_scratch():
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, "k_actor_bwd")
    assert sorted(r.args for r in rows) == [(4,), (16,)]
    rows += [r for base in ("k_actor_wgrad", "k_actor_grad_reduce", "k_actor_pack_t") for r in BM.kernels(klib.LIB_PATH, base)]
    assert len(rows) == 5
    for r in rows:
        assert r.scratch == 0 and r.lds == 0 and r.vgpr + r.agpr <= 512, r
