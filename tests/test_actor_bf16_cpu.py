"""kmanip_actor_bf16 on the CPU: the binding against the header, the packed size against its formula, the built
library's k_actor_bf16 kernels, and the bars that float32 accumulation sets for test_actor_bf16_gpu.py -- the bf16 definition
(include/kmanip.h) in NumPy with float32 sums against the same definition with float64 sums, on exactly the device test's cases."""
import ctypes as C
import os
import re

import numpy as np

import test_actor_cpu as AC
import test_actor_edges_cpu as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (in_dim, hidden, out_dim): in_dim 1, 17, 33, 49, 64 (K-steps of one column, half full, one over, full), out_dim 1, 5, 16, odd tile
# counts (80: tile 4 pairs with a zero tile; 48, 144, 208), one and eight K-steps a layer, NT = 4 (the first two) and NT = 16
SHAPES = [(1, (16, 16), 1), (17, (64, 64), 5), (33, (80, 48), 16), (49, (48, 80), 1), (64, (16, 256), 5), (17, (256, 16), 16),
          (33, (144, 208), 5), (64, (256, 256), 16)]
NS = (1, 16, 33)
CASES = [(s, a, norm) for s in SHAPES for a in AC.ACTIVATIONS for norm in ("none", "both")]
# The worst |float32 sums - float64 sums| of the bf16 definition's mean over CASES x NS.  A float32 sum can carry a hidden unit across a
# bf16 rounding boundary (one part in 2^8 of the unit, times a weight): that is most of the figure, and it is measured, not excluded.
# Measured here and committed; the device's bar is 8 x that, as sections 45 to 47 set theirs.
SPREAD = 4.7e-4
BAR = 8 * SPREAD
# The worst |logp of the float32 network - logp of the bf16 behaviour policy| at raw = mean_bf16 + sd z over 132 records of PPO_SHAPE:
# the two float64 references, the distance bf16 puts between them.  The bar of actor_grad's logp against logp_old is 8 x that.
PPO_SHAPE = (27, (64, 64), 7)
LOGP_SPREAD = 4.4e-2
LOGP_BAR = 8 * LOGP_SPREAD


def bf16(a):
    """A float32 or float64 array rounded to the nearest bf16, ties to even, in one rounding, in its own dtype."""
    a = np.ascontiguousarray(a)
    sh, I = (16, np.uint32) if a.dtype == np.float32 else (45, np.uint64)
    b = a.view(I)
    return ((b + I((1 << (sh - 1)) - 1) + ((b >> I(sh)) & I(1))) & ~I((1 << sh) - 1)).view(a.dtype)


def mean_bf16(net, obs, activation, dtype):
    """include/kmanip.h's bf16 definition with sums in `dtype`."""
    f = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0))
    h = bf16(((obs - net["obs_mean"]) * net["obs_inv_std"]).astype(np.float32).astype(dtype))
    for l in range(3):
        h = h @ bf16(net["w%d" % l].astype(dtype)).T + net["b%d" % l].astype(dtype)
        h = bf16(f(h)) if l < 2 else h
    return h


def packed_bf16(net, dims):
    """kmanip_actor_bf16's buffer as uint16, by the header's formula."""
    parts = []
    for l, (i, o) in enumerate(zip(dims, dims[1:])):
        ot, ks = -(-o // 16), 2 * -(-i // 64)
        w, b = np.zeros((16 * ot, 32 * ks), np.float32), np.zeros(16 * ot, np.float32)
        w[:o, :i], b[:o] = net["w%d" % l], net["b%d" % l]
        bits = (bf16(w).view(np.uint32) >> 16).astype(np.uint16).reshape(ot, 16, ks, 2, 4, 4)       # [t2, m, s, half, g, c]
        parts += [bits.transpose(0, 2, 4, 1, 3, 5).reshape(-1), b.view(np.uint16)]                  # [t2, s, lane (g, m), half, c]
    return np.concatenate(parts)


def case_net(shape, norm):
    return EC.normed(AC.network(*shape), norm), EC.forward_obs(shape[0])


def test_the_binding_the_packed_size_and_the_kernels():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import build_matrix as BM
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    L, D, vp = klib.load(), C.POINTER(klib.KActorDesc), C.c_void_p
    want = {"kmanip_actor_bf16_packed_bytes": [D], "kmanip_actor_bf16_pack": [vp, D, C.POINTER(klib.KActorWeights), vp, vp],
            "kmanip_actor_bf16": [vp, D, vp, C.POINTER(klib.KActorIn), C.c_int, C.POINTER(klib.KActorDev), vp]}
    for name, args in want.items():
        decl = re.search(r"KMANIP_API \w+ %s\(([^)]*)\);" % name, hdr).group(1)
        assert name in klib.EXPORTS and getattr(L, name).argtypes == args and len(decl.split(",")) == len(args), name
    assert L.kmanip_actor_bf16_packed_bytes.restype == C.c_size_t and "#define KM_ACTOR_BF16_KGROUP %d " % klib.KM_ACTOR_BF16_KGROUP in hdr
    for in_dim, hidden, od in [(27, (64, 64), 7), (47, (256, 256), 14), (1, (16, 16), 1), (64, (80, 144), 16), (33, (256, 16), 1)]:
        d = klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, 0)
        assert L.kmanip_actor_bf16_packed_bytes(C.byref(d)) == klib.actor_bf16_packed_bytes(in_dim, hidden, od)
        assert 2 * packed_bf16(AC.network(in_dim, hidden, od), (in_dim,) + hidden + (od,)).size == klib.actor_bf16_packed_bytes(in_dim, hidden, od)
    assert klib.actor_bf16_packed_bytes(27, (64, 64), 7) == (4 * 2 + 4 * 2 + 1 * 2) * 1024 + (4 + 4 + 1) * 64 == 19008
    for in_dim, hidden, od, a in [(0, (64, 64), 7, 0), (65, (64, 64), 7, 0), (27, (8, 64), 7, 0), (27, (64, 272), 7, 0), (27, (64, 40), 7, 0),
                                  (27, (64, 64), 0, 0), (27, (64, 64), 17, 0), (27, (64, 64), 7, 2)]:
        assert L.kmanip_actor_bf16_packed_bytes(C.byref(klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, a))) == 0
    rows = BM.kernels(klib.LIB_PATH, "k_actor_bf16")
    assert sorted(r.args for r in rows) == [(4,), (16,)]
    for r in rows:
        assert r.scratch == 0 and r.lds == 0 and r.vgpr + r.agpr <= 512, r
    assert [r.scratch for r in BM.kernels(klib.LIB_PATH, "k_actor_pack_bf16")] == [0]


def test_the_float32_sums_of_the_bf16_definition_set_the_device_bars():
    worst = 0.0
    for shape, a, norm in CASES:
        net, obs = case_net(shape, norm)
        for n in NS:
            worst = max(worst, float(np.abs(mean_bf16(net, obs[:n], a, np.float32) - mean_bf16(net, obs[:n], a, np.float64)).max()))
    print("\nworst |float32 sums - float64 sums| of the bf16 mean: %.3e" % worst)
    assert SPREAD / 2 <= worst <= 2 * SPREAD and BAR == 8 * SPREAD
    # the logp bar: the float32 network's density of the bf16 policy's sample against the bf16 policy's own
    net, rng = AC.network(*PPO_SHAPE), np.random.default_rng(49)
    obs, z = rng.normal(0.0, 1.0, (132, PPO_SHAPE[0])), rng.normal(0.0, 1.0, (132, PPO_SHAPE[2])).astype(np.float32).astype(np.float64)
    sd = np.exp(net["log_std"].astype(np.float64))
    u = z + (mean_bf16(net, obs, "tanh", np.float64) - AC.mean_of(net, obs, "tanh", np.float64)) / sd
    dlogp = float(np.abs((-0.5 * (u * u - z * z)).sum(-1)).max())
    print("worst |logp float32 network - logp_old| %.3e" % dlogp)
    assert LOGP_SPREAD / 2 <= dlogp <= 2 * LOGP_SPREAD and LOGP_BAR == 8 * LOGP_SPREAD
