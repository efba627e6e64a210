"""kmanip_actor on the CPU: the bar the float32 arithmetic sets for the device test, the binding against the
header, the packed size against its formula, and the built library's k_actor kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import build_matrix as BM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_DIMS = {"KManipSoloArm": 27, "KManipDualArm": 47}
HIDDEN = [(16, 16), (64, 32), (256, 256)]
ACTIVATIONS = ["tanh", "relu"]
# The worst |float32 - float64| of the mean over the cases below (both in_dims, every HIDDEN, both activations, 33 rows), NumPy float32
# matmuls against float64 ones on the same float32 weights and float32-rounded inputs.  Measured here and committed; the device's bar
# is 8 x that, one digit up: the 8 covers the K order of a 64-step MFMA chain against BLAS's and tanhf's few ulps.
SPREAD = 9.5e-7
BAR = 8e-6


def network(in_dim, hidden, out_dim, seed=0):
    """float32 weights and biases with all entries distinct (no symmetric init: a transposed tile or a permuted K-block shows), a
    log_std, and a non-trivial float64 obs_mean / obs_inv_std."""
    rng = np.random.default_rng(1000 * in_dim + hidden[0] + seed)
    dims = (in_dim,) + tuple(hidden) + (out_dim,)
    net = {}
    grid = lambda shape: (rng.permutation(int(np.prod(shape))).reshape(shape) + 0.5) / np.prod(shape) * 2.0 - 1.0      # distinct, in (-1, 1)
    for l, (i, o) in enumerate(zip(dims, dims[1:])):
        net["w%d" % l] = (grid((o, i)) * 2.0 / np.sqrt(i)).astype(np.float32)
        net["b%d" % l] = (grid((o,)) * 0.5).astype(np.float32)
    assert all(np.unique(v).size == v.size for v in net.values())
    net["log_std"] = rng.uniform(-1.0, 0.2, out_dim).astype(np.float32)
    net["obs_mean"], net["obs_inv_std"] = rng.uniform(-0.3, 0.3, in_dim), rng.uniform(0.5, 2.0, in_dim)
    return net


def mean_of(net, obs, activation, dtype):
    """The network's mean in `dtype` on the float32-rounded normalised input."""
    f = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0))
    h = ((obs - net["obs_mean"]) * net["obs_inv_std"]).astype(np.float32).astype(dtype)
    for l in range(3):
        h = h @ net["w%d" % l].T.astype(dtype) + net["b%d" % l].astype(dtype)
        h = f(h) if l < 2 else h
    return h


def test_the_float32_spread_sets_the_device_bar():
    worst = 0.0
    for in_dim in IN_DIMS.values():
        obs = np.random.default_rng(in_dim).normal(0.0, 1.0, (33, in_dim))
        for hidden in HIDDEN:
            net = network(in_dim, hidden, 14 if in_dim == 47 else 7)
            for a in ACTIVATIONS:
                worst = max(worst, float(np.abs(mean_of(net, obs, a, np.float32) - mean_of(net, obs, a, np.float64)).max()))
    print("\nworst |float32 - float64| of the mean: %.3e" % worst)
    assert worst <= 2 * SPREAD and 8 * SPREAD <= BAR <= 10 * SPREAD      # (another BLAS orders its sums differently: a factor, not a digit)


def test_the_binding_has_the_headers_layout_and_the_packed_size_its_formula():
    from gym_kmanip_amd import lib as klib
    from gym_kmanip_amd import model
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    want = {"KActorDesc": ["in_dim", "hidden", "out_dim", "activation"], "KActorWeights": ["w0", "b0", "w1", "b1", "w2", "b2"],
            "KActorIn": ["envs", "obs", "obs_mean", "obs_inv_std", "log_std"], "KActorDev": ["mean", "act", "raw", "noise", "logp", "status"]}
    for name, names in want.items():
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
        at = [re.search(r"[ *]%s[,;\[]" % nm, body).start() for nm in names]
        assert at == sorted(at) and [nm for nm, _ in getattr(klib, name)._fields_] == names, name
    assert (C.sizeof(klib.KActorDesc), C.sizeof(klib.KActorWeights), C.sizeof(klib.KActorIn), C.sizeof(klib.KActorDev)) == (20, 48, 40, 48)
    assert klib.KActorDesc.hidden.size == 8 and klib.KActorDev.logp.offset == 32
    assert "#define KM_POL_CTR3(step, blk) (0x40000000u + 4u * (uint32_t)(step) + (uint32_t)(blk))" in hdr
    assert model.KM_POL_CTR3(5, 2) == 0x40000000 + 22
    assert {"kmanip_actor", "kmanip_actor_pack", "kmanip_actor_packed_floats"} <= set(klib.EXPORTS)
    L = klib.load()
    assert L.kmanip_actor.argtypes == [C.c_void_p, C.POINTER(klib.KActorDesc), C.c_void_p, C.POINTER(klib.KActorIn), C.c_int,
                                       C.POINTER(klib.KActorDev), C.c_void_p]
    for in_dim, hidden, od in [(27, (64, 64), 7), (47, (256, 256), 14), (1, (16, 16), 1), (64, (80, 144), 16), (33, (256, 16), 1)]:
        d = klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, 0)
        assert L.kmanip_actor_packed_floats(C.byref(d)) == klib.actor_packed_floats(in_dim, hidden, od)
    assert klib.actor_packed_floats(27, (64, 64), 7) == (4 * 4 + 4 * 4 + 1 * 4) * 256 + (4 + 4 + 1) * 16 == 9360
    for in_dim, hidden, od, a in [(0, (64, 64), 7, 0), (65, (64, 64), 7, 0), (27, (8, 64), 7, 0), (27, (64, 272), 7, 0), (27, (64, 40), 7, 0),
                                  (27, (64, 64), 0, 0), (27, (64, 64), 17, 0), (27, (64, 64), 7, 2)]:
        assert L.kmanip_actor_packed_floats(C.byref(klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, a))) == 0


def test_the_library_holds_two_actor_kernels_without_scratch():
    from gym_kmanip_amd import lib as klib
    rows = BM.kernels(klib.LIB_PATH, "k_actor")
    assert sorted(r.args for r in rows) == [(4,), (16,)]
    for r in rows:
        assert r.scratch == 0 and r.lds == 0 and r.vgpr + r.agpr <= 512, r
    assert [r.scratch for r in BM.kernels(klib.LIB_PATH, "k_actor_pack")] == [0]
