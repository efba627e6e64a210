"""kmanip_actor_grad_bf16 on the CPU: the bar that float32 accumulation sets for test_actor_grad_bf16_gpu.py --
gym_kmanip_amd.actor.grad_bf16_definition with float32 sums against the same program with float64 sums, on exactly the device test's
random cases -- and the bindings, the two size formulas and the built library's kernels."""
import ctypes as C
import os
import re

import numpy as np

from test_actor_cpu import ACTIVATIONS, BM, ROOT, network
from test_actor_grad_cpu import CLIP, HEADS, NREC, inputs

# NT = 4 with one tile a layer; five and three tiles (an odd count pairs with a zero tile); NT = 4 full; NT = 16 with nine tiles
SHAPES = [(27, (16, 16), 7), (49, (80, 48), 5), (64, (64, 64), 16), (17, (256, 144), 1)]
ROWS = [list(range(3)), None, [(7 * r + 3) % NREC for r in range(300)]]      # n = 3, 33 (two K-steps), 300 (two K-splits of 160)
# The worst max|g32 - g64| / max|g64| over every gradient tensor of SHAPES x ACTIVATIONS x HEADS x ROWS.  A float32 sum can carry an
# activation or a dz across a bf16 rounding boundary (one part in 2^8 of it): that dominates the figure and is not excluded.  Measured
# here and committed; the device's bar is 8 x that, as sections 45 to 49 set theirs.
SPREAD = 3.5e-4
BAR = 8 * SPREAD


def definition(shape, activation, head, rows, sum_dtype=None):
    """grad_bf16_definition on the case's records: test_actor_cpu.network's weights, test_actor_grad_cpu.inputs' records."""
    import torch
    from gym_kmanip_amd.actor import grad_bf16_definition
    net = network(*shape)
    rec, pick = inputs(net, shape[0], shape[2], activation), np.arange(NREC) if rows is None else np.array(rows)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))
    x = t(((rec["obs"][pick] - net["obs_mean"]) * net["obs_inv_std"]).astype(np.float32))
    r = {k: t(rec[k][pick]) for k in {"given": ("g",), "mse": ("target",), "ppo": ("raw", "logp_old", "adv")}[head]}
    w = {k: t(net[k]) for k in ("w0", "b0", "w1", "b1", "w2", "b2", "log_std")}
    return grad_bf16_definition(w, x, activation, head, dict(r, clip=CLIP), 1.0 / len(pick), sum_dtype)


def test_the_float32_sums_of_the_definition_set_the_device_bar():
    import torch
    worst = {}
    for shape in SHAPES:
        for a in ACTIVATIONS:
            for head in HEADS:
                for rows in ROWS:
                    g32, g64 = (definition(shape, a, head, rows, dt)["grads"] for dt in (torch.float32, None))
                    for k in g64:
                        worst[k] = max(worst.get(k, 0.0), float((g32[k] - g64[k]).abs().max() / g64[k].abs().max()))
    print("\nworst max|g32 - g64| / max|g64| by tensor: %s" % {k: "%.3e" % v for k, v in worst.items()})
    assert SPREAD / 2 <= max(worst.values()) <= 2 * SPREAD and BAR == 8 * SPREAD


def test_the_bindings_the_sizes_and_the_kernels():
    from gym_kmanip_amd import lib as klib
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    L, D, vp = klib.load(), C.POINTER(klib.KActorDesc), C.c_void_p
    want = {"kmanip_actor_grad_bf16_packed_bytes": [D], "kmanip_actor_grad_bf16_workspace_bytes": [D, C.c_int],
            "kmanip_actor_grad_bf16_pack": [vp, D, C.POINTER(klib.KActorWeights), vp, vp],
            "kmanip_actor_grad_bf16": [vp, D, vp, vp, C.POINTER(klib.KActorGradIn), C.c_int, vp, C.POINTER(klib.KActorGradDev), vp]}
    for name, args in want.items():
        decl = re.search(r"KMANIP_API \w+ %s\(([^)]*)\);" % name, hdr).group(1)
        assert name in klib.EXPORTS and getattr(L, name).argtypes == args and len(decl.split(",")) == len(args), name
        assert not name.endswith("bytes") or getattr(L, name).restype == C.c_size_t
    for in_dim, hidden, od in SHAPES + [(1, (16, 16), 1), (64, (256, 256), 16), (33, (256, 16), 1)]:
        d = klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, 0)
        assert L.kmanip_actor_grad_bf16_packed_bytes(C.byref(d)) == klib.actor_grad_bf16_packed_bytes(in_dim, hidden, od) > 0
        for n in (0, 1, 32, 33, 256, 257, 300, 600, 4096, 65536, 65600):
            assert L.kmanip_actor_grad_bf16_workspace_bytes(C.byref(d), n) == klib.actor_grad_bf16_workspace_bytes(in_dim, hidden, od, n) > 0
    assert klib.actor_grad_bf16_packed_bytes(27, (64, 64), 7) == 4 * (2 * 1024 + 64) * 2
    assert [klib.actor_grad_bf16_splits(n) for n in (0, 33, 300, 600, 65536)] == [(32, 0, 32), (64, 1, 64), (320, 2, 160), (608, 3, 224), (65536, 64, 1024)]
    assert klib.actor_grad_bf16_workspace_bytes(27, (64, 64), 7, 33) == 32 * (2 + 8 + 8 + 1) * 64 + 64 * 64 + 4 * (256 * (8 + 16 + 4) + 16 * 10)
    for in_dim, hidden, od, a in [(0, (64, 64), 7, 0), (65, (64, 64), 7, 0), (27, (8, 64), 7, 0), (27, (64, 272), 7, 0), (27, (64, 40), 7, 0),
                                  (27, (64, 64), 17, 0), (27, (64, 64), 7, 2)]:
        d = klib.KActorDesc(in_dim, (C.c_int32 * 2)(*hidden), od, a)
        assert L.kmanip_actor_grad_bf16_packed_bytes(C.byref(d)) == 0 and L.kmanip_actor_grad_bf16_workspace_bytes(C.byref(d), 33) == 0
    assert L.kmanip_actor_grad_bf16_workspace_bytes(C.byref(klib.KActorDesc(27, (C.c_int32 * 2)(64, 64), 7, 0)), -1) == 0
    rows = BM.kernels(klib.LIB_PATH, "k_actor_bwd_bf16")
    assert sorted(r.args for r in rows) == [(4,), (16,)]
    rows += [r for base in ("k_actor_wgrad_bf16", "k_actor_pack_t_bf16") for r in BM.kernels(klib.LIB_PATH, base)]
    print("\n%s" % "\n".join(str(r) for r in rows))
    assert len(rows) == 4 and all(r.scratch == 0 and r.lds == 0 and r.vgpr <= 512 for r in rows)      # (vgpr_count is the unified total, AGPRs included)
