"""The edges of kmanip_actor and kmanip_actor_grad on the CPU: the shape lists of the device tests in
test_actor_edges_gpu.py and test_actor_edges_grad_gpu.py, and the bars the float32 arithmetic sets for them -- NumPy float32 against
float64 on the same float32 weights, as test_actor_cpu and test_actor_grad_cpu measure theirs."""
import numpy as np

import test_actor_cpu as AC
import test_actor_grad_cpu as AG

# (in_dim, hidden, out_dim, activation): in_dim 1, 16, 17, 48, 49, 64 (the first layer's four input tiles full, empty or of one column),
# out_dim 1, 4, 5, 12, 13, 16 (the last tile's lane groups full or empty), one hidden size above 64 and one not (NT = 16 by either),
# tile counts that are no multiple of KM_ACTOR_KGROUP (80, 144, 208, 240), the longest NT = 4 chain (64, 64), both activations.
SHAPES = [(1, (64, 64), 1, "tanh"), (16, (64, 80), 4, "relu"), (17, (80, 64), 5, "tanh"), (48, (16, 256), 12, "tanh"),
          (49, (256, 16), 13, "relu"), (64, (144, 208), 16, "tanh"), (49, (240, 256), 5, "tanh"), (64, (48, 16), 16, "relu"),
          (17, (64, 64), 13, "relu"), (1, (144, 208), 1, "relu"), (48, (240, 256), 4, "relu"), (16, (48, 16), 12, "tanh")]
NORMS = ["none", "both", "mean", "inv_std"]      # which of obs_mean / obs_inv_std the actor has; Actor's default is "none"
ALL_NORMS = [SHAPES[2], SHAPES[5]]               # the shapes that run all four; the others run the default
NS = (1, 16, 33)
# The worst |float32 - float64| of the mean over forward_cases() at n = 1, 16 and 33.  Measured here and committed.  It is below
# test_actor_cpu.SPREAD, so the device's bar for these shapes is test_actor_cpu.BAR as it stands.
SPREAD = 6.0e-7
BAR = AC.BAR if SPREAD < AC.SPREAD else 8 * SPREAD

# kmanip_actor_grad's K-split plan: the shapes (NT = 4 and NT = 16), (activation, head), and the row counts -- one row, one tile, an
# exactly full split, a second split of 128 of its 144 rows, 16 full splits, and 16385: np = 16400, KM_AGRAD_MAX_SPLITS = 64 splits of
# 272 rows of which 0..59 are full, 60 holds 80 rows and 61..63 are empty.
GRAD_SHAPES = [(27, (16, 16), 7), (27, (80, 48), 5)]
GRAD_HEADS = [("tanh", "given"), ("tanh", "mse"), ("tanh", "ppo"), ("relu", "ppo")]
GRAD_NS = [1, 16, 256, 257, 4096, 16385]
# The worst max|g32 - g64| / max|g64| over every gradient tensor of GRAD_SHAPES x GRAD_HEADS x GRAD_NS, the float32 sums over the rows
# taken twice -- in NumPy's order and in the plan's (ascending within a split, the splits ascending) -- and the larger kept.
# Measured here and committed; the device's bar is 8 x that.  NumPy's order sets it: b0 of (27, (80, 48), 5), tanh, MSE at 16385 rows,
# one running float32 sum of 16385 terms (4.5e-5); the plan's blocked order stays at 1.8e-6, and the device at 1.3e-6 (DESIGN.md
# section 47), so this bar catches a lost or doubled split, not a rounding: the element-wise probes are the fine checks.
GRAD_SPREAD = 4.5e-5
GRAD_BAR = 8 * GRAD_SPREAD


def grad_rows(n):
    return [(7 * r + 3) % AG.NREC for r in range(n)]


def normed(net, norm):
    """`net` with the normalisation setting `norm`: an unset obs_mean is 0.0 and an unset obs_inv_std 1.0, which are exact in the
    float64 formula, so mean_of and grads_of compute what the kernels' branches do."""
    net = dict(net)
    if norm in ("none", "inv_std"):
        net["obs_mean"] = np.zeros_like(net["obs_mean"])
    if norm in ("none", "mean"):
        net["obs_inv_std"] = np.ones_like(net["obs_inv_std"])
    return net


def forward_cases():
    return [(s, norm) for s in SHAPES for norm in (NORMS if s in ALL_NORMS else NORMS[:1])]


def forward_obs(in_dim):
    return np.random.default_rng(in_dim).normal(0.0, 1.0, (33, in_dim))


def plan_rowsum(n):
    """The float32 sum over n rows in the K-split plan's order: each split's rows ascending from 0.f, then the splits ascending from
    0.f; an empty split adds 0.f, as the reduce kernel adds its zero partial."""
    from gym_kmanip_amd import lib as klib
    _, splits, length = klib.actor_grad_splits(n)

    def rowsum(a, b=None):
        total = np.zeros(a.shape[1:] if b is None else (a.shape[1], b.shape[1]), dtype=a.dtype)
        for s in range(splits):
            lo, hi = s * length, min(n, (s + 1) * length)
            if hi <= lo:
                total = total + np.zeros_like(total)
                continue
            terms = a[lo:hi] if b is None else a[lo:hi, :, None] * b[lo:hi, None, :]
            total = total + np.cumsum(terms, axis=0, dtype=a.dtype)[-1]          # (cumsum adds strictly in order)
        return total
    return rowsum


def test_the_shape_list_covers_what_it_says():
    assert {s[0] for s in SHAPES} >= {1, 16, 17, 48, 49, 64} and {s[2] for s in SHAPES} >= {1, 4, 5, 12, 13, 16}
    assert {s[1] for s in SHAPES} >= {(64, 64), (64, 80), (80, 64), (16, 256), (256, 16), (144, 208), (240, 256), (48, 16)}
    assert {s[3] for s in SHAPES} == set(AC.ACTIVATIONS) and {a for a, _ in GRAD_HEADS} == set(AC.ACTIVATIONS)
    cases = forward_cases()
    assert all((s, "none") in cases for s in SHAPES) and sum(norm == "inv_std" for _, norm in cases) >= 2 and len(cases) == len(SHAPES) + 6
    assert {h for _, h in GRAD_HEADS} == set(AG.HEADS)
    assert [max(s[1]) <= 64 for s in GRAD_SHAPES] == [True, False]            # NT = 4 and NT = 16


def test_the_float32_spread_of_the_edge_shapes_sets_the_forward_bar():
    worst = 0.0
    for (in_dim, hidden, od, a), norm in forward_cases():
        net, obs = normed(AC.network(in_dim, hidden, od), norm), forward_obs(in_dim)
        for n in NS:
            err = float(np.abs(AC.mean_of(net, obs[:n], a, np.float32) - AC.mean_of(net, obs[:n], a, np.float64)).max())
            worst = max(worst, err)
    print("\nworst |float32 - float64| of the mean over the edge shapes: %.3e (test_actor_cpu.SPREAD %.3e)" % (worst, AC.SPREAD))
    assert SPREAD / 2 <= worst <= 2 * SPREAD
    assert BAR == (AC.BAR if SPREAD < AC.SPREAD else 8 * SPREAD)


def test_the_float32_spread_of_the_k_split_plan_sets_the_gradient_bar():
    """16385 rows: a float32 sum of that many terms depends on its order, so the float32 program runs with both."""
    from gym_kmanip_amd import lib as klib
    assert klib.actor_grad_splits(16385) == (16400, 64, 272) and [klib.actor_grad_splits(n)[1] for n in GRAD_NS] == [1, 1, 1, 2, 16, 64]
    worst = {}
    for shape in GRAD_SHAPES:
        net = AC.network(*shape)
        for a, head in GRAD_HEADS:
            rec = AG.inputs(net, shape[0], shape[2], a)
            for n in GRAD_NS:
                rows = grad_rows(n)
                g64 = AG.grads_of(net, rec, a, head, rows, np.float64)
                for order, rowsum in (("numpy", None), ("plan", plan_rowsum(n))):
                    g32 = AG.grads_of(net, rec, a, head, rows, np.float32, rowsum=rowsum)
                    assert all(g32[k].dtype == np.float32 and g32[k].shape == g64[k].shape for k in g64)
                    err, k = max((float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()), k) for k in g64)
                    if err > worst.get(order, (0.0,))[0]:
                        worst[order] = (err, shape, a, head, n, k)
    for order, w in worst.items():
        print("\nworst max|g32 - g64| / max|g64|, rows summed in %s order: %.3e at %s" % (order, w[0], w[1:]))
    top = max(w[0] for w in worst.values())
    assert GRAD_SPREAD / 2 <= top <= 2 * GRAD_SPREAD and GRAD_BAR == 8 * GRAD_SPREAD
