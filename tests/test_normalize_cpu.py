"""kmanip_obs_stats and kmanip_reward_scale on the CPU: the bindings against the header, the size formulas, the
built library's four kernels, and THE BAR of the device tests: `obs_stats_model` and `reward_scale_model` are NumPy float64 programs in
the kernels' order (shift, per-lane sums, ascending merges), held against normalize.py's longdouble two-pass references on the device
tests' cases.  The project's bar for float64 reductions is 1e-12 relative (section 48's stats); the models stay inside it on every
case (worst 8.3e-14 for the observations, 1.7e-15 for the rewards), so BAR is that figure: nothing here is derived from a device's output."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_actor_cpu import BM, ROOT
from gym_kmanip_amd import lib as klib
from gym_kmanip_amd.normalize import obs_stats_reference, reward_scale_reference

BAR, EPS, GAMMA = 1e-12, 1e-8, 0.97
DIMS = (1, 27, 49, 64)
SHAPES = ((1, 1), (3, 5), (9, 257), (17, 300))          # below and above one chunk of 8 steps, across a block edge of 256 envs
PATTERNS = ("none", "every", "random")


def row_cases(dim):
    """From lib's constants: single folds that leave a ragged pass, a ragged unroll and a ragged last block, then three successive
    folds of different sizes (more than a block, less than a pass, a ragged unroll)."""
    p, b = klib.KM_OBS_STATS_BLOCK // dim, klib.obs_stats_block_rows(1, dim)
    c = (1, p - 1, p, p + 1, klib.KM_OBS_STATS_UNROLL * p + 1, b + 1, 3 * b - 1)
    return [(n,) for n in c] + [(c[5], c[1], c[4])]


def obs_rows(dim, n, seed=0):
    """Column 0 is 1e3 + 1e-2 noise (an unshifted sum of squares loses ten digits there); from dim 3 on the last column is constant;
    the others have means of 1 to 3 either sign and spreads of 0.1 to 1."""
    cols = np.random.default_rng(dim)
    off, scale = cols.uniform(1.0, 3.0, dim) * cols.choice([-1.0, 1.0], dim), cols.uniform(0.1, 1.0, dim)
    noise = np.random.default_rng(1000 * dim + 7 * n + seed).normal(0.0, 1.0, (n, dim))
    x = off + scale * noise
    x[:, 0] = 1e3 + 1e-2 * noise[:, 0]
    if dim >= 3:
        x[:, -1] = 0.75
    return x


def reward_inputs(T, N, pattern, call):
    rng = np.random.default_rng(100 * T + N + 7919 * call)
    done = {"none": np.zeros((T, N)), "every": np.ones((T, N)), "random": rng.random((T, N)) < 0.3}[pattern].astype(np.uint8)
    return rng.uniform(-0.2, 1.0, (T, N)), done * (1 + np.arange(T * N).reshape(T, N) % 3).astype(np.uint8)


def merge(na, ma, M2a, R, c, s1, s2):
    """include/kmanip.h's merge in float64 (arrays or scalars)."""
    mb, M2b = c + s1 / R, np.maximum(s2 - (s1 * s1) / R, 0.0)
    if not na > 0:
        return float(R), mb, M2b
    n, delta = na + R, mb - ma
    return n, ma + (delta * R) / n, (M2a + M2b) + (((delta * delta) * na) * R) / n


def obs_stats_model(state, x):
    """k_obs_stats and k_obs_stats_finish in NumPy float64 on a state [1 + 2 dim] and rows [R, dim]: (new state, mean, inv_std)."""
    R, dim = x.shape
    p, rows = klib.KM_OBS_STATS_BLOCK // dim, klib.obs_stats_block_rows(R, dim)
    na, ma, M2a = state[0], state[1:1 + dim], state[1 + dim:]
    c = ma if na > 0 else x[0]
    S1, S2 = np.zeros(dim), np.zeros(dim)
    for r0 in range(0, R, rows):                                   # blocks ascending
        d = x[r0:r0 + rows] - c
        b1, b2 = np.zeros(dim), np.zeros(dim)
        for off in range(min(p, len(d))):                          # a column's lanes, ascending row offset; cumsum adds in sequence
            b1, b2 = b1 + np.cumsum(d[off::p], 0)[-1], b2 + np.cumsum(d[off::p] * d[off::p], 0)[-1]
        S1, S2 = S1 + b1, S2 + b2
    n, mean, M2 = merge(na, ma, M2a, float(R), c, S1, S2)
    return np.concatenate([[n], mean, M2]), mean, 1.0 / np.sqrt(M2 / n + EPS)


def reward_scale_model(state, reward, done):
    """k_return_stats and k_reward_scale_finish in NumPy float64 on a state [3 + N]: (new state, scaled, stats)."""
    T, N = reward.shape
    G = state[3:].copy()
    c = state[1] if state[0] > 0 else GAMMA * G[0] + reward[0, 0]
    nb = -(-N // klib.KM_GAE_BLOCK)
    s = np.zeros((2, nb * klib.KM_GAE_BLOCK))
    for t in range(T):
        G = GAMMA * G + reward[t]
        s[0, :N], s[1, :N] = s[0, :N] + (G - c), s[1, :N] + (G - c) * (G - c)
        G = np.where(done[t] != 0, 0.0, G)
    s = s.reshape(2, nb, -1, 64)
    for o in (32, 16, 8, 4, 2, 1):                                 # __shfl_xor within a wave
        s = s + s[..., np.arange(64) ^ o]
    pair = np.cumsum(np.cumsum(s[..., 0], 2)[..., -1], 1)[:, -1]      # the waves of a block ascending, then the blocks ascending
    n, mean, M2 = merge(state[0], state[1], state[2], float(T * N), c, pair[0], pair[1])
    return np.concatenate([[n, mean, M2], G]), reward / np.sqrt(M2 / n + EPS), np.array([mean, np.sqrt(M2 / n)])


def close(got, ref):
    """Every entry within BAR relative of the longdouble reference (an exact zero must be met exactly)."""
    err = np.abs(np.asarray(got, np.longdouble) - ref)
    return bool(np.all(err <= BAR * np.abs(ref))), float(np.max(err / np.maximum(np.abs(ref), np.finfo(np.float64).tiny)))


@pytest.mark.parametrize("dim", DIMS)
def test_the_obs_model_in_kernel_order_stays_inside_the_bar(dim):
    worst = 0.0
    for sizes in row_cases(dim):
        state, seen = np.zeros(1 + 2 * dim), []
        for k, n in enumerate(sizes):
            seen.append(obs_rows(dim, n, k))
            state, mean, inv_std = obs_stats_model(state, seen[-1])
        ref = obs_stats_reference(np.concatenate(seen), EPS)
        for got, want in zip((mean, state[1 + dim:] / state[0], inv_std), ref):
            ok, err = close(got, want)
            worst = max(worst, err)
            assert ok, (sizes, err)
        assert state[0] == sum(sizes) and (dim < 3 or inv_std[-1] == 1.0 / np.sqrt(EPS))
    print("\ndim %d: worst relative error of the float64 model %.2e" % (dim, worst))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_reward_model_in_kernel_order_stays_inside_the_bar(shape, pattern):
    state, hist = np.zeros(3 + shape[1]), []
    for call in range(2):
        reward, done = reward_inputs(*shape, pattern, call)
        hist.append((reward, done))
        state, scaled, stats = reward_scale_model(state, reward, done)
        mean, var, carry = reward_scale_reference(np.concatenate([h[0] for h in hist]), np.concatenate([h[1] for h in hist]), GAMMA)
        res = [close(g, w) for g, w in ((scaled, reward / np.sqrt(var + EPS)), (stats, np.array([mean, np.sqrt(var)])), (state[3:], carry))]
        print("\n%s %s call %d: worst relative error %.2e" % (shape, pattern, call, max(r[1] for r in res)))
        assert all(r[0] for r in res), res


def test_the_bindings_have_the_headers_layout_and_the_sizes_their_formulas():
    hdr = open(os.path.join(ROOT, "include", "kmanip.h")).read()
    for name, (names, size) in {"KObsStatsIn": (["obs", "n_rows", "dim", "eps"], 24), "KRewardScaleIn": (["reward", "done", "T", "N", "gamma", "eps"], 40)}.items():
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
        at = [re.search(r"[ *]%s[,;]" % nm, body).start() for nm in names]
        assert at == sorted(at) and [nm for nm, _ in getattr(klib, name)._fields_] == names and C.sizeof(getattr(klib, name)) == size
    new = {"kmanip_obs_stats", "kmanip_obs_stats_workspace_doubles", "kmanip_reward_scale", "kmanip_reward_scale_workspace_doubles"}
    assert new <= set(klib.EXPORTS) and all("KMANIP_API" in ln for ln in hdr.splitlines() if any(" %s(" % s in ln for s in new))
    assert all("#define KM_OBS_STATS_%s %d" % kv in re.sub(" +", " ", hdr) for kv in (("BLOCK", klib.KM_OBS_STATS_BLOCK), ("UNROLL", klib.KM_OBS_STATS_UNROLL),
               ("PASSES", klib.KM_OBS_STATS_PASSES), ("MAX_BLOCKS", klib.KM_OBS_STATS_MAX_BLOCKS)))
    L = klib.load()
    for n, dim, want in [(1, 27, 54), (576, 27, 54), (577, 27, 108), (262144, 27, 2 * 27 * 456), (0, 27, 0), (-1, 27, 0), (5, 0, 0), (5, 65, 0),
                         (767, 64, 384), (16385, 1, 4), (2 ** 31 - 1, 1, 2 * 1024), (2 ** 31 - 1, 64, 2 * 64 * 1024)]:
        assert L.kmanip_obs_stats_workspace_doubles(n, dim) == klib.obs_stats_workspace_doubles(n, dim) == want, (n, dim)
    for n, want in [(-1, 0), (0, 0), (1, 7), (256, 262), (257, 265), (4096, 4 + 32 + 4096)]:
        assert L.kmanip_reward_scale_workspace_doubles(n) == klib.reward_scale_workspace_doubles(n) == want


@pytest.mark.parametrize("base,lds", [("k_obs_stats", 2 * 256 * 8), ("k_obs_stats_finish", 4096 * 8), ("k_return_stats", 64), ("k_reward_scale_finish", 8)])
def test_the_library_holds_the_new_kernels_without_scratch(base, lds):
    rows = BM.kernels(klib.LIB_PATH, base)
    assert len(rows) == 1 and rows[0].scratch == 0 and rows[0].lds == lds and rows[0].vgpr + rows[0].agpr <= 128, rows
