"""Running statistics for PPO on the device (include/kmanip.h KObsStatsIn, KRewardScaleIn): what RL users know as
VecNormalize, as two library calls between collect() and gae() -- no torch arithmetic, no host synchronisation, the same bytes on
every run.

ObsStats     the column moments of every observation seen, folded batch by batch (kmanip_obs_stats); `mean` and `inv_std` are the
             tensors an Actor takes as obs_mean / obs_inv_std, and attach() hands THESE VERY tensors to the actors: an update reaches
             every network with no copy
RewardScale  the moments of the discounted return of every env, carried across calls (kmanip_reward_scale); update() returns the
             buffer's rewards divided by the running standard deviation

obs_stats_reference / reward_scale_reference (each class's `reference`) are the definitions in NumPy longdouble: two passes, no shift, no
merge."""
from __future__ import annotations

import ctypes as C

from . import lib as _libmod


def obs_stats_reference(rows, eps=1e-8):
    """kmanip_obs_stats' definition over ALL rows folded so far (array-like [n, dim], n >= 1), two passes in NumPy longdouble: (mean,
    M2 / n, inv_std)."""
    import numpy as np
    x = np.asarray(rows, dtype=np.longdouble)
    mean = x.sum(0) / x.shape[0]
    var = ((x - mean) ** 2).sum(0) / x.shape[0]
    return mean, var, 1 / np.sqrt(var + np.longdouble(eps))


def reward_scale_reference(reward, done, gamma):
    """kmanip_reward_scale's definition over the WHOLE history (array-likes [T total, N], every call's buffer concatenated in time), the
    plain loop in NumPy longdouble: (mean, M2 / n of all returns, the carried returns after the last step)."""
    import numpy as np
    r, d = np.asarray(reward, dtype=np.longdouble), np.asarray(done) != 0
    G, every = np.zeros(r.shape[1], np.longdouble), []
    for t in range(r.shape[0]):
        G = np.longdouble(gamma) * G + r[t]
        every.append(G)
        G = np.where(d[t], 0, G)
    every = np.stack(every)
    mean = every.sum() / every.size
    return mean, ((every - mean) ** 2).sum() / every.size, G


class ObsStats:
    def __init__(self, env, dim=None, eps=1e-8):
        """env: the KManipEnvHip whose device and handle are used; dim: None = the env's obs_dim.  `state` is float64 [1 + 2 dim]:
        the count, the means, the sums of squared distances from the mean; `mean` starts at 0 and `inv_std` at 1 (no normalisation)."""
        import torch
        self.env, self.dim, self.eps = env, int(env.cm.obs_dim if dim is None else dim), float(eps)
        if not 1 <= self.dim <= _libmod.KM_ACTOR_MAX_IN:
            raise _libmod.KManipError("ObsStats: dim is in 1 .. %d" % _libmod.KM_ACTOR_MAX_IN)
        self.state = torch.zeros((1 + 2 * self.dim,), dtype=torch.float64, device=env.device)
        self.mean = torch.zeros((self.dim,), dtype=torch.float64, device=env.device)
        self.inv_std = torch.ones((self.dim,), dtype=torch.float64, device=env.device)
        self.workspace = None

    def update(self, obs):
        """kmanip_obs_stats: every leading row of `obs` (contiguous float64 [..., dim]) folded into the state, `mean` and `inv_std`
        rewritten in place -- two launches on the current stream.  Returns self."""
        import torch
        e = self.env
        e._check_buf(obs, tuple(obs.shape[:-1]) + (self.dim,) if isinstance(obs, torch.Tensor) and obs.dim() else (-1, self.dim), torch.float64, "obs")
        n = obs.numel() // self.dim
        need = _libmod.obs_stats_workspace_doubles(n, self.dim)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty((max(need, 2),), dtype=torch.float64, device=e.device)
        oi = _libmod.KObsStatsIn(obs=obs.data_ptr() if n else None, n_rows=n, dim=self.dim, eps=self.eps)
        e._check(e.L.kmanip_obs_stats(e.h, C.byref(oi), C.c_void_p(self.state.data_ptr()), C.c_void_p(self.workspace.data_ptr()),
                                      C.c_void_p(self.mean.data_ptr()), C.c_void_p(self.inv_std.data_ptr()), e._stream()), "kmanip_obs_stats")
        return self

    def attach(self, *actors):
        """Each actor's obs_mean / obs_inv_std become `mean` / `inv_std` themselves (not copies).  Returns self."""
        for a in actors:
            if a.in_dim != self.dim:
                raise _libmod.KManipError("ObsStats.attach: the actor reads %d inputs, the statistics have %d columns" % (a.in_dim, self.dim))
            a.obs_mean, a.obs_inv_std = self.mean, self.inv_std
        return self

    def reference(self, rows):
        """obs_stats_reference with this eps: (mean, M2 / n, inv_std) of all rows folded so far, in longdouble."""
        return obs_stats_reference(rows, self.eps)


class RewardScale:
    def __init__(self, env, gamma, eps=1e-8):
        """`state` is float64 [3 + num_envs]: the count, mean and sum of squared distances of every discounted return seen, then each
        env's carried return; `stats` [2] the running mean and std."""
        import torch
        self.env, self.gamma, self.eps = env, float(gamma), float(eps)
        self.state = torch.zeros((3 + env.num_envs,), dtype=torch.float64, device=env.device)
        self.stats = torch.zeros((2,), dtype=torch.float64, device=env.device)
        self.workspace = torch.empty((_libmod.reward_scale_workspace_doubles(env.num_envs),), dtype=torch.float64, device=env.device)
        self.scaled = None

    def update(self, buf):
        """kmanip_reward_scale on a collect() buffer's reward and done [T, num_envs]: the returns continue from the carried ones, their
        moments merge into the state, and the rewards divided by the new running std are returned -- a float64 [T, num_envs] tensor
        allocated once per T and overwritten by the next call.  Two launches on the current stream."""
        import torch
        e, N = self.env, self.env.num_envs
        T = int(buf["reward"].shape[0]) if isinstance(buf["reward"], torch.Tensor) and buf["reward"].dim() == 2 else -1
        e._check_buf(buf["reward"], (T, N), torch.float64, "reward")
        e._check_buf(buf["done"], (T, N), torch.uint8, "done")
        if self.scaled is None or self.scaled.shape[0] != T:
            self.scaled = torch.empty((T, N), dtype=torch.float64, device=e.device)
        ri = _libmod.KRewardScaleIn(reward=buf["reward"].data_ptr(), done=buf["done"].data_ptr(), T=T, N=N, gamma=self.gamma, eps=self.eps)
        e._check(e.L.kmanip_reward_scale(e.h, C.byref(ri), C.c_void_p(self.state.data_ptr()), C.c_void_p(self.workspace.data_ptr()),
                                         C.c_void_p(self.scaled.data_ptr()), C.c_void_p(self.stats.data_ptr()), e._stream()), "kmanip_reward_scale")
        return self.scaled

    def reference(self, reward, done):
        """reward_scale_reference with this gamma: (mean, M2 / n, carried returns) of the whole history, in longdouble."""
        return reward_scale_reference(reward, done, self.gamma)
