"""PPO on the device: a small driver over the library's five training calls.  One iteration is a fixed sequence
of launches on the current stream -- collect, gae, then per epoch and minibatch actor_grad (the clipped surrogate) + actor_adam for
the policy and actor_grad (the squared error on the returns) + actor_adam for the critic -- with no torch arithmetic on the parameters
and no host synchronisation: the same seeds give the same bytes.  With normalize_obs / normalize_reward two more
library calls join the stream: kmanip_reward_scale between collect and gae, kmanip_obs_stats after the last Adam step.

PPO          the driver: buffers allocated once, iterate() runs one iteration and returns device tensors

Out of scope, as in include/kmanip.h: an entropy bonus, value-loss clipping, per-minibatch advantage normalisation, learning-rate
schedules (set .lr between iterations), clipping the normalised observations."""


class PPO:
    def __init__(self, env, actor, critic, nsteps=16, epochs=4, minibatches=4, lr=3e-4, gamma=0.99, lam=0.95, clip=0.2, max_grad_norm=0.5,
                 betas=(0.9, 0.999), eps=1e-8, seed=0, collect_precision="f32", update_precision="f32",
                 normalize_obs=False, normalize_reward=False):
        """env: a KManipEnvHip; actor, critic: Actors mapping obs_dim to act_dim and to 1.  Each iteration collects nsteps steps of
        every env and makes `epochs` passes over the nsteps * num_envs records in `minibatches` index lists each, drawn from a host
        generator seeded with `seed` (a permutation per epoch).  collect_precision="bf16" collects with kmanip_actor_bf16: the behaviour
        policy is the bf16 network and logp_old its density, against which actor_grad (float32, unchanged) forms the exact importance
        ratio; iterate() then refreshes the bf16 copy with actor.repack_bf16() before each collect, after the previous Adam steps.
        update_precision="bf16" (it needs collect_precision="bf16") runs the POLICY's actor_grad as kmanip_actor_grad_bf16 (DESIGN.md
        section 50): the learner's forward is the behaviour policy's to the bit, so the ratio of the first minibatch starts at 1;
        actor.repack_bf16() then follows every policy Adam step.  The critic stays float32.
        normalize_obs: one normalize.ObsStats (self.obs_stats) is attached to actor and critic.  The statistics are FROZEN from collect
        to the last Adam step of an iteration -- logp_old, value and the learner's forward all see the same normalisation, so the first
        minibatch's ratio still starts at 1 -- and are folded with buf["obs"][:nsteps] at the end of iterate(): the first iteration
        runs with mean 0 and inverse std 1.  normalize_reward: gae reads the rewards divided by the running std of the discounted
        return (normalize.RewardScale, self.reward_scale, with this gamma); iterate() still reports the raw mean reward.  Both False:
        the launches and the bytes of section 50."""
        import torch
        self.env, self.actor, self.critic = env, actor, critic
        self.nsteps, self.epochs, self.minibatches = int(nsteps), int(epochs), int(minibatches)
        if collect_precision not in ("f32", "bf16"):
            raise ValueError("PPO: collect_precision is 'f32' or 'bf16'")
        if update_precision not in ("f32", "bf16") or (update_precision == "bf16" and collect_precision != "bf16"):
            raise ValueError("PPO: update_precision is 'f32' or 'bf16', and 'bf16' needs collect_precision='bf16'")
        self.collect_precision, self.update_precision = collect_precision, update_precision
        self.lr, self.gamma, self.lam, self.clip, self.max_grad_norm, self.betas, self.eps = lr, gamma, lam, clip, max_grad_norm, betas, eps
        self.n = self.nsteps * env.num_envs
        if not 1 <= self.minibatches <= self.n:
            raise ValueError("PPO: between 1 and nsteps * num_envs minibatches")
        self.gen = torch.Generator().manual_seed(int(seed))
        self.idx = torch.empty((self.epochs, self.n), dtype=torch.int32, device=env.device)
        self.buf = self.adv = None
        self.grads = [{}, {}]                        # actor_grad's outputs by minibatch size, policy and critic: allocated once each
        self.iterations = 0
        self.obs_stats = self.reward_scale = None
        if normalize_obs or normalize_reward:
            from .normalize import ObsStats, RewardScale
            if normalize_obs:
                self.obs_stats = ObsStats(env).attach(actor, critic)
            if normalize_reward:
                self.reward_scale = RewardScale(env, gamma)

    def _step(self, which, net, obs, rows, **head):
        env, n = self.env, int(rows.numel())
        bf16 = which == 0 and self.update_precision == "bf16"
        out = env.actor_grad(net, obs, idx=rows, out=self.grads[which].get(n), set_grad=False, precision="bf16" if bf16 else "f32", **head)
        self.grads[which][n] = out
        env.actor_adam(net, self.lr, self.betas, self.eps, self.max_grad_norm, grads=out, log_std=which == 0)
        if bf16:
            net.repack_bf16()
        return out["row_loss"].mean()

    def iterate(self):
        """One iteration.  Returns {"policy_loss", "value_loss": the mean row_loss of every update [epochs, minibatches], "reward": the
        mean reward of the rollout, "adv_stats": kmanip_gae's mean and std}, all device tensors: nothing is read back here."""
        import torch
        env, T, n = self.env, self.nsteps, self.n
        # the index lists: drawn on the host and uploaded before the first launch, from pinned memory of their own (torch keeps the block
        # until the copy has run: the host never waits for it and never writes over it)
        host = torch.stack([torch.randperm(n, generator=self.gen) for _ in range(self.epochs)]).to(torch.int32).pin_memory()
        self.idx.copy_(host, non_blocking=True)
        if self.collect_precision == "bf16":
            self.actor.repack_bf16()
        self.buf = env.collect(self.actor, T, critic=self.critic, out=self.buf, precision=self.collect_precision)
        gbuf = self.buf if self.reward_scale is None else dict(self.buf, reward=self.reward_scale.update(self.buf))
        self.adv = env.gae(gbuf, self.gamma, self.lam, normalize=True, out=self.adv)
        obs = self.buf["obs"][:T].view(n, -1)
        ppo = dict(raw=self.buf["raw"].view(n, -1), logp_old=self.buf["logp"].view(n), adv=self.adv["adv"].view(n), clip=self.clip)
        ret = self.adv["ret"].view(n, 1)
        cuts = [n * k // self.minibatches for k in range(self.minibatches + 1)]
        losses = [[], []]
        for e in range(self.epochs):
            for lo, hi in zip(cuts, cuts[1:]):
                rows = self.idx[e, lo:hi]
                losses[0].append(self._step(0, self.actor, obs, rows, ppo=ppo))
                losses[1].append(self._step(1, self.critic, obs, rows, target=ret))
        if self.obs_stats is not None:
            self.obs_stats.update(self.buf["obs"][:T])
        self.iterations += 1
        shape = (self.epochs, self.minibatches)
        return {"policy_loss": torch.stack(losses[0]).view(shape), "value_loss": torch.stack(losses[1]).view(shape),
                "reward": self.buf["reward"].mean(), "adv_stats": self.adv["stats"]}
