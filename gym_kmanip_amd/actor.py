"""A learned state-based policy for the batched env: the MLP kmanip_actor evaluates on the matrix cores (include/kmanip.h KActorDesc;
DESIGN.md section 45).

`Actor` owns the torch parameter tensors -- w0, b0, w1, b1, w2, b2, log_std: float32, on the env's device, what a torch optimiser
takes -- and the packed copy the kernel reads; `repack()` rebuilds that copy after the parameters change (three launches, no torch
arithmetic).  `KManipEnvHip.actor_eval` runs it, `KManipEnvHip.collect` runs it between steps; `reference` is the same network in
torch float64: the definition.  `KManipEnvHip.actor_grad` writes the loss gradients of the parameters (kmanip_actor_grad; DESIGN.md
section 46) from the transposed packed copy repack() also keeps; `loss_reference` is that loss in torch float64 under autograd.
`KManipEnvHip.actor_adam` (kmanip_actor_adam) is the optimiser step on these tensors: it keeps its moments in
`adam_state` and its step count in `adam_step`, and rewrites both packed copies itself -- no repack() after it.
`repack_bf16()` keeps a third copy, `packed_bf16`: the weights rounded to bf16 for kmanip_actor_bf16, which
`actor_eval` and `collect` run with precision="bf16".  Neither repack() nor actor_adam touches it: whoever changes the parameters calls
repack_bf16() before the next bf16 evaluation (PPO with collect_precision="bf16" does, once per iteration).
`KManipEnvHip.actor_grad(..., precision="bf16")` (kmanip_actor_grad_bf16) is the gradient of that bf16 network with
bf16 operands, from `packed_bf16` and a fourth copy, `packed_bf16_t`, which repack_bf16() refreshes once it exists;
`loss_reference(precision="bf16")` is its definition, `grad_bf16_definition` the program over plain tensors.
"""
from __future__ import annotations

import ctypes as C

from . import lib as _libmod

_NAMES = ("w0", "b0", "w1", "b1", "w2", "b2")


def round_bf16(t):
    """A float64 tensor rounded to the nearest bf16, ties to even, in ONE rounding (through float32 it would be two): the value keeps
    its 8 leading significand bits.  Exact for zeros and for every magnitude in bf16's normal range."""
    import torch
    bits = t.contiguous().view(torch.int64)
    return ((bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) & ~((1 << 45) - 1)).view(torch.float64)


def grad_bf16_definition(w, x, activation, head, rec, scale, sum_dtype=None):
    """kmanip_actor_grad_bf16's definition (include/kmanip.h) as a program over plain tensors.  w: the float32 parameters by name,
    widened to float64 (log_std with "ppo"); x: float64 [n, in_dim], the normalised input already rounded to float32; rec: the rows'
    float64 head inputs -- {"g"} | {"target"} | {"raw", "logp_old", "adv", "clip"}.  Every product's operands are rounded to bf16
    (round_bf16: one rounding) and summed in `sum_dtype` (None: float64, the reference; torch.float32: the arithmetic of the matrix
    cores, which bounds the device's distance from the reference); the head is float64 per row on the mean.  Returns {"grads",
    "row_loss" (not "given"), "logp" ("ppo"), "inter": x, h1, h2, dz3, dz2, dz1 as they are BEFORE their rounding to bf16}."""
    import math
    import torch
    f64, sd_ = torch.float64, sum_dtype or torch.float64
    q = round_bf16
    f = torch.tanh if activation == "tanh" else torch.relu
    dact = (lambda h: 1.0 - h * h) if activation == "tanh" else (lambda h: (h > 0).to(sd_))
    mm = lambda a, b: a.to(sd_) @ b.to(sd_)
    wq = [q(w[nm]) for nm in ("w0", "w1", "w2")]
    inter, hs = {"x": x}, [q(x)]
    for l in range(2):
        inter["h%d" % (l + 1)] = f(mm(hs[l], wq[l].T) + w["b%d" % l].to(sd_)).to(f64)
        hs.append(q(inter["h%d" % (l + 1)]))
    mean = (mm(hs[2], wq[2].T) + w["b2"].to(sd_)).to(f64)
    out, lt = {}, None
    if head == "given":
        gm = scale * rec["g"]
    elif head == "mse":
        e = mean - rec["target"]
        gm, out["row_loss"] = scale * e, 0.5 * (e * e).sum(-1)
    elif head == "ppo":
        ls = w["log_std"]
        sd = ls.exp().to(torch.float32).to(f64)
        u = (rec["raw"] - mean) / sd
        out["logp"] = (-0.5 * u * u - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        rho, adv, clip = (out["logp"] - rec["logp_old"]).exp(), rec["adv"], float(rec["clip"])
        s, cl = rho * adv, rho.clamp(1.0 - clip, 1.0 + clip) * adv
        coef = torch.where(s <= cl, -scale * adv * rho, torch.zeros_like(rho))[:, None]
        out["row_loss"] = -torch.minimum(s, cl)
        gm, lt = coef * u / sd, (coef * (u * u - 1.0)).to(torch.float32)
    else:
        raise ValueError("grad_bf16_definition: head is 'given', 'mse' or 'ppo'")
    grads, dz = {}, gm.to(torch.float32).to(f64)
    for l in (2, 1, 0):
        inter["dz%d" % (l + 1)] = dz
        dz = q(dz)
        grads["w%d" % l], grads["b%d" % l] = mm(dz.T, hs[l]).to(f64), dz.to(sd_).sum(0).to(f64)
        if l:
            dz = (mm(dz, wq[l]) * dact(hs[l].to(sd_))).to(f64)
    if lt is not None:
        grads["log_std"] = lt.to(sd_).sum(0).to(f64)
    out.update(grads=grads, inter=inter)
    return out


class Actor:
    def __init__(self, env, hidden=(64, 64), activation="tanh", out_dim=None, in_dim=None, seed=0):
        """env: the KManipEnvHip the network belongs to (device, library handle).  in_dim / out_dim: None = the env's obs_dim /
        act_dim.  The weights start as torch.nn.Linear's do, uniform in +-1 / sqrt(fan in), from a generator of their own seeded
        with `seed`; log_std starts at zero.  obs_mean / obs_inv_std: None, or float64 [in_dim] device tensors the caller sets."""
        import torch
        self.env = env
        self.in_dim = int(env.cm.obs_dim if in_dim is None else in_dim)
        self.out_dim = int(env.cm.act_dim if out_dim is None else out_dim)
        self.hidden = tuple(int(v) for v in hidden)
        if len(self.hidden) != 2 or activation not in _libmod.KM_ACTOR:
            raise ValueError("Actor: two hidden sizes and an activation of %s" % sorted(_libmod.KM_ACTOR))
        self.activation = activation
        self.desc = _libmod.KActorDesc(self.in_dim, (C.c_int32 * 2)(*self.hidden), self.out_dim, _libmod.KM_ACTOR[activation])
        floats = env.L.kmanip_actor_packed_floats(C.byref(self.desc))
        if not floats:
            raise _libmod.KManipError("Actor: %d -> %s -> %d is outside what kmanip_actor takes (in_dim 1..%d, hidden sizes multiples of 16 "
                                      "in 16..%d, out_dim 1..%d)" % (self.in_dim, self.hidden, self.out_dim, _libmod.KM_ACTOR_MAX_IN,
                                                                    _libmod.KM_ACTOR_MAX_HIDDEN, _libmod.KM_ACTOR_MAX_OUT))
        gen = torch.Generator().manual_seed(int(seed))
        dims = (self.in_dim,) + self.hidden + (self.out_dim,)
        for l, (i, o) in enumerate(zip(dims, dims[1:])):
            bound = i ** -0.5
            setattr(self, "w%d" % l, ((torch.rand((o, i), generator=gen) * 2 - 1) * bound).to(env.device))
            setattr(self, "b%d" % l, ((torch.rand((o,), generator=gen) * 2 - 1) * bound).to(env.device))
        self.log_std = torch.zeros((self.out_dim,), dtype=torch.float32, device=env.device)
        self.obs_mean = self.obs_inv_std = None
        self.packed = torch.empty((floats,), dtype=torch.float32, device=env.device)
        self.packed_t = torch.empty((env.L.kmanip_actor_grad_packed_floats(C.byref(self.desc)),), dtype=torch.float32, device=env.device)
        self.packed_bf16 = None                      # kmanip_actor_bf16's buffer: repack_bf16() allocates and fills it
        self.packed_bf16_t = None                    # kmanip_actor_grad_bf16's: actor_grad(precision="bf16") allocates it, repack_bf16() refreshes it
        self.grad_workspace = {}                     # (n, precision) -> the gradient call's workspace (KManipEnvHip.actor_grad)
        self.adam_state, self.adam_step = None, 0    # kmanip_actor_adam's moments and step count (KManipEnvHip.actor_adam)
        self.repack()

    @classmethod
    def from_module(cls, env, module, **kw):
        """An Actor with the weights of a torch.nn.Sequential of three Linear layers with a Tanh or a ReLU after the first two."""
        import torch
        lin = [m for m in module if isinstance(m, torch.nn.Linear)]
        acts = {type(m) for m in module if not isinstance(m, torch.nn.Linear)}
        if len(lin) != 3 or acts not in ({torch.nn.Tanh}, {torch.nn.ReLU}) or any(m.bias is None for m in lin):
            raise ValueError("Actor.from_module: three biased Linear layers and one kind of activation, Tanh or ReLU")
        a = cls(env, hidden=(lin[0].out_features, lin[1].out_features), activation="tanh" if acts == {torch.nn.Tanh} else "relu",
                out_dim=lin[2].out_features, in_dim=lin[0].in_features, **kw)
        with torch.no_grad():
            for l, m in enumerate(lin):
                getattr(a, "w%d" % l).copy_(m.weight)
                getattr(a, "b%d" % l).copy_(m.bias)
        a.repack()
        return a

    def parameters(self):
        """The tensors a torch optimiser takes (after its step: repack())."""
        return [getattr(self, nm) for nm in _NAMES] + [self.log_std]

    def repack(self):
        """kmanip_actor_pack and kmanip_actor_grad_pack: the parameter tensors as they are now into the buffers the kernels read (the
        second holds W2^T and W1^T for the backward), on the current stream."""
        import torch
        e, dims = self.env, (self.in_dim,) + self.hidden + (self.out_dim,)
        for l in range(3):
            e._check_buf(getattr(self, "w%d" % l), (dims[l + 1], dims[l]), torch.float32, "w%d" % l)
            e._check_buf(getattr(self, "b%d" % l), (dims[l + 1],), torch.float32, "b%d" % l)
        wt = self._weights()
        e._check(e.L.kmanip_actor_pack(e.h, C.byref(self.desc), C.byref(wt), C.c_void_p(self.packed.data_ptr()), e._stream()),
                 "kmanip_actor_pack")
        e._check(e.L.kmanip_actor_grad_pack(e.h, C.byref(self.desc), C.byref(wt), C.c_void_p(self.packed_t.data_ptr()), e._stream()),
                 "kmanip_actor_grad_pack")

    def _weights(self):
        wt = _libmod.KActorWeights()
        for nm in _NAMES:
            setattr(wt, nm, getattr(self, nm).data_ptr())
        return wt

    def repack_bf16(self, with_t=False):
        """kmanip_actor_bf16_pack: the parameter tensors as they are now, rounded to bf16 (nearest-even), into `packed_bf16` (allocated on
        first use), on the current stream.  repack() and KManipEnvHip.actor_adam do not refresh this copy: call this after the
        parameters change and before the next evaluation with precision="bf16".  Once `packed_bf16_t` exists (with_t, or a first
        actor_grad with precision="bf16") kmanip_actor_grad_bf16_pack refreshes that transposed copy here too: two more launches."""
        import torch
        e = self.env
        if self.packed_bf16 is None:
            self.packed_bf16 = torch.empty((e.L.kmanip_actor_bf16_packed_bytes(C.byref(self.desc)),), dtype=torch.uint8, device=e.device)
        if with_t and self.packed_bf16_t is None:
            self.packed_bf16_t = torch.empty((e.L.kmanip_actor_grad_bf16_packed_bytes(C.byref(self.desc)),), dtype=torch.uint8, device=e.device)
        wt = self._weights()
        e._check(e.L.kmanip_actor_bf16_pack(e.h, C.byref(self.desc), C.byref(wt), C.c_void_p(self.packed_bf16.data_ptr()), e._stream()),
                 "kmanip_actor_bf16_pack")
        if self.packed_bf16_t is not None:
            e._check(e.L.kmanip_actor_grad_bf16_pack(e.h, C.byref(self.desc), C.byref(wt), C.c_void_p(self.packed_bf16_t.data_ptr()), e._stream()),
                     "kmanip_actor_grad_bf16_pack")

    def torch_eval(self, obs):
        """The policy as a torch float32 program on the same parameters -- cast, normalise, three matmuls, sample from torch's global
        generator, clamp, log-probability: what a training script runs between steps without kmanip_actor, for comparisons of cost
        (examples/actor_rollout.py --torch, tests/tools/actor_cost.py).  Returns (act, raw, logp), all float32."""
        import math
        import torch
        x = obs.to(torch.float32)
        if self.obs_mean is not None:
            x = x - self.obs_mean.to(torch.float32)
        if self.obs_inv_std is not None:
            x = x * self.obs_inv_std.to(torch.float32)
        f = torch.tanh if self.activation == "tanh" else torch.relu
        mean = torch.addmm(self.b2, f(torch.addmm(self.b1, f(torch.addmm(self.b0, x, self.w0.T)), self.w1.T)), self.w2.T)
        z = torch.randn_like(mean)
        raw = mean + self.log_std.exp() * z
        return raw.clamp(-1.0, 1.0), raw, (-0.5 * z * z - self.log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1)

    def reference(self, obs, noise=None, precision="f32"):
        """The same network in torch float64: float32 weights widened, the normalised input rounded to float32 as the kernel rounds
        it.  precision="bf16" is kmanip_actor_bf16's definition: the same float64 program with the weights, that float32 input and each
        hidden layer's output rounded to bf16 (nearest-even) before the next product; biases and the last layer's output are not
        rounded.  Returns {"mean"}; with `noise` [n, out_dim] (the kernel's, or model.draw_policy_noise's) also raw, act and logp by
        include/kmanip.h's definition (raw and act in float32, logp in float64)."""
        import math
        import torch
        x = obs.to(torch.float64)
        if self.obs_mean is not None:
            x = x - self.obs_mean
        if self.obs_inv_std is not None:
            x = x * self.obs_inv_std
        if precision not in ("f32", "bf16"):
            raise ValueError("reference: precision is 'f32' or 'bf16'")
        q = round_bf16 if precision == "bf16" else (lambda v: v)
        x = q(x.to(torch.float32).to(torch.float64))
        f = torch.tanh if self.activation == "tanh" else torch.relu
        w = [getattr(self, nm).to(torch.float64) for nm in _NAMES]
        h = q(f(x @ q(w[0]).T + w[1]))
        h = q(f(h @ q(w[2]).T + w[3]))
        out = {"mean": h @ q(w[4]).T + w[5]}
        if noise is not None:
            z = noise.to(torch.float32)
            sd = self.log_std.to(torch.float64).exp().to(torch.float32)
            out["raw"] = out["mean"].to(torch.float32) + sd * z
            out["act"] = out["raw"].clamp(-1.0, 1.0)
            zd = z.to(torch.float64)
            out["logp"] = (-0.5 * zd * zd - self.log_std.to(torch.float64) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        return out

    def loss_reference(self, obs, head, g=None, target=None, ppo=None, idx=None, scale=None, precision="f32"):
        """kmanip_actor_grad's loss in torch float64 under autograd: the definition (include/kmanip.h KActorGradIn).  obs: float64
        [n_records, in_dim]; idx: the records of the rows (None: all, in order); head "given" (g [n_records, out_dim]: the loss is
        scale sum g . mean), "mse" (target) or "ppo" (a dict of raw, logp_old, adv, clip); scale: None = 1 / n.  Returns {"grads": a
        dict by parameter name (log_std for "ppo" only), "row_loss" [n] (not for "given"), "logp" [n] ("ppo")}, all float64.
        precision="bf16" is kmanip_actor_grad_bf16's definition, grad_bf16_definition with float64 sums: explicit formulas, since
        act' from the rounded activation and the roundings of dz are no forward program's autograd (it also returns "inter")."""
        import math
        import torch
        rows = torch.arange(obs.shape[0], device=obs.device) if idx is None else torch.as_tensor(idx, device=obs.device).long()
        scale = 1.0 / max(len(rows), 1) if scale is None else float(scale)
        x = obs.to(torch.float64)[rows]
        if self.obs_mean is not None:
            x = x - self.obs_mean
        if self.obs_inv_std is not None:
            x = x * self.obs_inv_std
        x = x.to(torch.float32).to(torch.float64)
        names = _NAMES + (("log_std",) if head == "ppo" else ())
        if precision == "bf16":
            rec = {"given": {"g": g}, "mse": {"target": target}}.get(head) or {k: ppo[k] for k in ("raw", "logp_old", "adv")}
            rec = dict({k: v.to(torch.float64)[rows] for k, v in rec.items()}, **({"clip": ppo["clip"]} if head == "ppo" else {}))
            return grad_bf16_definition({nm: getattr(self, nm).to(torch.float64) for nm in names}, x, self.activation, head, rec, scale)
        if precision != "f32":
            raise ValueError("loss_reference: precision is 'f32' or 'bf16'")
        f = torch.tanh if self.activation == "tanh" else torch.relu
        w = {nm: getattr(self, nm).to(torch.float64).requires_grad_() for nm in names}
        mean = f(f(x @ w["w0"].T + w["b0"]) @ w["w1"].T + w["b1"]) @ w["w2"].T + w["b2"]
        out = {}
        if head == "given":
            total = (g.to(torch.float64)[rows] * mean).sum()
        elif head == "mse":
            out["row_loss"] = 0.5 * ((mean - target.to(torch.float64)[rows]) ** 2).sum(-1)
            total = out["row_loss"].sum()
        elif head == "ppo":
            ls = w["log_std"]
            sd = ls.exp()
            sd = sd + (sd.detach().to(torch.float32).to(torch.float64) - sd.detach())        # the kernel's float32 value, exp's derivative
            u = (ppo["raw"].to(torch.float64)[rows] - mean) / sd
            out["logp"] = (-0.5 * u * u - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)
            rho, adv, clip = (out["logp"] - ppo["logp_old"].to(torch.float64)[rows]).exp(), ppo["adv"].to(torch.float64)[rows], float(ppo["clip"])
            out["row_loss"] = -torch.minimum(rho * adv, rho.clamp(1.0 - clip, 1.0 + clip) * adv)
            total = out["row_loss"].sum()
        else:
            raise ValueError("loss_reference: head is 'given', 'mse' or 'ppo'")
        grads = torch.autograd.grad(scale * total, [w[nm] for nm in names])
        out = {k: v.detach() for k, v in out.items()}
        out["grads"] = dict(zip(names, grads))
        return out
