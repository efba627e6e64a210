"""Closed-loop rollouts from the CPU oracle: the reference of kmanip_feedback.  oracle/ and rollout_oracle.py stay as they are.

OracleFeedback is OracleRollout with .rollout_feedback of the device's shapes: per row and step, derivatives.tangent_diff on CPU
tensors, a NumPy matvec, then OracleRollout's own one-step path (_step), with the device's status rules -- a non-finite u at step t
stops the row with status 1 and steps_done = t, a gain index outside 0 .. ng-1 gives status 2, the ctrl record of a step is written
with the step's other records and is zero from steps_done on.

THE FIXED GAIN SET (fixed_policy; rng = default_rng(5), s = 1), per trajectory g and step t, drawn in this order: the whole
[ng, nstep, nu, nv] block of qpos columns, then the whole block of qvel columns --
  K[i, i] = -0.5 s and K[i, nv + i] = -0.02 s for i < nu, plus 0.05 s N(0, 1) on the qpos columns and 0.005 s N(0, 1) on the qvel columns.
THE FIXED REFERENCES (fixed_policy; the same generator, after the gains): the cell's state plus 1e-2 N(0, 1) on joints and cube
position (one [ng, nstep, nl + 3] draw), then on qvel (one [ng, nstep, nv] draw); the cube is rotated by 0.3 rad about its body axis
t mod 3 at step t (derivatives.tangent_perturb)."""
import numpy as np

import rollout_oracle as RO

FIELDS = RO.FIELDS + ("ctrl",)
NSTEP = RO.NSTEP
GAIN_SEED = 5
_RUNS = {}


def fixed_policy(cm, qpos, qvel, nstep=NSTEP, s=1.0):
    """(gains [ng, nstep, nu, 2 nv], qpos_ref [ng, nstep, nq], qvel_ref [ng, nstep, nv]) of the module's header for the ng states
    (qpos, qvel), one trajectory per state."""
    import torch
    from gym_kmanip_amd.derivatives import tangent_perturb
    rng = np.random.default_rng(GAIN_SEED)
    ng, nl, nv, nu = len(qpos), cm.nlink, cm.nv, cm.nu
    K = np.zeros((ng, nstep, nu, 2 * nv))
    K[..., :nv] = 0.05 * s * rng.standard_normal((ng, nstep, nu, nv))
    K[..., nv:] = 0.005 * s * rng.standard_normal((ng, nstep, nu, nv))
    for i in range(nu):
        K[..., i, i] += -0.5 * s
        K[..., i, nv + i] += -0.02 * s
    qr = np.repeat(qpos[:, None, :], nstep, axis=1).copy()
    vr = np.repeat(qvel[:, None, :], nstep, axis=1).copy()
    qr[..., :nl + 3] += 1e-2 * rng.standard_normal((ng, nstep, nl + 3))
    vr += 1e-2 * rng.standard_normal((ng, nstep, nv))
    for t in range(nstep):
        qr[:, t] = tangent_perturb(cm, torch.from_numpy(qr[:, t].copy()), nl + 3 + t % 3, 0.3).numpy()
    return K, qr, vr


class OracleFeedback(RO.OracleRollout):
    """OracleRollout plus KManipEnvHip.rollout_feedback.  Every rollout_feedback call is recorded in .fb_calls as the dict of NumPy
    rows it was handed (n, nstep and nsub with them)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.fb_calls = []

    def rollout_feedback(self, envs=None, qpos=None, qvel=None, ctrl=None, warm=None, qfrc_applied=None, gains=None, qpos_ref=None,
                         qvel_ref=None, gain_index=None, nstep=None, nsub=None, out=None, fields=None, gains_t=None):
        import torch
        from gym_kmanip_amd.derivatives import tangent_diff
        is_t = lambda t: isinstance(t, torch.Tensor)
        cm = self.cm
        nq, nv, nu = cm.nq, cm.nv, cm.nu
        as_torch = any(is_t(t) for t in (envs, qpos, qvel, ctrl, warm, qfrc_applied, gains, gains_t, qpos_ref, qvel_ref))
        np_ = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if is_t(t) else t)
        given = dict(qpos=np_(qpos), qvel=np_(qvel), ctrl=np_(ctrl), warm=np_(warm), qfrc_applied=np_(qfrc_applied))
        assert (gains is None) != (gains_t is None)
        K = np_(gains) if gains is not None else np.ascontiguousarray(np.swapaxes(np_(gains_t), -1, -2))
        qr, vr = np_(qpos_ref), np_(qvel_ref)
        per_step = K.ndim == 4
        ng = len(K)
        idx = None if envs is None else np.asarray(np_(envs), dtype=np.int64).reshape(-1)
        gidx = None if gain_index is None else np.asarray(np_(gain_index), dtype=np.int64).reshape(-1)
        n = len(idx) if idx is not None else next((len(v) for v in given.values() if v is not None), self.num_envs)
        lengths = {given[k].shape[1] for k in ("ctrl", "qfrc_applied") if given[k] is not None and given[k].ndim == 3}
        if per_step:
            lengths.add(K.shape[1])
        if nstep is not None:
            lengths.add(int(nstep))
        assert len(lengths) <= 1, "nstep and the per-step tensors disagree"
        nstep = lengths.pop() if lengths else 1
        lead = (ng, nstep) if per_step else (ng,)
        assert K.shape == lead + (nu, 2 * nv) and qr.shape == lead + (nq,) and vr.shape == lead + (nv,)
        assert gidx is not None or ng >= n
        nsub = cm.desc.n_sub_steps if not nsub else int(nsub)
        self.fb_calls.append(dict(given, envs=idx, gain_index=gidx, gains=K, qpos_ref=qr, qvel_ref=vr, n=n, nstep=nstep, nsub=nsub))
        names = list(fields) if fields is not None else list(FIELDS)
        assert not set(names) - set(FIELDS), names
        res = dict(qpos=np.zeros((n, nstep, nq)), qvel=np.zeros((n, nstep, nv)), qacc_warm=np.zeros((n, nstep, nv)),
                   contact_mask=np.zeros((n, nstep), dtype=np.uint32), reward=np.zeros((n, nstep)), status=np.zeros(n, dtype=np.uint8),
                   steps_done=np.zeros(n, dtype=np.int32), ctrl=np.zeros((n, nstep, nu)))
        trail = "contact_mask" in names or "reward" in names
        for r in range(n):
            e = r if idx is None else int(idx[r])
            g = r if gidx is None else int(gidx[r])
            if not (0 <= e < self.num_envs and 0 <= g < ng):
                res["status"][r] = 2
                continue
            get = lambda k: given[k][r] if given[k] is not None else self.state[k][e]
            at = lambda a, t: a[r, t] if a.ndim == 3 else a[r]
            m = self.models[e]
            orc = self._orc[id(m)]
            q, v, w = (np.array(get(k), dtype=np.float64) for k in ("qpos", "qvel", "warm"))
            ok = np.isfinite(q).all() and np.isfinite(v).all() and np.isfinite(w).all()
            for t in range(nstep):
                c = at(given["ctrl"], t) if given["ctrl"] is not None else self.state["ctrl"][e]
                tau = at(given["qfrc_applied"], t) if given["qfrc_applied"] is not None else (None if self.applied is None else self.applied[e])
                if not (ok and np.isfinite(c).all() and (tau is None or np.isfinite(tau).all())):
                    res["status"][r] = 1
                    break
                gt = (g, t) if per_step else (g,)
                dq = tangent_diff(cm, torch.from_numpy(q[None].copy()), torch.from_numpy(qr[gt][None].copy())).numpy()[0]
                with np.errstate(all="ignore"):
                    u = c + K[gt] @ np.concatenate([dq, v - vr[gt]])
                if not np.isfinite(u).all():
                    res["status"][r] = 1
                    break
                q, v, w, bad = self._step(m, orc, q, v, u, w, tau, nsub)
                if bad:
                    res["status"][r] = 1
                    break
                res["qpos"][r, t], res["qvel"][r, t], res["qacc_warm"][r, t], res["ctrl"][r, t] = q, v, w, u
                if trail:
                    res["contact_mask"][r, t] = orc.contact_mask(q)[0]
                    res["reward"][r, t] = orc.observe(q, v)[1]
                res["steps_done"][r] = t + 1
        res["contact_mask"] = res["contact_mask"].view(np.int32)
        return {k: (torch.from_numpy(res[k]) if as_torch else res[k]) for k in names}


def cell_runs(asset, solver="newton", mode="plain", nsub=None, nstep=NSTEP, s=1.0):
    """rollout_oracle.cell_runs under the fixed policy: the regime cells as caller rows on an OracleFeedback of 2 envs, one gain
    trajectory per cell (the twin rows name theirs through gain_index), computed once per argument set and shared by the tests.
    dict(cm, rows, labels, policy (gains, qpos_ref, qvel_ref), open (the open-loop run: rollout_oracle's own entry), ref, twin,
    twin_rows)."""
    key = (asset, solver, mode, nsub, nstep, s)
    if key not in _RUNS:
        run = RO.cell_runs(asset, solver, mode, nsub, nstep)
        cm, rows = run["cm"], run["rows"]
        K, qr, vr = fixed_policy(cm, rows["qpos"], rows["qvel"], nstep, s)
        pol = dict(gains=K, qpos_ref=qr, qvel_ref=vr)
        models = RO.env_params(cm)[1] if "params" in mode else None
        env = OracleFeedback(cm, 2, models=models)
        pick = run["twin_rows"]
        twin = {k: np.ascontiguousarray(v[pick]) for k, v in rows.items()}
        twin["qvel"] = twin["qvel"] * (1.0 + 1e-15)
        _RUNS[key] = dict(cm=cm, rows=rows, labels=run["labels"], policy=pol, open=run["ref"],
                          ref=env.rollout_feedback(nstep=nstep, nsub=nsub, **rows, **pol),
                          twin=env.rollout_feedback(nstep=nstep, nsub=nsub, gain_index=pick.astype(np.int32), **twin, **pol), twin_rows=pick)
    return _RUNS[key]
