"""Step derivatives in the per-env physics parameters from the CPU oracle: the reference of kmanip_param_fd.
oracle/, rollout_oracle.py and feedback_oracle.py stay as they are.

Per row r and column c (parameter k, the c-th name of ENV_PARAMS that `wrt` holds), with p the row's parameter vector:
  e = fl(eps_k * p_k) if relative else eps_k;  plus = fl(p_k + e);  minus = fl(p_k - e)
  two OracleRollouts over model.with_env_params(cm, **p with p_k = plus / minus) take ONE step (nsub sub-steps) each from the row's
  state and warm + warm_offset;  column = [tangent_diff(qpos+, qpos-) ; qvel+ - qvel-] / fl(2.0 * e), NumPy float64.
Statuses are the device's: 2 an env index outside the stand-in; 3 the row's parameters, plus or minus outside the parameter's limits
(model.check_env_param), or e zero or not finite -- nothing is stepped; 1 either row stopped.  A nonzero column is zeros; the contact
mask of a row that did not step or stopped is 0.

OracleParamFd is OracleFeedback with .param_fd of KManipEnvHip's signature and shapes, and .set_env_params / .get_env_params, which
rebuild the stand-in's per-env models: sysid.identify runs on it unchanged."""
import numpy as np

import feedback_oracle as FO
import rollout_oracle as RO

# the issue's check values: 1.5 x the model's cube mass, friction 0.7, friction loss 0.02, kp_scale 1.2
TRUE_PARAMS = dict(cube_mass=1.5, cube_friction=0.7, cube_frictionloss=0.02, kp_scale=1.2)      # (cube_mass: a factor on the model's)
KINDS = ("P_qpos", "P_qvel")
_REF = {}


def true_params(cm):
    return dict(TRUE_PARAMS, cube_mass=TRUE_PARAMS["cube_mass"] * cm.desc.cube_mass)


def _value_ok(name, v):
    from gym_kmanip_amd.model import check_env_param
    try:
        check_env_param(name, v)
    except ValueError:
        return False
    return True


def param_fd_rows(cm, num_envs, envs, qpos, qvel, ctrl, warm, params, wrt, eps, relative=True, warm_offset=1.0, nsub=None, qfrc_applied=None):
    """The reference over NumPy rows: params [n, KM_EP_N], eps [KM_EP_N].  dict(deriv_t [n, npar, 2 nv], status_cols [n, npar] uint8,
    contact_mask_fd [n, npar, 2] int32)."""
    import torch
    from gym_kmanip_amd.derivatives import tangent_diff
    from gym_kmanip_amd.model import ENV_PARAMS, with_env_params
    order = [k for k, name in enumerate(ENV_PARAMS) if name in wrt]
    n, nv, npar = len(qpos), cm.nv, len(order)
    deriv = np.zeros((n, npar, 2 * nv))
    status = np.zeros((n, npar), dtype=np.uint8)
    mask = np.zeros((n, npar, 2), dtype=np.int32)
    for r in range(n):
        e_idx = r if envs is None else int(envs[r])
        if not 0 <= e_idx < num_envs:
            status[r] = 2
            continue
        p = np.array(params[r], dtype=np.float64)
        row_ok = all(_value_ok(name, p[j]) for j, name in enumerate(ENV_PARAMS))
        for c, k in enumerate(order):
            with np.errstate(all="ignore"):
                e = np.float64(eps[k]) * p[k] if relative else np.float64(eps[k])
                plus, minus = p[k] + e, p[k] - e
            if not (row_ok and np.isfinite(e) and e != 0.0 and _value_ok(ENV_PARAMS[k], plus) and _value_ok(ENV_PARAMS[k], minus)):
                status[r, c] = 3
                continue
            ends = []
            for side, val in enumerate((plus, minus)):
                pv = p.copy()
                pv[k] = val
                m = with_env_params(cm, **{name: float(pv[j]) for j, name in enumerate(ENV_PARAMS)})
                env = RO.OracleRollout(cm, 1, models=[m])
                with np.errstate(all="ignore"):
                    w0 = warm[r:r + 1] + warm_offset
                out = env.rollout(envs=np.zeros(1, dtype=np.int32), qpos=qpos[r:r + 1], qvel=qvel[r:r + 1], ctrl=ctrl[r:r + 1], warm=w0,
                                  qfrc_applied=None if qfrc_applied is None else qfrc_applied[r:r + 1], nstep=1, nsub=nsub,
                                  fields=("qpos", "qvel", "contact_mask", "status"))
                ends.append(out)
                if out["status"][0] == 0:
                    mask[r, c, side] = out["contact_mask"][0, 0]
            if ends[0]["status"][0] or ends[1]["status"][0]:
                status[r, c] = 1
                continue
            dq = tangent_diff(cm, torch.from_numpy(ends[0]["qpos"][:, 0].copy()), torch.from_numpy(ends[1]["qpos"][:, 0].copy())).numpy()[0]
            dv = ends[0]["qvel"][0, 0] - ends[1]["qvel"][0, 0]
            deriv[r, c] = np.concatenate([dq, dv]) / (2.0 * e)
    return dict(deriv_t=deriv, status_cols=status, contact_mask_fd=mask)


class OracleParamFd(FO.OracleFeedback):
    """OracleFeedback plus KManipEnvHip.param_fd, set_env_params and get_env_params.  .params [num_envs, KM_EP_N]: the values in force
    (the compiled model's until set_env_params); .models follows them."""

    def __init__(self, cm, num_envs=1, **kw):
        from gym_kmanip_amd.model import ENV_PARAMS, env_param_defaults
        super().__init__(cm, num_envs, **kw)
        base = env_param_defaults(cm)
        self.params = np.tile(np.array([base[name] for name in ENV_PARAMS]), (num_envs, 1))
        self.param_fd_calls = 0
        self._ep_ranges = None

    def set_env_params(self, **fields):
        from oracle.oracle import Oracle
        from gym_kmanip_amd.model import ENV_PARAMS, env_param_defaults, with_env_params
        assert not set(fields) - set(ENV_PARAMS), fields
        base = env_param_defaults(self.cm)
        as_np = lambda v: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)
        p = np.stack([np.broadcast_to(as_np(base[name] if fields.get(name) is None else fields[name]), (self.num_envs,))
                      for name in ENV_PARAMS], axis=1).copy()
        models = [with_env_params(self.cm, **{name: float(p[e, j]) for j, name in enumerate(ENV_PARAMS)}) for e in range(self.num_envs)]
        self.params, self.models = p, models
        self._orc = {id(m): Oracle(m, 1) for m in models}

    def get_env_params(self):
        import torch
        from gym_kmanip_amd.model import ENV_PARAMS
        return {name: torch.from_numpy(self.params[:, j].copy()) for j, name in enumerate(ENV_PARAMS)}

    def param_fd(self, envs=None, qpos=None, qvel=None, ctrl=None, qfrc_applied=None, warm=None, params=None, nsub=None, eps=1e-4,
                 relative=True, wrt=None, warm_offset=1.0, out=None):
        import torch
        from gym_kmanip_amd.model import ENV_PARAMS
        wrt = ENV_PARAMS if wrt is None else ((wrt,) if isinstance(wrt, str) else tuple(wrt))
        assert not set(wrt) - set(ENV_PARAMS), wrt
        is_t = lambda t: isinstance(t, torch.Tensor)
        np_ = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if is_t(t) else t)
        idx = None if envs is None else np.asarray(np_(envs), dtype=np.int64).reshape(-1)
        given = dict(qpos=np_(qpos), qvel=np_(qvel), ctrl=np_(ctrl), warm=np_(warm))
        n = len(idx) if idx is not None else next((len(v) for v in given.values() if v is not None), self.num_envs)
        env_of = np.arange(n) if idx is None else idx
        safe = np.clip(env_of, 0, self.num_envs - 1)
        for k in given:                                  # a None field: what the named env stores
            if given[k] is None:
                given[k] = np.ascontiguousarray(self.state[k][safe])
        if isinstance(params, dict):
            cols = [self.params[safe, j] if params.get(name) is None else np.broadcast_to(np.asarray(np_(params[name]), dtype=np.float64), (n,))
                    for j, name in enumerate(ENV_PARAMS)]
            p = np.stack(cols, axis=1)
        else:
            p = self.params[safe] if params is None else np_(params)
        e = np.array([float(eps.get(name, 1e-4) if isinstance(eps, dict) else eps) for name in ENV_PARAMS])
        self.param_fd_calls += 1
        res = param_fd_rows(self.cm, self.num_envs, env_of, given["qpos"], given["qvel"], given["ctrl"], given["warm"], p, wrt, e, relative,
                            warm_offset, nsub, np_(qfrc_applied))
        res = {k: torch.from_numpy(v) for k, v in res.items()}
        res["P"] = res["deriv_t"].transpose(1, 2)
        res["status_fd"] = res["status_cols"].amax(dim=1) if res["status_cols"].shape[1] else torch.zeros(n, dtype=torch.uint8)
        res["contact_mask_fd"] = res["contact_mask_fd"].permute(1, 2, 0)
        res["wrt"] = tuple(name for name in ENV_PARAMS if name in wrt)
        return res


def fd_params(cm, n):
    """[n, KM_EP_N]: the check values (true_params) on every row."""
    from gym_kmanip_amd.model import ENV_PARAMS
    p = true_params(cm)
    return np.tile(np.array([p[name] for name in ENV_PARAMS]), (n, 1))


def reference(asset, nsub, twin=False):
    """param_fd on rollout_oracle's FD_CELLS rows (envs = arange(6) % 2) at the check values, the model at the default solver
    tolerance, eps 1e-4 relative, warm_offset 1: computed once, (cm, rows, params, result as NumPy).  twin: from qvel (1 + 1e-15)."""
    key = (asset, nsub, twin)
    if key not in _REF:
        cm = RO.fd_model(asset, 1e-8)
        rows = RO.fd_rows(asset, cm)
        if twin:
            rows["qvel"] = rows["qvel"] * (1.0 + 1e-15)
        p = fd_params(cm, len(rows["qpos"]))
        from gym_kmanip_amd.model import ENV_PARAMS
        res = param_fd_rows(cm, 2, rows["envs"], rows["qpos"], rows["qvel"], rows["ctrl"], rows["warm"], p, ENV_PARAMS, np.full(4, 1e-4),
                            True, 1.0, nsub)
        _REF[key] = (cm, rows, p, res)
    return _REF[key]


def blocks(deriv_t, nv):
    """The two column kinds the bars are set for: the qpos (tangent) and the qvel rows of P, from deriv_t [n, npar, 2 nv]."""
    d = np.asarray(deriv_t)
    return {"P_qpos": d[:, :, :nv], "P_qvel": d[:, :, nv:]}
