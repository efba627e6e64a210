"""Open-loop rollouts in ctrl space from the CPU oracle, in NumPy: the reference of kmanip_rollout.  oracle/ itself stays as it is.

One step of one row is nsub sub-steps, each a plain mj_step:
  - a row without an applied force whose env has the compiled model iterates Oracle.physics_step(qpos, qvel, ctrl, warm,
    qpos_step1=qpos, nsub) -- the oracle's own sub-step loop with nothing teleported;
  - a row with a force, or whose env has parameters of its own, iterates applied_oracle.physics_step(cm_of_env, orc, qpos, qvel, ctrl,
    warm, tau, nsub), the restatement in NumPy with the force in qacc_smooth; cm_of_env = model.with_env_params(...) is handed in
    as `models`.
The contact mask of the state after a step is Oracle.contact_mask of it, the reward Oracle.observe's.

OracleRollout is a CPU stand-in for KManipEnvHip with .cm and .rollout(...) of the device's shapes, so that
gym_kmanip_amd.derivatives.transition_fd runs on it unchanged and both sides are handed the same rows.  It takes NumPy arrays or
CPU torch tensors and returns torch tensors if it was handed any, NumPy arrays otherwise."""
import numpy as np

import applied_oracle as AO

FIELDS = ("qpos", "qvel", "qacc_warm", "contact_mask", "reward", "status", "steps_done")


NSTEP = 3
PARAMS = dict(cube_mass=2.0, cube_friction=0.5, cube_frictionloss=0.0, kp_scale=1.3)      # (cube_mass: a factor on the model's)
TWIN_STRIDE = 4
_RUNS = {}


def step_forces(cm, n, nstep=NSTEP):
    """[n, nstep, nv]: the test forces (applied_oracle.draw_test_forces) given per step, a different row each step: tau (t + 1) / nstep."""
    tau = AO.draw_test_forces(cm, n)
    return np.ascontiguousarray(tau[:, None, :] * (np.arange(1, nstep + 1)[None, :, None] / float(nstep)))


def env_params(cm):
    """{name: [2]} explicit per-env parameters of a 2-env handle, different per env (env 0 the compiled model's values), and the
    two compiled models."""
    from gym_kmanip_amd.model import env_param_defaults, with_env_params
    p = dict(PARAMS, cube_mass=PARAMS["cube_mass"] * cm.desc.cube_mass)
    base = env_param_defaults(cm)
    return {k: np.array([base[k], p[k]]) for k in p}, [cm, with_env_params(cm, **p)]


def cell_runs(asset, solver="newton", mode="plain", nsub=None, nstep=NSTEP):
    """The regime cells of the asset (regime_states.cells) sent as caller rows to an OracleRollout of 2 envs (envs = arange(n) % 2),
    nstep steps of nsub sub-steps: computed once per argument set and shared by the tests.  mode: "plain", "forced" (step_forces per
    step), "params" (env_params: env 1's model differs), "params+forced".  dict(cm, rows (the keyword arguments of rollout() as NumPy
    arrays), labels, ref, twin, twin_rows): twin is the same run from qvel (1 + 1e-15) -- the distance between the two is the
    reference's own error in the cell -- on every cell where the rows take the oracle's own step, on every TWIN_STRIDE-th (twin_rows)
    where they take the restatement in NumPy (7 ms a sub-step)."""
    import regime_states as R
    from oracle.oracle import Oracle
    key = (asset, solver, mode, nsub, nstep)
    if key not in _RUNS:
        cm = R.model(asset, solver)
        qpos, qvel, ctrl, labels = R.cells(asset)
        n = len(labels)
        warm = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
        models = env_params(cm)[1] if "params" in mode else None
        rows = dict(envs=(np.arange(n) % 2).astype(np.int32), qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm)
        if "forced" in mode:
            rows["qfrc_applied"] = step_forces(cm, n, nstep)
        env = OracleRollout(cm, 2, models=models)
        # (the strided twins start at row 1 where the envs' models differ: odd rows name env 1, the one with parameters of its own)
        pick = np.arange(n) if mode == "plain" else np.arange(1 if "params" in mode else 0, n, TWIN_STRIDE)
        twin = {k: np.ascontiguousarray(v[pick]) for k, v in rows.items()}
        twin["qvel"] = twin["qvel"] * (1.0 + 1e-15)
        _RUNS[key] = dict(cm=cm, rows=rows, labels=labels, ref=env.rollout(nstep=nstep, nsub=nsub, **rows),
                          twin=env.rollout(nstep=nstep, nsub=nsub, **twin), twin_rows=pick)
    return _RUNS[key]


class OracleRollout:
    """KManipEnvHip.rollout on the CPU oracle.  state: dict(qpos, qvel, ctrl, warm) of [num_envs, ..] arrays, what the envs "store"
    (needed only for fields a call leaves None); models: one compiled model per env (default: cm for all); applied: [num_envs, nv]
    the "bound" force or None.  Every call is recorded in .calls as the dict of NumPy rows it was handed."""

    def __init__(self, cm, num_envs=1, state=None, models=None, applied=None):
        from oracle.oracle import Oracle
        self.cm, self.num_envs = cm, num_envs
        self.models = [cm] * num_envs if models is None else list(models)
        self._orc = {}
        for m in self.models:
            if id(m) not in self._orc:
                self._orc[id(m)] = Oracle(m, 1)
        self.state, self.applied = state, applied
        self.calls = []

    def _step(self, m, orc, qpos, qvel, ctrl, warm, tau, nsub):
        """(qpos, qvel, warm, bad) one step on."""
        if tau is None and m is self.cm:
            q, v, w, bad = orc.physics_step(qpos, qvel, ctrl, warm, qpos, nsub)[:4]
        else:
            q, v, w = AO.physics_step(m, orc, qpos, qvel, ctrl, warm, np.zeros(self.cm.nv) if tau is None else tau, nsub)
            bad = 0
        if not (np.isfinite(q).all() and np.isfinite(v).all() and np.isfinite(w).all() and np.abs(w).max() <= 1e10):
            bad = 1
        return q, v, w, bad

    def rollout(self, envs=None, qpos=None, qvel=None, ctrl=None, warm=None, qfrc_applied=None, nstep=None, nsub=None, out=None,
                fields=None):
        try:
            import torch
            is_t = lambda t: isinstance(t, torch.Tensor)
        except ImportError:                      # (NumPy callers need no torch)
            torch, is_t = None, (lambda t: False)
        cm = self.cm
        nq, nv = cm.nq, cm.nv
        as_torch = any(is_t(t) for t in (envs, qpos, qvel, ctrl, warm, qfrc_applied))
        np_ = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if is_t(t) else t)
        given = dict(qpos=np_(qpos), qvel=np_(qvel), ctrl=np_(ctrl), warm=np_(warm), qfrc_applied=np_(qfrc_applied))
        idx = None if envs is None else np.asarray(np_(envs), dtype=np.int64).reshape(-1)
        n = len(idx) if idx is not None else next((len(v) for v in given.values() if v is not None), self.num_envs)
        lengths = {given[k].shape[1] for k in ("ctrl", "qfrc_applied") if given[k] is not None and given[k].ndim == 3}
        if nstep is not None:
            lengths.add(int(nstep))
        assert len(lengths) <= 1, "nstep and the per-step tensors disagree"
        nstep = lengths.pop() if lengths else 1
        nsub = cm.desc.n_sub_steps if not nsub else int(nsub)
        self.calls.append(dict(given, envs=idx, nstep=nstep, nsub=nsub))
        names = list(fields) if fields is not None else list(FIELDS)
        assert not set(names) - set(FIELDS), names
        res = dict(qpos=np.zeros((n, nstep, nq)), qvel=np.zeros((n, nstep, nv)), qacc_warm=np.zeros((n, nstep, nv)),
                   contact_mask=np.zeros((n, nstep), dtype=np.uint32), reward=np.zeros((n, nstep)), status=np.zeros(n, dtype=np.uint8),
                   steps_done=np.zeros(n, dtype=np.int32))
        trail = "contact_mask" in names or "reward" in names
        for r in range(n):
            e = r if idx is None else int(idx[r])
            if not 0 <= e < self.num_envs:
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
                q, v, w, bad = self._step(m, orc, q, v, c, w, tau, nsub)
                if bad:
                    res["status"][r] = 1
                    break
                res["qpos"][r, t], res["qvel"][r, t], res["qacc_warm"][r, t] = q, v, w
                if trail:
                    res["contact_mask"][r, t] = orc.contact_mask(q)[0]
                    res["reward"][r, t] = orc.observe(q, v)[1]
                res["steps_done"][r] = t + 1
        res["contact_mask"] = res["contact_mask"].view(np.int32)
        return {k: (torch.from_numpy(res[k]) if as_torch else res[k]) for k in names}


# ------------------------------------------------------------------------------------------------- transition_fd on chosen cells
# six cells per asset: the free cube in flight (C2: its first impact falls inside a control step), resting contact (T1: the arm lying
# on the table, the cube at rest on it), a grasp (G1), a pinch (P1; the single arm reaches none: its one-finger push G3 stands in, as
# in DESIGN.md section 26), joint limits (L1) and a servo at its force limit (F1)
FD_CELLS = {"solo_arm": ("C2", "T1", "G1", "G3", "L1", "F1"), "dual_arm": ("C2", "T1", "G1", "P1", "L1", "F1"),
            "torso": ("C2", "T1", "G1", "P1", "L1", "F1")}
# the solver tolerance of the derivative tests' models (the default is 1e-8): DESIGN.md section 27 records the scan behind it
FD_TOLERANCE = 1e-10
FD_BLOCKS = ("A_qpos", "A_qvel", "B_qpos", "B_qvel")
_FD = {}


def fd_model(asset, tolerance=FD_TOLERANCE):
    import mujoco_pin
    from gym_kmanip_amd.model import compile_model
    return compile_model(mujoco_pin.qpos_spec(asset), auto_reset=False, solver="newton", solver_tolerance=tolerance)


def fd_rows(asset, cm):
    """The FD_CELLS rows of the asset as transition_fd's keyword arguments (NumPy), envs = arange(6) % 2."""
    import regime_states as R
    from oracle.oracle import Oracle
    qpos, qvel, ctrl, labels = R.cells(asset)
    pick = [labels.index(c) for c in FD_CELLS[asset]]
    warm = R.warm_start(cm, Oracle(cm, 1), qpos, qvel, ctrl)
    return dict(envs=(np.arange(len(pick)) % 2).astype(np.int32), qpos=qpos[pick], qvel=qvel[pick], ctrl=ctrl[pick], warm=warm[pick])


def fd_blocks(d, nv):
    """The four blocks of a transition_fd result the bars are set for: the qpos (tangent) and the qvel rows of A and of B."""
    A, B = (d[k].detach().cpu().numpy() for k in ("A", "B"))
    return {"A_qpos": A[:, :nv], "A_qvel": A[:, nv:], "B_qpos": B[:, :nv], "B_qvel": B[:, nv:]}


def fd_dist(a, b):
    """{block: [cells]} worst |a - b| of every cell's block, normalised by max(1, max|a|) of that cell's block."""
    out = {}
    for k in a:
        n = len(a[k])
        out[k] = np.abs(a[k] - b[k]).reshape(n, -1).max(axis=1) / np.maximum(1.0, np.abs(a[k]).reshape(n, -1).max(axis=1))
    return out


def fd_reference(asset, nsub, twin=False, tolerance=FD_TOLERANCE):
    """transition_fd over OracleRollout on the FD_CELLS rows (twin: from qvel (1 + 1e-15)), computed once: (cm, rows, env, result)."""
    import torch
    from gym_kmanip_amd.derivatives import transition_fd
    key = (asset, nsub, twin, tolerance)
    if key not in _FD:
        cm = fd_model(asset, tolerance)
        rows = fd_rows(asset, cm)
        if twin:
            rows["qvel"] = rows["qvel"] * (1.0 + 1e-15)
        env = OracleRollout(cm, 2)
        _FD[key] = (cm, rows, env, transition_fd(env, nsub=nsub, **{k: torch.from_numpy(v) for k, v in rows.items()}))
    return _FD[key]
