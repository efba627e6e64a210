"""Forward dynamics at given rows from the CPU oracle, in NumPy: the reference of kmanip_forward.  oracle/ itself stays as it is.

One row is applied_oracle.forces_decode(cm_of_env, orc, qpos, qvel, ctrl, warm, tau): Oracle.dynamics of the row's state, the exact
minimiser of the forward problem under the applied force (applied_oracle.newton_exact: unique, so the warm start does not enter)
and force_oracle.decode of it.  cm_of_env is model.with_env_params(...) for a row whose env has parameters.

OracleForward is a CPU stand-in for KManipEnvHip with .cm and .forward(...) of the device's shapes (CPU torch tensors), so that
gym_kmanip_amd.derivatives.forward_fd runs on it unchanged and both sides are handed the same rows.  hinv_and_pattern gives what
the reference's own derivative check needs: H^-1 of the row's active set and the activity pattern of its constraint rows."""
import numpy as np

import applied_oracle as AO
import force_oracle as FO


def row(cm, orc, qpos, qvel, ctrl, warm=None, tau=None, geometry=True):
    """forces_decode of one row; tau None = no applied force."""
    tau = np.zeros(cm.nv) if tau is None else tau
    warm = np.zeros(cm.nv) if warm is None else warm
    return AO.forces_decode(cm, orc, np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64),
                            np.asarray(ctrl, dtype=np.float64), warm, np.asarray(tau, dtype=np.float64), geometry=geometry)


def hinv_and_pattern(cm, orc, qpos, qvel, ctrl, qacc):
    """(H^-1, pattern) of one row at its solution qacc: H = M + J^T diag(h) J with h the rows' second derivatives there
    (applied_oracle._rows), pattern = the branch every constraint row is in (friction loss: -1 low, 0 quadratic, +1 high; one-sided
    rows: 1 active, 0 inactive) followed by the contact mask.  While the pattern is the same, qacc is affine in the applied force
    with slope H^-1.  (The rows do not depend on the force: Oracle.dynamics again, no second solve.)"""
    dyn = orc.dynamics(qpos, qvel, ctrl)
    types, floss = orc.constraint_rows(qpos, qvel)
    x = dyn["J"] @ qacc - dyn["aref"]
    h = AO._rows(x, dyn["R"], types, floss)[2] if len(x) else np.zeros(0)
    fl = types == 0
    pat = np.where(x < 0, 1, 0)
    if fl.any():
        Rb = dyn["R"][fl] * floss[fl]
        pat[fl] = np.where(x[fl] <= -Rb, -1, np.where(x[fl] >= Rb, 1, 0))
    H = dyn["M"] + dyn["J"].T @ (h[:, None] * dyn["J"])
    return np.linalg.inv(H), tuple(int(p) for p in pat) + (int(orc.contact_mask(qpos)[0]),)


def slot_layout(nlink, mask):
    """{slot: bit} of a mask in an order KForcesDev allows: the corner bits in the 4 corner slots, the sphere-cube bits in the next
    KM_SPHERE_SLOTS, the sphere-table bits in the rest, each kind in bit order."""
    nss = 2 * (nlink // 10)
    out, nxt = {}, {0: 0, 1: 4, 2: 4 + nss}
    for b in FO.mask_bits(mask):
        kind = 0 if b < 8 else 1 if b < 20 else 2
        out[nxt[kind]] = b
        nxt[kind] += 1
    return out


class OracleForward:
    """KManipEnvHip.forward on the CPU oracle.  state: dict(qpos, qvel, ctrl, warm) of [num_envs, ..] arrays, what the envs "store"
    (needed only for fields a call leaves None); models: one compiled model per env (default: cm for all); applied: [num_envs, nv]
    the "bound" force or None.  Every call is recorded in .calls as the dict of NumPy rows it was handed; with patterns=True
    .patterns also gets, per call, every row's hinv_and_pattern pattern (None for a row with a nonzero status)."""

    def __init__(self, cm, num_envs=1, state=None, models=None, applied=None, patterns=False):
        from oracle.oracle import Oracle
        self.cm, self.num_envs = cm, num_envs
        self.models = [cm] * num_envs if models is None else list(models)
        self._orc = {}
        for m in self.models:
            if id(m) not in self._orc:
                self._orc[id(m)] = Oracle(m, 1)
        self.state, self.applied = state, applied
        self.calls = []
        self.patterns = [] if patterns else None

    def forward(self, envs=None, qpos=None, qvel=None, ctrl=None, warm=None, qfrc_applied=None, out=None, fields=None):
        import torch
        from gym_kmanip_amd.model import contact_slots
        cm = self.cm
        nv, nu, nc = cm.nv, cm.nu, contact_slots(cm.nlink)
        np_ = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
        given = dict(qpos=np_(qpos), qvel=np_(qvel), ctrl=np_(ctrl), warm=np_(warm), qfrc_applied=np_(qfrc_applied))
        idx = None if envs is None else np.asarray(np_(envs), dtype=np.int64).reshape(-1)
        n = len(idx) if idx is not None else next((len(v) for v in given.values() if v is not None), self.num_envs)
        self.calls.append(dict(given, envs=idx))
        names = list(fields) if fields is not None else ["qacc", "qfrc_constraint", "qfrc_actuator", "contact_force", "contact_bit",
                                                         "contact_frame", "contact_pos", "contact_dist", "contact_mask", "status"]
        geometry = any(k in names for k in ("contact_frame", "contact_pos", "contact_dist"))
        res = dict(qacc=np.zeros((n, nv)), qfrc_constraint=np.zeros((n, nv)), qfrc_actuator=np.zeros((n, nu)),
                   contact_force=np.zeros((n, nc, 4)), contact_bit=np.full((n, nc), -1, dtype=np.int32), contact_frame=np.zeros((n, nc, 9)),
                   contact_pos=np.zeros((n, nc, 3)), contact_dist=np.zeros((n, nc)), contact_mask=np.zeros(n, dtype=np.uint32),
                   status=np.zeros(n, dtype=np.uint8))
        pats = [None] * n
        for r in range(n):
            e = r if idx is None else int(idx[r])
            if not 0 <= e < self.num_envs:
                res["status"][r] = 2
                continue
            get = lambda k: given[k][r] if given[k] is not None else self.state[k][e]
            tau = given["qfrc_applied"][r] if given["qfrc_applied"] is not None else (None if self.applied is None else self.applied[e])
            # (the exact minimiser does not depend on its starting point: without a stored warm start the row's is zero)
            wm = get("warm") if given["warm"] is not None or (self.state and "warm" in self.state) else np.zeros(nv)
            vals = [get("qpos"), get("qvel"), get("ctrl"), wm] + ([] if tau is None else [tau])
            if not all(np.isfinite(v).all() for v in vals):
                res["status"][r] = 1
                continue
            m = self.models[e]
            o = row(m, self._orc[id(m)], vals[0], vals[1], vals[2], vals[3], tau, geometry=geometry)
            res["qacc"][r], res["qfrc_constraint"][r], res["qfrc_actuator"][r] = o["qacc"], o["qfrc_constraint"], o["qfrc_actuator"]
            res["contact_mask"][r] = o["mask"]
            if self.patterns is not None:
                pats[r] = hinv_and_pattern(m, self._orc[id(m)], vals[0], vals[1], vals[2], o["qacc"])[1]
            for s, b in slot_layout(cm.nlink, o["mask"]).items():
                c = o["contacts"][b]
                res["contact_bit"][r, s], res["contact_force"][r, s] = b, c["force"]
                if geometry:
                    res["contact_frame"][r, s], res["contact_pos"][r, s], res["contact_dist"][r, s] = c["frame"], c["pos"], c["dist"]
        if self.patterns is not None:
            self.patterns.append(pats)
        res["contact_mask"] = res["contact_mask"].view(np.int32)
        return {k: torch.from_numpy(res[k]) for k in names}
