"""`env_hip` -- the MI355X backend behind gym-kmanip's own backend seam.

The reference picks a backend by calling a module-level `new(gym_env)` and then only ever calls
k_reset / k_step / k_render / k_close on the returned object (reference gym_kmanip/env_base.py:192-200,
:217,:221,:242,:266); `env_sim.new` (env_sim.py:206-211) and `env_real.new` are the two existing
backends.  `env_hip.new(gym_env, num_envs, device)` is the third: same attribute reads from `gym_env`
(mjcf_filename, seed, q_len, q_pos_home, q_id_*_mask, ctrl_id_*_grip, obs_list, act_list), same return
tuple `(terminated, reward, discount, observation, sim_time)` (env_sim.py:194,200), every element with a
leading [num_envs] dimension and the observation an OrderedDict in obs_list order.

Buffers are PyTorch-ROCm tensors (device memory + streams only; all arithmetic is in the HIP library).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Optional

import numpy as np

from . import lib as _libmod
from .model import (CAMERAS, CONTROL_TIMESTEP, ENV_PARAMS, ENV_SPECS, KM_ACT_KEYS, KM_CAM_INDEX, KM_VP_N, VISUAL_PARAMS,
                    CompiledModel, EnvSpec, camera_intrinsics, check_link_capsules, check_visual_param, compile_model, env_param_defaults,
                    link_capsules, visual_param_defaults, visual_param_vector)

MJCF_TO_ASSET = {"_env_solo_arm.xml": "solo_arm", "_env_dual_arm.xml": "dual_arm", "_env_torso.xml": "torso"}


def _torch():
    import torch
    return torch


class KManipEnvHip:
    """Batched simulated backend.  One instance <-> one device <-> one stream at a time."""

    def __init__(self, cm: CompiledModel, num_envs: int = 1, device: int = 0, seed: int = 0,
                 env_id_offset: int = 0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _libmod.KManipError("env_hip needs a HIP device (torch.cuda.is_available() is False); "
                                      "there is no CPU fallback")
        self.L = _libmod.load()
        self.cm = cm
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", device)
        self.device_index = device
        self.seed, self.env_id_offset = int(seed), int(env_id_offset)
        h = C.c_void_p()
        rc = self.L.kmanip_create(C.byref(cm.desc), self.num_envs, device, C.c_uint64(seed),
                                  C.c_int64(env_id_offset), C.byref(h))
        if rc != 0:
            raise _libmod.KManipError("kmanip_create failed (%d): %s" % (rc, self.L.kmanip_last_error(None).decode()))
        self.h = h
        n = self.num_envs
        self.obs = torch.zeros((n, cm.obs_dim), dtype=torch.float64, device=self.device)
        self.reward = torch.zeros((n,), dtype=torch.float64, device=self.device)
        self.done = torch.zeros((n,), dtype=torch.uint8, device=self.device)
        self.act = torch.zeros((n, cm.act_dim), dtype=torch.float32, device=self.device)
        # k_step return values that never change (terminated is always False in the reference: get_termination -> None,
        # discount 1.0) and the device-side counters behind sim_time: allocated once, no per-step allocation or sync
        self.terminated = torch.zeros((n,), dtype=torch.bool, device=self.device)
        self.discount = torch.ones((n,), dtype=torch.float64, device=self.device)
        self.sim_time = torch.zeros((n,), dtype=torch.float64, device=self.device)
        self._check(self.L.kmanip_bind_sim_time(self.h, C.c_void_p(self.sim_time.data_ptr())), "kmanip_bind_sim_time")
        self._ep_active = False          # per-env parameters in force (set_env_params / set_env_param_ranges)
        self._ep_ranges = None           # (lo, hi) float64[KM_EP_N] of ranges mode, or None
        self._vp_active = False          # per-env visual parameters in force (set_visual_params / set_visual_param_ranges)
        self._vp_ranges = None           # (lo, hi) float64[KM_VP_N] of visual ranges mode, or None
        self.applied_force = None        # the bound qfrc_applied tensor (bind_applied_force), or None

    # ------------------------------------------------------------------ helpers
    def _check(self, rc, what):
        if rc != 0:
            raise _libmod.KManipError("%s failed (%d): %s" % (what, rc, self.L.kmanip_last_error(self.h).decode()))

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def obs_dict(self, obs=None) -> "OrderedDict":
        """Zero-copy per-key views of the flat observation, in obs_list order (env_sim.py:111-139)."""
        obs = self.obs if obs is None else obs
        out = OrderedDict()
        for key in self.cm.spec.obs_list:
            if key in self.cm.obs_slices:
                out[key] = obs[:, self.cm.obs_slices[key]]
        return out

    def _check_buf(self, t, shape, dtype, what):
        """Device / dtype / layout checks of a caller-supplied tensor whose raw pointer goes to the kernel (a float64
        action, a CPU tensor, a strided view or a wrong leading dimension would otherwise be silent garbage or a fault)."""
        torch = _torch()
        if not isinstance(t, torch.Tensor):
            raise _libmod.KManipError("%s must be a torch tensor on %s, got %s" % (what, self.device, type(t).__name__))
        if (not t.is_cuda) or t.device != self.device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise _libmod.KManipError("%s must be a contiguous %s tensor of shape %s on %s; got %s %s on %s%s" % (
                what, dtype, tuple(shape), self.device, t.dtype, tuple(t.shape), t.device,
                "" if t.is_contiguous() else " (non-contiguous)"))

    def _query_out(self, table, lead, dims, out, fields, dev, noun):
        """The outputs of a query: `table` maps a field to (trailing shape in terms of `dims`, dtype name); a field is `lead` + that
        shape, or lead[:1] where the table has None (one value per row).  The fields are those of `out`, else `fields`, else all;
        without `out` they are allocated.  Every tensor is checked and its pointer set in `dev`, the entry's ctypes struct.
        Returns `out`."""
        torch = _torch()
        shapes = {name: (lead[:1] if shp is None else lead + tuple(dims.get(d, d) for d in shp), getattr(torch, dt))
                  for name, (shp, dt) in table.items()}
        names = list(out) if out is not None else list(shapes) if fields is None else list(fields)
        unknown = set(names) - set(shapes)
        if unknown:
            raise ValueError("unknown %s field(s) %s" % (noun, sorted(unknown)))
        if out is None:
            out = {name: torch.empty(shapes[name][0], dtype=shapes[name][1], device=self.device) for name in names}
        for name, t in out.items():
            self._check_buf(t, shapes[name][0], shapes[name][1], name)
            setattr(dev, name, t.data_ptr())
        return out

    def _query_rows(self, envs, given, ins):
        """The rows of forward() / rollout(): n = len(envs), else the rows of the first given tensor, else num_envs.  `given`:
        (field of `ins`, tensor or None, shape of one row) triples; every tensor is checked as float64 [n, *shape] (n = -1, which
        no tensor passes, for one without a leading dimension) and its pointer set in `ins`, the entry's ctypes input struct.
        Returns (n, the env index tensor or None: the caller holds it until the launch)."""
        torch = _torch()
        idx, _, n = self._env_index(envs)
        if idx is not None:
            ins.env_index = idx.data_ptr()
        if n is None:
            first = next((t for _, t, _ in given if t is not None), None)
            n = self.num_envs if first is None else (int(first.shape[0]) if isinstance(first, torch.Tensor) and first.dim() else -1)
        for name, t, shape in given:
            if t is not None:
                self._check_buf(t, (n,) + shape, torch.float64, "warm" if name == "qacc_warm" else name)
                setattr(ins, name, t.data_ptr())
        return n, idx

    def pack_action(self, action) -> "object":
        """dict of arrays keyed like the reference action space (env_base.py:151-188) -> flat [N, act_dim].  A dict of
        DEVICE tensors is packed on the device (one strided copy per key into the handle's action buffer: no host
        round trip, no allocation); NumPy / list values go through one host buffer and a single upload."""
        torch = _torch()
        if isinstance(action, dict):
            if any(isinstance(v, torch.Tensor) and v.is_cuda for v in action.values()):
                keys = list(self.cm.act_slices)
                if all(k in action and isinstance(action[k], torch.Tensor) and action[k].is_cuda
                       and action[k].dtype == torch.float32 for k in keys):
                    # the usual case: every key present, on the device -> ONE concatenation kernel into the action buffer
                    torch.cat([action[k].reshape(self.num_envs, -1) for k in keys], dim=1, out=self.act)
                    return self.act
                self.act.zero_()
                for key, sl in self.cm.act_slices.items():
                    if key in action:
                        v = action[key]
                        if not isinstance(v, torch.Tensor):
                            v = torch.as_tensor(np.asarray(v, dtype=np.float32))
                        self.act[:, sl].copy_(v.reshape(self.num_envs, -1), non_blocking=True)
                return self.act
            flat = np.zeros((self.num_envs, self.cm.act_dim), dtype=np.float32)
            for key, sl in self.cm.act_slices.items():
                if key in action:
                    flat[:, sl] = np.asarray(action[key], dtype=np.float32).reshape(self.num_envs, -1)
            return torch.from_numpy(flat).to(self.device)
        if isinstance(action, torch.Tensor):
            return action.to(device=self.device, dtype=torch.float32).reshape(self.num_envs, self.cm.act_dim).contiguous()
        return torch.as_tensor(np.asarray(action, dtype=np.float32).reshape(self.num_envs, self.cm.act_dim),
                               device=self.device)

    # ------------------------------------------------------------------ the seam (k_* methods)
    def k_reset(self, mask=None):
        """KManipEnvSim.k_reset (env_sim.py:190-194): (terminated, reward, discount, observation, sim_time)."""
        torch = _torch()
        mp = None
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            mp = C.c_void_p(mask.data_ptr())
        self._check(self.L.kmanip_reset(self.h, mp, C.c_void_p(self.obs.data_ptr()), self._stream()), "kmanip_reset")
        return self.terminated, None, None, self.obs_dict(), 0.0

    def step_flat(self, act):
        """Raw batched step on device tensors: returns (obs, reward, done) views of the handle's buffers."""
        self._check_buf(act, (self.num_envs, self.cm.act_dim), _torch().float32, "act")
        self._check(self.L.kmanip_step(self.h, C.c_void_p(act.data_ptr()), C.c_void_p(self.obs.data_ptr()),
                                       C.c_void_p(self.reward.data_ptr()), C.c_void_p(self.done.data_ptr()),
                                       self._stream()), "kmanip_step")
        return self.obs, self.reward, self.done

    def bind_reward_done_record(self, rec0=None, rec1=None):
        """kmanip_bind_reward_done_record: every step_flat / k_step then also writes the packed (reward, done) record of the
        multi-GPU exchange (gym_kmanip_amd/dist.py) into rec0 or rec1 -- float64 [num_envs, 2] device tensors; which one is the
        CALLER's choice (select_reward_done_record, rec0 after the bind) -- so that the all-gather needs no packing kernel on the
        step's stream.  None, None unbinds."""
        torch = _torch()
        if (rec0 is None) != (rec1 is None):
            raise _libmod.KManipError("bind_reward_done_record: two buffers or none")
        for t in (rec0, rec1):
            if t is not None:
                self._check_buf(t, (self.num_envs, 2), torch.float64, "record")
        self._rd_rec = (rec0, rec1)                          # (keeps the tensors alive while bound)
        p = [C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0) for t in (rec0, rec1)]
        self._check(self.L.kmanip_bind_reward_done_record(self.h, p[0], p[1]), "kmanip_bind_reward_done_record")

    def bind_applied_force(self, t=None):
        """kmanip_bind_applied_force: MuJoCo's data.qfrc_applied.  `t`: a float64, contiguous [num_envs, nv] tensor on this handle's
        device, row e = env e in the dof order of kinematics()' qM / qfrc_bias: joint torques / forces, then the force on the cube
        (world frame), then the torque on it (cube frame); gym_kmanip_amd.applied has helpers that fill such rows.  While bound,
        every sub-step of step_flat / k_step / step_chunk adds the row to the smooth forces, and forces() reports the forced
        state; the library only ever reads the tensor, once per launch on the step's stream, so writing into it between steps
        is how the force changes.  It is not state (state_tensors, copy_envs_from, checkpoint do not carry it) and resets ignore it.
        Anything but such a tensor raises before the library is called and leaves the binding as it was.  The handle keeps a
        reference; None unbinds (the default kernels again).  Returns `t`."""
        if t is not None:
            self._check_buf(t, (self.num_envs, self.cm.nv), _torch().float64, "applied force")
        self._check(self.L.kmanip_bind_applied_force(self.h, C.c_void_p(t.data_ptr()) if t is not None else None),
                    "kmanip_bind_applied_force")
        self.applied_force = t
        return t

    def new_applied_force(self):
        """Allocate a zero [num_envs, nv] float64 tensor, bind it (bind_applied_force) and return it."""
        return self.bind_applied_force(_torch().zeros((self.num_envs, self.cm.nv), dtype=_torch().float64, device=self.device))

    def select_reward_done_record(self, index: int):
        """kmanip_select_reward_done_record: the bound buffer (0 / 1) the following steps fill.  The caller must have made the
        step's stream wait for whatever still reads that buffer (include/kmanip.h: ordering invariant)."""
        self._check(self.L.kmanip_select_reward_done_record(self.h, int(index)), "kmanip_select_reward_done_record")

    def observe(self, obs=None, reward=None):
        """kmanip_observe: get_observation + get_reward (env_sim.py:110-179) of the CURRENT state, no step; fills and returns
        (self.obs, self.reward) unless other float64 device tensors are given."""
        torch = _torch()
        obs = self.obs if obs is None else obs
        reward = self.reward if reward is None else reward
        self._check_buf(obs, (self.num_envs, self.cm.obs_dim), torch.float64, "obs")
        self._check_buf(reward, (self.num_envs,), torch.float64, "reward")
        self._check(self.L.kmanip_observe(self.h, C.c_void_p(obs.data_ptr()), C.c_void_p(reward.data_ptr()), self._stream()),
                    "kmanip_observe")
        return obs, reward

    # KForcesDev field -> (trailing shape in terms of nv / nu / nc = contact slots, dtype name)
    _FORCE_FIELDS = {"qacc": (("nv",), "float64"), "qfrc_constraint": (("nv",), "float64"), "qfrc_actuator": (("nu",), "float64"),
                     "contact_force": (("nc", 4), "float64"), "contact_bit": (("nc",), "int32"), "contact_frame": (("nc", 9), "float64"),
                     "contact_pos": (("nc", 3), "float64"), "contact_dist": (("nc",), "float64"), "contact_mask": ((), "int32"),
                     "status": ((), "uint8")}

    def forces(self, out=None, fields=None):
        """kmanip_forces: qacc, joint forces and contact forces of every env's CURRENT state (mj_forward with actuation; one launch
        on the current stream, no synchronisation; the handle is only read).  Returns a dict of device tensors:
          qacc, qfrc_constraint [n, nv]; qfrc_actuator [n, nu]; contact_force [n, NC, 4] (normal, tangent 1, tangent 2, torsion in
          the contact frame); contact_bit [n, NC] int32 (KM_CON_* bit index of the pair in the slot, -1 = empty); contact_frame
          [n, NC, 9]; contact_pos [n, NC, 3]; contact_dist [n, NC]; contact_mask [n] int32 (the uint32 mask's bits); status [n] uint8
        NC = model.contact_slots(nlink).  `fields`: the names wanted (default: all); `out`: a dict of such tensors to fill -- only
        the fields it names are computed -- returned as given.  Newton handles only."""
        from .model import contact_slots
        dims = {"nv": self.cm.nv, "nu": self.cm.nu, "nc": contact_slots(self.cm.nlink)}
        fd = _libmod.KForcesDev()
        out = self._query_out(self._FORCE_FIELDS, (self.num_envs,), dims, out, fields, fd, "force")
        self._check(self.L.kmanip_forces(self.h, C.byref(fd), self._stream()), "kmanip_forces")
        return out

    # KInverseDev field -> (trailing shape in terms of nv / nc = contact slots, dtype name)
    _INVERSE_FIELDS = {"qfrc_inverse": (("nv",), "float64"), "qfrc_constraint": (("nv",), "float64"), "contact_force": (("nc", 4), "float64"),
                       "contact_bit": (("nc",), "int32"), "contact_mask": ((), "int32"), "status": ((), "uint8")}

    def inverse(self, qacc, qpos=None, qvel=None, out=None, fields=None):
        """kmanip_inverse: MuJoCo's mj_inverse -- the generalised force that produces the GIVEN acceleration (one launch on the current
        stream, no synchronisation, nothing solved; the handle is only read; either solver).  qacc: float64 [n, nv] in the dof order
        of kinematics()' qM / qfrc_bias; qpos [n, nq] / qvel [n, nv]: the state to evaluate at, None = the handle's (a given one is
        used exactly as set_state_tensors followed by the call would use it, and the handle keeps its own).  Returns a dict of
        device tensors:
          qfrc_inverse [n, nv] = M qacc + qfrc_bias - qfrc_constraint: the total force (servos + applied) behind qacc;
          qfrc_constraint [n, nv] = J^T f(qacc): friction loss, limits and contacts at that acceleration; contact_force [n, NC, 4],
          contact_bit [n, NC] int32, contact_mask [n] int32: as forces(), at that acceleration (normal_by_bit / finger_force work on
          the result); status [n] uint8 (1: non-finite state or qacc, everything else of the env 0, contact_bit -1)
        `fields`: the names wanted (default: all); `out`: a dict of such tensors to fill -- only the fields it names are computed --
        returned as given.  ctrl, the warm start and a bound applied force do not enter; gym_kmanip_amd.applied.from_inverse turns
        the result into rows for bind_applied_force."""
        torch = _torch()
        from .model import contact_slots
        dims = {"nv": self.cm.nv, "nc": contact_slots(self.cm.nlink)}
        iv = _libmod.KInverseIn()
        for name, t, width in (("qacc", qacc, self.cm.nv), ("qpos", qpos, self.cm.nq), ("qvel", qvel, self.cm.nv)):
            if t is not None or name == "qacc":
                self._check_buf(t, (self.num_envs, width), torch.float64, name)
                setattr(iv, name, t.data_ptr())
        od = _libmod.KInverseDev()
        out = self._query_out(self._INVERSE_FIELDS, (self.num_envs,), dims, out, fields, od, "inverse")
        self._check(self.L.kmanip_inverse(self.h, C.byref(iv), C.byref(od), self._stream()), "kmanip_inverse")
        return out

    def forward(self, envs=None, qpos=None, qvel=None, ctrl=None, warm=None, qfrc_applied=None, out=None, fields=None):
        """kmanip_forward: MuJoCo's mj_forward on a scratch mjData -- qacc, joint forces and contact forces at rows the CALLER
        passes, as many as it likes (one launch on the current stream, no synchronisation; the handle is only read, to the bit).
        Row r takes the model parameters (per-env parameters included) of env envs[r] -- an int32 device tensor or anything
        torch.as_tensor takes, repeats allowed, more rows than envs allowed; None = row r is env r, and then at most num_envs
        rows -- and, per field, the caller's row or, for None, what that env stores: qpos [n, nq], qvel [n, nv], ctrl [n, nu]
        (used exactly as given, no float32 rounding), warm [n, nv] (the solver's starting point), qfrc_applied [n, nv] (None:
        the env's row of a bound applied force, none if nothing is bound).  n = len(envs), else the rows of the first given
        tensor, else num_envs.  With everything None it computes what forces() computes.  Returns the dict forces() returns,
        n rows (normal_by_bit / finger_force work on it); status [n] uint8: 0 ok; 1 a non-finite value in an input the row uses,
        given or stored, a failed factorisation or a bad qacc; 2 an env index outside 0 .. num_envs-1 (never used as an
        address; state_index_errors does not count it) -- every other output of such a row is 0 and contact_bit -1.
        `fields`: the names wanted (default: all); `out`: a dict of such tensors to fill -- only the fields it names are
        computed -- returned as given.  Newton handles only."""
        from .model import contact_slots
        fi = _libmod.KForwardIn()
        n, idx = self._query_rows(envs, (("qpos", qpos, (self.cm.nq,)), ("qvel", qvel, (self.cm.nv,)), ("ctrl", ctrl, (self.cm.nu,)),
                                         ("qacc_warm", warm, (self.cm.nv,)), ("qfrc_applied", qfrc_applied, (self.cm.nv,))), fi)
        dims = {"nv": self.cm.nv, "nu": self.cm.nu, "nc": contact_slots(self.cm.nlink)}
        fd = _libmod.KForcesDev()
        out = self._query_out(self._FORCE_FIELDS, (n,), dims, out, fields, fd, "force")
        self._check(self.L.kmanip_forward(self.h, C.byref(fi), n, C.byref(fd), self._stream()), "kmanip_forward")
        return out

    def _stepped_rows(self, what, envs, qpos, qvel, ctrl, warm, qfrc_applied, nstep, nsub, ins, per_step_lengths=()):
        """The rows of rollout() / rollout_feedback(): nstep from the rank-3 tensors (and `per_step_lengths`, further per-step
        lengths of the caller's), else the argument, else 1; every given tensor checked and set in `ins` (_query_rows), the two
        per-step flags with them.  Returns (n, nstep, nsub for the library, the env index tensor or None)."""
        torch = _torch()
        stepped = (("ctrl", ctrl, self.cm.nu), ("qfrc_applied", qfrc_applied, self.cm.nv))
        per_step = {name: isinstance(t, torch.Tensor) and t.dim() == 3 for name, t, _ in stepped}
        lengths = {int(t.shape[1]) for name, t, _ in stepped if per_step[name]} | {int(x) for x in per_step_lengths}
        if nstep is not None:
            lengths.add(int(nstep))
        if len(lengths) > 1:
            raise _libmod.KManipError("%s: nstep and the per-step tensors disagree: %s" % (what, sorted(lengths)))
        nstep = lengths.pop() if lengths else 1
        nsub = 0 if nsub is None else int(nsub)          # (0: the model's n_sub_steps; a negative one is refused by the library)
        given = (("qpos", qpos, (self.cm.nq,)), ("qvel", qvel, (self.cm.nv,)), ("qacc_warm", warm, (self.cm.nv,)))
        given += tuple((name, t, (nstep, width) if per_step[name] else (width,)) for name, t, width in stepped)
        n, idx = self._query_rows(envs, given, ins)
        ins.ctrl_per_step, ins.frc_per_step = int(per_step["ctrl"]), int(per_step["qfrc_applied"])
        return n, nstep, nsub, idx

    # KRolloutDev field -> (trailing shape in terms of nq / nv, or None for the per-row fields, dtype name)
    _ROLLOUT_FIELDS = {"qpos": (("nq",), "float64"), "qvel": (("nv",), "float64"), "qacc_warm": (("nv",), "float64"),
                       "contact_mask": ((), "int32"), "reward": ((), "float64"), "status": (None, "uint8"), "steps_done": (None, "int32")}

    def rollout(self, envs=None, qpos=None, qvel=None, ctrl=None, warm=None, qfrc_applied=None, nstep=None, nsub=None, out=None,
                fields=None):
        """kmanip_rollout: MuJoCo's `rollout` -- open-loop integration in ctrl space from rows the CALLER passes, as many as it likes
        (one launch on the current stream, no synchronisation; the handle is only read, to the bit; the handle's solver).  Rows
        and their None fields as in forward(): row r takes the model parameters of env envs[r] and, per field, the caller's row
        or what that env stores -- qpos [n, nq], qvel [n, nv], warm [n, nv] (the first sub-step's starting point).  ctrl [n, nu]
        is held for all steps, ctrl [n, nstep, nu] gives row (r, t) to step t; it is used exactly as given: no action decode, no
        IK, no CTRL_ALPHA filter, no float32 rounding (the servos' own clamps act).  qfrc_applied [n, nv] / [n, nstep, nv]
        likewise (None: the env's row of a bound applied force, held, none if nothing is bound).  nstep: given by a rank-3
        tensor, else the argument, else 1.  One step is nsub sub-steps (None: the model's n_sub_steps, a control step; 1:
        MuJoCo's mj_step).  Returns a dict of device tensors:
          qpos [n, nstep, nq], qvel, qacc_warm [n, nstep, nv]: the state after each step; contact_mask [n, nstep] int32 (the uint32
          mask's bits) and reward [n, nstep]: of that state, as the step reports them; status [n] uint8: 0 ran all steps; 1 a
          non-finite input the row uses, a failed factorisation, a bad qacc or a non-finite qpos; 2 an env index outside
          0 .. num_envs-1 (never used as an address; state_index_errors does not count it); steps_done [n] int32: the steps
          recorded before the row stopped -- its records from there on are zeros.  A row never resets.
        `fields`: the names wanted (default: all; without contact_mask and reward the kernel skips the kinematics + collision
        pass that feeds them); `out`: a dict of such tensors to fill -- only the fields it names are computed -- returned as
        given."""
        ri = _libmod.KRolloutIn()
        n, nstep, nsub, idx = self._stepped_rows("rollout", envs, qpos, qvel, ctrl, warm, qfrc_applied, nstep, nsub, ri)
        rd = _libmod.KRolloutDev()
        out = self._query_out(self._ROLLOUT_FIELDS, (n, nstep), {"nq": self.cm.nq, "nv": self.cm.nv}, out, fields, rd, "rollout")
        self._check(self.L.kmanip_rollout(self.h, C.byref(ri), n, nstep, nsub, C.byref(rd), self._stream()), "kmanip_rollout")
        return out

    _FEEDBACK_FIELDS = dict(_ROLLOUT_FIELDS, ctrl=(("nu",), "float64"))

    def rollout_feedback(self, envs=None, qpos=None, qvel=None, ctrl=None, warm=None, qfrc_applied=None, gains=None, qpos_ref=None,
                         qvel_ref=None, gain_index=None, nstep=None, nsub=None, out=None, fields=None, gains_t=None, ctrl_lo=None,
                         ctrl_hi=None):
        """kmanip_feedback: rollout() with a per-step affine state feedback evaluated on the device, in the same ONE launch -- the
        policy of an iLQR / DDP backward pass, a regulator, or the stabilising feedback under MPPI samples.  At the START of every
        step t, with (q, v) the row's state there,
          dx = [derivatives.tangent_diff(q, qpos_ref[g, t]) ; v - qvel_ref[g, t]],    u = ctrl[r, t] + gains[g, t] @ dx
        and u acts during step t (unclamped: the servos' own clamps act in the sub-steps).  Rows, their None fields, ctrl /
        qfrc_applied held or per step, nstep and nsub as in rollout(); ctrl is the open-loop term.
          gains [ng, nstep, nu, 2 nv] per step, or [ng, nu, 2 nv] held for all steps (a regulator), in the textbook orientation: the
            library is handed the transposed contiguous copy.  gains_t [ng, nstep, 2 nv, nu] / [ng, 2 nv, nu] in its place skips
            that copy.
          qpos_ref [ng, nstep, nq] / [ng, nq], qvel_ref [ng, nstep, nv] / [ng, nv]: the reference state BEFORE step t, per step or
            held like the gains.  Record t of an earlier rollout is the state AFTER step t, i.e. the reference of step t + 1.
          gain_index: int32 [n], row r follows trajectory gain_index[r] (repeats allowed); None = row r follows trajectory r.
        Returns rollout()'s dict plus ctrl [n, nstep, nu], the u of every step; status 1 also for a non-finite u (steps_done = the
        step it was computed for), status 2 also for a gain index outside 0 .. ng-1 (never used as an address).  With zero gains
        the result is rollout()'s, bit for bit.
        ctrl_lo / ctrl_hi [nu], or [ng, nu] a box per gain trajectory (one of them None: that side is unbounded): kmanip_feedback_box,
        the same launch with u = clip(u, ctrl_lo, ctrl_hi) after the finite-u test -- the clamped u acts and is what `ctrl` records;
        a row whose box has lo <= hi false somewhere (a NaN bound too) gets status 1 and no step.  Both None: kmanip_feedback."""
        torch = _torch()
        if (gains is None) == (gains_t is None):
            raise _libmod.KManipError("rollout_feedback: give gains or gains_t (one of them)")
        if gains is not None:
            if not isinstance(gains, torch.Tensor) or gains.dim() not in (3, 4):
                raise _libmod.KManipError("rollout_feedback: gains must be a [ng, nstep, nu, 2 nv] or [ng, nu, 2 nv] tensor")
            gains_t = gains.transpose(-1, -2).contiguous()
        if not isinstance(gains_t, torch.Tensor) or gains_t.dim() not in (3, 4):
            raise _libmod.KManipError("rollout_feedback: gains_t must be a [ng, nstep, 2 nv, nu] or [ng, 2 nv, nu] tensor")
        per_step = gains_t.dim() == 4
        ng = int(gains_t.shape[0])
        boxed = ctrl_lo is not None or ctrl_hi is not None
        fi = _libmod.KFeedbackBoxIn() if boxed else _libmod.KFeedbackIn()
        n, nstep, nsub, idx = self._stepped_rows("rollout_feedback", envs, qpos, qvel, ctrl, warm, qfrc_applied, nstep, nsub, fi,
                                                 per_step_lengths=(gains_t.shape[1],) if per_step else ())
        lead = (ng, nstep) if per_step else (ng,)
        for name, t, shape in (("gain_t", gains_t, (2 * self.cm.nv, self.cm.nu)), ("qpos_ref", qpos_ref, (self.cm.nq,)),
                               ("qvel_ref", qvel_ref, (self.cm.nv,))):
            self._check_buf(t, lead + shape, torch.float64, "gains" if name == "gain_t" else name)
            setattr(fi, name, t.data_ptr())
        gidx, _, gn = self._env_index(gain_index, "gain_index")
        if gidx is not None:
            if gn != n:
                raise _libmod.KManipError("rollout_feedback: gain_index has %d entries for %d rows" % (gn, n))
            fi.gain_index = gidx.data_ptr()
        fi.ng, fi.gain_per_step = ng, int(per_step)
        fd = _libmod.KFeedbackDev()
        out = self._query_out(self._FEEDBACK_FIELDS, (n, nstep), {"nq": self.cm.nq, "nv": self.cm.nv, "nu": self.cm.nu}, out, fields, fd,
                              "rollout_feedback")
        if boxed:
            box = self._box("rollout_feedback", ctrl_lo, ctrl_hi, ng)
            fi.lo, fi.hi, fi.box_per_traj = box[0].data_ptr(), box[1].data_ptr(), int(box[0].dim() == 2)
            self._check(self.L.kmanip_feedback_box(self.h, C.byref(fi), n, nstep, nsub, C.byref(fd), self._stream()), "kmanip_feedback_box")
            return out
        self._check(self.L.kmanip_feedback(self.h, C.byref(fi), n, nstep, nsub, C.byref(fd), self._stream()), "kmanip_feedback")
        return out

    def _box(self, what, lo, hi, rows):
        """(lo, hi) of a control box as checked float64 device tensors, both [nu] or both [rows, nu]; a None side is -inf / +inf."""
        torch = _torch()
        nu = self.cm.nu
        shape = next(tuple(t.shape) for t in (lo, hi) if isinstance(t, torch.Tensor)) if any(isinstance(t, torch.Tensor) for t in (lo, hi)) else (nu,)
        if shape not in ((nu,), (rows, nu)):
            raise _libmod.KManipError("%s: the box must be [nu] or [%d, nu] tensors, got %s" % (what, rows, shape))
        res = []
        for name, t, fill in (("lo", lo, float("-inf")), ("hi", hi, float("inf"))):
            if t is None:
                t = torch.full(shape, fill, dtype=torch.float64, device=self.device)
            elif not isinstance(t, torch.Tensor):
                t = torch.as_tensor(t, dtype=torch.float64, device=self.device)
            t = t.contiguous()
            self._check_buf(t, shape, torch.float64, "%s: %s" % (what, name))
            res.append(t)
        return tuple(res)

    # KTransFdDev field -> (trailing shape in terms of nq / nv / ncol / nx = 2 nv, dtype name)
    _TRANSFD_FIELDS = {"qpos": (("nq",), "float64"), "qvel": (("nv",), "float64"), "qacc_warm": (("nv",), "float64"),
                       "contact_mask": ((), "int32"), "status": ((), "uint8"), "deriv_t": (("ncol", "nx"), "float64"),
                       "status_cols": (("ncol",), "uint8"), "contact_mask_fd": (("ncol", 2), "int32")}

    def transition_fd(self, envs=None, qpos=None, qvel=None, ctrl=None, qfrc_applied=None, warm=None, nsub=None, eps=1e-6,
                      wrt=("qpos", "qvel", "ctrl"), warm_offset=1.0, out=None):
        """kmanip_transition_fd: derivatives.transition_fd -- MuJoCo's mjd_transitionFD, centred finite differences of ONE step (nsub
        sub-steps; None = the model's) with respect to the inputs named in `wrt` -- in ONE library call of two launches: the nominal
        rows through rollout()'s kernel, then a kernel that perturbs the rows, steps the +eps and -eps copies side by side in one
        wave and writes the quotients.  No perturbed row and no perturbed state reaches memory, and no torch arithmetic runs.
        Rows and their None fields as in rollout(): unlike derivatives.transition_fd a differentiated input may stay None (the named
        env's stored values are then differentiated about).  Per row the arithmetic is derivatives.transition_fd's, operation for
        operation: see there for eps, the warm start (`warm`, warm_offset) and the piecewise-smooth caveat.  Returns its dict:
          qpos [n, nq], qvel [n, nv], qacc_warm [n, nv], contact_mask [n] int32, status [n] uint8      the nominal rows one step on
          A [n, 2 nv, 2 nv] (wrt holds qpos and qvel; else dnext_dqpos / dnext_dqvel [n, 2 nv, nv]), B [n, 2 nv, nu] (ctrl),
          dnext_dfrc [n, 2 nv, nv] (qfrc_applied): TRANSPOSED VIEWS, no copy, of the one buffer the kernel writes, also returned as
          deriv_t [n, ncol, 2 nv] with the columns in the order qpos, qvel, ctrl, qfrc_applied whatever the order of `wrt`
          status_cols [n, ncol] uint8 and status_fd [n] = its largest entry per row (nonzero: the column is zeros, not a derivative)
          contact_mask_fd [ncol, 2, n] int32: the mask after the step of every perturbed row, + then -, columns in `wrt` order
        `out`: a dict of tensors to fill, keyed by the kernel's own outputs (qpos, qvel, qacc_warm, contact_mask, status, deriv_t,
        status_cols, contact_mask_fd [n, ncol, 2]); only the fields it names are computed -- without contact_mask_fd the perturbed
        rows skip the kinematics + collision pass -- plus the two the call cannot do without, which are allocated: deriv_t, and
        qacc_warm when `warm` is None (it is then the warm-start base of the perturbed rows).  A differentiated qfrc_applied left
        None is rows of zeros, as in derivatives.transition_fd (also while a force is bound: pass its rows to differentiate about it)."""
        torch = _torch()
        cm = self.cm
        wrt = tuple(wrt)
        unknown = set(wrt) - set(_libmod.KM_WRT)
        if unknown:
            raise ValueError("unknown wrt name(s) %s" % sorted(unknown))
        if len(set(wrt)) != len(wrt):
            raise ValueError("transition_fd: a name is repeated in wrt %s" % (wrt,))
        width = {"qpos": cm.nv, "qvel": cm.nv, "ctrl": cm.nu, "qfrc_applied": cm.nv}
        order = [name for name in _libmod.KM_WRT if name in wrt]             # the kernel's column order
        ncol = sum(width[name] for name in order)
        fi = _libmod.KTransFdIn()
        given = [("qpos", qpos, (cm.nq,)), ("qvel", qvel, (cm.nv,)), ("qacc_warm", warm, (cm.nv,)), ("ctrl", ctrl, (cm.nu,)),
                 ("qfrc_applied", qfrc_applied, (cm.nv,))]
        n, idx = self._query_rows(envs, given, fi)
        if "qfrc_applied" in wrt and qfrc_applied is None and self.applied_force is not None and n > 0:
            qfrc_applied = torch.zeros((n, cm.nv), dtype=torch.float64, device=self.device)
            fi.qfrc_applied = qfrc_applied.data_ptr()
        fi.wrt, fi.eps, fi.warm_offset = sum(_libmod.KM_WRT[name] for name in order), float(eps), float(warm_offset)
        fd_fields = ("deriv_t", "status_cols", "contact_mask_fd")
        names = list(self._TRANSFD_FIELDS) if out is None else list(out)
        if ncol == 0 or n == 0:              # nothing to differentiate: the nominal rows only, as derivatives.transition_fd returns them
            names = [name for name in names if name not in fd_fields]
        else:
            names += [name for name in ("deriv_t",) + (("qacc_warm",) if warm is None else ()) if name not in names]
        dims = {"nq": cm.nq, "nv": cm.nv, "ncol": ncol, "nx": 2 * cm.nv}
        res = {}
        for name in names:
            if out is not None and name in out:
                res[name] = out[name]
            elif name in self._TRANSFD_FIELDS:
                shp, dt = self._TRANSFD_FIELDS[name]
                res[name] = torch.empty((n,) + tuple(dims[d] if isinstance(d, str) else d for d in shp), dtype=getattr(torch, dt), device=self.device)
            else:
                res[name] = None             # (_query_out names it in its error)
        fd = _libmod.KTransFdDev()
        self._query_out(self._TRANSFD_FIELDS, (n,), dims, res, None, fd, "transition_fd")
        self._check(self.L.kmanip_transition_fd(self.h, C.byref(fi), n, 0 if nsub is None else int(nsub), C.byref(fd), self._stream()),
                    "kmanip_transition_fd")
        if "deriv_t" not in res:
            return res
        d = res["deriv_t"].transpose(1, 2)                                   # [n, 2 nv, ncol], a view
        blocks, c = {}, 0
        for name in order:
            blocks[name] = d[:, :, c:c + width[name]]
            c += width[name]
        if "qpos" in blocks and "qvel" in blocks:
            res["A"] = d[:, :, :2 * cm.nv]
        else:
            for name in ("qpos", "qvel"):
                if name in blocks:
                    res["dnext_d" + name] = blocks[name]
        if "ctrl" in blocks:
            res["B"] = blocks["ctrl"]
        if "qfrc_applied" in blocks:
            res["dnext_dfrc"] = blocks["qfrc_applied"]
        if "status_cols" in res:
            res["status_fd"] = res["status_cols"].amax(dim=1)
        if "contact_mask_fd" in res:
            m = res["contact_mask_fd"]
            if list(wrt) != order:           # the caller's column order
                start = {name: sum(width[o] for o in order[:order.index(name)]) for name in order}
                cols = torch.cat([torch.arange(start[name], start[name] + width[name], device=self.device) for name in wrt])
                m = m[:, cols]
            res["contact_mask_fd"] = m.permute(1, 2, 0)
        return res

    # KParamFdDev field -> (trailing shape in terms of npar / nx = 2 nv, dtype name)
    _PARAMFD_FIELDS = {"deriv_t": (("npar", "nx"), "float64"), "status_cols": (("npar",), "uint8"), "contact_mask_fd": (("npar", 2), "int32")}

    def param_fd(self, envs=None, qpos=None, qvel=None, ctrl=None, qfrc_applied=None, warm=None, params=None, nsub=None, eps=1e-4,
                 relative=True, wrt=ENV_PARAMS, warm_offset=1.0, out=None):
        """kmanip_param_fd: centred finite differences of ONE step (nsub sub-steps; None = the model's) with respect to the per-env
        physics parameters named in `wrt` (model.ENV_PARAMS names), in ONE launch: the + and - rows of a column step side by side in
        one wave with the parameter replaced in the kernel's workspace.  The handle is only read -- its own parameters included --
        and the call works on a handle that never called set_env_params.  Rows and their None fields as in rollout(); warm None is
        the named env's stored warm start (there is no nominal launch), and warm + warm_offset starts both rows' first sub-step, as in
        transition_fd and for its reason.
          params: {name: [n] tensor or scalar} (unnamed: what the row's env has in force) or an [n, KM_EP_N] tensor, the parameters
            the rows are differentiated ABOUT; None: the values in force for the named envs (the compiled model's without any).
          eps: a scalar or {name: value}; relative: e = eps * p_k, else e = eps.  Per column plus = p_k + e, minus = p_k - e and the
            quotient [tangent_diff(qpos+, qpos-) ; qvel+ - qvel-] / (2.0 * e), every operation rounded on its own.
        Returns a dict of device tensors:
          P [n, 2 nv, npar] = d x' / d p, a TRANSPOSED VIEW of deriv_t [n, npar, 2 nv]; the columns in ENV_PARAMS order whatever the
            order of `wrt`, named by the entry wrt (a tuple)
          status_cols [n, npar] uint8 and status_fd [n] = its largest entry per row: 0 a derivative; 1 the + or - row stopped; 2 an
            env index outside the handle; 3 the row's parameters or a perturbed value outside the parameter's limits (the derivative
            in cube_frictionloss AT 0 is refused: its rows exist only above 0).  Nonzero: the column is zeros
          contact_mask_fd [npar, 2, n] int32: the mask after the step of every perturbed row, + then - (transition_fd's layout)
        `out`: a dict of tensors to fill, keyed by the kernel's own outputs (deriv_t, status_cols, contact_mask_fd [n, npar, 2]); only
        the fields it names are computed, plus deriv_t, which is allocated if missing."""
        torch = _torch()
        cm = self.cm
        wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
        unknown = set(wrt) - set(ENV_PARAMS)
        if unknown:
            raise ValueError("unknown env parameter(s) %s (known: %s)" % (sorted(unknown), ", ".join(ENV_PARAMS)))
        if len(set(wrt)) != len(wrt):
            raise ValueError("param_fd: a name is repeated in wrt %s" % (wrt,))
        order = tuple(name for name in ENV_PARAMS if name in wrt)            # the kernel's column order
        npar = len(order)
        fi = _libmod.KParamFdIn()
        given = [("qpos", qpos, (cm.nq,)), ("qvel", qvel, (cm.nv,)), ("qacc_warm", warm, (cm.nv,)), ("ctrl", ctrl, (cm.nu,)),
                 ("qfrc_applied", qfrc_applied, (cm.nv,))]
        n, idx = self._query_rows(envs, given, fi)
        if isinstance(params, dict):
            unknown = set(params) - set(ENV_PARAMS)
            if unknown:
                raise ValueError("unknown env parameter(s) %s (known: %s)" % (sorted(unknown), ", ".join(ENV_PARAMS)))
            cur = self.get_env_params()
            rows = torch.arange(n, device=self.device) if idx is None else idx.long().clamp(0, self.num_envs - 1)
            cols = [cur[name][rows] if params.get(name) is None else
                    torch.as_tensor(params[name], dtype=torch.float64).to(self.device).expand(n) for name in ENV_PARAMS]
            params = torch.stack(cols, dim=1).contiguous()
        if params is not None:
            self._check_buf(params, (n, len(ENV_PARAMS)), torch.float64, "params")
            fi.params = params.data_ptr()
        fi.wrt = sum(1 << ENV_PARAMS.index(name) for name in order)
        for k, name in enumerate(ENV_PARAMS):
            fi.eps[k] = float(eps.get(name, 1e-4) if isinstance(eps, dict) else eps)
        fi.eps_relative, fi.warm_offset = int(bool(relative)), float(warm_offset)
        names = list(self._PARAMFD_FIELDS) if out is None else list(out)
        if "deriv_t" not in names:
            names.append("deriv_t")
        dims = {"npar": npar, "nx": 2 * cm.nv}
        res = {}
        for name in names:
            if out is not None and name in out:
                res[name] = out[name]
            elif name in self._PARAMFD_FIELDS:
                shp, dt = self._PARAMFD_FIELDS[name]
                res[name] = torch.empty((n,) + tuple(dims[d] if isinstance(d, str) else d for d in shp), dtype=getattr(torch, dt), device=self.device)
            else:
                res[name] = None             # (_query_out names it in its error)
        fd = _libmod.KParamFdDev()
        self._query_out(self._PARAMFD_FIELDS, (n,), dims, res, None, fd, "param_fd")
        self._check(self.L.kmanip_param_fd(self.h, C.byref(fi), n, 0 if nsub is None else int(nsub), C.byref(fd), self._stream()),
                    "kmanip_param_fd")
        res["P"] = res["deriv_t"].transpose(1, 2)
        if "status_cols" in res:
            res["status_fd"] = res["status_cols"].amax(dim=1) if npar else torch.zeros((n,), dtype=torch.uint8, device=self.device)
        if "contact_mask_fd" in res:
            res["contact_mask_fd"] = res["contact_mask_fd"].permute(1, 2, 0)
        res["wrt"] = order
        return res

    # KLqrDev field ->(trailing shape in terms of T / nx / nu, or None for the per-problem fields, dtype name)
    _LQR_FIELDS = {"k": (("T", "nu"), "float64"), "gain_t": (("T", "nx", "nu"), "float64"), "dv": ((2,), "float64"),
                   "status": (None, "uint8"), "fail_step": (None, "int32")}

    def _dyn_in(self, what, li, n, T, A, B, deriv_t, ncol=None):
        """The step Jacobians of n problems of T steps set in `li` (a_t, b_t, a_stride, b_stride: KLqrIn's and KAdjointIn's first four
        fields): deriv_t [n, T, ncol, nx] read where it lies (ncol = nx + nu unless the caller allows more columns after them), or A
        and B through one transposed contiguous copy each.  Returns the tensors the caller holds until the launch."""
        torch = _torch()
        nx, nu, f64 = 2 * self.cm.nv, self.cm.nu, torch.float64
        if (deriv_t is None) == (A is None and B is None) or (A is None) != (B is None):
            raise _libmod.KManipError("%s: give deriv_t, or A and B" % what)
        if deriv_t is not None:
            ncol = nx + nu if ncol is None else ncol
            self._check_buf(deriv_t, (n, T, ncol, nx), f64, "deriv_t")
            li.a_t, li.b_t = deriv_t.data_ptr(), deriv_t.data_ptr() + 8 * nx * nx
            li.a_stride = li.b_stride = ncol * nx
            return (deriv_t,)
        for name, t, shape in (("A", A, (n, T, nx, nx)), ("B", B, (n, T, nx, nu))):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise _libmod.KManipError("%s: %s must be a tensor of shape %s" % (what, name, shape))
        a_t, b_t = A.transpose(2, 3).contiguous(), B.transpose(2, 3).contiguous()
        self._check_buf(a_t, (n, T, nx, nx), f64, "A")
        self._check_buf(b_t, (n, T, nu, nx), f64, "B")
        li.a_t, li.b_t, li.a_stride, li.b_stride = a_t.data_ptr(), b_t.data_ptr(), 0, 0
        return (a_t, b_t)

    # KAdjointDev field -> (trailing shape, dtype name); the leading dimension is n m rows
    _ADJOINT_FIELDS = {"lam": (("T1", "nx"), "float64"), "mu": (("T", "nu"), "float64")}

    def adjoint(self, gx, gu=None, A=None, B=None, deriv_t=None, gains=None, gains_t=None, m=1, out=None):
        """kmanip_adjoint: derivatives.adjoint_pass -- the adjoint sweep of a rollout, the gradient of a scalar loss with respect to
        the controls and the initial state -- for n problems of T steps and m cotangent vectors each in ONE launch on the current
        stream, a workgroup per problem with the loop over the steps inside the kernel and each step's Jacobians read once for all
        m vectors (no synchronisation; the handle gives the device and the sizes and is only read).
          gx [n m, T + 1, nx], gu [n m, T, nu] or None (zeros): the loss's direct partials, row e m + j vector j of problem e.
          deriv_t [n, T, ncol >= nx + nu, nx]: transition_fd's buffer, read where it lies (columns after ctrl's are skipped by the
            stride), or A [n, T, nx, nx] and B [n, T, nx, nu], which get one transposed contiguous copy each.
          gains [n, T, nu, nx] (one transposed copy) or gains_t [n, T, nx, nu] (rollout_feedback's, lqr_backward's; no copy), or
            neither: open loop.
        Returns dict(lam [n m, T + 1, nx], mu [n m, T, nu]) by adjoint_pass's recursion; include/kmanip.h KAdjointIn states the
        order of every sum.  `out`: a dict of tensors to fill, keyed lam / mu; only the fields it names are computed."""
        torch = _torch()
        nx, nu, f64 = 2 * self.cm.nv, self.cm.nu, torch.float64
        m = int(m)
        if m < 1:
            raise _libmod.KManipError("adjoint: m must be at least 1")
        if not isinstance(gx, torch.Tensor) or gx.dim() != 3 or gx.shape[0] % m or gx.shape[1] < 1:
            raise _libmod.KManipError("adjoint: gx must be a [n m, T + 1, nx] tensor")
        n, T = int(gx.shape[0]) // m, int(gx.shape[1]) - 1
        ai = _libmod.KAdjointIn()
        ncol = None
        if isinstance(deriv_t, torch.Tensor) and deriv_t.dim() == 4 and deriv_t.shape[2] > nx + nu:
            ncol = int(deriv_t.shape[2])
        keep = self._dyn_in("adjoint", ai, n, T, A, B, deriv_t, ncol=ncol)
        gx = gx.contiguous()
        self._check_buf(gx, (n * m, T + 1, nx), f64, "gx")
        ai.gx = gx.data_ptr()
        keep += (gx,)
        if gu is not None:
            gu = gu.contiguous() if isinstance(gu, torch.Tensor) else gu
            self._check_buf(gu, (n * m, T, nu), f64, "gu")
            ai.gu = gu.data_ptr()
            keep += (gu,)
        if gains is not None and gains_t is not None:
            raise _libmod.KManipError("adjoint: give gains or gains_t, not both")
        if gains is not None:
            if not isinstance(gains, torch.Tensor) or tuple(gains.shape) != (n, T, nu, nx):
                raise _libmod.KManipError("adjoint: gains must be a tensor of shape %s" % ((n, T, nu, nx),))
            gains_t = gains.transpose(2, 3)
        if gains_t is not None:
            gains_t = gains_t.contiguous() if isinstance(gains_t, torch.Tensor) else gains_t
            self._check_buf(gains_t, (n, T, nx, nu), f64, "gains_t")
            ai.gain_t = gains_t.data_ptr()
            keep += (gains_t,)
        ad = _libmod.KAdjointDev()
        res = self._query_out(self._ADJOINT_FIELDS, (n * m,), {"T": T, "T1": T + 1, "nx": nx, "nu": nu}, out, None, ad, "adjoint")
        if n > 0 and T == 0 and "lam" in res:          # (nothing is launched: lam[T] = gx[T] is all there is)
            res["lam"].copy_(gx)
        self._check(self.L.kmanip_adjoint(self.h, C.byref(ai), n, T, m, C.byref(ad), self._stream()), "kmanip_adjoint")
        del keep                             # (the stream orders the launch before the allocator reuses the copies)
        return res

    def _lqr_in(self, what, li, lx, lu, lxx, luu, A, B, deriv_t, reg):
        """The checked inputs of lqr_backward() / lqr_backward_box() set in the KLqrIn `li`.  Returns (n, T, the tensors the caller
        holds until the launch)."""
        torch = _torch()
        nx, nu, f64 = 2 * self.cm.nv, self.cm.nu, torch.float64
        if not isinstance(lu, torch.Tensor) or lu.dim() != 3:
            raise _libmod.KManipError("%s: lu must be a [n, T, nu] tensor" % what)
        n, T = int(lu.shape[0]), int(lu.shape[1])
        keep = self._dyn_in(what, li, n, T, A, B, deriv_t)
        # (the cost's derivatives come as torch made them -- QuadraticCost hands an einsum's strided lx and an expanded luu: a view
        # gets one contiguous copy, everything else about it is checked)
        dense = lambda t: t.contiguous() if isinstance(t, torch.Tensor) else t
        for name, t, shape in (("lx", lx, (n, T + 1, nx)), ("lu", lu, (n, T, nu))):
            t = dense(t)
            self._check_buf(t, shape, f64, name)
            setattr(li, name, t.data_ptr())
            keep += (t,)
        for name, t, shape in (("lxx", lxx, (T + 1, nx, nx)), ("luu", luu, (T, nu, nu))):
            per_env = isinstance(t, torch.Tensor) and t.dim() == 4
            t = dense(t)
            self._check_buf(t, ((n,) if per_env else ()) + shape, f64, name)
            setattr(li, name, t.data_ptr())
            setattr(li, name + "_per_env", int(per_env))
            keep += (t,)
        if isinstance(reg, torch.Tensor) or reg != 0.0:
            reg = torch.as_tensor(reg, dtype=f64, device=self.device)
            reg = (reg.expand(n) if reg.dim() == 0 else reg).contiguous()
            self._check_buf(reg, (n,), f64, "reg")
            li.reg = reg.data_ptr()
            keep += (reg,)
        return n, T, keep

    _LQR_BOX_FIELDS = dict(_LQR_FIELDS, clamped=(("T",), "int32"), qp_iters=(("T",), "int32"))

    def lqr_backward_box(self, lx, lu, lxx, luu, u, lo, hi, A=None, B=None, deriv_t=None, reg=0.0, out=None):
        """kmanip_lqr_backward_box: ilqr.backward_pass_box -- the backward pass of control-limited DDP -- for n problems of T steps in
        ONE launch: lqr_backward() with the box lo <= u + du <= hi on the controls, a projected-Newton box QP per step inside the
        kernel (include/kmanip.h KLqrBoxIn states the iteration and its scale-free termination rule).  lqr_backward()'s arguments,
        and u [n, T, nu] the nominal controls; lo, hi [nu] shared or [n, nu] per problem (None or +-inf: unbounded on that side).
        Returns lqr_backward()'s dict plus clamped [n, T] int32 (the uint32 mask's bits: bit i set where actuator i ended the
        step's QP on a bound -- those rows of K are exact zeros) and qp_iters [n, T] int32.  status: 1 also for a box with lo <= hi
        false somewhere (a NaN bound, a non-finite u), 3 for a QP that hit its iteration cap; such a problem's outputs are zeros.
        `out`: as in lqr_backward(), keyed by k, gain_t, dv, status, fail_step, clamped, qp_iters."""
        torch = _torch()
        nx, nu = 2 * self.cm.nv, self.cm.nu
        li = _libmod.KLqrBoxIn()
        n, T, keep = self._lqr_in("lqr_backward_box", li.lqr, lx, lu, lxx, luu, A, B, deriv_t, reg)
        u = u.contiguous() if isinstance(u, torch.Tensor) else u
        self._check_buf(u, (n, T, nu), torch.float64, "u")
        box = self._box("lqr_backward_box", lo, hi, n)
        li.u, li.lo, li.hi, li.box_per_env = u.data_ptr(), box[0].data_ptr(), box[1].data_ptr(), int(box[0].dim() == 2)
        keep += (u,) + box
        table = self._LQR_BOX_FIELDS
        if out is not None and set(out) - set(table):
            raise ValueError("unknown lqr_backward_box field(s) %s" % sorted(set(out) - set(table)))
        dims = {"T": T, "nx": nx, "nu": nu}
        res = {name: out[name] if out is not None and name in out else
               torch.empty((n,) + (() if shp is None else tuple(dims.get(d, d) for d in shp)), dtype=getattr(torch, dt), device=self.device)
               for name, (shp, dt) in table.items()}
        if n == 0 or T == 0:                 # (nothing is launched: what a problem of no steps gives)
            for name in ("k", "gain_t", "dv", "status", "clamped", "qp_iters"):
                res[name].zero_()
            res["fail_step"].fill_(-1)
        ld = _libmod.KLqrBoxDev()
        for name, t in res.items():
            shp, dt = table[name]
            self._check_buf(t, (n,) + (() if shp is None else tuple(dims.get(d, d) for d in shp)), getattr(torch, dt), name)
            setattr(ld if name in ("clamped", "qp_iters") else ld.lqr, name, t.data_ptr())
        self._check(self.L.kmanip_lqr_backward_box(self.h, C.byref(li), n, T, C.byref(ld), self._stream()), "kmanip_lqr_backward_box")
        del keep                             # (the stream orders the launch before the allocator reuses the copies)
        return {"k": res["k"], "gains_t": res["gain_t"], "K": res["gain_t"].transpose(2, 3), "dV": res["dv"], "status": res["status"],
                "fail_step": res["fail_step"], "clamped": res["clamped"], "qp_iters": res["qp_iters"]}

    def lqr_backward(self, lx, lu, lxx, luu, A=None, B=None, deriv_t=None, reg=0.0, out=None):
        """kmanip_lqr_backward: ilqr.backward_pass -- the Riccati recursion of iLQR -- for n problems of T steps in ONE launch on the
        current stream, a workgroup per problem with the loop over the steps inside the kernel (no synchronisation; the handle gives
        the device and the sizes nx = 2 nv, nu, and is only read; n has nothing to do with num_envs).
          deriv_t [n, T, nx + nu, nx]: transition_fd's buffer over the n T rows e T + t with the default wrt, read where it lies (no
            copy), or A [n, T, nx, nx] and B [n, T, nx, nu], which get one transposed contiguous copy each.
          lx [n, T + 1, nx], lu [n, T, nu]; lxx [n, T + 1, nx, nx] or [T + 1, nx, nx] shared by the problems, luu [n, T, nu, nu] or
            [T, nu, nu]; entry T of lx / lxx is the final cost's.  reg: a number or [n], added to the diagonal of Quu for the solve.
        Returns a dict: k [n, T, nu]; gains_t [n, T, nx, nu], what rollout_feedback(gains_t=...) takes; K [n, T, nu, nx], its
        transposed view; dV [n, 2]; status [n] uint8 and fail_step [n] int32 -- 0 and -1, or 1 and the step at which Quu + reg I
        had a Cholesky pivot that was not positive and finite: that problem's k, gains_t and dV are then zeros, all steps.
        `out`: a dict of tensors to fill, keyed by the kernel's outputs (k, gain_t, dv, status, fail_step); the others are allocated."""
        torch = _torch()
        nx, nu = 2 * self.cm.nv, self.cm.nu
        li = _libmod.KLqrIn()
        n, T, keep = self._lqr_in("lqr_backward", li, lx, lu, lxx, luu, A, B, deriv_t, reg)
        if out is not None and set(out) - set(self._LQR_FIELDS):
            raise ValueError("unknown lqr_backward field(s) %s" % sorted(set(out) - set(self._LQR_FIELDS)))
        ld = _libmod.KLqrDev()
        res = {name: out[name] if out is not None and name in out else
               torch.empty((n,) + (() if shp is None else tuple({"T": T, "nx": nx, "nu": nu}.get(d, d) for d in shp)), dtype=getattr(torch, dt),
                           device=self.device) for name, (shp, dt) in self._LQR_FIELDS.items()}
        if n == 0 or T == 0:                 # (nothing is launched: what a problem of no steps gives)
            for name in ("k", "gain_t", "dv", "status"):
                res[name].zero_()
            res["fail_step"].fill_(-1)
        self._query_out(self._LQR_FIELDS, (n,), {"T": T, "nx": nx, "nu": nu}, res, None, ld, "lqr_backward")
        self._check(self.L.kmanip_lqr_backward(self.h, C.byref(li), n, T, C.byref(ld), self._stream()), "kmanip_lqr_backward")
        del keep                             # (the stream orders the launch before the allocator reuses the copies)
        return {"k": res["k"], "gains_t": res["gain_t"], "K": res["gain_t"].transpose(2, 3), "dV": res["dv"], "status": res["status"],
                "fail_step": res["fail_step"]}

    def normal_by_bit(self, f):
        """[n, 32] float64: the normal force of the contact at each KM_CON_* mask bit of a forces() / forward() / inverse() result
        (it needs contact_force and contact_bit; n = the result's rows), 0 where the bit is clear.  Device-side indexing only: no
        further C call."""
        torch = _torch()
        bit = f["contact_bit"].to(torch.int64)
        normal = torch.where(bit >= 0, f["contact_force"][:, :, 0], torch.zeros((), dtype=torch.float64, device=bit.device))
        out = torch.zeros((bit.shape[0], 32), dtype=torch.float64, device=bit.device)
        return out.scatter_add_(1, bit.clamp(min=0), normal)

    def finger_force(self, f):
        """[n, 2 * narm] float64: normal force of each finger sphere on the cube (the bits of KM_CON_FINGERS_CUBE) of a forces() /
        forward() result."""
        return self.normal_by_bit(f)[:, 8:8 + 2 * (self.cm.nlink // 10)]

    # KKinDev field -> (trailing shape in terms of nl = links, nv, na = KM_MAX_ARMS, dtype name)
    _KIN_FIELDS = {"link_xpos": (("nl", 3), "float64"), "link_xmat": (("nl", 9), "float64"), "site_xpos": (("na", 3), "float64"),
                   "site_xmat": (("na", 9), "float64"), "site_jacp": (("na", 3, "nv"), "float64"), "site_jacr": (("na", 3, "nv"), "float64"),
                   "site_vel": (("na", 6), "float64"), "qM": (("nv", "nv"), "float64"), "qfrc_bias": (("nv",), "float64"),
                   "status": ((), "uint8")}

    def kinematics(self, out=None, fields=None):
        """kmanip_kinematics: link and site poses, site Jacobians, joint-space inertia and bias forces of every env's CURRENT state
        (one launch on the current stream, no synchronisation; the handle is only read; either solver).  Returns a dict of device
        tensors:
          link_xpos [n, nlink, 3], link_xmat [n, nlink, 9] (MuJoCo's data.xpos / data.xmat of the link bodies); site_xpos [n, 2, 3],
          site_xmat [n, 2, 9] (arm 0 = right; an absent arm: zeros); site_jacp, site_jacr [n, 2, 3, nv] (mj_jacSite, all nv columns);
          site_vel [n, 2, 6] (jacp qvel, jacr qvel); qM [n, nv, nv] (mj_fullM, cube block diag(m, m, m, I)); qfrc_bias [n, nv];
          status [n] uint8 (1: non-finite state, everything else of the env 0)
        `fields`: the names wanted (default: all); `out`: a dict of such tensors to fill -- only the fields it names are computed --
        returned as given."""
        dims = {"nl": self.cm.nlink, "nv": self.cm.nv, "na": 2}
        kd = _libmod.KKinDev()
        out = self._query_out(self._KIN_FIELDS, (self.num_envs,), dims, out, fields, kd, "kinematics")
        self._check(self.L.kmanip_kinematics(self.h, C.byref(kd), self._stream()), "kmanip_kinematics")
        return out

    def kinematics_at(self, envs=None, qpos=None, qvel=None, out=None, fields=None):
        """kmanip_kinematics_rows: kinematics() at rows the CALLER passes, as many as it likes -- the states of a nominal trajectory,
        the rows of a line search (one launch on the current stream, no synchronisation; the handle is only read; either solver).
        Row r takes the per-env parameters of env envs[r] (forward()'s rules: repeats allowed, more rows than envs allowed; None =
        row r is env r, and then at most num_envs rows) and the caller's row of qpos [n, nq] / qvel [n, nv] or, for None, what that
        env stores.  n = len(envs), else the rows of the first given tensor, else num_envs.  With everything None it returns
        kinematics()' bits.  Returns kinematics()' dict with n leading rows; status [n] uint8: 0 ok; 1 a non-finite qpos or qvel the
        row uses, given or stored; 2 an env index outside 0 .. num_envs-1 (never used as an address) -- every other output of such a
        row is 0.  `fields`, `out`: as in kinematics(); without qM and qfrc_bias the kernel stops after the forward kinematics, and
        the other fields' bits are the same."""
        ki = _libmod.KKinRowsIn()
        n, idx = self._query_rows(envs, (("qpos", qpos, (self.cm.nq,)), ("qvel", qvel, (self.cm.nv,))), ki)
        dims = {"nl": self.cm.nlink, "nv": self.cm.nv, "na": 2}
        kd = _libmod.KKinDev()
        out = self._query_out(self._KIN_FIELDS, (n,), dims, out, fields, kd, "kinematics")
        self._check(self.L.kmanip_kinematics_rows(self.h, C.byref(ki), n, C.byref(kd), self._stream()), "kmanip_kinematics_rows")
        return out

    # KSiteCostDev field -> (trailing shape in terms of nx = 2 nv, na = KM_MAX_ARMS, dtype name)
    _SITE_COST_FIELDS = {"cost": ((), "float64"), "lx": (("nx",), "float64"), "lxx": (("nx", "nx"), "float64"),
                         "site_xpos": (("na", 3), "float64"), "resid": (("na", 6), "float64"), "status": ((), "uint8")}

    def site_cost(self, target_pos, weight, envs=None, qpos=None, target_quat=None, follow_cube=(False, False), out=None, fields=None):
        """kmanip_site_cost: a site-pose cost of n rows of states, its gradient and Gauss-Newton Hessian in ONE launch (the handle is
        only read; either solver).  Per row r, over the present arms a, in transition_fd's tangent x = [dq ; qvel], nx = 2 nv:
          e_pos = site_xpos - (target_pos[r, a] + follow_cube[a] * cube position); e_rot = the world-frame rotation vector (|.| <= pi)
          of R_site R_target^T, R_target from target_quat[r, a] (wxyz, normalised; read only where weight[r, a, 1] != 0)
          cost = 1/2 sum_a (weight[r, a, 0] |e_pos|^2 + weight[r, a, 1] |e_rot|^2); lx = sum_a (w0 Jp' e_pos + w1 Jr' e_rot) with Jp =
          site_jacp and -follow_cube[a] I on the cube's position columns, Jr = site_jacr; lxx = sum_a (w0 Jp' Jp + w1 Jr' Jr)
        target_pos [n, 2, 3] and weight [n, 2, 2] float64, required; target_quat [n, 2, 4] or None (no rotation term); envs, qpos:
        kinematics_at()'s rows; qvel does not enter.  follow_cube: a bool, or one per arm.  Returns a dict of device tensors:
          cost [n]; lx [n, nx] (exact zeros from nv on); lxx [n, nx, nx] (bitwise symmetric, exact zeros outside the nv x nv block);
          site_xpos [n, 2, 3]; resid [n, 2, 6] (e_pos, e_rot); status [n] uint8: 0 ok; 1 a non-finite qpos the row uses, or a
          non-finite target or weight of a present arm; 2 an env index out of range -- every other output of such a row is 0
        `fields`: the names wanted (default: all); `out`: a dict of such tensors to fill, returned as given."""
        si = _libmod.KSiteCostIn()
        n, idx = self._query_rows(envs, (("qpos", qpos, (self.cm.nq,)), ("target_pos", target_pos, (2, 3)), ("weight", weight, (2, 2)),
                                         ("target_quat", target_quat, (2, 4))), si)
        fc = (follow_cube, follow_cube) if isinstance(follow_cube, (bool, int)) else tuple(follow_cube)
        si.follow_cube[0], si.follow_cube[1] = int(bool(fc[0])), int(bool(fc[1]))
        sd = _libmod.KSiteCostDev()
        out = self._query_out(self._SITE_COST_FIELDS, (n,), {"nx": 2 * self.cm.nv, "na": 2}, out, fields, sd, "site cost")
        self._check(self.L.kmanip_site_cost(self.h, C.byref(si), n, C.byref(sd), self._stream()), "kmanip_site_cost")
        return out

    def site_jacobian(self, k, arm):
        """[n, 6, nv] float64: the 6 x nv site Jacobian of `arm` (0 = right) from a kinematics() result (it needs site_jacp and
        site_jacr), jacp over jacr: one cat, no further C call."""
        return _torch().cat((k["site_jacp"][:, arm], k["site_jacr"][:, arm]), dim=1)

    def step_chunk(self, acts, obs=None, reward=None, done=None):
        """K control steps in one launch (kmanip_step_chunk): acts float32 [K, num_envs, act_dim] on the device ->
        (obs [K, N, obs_dim] f64, reward [K, N] f64, done [K, N] u8).  Same results as K step_flat calls; self.obs /
        self.reward / self.done are left holding the last step."""
        torch = _torch()
        K = int(acts.shape[0])
        n = self.num_envs
        self._check_buf(acts, (K, n, self.cm.act_dim), torch.float32, "acts")
        for t, shp, dt, nm in ((obs, (K, n, self.cm.obs_dim), torch.float64, "obs"), (reward, (K, n), torch.float64, "reward"),
                               (done, (K, n), torch.uint8, "done")):
            if t is not None:
                self._check_buf(t, shp, dt, nm)
        if obs is None:
            obs = torch.empty((K, n, self.cm.obs_dim), dtype=torch.float64, device=self.device)
        if reward is None:
            reward = torch.empty((K, n), dtype=torch.float64, device=self.device)
        if done is None:
            done = torch.empty((K, n), dtype=torch.uint8, device=self.device)
        self._check(self.L.kmanip_step_chunk(self.h, K, C.c_void_p(acts.data_ptr()), C.c_void_p(obs.data_ptr()),
                                             C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()), self._stream()),
                    "kmanip_step_chunk")
        self.obs.copy_(obs[-1]); self.reward.copy_(reward[-1]); self.done.copy_(done[-1])
        return obs, reward, done

    def k_step(self, action):
        """KManipEnvSim.k_step (env_sim.py:196-200).  `terminated` is always False in the reference
        (get_termination -> None); the TimeLimit truncation and the divergence flag are in `self.done`.
        ALIASING: the returned reward / terminated / sim_time tensors and the observation dict's values are the handle's live
        device buffers (views of self.obs), overwritten in place by the next step -- clone() what goes into a rollout list or
        a replay buffer."""
        torch = _torch()
        act = self.pack_action(action)
        self.last_act = act                      # the flat float32 row this step ran on (episode loggers read it)
        self.step_flat(act)
        # sim_time = data.time of each env (env_sim.py:194,200) = steps since its last reset x control_timestep: the step
        # kernel itself fills the bound device buffer -- no extra launch, no host synchronisation
        return self.terminated, self.reward, self.discount, self.obs_dict(), self.sim_time

    def _cam_index(self, cam):
        name = getattr(cam, "name", cam)
        if name not in KM_CAM_INDEX or not self.cm.desc.cam_present[KM_CAM_INDEX[name]]:
            have = [n for n, i in KM_CAM_INDEX.items() if self.cm.desc.cam_present[i]]
            raise _libmod.KManipError("no camera %r in this model; cameras: %s" % (name, ", ".join(have)))
        return KM_CAM_INDEX[name]

    def render_depth(self, cam="grip_r", height: int = 64, width: int = 64, out=None):
        """float32 depth image [num_envs, height, width] (metres along the optical axis) of every env's current state
        -- BASELINE.json config 5's observation (camera branch of env_sim.py:140-145).  Draws the link capsules of
        set_render_links only while set_depth_links is on."""
        torch = _torch()
        ci = self._cam_index(cam)
        if out is None:
            out = torch.empty((self.num_envs, height, width), dtype=torch.float32, device=self.device)
        else:
            self._check_buf(out, (self.num_envs, height, width), torch.float32, "depth")
        self._check(self.L.kmanip_render_depth(self.h, ci, height, width, C.c_void_p(out.data_ptr()), self._stream()),
                    "kmanip_render_depth")
        return out

    def render_rgb(self, cam="top", height=None, width=None, out=None):
        """uint8 RGB image [num_envs, height, width, 3] -- what physics.render(height, width, camera_id) returns in the
        reference (env_sim.py:141-145,187-188).  Size defaults to the camera's reference resolution (__init__.py:157-161)."""
        torch = _torch()
        ci = self._cam_index(cam)
        spec = CAMERAS[getattr(cam, "name", cam)]
        height = spec.h if height is None else height
        width = spec.w if width is None else width
        if out is None:
            out = torch.empty((self.num_envs, height, width, 3), dtype=torch.uint8, device=self.device)
        else:
            self._check_buf(out, (self.num_envs, height, width, 3), torch.uint8, "rgb")
        self._check(self.L.kmanip_render_rgb(self.h, ci, height, width, C.c_void_p(out.data_ptr()), self._stream()),
                    "kmanip_render_rgb")
        return out

    def render_seg(self, cam="top", height=None, width=None, out=None):
        """uint8 segmentation labels [num_envs, height, width] of the camera's ray cast (kmanip_render_seg): KM_SEG_* values --
        0 background, 1 table, 2 cube, 3 / 4 the right / left arm's finger spheres and, while a capsule list is set
        (set_render_links), that arm's link capsules.  Size defaults as in render_rgb."""
        torch = _torch()
        ci = self._cam_index(cam)
        spec = CAMERAS[getattr(cam, "name", cam)]
        height = spec.h if height is None else height
        width = spec.w if width is None else width
        if out is None:
            out = torch.empty((self.num_envs, height, width), dtype=torch.uint8, device=self.device)
        else:
            self._check_buf(out, (self.num_envs, height, width), torch.uint8, "segmentation")
        self._check(self.L.kmanip_render_seg(self.h, ci, height, width, C.c_void_p(out.data_ptr()), self._stream()),
                    "kmanip_render_seg")
        return out

    def render_cameras(self, cams=None, out=None, segmentation: bool = False):
        """Every camera of the observation (default: this id's `cameras`, head first) at its reference resolution in ONE launch
        (kmanip_render_rgb_multi): {name: uint8 [num_envs, h, w, 3]}.  `out` = such a dict of buffers to fill.
        segmentation=True: the same launch (kmanip_render_labels_multi) also fills "segmentation/<name>": uint8 [num_envs, h, w]
        labels (render_seg); `out` may supply those buffers too."""
        torch = _torch()
        names = [getattr(c, "name", c) for c in (self.cm.cameras if cams is None else cams)]
        if not names:
            return {}
        if segmentation:
            return self._render_cameras_labels(names, out)
        bufs = {}
        for nm in names:
            spec = CAMERAS[nm]
            t = None if out is None else out[nm]
            if t is None:
                t = torch.empty((self.num_envs, spec.h, spec.w, 3), dtype=torch.uint8, device=self.device)
            else:
                self._check_buf(t, (self.num_envs, spec.h, spec.w, 3), torch.uint8, "rgb")
            bufs[nm] = t
        n = len(names)
        ci = (C.c_int32 * n)(*[self._cam_index(nm) for nm in names])
        hh = (C.c_int32 * n)(*[CAMERAS[nm].h for nm in names])
        ww = (C.c_int32 * n)(*[CAMERAS[nm].w for nm in names])
        pp = (C.c_void_p * n)(*[bufs[nm].data_ptr() for nm in names])
        self._check(self.L.kmanip_render_rgb_multi(self.h, n, ci, hh, ww, pp, self._stream()), "kmanip_render_rgb_multi")
        return bufs

    def _render_cameras_labels(self, names, out):
        torch = _torch()
        bufs = {}
        for prefix, tail, what in (("", (3,), "rgb"), ("segmentation/", (), "segmentation")):
            for nm in names:
                spec = CAMERAS[nm]
                shape = (self.num_envs, spec.h, spec.w) + tail
                t = None if out is None else out.get(prefix + nm)
                if t is None:
                    t = torch.empty(shape, dtype=torch.uint8, device=self.device)
                else:
                    self._check_buf(t, shape, torch.uint8, what)
                bufs[prefix + nm] = t
        n = len(names)
        ci = (C.c_int32 * n)(*[self._cam_index(nm) for nm in names])
        hh = (C.c_int32 * n)(*[CAMERAS[nm].h for nm in names])
        ww = (C.c_int32 * n)(*[CAMERAS[nm].w for nm in names])
        pp = (C.c_void_p * n)(*[bufs[nm].data_ptr() for nm in names])
        ss = (C.c_void_p * n)(*[bufs["segmentation/" + nm].data_ptr() for nm in names])
        self._check(self.L.kmanip_render_labels_multi(self.h, n, ci, hh, ww, pp, ss, self._stream()), "kmanip_render_labels_multi")
        return bufs

    def camera_poses(self, cam="head", out=None):
        """Camera `cam`'s pose in every env (kmanip_get_camera_poses): {"pos": [n, 3], "mat": [n, 3, 3]} float64 device tensors,
        views of one [n, 12] buffer (`out`, if given).  MuJoCo's cam_xpos / cam_xmat as the renders build them: the COLUMNS of
        `mat` are the camera's x (right), y (up) and z axes in the world frame, and the camera looks along -z; a camera-frame
        point p_c of render_points is the world point pos + mat @ p_c.  Follows set_render_source and the per-env camera offset
        of the visual parameters as render_depth does."""
        torch = _torch()
        ci = self._cam_index(cam)
        if out is None:
            out = torch.empty((self.num_envs, 12), dtype=torch.float64, device=self.device)
        else:
            self._check_buf(out, (self.num_envs, 12), torch.float64, "camera poses")
        self._check(self.L.kmanip_get_camera_poses(self.h, ci, C.c_void_p(out.data_ptr()), self._stream()), "kmanip_get_camera_poses")
        return {"pos": out[:, :3], "mat": out[:, 3:].view(self.num_envs, 3, 3)}

    def camera_intrinsics(self, cam="head", height=None, width=None) -> dict:
        """Pinhole intrinsics of a height x width image of `cam` (default: the camera's reference resolution), host arithmetic
        from the compiled model (model.camera_intrinsics): {"f", "cx", "cy", "fovy"} with f = (height / 2) / tan(fovy / 2) in
        pixels, cx = width / 2, cy = height / 2, fovy in degrees.  Pixel convention of every render here: pixel (r, c) is the ray
        through the pixel's centre, dx = (c + 0.5 - cx) / f to the right and dy = -(r + 0.5 - cy) / f upwards, direction
        x dx + y dy - z in the camera's axes (camera_poses); a depth D (render_depth: metres along the optical axis) is the
        camera-frame point (D dx, D dy, -D)."""
        self._cam_index(cam)
        try:
            return camera_intrinsics(self.cm, cam, height, width)
        except ValueError as e:
            raise _libmod.KManipError(str(e)) from None

    def render_points(self, cam="grip_r", height: int = 64, width: int = 64, frame="world", out=None, depth_out=None):
        """Point cloud float32 [num_envs, height, width, 3] of the camera's depth image (kmanip_render_points): the
        back-projection of what render_depth draws on this handle now (the link capsules only while set_depth_links is on), by
        the same float64 ray cast, in the "world" frame or the "camera" frame (camera_intrinsics has the pixel convention,
        camera_poses the frame).  depth_out: a float32 [num_envs, height, width] tensor that the same launch fills with the
        depth image.  A pixel without a hit is the point on the far plane: mask with depth >= cm.desc.cam_zfar."""
        torch = _torch()
        ci = self._cam_index(cam)
        if frame not in _libmod.KM_POINTS_FRAMES:
            raise _libmod.KManipError("render_points: frame must be 'world' or 'camera', got %r" % (frame,))
        if out is None:
            out = torch.empty((self.num_envs, height, width, 3), dtype=torch.float32, device=self.device)
        else:
            self._check_buf(out, (self.num_envs, height, width, 3), torch.float32, "points")
        dp = None
        if depth_out is not None:
            self._check_buf(depth_out, (self.num_envs, height, width), torch.float32, "depth")
            dp = C.c_void_p(depth_out.data_ptr())
        self._check(self.L.kmanip_render_points(self.h, ci, height, width, _libmod.KM_POINTS_FRAMES[frame], C.c_void_p(out.data_ptr()), dp,
                                                self._stream()), "kmanip_render_points")
        return out

    def set_render_links(self, caps=True):
        """Draw the arm links as capsules in every RGB and label render of this handle (kmanip_set_render_links; depth renders
        draw them only after set_depth_links).  True: the model's default list (model.link_capsules); a list of dicts with the fields of KLinkCapsule
        (link, label, cam_mask, p0, seg, radius) or of tuples in that order: that list; None / False / an empty list: no
        capsules, the default kernels again.  Synchronous.  A bad list raises and leaves the list in force unchanged."""
        if caps is None or caps is False:
            caps = []
        elif caps is True:
            caps = link_capsules(self.cm)
        try:
            caps = check_link_capsules(self.cm, caps)
        except ValueError as e:
            raise _libmod.KManipError("set_render_links: %s" % e) from None
        arr = (_libmod.KLinkCapsule * max(len(caps), 1))()
        for a, c in zip(arr, caps):
            a.link, a.label, a.cam_mask, a.radius = c["link"], c["label"], c["cam_mask"], c["radius"]
            a.p0[:] = c["p0"]
            a.seg[:] = c["seg"]
        self._check(self.L.kmanip_set_render_links(self.h, len(caps), arr if caps else None), "kmanip_set_render_links")

    def get_render_links(self) -> list:
        """The capsule list in force (kmanip_get_render_links), as set_render_links takes it; [] without one."""
        arr = (_libmod.KLinkCapsule * _libmod.KM_MAX_LINK_CAPSULES)()
        n = C.c_int(0)
        self._check(self.L.kmanip_get_render_links(self.h, C.byref(n), arr), "kmanip_get_render_links")
        return [{"link": a.link, "label": a.label, "cam_mask": a.cam_mask, "p0": tuple(a.p0), "seg": tuple(a.seg), "radius": a.radius}
                for a in arr[:n.value]]

    def set_depth_links(self, on=True):
        """render_depth and the in-step render of bind_step_depth draw the capsule list of set_render_links too
        (kmanip_set_depth_links): the float64 depth ray cast with the capsules, so that depth, RGB and labels show one scene.
        A flag of its own, off by default and kept across changes of the list; with the flag off or no list set the depth
        renders are exactly the default ones.  Synchronous."""
        self._check(self.L.kmanip_set_depth_links(self.h, 1 if on else 0), "kmanip_set_depth_links")

    def get_depth_links(self) -> bool:
        """Whether depth renders draw the capsule list (kmanip_get_depth_links)."""
        on = C.c_int(0)
        self._check(self.L.kmanip_get_depth_links(self.h, C.byref(on)), "kmanip_get_depth_links")
        return bool(on.value)

    def snapshot_render_state(self, slot: int):
        """Copy qpos -- all a render reads of the state -- into snapshot `slot` (0 / 1) on the current stream
        (kmanip_snapshot_render_state); `set_render_source(slot)` then points the render_* calls at it."""
        self._check(self.L.kmanip_snapshot_render_state(self.h, int(slot), self._stream()), "kmanip_snapshot_render_state")

    def set_render_source(self, slot: int = -1):
        """-1: the render_* calls read the live state (default); 0 / 1: that snapshot (pipeline.RenderBehind)."""
        self._check(self.L.kmanip_set_render_source(self.h, int(slot)), "kmanip_set_render_source")

    def bind_step_depth(self, cam="grip_r", height: int = 64, width: int = 64, out=None):
        """BASELINE config 5: every step_flat / k_step from now on also renders `cam` into the returned buffer
        (float32 [num_envs, height, width]), in the same C call.  bind_step_depth(None) unbinds.  With set_depth_links on and a
        capsule list set, that render draws the capsules, as render_depth does."""
        torch = _torch()
        if cam is None:
            self._check(self.L.kmanip_bind_step_depth(self.h, 0, 0, 0, None), "kmanip_bind_step_depth")
            self.step_depth = None
            return None
        if out is None:
            out = torch.empty((self.num_envs, height, width), dtype=torch.float32, device=self.device)
        self._check_buf(out, (self.num_envs, height, width), torch.float32, "depth")
        self._check(self.L.kmanip_bind_step_depth(self.h, self._cam_index(cam), height, width, C.c_void_p(out.data_ptr())),
                    "kmanip_bind_step_depth")
        self.step_depth = out                     # keeps the buffer alive while it is bound
        return out

    def scripted_action(self, act=None, generator=None):
        """The reference's synthetic-data policy (examples/2_synthetic_data.py:28-41) for every env, on device:
        action_space.sample() with eer_pos replaced by the unit vector from the right EE site to the cube.
        `act` (float32 [num_envs, act_dim] on the device) is filled with U(-1, 1) when None; returns it."""
        torch = _torch()
        if act is None:
            act = torch.rand((self.num_envs, self.cm.act_dim), device=self.device, generator=generator) * 2 - 1
        self._check(self.L.kmanip_scripted_action(self.h, C.c_void_p(act.data_ptr()), self._stream()), "kmanip_scripted_action")
        return act

    def sample_action(self, act=None, ahead=0):
        """action_space.sample() for every env on the device (examples/2_log_with_h5py.py:22-26): U[-1, 1) float32 from the
        counter-based stream keyed (seed; global env id, episode, step) -- identical to the CPU oracle's.  `ahead`: the action
        the env needs that many control steps from now (TimeLimit-only episodes).  Returns the [num_envs, act_dim] tensor."""
        torch = _torch()
        if act is None:
            act = torch.empty((self.num_envs, self.cm.act_dim), dtype=torch.float32, device=self.device)
        self._check_buf(act, (self.num_envs, self.cm.act_dim), torch.float32, "act")
        self._check(self.L.kmanip_sample_action(self.h, C.c_void_p(act.data_ptr()), int(ahead), self._stream()), "kmanip_sample_action")
        return act

    def k_render(self, cam):
        """KManipEnvSim.k_render (env_sim.py:187-188): physics.render(cam.h, cam.w, camera_id=cam.name) -> uint8 RGB,
        for every env ([num_envs, h, w, 3], device tensor).  `cam` is a Cam (model.CAMERAS) or a camera name."""
        return self.render_rgb(cam)

    def k_close(self):
        if getattr(self, "h", None):
            self.L.kmanip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.k_close()
        except Exception:
            pass

    # ------------------------------------------------------------------ state / diagnostics (parity tests)
    def get_state(self):
        cm, n = self.cm, self.num_envs
        qpos = np.zeros((n, cm.nq)); qvel = np.zeros((n, cm.nv)); ctrl = np.zeros((n, cm.nu)); warm = np.zeros((n, cm.nv))
        step = np.zeros(n, dtype=np.int32)
        p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        self._check(self.L.kmanip_get_state(self.h, p(qpos), p(qvel), p(ctrl), p(warm), p(step, C.c_int32)), "kmanip_get_state")
        return qpos, qvel, ctrl, warm, step

    def step_counters(self):
        """Per-env step index inside the current episode (only the int32 counters cross PCIe)."""
        step = np.zeros(self.num_envs, dtype=np.int32)
        self._check(self.L.kmanip_get_state(self.h, None, None, None, None, step.ctypes.data_as(C.POINTER(C.c_int32))),
                    "kmanip_get_state")
        return step

    def set_seed(self, seed: int, restart_episodes: bool = True):
        """Re-key the cube-spawn stream (KManipEnv.reset(seed=...)); with restart_episodes the next k_reset is episode 0."""
        self._check(self.L.kmanip_set_seed(self.h, C.c_uint64(int(seed)), int(restart_episodes)), "kmanip_set_seed")
        self.seed = int(seed)

    def get_episode(self):
        """Per-env episode counter (keys the cube-spawn stream together with seed and global env id)."""
        ep = np.zeros(self.num_envs, dtype=np.int32)
        self._check(self.L.kmanip_get_episode(self.h, ep.ctypes.data_as(C.POINTER(C.c_int32))), "kmanip_get_episode")
        return ep

    def set_episode(self, episode):
        ep = np.ascontiguousarray(episode, dtype=np.int32)
        assert ep.shape == (self.num_envs,)
        self._check(self.L.kmanip_set_episode(self.h, ep.ctypes.data_as(C.POINTER(C.c_int32))), "kmanip_set_episode")

    def checkpoint(self):
        """Complete restartable state: (qpos, qvel, ctrl, qacc_warmstart, step_idx, episode, env_params, visual_params) as host
        arrays; env_params is None without per-env parameters, else (values float64[KM_EP_N, num_envs], lo, hi) -- lo / hi the
        ranges of ranges mode or None; visual_params likewise: None, or (values float64[KM_VP_N, num_envs] or None, lo, hi) --
        explicit values, or the ranges (the draw is a function of seed and episode, both restored with the state)."""
        ep = None
        if self._ep_active:
            vals = np.stack([v.cpu().numpy() for v in self.get_env_params().values()])
            lo, hi = (None, None) if self._ep_ranges is None else (self._ep_ranges[0].copy(), self._ep_ranges[1].copy())
            ep = (vals, lo, hi)
        vp = None
        if self._vp_active:
            if self._vp_ranges is None:
                vp = (self._get_visual_raw().cpu().numpy(), None, None)
            else:
                vp = (None, self._vp_ranges[0].copy(), self._vp_ranges[1].copy())
        return self.get_state() + (self.get_episode(), ep, vp)

    def restore(self, ckpt):
        qpos, qvel, ctrl, warm, step, episode = ckpt[:6]
        self.set_state(qpos, qvel, ctrl, warm, step)
        self.set_episode(episode)
        if len(ckpt) > 6:
            ep = ckpt[6]
            if ep is None:
                self.clear_env_params()
            else:
                vals, lo, hi = ep
                self.set_env_params(**{name: vals[k] for k, name in enumerate(ENV_PARAMS)})
                if lo is not None:
                    self._set_ranges_raw(lo, hi)
        if len(ckpt) > 7:
            vp = ckpt[7]
            if vp is None:
                self.clear_visual_params()
            elif vp[0] is not None:
                self._set_visual_raw(_torch().as_tensor(np.ascontiguousarray(vp[0], dtype=np.float64)).to(self.device))
            else:
                self._set_visual_ranges_raw(vp[1], vp[2])

    # ------------------------------------------------------------------ the state on the device
    _STATE_FIELDS = (("qpos", "qpos", "nq"), ("qvel", "qvel", "nv"), ("ctrl", "ctrl", "nu"), ("warm", "qacc_warm", "nv"),
                     ("step", "step_idx", None), ("episode", "episode", None))

    def _env_index(self, envs, what="envs"):
        """(int32 device tensor or None, its C pointer, n) of an env index: None = envs 0 .. num_envs-1."""
        torch = _torch()
        if envs is None:
            return None, None, None
        if not (isinstance(envs, torch.Tensor) and envs.is_cuda and envs.dtype == torch.int32):
            envs = torch.as_tensor(envs).to(device=self.device, dtype=torch.int32)
        envs = envs.contiguous()
        self._check_buf(envs, (envs.numel(),), torch.int32, what)
        return envs, C.c_void_p(envs.data_ptr()), int(envs.numel())

    def _state_dev(self, tensors, n):
        """KStateDev of a {name: tensor or None} dict, every tensor checked against n rows."""
        torch = _torch()
        sd = _libmod.KStateDev()
        for name, cname, width in self._STATE_FIELDS:
            t = tensors.get(name)
            if t is None:
                continue
            if width is None:
                self._check_buf(t, (n,), torch.int32, name)
            else:
                self._check_buf(t, (n, getattr(self.cm, width)), torch.float64, name)
            setattr(sd, cname, t.data_ptr())
        return sd

    def state_tensors(self, envs=None, out=None):
        """The state of `envs` as device tensors (kmanip_get_state_dev: one launch on the current stream, no synchronisation):
        {"qpos" [n, nq], "qvel" [n, nv], "ctrl" [n, nu], "warm" [n, nv] float64, "step" [n], "episode" [n] int32}; row j is env
        envs[j].  `envs`: an int32 device tensor or anything torch.as_tensor takes (repeats allowed); None = every env.  `out`: a
        dict of such tensors to fill -- only the fields it names are read (the others are skipped) -- returned as given."""
        torch = _torch()
        idx, ip, n = self._env_index(envs)
        n = self.num_envs if idx is None else n
        if out is None:
            out = {}
            for name, _, width in self._STATE_FIELDS:
                out[name] = (torch.empty((n,), dtype=torch.int32, device=self.device) if width is None else
                             torch.empty((n, getattr(self.cm, width)), dtype=torch.float64, device=self.device))
        unknown = set(out) - {f[0] for f in self._STATE_FIELDS}
        if unknown:
            raise ValueError("unknown state field(s) %s" % sorted(unknown))
        sd = self._state_dev(out, n)
        self._check(self.L.kmanip_get_state_dev(self.h, ip, n, C.byref(sd), self._stream()), "kmanip_get_state_dev")
        return out

    def set_state_tensors(self, envs=None, qpos=None, qvel=None, ctrl=None, warm=None, step=None, episode=None):
        """Write the given fields of `envs` from device tensors shaped as state_tensors returns them (kmanip_set_state_dev: one
        launch on the current stream).  Fields left None and envs not named keep every bit.  With `step` the bound sim_time of
        those envs follows; observations, rewards, done bytes and contact masks do not: call observe() for them."""
        idx, ip, n = self._env_index(envs)
        n = self.num_envs if idx is None else n
        sd = self._state_dev(dict(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm, step=step, episode=episode), n)
        self._check(self.L.kmanip_set_state_dev(self.h, ip, n, C.byref(sd), self._stream()), "kmanip_set_state_dev")

    def copy_envs_from(self, src, src_envs=None, dst_envs=None, episode=False, env_params=True):
        """Env dst_envs[j] of this handle becomes env src_envs[j] of `src` (kmanip_copy_envs, on the current stream): qpos, qvel,
        ctrl, warm start and step counter, the episode counter with episode=True, the per-env physics parameters with
        env_params=True.  An index left None is 0 .. n-1; with both None, n = this handle's num_envs.  `src` may be this handle
        (any permutation: every source is read before any destination is written).  With env_params=True, a `src` that has
        per-env parameters and a destination that has none, this handle first gets explicit parameters at the model's values
        (set_env_params: synchronous) -- only after the library has accepted every other argument: a refused copy leaves this handle as it
        was.  The clone's random streams stay its own: it follows its source only until a reset."""
        sidx, sp, sn = self._env_index(src_envs, "src_envs")
        didx, dp, dn = self._env_index(dst_envs, "dst_envs")
        if sn is not None and dn is not None and sn != dn:
            raise _libmod.KManipError("copy_envs_from: src_envs and dst_envs must have the same length (%d, %d)" % (sn, dn))
        n = dn if dn is not None else sn if sn is not None else self.num_envs
        flags = (_libmod.KM_COPY_EPISODE if episode else 0) | (_libmod.KM_COPY_ENV_PARAMS if env_params else 0)
        rc = self.L.kmanip_copy_envs(self.h, dp, src.h, sp, n, flags, self._stream())
        if rc != 0 and env_params and src._ep_active and not self._ep_active and \
                b"destination has no per-env parameters" in self.L.kmanip_last_error(self.h):
            # the library checks this last: every other argument was accepted, so only now does the destination change
            self.set_env_params()
            rc = self.L.kmanip_copy_envs(self.h, dp, src.h, sp, n, flags, self._stream())
        self._check(rc, "kmanip_copy_envs")

    def state_index_errors(self) -> int:
        """How many index entries outside 0 .. num_envs-1 state_tensors / set_state_tensors / copy_envs_from (as the destination)
        skipped since the last call; reads and clears the device counter (synchronous)."""
        c = C.c_int64(0)
        self._check(self.L.kmanip_state_index_errors(self.h, C.byref(c)), "kmanip_state_index_errors")
        return int(c.value)

    # ------------------------------------------------------------------ per-env physics parameters (domain randomisation)
    def set_env_params(self, **fields):
        """Explicit per-env values (and ranges mode off): each of cube_mass, cube_friction, cube_frictionloss, kp_scale a
        scalar or a [num_envs] tensor / array; unnamed fields keep the model's values.  Env e then behaves exactly like a
        handle of model.with_env_params(cm, **values of e).  Bad values raise KManipError, leaving the handle unchanged."""
        torch = _torch()
        unknown = set(fields) - set(ENV_PARAMS)
        if unknown:
            raise ValueError("unknown env parameter(s) %s (known: %s)" % (sorted(unknown), ", ".join(ENV_PARAMS)))
        base = env_param_defaults(self.cm)
        p = torch.empty((len(ENV_PARAMS), self.num_envs), dtype=torch.float64, device=self.device)
        for k, name in enumerate(ENV_PARAMS):
            v = fields.get(name)
            p[k] = base[name] if v is None else torch.as_tensor(v, dtype=torch.float64).to(self.device).expand(self.num_envs)
        self._check(self.L.kmanip_set_env_params(self.h, C.c_void_p(p.data_ptr()), self._stream()), "kmanip_set_env_params")
        self._ep_active, self._ep_ranges = True, None

    def get_env_params(self):
        """{name: float64[num_envs] device tensor} of the values in force (the drawn ones in ranges mode)."""
        torch = _torch()
        p = torch.empty((len(ENV_PARAMS), self.num_envs), dtype=torch.float64, device=self.device)
        self._check(self.L.kmanip_get_env_params(self.h, C.c_void_p(p.data_ptr()), self._stream()), "kmanip_get_env_params")
        return {name: p[k] for k, name in enumerate(ENV_PARAMS)}

    def set_env_param_ranges(self, **ranges):
        """Ranges mode: every reset of an env (k_reset or the auto-reset inside a step) draws each named parameter uniformly
        from (lo, hi) for the new episode, from the seed's counter-based stream; unnamed parameters are pinned to the model's
        value, lo == hi pins a value.  No argument turns ranges mode off (the values in force stay)."""
        if not ranges:
            self._check(self.L.kmanip_set_env_param_ranges(self.h, None, None), "kmanip_set_env_param_ranges")
            self._ep_ranges = None
            return
        unknown = set(ranges) - set(ENV_PARAMS)
        if unknown:
            raise ValueError("unknown env parameter(s) %s (known: %s)" % (sorted(unknown), ", ".join(ENV_PARAMS)))
        base = env_param_defaults(self.cm)
        lo = np.array([base[n] for n in ENV_PARAMS]); hi = lo.copy()
        for k, name in enumerate(ENV_PARAMS):
            if name in ranges:
                lo[k], hi[k] = (float(x) for x in ranges[name])
        self._set_ranges_raw(lo, hi)

    def _set_ranges_raw(self, lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.float64); hi = np.ascontiguousarray(hi, dtype=np.float64)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self.L.kmanip_set_env_param_ranges(self.h, ptr(lo), ptr(hi)), "kmanip_set_env_param_ranges")
        self._ep_active, self._ep_ranges = True, (lo.copy(), hi.copy())

    def clear_env_params(self):
        """Back to the compiled model for every env (bit-identical to a handle that never had parameters)."""
        self._check(self.L.kmanip_set_env_params(self.h, None, self._stream()), "kmanip_set_env_params")
        self._ep_active, self._ep_ranges = False, None

    # ------------------------------------------------------------------ per-env visual parameters (camera renders)
    def set_visual_params(self, **fields):
        """Explicit per-env visual values (and visual ranges mode off): cube_rgb, table_rgb, robot_rgb, background_rgb and
        camera_offset as [num_envs, 3] or a broadcast (3,); ambient, headlight and directional as [num_envs] or a scalar.  Unnamed
        fields keep their defaults (model.visual_param_defaults).  Names, shapes and limits (colours in [0, 1], light terms >= 0,
        |camera offset| <= 0.25 m, finite) are checked before the library is called; the renders then use the env's values."""
        torch = _torch()
        unknown = set(fields) - set(VISUAL_PARAMS)
        if unknown:
            raise ValueError("unknown visual parameter(s) %s (known: %s)" % (sorted(unknown), ", ".join(VISUAL_PARAMS)))
        n = self.num_envs
        rows = {}
        for name, v in fields.items():
            k, m = VISUAL_PARAMS[name]
            a = check_visual_param(name, v.cpu().numpy() if hasattr(v, "cpu") else v)
            if m == 3 and a.shape not in ((3,), (n, 3)):
                raise ValueError("%s: expected shape (3,) or (%d, 3), got %s" % (name, n, a.shape))
            if m == 1 and a.shape not in ((), (n,)):
                raise ValueError("%s: expected a scalar or shape (%d,), got %s" % (name, n, a.shape))
            rows[name] = np.broadcast_to(a, (n, 3) if m == 3 else (n,))
        p = np.empty((KM_VP_N, n))
        p[:] = visual_param_vector({})[:, None]
        for name, a in rows.items():
            k, m = VISUAL_PARAMS[name]
            p[k:k + m] = a.T if m == 3 else a[None]
        self._set_visual_raw(torch.from_numpy(p).to(self.device))

    def _set_visual_raw(self, p):
        p = p.to(dtype=_torch().float64).contiguous()
        self._check(self.L.kmanip_set_visual_params(self.h, C.c_void_p(p.data_ptr()), self._stream()), "kmanip_set_visual_params")
        self._vp_active, self._vp_ranges = True, None

    def _get_visual_raw(self):
        p = _torch().empty((KM_VP_N, self.num_envs), dtype=_torch().float64, device=self.device)
        self._check(self.L.kmanip_get_visual_params(self.h, C.c_void_p(p.data_ptr()), self._stream()), "kmanip_get_visual_params")
        return p

    def get_visual_params(self):
        """{name: float64 device tensor [num_envs, 3] or [num_envs]} of the values in force: the defaults when none are set, the
        draw of every env's current episode in ranges mode."""
        p = self._get_visual_raw()
        return {name: (p[k:k + m].T if m == 3 else p[k]) for name, (k, m) in VISUAL_PARAMS.items()}

    def set_visual_param_ranges(self, **ranges):
        """Visual ranges mode: each named parameter (name=(lo, hi), lo / hi scalars or 3-vectors for the rgb / offset fields) is
        drawn per env and episode from the seed's counter-based stream; every reset redraws.  Unnamed parameters stay at their
        defaults.  No argument turns ranges mode off, keeping every env's current draw as explicit values."""
        if not ranges:
            self._check(self.L.kmanip_set_visual_param_ranges(self.h, None, None), "kmanip_set_visual_param_ranges")
            self._vp_ranges = None
            return
        unknown = set(ranges) - set(VISUAL_PARAMS)
        if unknown:
            raise ValueError("unknown visual parameter(s) %s (known: %s)" % (sorted(unknown), ", ".join(VISUAL_PARAMS)))
        lo, hi = visual_param_vector({}), visual_param_vector({})
        for name, r in ranges.items():
            k, m = VISUAL_PARAMS[name]
            if len(r) != 2:
                raise ValueError("%s: expected (lo, hi)" % name)
            a, b = (check_visual_param(name, x) for x in r)
            if a.shape not in ((), (m,)) or b.shape not in ((), (m,)) or (m == 1 and (a.shape or b.shape)):
                raise ValueError("%s: lo / hi must be scalars%s" % (name, " or 3-vectors" if m == 3 else ""))
            if (a > b).any():
                raise ValueError("%s: lo > hi" % name)
            lo[k:k + m], hi[k:k + m] = a, b
        self._set_visual_ranges_raw(lo, hi)

    def _set_visual_ranges_raw(self, lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.float64); hi = np.ascontiguousarray(hi, dtype=np.float64)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self.L.kmanip_set_visual_param_ranges(self.h, ptr(lo), ptr(hi)), "kmanip_set_visual_param_ranges")
        self._vp_active, self._vp_ranges = True, (lo.copy(), hi.copy())

    def clear_visual_params(self):
        """Back to the default render kernels for every env (bit-identical to a handle that never had visual parameters)."""
        self._check(self.L.kmanip_set_visual_params(self.h, None, self._stream()), "kmanip_set_visual_params")
        self._vp_active, self._vp_ranges = False, None

    def set_state(self, qpos=None, qvel=None, ctrl=None, warm=None, step=None):
        def p(a, dt, t):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=dt)
            return a, a.ctypes.data_as(C.POINTER(t))
        keep = []
        args = []
        for a, dt, t in [(qpos, np.float64, C.c_double), (qvel, np.float64, C.c_double), (ctrl, np.float64, C.c_double),
                         (warm, np.float64, C.c_double), (step, np.int32, C.c_int32)]:
            arr, ptr = p(a, dt, t)
            keep.append(arr); args.append(ptr)
        self._check(self.L.kmanip_set_state(self.h, *args), "kmanip_set_state")

    def get_diag(self):
        n = self.num_envs
        mask = np.zeros(n, dtype=np.uint32); nfev = np.zeros((n, 2), dtype=np.int32); st = np.zeros((n, 2), dtype=np.int32)
        self._check(self.L.kmanip_get_diag(self.h, mask.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           nfev.ctypes.data_as(C.POINTER(C.c_int32)),
                                           st.ctypes.data_as(C.POINTER(C.c_int32))), "kmanip_get_diag")
        return mask, nfev, st

    def ik(self, arm, qpos, goal_pos, goal_quat):
        """Batched ik_mujoco.ik on device: returns (q_out, qpos_after, nfev, status)."""
        qpos = np.ascontiguousarray(qpos, dtype=np.float64).copy()
        n = qpos.shape[0]
        gp = np.ascontiguousarray(goal_pos, dtype=np.float64); gq = np.ascontiguousarray(goal_quat, dtype=np.float64)
        nik = self.cm.desc.arm_nq[arm]
        q = np.zeros((n, nik)); nfev = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
        p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        self._check(self.L.kmanip_ik(self.h, arm, n, p(qpos), p(gp), p(gq), p(q), p(nfev, C.c_int32), p(st, C.c_int32)), "kmanip_ik")
        return q, qpos, nfev, st

    def ik_eval(self, arm, qpos, goal_pos, goal_quat):
        """(ik_res, ik_jac) of the device IK at x = qpos[q_mask], q_pos_prev = x: res [n, 6+2N], jac [n, 6+2N, N]."""
        qpos = np.ascontiguousarray(qpos, dtype=np.float64)
        n = qpos.shape[0]
        gp = np.ascontiguousarray(goal_pos, dtype=np.float64); gq = np.ascontiguousarray(goal_quat, dtype=np.float64)
        nik = self.cm.desc.arm_nq[arm]
        res = np.zeros((n, 6 + 2 * nik)); jac = np.zeros((n, 6 + 2 * nik, nik))
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self.L.kmanip_ik_eval(self.h, arm, n, p(qpos), p(gp), p(gq), p(res), p(jac)), "kmanip_ik_eval")
        return res, jac

    def dbg_math(self, fn, rows):
        """Diagnostic (include/kmanip_debug.h kmanip_dbg_math): the helper `fn` of the kernels' math headers (a key of lib.MATH_FNS)
        on every row of `rows`, a contiguous float64 device tensor [n, arguments].  Returns the device tensor [n, results]; one launch
        on the current stream, no synchronisation; the handle is only read."""
        torch = _torch()
        code, ic, oc = _libmod.MATH_FNS[fn]
        n = int(rows.shape[0])
        self._check_buf(rows, (n, ic), torch.float64, "dbg_math rows")
        out = torch.empty((n, oc), dtype=torch.float64, device=self.device)
        self._check(self.L.kmanip_dbg_math(self.h, code, n, C.c_void_p(rows.data_ptr()), ic, C.c_void_p(out.data_ptr()), oc, self._stream()),
                    "kmanip_dbg_math")
        return out

    def enable_timing(self, on=True):
        """on = True / 1: events around every step; an int k > 1: around every k-th step (the sampled average; an event pair costs
        the stream about 5 us); False / 0: off."""
        self._check(self.L.kmanip_enable_timing(self.h, int(on)), "kmanip_enable_timing")

    def timing_summary(self):
        """(ik_ms_sum, dyn_ms_sum, render_ms_sum, nsteps) of the steps recorded since enable_timing / the last summary: 0 (the IK
        runs inside k_step; the slot is kept for the C ABI), k_step, and the in-step render kernel (bind_step_depth; 0 when nothing is bound)."""
        a = C.c_double(); b = C.c_double(); r = C.c_double(); n = C.c_int32()
        self._check(self.L.kmanip_timing_summary(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(n)), "kmanip_timing_summary")
        return float(a.value), float(b.value), float(r.value), int(n.value)


def spec_from_gym_env(gym_env) -> EnvSpec:
    """Read the same attributes env_sim.new reads from the KManipEnv instance."""
    return EnvSpec(env_id=getattr(gym_env, "env_id", "custom"), asset=MJCF_TO_ASSET[gym_env.mjcf_filename],
                   obs_list=list(gym_env.obs_list), act_list=list(gym_env.act_list),
                   q_pos_home=np.asarray(gym_env.q_pos_home, dtype=np.float32),
                   q_id_r_mask=None if gym_env.q_id_r_mask is None else list(gym_env.q_id_r_mask),
                   q_id_l_mask=None if getattr(gym_env, "q_id_l_mask", None) is None else list(gym_env.q_id_l_mask),
                   ctrl_id_r_grip=None if gym_env.ctrl_id_r_grip is None else list(gym_env.ctrl_id_r_grip),
                   ctrl_id_l_grip=None if getattr(gym_env, "ctrl_id_l_grip", None) is None else list(gym_env.ctrl_id_l_grip))


def new(gym_env, num_envs: int = 1, device: int = 0, env_id_offset: int = 0, **compile_kw) -> KManipEnvHip:
    """Drop-in third backend: `self.env = env_hip.new(self)` in KManipEnv.__init__ (env_base.py:192-200)."""
    cm = compile_model(spec_from_gym_env(gym_env), **compile_kw)
    return KManipEnvHip(cm, num_envs=num_envs, device=device, seed=int(getattr(gym_env, "seed", 0) or 0),
                        env_id_offset=env_id_offset)


def make(env_id: str, num_envs: int = 1, device: int = 0, seed: int = 0, env_id_offset: int = 0, **compile_kw) -> KManipEnvHip:
    """Shortcut used by bench/tests: build straight from a registered env id (__init__.py:244-483)."""
    return KManipEnvHip(compile_model(ENV_SPECS[env_id], **compile_kw), num_envs=num_envs, device=device, seed=seed,
                        env_id_offset=env_id_offset)
