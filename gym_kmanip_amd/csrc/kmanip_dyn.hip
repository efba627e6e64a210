// kmanip_dyn.hip -- one control step (or a chunk of them) of every env in ONE launch (gfx950, wave64).
//
// Replaces, for every env, KManipEnvSim.k_step (reference gym_kmanip/env_sim.py:196-200): KManipTask.before_step
// (env_sim.py:38-108: action decode + IK, device code in kmanip_ik_coop.hpp, fused in here) and then
// `physics.step(n_sub_steps)` as dm_control runs it (control_timestep :210), legacy order
//   mj_step2 (on products of the PRE-IK state) ; (n-1) x mj_step ; mj_step1
// followed by KManipTask.get_reward (env_sim.py:148-179) and get_observation (env_sim.py:110-146), the
// TimeLimit done flag (__init__.py:28,247) and, when enabled, the auto-reset
// (KManipTask.initialize_episode env_sim.py:23-36 + dm_control's mj_forward without actuation).
//
// Execution model ("many envs per wavefront"): a workgroup is ONE wave of 64 lanes holding 64/G envs;
// each env is owned by a group of G lanes (G = 16 for nv = 16, G = 32 for nv = 26), lane d of the group
// owning dof d: its component of qacc, its COLUMN of every contact-basis Jacobian, its ROW of the joint-space
// inertia, of the Newton Hessian and of its Cholesky factor, and its own single-dof constraint rows all live in
// that lane's registers.  The cooperative linear algebra exchanges values with DPP row broadcasts folded into the
// FMA (v_fmac_f64_dpp row_newbcast; v_permlane16_swap copies for the two-row groups) -- no LDS, no synchronisation.
// Per-env data that needs lane-indexed random access (body frames, M^-1, contact geometry and records) sits in LDS:
// 7 KB per env for Solo, 15 KB for Dual/Torso in the Newton variant.  The kernel needs 400-500 registers, i.e. one
// wave per SIMD: 16 Solo envs per CU, all 4096 envs of the headline config resident in a single round.  HBM is
// touched once on entry and once on exit with struct-of-arrays coalesced columns.  Per-env reductions are DPP row
// reductions (row_mirror / row_half_mirror / quad_perm, v_permlane16_swap across the rows of a 32-lane group) whose
// result is bitwise identical on every lane (they opt out of FMA contraction for that reason).  A lane group never
// needs s_barrier: all its lanes sit in one wave.
//
// Formulations deliberately differ from the oracle's (so parity is a cross-check, not a re-run):
//   mass matrix      : composite inertias about the world origin, one column per lane (oracle: link-frame CRBA)
//   bias forces      : per-body bias wrenches projected with J^T   (oracle: RNE backward recursion)
//   M^-1             : explicit inverse, Gauss-Jordan on register rows (oracle: Cholesky factor + solves)
//   Newton           : incremental state, Hessian rows / Cholesky / solves in registers (oracle: dense, recomputed per iteration)
//   constraint rows  : single-dof rows + 4-vector contact bases, pyramid edges expanded on the fly
//   PGS              : per-contact block form on the 4x4 Gram matrix (algebraically the same row order)
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
// the build macros (KM_VAR_*, the per-build kernel and launcher names), the variant namespace and the device code of one step, by phase
#include "kmanip_dyn_variant.hpp"
// ---------------------------------------------------------------------------------------------
// EPB = envs per single-wave workgroup (<= 64 / G).  Fewer envs per wave = more waves per SIMD: the kernel is
// bound by LDS/dependent-issue latency, so waves of different envs hide each other's waits.
template <int NL, int G, int SOLVER, int EPB, bool CHUNK>
__global__ __launch_bounds__(64) void KM_KERNEL(k_step)(const KDeviceModel* __restrict__ dm, KDeviceState st, const float* __restrict__ act,
                                             double* __restrict__ obs, double* __restrict__ reward, uint8_t* __restrict__ done,
                                             int nchunk) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  // wave slot -> env: the identity behind the XCD-aware block mapping, or -- launches of several residency rounds -- the
  // predicted-cost order of k_sort_envs with workgroup 0 first (longest-processing-time-first dispatch); or SPREAD's deal of
  // the slot's block.  Looked up BEFORE the model is staged: the dependent loads wait beside the staging's own.
  const int slot = (st.slot_env ? (int)blockIdx.x : xcd_block(blockIdx.x, gridDim.x)) * EPB + grp;
  int env = -1;
  unsigned long long heavy_mask = 0, s1_mask = 0, s2_mask = 0;
  if (st.spread_in) {
    // SPREAD (KDeviceState): the 64 flags of this wave's block of 64 consecutive envs, one per lane (every lane votes: before any exit)
    const int blk = (slot - grp) / 64;
    const int fl = st.spread_in[blk * 64 + lane];
    heavy_mask = __ballot((fl & 1) != 0);
    s1_mask = __ballot((fl & 2) != 0);
    s2_mask = __ballot((fl & 4) != 0);
  }
  if (grp >= EPB) {
  } else if (st.spread_in) {
    const int wv = (slot - grp) / EPB;                        // this wave's index in slot space (xcd_block keeps an XCD's waves together)
    env = (wv / (64 / EPB)) * 64 + spread_pick(heavy_mask, s1_mask, s2_mask, wv % (64 / EPB), grp, EPB);
  } else if (slot < st.num_envs) {
    env = st.slot_env ? st.slot_env[slot] : slot;
  }
  stage_model<NL>(lm, dm);
  if (env < 0) return;                                 // whole group exits together
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane (KM_VAR_PAR: set by ep_load below)
#if !KM_VAR_PAR
  invm = cube_invm<NL>(m, sub);
#endif
  Prof pf;
  pf.start();
  const unsigned long long t_wave0 = st.wave_clk ? __builtin_amdgcn_s_memtime() : 0ull;
  const unsigned long long r_wave0 = st.wave_clk ? __builtin_amdgcn_s_memrealtime() : 0ull;
#ifdef KM_DEBUG_NANFILL   // diagnostic build (-DKM_DEBUG_NANFILL=<value>): poison the workspace, so that a read of LDS this launch did not write shows
  { double* wp = reinterpret_cast<double*>(&w); for (int i = sub; i < (int)(sizeof(Ws<NL>) / 8); i += G) wp[i] = KM_DEBUG_NANFILL; GSYNC(); }
#endif
  init_ws<NL>(w, sub);
#if KM_VAR_PAR
  ep_load<NL>(w, dm, st, env, sub, invm);       // (after the diagnostic poisoning above: Ws::ep is part of the workspace)
#endif
  load_state<NL, G>(w, st, env, sub);
#if KM_VAR_FRC
  const int frc_bad = load_applied<NL, G>(w, st, env, sub);      // (a chunk holds the row for all its steps)
#endif
  int step_idx = st.step_idx[env], episode = st.episode[env];
  const size_t NE = (size_t)st.num_envs;
  GSYNC();
  pf.ph(29);
  // nchunk control steps per launch (kmanip_step: 1).  With a chunk of pre-supplied actions every wave runs its envs
  // through all of them without meeting the other waves at a launch boundary, so the batch advances at the MEAN wave
  // speed instead of the slowest wave's; the state stays in LDS between the steps of a chunk.
  const int nsteps = CHUNK ? nchunk : 1;      // (the single-step kernel keeps its register allocation: no outer loop)
  int spread_next = 0;                        // this env's SPREAD flag for the next launch (the state it ENDS the step in)
  for (int kc = 0; kc < nsteps; kc++) {
  if (kc > 0) {
    // what load_state does for the first step: ctrl <- float32(ctrl) (env_sim.py:40), qpos_ik <- qpos
    if (sub < NL) { w.ctrl[sub] = (real)(float)w.ctrl[sub]; w.qpos_ik[sub] = w.qpos[sub]; }
    if (sub == 0) { w.bad = 0; w.work = 0; }
    GSYNC();
  }
  // ---- KManipTask.before_step: 8 lanes per arm, one arm per 16-lane DPP row of the group (lanes 0-7 of row 0: right arm;
  // of row 1, in the two-row groups: left arm), the rest idle.
  // Fused here so that an env whose IK needs many evaluations delays only its own wave, not the whole batch.
  // (chunk kernels: the lane index is made opaque once per control step, like the dof index per sub-step below -- otherwise the
  // IK's per-lane chain constants, invariant across the steps of a chunk, are hoisted out of the chunk loop and kept alive
  // through the physics: the two-arm chunk kernels sat at the 512-register cap with 268 / 116 bytes of scratch)
  int subk = sub;
  if constexpr (CHUNK) asm volatile("" : "+v"(subk));
  const int arm = subk / GS;
  if (subk % GS < GI && arm < KM_MAX_ARMS && (NL > 10 || arm == 0) && m->arm_present[arm]) {
    LdsIO<NL> io{w, st, env};
    const float* arow = act + ((size_t)kc * NE + env) * m->act_dim;
    if (m->arm_nq[arm] == 7) coop_before_step<7>(dm, arm, subk % GS, arow, io, &pf);
    else coop_before_step<6>(dm, arm, subk % GS, arow, io, &pf);
  }
  GSYNC();
  pf.ph(30);
#if KM_VAR_FRC
  // a non-finite applied force: the env counts as diverged for this step before a sub-step starts
  int bad = frc_bad;
  spread_next = 0;
  const int nsub = frc_bad ? 0 : m->n_sub_steps;
#else
  int bad = 0;
  spread_next = 0;
  const int nsub = m->n_sub_steps;
#endif
  for (int s = 0; s < nsub; s++) {
    // the lane's dof index, opaque to the optimiser once per sub-step: everything derived from it (LDS addresses, per-link
    // constants, masks) is recomputed inside the sub-step instead of being hoisted out of this loop and kept alive -- or
    // shuttled through AGPRs -- across all ten (380 -> 318 registers, measured)
    int subv = sub; asm volatile("" : "+v"(subv));
    CReg<NL> cr;                       // (one per sub-step: nothing of it can be carried round the loops)
    step1_products<NL, G, SOLVER>(w, lm, m, subv, cr, invm, pf);      // s == 0: products of the pre-IK state (stale mj_step2)
    real a = solve<NL, G, SOLVER>(w, lm, m, subv, 1, cr, invm, pf);
    pf.ph(28);
    int lb = (sub < NV) && (!isfinite(a) || fabs(a) > 1e10);   // mjWARN_BADQACC
    bad = gor<G>(lb) | w.bad;
    if (bad) break;
    if (s == 0) {                                        // the IK teleported the arm (ik_mujoco.py:34,67)
      if (sub < NL) w.qpos[sub] = w.qpos_ik[sub];
      GSYNC();
    }
    integrate<NL, G>(w, m, sub, a);
    pf.ph(27);
  }
  if (!bad) {
    int lb = 0;
    for (int i = sub; i < NQ; i += G) lb |= !isfinite(w.qpos[i]);
    bad = gor<G>(lb);
  }
  uint8_t dn = 0;
  real rew = 0;
  double* obs_row = obs + ((size_t)kc * NE + env) * m->obs_dim;
  if (!bad) {
    // trailing mj_step1: kinematics + collision feed reward and the contact mask
    fk_parallel<NL, G>(w, lm, sub);
    const int near_cube = collide_parallel<NL, G, true>(w, lm, m, sub, st.near_margin);
    // the cost score of an env that is not heavy (spread_pick): bit 1 a sphere on the table, bit 0 a cube that does not rest on four corners
    {
      const int tb = (w.contact_mask & KM_CON_ANY_SPHERE_TABLE) != 0, cb = __popc(w.contact_mask & KM_CON_ANY_CUBE_TABLE) != 4;
      spread_next = (near_cube != 0) | (2 * tb + cb) << 1;      // bit 0: heavy (a collider on or near the cube)
    }
    if constexpr (KM_WORK_COUNTERS(NL)) { if (sub == 0 && near_cube) w.work |= 1 << 30; }     // (bit 30: a collider on or close to the cube)
    rew = env_reward<NL, G>(w, m, sub);
    write_obs<NL, G>(w, lm, m, sub, obs_row);
    if (sub == 0) st.contact_mask[env] = w.contact_mask;
  } else {
    dn |= KM_DONE_DIVERGED;
    for (int i = sub; i < m->obs_dim; i += G) obs_row[i] = 0;
    if (sub == 0) st.contact_mask[env] = 0;
  }
  step_idx += 1;
  if (step_idx >= m->max_episode_steps) dn |= KM_DONE_TRUNCATED;
  if (dn && (m->auto_reset || bad)) {
    episode += 1; step_idx = 0;
    spread_next = 0;                              // (the respawned cube is nowhere near the home pose)
    GSYNC();
    pf.ph(31);
    CReg<NL> cr;
    reset_env<NL, G, SOLVER>(w, lm, dm, sub, st, env, episode, cr, invm, pf);
    write_obs<NL, G>(w, lm, m, sub, obs_row);
    pf.ph(32);
  }
  if (sub == 0) {
    reward[(size_t)kc * NE + env] = rew; done[(size_t)kc * NE + env] = dn;
    if (!CHUNK && st.rd_rec) { st.rd_rec[2 * (size_t)env] = rew; st.rd_rec[2 * (size_t)env + 1] = (real)dn; }
  }
  GSYNC();
  }   // chunk
  if (sub == 0) {
    st.step_idx[env] = step_idx; st.episode[env] = episode;
    if (st.sim_time) st.sim_time[env] = step_idx * st.control_dt;
    if (st.spread_out) st.spread_out[env] = (uint8_t)spread_next;      // (a chunk: the state its LAST step ends in)
    if constexpr (KM_WORK_COUNTERS(NL)) st.work[env] = w.work;      // (the last control step's: what the next launch's slot order is predicted from)
    // (diagnostics: core-clock cycles in the low 40 bits; above them the wave's START on the constant 100 MHz clock, 24 bits)
    if (st.wave_clk) st.wave_clk[slot] = ((__builtin_amdgcn_s_memtime() - t_wave0) & 0xFFFFFFFFFFull) | ((r_wave0 & 0xFFFFFFull) << 40);
  }
  store_state<NL, G>(w, st, env, sub);
  pf.ph(31);
  pf.flush();
}

// KManipEnvSim.k_reset for the envs selected by mask (NULL = all)
template <int NL, int G, int SOLVER, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_reset)(const KDeviceModel* __restrict__ dm, KDeviceState st,
                                              const uint8_t* __restrict__ mask, double* __restrict__ obs) {
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  stage_model<NL>(lm, dm);
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  const int env = xcd_block(blockIdx.x, gridDim.x) * EPB + grp;
  if (grp >= EPB || env >= st.num_envs) return;
  if (mask && !mask[env]) return;
  Ws<NL>& w = ws[grp];
  CReg<NL> cr;
  real invm = 0;
  env_invm<NL>(w, dm, st, env, sub, invm);
  int episode = st.episode[env] + 1;
  Prof pf;
  pf.start();
  init_ws<NL>(w, sub);
  reset_env<NL, G, SOLVER>(w, lm, dm, sub, st, env, episode, cr, invm, pf);
  if (obs) write_obs<NL, G>(w, lm, m, sub, obs + (size_t)env * m->obs_dim);
  if (sub == 0) { st.step_idx[env] = 0; st.episode[env] = episode; st.contact_mask[env] = 0; if (st.sim_time) st.sim_time[env] = 0; }
  GSYNC();
  store_state<NL, G>(w, st, env, sub);
}

// get_observation + get_reward of the CURRENT state (no step): what a trailing mj_step1 and the two task methods give
template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void k_observe(const KDeviceModel* __restrict__ dm, KDeviceState st, double* __restrict__ obs,
                                                double* __restrict__ reward) {
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int env;
  if (!query_env<NL, EPB>(lm, dm, st, grp, env)) return;
  Ws<NL>& w = ws[grp];
  real invm = 0;
  query_load<NL, G>(w, dm, st, env, sub, invm);
  GSYNC();
  // a state restored from a diverged checkpoint: what k_step reports for such an env -- zero observation and reward, no contacts
  // (the kinematics of a non-finite state would put garbage into the mask the diagnostics and the next cost sort read)
  if (state_nonfinite<NL, G>(w, sub)) {
    if (obs) for (int i = sub; i < m->obs_dim; i += G) obs[(size_t)env * m->obs_dim + i] = 0;
    if (sub == 0) { st.contact_mask[env] = 0; if (reward) reward[env] = 0; }
    return;
  }
  fk_parallel<NL, G>(w, lm, sub);
  collide_parallel<NL, G>(w, lm, m, sub);
  const real rew = env_reward<NL, G>(w, m, sub);
  if (obs) write_obs<NL, G>(w, lm, m, sub, obs + (size_t)env * m->obs_dim);
  if (sub == 0) { st.contact_mask[env] = w.contact_mask; if (reward) reward[env] = rew; }
}

template <int NL, int G, int SOLVER, int EPB>
static void launch_step_e(const KDeviceModel* dm, const KDeviceState& st, const float* act, double* obs, double* reward, uint8_t* done, int nchunk, hipStream_t stream) {
  if (nchunk > 1) {
    if constexpr (EPB == 64 / G) hipLaunchKernelGGL((KM_KERNEL(k_step)<NL, G, SOLVER, EPB, true>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, act, obs, reward, done, nchunk);
  } else {
    hipLaunchKernelGGL((KM_KERNEL(k_step)<NL, G, SOLVER, EPB, false>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, act, obs, reward, done, 1);
  }
}
template <int NL, int G, int SOLVER, int EPB>
static void launch_reset_e(const KDeviceModel* dm, const KDeviceState& st, const uint8_t* mask, double* obs, hipStream_t stream) {
  hipLaunchKernelGGL((KM_KERNEL(k_reset)<NL, G, SOLVER, EPB>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, mask, obs);
}
template <int NL, int G, int SOLVER>
static void launch_step_t(const KDeviceModel* dm, const KDeviceState& st, const float* act, double* obs, double* reward, uint8_t* done, int nchunk,
                          int epb, hipStream_t stream) {
  if constexpr (64 / G >= 4) if (epb == 4) return launch_step_e<NL, G, SOLVER, 4>(dm, st, act, obs, reward, done, nchunk, stream);
  if (epb == 2) return launch_step_e<NL, G, SOLVER, 2>(dm, st, act, obs, reward, done, nchunk, stream);
  launch_step_e<NL, G, SOLVER, 1>(dm, st, act, obs, reward, done, nchunk, stream);
}
template <int NL, int G, int SOLVER>
static void launch_reset_t(const KDeviceModel* dm, const KDeviceState& st, const uint8_t* mask, double* obs, int epb, hipStream_t stream) {
  if constexpr (64 / G >= 4) if (epb == 4) return launch_reset_e<NL, G, SOLVER, 4>(dm, st, mask, obs, stream);
  if (epb == 2) return launch_reset_e<NL, G, SOLVER, 2>(dm, st, mask, obs, stream);
  launch_reset_e<NL, G, SOLVER, 1>(dm, st, mask, obs, stream);
}
// kmanip_create, once: the LDS image of the model constants into KDeviceModel::staged (one workgroup)
template <int NL>
__global__ __launch_bounds__(64) void k_prepare_model(KDeviceModel* dm) {
  __shared__ LModel<NL> lm;
  { unsigned char* z = reinterpret_cast<unsigned char*>(&lm); for (int i = threadIdx.x; i < (int)sizeof(LModel<NL>); i += 64) z[i] = 0; }      // (padding bytes: defined)
  __syncthreads();
  build_lmodel<NL>(lm, dm);
  const uint4* src = reinterpret_cast<const uint4*>(&lm);
  uint4* dst = reinterpret_cast<uint4*>(dm->staged);
  for (int i = threadIdx.x; i < (int)(sizeof(LModel<NL>) / 16); i += 64) dst[i] = src[i];
}
template <int NL, int G>
static void launch_observe_t(const KDeviceModel* dm, const KDeviceState& st, double* obs, double* reward, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((k_observe<NL, G, EPB>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, obs, reward);
}
KM_VARIANT_END
// ---- one (NL, G, SOLVER[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file sixteen times, in parallel)
void KM_LAUNCHER3(step)(const KDeviceModel* dm, const KDeviceState& st, const float* act,
                                                                    double* obs, double* reward, uint8_t* done, int nchunk, int epb,
                                                                    hipStream_t stream) {
  launch_step_t<KM_VAR_NL, KM_VAR_G, KM_VAR_SOLVER>(dm, st, act, obs, reward, done, nchunk, epb, stream);
}
#if !KM_VAR_FRC      // (a reset ignores the applied force: the force builds have no reset kernel)
void KM_LAUNCHER3(reset)(const KDeviceModel* dm, const KDeviceState& st,
                                                                     const uint8_t* mask, double* obs, int epb, hipStream_t stream) {
  launch_reset_t<KM_VAR_NL, KM_VAR_G, KM_VAR_SOLVER>(dm, st, mask, obs, epb, stream);
}
#endif
#if KM_VAR_SOLVER == 1 && !KM_VAR_PAR && !KM_VAR_FRC      // (solver-independent: one copy per link-count class)
void KM_LAUNCHER3(prepare)(KDeviceModel* dm, hipStream_t stream) {
  hipLaunchKernelGGL((k_prepare_model<KM_VAR_NL>), dim3(1), dim3(64), 0, stream, dm);
}
void KM_LAUNCHER3(observe)(const KDeviceModel* dm, const KDeviceState& st, double* obs,
                                                                       double* reward, hipStream_t stream) {
  launch_observe_t<KM_VAR_NL, KM_VAR_G>(dm, st, obs, reward, stream);
}
#endif
// ---- KM_PROFILE builds: host accessors of the phase accumulators (g_prof, kmanip_device.hpp)
#ifdef KM_PROFILE
#if KM_VAR_NL == 10 && KM_VAR_SOLVER == 1 && !KM_VAR_PAR && !KM_VAR_FRC
extern "C" int kmanip_dbg_prof(unsigned long long* out, int reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * KM_NPH) != hipSuccess) return -1;
  if (reset) { unsigned long long z[KM_NPH] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
extern "C" int kmanip_dbg_prof_blocks(unsigned long long* out, int nblocks) {
  if (nblocks > KM_PROF_BLOCKS) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof_blk), sizeof(unsigned long long) * KM_NPH * 4 * nblocks) == hipSuccess ? 0 : -1;
}
#endif
#if KM_VAR_NL == 20 && KM_VAR_SOLVER == 1 && !KM_VAR_PAR && !KM_VAR_FRC
extern "C" int kmanip_dbg_prof20(unsigned long long* out, int reset) {          // the DualArm / Torso Newton object's accumulators
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * KM_NPH) != hipSuccess) return -1;
  if (reset) { unsigned long long z[KM_NPH] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
#endif
#endif
