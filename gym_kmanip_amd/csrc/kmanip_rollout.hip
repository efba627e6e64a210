// kmanip_rollout.hip -- open-loop rollouts in ctrl space from rows the CALLER passes, as many as it likes, in ONE launch (gfx950,
// wave64): kmanip_rollout.
//
// MuJoCo's `rollout`: row r names an env (KRolloutIn::env_index; NULL = row r is env r), takes that env's model parameters and, per
// field, either the caller's row of qpos / qvel / qacc_warm / ctrl / qfrc_applied or what the env stores, and is integrated for nstep
// steps of nsub sub-steps each; the state after every step is recorded at the row.  ctrl and the force are either held or given per
// step, and ctrl is used exactly as given: no action decode, no IK, no CTRL_ALPHA filter, no float32 rounding.  Nothing of the handle
// is written, nothing resets and no random number is drawn; a row that diverges stops there.
// The device code of a sub-step is k_step's (kmanip_dyn.hip) -- step1_products, solve with actuation, the bad-qacc test, integrate, the
// warm start carried by integrate -- with qpos_ik == qpos: no teleport, every sub-step a plain mj_step.  Both solvers: the rollout
// runs the handle's (only solve's return value is read, no register of the Newton path).  The optional trailing pass per step is
// k_step's too: fk_parallel + collide_parallel + env_reward on the state after the step.  The entry is k_forward's
// (kmanip_forward.hip), restated here rather than shared: a helper moved into the common headers reorders the code of the other
// kernels.  A translation unit of its own, so that every other object is the one it was, to the register.
// One wave per workgroup, 64 / G ROWS per wave; the state stays in LDS for all nstep x nsub sub-steps.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"

// zero records of steps t0 .. nstep-1 of one row (a row that stopped, or never started), then its status and step count
template <int NL, int G>
__device__ __forceinline__ void rollout_finish(const KRolloutDev& out, size_t row, int sub, int nstep, int t0, int status) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  for (int t = t0; t < nstep; t++) {
    const size_t e = row * (size_t)nstep + t;
    if (out.qpos) for (int i = sub; i < NQ; i += G) out.qpos[e * NQ + i] = 0.0;
    if (sub < NV) {
      if (out.qvel) out.qvel[e * NV + sub] = 0.0;
      if (out.qacc_warm) out.qacc_warm[e * NV + sub] = 0.0;
    }
    if (sub == 0) {
      if (out.contact_mask) out.contact_mask[e] = 0u;
      if (out.reward) out.reward[e] = 0.0;
    }
  }
  if (sub == 0) {
    if (out.status) out.status[row] = (uint8_t)status;
    if (out.steps_done) out.steps_done[row] = t0;
  }
}

template <int NL, int G, int SOLVER, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_rollout)(const KDeviceModel* __restrict__ dm, KDeviceState st, KRolloutIn in, int n, int nstep,
                                                           int nsub, KRolloutDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  static_assert(NV <= G, "lane = dof");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  // k_forward's entry: the model staged by every lane, then a group without a row exits whole
  stage_model<NL>(lm, dm);
  const int row = xcd_block(blockIdx.x, gridDim.x) * EPB + grp;
  if (grp >= EPB || row >= n) return;
  const size_t r = (size_t)row;
  const int env = in.env_index ? in.env_index[row] : row;
  // an index outside the handle (group-uniform): never used as an address
  if (env < 0 || env >= st.num_envs) { rollout_finish<NL, G>(out, r, sub, nstep, 0, 2); return; }
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  const int NE = st.num_envs;
  init_ws<NL>(w, sub);
  env_invm<NL>(w, dm, st, env, sub, invm);
  // the caller's rows of the state and of step 0's (or the held) ctrl and force, requested before the handle's columns are waited
  // for; row (r, t) of a per-step tensor is row r * nstep + t
  constexpr int KQ = (NQ + G - 1) / G, KV = (NV + G - 1) / G, KL = (NL + G - 1) / G;
  // (a per-step flag counts only with the caller's own tensor: kmanip_rollout refuses it on a NULL one)
  const bool cstep = in.ctrl_per_step && in.ctrl;
  const double* crow = in.ctrl ? in.ctrl + r * (cstep ? (size_t)nstep : (size_t)1) * NL : nullptr;
  real gq[KQ], gv[KV], gw[KV], gc[KL];
#pragma unroll
  for (int k = 0; k < KQ; k++) { const int i = sub + G * k, ic = i < NQ ? i : NQ - 1; gq[k] = in.qpos ? in.qpos[r * NQ + ic] : 0.0; }
#pragma unroll
  for (int k = 0; k < KV; k++) {
    const int i = sub + G * k, ic = i < NV ? i : NV - 1;
    gv[k] = in.qvel ? in.qvel[r * NV + ic] : 0.0;
    gw[k] = in.qacc_warm ? in.qacc_warm[r * NV + ic] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < KL; k++) { const int i = sub + G * k, ic = i < NL ? i : NL - 1; gc[k] = crow ? crow[ic] : st.ctrl[(size_t)ic * NE + env]; }
#if KM_VAR_FRC
  // the caller's rows or the env's row of the bound buffer (the launcher picks this build only if one of the two exists)
  const int fv = sub < NV ? sub : NV - 1;
  const bool fstep = in.frc_per_step && in.qfrc_applied;
  const double* frow = in.qfrc_applied ? in.qfrc_applied + r * (fstep ? (size_t)nstep : (size_t)1) * NV
                                       : (st.qfrc_applied ? st.qfrc_applied + (size_t)env * NV : nullptr);
  const real fap = frow ? frow[fv] : 0.0;
#endif
  load_state<NL, G>(w, st, env, sub);
  // the overrides: each lane rewrites the entries it wrote in load_state (the same lane -> index map); ctrl as given / stored
#pragma unroll
  for (int k = 0; k < KQ; k++) { const int i = sub + G * k; if (in.qpos && i < NQ) w.qpos[i] = gq[k]; }
#pragma unroll
  for (int k = 0; k < KV; k++) { const int i = sub + G * k; if (i < NV) { if (in.qvel) w.qvel[i] = gv[k]; if (in.qacc_warm) w.warm[i] = gw[k]; } }
#pragma unroll
  for (int k = 0; k < KL; k++) { const int i = sub + G * k; if (i < NL) w.ctrl[i] = gc[k]; }
  int lb = 0;                          // this lane's reasons for status 1
#pragma unroll
  for (int k = 0; k < KV; k++) { const int i = sub + G * k; if (i < NV) lb |= !isfinite(in.qacc_warm ? gw[k] : w.warm[i]); }
#pragma unroll
  for (int k = 0; k < KL; k++) lb |= !isfinite(gc[k]);      // (lanes past the last actuator hold a copy of it)
#if KM_VAR_FRC
  {                                    // load_applied's test: a row with a non-finite component is stored as zeros and computes nothing
    const int frc_bad = gor<G>(!isfinite(fap));
    if (sub < NV) w.frc[sub] = frc_bad ? 0.0 : fap;
    lb |= frc_bad;
  }
#endif
  GSYNC();
  // a non-finite input of step 0, given or stored: status 1, no step
  if (state_nonfinite<NL, G>(w, sub, lb)) { rollout_finish<NL, G>(out, r, sub, nstep, 0, 1); return; }
  Prof pf;
  pf.start();
  const bool trail = out.contact_mask || out.reward;       // (kernel arguments: uniform over the launch)
  int t = 0, status = 0;
  for (; t < nstep; t++) {
    // the next step's ctrl / force entries, requested now: they arrive under this step's sub-steps
    const bool more = t + 1 < nstep;
    real nc[KL];
#pragma unroll
    for (int k = 0; k < KL; k++) { const int i = sub + G * k, ic = i < NL ? i : NL - 1; nc[k] = (cstep && more) ? crow[(size_t)(t + 1) * NL + ic] : 0.0; }
#if KM_VAR_FRC
    const real nf = (fstep && more) ? frow[(size_t)(t + 1) * NV + fv] : 0.0;
#endif
    int bad = 0;
    for (int s = 0; s < nsub; s++) {
      // k_step's sub-step: the lane's dof index opaque to the optimiser once per sub-step, so that nothing derived from it is hoisted
      // out of the loops and kept alive across them
      int subv = sub; asm volatile("" : "+v"(subv));
      CReg<NL> cr;                     // (one per sub-step: nothing of it can be carried round the loops)
      step1_products<NL, G, SOLVER>(w, lm, m, subv, cr, invm, pf);
      real a = solve<NL, G, SOLVER>(w, lm, m, subv, 1, cr, invm, pf);
      int la = (sub < NV) && (!isfinite(a) || fabs(a) > 1e10);   // mjWARN_BADQACC
      bad = gor<G>(la) | w.bad;
      if (bad) break;
      integrate<NL, G>(w, m, sub, a);
    }
    if (!bad) {
      int lq = 0;
      for (int i = sub; i < NQ; i += G) lq |= !isfinite(w.qpos[i]);
      bad = gor<G>(lq);
    }
    if (bad) { status = 1; break; }
    // ---- the record of step t: lane = component, each row contiguous
    int subr = sub; asm volatile("" : "+v"(subr));
    const size_t e = r * (size_t)nstep + t;
    if (out.qpos) for (int i = subr; i < NQ; i += G) out.qpos[e * NQ + i] = w.qpos[i];
    if (subr < NV) {
      if (out.qvel) out.qvel[e * NV + subr] = w.qvel[subr];
      if (out.qacc_warm) out.qacc_warm[e * NV + subr] = w.warm[subr];
    }
    if (trail) {
      // k_step's trailing mj_step1: kinematics + collision feed the contact mask and the reward
      fk_parallel<NL, G>(w, lm, subr);
      collide_parallel<NL, G>(w, lm, m, subr);
      const real rew = env_reward<NL, G>(w, m, subr);
      if (subr == 0) {
        if (out.contact_mask) out.contact_mask[e] = w.contact_mask;
        if (out.reward) out.reward[e] = rew;
      }
    }
    if (more) {
      // step t + 1's inputs into the workspace; a non-finite entry ends the row here, t + 1 steps recorded
      int ln = 0;
      if (cstep) {
#pragma unroll
        for (int k = 0; k < KL; k++) { const int i = sub + G * k; if (i < NL) w.ctrl[i] = nc[k]; ln |= !isfinite(nc[k]); }
      }
#if KM_VAR_FRC
      if (fstep) {
        const int frc_bad = gor<G>(!isfinite(nf));
        if (sub < NV) w.frc[sub] = frc_bad ? 0.0 : nf;
        ln |= frc_bad;
      }
#endif
      if (sub == 0) { w.bad = 0; w.work = 0; }
      const int stop = gor<G>(ln);
      GSYNC();
      if (stop) { status = 1; t++; break; }
    }
  }
  rollout_finish<NL, G>(out, r, sub, nstep, t, status);
}

template <int NL, int G, int SOLVER>
static void launch_rollout_t(const KDeviceModel* dm, const KDeviceState& st, const KRolloutIn& in, int n, int nstep, int nsub,
                             const KRolloutDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(k_rollout)<NL, G, SOLVER, EPB>), dim3((n + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, in, n, nstep, nsub, out);
}
KM_VARIANT_END
// ---- one (NL, G, SOLVER[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file sixteen times)
void KM_LAUNCHER3(rollout)(const KDeviceModel* dm, const KDeviceState& st, const KRolloutIn& in, int n, int nstep, int nsub,
                           const KRolloutDev& out, hipStream_t stream) {
  launch_rollout_t<KM_VAR_NL, KM_VAR_G, KM_VAR_SOLVER>(dm, st, in, n, nstep, nsub, out, stream);
}
