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
// (row_env, row_load), written once for both in kmanip_dyn_rows.hpp, a header only those units and kmanip_forces.hip include: a helper
// moved into the common headers reorders the code of the other kernels.  A translation unit of its own, so
// that the step's and the state queries' objects are the ones they were, to the register.
// One wave per workgroup, 64 / G ROWS per wave; the state stays in LDS for all nstep x nsub sub-steps.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load: shared with k_forward)

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
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, KL = (NL + G - 1) / G;
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int row, env;
  if (!row_env<NL, EPB>(lm, dm, in, n, grp, row, env)) return;      // whole group exits together
  const size_t r = (size_t)row;
  // an index outside the handle (group-uniform): never used as an address
  if (env < 0 || env >= st.num_envs) { rollout_finish<NL, G>(out, r, sub, nstep, 0, 2); return; }
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  init_ws<NL>(w, sub);            // (query_load's calls, row_load in load_state's place)
  env_invm<NL>(w, dm, st, env, sub, invm);
  // the caller's rows of ctrl and the force, held or step 0's: row (r, t) of a per-step tensor is row r * nstep + t
  // (a per-step flag counts only with the caller's own tensor: kmanip_rollout refuses it on a NULL one)
  const bool cstep = in.ctrl_per_step && in.ctrl, fstep = in.frc_per_step && in.qfrc_applied;
  const double* crow = in.ctrl ? in.ctrl + r * (cstep ? (size_t)nstep : (size_t)1) * NL : nullptr;
  const double* frow = in.qfrc_applied ? in.qfrc_applied + r * (fstep ? (size_t)nstep : (size_t)1) * NV : nullptr;
  const int lb = row_load<NL, G>(w, st, in, r, env, sub, crow, frow);
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
    const real nf = (fstep && more) ? frow[(size_t)(t + 1) * NV + (sub < NV ? sub : NV - 1)] : 0.0;
#endif
    int bad = 0;
    for (int s = 0; s < nsub; s++) {
      // k_step's sub-step: the lane's dof index opaque to the optimiser once per sub-step, so that nothing derived from it is hoisted
      // out of the loops and kept alive across them
      int subv = sub; asm volatile("" : "+v"(subv));
      CReg<NL> cr;                     // (one per sub-step: nothing of it can be carried round the loops)
      step1_products<NL, G, SOLVER>(w, lm, m, subv, cr, invm, pf);
      real a = solve<NL, G, SOLVER>(w, lm, m, subv, 1, cr, invm, pf);
      // bad_qacc (kmanip_dyn_rows.hpp), spelt out: through the helper the two-arm kernels' loop is scheduled differently
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
