// kmanip_rollout.hip -- rollouts in ctrl space from rows the CALLER passes, as many as it likes, in ONE launch (gfx950, wave64): the
// source of three kernels, open-loop kmanip_rollout (k_rollout), compiled with -DKM_VAR_FB=1 closed-loop kmanip_feedback (k_feedback)
// and, with -DKM_VAR_FB=2, kmanip_feedback_box (k_boxfb): k_feedback with the policy's output clamped to a box.
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
//
// KM_VAR_FB=1 adds a time-varying affine state feedback evaluated at every step boundary, t = 0 included:
//   dx  = [ tangent_diff(qpos, qpos_ref[g, t]) ; qvel - qvel_ref[g, t] ]                       (2 nv)
//   u_i = ctrl[r, t, i] + sum_j gain_t[g, t, j, i] dx_j              (j ascending, an FMA chain from 0, then one add)
// g = gain_index[r] (NULL: r), the policy an iLQR backward pass returns, a regulator (the one gain held) or the stabilising
// feedback under MPPI samples.  u replaces the step's ctrl in the workspace and is recorded, unclamped, with the step; everything
// else -- the entry, the sub-step loop, the trailing pass, status and steps_done, the zero tail, the next step's open-loop force
// requested under the current one -- is written once below for both kernels (DESIGN.md sections 27, 29 and 30): the feedback-only
// statements stand in #if KM_VAR_FB regions, so that each object still sees, after preprocessing, the statements of its kernel alone.
// The gain is stored TRANSPOSED, [2 nv, nu]: lane = actuator, so the lanes of a group read consecutive addresses for every j; each
// lane requests its 2 nv entries before the tangent difference is computed, and they are dead before the first sub-step starts
// (the 20-link Newton variant has no room for 52 doubles across the loop).  dx goes through a small LDS array of this unit's own
// (Ws is every kernel's and stays as it is); the lanes of a group read the same dx_j: a broadcast.
//
// KM_VAR_FB=2 is KM_VAR_FB=1 with  u_i = min(max(u_i, lo[b, i]), hi[b, i]),  b = box_per_traj ? g : 0,  after the finite-u test
// (DESIGN.md section 39): the clamped u acts and is recorded.  The lane's two bounds are requested with its gain column, every step:
// nothing of the box is kept across the sub-steps.  A box with lo_i <= hi_i false stops the row before its first step, status 1.
// The clamp statements stand in #if KM_VAR_FB == 2 regions of their own: k_feedback's text after preprocessing is what it was.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load: shared with k_forward; quat_log_diff: with k_transfd)

// KM_VAR_FB=1: the closed-loop build of this unit (the Makefile's kmanip_feedback_* objects), next to KM_VAR_PAR and KM_VAR_FRC.  It
// names the structs (KFeedbackIn / KFeedbackDev begin with KRolloutIn's / KRolloutDev's fields), the kernel and the launcher.
#ifndef KM_VAR_FB
#define KM_VAR_FB 0
#endif
#if KM_VAR_FB == 2
typedef KFeedbackBoxIn RollIn;
typedef KFeedbackDev RollDev;
#define KM_ROLL_KERNEL k_boxfb
#define KM_ROLL_LAUNCHER KM_LAUNCHER3(boxfb)
#elif KM_VAR_FB
typedef KFeedbackIn RollIn;
typedef KFeedbackDev RollDev;
#define KM_ROLL_KERNEL k_feedback
#define KM_ROLL_LAUNCHER KM_LAUNCHER3(feedback)
#else
typedef KRolloutIn RollIn;
typedef KRolloutDev RollDev;
#define KM_ROLL_KERNEL k_rollout
#define KM_ROLL_LAUNCHER KM_LAUNCHER3(rollout)
#endif

// zero records of steps t0 .. nstep-1 of one row (a row that stopped, or never started), then its status and step count
template <int NL, int G>
__device__ __forceinline__ void rollout_finish(const RollDev& out, size_t row, int sub, int nstep, int t0, int status) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  for (int t = t0; t < nstep; t++) {
    const size_t e = row * (size_t)nstep + t;
    if (out.qpos) for (int i = sub; i < NQ; i += G) out.qpos[e * NQ + i] = 0.0;
    if (sub < NV) {
      if (out.qvel) out.qvel[e * NV + sub] = 0.0;
      if (out.qacc_warm) out.qacc_warm[e * NV + sub] = 0.0;
    }
#if KM_VAR_FB
    if (sub < NL && out.ctrl) out.ctrl[e * NL + sub] = 0.0;
#endif
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
__global__ __launch_bounds__(64) void KM_KERNEL(KM_ROLL_KERNEL)(const KDeviceModel* __restrict__ dm, KDeviceState st, RollIn in, int n, int nstep,
                                                                int nsub, RollDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
#if KM_VAR_FB
  constexpr int KQ = (NQ + G - 1) / G, NX = 2 * NV;
  static_assert(NL <= G && NV <= G, "lane = actuator, lane = dof");
  __shared__ real dxs[EPB][NX];        // the policy's state difference, per row
  real* dx = dxs[grp];
#endif
  int row, env;
  if (!row_env<NL, EPB>(lm, dm, in, n, grp, row, env)) return;      // whole group exits together
  const size_t r = (size_t)row;
  // an index outside the handle (group-uniform): never used as an address
#if KM_VAR_FB
  // (likewise the row's gain trajectory outside its range)
  const int g = in.gain_index ? in.gain_index[row] : row;
  if (env < 0 || env >= st.num_envs || g < 0 || g >= in.ng) { rollout_finish<NL, G>(out, r, sub, nstep, 0, 2); return; }
#else
  if (env < 0 || env >= st.num_envs) { rollout_finish<NL, G>(out, r, sub, nstep, 0, 2); return; }
#endif
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  init_ws<NL>(w, sub);            // (query_load's calls, row_load in load_state's place)
  env_invm<NL>(w, dm, st, env, sub, invm);
  // the caller's rows of ctrl and the force, held or step 0's: row (r, t) of a per-step tensor is row r * nstep + t
  // (a per-step flag counts only with the caller's own tensor: the host entry refuses it on a NULL one)
  const bool cstep = in.ctrl_per_step && in.ctrl, fstep = in.frc_per_step && in.qfrc_applied;
  const double* crow = in.ctrl ? in.ctrl + r * (cstep ? (size_t)nstep : (size_t)1) * NL : nullptr;
  const double* frow = in.qfrc_applied ? in.qfrc_applied + r * (fstep ? (size_t)nstep : (size_t)1) * NV : nullptr;
  const int lb = row_load<NL, G>(w, st, in, r, env, sub, crow, frow);
  // a non-finite input of step 0, given or stored: status 1, no step
  if (state_nonfinite<NL, G>(w, sub, lb)) { rollout_finish<NL, G>(out, r, sub, nstep, 0, 1); return; }
#if KM_VAR_FB
  // this lane's actuator (lanes past the last hold a copy of it) and dof, and the open-loop term of step 0: what row_load stored
  const int ia = sub < NL ? sub : NL - 1, iv = sub < NV ? sub : NV - 1;
  real oc = w.ctrl[ia];
  // entry (g, t) of the references and the gain: t = 0 throughout while one gain is held
  const size_t gT = (size_t)g * (in.gain_per_step ? (size_t)nstep : (size_t)1);
#endif
#if KM_VAR_FB == 2
  // this actuator's bounds: an empty box or a NaN bound anywhere in the row's box is status 1, no step
  const size_t bx = (in.box_per_traj ? (size_t)g : (size_t)0) * NL + ia;
  if (gor<G>(!(in.lo[bx] <= in.hi[bx]))) { rollout_finish<NL, G>(out, r, sub, nstep, 0, 1); return; }
#endif
  Prof pf;
  pf.start();
  const bool trail = out.contact_mask || out.reward;       // (kernel arguments: uniform over the launch)
  int t = 0, status = 0;
  for (; t < nstep; t++) {
    // the next step's open-loop ctrl / force entries, requested now: they arrive under this step's sub-steps
    const bool more = t + 1 < nstep;
#if KM_VAR_FB
    // (a held ctrl is simply asked for again: the policy overwrites the workspace's copy every step)
    real nc = 0.0;
    if (more) nc = crow ? crow[(cstep ? (size_t)(t + 1) * NL : (size_t)0) + ia] : st.ctrl[(size_t)ia * st.num_envs + env];
#else
    constexpr int KL = (NL + G - 1) / G;
    real nc[KL];
#pragma unroll
    for (int k = 0; k < KL; k++) { const int i = sub + G * k, ic = i < NL ? i : NL - 1; nc[k] = (cstep && more) ? crow[(size_t)(t + 1) * NL + ic] : 0.0; }
#endif
#if KM_VAR_FRC
    const real nf = (fstep && more) ? frow[(size_t)(t + 1) * NV + (sub < NV ? sub : NV - 1)] : 0.0;
#endif
#if KM_VAR_FB
    // ---- the policy at the start of step t
    {
      const size_t gt = gT + (in.gain_per_step ? (size_t)t : (size_t)0);
      // this actuator's column of the transposed gain, all 2 nv entries requested together, ahead of the arithmetic below
      const double* kcol = in.gain_t + gt * NX * NL + ia;
      real kg[NX];
#pragma unroll
      for (int j = 0; j < NX; j++) kg[j] = kcol[(size_t)j * NL];
#if KM_VAR_FB == 2
      const real bl = in.lo[bx], bh = in.hi[bx];
#endif
      const double* qr = in.qpos_ref + gt * NQ;
      real rq[KQ], ra[4], qb[4], rot[3];
#pragma unroll
      for (int k = 0; k < KQ; k++) { const int i = sub + G * k; rq[k] = qr[i < NQ ? i : NQ - 1]; }
      const real rv = in.qvel_ref[gt * NV + iv];
#pragma unroll
      for (int k = 0; k < 4; k++) { ra[k] = qr[NL + 3 + k]; qb[k] = w.qpos[NL + 3 + k]; }
      // joints and cube position: lane = coordinate; the rotation: every lane computes it, lanes 0 .. 2 store it; qvel: lane = dof
#pragma unroll
      for (int k = 0; k < KQ; k++) { const int i = sub + G * k; if (i < NL + 3) dx[i] = w.qpos[i] - rq[k]; }
      quat_log_diff(ra, qb, rot);
      if (sub < 3) dx[NL + 3 + sub] = rot[sub];
      if (sub < NV) dx[NV + sub] = w.qvel[sub] - rv;
      GSYNC();
      real acc = 0.0;
#pragma unroll
      for (int j = 0; j < NX; j++) acc = fma(kg[j], dx[j], acc);
      const real u = oc + acc;
      // a non-finite u (a non-finite reference or gain entry the row uses, or an overflow): the row stops, t steps recorded
      if (gor<G>(!isfinite(u))) { status = 1; break; }
#if KM_VAR_FB == 2
      if (sub < NL) w.ctrl[sub] = fmin(fmax(u, bl), bh);
#else
      if (sub < NL) w.ctrl[sub] = u;
#endif
      GSYNC();
    }
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
#if KM_VAR_FB
    if (subr < NL && out.ctrl) out.ctrl[e * NL + subr] = w.ctrl[subr];      // (the ctrl that acted is the workspace's)
#endif
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
      // step t + 1's open-loop inputs (into the workspace, or kept for the policy); a non-finite entry ends the row here, t + 1
      // steps recorded
#if KM_VAR_FB
      oc = nc;
      int ln = !isfinite(nc);
#else
      int ln = 0;
      if (cstep) {
#pragma unroll
        for (int k = 0; k < KL; k++) { const int i = sub + G * k; if (i < NL) w.ctrl[i] = nc[k]; ln |= !isfinite(nc[k]); }
      }
#endif
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
static void launch_rollout_t(const KDeviceModel* dm, const KDeviceState& st, const RollIn& in, int n, int nstep, int nsub, const RollDev& out,
                             hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(KM_ROLL_KERNEL)<NL, G, SOLVER, EPB>), dim3((n + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, in, n, nstep, nsub, out);
}
KM_VARIANT_END
// ---- one (NL, G, SOLVER[, PAR][, FRC][, FB]) variant per translation unit (the Makefile compiles this file forty-eight times)
void KM_ROLL_LAUNCHER(const KDeviceModel* dm, const KDeviceState& st, const RollIn& in, int n, int nstep, int nsub, const RollDev& out,
                      hipStream_t stream) {
  launch_rollout_t<KM_VAR_NL, KM_VAR_G, KM_VAR_SOLVER>(dm, st, in, n, nstep, nsub, out, stream);
}
