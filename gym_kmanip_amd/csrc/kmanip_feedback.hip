// kmanip_feedback.hip -- closed-loop rollouts in ctrl space from rows the CALLER passes, in ONE launch (gfx950, wave64):
// kmanip_feedback, the sibling of kmanip_rollout (kmanip_rollout.hip) with a time-varying affine state feedback evaluated at every
// step boundary, t = 0 included:
//   dx  = [ tangent_diff(qpos, qpos_ref[g, t]) ; qvel - qvel_ref[g, t] ]                       (2 nv)
//   u_i = ctrl[r, t, i] + sum_j gain_t[g, t, j, i] dx_j              (j ascending, an FMA chain from 0, then one add)
// g = gain_index[r] (NULL: r), the policy an iLQR backward pass returns, a regulator (the one gain held) or the stabilising
// feedback under MPPI samples.  u replaces the step's ctrl in the workspace and is recorded, unclamped, with the step; everything
// else -- the entry (row_env, row_load), the sub-step loop, the trailing pass, status and steps_done, the zero tail, the next
// step's open-loop ctrl / force requested under the current one -- is k_rollout's body (DESIGN.md sections 27 and 29).
// The gain is stored TRANSPOSED, [2 nv, nu]: lane = actuator, so the lanes of a group read consecutive addresses for every j; each
// lane requests its 2 nv entries before the tangent difference is computed, and they are dead before the first sub-step starts
// (the 20-link Newton variant has no room for 52 doubles across the loop).  dx goes through a small LDS array of this unit's own
// (Ws is every kernel's and stays as it is); the lanes of a group read the same dx_j: a broadcast.
// A translation unit of its own over the same headers, so that every other object is the one it was, to the register.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load: shared with k_forward and k_rollout)

// zero records of steps t0 .. nstep-1 of one row (a row that stopped, or never started), then its status and step count
template <int NL, int G>
__device__ __forceinline__ void feedback_finish(const KFeedbackDev& out, size_t row, int sub, int nstep, int t0, int status) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  for (int t = t0; t < nstep; t++) {
    const size_t e = row * (size_t)nstep + t;
    if (out.qpos) for (int i = sub; i < NQ; i += G) out.qpos[e * NQ + i] = 0.0;
    if (sub < NV) {
      if (out.qvel) out.qvel[e * NV + sub] = 0.0;
      if (out.qacc_warm) out.qacc_warm[e * NV + sub] = 0.0;
    }
    if (sub < NL && out.ctrl) out.ctrl[e * NL + sub] = 0.0;
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

// The rotation part of derivatives.tangent_diff (MuJoCo's mj_differentiatePos): the body-frame log of conj(a) (x) b, a = the
// reference's quaternion, b = the state's, operation for operation as the Python spells it.  No contraction: the vector part is two
// differences of separately rounded products, so that equal quaternions give exactly zero (with an FMA, wa xb - xa wb would be the
// rounding error of a product).
__device__ __forceinline__ void quat_log_diff(const real (&a)[4], const real (&b)[4], real (&r)[3]) {
#pragma clang fp contract(off)
  const real wa = a[0], xa = a[1], ya = a[2], za = a[3], wb = b[0], xb = b[1], yb = b[2], zb = b[3];
  const real w = ((wa * wb + xa * xb) + ya * yb) + za * zb;
  const real x = (wa * xb - xa * wb) + (za * yb - ya * zb);
  const real y = (wa * yb - ya * wb) + (xa * zb - za * xb);
  const real z = (wa * zb - za * wb) + (ya * xb - xa * yb);
  const real s = sqrt((x * x + y * y) + z * z);
  real ang = 2.0 * atan2(s, w);
  if (ang > 3.141592653589793) ang = ang - 6.283185307179586;
  // angle / sin(angle / 2) -> 2 / w as the vector part vanishes
  const real k = s > 0 ? ang / s : 2.0 / (w != 0 ? w : 1.0);
  r[0] = k * x; r[1] = k * y; r[2] = k * z;
}

template <int NL, int G, int SOLVER, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_feedback)(const KDeviceModel* __restrict__ dm, KDeviceState st, KFeedbackIn in, int n, int nstep,
                                                            int nsub, KFeedbackDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, KQ = (NQ + G - 1) / G, NX = 2 * NV;
  static_assert(NL <= G && NV <= G, "lane = actuator, lane = dof");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  __shared__ real dxs[EPB][NX];        // the policy's state difference, per row
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int row, env;
  if (!row_env<NL, EPB>(lm, dm, in, n, grp, row, env)) return;      // whole group exits together
  const size_t r = (size_t)row;
  // the gain trajectory of the row, and the env: indices outside their range (group-uniform) are never used as addresses
  const int g = in.gain_index ? in.gain_index[row] : row;
  if (env < 0 || env >= st.num_envs || g < 0 || g >= in.ng) { feedback_finish<NL, G>(out, r, sub, nstep, 0, 2); return; }
  Ws<NL>& w = ws[grp];
  real* dx = dxs[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  init_ws<NL>(w, sub);
  env_invm<NL>(w, dm, st, env, sub, invm);
  const bool cstep = in.ctrl_per_step && in.ctrl, fstep = in.frc_per_step && in.qfrc_applied;
  const double* crow = in.ctrl ? in.ctrl + r * (cstep ? (size_t)nstep : (size_t)1) * NL : nullptr;
  const double* frow = in.qfrc_applied ? in.qfrc_applied + r * (fstep ? (size_t)nstep : (size_t)1) * NV : nullptr;
  const int lb = row_load<NL, G>(w, st, in, r, env, sub, crow, frow);
  // a non-finite input of step 0, given or stored: status 1, no step
  if (state_nonfinite<NL, G>(w, sub, lb)) { feedback_finish<NL, G>(out, r, sub, nstep, 0, 1); return; }
  // this lane's actuator (lanes past the last hold a copy of it) and dof, and the open-loop term of step 0: what row_load stored
  const int ia = sub < NL ? sub : NL - 1, iv = sub < NV ? sub : NV - 1;
  real oc = w.ctrl[ia];
  // entry (g, t) of the references and the gain: t = 0 throughout while one gain is held
  const size_t gT = (size_t)g * (in.gain_per_step ? (size_t)nstep : (size_t)1);
  Prof pf;
  pf.start();
  const bool trail = out.contact_mask || out.reward;       // (kernel arguments: uniform over the launch)
  int t = 0, status = 0;
  for (; t < nstep; t++) {
    // the next step's open-loop ctrl / force entries, requested now: they arrive under this step's sub-steps (a held ctrl is
    // simply asked for again: the policy overwrites the workspace's copy every step)
    const bool more = t + 1 < nstep;
    real nc = 0.0;
    if (more) nc = crow ? crow[(cstep ? (size_t)(t + 1) * NL : (size_t)0) + ia] : st.ctrl[(size_t)ia * st.num_envs + env];
#if KM_VAR_FRC
    const real nf = (fstep && more) ? frow[(size_t)(t + 1) * NV + iv] : 0.0;
#endif
    // ---- the policy at the start of step t
    {
      const size_t gt = gT + (in.gain_per_step ? (size_t)t : (size_t)0);
      // this actuator's column of the transposed gain, all 2 nv entries requested together, ahead of the arithmetic below
      const double* kcol = in.gain_t + gt * NX * NL + ia;
      real kg[NX];
#pragma unroll
      for (int j = 0; j < NX; j++) kg[j] = kcol[(size_t)j * NL];
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
      if (sub < NL) w.ctrl[sub] = u;
      GSYNC();
    }
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
    // ---- the record of step t: lane = component, each row contiguous; the ctrl that acted is the workspace's
    int subr = sub; asm volatile("" : "+v"(subr));
    const size_t e = r * (size_t)nstep + t;
    if (out.qpos) for (int i = subr; i < NQ; i += G) out.qpos[e * NQ + i] = w.qpos[i];
    if (subr < NV) {
      if (out.qvel) out.qvel[e * NV + subr] = w.qvel[subr];
      if (out.qacc_warm) out.qacc_warm[e * NV + subr] = w.warm[subr];
    }
    if (subr < NL && out.ctrl) out.ctrl[e * NL + subr] = w.ctrl[subr];
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
      // step t + 1's open-loop inputs; a non-finite entry ends the row here, t + 1 steps recorded
      oc = nc;
      int ln = !isfinite(nc);
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
  feedback_finish<NL, G>(out, r, sub, nstep, t, status);
}

template <int NL, int G, int SOLVER>
static void launch_feedback_t(const KDeviceModel* dm, const KDeviceState& st, const KFeedbackIn& in, int n, int nstep, int nsub,
                              const KFeedbackDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(k_feedback)<NL, G, SOLVER, EPB>), dim3((n + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, in, n, nstep, nsub, out);
}
KM_VARIANT_END
// ---- one (NL, G, SOLVER[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file sixteen times)
void KM_LAUNCHER3(feedback)(const KDeviceModel* dm, const KDeviceState& st, const KFeedbackIn& in, int n, int nstep, int nsub,
                            const KFeedbackDev& out, hipStream_t stream) {
  launch_feedback_t<KM_VAR_NL, KM_VAR_G, KM_VAR_SOLVER>(dm, st, in, n, nstep, nsub, out, stream);
}
