// kmanip_forces.hip -- contact forces, qacc and joint forces of every env's CURRENT state in ONE launch (gfx950, wave64): kmanip_forces.
//
// mj_forward with actuation at (qpos, qvel, ctrl) as stored: what dm_control's physics.forward() followed by data.qacc, data.qfrc_constraint,
// data.qfrc_actuator and mj_contactForce of every contact gives.  The device code is the step's own -- the headers of kmanip_dyn.hip,
// included here under the same build macros: step1_products and then solve once, without integrating, as reset_env does -- in a
// translation unit of its own, so that the k_step / k_reset objects are the ones they were, to the register.  After the solve the
// Newton path holds everything the outputs need:
//   slot forces      slot_project<KM_SUB_ALL> + slot_eval<false> at the final qacc on the lane that owns contact slot c: the sum of the
//                    slot's pyramid-edge forces along its four basis rows (normal, two tangents, torsion) = MuJoCo's mj_contactForce decode
//   qfrc_constraint  mass_mul(qacc - qacc_smooth)
//   qfrc_actuator    the clamp of solve_newton, re-evaluated
// Newton variants only (the PGS path keeps edge forces in LDS records of another layout; kmanip_forces refuses a PGS handle), both
// parameter builds, 64 / G envs per wave like k_observe.  The handle is read only: nothing of KDeviceState is written.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here)
static_assert(KM_VAR_SOLVER == 1, "k_forces reads the Newton path's registers");

// one env's rows of every requested output: lane = dof for the nv- and nu-wide rows, lane = slot for the slot rows.
// ok = false: status 1, every value 0, every slot empty.
template <int NL, int G>
__device__ __forceinline__ void write_forces(const KForcesDev& out, int env, int sub, bool ok, real a, real fc, real fa, const real (&F)[4],
                                             int bit, const real (&fr)[9], const real (&cp)[3], real dist, uint32_t mask) {
  constexpr int NV = Dim<NL>::NV;
  const size_t e = (size_t)env;
  if (sub < NV) {
    if (out.qacc) out.qacc[e * NV + sub] = ok ? a : 0.0;
    if (out.qfrc_constraint) out.qfrc_constraint[e * NV + sub] = ok ? fc : 0.0;
  }
  if (sub < NL && out.qfrc_actuator) out.qfrc_actuator[e * NL + sub] = ok ? fa : 0.0;
  write_slot_rows<NL>(out, e, sub, ok, F, bit, fr, cp, dist);
  if (sub == 0) {
    if (out.contact_mask) out.contact_mask[e] = ok ? mask : 0u;
    if (out.status) out.status[e] = ok ? 0 : 1;
  }
}

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL_FRC_FIRST(forces)(const KDeviceModel* __restrict__ dm, KDeviceState st, KForcesDev out) {
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC;
  static_assert(NC <= 16, "the slot lanes sit in the group's first DPP row");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int env;
  if (!query_env<NL, EPB>(lm, dm, st, grp, env)) return;      // whole group exits together
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  query_load<NL, G>(w, dm, st, env, sub, invm);
  // ctrl exactly as stored: load_state's float32 rounding is the start of before_step, which does not run here
  for (int i = sub; i < NL; i += G) w.ctrl[i] = st.ctrl[(size_t)i * st.num_envs + env];
#if KM_VAR_FRC
  const int frc_bad = load_applied<NL, G>(w, st, env, sub);
#else
  const int frc_bad = 0;
#endif
  GSYNC();
  const real F0[4] = {0, 0, 0, 0}, fr0[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cp0[3] = {0, 0, 0};
  // a non-finite state (k_observe's test) or, in the force builds, a non-finite applied force: status 1, nothing else computed
  if (state_nonfinite<NL, G>(w, sub, frc_bad)) { write_forces<NL, G>(out, env, sub, false, 0, 0, 0, F0, -1, fr0, cp0, 0, 0u); return; }
  Prof pf;
  pf.start();
  CReg<NL> cr;
  step1_products<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, cr, invm, pf);
  const real a = solve<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, 1, cr, invm, pf);
  {                                                    // a failed factorisation or mjWARN_BADQACC, as k_step tests it
    const int la = (sub < NV) && (!isfinite(a) || fabs(a) > 1e10);
    if (gor<G>(la) | w.bad) { write_forces<NL, G>(out, env, sub, false, 0, 0, 0, F0, -1, fr0, cp0, 0, 0u); return; }
  }
  // ---- everything the outputs read from LDS in one batch: solve_newton's inputs again (its right-hand sides are still in w.tmp,
  // M^-1 in w.Minv), this lane's slot geometry
  const int si = sub < NL ? sub : NL - 1, sv = sub < NV ? sub : NV - 1, cs = sub < NC ? sub : NC - 1;
  real ctl = w.ctrl[si], cr0 = lm.ctrlrange[si][0], cr1 = lm.ctrlrange[si][1], kpv = KM_EP_KP(w, lm, si), qps = w.qpos[si];
  real fr0_ = lm.forcerange[si][0], fr1_ = lm.forcerange[si][1], rhs = w.tmp[sv];
  const int flim = lm.forcelimited[si];
  real mrow[NL], tv[NL], fr[9], cp[3];
#pragma unroll
  for (int j = 0; j < NL; j++) { mrow[j] = w.Minv[si][j]; tv[j] = w.tmp[j]; }
#pragma unroll
  for (int k = 0; k < 9; k++) fr[k] = w.c_frame[cs][k];
#pragma unroll
  for (int k = 0; k < 3; k++) cp[k] = w.c_pos[cs][k];
  const real dist = w.c_dist[cs];
  const int sph = w.slot_sph[cs];
  const uint32_t act = w.cact, mask = w.contact_mask;
  // qacc_smooth as solve_newton formed it, then qfrc_constraint = M (qacc - qacc_smooth)
  real a_s = 0;
  if (sub < NL) {
#pragma unroll
    for (int j = 0; j < NL; j++) a_s += mrow[j] * tv[j];
  } else if (sub < NV) a_s = rhs * invm;
  const real mdiag = (sub >= NL && sub < NV) ? 1.0 / invm : 0.0;
  const real fc = mass_mul<NL, G>(cr, sub, mdiag, sub < NV ? a - a_s : 0.0);
  // the servo force: solve_newton's clamp
  real fa = kpv * fmin(fmax(ctl, cr0), cr1) - kpv * qps;
  if (flim) fa = fmin(fmax(fa, fr0_), fr1_);
  // the slot forces at the final qacc, on the slot lanes (two-row groups: of the first DPP row -- lanes sub < NC)
  real u[4], F[4], Wd[7];
  slot_project<NL, G, KM_SUB_ALL>(w, cr, act, sub, a, u);
#pragma unroll
  for (int k = 0; k < 4; k++) u[k] -= cr.sc.A[k];
  slot_eval<false>(cr.sc, u, F, Wd);
  int bit = -1;      // (the slot lanes: which pair sits in the lane's slot)
  if (sub < NC) bit = slot_contact_bit<NL>(sub, act, mask, sph);
  write_forces<NL, G>(out, env, sub, true, a, fc, fa, F, bit, fr, cp, dist, mask);
}

template <int NL, int G>
static void launch_forces_t(const KDeviceModel* dm, const KDeviceState& st, const KForcesDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL_FRC_FIRST(forces)<NL, G, EPB>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, out);
}
KM_VARIANT_END
// ---- one (NL, G[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file eight times)
void KM_LAUNCHER2(forces)(const KDeviceModel* dm, const KDeviceState& st, const KForcesDev& out, hipStream_t stream) {
  launch_forces_t<KM_VAR_NL, KM_VAR_G>(dm, st, out, stream);
}
