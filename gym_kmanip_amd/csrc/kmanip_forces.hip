// kmanip_forces.hip -- contact forces, qacc and joint forces of every env's CURRENT state in ONE launch (gfx950, wave64): kmanip_forces.
//
// mj_forward with actuation at (qpos, qvel, ctrl) as stored: what dm_control's physics.forward() followed by data.qacc, data.qfrc_constraint,
// data.qfrc_actuator and mj_contactForce of every contact gives.  The device code is the step's own -- the headers of kmanip_dyn.hip,
// included here under the same build macros: step1_products and then solve once, without integrating, as reset_env does -- in a
// translation unit of its own, so that the k_step / k_reset objects are the ones they were, to the register.  After the solve the
// Newton path holds everything the outputs need (forces_decode, kmanip_dyn_rows.hpp: shared with k_forward):
//   slot forces      slot_project<KM_SUB_ALL> + slot_eval<false> at the final qacc on the lane that owns contact slot c: the sum of the
//                    slot's pyramid-edge forces along its four basis rows (normal, two tangents, torsion) = MuJoCo's mj_contactForce decode
//   qfrc_constraint  mass_mul(qacc - qacc_smooth)
//   qfrc_actuator    the clamp of solve_newton, re-evaluated
// Newton variants only (the PGS path keeps edge forces in LDS records of another layout; kmanip_forces refuses a PGS handle), both
// parameter builds, 64 / G envs per wave like k_observe.  The handle is read only: nothing of KDeviceState is written.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here)
#include "kmanip_dyn_rows.hpp"         // (forces_decode, write_forces_row, bad_qacc: shared with k_forward)
static_assert(KM_VAR_SOLVER == 1, "k_forces reads the Newton path's registers");

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL_FRC_FIRST(forces)(const KDeviceModel* __restrict__ dm, KDeviceState st, KForcesDev out) {
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
  // a non-finite state (k_observe's test) or, in the force builds, a non-finite applied force: status 1, nothing else computed
  if (state_nonfinite<NL, G>(w, sub, frc_bad)) { write_forces_row<NL>(out, env, sub, 1); return; }
  Prof pf;
  pf.start();
  CReg<NL> cr;
  step1_products<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, cr, invm, pf);
  const real a = solve<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, 1, cr, invm, pf);
  if (bad_qacc<NL, G>(w, sub, a)) { write_forces_row<NL>(out, env, sub, 1); return; }
  write_forces_row<NL>(out, env, sub, 0, a, forces_decode<NL, G>(w, lm, cr, sub, invm, a));
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
