// kmanip_forward.hip -- contact forces, qacc and joint forces at rows the CALLER passes, as many as it likes, in ONE launch (gfx950,
// wave64): kmanip_forward.
//
// mj_forward with actuation on a scratch mjData: row r names an env (KForwardIn::env_index; NULL = row r is env r), takes that env's
// model parameters and, per field, either the caller's row r of qpos / qvel / ctrl / qacc_warm / qfrc_applied or what the env stores
// (the bound applied force for the last).  Nothing of the handle is written, so a planner evaluates K hypotheses per env without
// cloning K n envs.  The device code is k_forces' (kmanip_forces.hip), which is the step's own -- the headers of kmanip_dyn.hip,
// included here under the same build macros: step1_products, solve once without integrating, then the decode of the Newton path's
// registers into the outputs (forces_decode, written once for both kernels in kmanip_dyn_rows.hpp, a header only these units and
// kmanip_rollout.hip include: a helper moved into the common headers reorders the code of the other kernels) --
// in a translation unit of its own, so that the k_step / k_reset / k_observe / k_kinematics / k_inverse objects are the ones they
// were, to the register.  The entry over rows (row_env, row_load) is that header's too.  With every input NULL and n = num_envs a row
// computes what k_forces computes for that env.  Newton variants only (kmanip_forward refuses a PGS handle), both parameter builds
// and both applied-force builds, 64 / G ROWS per wave.  The outputs are written at the row, not at the env.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here)
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load: shared with k_rollout; forces_decode, write_forces_row, bad_qacc: with k_forces)
static_assert(KM_VAR_SOLVER == 1, "k_forward reads the Newton path's registers");

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_forward)(const KDeviceModel* __restrict__ dm, KDeviceState st, KForwardIn in, int n, KForcesDev out) {
  constexpr int NV = Dim<NL>::NV;
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int row, env;
  if (!row_env<NL, EPB>(lm, dm, in, n, grp, row, env)) return;      // whole group exits together
  // an index outside the handle (group-uniform): never used as an address
  if (env < 0 || env >= st.num_envs) { write_forces_row<NL>(out, row, sub, 2); return; }
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  const size_t r = (size_t)row;
  init_ws<NL>(w, sub);            // (query_load's calls, row_load in load_state's place)
  env_invm<NL>(w, dm, st, env, sub, invm);
  const int lb = row_load<NL, G>(w, st, in, r, env, sub, in.ctrl ? in.ctrl + r * NL : nullptr,
                                 in.qfrc_applied ? in.qfrc_applied + r * NV : nullptr);
  // a non-finite input, given or stored (k_observe's test of the state, and ctrl, the warm start and the force): status 1, nothing
  // else computed
  if (state_nonfinite<NL, G>(w, sub, lb)) { write_forces_row<NL>(out, row, sub, 1); return; }
  Prof pf;
  pf.start();
  CReg<NL> cr;
  step1_products<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, cr, invm, pf);
  const real a = solve<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, 1, cr, invm, pf);
  if (bad_qacc<NL, G>(w, sub, a)) { write_forces_row<NL>(out, row, sub, 1); return; }
  write_forces_row<NL>(out, row, sub, 0, a, forces_decode<NL, G>(w, lm, cr, sub, invm, a));
}

template <int NL, int G>
static void launch_forward_t(const KDeviceModel* dm, const KDeviceState& st, const KForwardIn& in, int n, const KForcesDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(k_forward)<NL, G, EPB>), dim3((n + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, in, n, out);
}
KM_VARIANT_END
// ---- one (NL, G[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file eight times)
void KM_LAUNCHER2(forward)(const KDeviceModel* dm, const KDeviceState& st, const KForwardIn& in, int n, const KForcesDev& out, hipStream_t stream) {
  launch_forward_t<KM_VAR_NL, KM_VAR_G>(dm, st, in, n, out, stream);
}
