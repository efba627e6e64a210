// kmanip_inverse.hip -- inverse dynamics of a GIVEN acceleration at every env's state in ONE launch (gfx950, wave64): kmanip_inverse.
//
// MuJoCo's mj_inverse: data.qfrc_inverse = M qacc + qfrc_bias - qfrc_constraint, with the constraint force a closed-form function of
// qacc -- the soft rows' forces at x = J qacc - aref (friction loss saturating at +-floss, limits and pyramid edges one-sided),
// mapped back by J^T.  No solve: it is the J^T f term of the Newton solver's gradient evaluation (newton_eval_sl), evaluated once at
// the caller's qacc.  The device code is the step's own -- the headers of kmanip_dyn.hip, included here under the same build macros:
// step1_products, then mass_mul, row_eval on the lane's own rows, slot_project / slot_eval on the slot lanes, slot_grad -- in a
// translation unit of its own, so that the k_step / k_reset / k_forces / k_observe / k_kinematics objects are the ones they were, to
// the register.  The state is the handle's or, per field, the caller's rows (KInverseIn), used as stored.  Nothing depends on the
// handle's solver: the workspace layout is private to a kernel and the Newton path's constraint assembly reads the model and the
// workspace only, so a PGS handle is served and returns the bits a Newton handle returns.  Both parameter builds, 64 / G envs per
// wave like k_forces.  The handle is read only: nothing of KDeviceState is written.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#define KM_VAR_FRC 0      // (no applied-force builds: a bound force does not enter)
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here)
static_assert(KM_VAR_SOLVER == 1, "k_inverse runs the Newton path's constraint assembly");

// one env's rows of every requested output: lane = dof for the nv-wide rows, lane = slot for the slot rows.
// ok = false: status 1, every value 0, every slot empty.
template <int NL, int G>
__device__ __forceinline__ void write_inverse(const KInverseDev& out, int env, int sub, bool ok, real fi, real fc, const real (&F)[4],
                                              int bit, uint32_t mask) {
  constexpr int NV = Dim<NL>::NV;
  const size_t e = (size_t)env;
  if (sub < NV) {
    if (out.qfrc_inverse) out.qfrc_inverse[e * NV + sub] = ok ? fi : 0.0;
    if (out.qfrc_constraint) out.qfrc_constraint[e * NV + sub] = ok ? fc : 0.0;
  }
  write_slot_rows<NL>(out, e, sub, ok, F, bit);
  if (sub == 0) {
    if (out.contact_mask) out.contact_mask[e] = ok ? mask : 0u;
    if (out.status) out.status[e] = ok ? 0 : 1;
  }
}

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_inverse)(const KDeviceModel* __restrict__ dm, KDeviceState st, KInverseIn in, KInverseDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, NC = Dim<NL>::NC;
  static_assert(NV <= G, "lane = dof");
  static_assert(NC <= 16, "the slot lanes sit in the group's first DPP row");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int env;
  if (!query_env<NL, EPB>(lm, dm, st, grp, env)) return;      // whole group exits together
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  const size_t e = (size_t)env;
  init_ws<NL>(w, sub);            // (query_load's calls, spelt out around the load below)
  env_invm<NL>(w, dm, st, env, sub, invm);
  // the caller's rows, requested before the handle's columns are waited for: this lane's qacc, and the state override
  const real a = sub < NV ? in.qacc[e * NV + sub] : 0.0;
  load_state<NL, G>(w, st, env, sub);
  if (in.qpos) for (int i = sub; i < NQ; i += G) w.qpos[i] = in.qpos[e * NQ + i];      // as stored: what kmanip_set_state_dev would have written
  if (in.qvel) for (int i = sub; i < NV; i += G) w.qvel[i] = in.qvel[e * NV + i];
  GSYNC();
  const real F0[4] = {0, 0, 0, 0};
  // a non-finite state (k_observe's test) or acceleration: status 1, nothing else computed
  if (state_nonfinite<NL, G>(w, sub, !isfinite(a))) { write_inverse<NL, G>(out, env, sub, false, 0, 0, F0, -1, 0u); return; }
  Prof pf;
  pf.start();
  CReg<NL> cr;
  step1_products<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, cr, invm, pf);
  // ---- everything the evaluation reads from LDS in one batch
  const int sv = sub < NV ? sub : NV - 1, cs = sub < NC ? sub : NC - 1;
  real bia = w.bias[sv];
  int sph = w.slot_sph[cs], wbad = w.bad;
  uint32_t act = w.cact, mask = w.contact_mask;
  km_pin(bia); km_pin_i(sph, wbad); asm volatile("" : "+v"(act), "+v"(mask));
  if (wbad) { write_inverse<NL, G>(out, env, sub, false, 0, 0, F0, -1, 0u); return; }      // a failed factorisation of M (group-uniform)
  // ---- one evaluation at the caller's qacc: M a, the lane's own rows, the slots, J^T F
  const real mdiag = (sub >= NL && sub < NV) ? 1.0 / invm : 0.0;
  const real Ma = mass_mul<NL, G>(cr, sub, mdiag, a);
  real fc = 0;
  {
    int q;
    if (cr.fl > 0) { real f; row_eval(0, a - cr.areff, cr.Rf, cr.Df, cr.fl, f, q); fc += f; }
    if (cr.sg != 0) { real f; row_eval(1, cr.sg * a - cr.arefl, cr.Rl, cr.Dl, 0.0, f, q); fc += cr.sg * f; }
  }
  real u[4], F[4], Wd[7];
  slot_project<NL, G, KM_SUB_ALL>(w, cr, act, sub, a, u);
#pragma unroll
  for (int k = 0; k < 4; k++) u[k] -= cr.sc.A[k];
  slot_eval<false>(cr.sc, u, F, Wd);
  real g = 0;
  slot_grad<NL, G, KM_SUB_ALL>(cr, act, F, g);          // g = -J^T F over the active slots
  fc -= g;
  const real fi = sub < NV ? (Ma + bia) - fc : 0.0;
  int bit = -1;      // (the slot lanes: which pair sits in the lane's slot)
  if (sub < NC) bit = slot_contact_bit<NL>(sub, act, mask, sph);
  write_inverse<NL, G>(out, env, sub, true, fi, fc, F, bit, mask);
}

template <int NL, int G>
static void launch_inverse_t(const KDeviceModel* dm, const KDeviceState& st, const KInverseIn& in, const KInverseDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(k_inverse)<NL, G, EPB>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, in, out);
}
KM_VARIANT_END
// ---- one (NL, G[, PAR]) variant per translation unit (the Makefile compiles this file four times)
void KM_LAUNCHER2(inverse)(const KDeviceModel* dm, const KDeviceState& st, const KInverseIn& in, const KInverseDev& out,
                                                     hipStream_t stream) {
  launch_inverse_t<KM_VAR_NL, KM_VAR_G>(dm, st, in, out, stream);
}
