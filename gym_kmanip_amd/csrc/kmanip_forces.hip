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
// ---- the build macros of kmanip_dyn.hip (the headers below read them); KM_VAR_SOLVER is always 1 here
#ifndef KM_VAR_PAR
#define KM_VAR_PAR 0
#endif
// KM_VAR_FRC=1: the applied-force builds (kmanip_bind_applied_force), as in kmanip_dyn.hip
#ifndef KM_VAR_FRC
#define KM_VAR_FRC 0
#endif
#if KM_VAR_PAR && KM_VAR_FRC
namespace km_envp_frc {
#define KM_K_FORCES k_frc_forces_ep
#elif KM_VAR_FRC
namespace km_frc {
#define KM_K_FORCES k_frc_forces      // ("frc" first: tools that list the k_forces kernels by name keep seeing the default four)
#elif KM_VAR_PAR
namespace km_envp {
#define KM_K_FORCES k_forces_ep
#else
#define KM_K_FORCES k_forces
#endif
#define KM_TREE_UNROLL(NL) NL <= 10 ? NL : 1
#ifdef KM_WORK_COUNTERS_ALL
#define KM_WORK_COUNTERS(NL) true
#else
#define KM_WORK_COUNTERS(NL) ((NL) > 10)
#endif
#define KM_WORK_ALL 40
#define KM_WORK_ARM 14
#define KM_WORK_PLAIN 3
#define KM_WORK_CUBE 5
#include "kmanip_dyn_ws.hpp"
#include "kmanip_dyn_tree.hpp"
#include "kmanip_dyn_constraints.hpp"
#include "kmanip_dyn_newton.hpp"
#include "kmanip_dyn_env.hpp"
static_assert(KM_VAR_SOLVER == 1, "k_forces reads the Newton path's registers");

// one env's rows of every requested output: lane = dof for the nv- and nu-wide rows, lane = slot for the slot rows.
// ok = false: status 1, every value 0, every slot empty.
template <int NL, int G>
__device__ __forceinline__ void write_forces(const KForcesDev& out, int env, int sub, bool ok, real a, real fc, real fa, const real (&F)[4],
                                             int bit, const real (&fr)[9], const real (&cp)[3], real dist, uint32_t mask) {
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC;
  const size_t e = (size_t)env;
  if (sub < NV) {
    if (out.qacc) out.qacc[e * NV + sub] = ok ? a : 0.0;
    if (out.qfrc_constraint) out.qfrc_constraint[e * NV + sub] = ok ? fc : 0.0;
  }
  if (sub < NL && out.qfrc_actuator) out.qfrc_actuator[e * NL + sub] = ok ? fa : 0.0;
  if (sub < NC) {
    const size_t s = e * NC + sub;
    const bool on = ok && bit >= 0;
    if (out.contact_force) {
#pragma unroll
      for (int k = 0; k < 4; k++) out.contact_force[s * 4 + k] = on ? F[k] : 0.0;
    }
    if (out.contact_bit) out.contact_bit[s] = on ? bit : -1;
    if (out.contact_frame) {
#pragma unroll
      for (int k = 0; k < 9; k++) out.contact_frame[s * 9 + k] = on ? fr[k] : 0.0;
    }
    if (out.contact_pos) {
#pragma unroll
      for (int k = 0; k < 3; k++) out.contact_pos[s * 3 + k] = on ? cp[k] : 0.0;
    }
    if (out.contact_dist) out.contact_dist[s] = on ? dist : 0.0;
  }
  if (sub == 0) {
    if (out.contact_mask) out.contact_mask[e] = ok ? mask : 0u;
    if (out.status) out.status[e] = ok ? 0 : 1;
  }
}

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_K_FORCES(const KDeviceModel* __restrict__ dm, KDeviceState st, KForcesDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, NC = Dim<NL>::NC, NSS = Dim<NL>::NSS;
  static_assert(NC <= 16, "the slot lanes sit in the group's first DPP row");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  stage_model<NL>(lm, dm);
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  const int env = xcd_block(blockIdx.x, gridDim.x) * EPB + grp;
  if (grp >= EPB || env >= st.num_envs) return;      // whole group exits together
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  init_ws<NL>(w, sub);
#if KM_VAR_PAR
  ep_load<NL>(w, dm, st, env, sub, invm);
#else
  if (sub >= NL && sub < NV) invm = sub < NL + 3 ? 1.0 / m->cube_mass : 1.0 / m->cube_inertia[sub - NL - 3];
#endif
  load_state<NL, G>(w, st, env, sub);
  // ctrl exactly as stored: load_state's float32 rounding is the start of before_step, which does not run here
  for (int i = sub; i < NL; i += G) w.ctrl[i] = st.ctrl[(size_t)i * st.num_envs + env];
#if KM_VAR_FRC
  const int frc_bad = load_applied<NL, G>(w, st, env, sub);
#endif
  GSYNC();
  const real F0[4] = {0, 0, 0, 0}, fr0[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cp0[3] = {0, 0, 0};
  // a non-finite state (k_observe's test) or, in the force builds, a non-finite applied force: status 1, nothing else computed
  int lb = 0;
#if KM_VAR_FRC
  lb = frc_bad;
#endif
  for (int i = sub; i < NQ; i += G) lb |= !isfinite(w.qpos[i]);
  for (int i = sub; i < NV; i += G) lb |= !isfinite(w.qvel[i]);
  if (gor<G>(lb)) { write_forces<NL, G>(out, env, sub, false, 0, 0, 0, F0, -1, fr0, cp0, 0, 0u); return; }
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
  // which KM_CON_* bit sits in this lane's slot: corner slots hold the penetrating corners in corner order (the mask's low byte has
  // exactly the kept ones), sphere slots name their sphere
  int bit = -1;
  if (sub < NC && ((act >> sub) & 1u)) {
    if (sub < 4) {
      uint32_t mm = mask & KM_CON_ANY_CUBE_TABLE;
      for (int k = 0; k < sub; k++) mm &= mm - 1u;
      bit = __ffs((int)mm) - 1;
    } else bit = (sub < 4 + NSS ? 8 : 20) + sph;
  }
  write_forces<NL, G>(out, env, sub, true, a, fc, fa, F, bit, fr, cp, dist, mask);
}

template <int NL, int G>
static void launch_forces_t(const KDeviceModel* dm, const KDeviceState& st, const KForcesDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_K_FORCES<NL, G, EPB>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, out);
}
#if KM_VAR_PAR && KM_VAR_FRC
}  // namespace km_envp_frc
using namespace km_envp_frc;
#define KM_LAUNCH_FORCES kmanip_launch_forces_ep_frc_
#elif KM_VAR_FRC
}  // namespace km_frc
using namespace km_frc;
#define KM_LAUNCH_FORCES kmanip_launch_forces_frc_
#elif KM_VAR_PAR
}  // namespace km_envp
using namespace km_envp;
#define KM_LAUNCH_FORCES kmanip_launch_forces_ep_
#else
#define KM_LAUNCH_FORCES kmanip_launch_forces_
#endif
// ---- one (NL, G[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file eight times)
#ifndef KM_VAR_NL
#error "compile with -DKM_VAR_NL=<10|20> -DKM_VAR_G=<16|32> -DKM_VAR_SOLVER=1"
#endif
#define KM_CAT3_(a, b, c) a##b##_##c
#define KM_CAT3(a, b, c) KM_CAT3_(a, b, c)
void KM_CAT3(KM_LAUNCH_FORCES, KM_VAR_NL, KM_VAR_G)(const KDeviceModel* dm, const KDeviceState& st, const KForcesDev& out, hipStream_t stream) {
  launch_forces_t<KM_VAR_NL, KM_VAR_G>(dm, st, out, stream);
}
