// kmanip_forward.hip -- contact forces, qacc and joint forces at rows the CALLER passes, as many as it likes, in ONE launch (gfx950,
// wave64): kmanip_forward.
//
// mj_forward with actuation on a scratch mjData: row r names an env (KForwardIn::env_index; NULL = row r is env r), takes that env's
// model parameters and, per field, either the caller's row r of qpos / qvel / ctrl / qacc_warm / qfrc_applied or what the env stores
// (the bound applied force for the last).  Nothing of the handle is written, so a planner evaluates K hypotheses per env without
// cloning K n envs.  The device code is k_forces' (kmanip_forces.hip), which is the step's own -- the headers of kmanip_dyn.hip,
// included here under the same build macros: step1_products, solve once without integrating, then the decode of the Newton path's
// registers into the outputs (restated below from k_forces rather than shared: a helper moved into the common headers reorders the
// code of the other kernels) -- in a translation unit of its own, so that the k_step / k_reset / k_forces /
// k_observe / k_kinematics / k_inverse objects are the ones they were, to the register.  With every input NULL and n = num_envs a row
// computes what k_forces computes for that env.  Newton variants only (kmanip_forward refuses a PGS handle), both parameter builds
// and both applied-force builds, 64 / G ROWS per wave.  The outputs are written at the row, not at the env.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here)
static_assert(KM_VAR_SOLVER == 1, "k_forward reads the Newton path's registers");

// one row of every requested output: lane = dof for the nv- and nu-wide rows, lane = slot for the slot rows.
// status 1 (non-finite input, failed factorisation, bad qacc) or 2 (env index out of range): every value 0, every slot empty.
template <int NL, int G>
__device__ __forceinline__ void write_forward(const KForcesDev& out, int row, int sub, int status, real a, real fc, real fa,
                                              const real (&F)[4], int bit, const real (&fr)[9], const real (&cp)[3], real dist, uint32_t mask) {
  constexpr int NV = Dim<NL>::NV;
  const size_t e = (size_t)row;
  const bool ok = status == 0;
  if (sub < NV) {
    if (out.qacc) out.qacc[e * NV + sub] = ok ? a : 0.0;
    if (out.qfrc_constraint) out.qfrc_constraint[e * NV + sub] = ok ? fc : 0.0;
  }
  if (sub < NL && out.qfrc_actuator) out.qfrc_actuator[e * NL + sub] = ok ? fa : 0.0;
  write_slot_rows<NL>(out, e, sub, ok, F, bit, fr, cp, dist);
  if (sub == 0) {
    if (out.contact_mask) out.contact_mask[e] = ok ? mask : 0u;
    if (out.status) out.status[e] = (uint8_t)status;
  }
}

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_forward)(const KDeviceModel* __restrict__ dm, KDeviceState st, KForwardIn in, int n, KForcesDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, NC = Dim<NL>::NC;
  static_assert(NV <= G, "lane = dof");
  static_assert(NC <= 16, "the slot lanes sit in the group's first DPP row");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  // the entry of a query kernel (query_env) over rows: the model staged by every lane, then a group without a row exits whole
  stage_model<NL>(lm, dm);
  const int row = xcd_block(blockIdx.x, gridDim.x) * EPB + grp;
  if (grp >= EPB || row >= n) return;
  const real F0[4] = {0, 0, 0, 0}, fr0[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cp0[3] = {0, 0, 0};
  const int env = in.env_index ? in.env_index[row] : row;
  // an index outside the handle (group-uniform): never used as an address
  if (env < 0 || env >= st.num_envs) { write_forward<NL, G>(out, row, sub, 2, 0, 0, 0, F0, -1, fr0, cp0, 0, 0u); return; }
  Ws<NL>& w = ws[grp];
  real invm = 0;                       // diagonal of M^-1 for the cube dof owned by this lane
  const size_t r = (size_t)row;
  const int NE = st.num_envs;
  init_ws<NL>(w, sub);            // (query_load's calls, spelt out around the loads below)
  env_invm<NL>(w, dm, st, env, sub, invm);
  // the caller's rows, requested before the handle's columns are waited for; ctrl exactly as given / stored (load_state's float32
  // rounding is the start of before_step, which does not run here)
  constexpr int KQ = (NQ + G - 1) / G, KV = (NV + G - 1) / G, KL = (NL + G - 1) / G;
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
  for (int k = 0; k < KL; k++) { const int i = sub + G * k, ic = i < NL ? i : NL - 1; gc[k] = in.ctrl ? in.ctrl[r * NL + ic] : st.ctrl[(size_t)ic * NE + env]; }
#if KM_VAR_FRC
  // the caller's row or the env's row of the bound buffer (the launcher picks this build only if one of the two exists)
  const double* fsrc = in.qfrc_applied ? in.qfrc_applied + r * NV : (st.qfrc_applied ? st.qfrc_applied + (size_t)env * NV : nullptr);
  const real fap = fsrc ? fsrc[sub < NV ? sub : NV - 1] : 0.0;
#endif
  load_state<NL, G>(w, st, env, sub);
  // the overrides: each lane rewrites the entries it wrote in load_state (the same lane -> index map)
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
  // a non-finite input, given or stored (k_observe's test of the state, and ctrl, the warm start and the force): status 1, nothing
  // else computed
  if (state_nonfinite<NL, G>(w, sub, lb)) { write_forward<NL, G>(out, row, sub, 1, 0, 0, 0, F0, -1, fr0, cp0, 0, 0u); return; }
  Prof pf;
  pf.start();
  CReg<NL> cr;
  step1_products<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, cr, invm, pf);
  const real a = solve<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, 1, cr, invm, pf);
  {                                                    // a failed factorisation or mjWARN_BADQACC, as k_forces tests it
    const int la = (sub < NV) && (!isfinite(a) || fabs(a) > 1e10);
    if (gor<G>(la) | w.bad) { write_forward<NL, G>(out, row, sub, 1, 0, 0, 0, F0, -1, fr0, cp0, 0, 0u); return; }
  }
  // ---- k_forces' decode, restated: everything the outputs read from LDS in one batch: solve_newton's inputs again (its right-hand
  // sides are still in w.tmp, M^-1 in w.Minv), this lane's slot geometry
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
  write_forward<NL, G>(out, row, sub, 0, a, fc, fa, F, bit, fr, cp, dist, mask);
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
