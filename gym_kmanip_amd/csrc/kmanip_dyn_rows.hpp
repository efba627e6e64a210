// kmanip_dyn_rows.hpp -- what the queries that solve share beyond the phase headers: the decode of the Newton path's registers into a
// KForcesDev row, its writer and the bad-qacc test (k_forces, k_forward; k_rollout's and k_feedback's sub-step spells the test out) and
// the entry of a kernel over rows the caller passes (k_forward, k_rollout, k_feedback, k_transfd, k_paramfd, k_kinrows, k_sitecost), and the quaternion log map of
// k_feedback, k_transfd, k_paramfd and k_sitecost (quat_log_diff).  Included by kmanip_forces.hip,
// kmanip_forward.hip, kmanip_rollout.hip (the source of k_rollout and k_feedback), kmanip_transfd.hip, kmanip_paramfd.hip and kmanip_sitekin.hip only, right after kmanip_dyn_variant.hpp
// and so inside the build's namespace: the other per-variant objects never see it and stay the ones they were (DESIGN.md sections 25 and 28).
#pragma once

// a failed factorisation or mjWARN_BADQACC, as k_step tests it: the same flag on every lane of the group
template <int NL, int G>
__device__ __forceinline__ int bad_qacc(const Ws<NL>& w, int sub, real a) {
  const int la = (sub < Dim<NL>::NV) && (!isfinite(a) || fabs(a) > 1e10);
  return gor<G>(la) | w.bad;
}

// ---- the KForcesDev row of one solved env / row.  Lane = dof: fc (qfrc_constraint), fa (qfrc_actuator); lane = slot: the rest.
struct ForcesRow {
  real fc = 0, fa = 0, F[4] = {0, 0, 0, 0};
  int bit = -1;                        // which pair sits in the lane's slot, -1 = none
  real fr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cp[3] = {0, 0, 0}, dist = 0;
  uint32_t mask = 0u;
};
// After solve returned qacc `a`, the Newton path holds everything the outputs need (kmanip_forces.hip's header).
template <int NL, int G>
__device__ __forceinline__ ForcesRow forces_decode(const Ws<NL>& w, const LModel<NL>& lm, const CReg<NL>& cr, int sub, real invm, real a) {
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC;
  static_assert(NC <= 16, "the slot lanes sit in the group's first DPP row");
  ForcesRow f;
  // everything the outputs read from LDS in one batch: solve_newton's inputs again (its right-hand sides are still in w.tmp, M^-1 in
  // w.Minv), this lane's slot geometry
  const int si = sub < NL ? sub : NL - 1, sv = sub < NV ? sub : NV - 1, cs = sub < NC ? sub : NC - 1;
  real ctl = w.ctrl[si], cr0 = lm.ctrlrange[si][0], cr1 = lm.ctrlrange[si][1], kpv = KM_EP_KP(w, lm, si), qps = w.qpos[si];
  real fr0 = lm.forcerange[si][0], fr1 = lm.forcerange[si][1], rhs = w.tmp[sv];
  const int flim = lm.forcelimited[si];
  real mrow[NL], tv[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) { mrow[j] = w.Minv[si][j]; tv[j] = w.tmp[j]; }
#pragma unroll
  for (int k = 0; k < 9; k++) f.fr[k] = w.c_frame[cs][k];
#pragma unroll
  for (int k = 0; k < 3; k++) f.cp[k] = w.c_pos[cs][k];
  f.dist = w.c_dist[cs];
  const int sph = w.slot_sph[cs];
  const uint32_t act = w.cact;
  f.mask = w.contact_mask;
  // qacc_smooth as solve_newton formed it, then qfrc_constraint = M (qacc - qacc_smooth)
  real a_s = 0;
  if (sub < NL) {
#pragma unroll
    for (int j = 0; j < NL; j++) a_s += mrow[j] * tv[j];
  } else if (sub < NV) a_s = rhs * invm;
  const real mdiag = (sub >= NL && sub < NV) ? 1.0 / invm : 0.0;
  f.fc = mass_mul<NL, G>(cr, sub, mdiag, sub < NV ? a - a_s : 0.0);
  // the servo force: solve_newton's clamp
  f.fa = kpv * fmin(fmax(ctl, cr0), cr1) - kpv * qps;
  if (flim) f.fa = fmin(fmax(f.fa, fr0), fr1);
  // the slot forces at the final qacc, on the slot lanes (two-row groups: of the first DPP row -- lanes sub < NC)
  real u[4], Wd[7];
  slot_project<NL, G, KM_SUB_ALL>(w, cr, act, sub, a, u);
#pragma unroll
  for (int k = 0; k < 4; k++) u[k] -= cr.sc.A[k];
  slot_eval<false>(cr.sc, u, f.F, Wd);
  if (sub < NC) f.bit = slot_contact_bit<NL>(sub, act, f.mask, sph);
  return f;
}
// Row `row` (an env for k_forces) of every requested output.  status 1 (non-finite input, failed factorisation, bad qacc) or 2 (env
// index out of range): every value 0, every slot empty -- the second form.
template <int NL>
__device__ __forceinline__ void write_forces_row(const KForcesDev& out, int row, int sub, int status, real a, const ForcesRow& f) {
  constexpr int NV = Dim<NL>::NV;
  const size_t e = (size_t)row;
  const bool ok = status == 0;
  if (sub < NV) {
    if (out.qacc) out.qacc[e * NV + sub] = ok ? a : 0.0;
    if (out.qfrc_constraint) out.qfrc_constraint[e * NV + sub] = ok ? f.fc : 0.0;
  }
  if (sub < NL && out.qfrc_actuator) out.qfrc_actuator[e * NL + sub] = ok ? f.fa : 0.0;
  write_slot_rows<NL>(out, e, sub, ok, f.F, f.bit, f.fr, f.cp, f.dist);
  if (sub == 0) {
    if (out.contact_mask) out.contact_mask[e] = ok ? f.mask : 0u;
    if (out.status) out.status[e] = (uint8_t)status;
  }
}
template <int NL>
__device__ __forceinline__ void write_forces_row(const KForcesDev& out, int row, int sub, int status) {
  write_forces_row<NL>(out, row, sub, status, 0, ForcesRow());
}

// ---- the entry of a kernel over n rows the caller passes, 64 / G rows per single-wave workgroup, in two parts like query_env /
// query_load, around the kernel's own returns (a group without a row; status 2).  In: KForwardIn, KRolloutIn or KFeedbackIn, which name
// env_index, qpos, qvel, qacc_warm, ctrl and qfrc_applied alike.
// row_env: the model staged (every lane: it ends in a workgroup barrier), lane group -> row behind the XCD-aware block mapping, row ->
// env (env_index NULL: row r is env r); false = no row.  The env is the caller's word: the kernel tests it before row_load uses it.
template <int NL, int EPB, class In>
__device__ __forceinline__ bool row_env(LModel<NL>& lm, const KDeviceModel* dm, const In& in, int n, int grp, int& row, int& env) {
  stage_model<NL>(lm, dm);
  row = xcd_block(blockIdx.x, gridDim.x) * EPB + grp;
  if (grp >= EPB || row >= n) return false;
  env = in.env_index ? in.env_index[row] : row;
  return true;
}
// row_load: query_load's load_state with the caller's row r of qpos / qvel / qacc_warm, where given, over the env's.  crow / frow: the
// row's ctrl and applied force as the caller gave them (held, or step 0's), NULL = what the env stores -- ctrl exactly as given /
// stored (load_state's float32 rounding is the start of before_step, which does not run here), the env's row of the bound force buffer
// if there is one.  Ends with the group synchronised.  Returns this lane's reasons for status 1 beyond the state's own:
// state_nonfinite's `lb`.  (query_load's other two calls, init_ws and env_invm, stay in the kernel, ahead of the row pointers: behind
// them k_rollout's sub-step loop is scheduled differently and runs about 1 % slower)
template <int NL, int G, class In>
__device__ __forceinline__ int row_load(Ws<NL>& w, const KDeviceState& st, const In& in, size_t r, int env, int sub, const double* crow,
                                        const double* frow) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  static_assert(NV <= G, "lane = dof");
  const int NE = st.num_envs;
  // the caller's rows, requested before the handle's columns are waited for
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
  for (int k = 0; k < KL; k++) { const int i = sub + G * k, ic = i < NL ? i : NL - 1; gc[k] = crow ? crow[ic] : st.ctrl[(size_t)ic * NE + env]; }
#if KM_VAR_FRC
  // (the launcher picks this build only if the caller's tensor or the bound buffer exists)
  if (!frow && st.qfrc_applied) frow = st.qfrc_applied + (size_t)env * NV;
  const real fap = frow ? frow[sub < NV ? sub : NV - 1] : 0.0;
#endif
  load_state<NL, G>(w, st, env, sub);
  // the overrides: each lane rewrites the entries it wrote in load_state (the same lane -> index map)
#pragma unroll
  for (int k = 0; k < KQ; k++) { const int i = sub + G * k; if (in.qpos && i < NQ) w.qpos[i] = gq[k]; }
#pragma unroll
  for (int k = 0; k < KV; k++) { const int i = sub + G * k; if (i < NV) { if (in.qvel) w.qvel[i] = gv[k]; if (in.qacc_warm) w.warm[i] = gw[k]; } }
#pragma unroll
  for (int k = 0; k < KL; k++) { const int i = sub + G * k; if (i < NL) w.ctrl[i] = gc[k]; }
  int lb = 0;
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
  return lb;
}

// ---- the log map of k_feedback's state difference (a = the reference's quaternion) and of k_transfd's quotient (a = the -eps row's)
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
