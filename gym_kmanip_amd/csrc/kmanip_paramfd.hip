// kmanip_paramfd.hip -- kmanip_param_fd's one launch (gfx950, wave64): the centred finite differences of ONE step of the rows the caller
// passes with respect to the per-env physics parameters KM_EP_* (DESIGN.md section 42).  k_transfd's sibling, and its shape: the work item
// is a PAIR p = r npar + c -- nominal row r, parameter column c (the c-th set bit of KParamFdIn::wrt) -- and the pair's two rows, +e and
// -e, sit in ADJACENT lane groups of one wave: two pairs per wave at G = 16, one at G = 32.  Each group enters through k_rollout's entry
// (row_env, row_load), takes the row's parameter vector with entry k replaced by p_k + e or p_k - e, derives Ws::ep and the lane's invm
// with ep_derive / ep_invm -- the one evaluation order model.py with_env_params restates -- runs k_rollout's sub-step loop for one
// step and meets its partner in an exchange array, where the + group forms [tangent_diff(q+, q-) ; v+ - v-] / (2.0 * e) and stores
// column c of the row's transposed derivative: 2 nv contiguous doubles.  No perturbed parameter or state reaches HBM, and the handle's
// own parameters (KDeviceState::envp) are only read.
// ALWAYS the KM_VAR_PAR build (Ws::ep and the KM_EP_* accessors are its): the Makefile compiles this file for the _ep_ and _ep_frc_
// builds only, and the launcher picks between those two whatever the handle's own steps run.
// NO GROUP LEAVES BEFORE THE EXCHANGE, except a whole pair without work: a bad index, a value outside its domain or a row that stops sets
// the group's status and falls through.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load, quat_log_diff)
#if !KM_VAR_PAR
#error "kmanip_paramfd.hip is a per-env parameter build: compile with -DKM_VAR_PAR=1"
#endif

// what the two groups of a pair hand each other: the state after the step and the row's status (k_transfd's TfdXch)
template <int NL>
struct PfdXch {
  real qpos[Dim<NL>::NQ], qvel[Dim<NL>::NV];
  int status, pad_;
};

// the perturbation of parameter value pk and the two values it gives, every operation rounded on its own (include/kmanip.h KParamFdDev)
__device__ __forceinline__ void pfd_perturb(real pk, real eps, int relative, real& e, real& plus, real& minus) {
#pragma clang fp contract(off)
  e = relative ? eps * pk : eps;
  plus = pk + e;
  minus = pk - e;
}

template <int NL, int G, int SOLVER, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_paramfd)(const KDeviceModel* __restrict__ dm, KDeviceState st, KParamFdIn in, KEnvParamDefaults model,
                                                           int n, int npar, int nsub, KParamFdDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, NX = 2 * NV;
  static_assert(EPB % 2 == 0 && EPB * G == 64, "the two rows of a pair sit in adjacent lane groups of the wave");
  static_assert(NL <= G && NV <= G, "lane = actuator, lane = dof");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  __shared__ PfdXch<NL> xch[EPB];
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  // perturbed row q = 2 p + (0: +e, 1: -e) behind the XCD-aware block mapping: row_env's, over 2 npar n rows without an index of their
  // own (the host entry keeps that count inside int); the env is nominal row r's
  KParamFdIn rin = in;
  rin.env_index = nullptr;
  int q, env;
  if (!row_env<NL, EPB>(lm, dm, rin, 2 * npar * n, grp, q, env)) return;      // (2 npar n is even: a whole pair leaves together)
  const int p = q >> 1, minus = q & 1, row = p / npar, c = p - row * npar;
  const size_t r = (size_t)row;
  env = in.env_index ? in.env_index[row] : row;
  // column c -> parameter k: the c-th set bit of wrt
  int k = 0;
  for (int b = 0, seen = 0; b < KM_EP_N; b++) {
    if ((in.wrt >> b) & 1) { if (seen == c) k = b; seen++; }
  }
  Ws<NL>& w = ws[grp];
  PfdXch<NL>& mine = xch[grp];
  int status = 0;
  real e = 0;
  // an index outside the handle (group-uniform): never used as an address
  if (env < 0 || env >= st.num_envs) status = 2;
  else {
    // the row's parameters: the caller's row, else the env's values in force, else the compiled model's
    real pv[KM_EP_N], plus, mns;
#pragma unroll
    for (int j = 0; j < KM_EP_N; j++)
      pv[j] = in.params ? in.params[r * KM_EP_N + j] : st.envp ? st.envp[(size_t)j * st.num_envs + env] : model.v[j];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < KM_EP_N; j++) ok = ok && ep_value_ok(j, pv[j]);
    real pk = pv[0], ek = in.eps[0];
#pragma unroll
    for (int j = 1; j < KM_EP_N; j++) { if (j == k) { pk = pv[j]; ek = in.eps[j]; } }
    pfd_perturb(pk, ek, in.eps_relative, e, plus, mns);
    // both groups of the pair test both values: a pair is refused as a whole, and nothing of it is stepped
    ok = ok && (e - e == 0.0) && e != 0.0 && ep_value_ok(k, plus) && ep_value_ok(k, mns);
    if (!ok) status = 3;
    else {
#pragma unroll
      for (int j = 0; j < KM_EP_N; j++) { if (j == k) pv[j] = minus ? mns : plus; }
      real invm = 0;                   // diagonal of M^-1 for the cube dof owned by this lane
      init_ws<NL>(w, sub);
      ep_derive<NL>(w, dm, pv, sub);
      invm = ep_invm<NL>(m, pv, sub);
      const double* crow = in.ctrl ? in.ctrl + r * NL : nullptr;
      const double* frow = in.qfrc_applied ? in.qfrc_applied + r * NV : nullptr;
      int lb = row_load<NL, G>(w, st, rin, r, env, sub, crow, frow);
      if (sub < NV) w.warm[sub] = w.warm[sub] + in.warm_offset;
      GSYNC();
      lb |= (sub < NV) && !isfinite(w.warm[sub]);        // (an overflow of the offset: the row's tests see the values it runs with)
      // a non-finite input, given or stored: status 1, no step
      if (state_nonfinite<NL, G>(w, sub, lb)) status = 1;
      else {
        Prof pf;
        pf.start();
        int bad = 0;
        for (int s = 0; s < nsub; s++) {
          // k_rollout's sub-step: the lane's dof index opaque to the optimiser once per sub-step
          int subv = sub; asm volatile("" : "+v"(subv));
          CReg<NL> cr;                 // (one per sub-step: nothing of it can be carried round the loop)
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
        if (bad) status = 1;
        else if (out.contact_mask_fd) {
          // k_step's trailing mj_step1, as far as the contact mask needs it
          int subr = sub; asm volatile("" : "+v"(subr));
          fk_parallel<NL, G>(w, lm, subr);
          collide_parallel<NL, G>(w, lm, m, subr);
        }
      }
    }
  }
  // ---- the exchange: both groups of the pair arrive here, whatever became of their rows
  if (status == 0) {
    for (int i = sub; i < NQ; i += G) mine.qpos[i] = w.qpos[i];
    if (sub < NV) mine.qvel[sub] = w.qvel[sub];
  }
  if (sub == 0) {
    mine.status = status;
    if (out.contact_mask_fd) out.contact_mask_fd[(size_t)p * 2 + minus] = status == 0 ? w.contact_mask : 0u;
  }
  GSYNC();
  if (minus) return;
  const PfdXch<NL>& other = xch[grp + 1];
  const int so = other.status, sc = status > so ? status : so;
  if (sub == 0 && out.status_cols) out.status_cols[p] = (uint8_t)sc;
  double* col = out.deriv_t + (size_t)p * NX;
  if (sc) {                            // a column that is no derivative: zeros
    for (int i = sub; i < NX; i += G) col[i] = 0.0;
    return;
  }
  // lane = component; every lane computes the log map of conj(q-) (x) q+
  real qa[4], qb[4], rot[3];
#pragma unroll
  for (int j = 0; j < 4; j++) { qa[j] = other.qpos[NL + 3 + j]; qb[j] = mine.qpos[NL + 3 + j]; }
  quat_log_diff(qa, qb, rot);
  const real den = 2.0 * e;
  for (int i = sub; i < NX; i += G) {
    real d;
    if (i >= NV) d = mine.qvel[i - NV] - other.qvel[i - NV];
    else if (i < NL + 3) d = mine.qpos[i] - other.qpos[i];
    else d = i == NL + 3 ? rot[0] : i == NL + 4 ? rot[1] : rot[2];
    col[i] = d / den;
  }
}

template <int NL, int G, int SOLVER>
static void launch_paramfd_t(const KDeviceModel* dm, const KDeviceState& st, const KParamFdIn& in, const KEnvParamDefaults& model, int n, int npar,
                             int nsub, const KParamFdDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G, PAIRS = EPB / 2;        // lane groups and pairs per wave
  const int pairs = n * npar;
  hipLaunchKernelGGL((KM_KERNEL(k_paramfd)<NL, G, SOLVER, EPB>), dim3((pairs + PAIRS - 1) / PAIRS), dim3(64), 0, stream, dm, st, in, model, n, npar,
                     nsub, out);
}
KM_VARIANT_END
// ---- one (NL, G, SOLVER, FRC) variant per translation unit (the Makefile compiles this file eight times)
void KM_LAUNCHER3(paramfd)(const KDeviceModel* dm, const KDeviceState& st, const KParamFdIn& in, const KEnvParamDefaults& model, int n, int npar,
                           int nsub, const KParamFdDev& out, hipStream_t stream) {
  launch_paramfd_t<KM_VAR_NL, KM_VAR_G, KM_VAR_SOLVER>(dm, st, in, model, n, npar, nsub, out, stream);
}
