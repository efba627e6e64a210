// kmanip_transfd.hip -- kmanip_transition_fd's second launch (gfx950, wave64): the centred finite differences of ONE step of the rows
// the caller passes, MuJoCo's mjd_transitionFD, with the perturbation and the quotient inside the kernel.
//
// gym_kmanip_amd/derivatives.py transition_fd builds 2 ncol n perturbed rows with torch arithmetic, sends them through k_rollout and
// forms the quotients with torch arithmetic again; those kernels, not the simulator, are where its time goes.  Here the work item is a
// PAIR p = r ncol + c -- nominal row r, tangent / input column c -- and the pair's two rows, +eps and -eps, sit in ADJACENT lane groups
// of one wave: two pairs per wave at G = 16, one at G = 32.  Each group loads nominal row r through k_rollout's entry (row_env,
// row_load), perturbs its copy in LDS, runs k_rollout's sub-step loop for one step, and the two meet in a small exchange array of this
// unit's own (Ws is every kernel's and stays as it is), where the + group forms [tangent_diff(q+, q-) ; v+ - v-] / (2.0 * eps) and
// stores column c of the row's transposed derivative: 2 nv contiguous doubles.  Neither the perturbed inputs nor the perturbed states
// ever reach HBM.
// Per row the arithmetic is derivatives.transition_fd's, operation for operation: +-eps added to one entry, or the cube's quaternion
// multiplied on the right by [cos(eps / 2), +-sin(eps / 2) e_k] as tangent_perturb spells the product (sin and cos taken once on the
// host); the warm start of the first sub-step the base (the caller's, else the nominal row's after its step: the first launch wrote
// it) plus warm_offset; the log map is k_feedback's, quat_log_diff of kmanip_dyn_rows.hpp; a division, not a reciprocal multiply.
// NO GROUP LEAVES BEFORE THE EXCHANGE, except a whole pair without work: a bad index or a row that stops sets the group's status and
// falls through, where k_rollout returns.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load: shared with k_forward and k_rollout; quat_log_diff: with k_feedback)

// what the two groups of a pair hand each other: the state after the step and the row's status
template <int NL>
struct TfdXch {
  real qpos[Dim<NL>::NQ], qvel[Dim<NL>::NV];
  int status, pad_;
};

// derivatives.tangent_perturb's rotation columns: q <- q (x) [w1, v1], v1 = sh e_k, every product and sum rounded on its own
__device__ __forceinline__ void tfd_quat_perturb(real (&q)[4], int k, real w1, real sh) {
#pragma clang fp contract(off)
  const real x1 = k == 0 ? sh : 0.0, y1 = k == 1 ? sh : 0.0, z1 = k == 2 ? sh : 0.0;
  const real w0 = q[0], x0 = q[1], y0 = q[2], z0 = q[3];
  q[0] = ((w0 * w1 - x0 * x1) - y0 * y1) - z0 * z1;
  q[1] = ((w0 * x1 + x0 * w1) + y0 * z1) - z0 * y1;
  q[2] = ((w0 * y1 - x0 * z1) + y0 * w1) + z0 * x1;
  q[3] = ((w0 * z1 + x0 * y1) - y0 * x1) + z0 * w1;
}

// ch, sh: cos(eps / 2), sin(eps / 2) from the host entry
template <int NL, int G, int SOLVER, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_transfd)(const KDeviceModel* __restrict__ dm, KDeviceState st, KTransFdIn in, int n, int nsub,
                                                           real ch, real sh, KTransFdDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, NX = 2 * NV;
  static_assert(EPB % 2 == 0 && EPB * G == 64, "the two rows of a pair sit in adjacent lane groups of the wave");
  static_assert(NL <= G && NV <= G, "lane = actuator, lane = dof");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  __shared__ TfdXch<NL> xch[EPB];
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  // the columns, always in this order: qpos (nv tangent columns), qvel (nv), ctrl (nu), qfrc_applied (nv)
  const int wq = (in.wrt & KM_WRT_QPOS) ? NV : 0, wv = (in.wrt & KM_WRT_QVEL) ? NV : 0, wc = (in.wrt & KM_WRT_CTRL) ? NL : 0;
  const int ncol = wq + wv + wc + ((in.wrt & KM_WRT_FRC) ? NV : 0);
  // perturbed row q = 2 p + (0: +eps, 1: -eps) behind the XCD-aware block mapping: row_env's, over 2 ncol n rows without an index of
  // their own (the host entry keeps that count inside int); the env is nominal row r's
  KTransFdIn rin = in;
  rin.env_index = nullptr;
  if (!rin.qacc_warm) rin.qacc_warm = out.qacc_warm;          // the warm-start base: the nominal row's, one step on
  int q, env;
  if (!row_env<NL, EPB>(lm, dm, rin, 2 * ncol * n, grp, q, env)) return;      // (2 ncol n is even: a whole pair leaves together)
  const int p = q >> 1, minus = q & 1, row = p / ncol, c = p - row * ncol;
  const size_t r = (size_t)row;
  env = in.env_index ? in.env_index[row] : row;
  Ws<NL>& w = ws[grp];
  TfdXch<NL>& mine = xch[grp];
  int status = 0;
  // an index outside the handle (group-uniform): never used as an address
  if (env < 0 || env >= st.num_envs) status = 2;
  else {
    real invm = 0;                     // diagonal of M^-1 for the cube dof owned by this lane
    init_ws<NL>(w, sub);
    env_invm<NL>(w, dm, st, env, sub, invm);
    const double* crow = in.ctrl ? in.ctrl + r * NL : nullptr;
    const double* frow = in.qfrc_applied ? in.qfrc_applied + r * NV : nullptr;
    int lb = row_load<NL, G>(w, st, rin, r, env, sub, crow, frow);
    // ---- the perturbation, each lane rewriting entries it owns (load_state's lane -> index map); one lane writes the quaternion
    {
      const real se = minus ? -in.eps : in.eps;
      if (sub < NV) w.warm[sub] = w.warm[sub] + in.warm_offset;
      if (c < wq) {
        if (c < NL + 3) { if (sub == c % G) w.qpos[c] = w.qpos[c] + se; }
        else if (sub == 0) {
          real qt[4];
#pragma unroll
          for (int k = 0; k < 4; k++) qt[k] = w.qpos[NL + 3 + k];
          tfd_quat_perturb(qt, c - NL - 3, ch, minus ? -sh : sh);
#pragma unroll
          for (int k = 0; k < 4; k++) w.qpos[NL + 3 + k] = qt[k];
        }
      } else if (c < wq + wv) { if (sub == c - wq) w.qvel[sub] = w.qvel[sub] + se; }
      else if (c < wq + wv + wc) { if (sub == c - wq - wv) w.ctrl[sub] = w.ctrl[sub] + se; }
#if KM_VAR_FRC
      else if (sub == c - wq - wv - wc) w.frc[sub] = w.frc[sub] + se;
#endif
      GSYNC();
      // what the perturbation can have made non-finite beyond the state (an overflow): the row's tests see the values it runs with
      lb |= (sub < NV) && !isfinite(w.warm[sub]);
      lb |= (sub < NL) && !isfinite(w.ctrl[sub]);
#if KM_VAR_FRC
      lb |= (sub < NV) && !isfinite(w.frc[sub]);
#endif
    }
    // a non-finite input, given or stored: status 1, no step
    if (state_nonfinite<NL, G>(w, sub, lb)) status = 1;
    else {
      Prof pf;
      pf.start();
      int bad = 0;
      for (int s = 0; s < nsub; s++) {
        // k_rollout's sub-step: the lane's dof index opaque to the optimiser once per sub-step
        int subv = sub; asm volatile("" : "+v"(subv));
        CReg<NL> cr;                   // (one per sub-step: nothing of it can be carried round the loop)
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
  const TfdXch<NL>& other = xch[grp + 1];
  const int so = other.status, sc = status > so ? status : so;
  if (sub == 0 && out.status_cols) out.status_cols[p] = (uint8_t)sc;
  double* col = out.deriv_t + (size_t)p * NX;
  if (sc) {                            // a column of a row that stopped: zeros
    for (int i = sub; i < NX; i += G) col[i] = 0.0;
    return;
  }
  // lane = component; every lane computes the log map of conj(q-) (x) q+
  real qa[4], qb[4], rot[3];
#pragma unroll
  for (int k = 0; k < 4; k++) { qa[k] = other.qpos[NL + 3 + k]; qb[k] = mine.qpos[NL + 3 + k]; }
  quat_log_diff(qa, qb, rot);
  const real den = 2.0 * in.eps;
  for (int i = sub; i < NX; i += G) {
    real d;
    if (i >= NV) d = mine.qvel[i - NV] - other.qvel[i - NV];
    else if (i < NL + 3) d = mine.qpos[i] - other.qpos[i];
    else d = i == NL + 3 ? rot[0] : i == NL + 4 ? rot[1] : rot[2];
    col[i] = d / den;
  }
}

template <int NL, int G, int SOLVER>
static void launch_transfd_t(const KDeviceModel* dm, const KDeviceState& st, const KTransFdIn& in, int n, int ncol, int nsub, double ch, double sh,
                             const KTransFdDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G, PAIRS = EPB / 2;        // lane groups and pairs per wave
  const int pairs = n * ncol;
  hipLaunchKernelGGL((KM_KERNEL(k_transfd)<NL, G, SOLVER, EPB>), dim3((pairs + PAIRS - 1) / PAIRS), dim3(64), 0, stream, dm, st, in, n, nsub, ch, sh, out);
}
KM_VARIANT_END
// ---- one (NL, G, SOLVER[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file sixteen times)
void KM_LAUNCHER3(transfd)(const KDeviceModel* dm, const KDeviceState& st, const KTransFdIn& in, int n, int ncol, int nsub, double ch, double sh,
                           const KTransFdDev& out, hipStream_t stream) {
  launch_transfd_t<KM_VAR_NL, KM_VAR_G, KM_VAR_SOLVER>(dm, st, in, n, ncol, nsub, ch, sh, out, stream);
}
