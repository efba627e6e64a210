// kmanip_forward_fd.hip -- kmanip_forward_fd's second launch (gfx950, wave64): the centred finite differences of the forward dynamics
// at rows the caller passes -- d qacc, d qfrc_constraint, d qfrc_actuator and d contact_force / d (qpos, qvel, ctrl, qfrc_applied) --
// with the perturbation and the quotient inside the kernel.  The kernels are k_fwdfd, the objects
// kmanip_fwdfd_*: names next to k_transfd's and k_paramfd's, and outside the patterns that count the k_forward kernels.
//
// gym_kmanip_amd/derivatives.py forward_fd builds 2 ncol n perturbed rows with torch arithmetic, sends them through k_forward and
// forms the quotients with torch arithmetic again; those kernels and the perturbed rows' trips through HBM, not the simulator, are
// where its time goes.  Here the work item is k_transfd's PAIR p = r ncol + c -- nominal row r, tangent / input column c -- and the
// pair's two rows, +eps and -eps, sit in ADJACENT lane groups of one wave: two pairs per wave at G = 16, one at G = 32.  Each group
// loads nominal row r through k_forward's entry (row_env, row_load), perturbs its copy in LDS, and runs k_forward's body: the
// products, one solve, the bad-qacc test, the decode of the Newton path's registers.  Nothing is integrated.
// THE EXCHANGE IS IN REGISTERS.  After forces_decode a lane holds its own qacc and qfrc_constraint (lane = dof), qfrc_actuator
// (lane = actuator) and the four force components of a contact slot (lane = slot), and the -eps group's value for the same `sub`
// sits exactly G lanes away: one lane-xor shuffle per value, (mine - theirs) / (2.0 * eps) in the + group's registers, one
// contiguous run of nout doubles stored per column.  No exchange array, no barrier behind the solve; status and contact mask travel
// the same way.  EVERY LANE OF THE WAVE MUST REACH THE SHUFFLES: no group leaves before them except a whole pair without work (at
// G = 16 the wave's other pair then exchanges among its own 32 lanes); a bad index or a failed row sets the group's status and falls
// through, where k_forward returns.
// Per row the arithmetic is derivatives.forward_fd's, operation for operation: +-eps added to one entry, or the cube's quaternion
// multiplied on the right by [cos(eps / 2), +-sin(eps / 2) e_k] as tangent_perturb spells the product (sin and cos taken once on the
// host); the warm start the nominal row's qacc (the first launch wrote it) plus warm_offset on every dof; a slot empty in a row
// counts as zeros, as k_forward writes it; a division, not a reciprocal multiply.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here)
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load, bad_qacc, forces_decode: shared with k_forward)
static_assert(KM_VAR_SOLVER == 1, "k_fwdfd reads the Newton path's registers");

// derivatives.tangent_perturb's rotation columns, restated from kmanip_transfd.hip (a helper moved into a shared header reorders the
// code of the other kernels, DESIGN.md sections 25 and 31): q <- q (x) [w1, v1], v1 = sh e_k, every product and sum rounded on its own
__device__ __forceinline__ void ffd_quat_perturb(real (&q)[4], int k, real w1, real sh) {
#pragma clang fp contract(off)
  const real x1 = k == 0 ? sh : 0.0, y1 = k == 1 ? sh : 0.0, z1 = k == 2 ? sh : 0.0;
  const real w0 = q[0], x0 = q[1], y0 = q[2], z0 = q[3];
  q[0] = ((w0 * w1 - x0 * x1) - y0 * y1) - z0 * z1;
  q[1] = ((w0 * x1 + x0 * w1) + y0 * z1) - z0 * y1;
  q[2] = ((w0 * y1 - x0 * z1) + y0 * w1) + z0 * x1;
  q[3] = ((w0 * z1 + x0 * y1) - y0 * x1) + z0 * w1;
}

// the same `sub` of the pair's other group: G lanes away, whichever of the two asks
template <int G> __device__ __forceinline__ real ffd_other(real v) { return __shfl_xor(v, G, 64); }
template <int G> __device__ __forceinline__ int ffd_other(int v) { return __shfl_xor(v, G, 64); }

// ch, sh: cos(eps / 2), sin(eps / 2) from the host entry
template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_fwdfd)(const KDeviceModel* __restrict__ dm, KDeviceState st, KForwardFdIn in, int n, real ch, real sh,
                                                         KForwardFdDev out) {
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC;
  static_assert(EPB % 2 == 0 && EPB * G == 64, "the two rows of a pair sit in adjacent lane groups of the wave");
  static_assert(NL <= G && NV <= G && NC <= G, "lane = actuator, lane = dof, lane = contact slot");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  // the columns, always in this order: qpos (nv tangent columns), qvel (nv), ctrl (nu), qfrc_applied (nv)
  const int wq = (in.wrt & KM_WRT_QPOS) ? NV : 0, wv = (in.wrt & KM_WRT_QVEL) ? NV : 0, wc = (in.wrt & KM_WRT_CTRL) ? NL : 0;
  const int ncol = wq + wv + wc + ((in.wrt & KM_WRT_FRC) ? NV : 0);
  // a column's run of outputs, the parts named in `of` in this order: qacc, qfrc_constraint, qfrc_actuator, contact_force
  const int na = (in.of & KM_OF_QACC) ? NV : 0, nc = (in.of & KM_OF_QFRC_CONSTRAINT) ? NV : 0, nu = (in.of & KM_OF_QFRC_ACTUATOR) ? NL : 0;
  const int nout = na + nc + nu + ((in.of & KM_OF_CONTACT_FORCE) ? 4 * NC : 0);
  // perturbed row q = 2 p + (0: +eps, 1: -eps) behind the XCD-aware block mapping: row_env's, over 2 ncol n rows without an index of
  // their own (the host entry keeps that count inside int); the env is nominal row r's, the warm-start base its qacc
  KForwardFdIn rin = in;
  rin.env_index = nullptr;
  rin.qacc_warm = out.qacc;
  int q, env;
  if (!row_env<NL, EPB>(lm, dm, rin, 2 * ncol * n, grp, q, env)) return;      // (2 ncol n is even: a whole pair leaves together)
  const int p = q >> 1, minus = q & 1, row = p / ncol, c = p - row * ncol;
  const size_t r = (size_t)row;
  env = in.env_index ? in.env_index[row] : row;
  Ws<NL>& w = ws[grp];
  int status = 0;
  real a = 0;
  ForcesRow f;
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
          ffd_quat_perturb(qt, c - NL - 3, ch, minus ? -sh : sh);
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
    // a non-finite input, given or stored: status 1, nothing solved
    if (state_nonfinite<NL, G>(w, sub, lb)) status = 1;
    else {
      Prof pf;
      pf.start();
      CReg<NL> cr;
      step1_products<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, cr, invm, pf);
      a = solve<NL, G, KM_SOLVER_NEWTON>(w, lm, m, sub, 1, cr, invm, pf);
      if (bad_qacc<NL, G>(w, sub, a)) status = 1;
      else f = forces_decode<NL, G>(w, lm, cr, sub, invm, a);
    }
  }
  // ---- the exchange: both groups of the pair arrive here, whatever became of their rows.  A row's values as k_forward would have
  // written them: an empty slot is zeros
  const bool on = status == 0 && f.bit >= 0;
  real F[4];
#pragma unroll
  for (int k = 0; k < 4; k++) F[k] = on ? f.F[k] : 0.0;
  const int mask = status == 0 ? (int)f.mask : 0;
  const real a_o = ffd_other<G>(a), fc_o = ffd_other<G>(f.fc), fa_o = ffd_other<G>(f.fa);
  real F_o[4];
#pragma unroll
  for (int k = 0; k < 4; k++) F_o[k] = ffd_other<G>(F[k]);
  const int status_o = ffd_other<G>(status), mask_o = ffd_other<G>(mask);
  if (minus) return;
  const int sc = status > status_o ? status : status_o;
  if (sub == 0) {
    if (out.status_cols) out.status_cols[p] = (uint8_t)sc;
    if (out.contact_mask_fd) { out.contact_mask_fd[(size_t)p * 2] = (uint32_t)mask; out.contact_mask_fd[(size_t)p * 2 + 1] = (uint32_t)mask_o; }
  }
  double* col = out.deriv_t + (size_t)p * nout;
  if (sc) {                            // a column of a row that failed: zeros
    for (int i = sub; i < nout; i += G) col[i] = 0.0;
    return;
  }
  const real den = 2.0 * in.eps;
  if (sub < NV) {
    if (na) col[sub] = (a - a_o) / den;
    if (nc) col[na + sub] = (f.fc - fc_o) / den;
  }
  if (sub < NL && nu) col[na + nc + sub] = (f.fa - fa_o) / den;
  if (sub < NC && (in.of & KM_OF_CONTACT_FORCE)) {
#pragma unroll
    for (int k = 0; k < 4; k++) col[na + nc + nu + sub * 4 + k] = (F[k] - F_o[k]) / den;
  }
}

template <int NL, int G>
static void launch_fwdfd_t(const KDeviceModel* dm, const KDeviceState& st, const KForwardFdIn& in, int n, int ncol, double ch, double sh,
                           const KForwardFdDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G, PAIRS = EPB / 2;        // lane groups and pairs per wave
  const int pairs = n * ncol;
  hipLaunchKernelGGL((KM_KERNEL(k_fwdfd)<NL, G, EPB>), dim3((pairs + PAIRS - 1) / PAIRS), dim3(64), 0, stream, dm, st, in, n, ch, sh, out);
}
KM_VARIANT_END
// ---- one (NL, G[, PAR][, FRC]) variant per translation unit (the Makefile compiles this file eight times)
void KM_LAUNCHER2(fwdfd)(const KDeviceModel* dm, const KDeviceState& st, const KForwardFdIn& in, int n, int ncol, double ch, double sh,
                         const KForwardFdDev& out, hipStream_t stream) {
  launch_fwdfd_t<KM_VAR_NL, KM_VAR_G>(dm, st, in, n, ncol, ch, sh, out, stream);
}
