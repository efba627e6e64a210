// kmanip_sitekin.hip -- two read-only queries at rows the CALLER passes, as many as it likes, each in ONE launch (gfx950, wave64):
// kmanip_kinematics_rows (k_kinrows) and kmanip_site_cost (k_sitecost).
//
// k_kinrows is k_kinematics (kmanip_kinematics.hip) behind k_forward's entry: row r names an env (KKinRowsIn::env_index; NULL = row r is
// env r), takes that env's per-env parameters and, per field, the caller's row of qpos / qvel or what the env stores; then kin_tree and
// k_kinematics' output epilogue, written at the row.  Where neither qM nor qfrc_bias is wanted the tree stops after
// fk_parallel (a wave-uniform branch on the kernel's arguments; the call is kin_tree's own, so the geometry's bits are the same).
// k_sitecost is the task-space cost of an iLQR iteration at such rows: fk_parallel alone, the site pose and the Jacobian columns as
// k_kinematics forms them (lane = dof), the position and rotation residuals against the row's targets, the cost, its gradient and
// the Gauss-Newton Hessian J'WJ.  For the Hessian lane j needs column i of every lane: the arm lanes park their twelve Jacobian
// entries in the workspace's bias-pass scratch (Ws::f: dead, no mass matrix is built; rows of 13 doubles, an odd stride), and row i
// is then one broadcast read per entry -- every lane of the group reads the same address -- where a width-G shuffle would cost two
// ds_bpermute per double, 24 per row; the cube's columns are constants and never leave the registers.  No LDS beyond the
// k_kinematics sibling's workspace, no scratch.  Both parameter builds, 64 / G ROWS per wave.  The handle is read only.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here, KM_VAR_FRC left to its default)
#include "kmanip_dyn_rows.hpp"         // (row_env, row_load, quat_log_diff)
static_assert(KM_VAR_SOLVER == 1, "the row kernels are built with the Newton workspace layout");

// ---- k_kinematics' device code, restated: kin_zero, write_kin_bad (with the status as an argument), kin_tree and the output epilogue
// (write_kin_row) are kmanip_kinematics.hip's text.  Moved into a header that both units include, k_kinematics kept its registers, LDS
// and scratch but not its scalar registers (68 -> 74 / 72), so that unit stays as it is.

// `count` zeros into row e of a field (consecutive lanes, consecutive addresses)
template <int G>
__device__ __forceinline__ void kin_zero(double* p, size_t e, int count, int sub) {
  if (p) for (int i = sub; i < count; i += G) p[e * count + i] = 0.0;
}
// a row that computes nothing: `status` (1 a non-finite state, 2 an env index out of range), every other output of the row 0
template <int NL, int G>
__device__ __forceinline__ void write_kin_bad(const KKinDev& out, int env, int sub, int status = 1) {
  constexpr int NV = Dim<NL>::NV;
  const size_t e = (size_t)env;
  kin_zero<G>(out.link_xpos, e, NL * 3, sub);
  kin_zero<G>(out.link_xmat, e, NL * 9, sub);
  kin_zero<G>(out.site_xpos, e, KM_MAX_ARMS * 3, sub);
  kin_zero<G>(out.site_xmat, e, KM_MAX_ARMS * 9, sub);
  kin_zero<G>(out.site_jacp, e, KM_MAX_ARMS * 3 * NV, sub);
  kin_zero<G>(out.site_jacr, e, KM_MAX_ARMS * 3 * NV, sub);
  kin_zero<G>(out.site_vel, e, KM_MAX_ARMS * 6, sub);
  kin_zero<G>(out.qM, e, NV * NV, sub);
  kin_zero<G>(out.qfrc_bias, e, NV, sub);
  if (sub == 0 && out.status) out.status[e] = (uint8_t)status;
}

// The tree phases of step1_products in front of invert_mass, at the state in w.qpos / w.qvel: M -> w.Minv (full rows), bias -> w.bias.
template <int NL, int G>
__device__ __forceinline__ void kin_tree(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub) {
  real kin[15];
  fk_parallel<NL, G>(w, lm, sub, G == 16 ? kin : nullptr);
  real FN[6];
  const int split = G == 32 ? lm.split : 0;
  int bli = -1, bbase = 0;
  if constexpr (G == 32) {
    const int row = (threadIdx.x >> 4) & 1, c = threadIdx.x & 15;
    bbase = row ? split : 0;
    bli = (split && c < (row ? NL - split : split)) ? bbase + c : -1;
    if (split) {                                 // entries between the blocks: never written below, read as part of the rows
      for (int e = sub; e < (int)(sizeof(w.Minv) / sizeof(real)); e += G) (&w.Minv[0][0])[e] = 0.0;
    }
  }
  if constexpr (G == 16) bias_bodies_rows<NL, NL>(w, lm, m, sub < NL ? sub : -1, 0, sub == NL, FN, kin);
  else if (split) {
    bias_bodies_rows<NL, KM_BLOCK_MAX>(w, lm, m, bli, bbase, false, FN);
    if (sub == NL) cube_bias<NL>(w, m);          // (lane NL also works on a link of the second block above)
  }
  else bias_bodies_parallel<NL, G>(w, lm, m, sub);
  GSYNC();                                       // (where the step collides: the zeroed M and the bias scratch are settled)
  if constexpr (G == 16) {
    composite_mass_bias_rows<NL, NL>(w, lm, sub < NL ? sub : -1, 0, FN, kin);
  } else if (split) {
    composite_mass_bias_rows<NL, KM_BLOCK_MAX>(w, lm, bli, bbase, FN);
  } else {
    composite_own<NL, G>(w, lm, sub);
    GSYNC();
    composite_accumulate<NL, G>(w, lm, sub);
    GSYNC();
    mass_matrix<NL, G>(w, lm, sub);              // (the upper triangle along the ancestor paths, zeros elsewhere)
    bias_project<NL, G>(w, lm, sub);
    GSYNC();
    mass_symmetrize<NL, G>(w, sub);
  }
  GSYNC();
}

// Row `row` of every requested output from the workspace after kin_tree (fk_parallel alone where neither qM nor qfrc_bias is wanted):
// status 0.
template <int NL, int G>
__device__ __forceinline__ void write_kin_row(const KKinDev& out, const Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m,
                                              const KDeviceModel* dm, int row, int sub) {
  constexpr int NV = Dim<NL>::NV;
  const size_t e = (size_t)row;
  // ---- link frames: the workspace's arrays as they lie
  if (out.link_xpos) for (int i = sub; i < NL * 3; i += G) out.link_xpos[e * (NL * 3) + i] = (&w.k.xpos[0][0])[i];
  if (out.link_xmat) for (int i = sub; i < NL * 9; i += G) out.link_xmat[e * (NL * 9) + i] = (&w.k.xmat[0][0])[i];
  // ---- this lane's dof: joint type, world axis, anchor, velocity
  const bool arm_dof = sub < NL;
  const int sj = arm_dof ? sub : NL - 1;
  const bool slide = lm.jtype[sj] == KM_JNT_SLIDE;
  const real ax[3] = {w.k.axis[sj][0], w.k.axis[sj][1], w.k.axis[sj][2]};
  const real oj[3] = {w.k.xpos[sj][0], w.k.xpos[sj][1], w.k.xpos[sj][2]};
  const real qv = w.qvel[sj];
  // ---- sites: pose from the link frame (every lane: the Jacobian needs the point), Jacobian columns, velocity
  if (out.site_xpos || out.site_xmat || out.site_jacp || out.site_jacr || out.site_vel) {
#pragma unroll
    for (int a = 0; a < KM_MAX_ARMS; a++) {
      real sx[3] = {0, 0, 0}, sm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, jp[3] = {0, 0, 0}, jr[3] = {0, 0, 0};
      if (m->arm_present[a]) {                           // (wave-uniform)
        const int l = m->arm_site_link[a];
        real R[9], t[3];
        const real so[3] = {m->arm_site_pos[a][0], m->arm_site_pos[a][1], m->arm_site_pos[a][2]};
#pragma unroll
        for (int c = 0; c < 9; c++) R[c] = w.k.xmat[l][c];
        mat_vec3(t, R, so);
#pragma unroll
        for (int c = 0; c < 3; c++) sx[c] = t[c] + w.k.xpos[l][c];
        const double* Rs = dm->x.site_R[a];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) sm[3 * i + j] = R[3 * i] * Rs[j] + R[3 * i + 1] * Rs[3 + j] + R[3 * i + 2] * Rs[6 + j];
        // column `sub`: non-zero only for the dofs of the site link's ancestors-or-self
        if (arm_dof && ((lm.anc[l] >> sub) & 1u)) {
          if (slide) { jp[0] = ax[0]; jp[1] = ax[1]; jp[2] = ax[2]; }
          else {
            const real r[3] = {sx[0] - oj[0], sx[1] - oj[1], sx[2] - oj[2]};
            cross3(jp, ax, r);
            jr[0] = ax[0]; jr[1] = ax[1]; jr[2] = ax[2];
          }
        }
      }
      if (out.site_xpos) {
#pragma unroll
        for (int k = 0; k < 3; k++) if (sub == k) out.site_xpos[e * (KM_MAX_ARMS * 3) + a * 3 + k] = sx[k];
      }
      if (out.site_xmat) {
#pragma unroll
        for (int k = 0; k < 9; k++) if (sub == k) out.site_xmat[e * (KM_MAX_ARMS * 9) + a * 9 + k] = sm[k];
      }
      if (sub < NV) {                                    // rows of nv: consecutive lanes write consecutive addresses
        const size_t base = (e * KM_MAX_ARMS + a) * 3 * NV + sub;
#pragma unroll
        for (int r = 0; r < 3; r++) {
          if (out.site_jacp) out.site_jacp[base + (size_t)r * NV] = jp[r];
          if (out.site_jacr) out.site_jacr[base + (size_t)r * NV] = jr[r];
        }
      }
      if (out.site_vel) {                                // J qvel: the sum over the dofs
        real v[6];
#pragma unroll
        for (int r = 0; r < 3; r++) { v[r] = jp[r] * qv; v[3 + r] = jr[r] * qv; }
        gsum_n<G, 6>(v);
#pragma unroll
        for (int k = 0; k < 6; k++) if (sub == k) out.site_vel[e * (KM_MAX_ARMS * 6) + a * 6 + k] = v[k];
      }
    }
  }
  // ---- the dense M: rows of nv, lane = column; the cube's block is diag(m, m, m, I)
  if (out.qM && sub < NV) {
    const size_t base = e * NV * NV + sub;
    for (int i = 0; i < NL; i++) {
      const real v = w.Minv[i][sj];
      out.qM[base + (size_t)i * NV] = arm_dof ? v : 0.0;
    }
    const int ck = sub >= NL + 3 ? sub - NL - 3 : 0;
    const real cd = sub < NL + 3 ? KM_EP_MASS(w, m) : KM_EP_INERTIA(w, m, ck);
    for (int i = NL; i < NV; i++) out.qM[base + (size_t)i * NV] = i == sub ? cd : 0.0;
  }
  if (out.qfrc_bias && sub < NV) out.qfrc_bias[e * NV + sub] = w.bias[sub];
  if (sub == 0 && out.status) out.status[e] = 0;
}

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_kinrows)(const KDeviceModel* __restrict__ dm, KDeviceState st, KKinRowsIn in, int n, KKinDev out) {
  static_assert(Dim<NL>::NV <= G, "lane = dof");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  const KForwardIn fin = {in.env_index, in.qpos, in.qvel, nullptr, nullptr, nullptr};
  int row, env;
  if (!row_env<NL, EPB>(lm, dm, fin, n, grp, row, env)) return;      // whole group exits together
  // an index outside the handle (group-uniform): never used as an address
  if (env < 0 || env >= st.num_envs) { write_kin_bad<NL, G>(out, row, sub, 2); return; }
  Ws<NL>& w = ws[grp];
  real invm = 0;      // (not needed: nothing is inverted)
  init_ws<NL>(w, sub);
  env_invm<NL>(w, dm, st, env, sub, invm);
  row_load<NL, G>(w, st, fin, (size_t)row, env, sub, nullptr, nullptr);      // (what it reports is about ctrl and the warm start: neither enters)
  // a non-finite state, given or stored (k_kinematics' test): status 1, nothing else computed
  if (state_nonfinite<NL, G>(w, sub)) { write_kin_bad<NL, G>(out, row, sub, 1); return; }
  if (out.qM || out.qfrc_bias) kin_tree<NL, G>(w, lm, m, sub);      // (wave-uniform)
  else {
    real kin[15];
    fk_parallel<NL, G>(w, lm, sub, G == 16 ? kin : nullptr);
  }
  write_kin_row<NL, G>(out, w, lm, m, dm, row, sub);
}

// `count` zeros into row e of a field of KSiteCostDev
template <int G>
__device__ __forceinline__ void sc_zero(double* p, size_t e, size_t count, int sub) {
  if (p) for (size_t i = sub; i < count; i += G) p[e * count + i] = 0.0;
}
// a row that computes nothing: status 1 or 2, every other output of the row 0
template <int NL, int G>
__device__ __forceinline__ void write_sc_bad(const KSiteCostDev& out, int row, int sub, int status) {
  constexpr size_t NX = 2 * Dim<NL>::NV;
  const size_t e = (size_t)row;
  sc_zero<G>(out.lx, e, NX, sub);
  sc_zero<G>(out.lxx, e, NX * NX, sub);
  sc_zero<G>(out.site_xpos, e, KM_MAX_ARMS * 3, sub);
  sc_zero<G>(out.resid, e, KM_MAX_ARMS * 6, sub);
  if (sub == 0) {
    if (out.cost) out.cost[e] = 0.0;
    if (out.status) out.status[e] = (uint8_t)status;
  }
}
// one term of a chain: acc + w * (a * b), the product rounded first (it is the same number on lane i for column j and on lane j for
// column i, so the Hessian is symmetric to the bit)
__device__ __forceinline__ real sc_term(real wgt, real a, real b, real acc) {
#pragma clang fp contract(off)
  const real p = a * b;
  return __builtin_fma(wgt, p, acc);
}

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_sitecost)(const KDeviceModel* __restrict__ dm, KDeviceState st, KSiteCostIn in, int n, KSiteCostDev out) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, NX = 2 * NV, JS = 13;      // JS: the parked rows' stride, odd (Ws' bank rule)
  static_assert(NV <= G, "lane = dof");
  static_assert(sizeof(Ws<NL>().f) >= sizeof(real) * NL * JS, "the parked Jacobian fits the bias-pass scratch");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  const KForwardIn fin = {in.env_index, in.qpos, nullptr, nullptr, nullptr, nullptr};
  int row, env;
  if (!row_env<NL, EPB>(lm, dm, fin, n, grp, row, env)) return;      // whole group exits together
  if (env < 0 || env >= st.num_envs) { write_sc_bad<NL, G>(out, row, sub, 2); return; }
  Ws<NL>& w = ws[grp];
  real invm = 0;
  const size_t r = (size_t)row;
  init_ws<NL>(w, sub);
  env_invm<NL>(w, dm, st, env, sub, invm);
  // the row's targets and weights, requested with the state (every lane of the group the same addresses); an absent arm's are never read
  real tp[KM_MAX_ARMS][3], tq[KM_MAX_ARMS][4], wt[KM_MAX_ARMS][2];
  int lb = 0;
#pragma unroll
  for (int a = 0; a < KM_MAX_ARMS; a++) {
    tp[a][0] = tp[a][1] = tp[a][2] = 0; tq[a][0] = 1; tq[a][1] = tq[a][2] = tq[a][3] = 0; wt[a][0] = wt[a][1] = 0;
    if (m->arm_present[a]) {                             // (wave-uniform)
      const size_t ra = r * KM_MAX_ARMS + a;
#pragma unroll
      for (int c = 0; c < 3; c++) tp[a][c] = in.target_pos[ra * 3 + c];
      wt[a][0] = in.weight[ra * 2];
      wt[a][1] = in.target_quat ? in.weight[ra * 2 + 1] : 0.0;
#pragma unroll
      for (int c = 0; c < 3; c++) lb |= !isfinite(tp[a][c]);
      lb |= !isfinite(wt[a][0]);
      lb |= !isfinite(wt[a][1]);
      if (wt[a][1] != 0) {                               // (group-uniform)
#pragma unroll
        for (int c = 0; c < 4; c++) { tq[a][c] = in.target_quat[ra * 4 + c]; lb |= !isfinite(tq[a][c]); }
      }
    }
  }
  row_load<NL, G>(w, st, fin, r, env, sub, nullptr, nullptr);
  // a non-finite qpos, given or stored, target or weight: status 1, nothing else computed.  qvel does not enter.
  for (int i = sub; i < NQ; i += G) lb |= !isfinite(w.qpos[i]);
  if (gor<G>(lb)) { write_sc_bad<NL, G>(out, row, sub, 1); return; }
  {
    real kin[15];
    fk_parallel<NL, G>(w, lm, sub, G == 16 ? kin : nullptr);
  }
  // ---- this lane's dof: joint type, world axis, anchor (k_kinematics' epilogue)
  const bool arm_dof = sub < NL;
  const int sj = arm_dof ? sub : NL - 1;
  const bool slide = lm.jtype[sj] == KM_JNT_SLIDE;
  const real ax[3] = {w.k.axis[sj][0], w.k.axis[sj][1], w.k.axis[sj][2]};
  const real oj[3] = {w.k.xpos[sj][0], w.k.xpos[sj][1], w.k.xpos[sj][2]};
  const real cube[3] = {w.qpos[NL], w.qpos[NL + 1], w.qpos[NL + 2]};
  real J[KM_MAX_ARMS][6], sxa[KM_MAX_ARMS][3], res[KM_MAX_ARMS][6];      // J: column `sub` of Jp (0..2) and Jr (3..5) per arm
  real cost = 0, g = 0;
#pragma unroll
  for (int a = 0; a < KM_MAX_ARMS; a++) {
#pragma unroll
    for (int c = 0; c < 6; c++) { J[a][c] = 0; res[a][c] = 0; }
    sxa[a][0] = sxa[a][1] = sxa[a][2] = 0;
    if (m->arm_present[a]) {                             // (wave-uniform)
      const int l = m->arm_site_link[a];
      const bool follow = in.follow_cube[a] != 0;
      real R[9], t[3], sm[9], jp[3] = {0, 0, 0}, jr[3] = {0, 0, 0};
      const real so[3] = {m->arm_site_pos[a][0], m->arm_site_pos[a][1], m->arm_site_pos[a][2]};
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = w.k.xmat[l][c];
      mat_vec3(t, R, so);
#pragma unroll
      for (int c = 0; c < 3; c++) sxa[a][c] = t[c] + w.k.xpos[l][c];
      if (arm_dof && ((lm.anc[l] >> sub) & 1u)) {
        if (slide) { jp[0] = ax[0]; jp[1] = ax[1]; jp[2] = ax[2]; }
        else {
          const real rr[3] = {sxa[a][0] - oj[0], sxa[a][1] - oj[1], sxa[a][2] - oj[2]};
          cross3(jp, ax, rr);
          jr[0] = ax[0]; jr[1] = ax[1]; jr[2] = ax[2];
        }
      }
      // the cube's position columns: -I where the target rides on the cube
#pragma unroll
      for (int c = 0; c < 3; c++) if (follow && sub == NL + c) jp[c] = -1.0;
#pragma unroll
      for (int c = 0; c < 3; c++) { J[a][c] = jp[c]; J[a][3 + c] = jr[c]; }
      // e_pos = site - (target + cube)
#pragma unroll
      for (int c = 0; c < 3; c++) res[a][c] = sxa[a][c] - (follow ? tp[a][c] + cube[c] : tp[a][c]);
      if (wt[a][1] != 0) {                               // e_rot: the world-frame log of q_site (x) conj(q_target)
        const double* Rs = dm->x.site_R[a];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) sm[3 * i + j] = R[3 * i] * Rs[j] + R[3 * i + 1] * Rs[3 + j] + R[3 * i + 2] * Rs[6 + j];
        real qs[4], qt[4] = {tq[a][0], tq[a][1], tq[a][2], tq[a][3]}, er[3];
        mat2quat(qs, sm);
        normalize4_fast(qt);
        const real ca[4] = {qs[0], -qs[1], -qs[2], -qs[3]}, cb[4] = {qt[0], -qt[1], -qt[2], -qt[3]};
        quat_log_diff(ca, cb, er);                      // conj(ca) (x) cb = q_site (x) conj(q_target)
        res[a][3] = er[0]; res[a][4] = er[1]; res[a][5] = er[2];
      }
      {
#pragma clang fp contract(off)
        const real* e = res[a];
        const real np = __builtin_fma(e[2], e[2], __builtin_fma(e[1], e[1], e[0] * e[0]));
        const real nr = __builtin_fma(e[5], e[5], __builtin_fma(e[4], e[4], e[3] * e[3]));
        cost = __builtin_fma(wt[a][1], nr, __builtin_fma(wt[a][0], np, cost));
        const real dp = __builtin_fma(e[2], J[a][2], __builtin_fma(e[1], J[a][1], e[0] * J[a][0]));
        const real dr = __builtin_fma(e[5], J[a][5], __builtin_fma(e[4], J[a][4], e[3] * J[a][3]));
        g = __builtin_fma(wt[a][1], dr, __builtin_fma(wt[a][0], dp, g));
      }
    }
  }
  // ---- cost, residuals, site positions, gradient
  if (sub == 0 && out.cost) out.cost[r] = 0.5 * cost;
#pragma unroll
  for (int a = 0; a < KM_MAX_ARMS; a++) {
    if (out.site_xpos) {
#pragma unroll
      for (int k = 0; k < 3; k++) if (sub == k) out.site_xpos[r * (KM_MAX_ARMS * 3) + a * 3 + k] = sxa[a][k];
    }
    if (out.resid) {
#pragma unroll
      for (int k = 0; k < 6; k++) if (sub == k) out.resid[r * (KM_MAX_ARMS * 6) + a * 6 + k] = res[a][k];
    }
  }
  if (out.lx && sub < NV) { out.lx[r * NX + sub] = g; out.lx[r * NX + NV + sub] = 0.0; }
  // ---- the Gauss-Newton Hessian, row by row: lane = column
  if (out.lxx) {                                         // (wave-uniform)
    real (*park)[JS] = reinterpret_cast<real (*)[JS]>(&w.f);
    if (arm_dof) {
#pragma unroll
      for (int a = 0; a < KM_MAX_ARMS; a++)
#pragma unroll
        for (int c = 0; c < 6; c++) park[sub][a * 6 + c] = J[a][c];
    }
    GSYNC();
    double* H = out.lxx + r * NX * NX;
    for (int i = 0; i < NX; i++) {
      real v = 0;
      if (i < NL + 3) {                                  // (the cube's rotation rows and the velocity rows are zeros)
        real Ji[KM_MAX_ARMS][6];
#pragma unroll
        for (int a = 0; a < KM_MAX_ARMS; a++)
#pragma unroll
          for (int c = 0; c < 6; c++) Ji[a][c] = i < NL ? park[i < NL ? i : 0][a * 6 + c] : ((c == i - NL && in.follow_cube[a] != 0 && m->arm_present[a]) ? -1.0 : 0.0);
        // one chain in a fixed order: arm 0 position c = 0..2, arm 0 rotation, then arm 1
#pragma unroll
        for (int a = 0; a < KM_MAX_ARMS; a++)
#pragma unroll
          for (int c = 0; c < 6; c++) v = sc_term(wt[a][c < 3 ? 0 : 1], Ji[a][c], J[a][c], v);
      }
      if (sub < NV) { H[(size_t)i * NX + sub] = v; H[(size_t)i * NX + NV + sub] = 0.0; }
    }
  }
  if (sub == 0 && out.status) out.status[r] = 0;
}

template <int NL, int G>
static void launch_kinrows_t(const KDeviceModel* dm, const KDeviceState& st, const KKinRowsIn& in, int n, const KKinDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(k_kinrows)<NL, G, EPB>), dim3((n + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, in, n, out);
}
template <int NL, int G>
static void launch_sitecost_t(const KDeviceModel* dm, const KDeviceState& st, const KSiteCostIn& in, int n, const KSiteCostDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(k_sitecost)<NL, G, EPB>), dim3((n + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, in, n, out);
}
KM_VARIANT_END
// ---- one (NL, G[, PAR]) variant per translation unit (the Makefile compiles this file four times)
void KM_LAUNCHER2(kinrows)(const KDeviceModel* dm, const KDeviceState& st, const KKinRowsIn& in, int n, const KKinDev& out, hipStream_t stream) {
  launch_kinrows_t<KM_VAR_NL, KM_VAR_G>(dm, st, in, n, out, stream);
}
void KM_LAUNCHER2(sitecost)(const KDeviceModel* dm, const KDeviceState& st, const KSiteCostIn& in, int n, const KSiteCostDev& out, hipStream_t stream) {
  launch_sitecost_t<KM_VAR_NL, KM_VAR_G>(dm, st, in, n, out, stream);
}
