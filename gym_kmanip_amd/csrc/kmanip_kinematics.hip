// kmanip_kinematics.hip -- link and site poses, site Jacobians, joint-space inertia and bias forces of every env's CURRENT state in ONE
// launch (gfx950, wave64): kmanip_kinematics.
//
// What dm_control users read off physics.data after a physics.forward(): data.xpos / data.xmat of the link bodies, the pose of the
// end-effector sites, mj_jacSite, mj_fullM and data.qfrc_bias.  The tree passes are the step's own -- the headers of kmanip_dyn.hip,
// included here under the same build macros: the phases of step1_products up to, and not including, invert_mass (fk_parallel, the
// bias-wrench pass, the composite / mass / bias-projection pass) in all three lane mappings, without collision, constraint
// assembly, inversion or solve -- in a translation unit of its own, so that the k_step / k_reset / k_observe / k_forces objects are
// the ones they were, to the register.  After them M sits in Ws::Minv (both triangles; mass_symmetrize completes the two-row path
// without a block split) and the bias forces in Ws::bias.  New here: the site pose from its link's frame, the Jacobian columns
// (lane = dof, ancestor test through LModel::anc), the site velocity (gsum over the dofs) and the dense rows of M with the cube's
// diagonal.  Nothing depends on the solver: the workspace layout is private to a kernel, so the Newton layout serves PGS handles
// too.  Both parameter builds, 64 / G envs per wave like k_observe.  The handle is read only: nothing of KDeviceState is written.
#include "kmanip_ik_coop.hpp"
#include <stdlib.h>
#include "kmanip_dyn_variant.hpp"      // (the build macros; KM_VAR_SOLVER is always 1 here, KM_VAR_FRC left to its default)
static_assert(KM_VAR_SOLVER == 1, "k_kinematics is built with the Newton workspace layout");

// `count` zeros into env e's row of a field (consecutive lanes, consecutive addresses)
template <int G>
__device__ __forceinline__ void kin_zero(double* p, size_t e, int count, int sub) {
  if (p) for (int i = sub; i < count; i += G) p[e * count + i] = 0.0;
}
// a non-finite state: status 1, every other output of the env 0
template <int NL, int G>
__device__ __forceinline__ void write_kin_bad(const KKinDev& out, int env, int sub) {
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
  if (sub == 0 && out.status) out.status[e] = 1;
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

template <int NL, int G, int EPB>
__global__ __launch_bounds__(64) void KM_KERNEL(k_kinematics)(const KDeviceModel* __restrict__ dm, KDeviceState st, KKinDev out) {
  constexpr int NV = Dim<NL>::NV;
  static_assert(NV <= G, "lane = dof");
  __shared__ Ws<NL> ws[EPB];
  __shared__ LModel<NL> lm;
  const KModelDesc* m = &dm->d;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int env;
  if (!query_env<NL, EPB>(lm, dm, st, grp, env)) return;      // whole group exits together
  Ws<NL>& w = ws[grp];
  real invm = 0;      // (not needed: nothing is inverted)
  query_load<NL, G>(w, dm, st, env, sub, invm);
  GSYNC();
  // a non-finite state (k_observe's test): status 1, nothing else computed
  if (state_nonfinite<NL, G>(w, sub)) { write_kin_bad<NL, G>(out, env, sub); return; }
  kin_tree<NL, G>(w, lm, m, sub);
  const size_t e = (size_t)env;
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

template <int NL, int G>
static void launch_kinematics_t(const KDeviceModel* dm, const KDeviceState& st, const KKinDev& out, hipStream_t stream) {
  constexpr int EPB = 64 / G;
  hipLaunchKernelGGL((KM_KERNEL(k_kinematics)<NL, G, EPB>), dim3((st.num_envs + EPB - 1) / EPB), dim3(64), 0, stream, dm, st, out);
}
KM_VARIANT_END
// ---- one (NL, G[, PAR]) variant per translation unit (the Makefile compiles this file four times)
void KM_LAUNCHER2(kinematics)(const KDeviceModel* dm, const KDeviceState& st, const KKinDev& out, hipStream_t stream) {
  launch_kinematics_t<KM_VAR_NL, KM_VAR_G>(dm, st, out, stream);
}
