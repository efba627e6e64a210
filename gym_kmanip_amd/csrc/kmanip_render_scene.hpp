// kmanip_render_scene.hpp -- the per-env set-up the camera render kernels share (kmanip_render.hip: depth and RGB;
// kmanip_render_labels.hip: segmentation labels): forward kinematics, the camera frame, the RGB ray cast's float32 scene with its
// bounding rectangles, and the table-span helpers of the pixel loops.
#pragma once
#include "kmanip_device.hpp"
#include <stdlib.h>

struct RenderScene {
  real xpos[KM_MAX_LINKS][3], xmat[KM_MAX_LINKS][9];
  real cam_o[3], cam_x[3], cam_y[3], cam_z[3];
  real cube_p[3], cube_R[9];
  real sph[KM_MAX_SPHERES][3];
  real focal;
  real cube_q[8];              // the cube's pose (qpos[nl .. nl + 6]) as read by lanes 0-6 at the top of the set-up
};
// what the camera / sphere lanes need from global memory, read at the top of render_fk together with the kinematics' inputs
struct RenderPre { int sl, cl, tl; real sp[3], cp[3], tp[3], tanhalf; };

// mj_kinematics, one link per lane + pointer jumping (block-wide barriers: the workgroup is 4 waves).
// Round 6: every global read of the set-up is issued at the top and waited for once -- the joint angle (HBM), the link's constants
// and its jump table for all four rounds (L2): read where they were used, each round's `jump[k][i]` cost another L2 round trip
// behind a barrier, and a launch whose 2048 workgroups all start together hides none of it (the 64 x 64 depth render: 8 of 39 us).
// lanes KM_VP_LANE0 .. of the VIS kernels: the env's visual parameters into vsv[KM_VP_N] (LDS), explicit values one per lane, the
// ranges draw one Philox block (two values) per lane
#define KM_VP_LANE0 96
__device__ __forceinline__ void render_vis_setup(const KDeviceState& st, const KVisArgs& va, int env, int i, double* vsv) {
  const int j = i - KM_VP_LANE0;
  if (va.range) {
    if (j >= 0 && j < (KM_VP_N + 1) / 2) {
      double o[2];
      km_vp_draw_pair(st.seed, st.env_id_offset + env, va.episode[env], j, va.range, o);
      vsv[2 * j] = o[0];
      if (2 * j + 1 < KM_VP_N) vsv[2 * j + 1] = o[1];
    }
  } else if (j >= 0 && j < KM_VP_N) vsv[j] = va.vp[(size_t)j * st.num_envs + env];
}

template <bool VIS>
__device__ __forceinline__ void render_fk(const KDeviceModel* dm, const KDeviceState& st, int env, int cam, RenderScene* sc, RenderPre& pre,
                                          const KVisArgs& va, double* vsv) {
  const KModelDesc* m = &dm->d;
  const int nl = m->nlink, NE = st.num_envs, i = threadIdx.x;
  const bool on = i < nl;
  const int ii = on ? i : 0;
  real R[9], p[3], Rl[9];
  int ja[4];
  // lanes 0-6: one component of the cube's pose each; lanes 64..: one collision sphere each; the camera's constants (wave-uniform)
  real cube_c = st.qpos[(size_t)(nl + (i < 7 ? i : 0)) * NE + env];
  {
    const int s = (i >= 64 && i < 64 + m->nsphere) ? i - 64 : 0;
    pre.sl = m->sphere_link[s];
    pre.sp[0] = m->sphere_pos[s][0]; pre.sp[1] = m->sphere_pos[s][1]; pre.sp[2] = m->sphere_pos[s][2];
    pre.cl = m->cam_link[cam]; pre.tl = m->cam_target_link[cam];
    for (int c = 0; c < 3; c++) { pre.cp[c] = m->cam_pos[cam][c]; pre.tp[c] = m->cam_target_pos[cam][c]; }
    pre.tanhalf = dm->x.cam_tanhalf[cam];
  }
  {
    const double* Rg = dm->x.link_R[ii];                // (normalised link_quat as a matrix: built once per model on the host)
#pragma unroll
    for (int c = 0; c < 9; c++) Rl[c] = Rg[c];
  }
  p[0] = m->link_pos[ii][0]; p[1] = m->link_pos[ii][1]; p[2] = m->link_pos[ii][2];
  real q = st.qpos[(size_t)ii * NE + env];
  int jt = m->jnt_type[ii];
#pragma unroll
  for (int k = 0; k < 4; k++) ja[k] = dm->x.jump[k][ii];
  const int rounds = dm->x.fk_rounds;
  km_pin(Rl); km_pin(p); km_pin(q, cube_c); km_pin_i(jt); km_pin_i(ja[0], ja[1]); km_pin_i(ja[2], ja[3]); km_pin(pre.sp); km_pin_i(pre.sl);
  if constexpr (VIS) render_vis_setup(st, va, env, i, vsv);     // (read by lane 0 and the scene set-up after the FK's barriers)
  if (i < 7) sc->cube_q[i] = cube_c;
  if (on) {
    if (jt == KM_JNT_SLIDE) {
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = Rl[c];
      p[0] += Rl[2] * q; p[1] += Rl[5] * q; p[2] += Rl[8] * q;
    } else {
      real sn, cs;
      km_sincos(q, &sn, &cs);
#pragma unroll
      for (int a = 0; a < 3; a++) {
        R[3 * a] = cs * Rl[3 * a] + sn * Rl[3 * a + 1];
        R[3 * a + 1] = cs * Rl[3 * a + 1] - sn * Rl[3 * a];
        R[3 * a + 2] = Rl[3 * a + 2];
      }
    }
#pragma unroll
    for (int c = 0; c < 9; c++) sc->xmat[i][c] = R[c];
    sc->xpos[i][0] = p[0]; sc->xpos[i][1] = p[1]; sc->xpos[i][2] = p[2];
  }
  __syncthreads();
  for (int k = 0; k < rounds; k++) {
    const int a = on ? (k == 0 ? ja[0] : (k == 1 ? ja[1] : (k == 2 ? ja[2] : ja[3]))) : -1;
    if (a >= 0) {
      real A[9], pa[3], Rn[9], t[3];
#pragma unroll
      for (int c = 0; c < 9; c++) A[c] = sc->xmat[a][c];
      pa[0] = sc->xpos[a][0]; pa[1] = sc->xpos[a][1]; pa[2] = sc->xpos[a][2];
      mat_vec3(t, A, p);
      p[0] = t[0] + pa[0]; p[1] = t[1] + pa[1]; p[2] = t[2] + pa[2];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = A[3 * r] * R[c] + A[3 * r + 1] * R[3 + c] + A[3 * r + 2] * R[6 + c];
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = Rn[c];
    }
    __syncthreads();
    if (a >= 0) {
#pragma unroll
      for (int c = 0; c < 9; c++) sc->xmat[i][c] = R[c];
      sc->xpos[i][0] = p[0]; sc->xpos[i][1] = p[1]; sc->xpos[i][2] = p[2];
    }
    __syncthreads();
  }
}

// Per-env scene after the FK: lane 0 builds the camera frame (mj_camlight, targetbody) and the cube pose, lanes 64.. one sphere
// centre each (another wave: in parallel with lane 0).  Caller synchronises afterwards.  VIS: the camera sits at cam_pos + the env's
// KM_VP_CAM_OFFSET (in cam_link's frame), exactly where a model with that cam_pos puts it (model.py with_visual_params).
template <bool VIS>
__device__ __forceinline__ void render_camera(const KDeviceModel* dm, const KDeviceState& st, int env, int cam, int height, RenderScene* sc, const RenderPre& pre,
                                              const double* vsv) {
  const KModelDesc* m = &dm->d;
  const int t = threadIdx.x;
  if (t == 0) {
    // camera frame: z = (cam - target)/|.|, x = (0,0,1) x z, y = z x x; a link of -1 = world frame
    const int cl = pre.cl, tl = pre.tl;
    real co[3], to[3], v[3];
    real cp[3] = {pre.cp[0], pre.cp[1], pre.cp[2]};
    if constexpr (VIS) { for (int c = 0; c < 3; c++) cp[c] += vsv[KM_VP_CAM_OFFSET + c]; }
    real tp[3] = {pre.tp[0], pre.tp[1], pre.tp[2]};
    if (cl < 0) { co[0] = cp[0]; co[1] = cp[1]; co[2] = cp[2]; }
    else { mat_vec3(v, sc->xmat[cl], cp); co[0] = sc->xpos[cl][0] + v[0]; co[1] = sc->xpos[cl][1] + v[1]; co[2] = sc->xpos[cl][2] + v[2]; }
    if (tl < 0) { to[0] = tp[0]; to[1] = tp[1]; to[2] = tp[2]; }
    else { mat_vec3(v, sc->xmat[tl], tp); to[0] = sc->xpos[tl][0] + v[0]; to[1] = sc->xpos[tl][1] + v[1]; to[2] = sc->xpos[tl][2] + v[2]; }
    real z[3] = {co[0] - to[0], co[1] - to[1], co[2] - to[2]}, up[3] = {0, 0, 1}, x[3], y[3];
    normalize3_fast(z);
    cross3(x, up, z); normalize3_fast(x);
    cross3(y, z, x); normalize3_fast(y);
    for (int c = 0; c < 3; c++) { sc->cam_o[c] = co[c]; sc->cam_x[c] = x[c]; sc->cam_y[c] = y[c]; sc->cam_z[c] = z[c]; }
    sc->focal = (0.5 * height) / pre.tanhalf;
    real cq[4];
    for (int c = 0; c < 3; c++) sc->cube_p[c] = sc->cube_q[c];
    for (int c = 0; c < 4; c++) cq[c] = sc->cube_q[3 + c];
    normalize4_fast(cq);
    quat2mat(sc->cube_R, cq);
  } else if (t >= 64 && t < 64 + m->nsphere) {
    const int s = t - 64, l = pre.sl;
    real sl[3] = {pre.sp[0], pre.sp[1], pre.sp[2]}, v[3];
    mat_vec3(v, sc->xmat[l], sl);
    sc->sph[s][0] = sc->xpos[l][0] + v[0]; sc->sph[s][1] = sc->xpos[l][1] + v[1]; sc->sph[s][2] = sc->xpos[l][2] + v[2];
  }
}

// ---- RGB -----------------------------------------------------------------------------------------------------------
#define KM_RGB_MAXSPH KM_RENDER_MAXVIS        // visible spheres (the two finger tips per arm)
struct RgbScene {              // float32 view of the scene for the pixel loop, built by lane 0 from the float64 RenderScene
  float o[3], X[3], Y[3], Z[3], inv_f, tz, zfar;
  float ol[3], DX[3], DY[3], DZ[3], half[3], R[9];       // cube: camera origin and the ray basis in the cube frame, half sizes, rotation
  float oc[KM_RGB_MAXSPH][3], cc[KM_RGB_MAXSPH], ir[KM_RGB_MAXSPH];   // spheres: origin - centre, |oc|^2 - r^2, 1 / r
  int nsph;
  // the table top seen from the camera: a ray direction d = X dx + Y dy - Z passes through the rectangle iff the four edge functions
  // te_a[i] dx + te_b[i] dy + te_c[i] (triple products of d with consecutive corners as seen from the camera, oriented so that the
  // rectangle's centre is positive) are all positive; te_i[i] = -1 / te_a[i] turns a row's values into its column span
  float te_a[4], te_b[4], te_c[4], te_i[4];
  int ubox[4];                     // union of the rectangles below
  int box[1 + KM_RGB_MAXSPH][4];   // screen-space bounding rectangle of the cube [0] and of every visible sphere: r0, r1, c0, c1 (inclusive)
  float tab_L;                 // directional-light sum on the table's normal
};
// the env's colours and light terms, float32, for the VIS pixel loop (a separate LDS object: the default kernel's layout stays as it is)
struct RgbVis {
  float col[3][3];             // material colour [mat - 1][channel]: table, cube, robot
  float k255[3];               // 255 x table colour: the table-only quads' per-channel factor
  uint32_t bg;                 // background pixel r | g << 8 | b << 16
  uint32_t bgw[3];             // four background pixels as the three dwords of a quad
  float amb, hl, ds;           // ambient, headlight diffuse, 0.3 x directional scale
};
// pixel (row, col) of the world point P; false if it is not safely in front of the camera
__device__ __forceinline__ bool rgb_project(const RenderScene& sc, const real* P, int height, int width, real& row, real& col) {
  const real pc[3] = {P[0] - sc.cam_o[0], P[1] - sc.cam_o[1], P[2] - sc.cam_o[2]};
  const real zc = -dot3(pc, sc.cam_z);
  if (!(zc > 1e-3)) return false;
  const real s = sc.focal / zc;
  col = dot3(pc, sc.cam_x) * s + 0.5 * width - 0.5;
  row = -dot3(pc, sc.cam_y) * s + 0.5 * height - 0.5;
  return true;
}
// The per-env set-up of the pixel loop, spread over the first 17 lanes of the workgroup (one lane did all of it in ~22 us, a tenth of
// a 2048-image launch at two residency rounds): lanes 0-7 project one cube corner each, lanes 8-11 one visible sphere each (its ray
// constants and rectangle), lanes 12-15 one table edge each, lane 16 the camera / cube-frame scalars; lane 0 then folds the corners
// into the cube's rectangle and the rectangles into their union.
struct RgbTmp { real row[8], col[8]; int ok[8]; };
template <bool VIS>
__device__ __forceinline__ void rgb_scene(const KDeviceModel* dm, const RenderScene& sc, int height, int width, RgbScene* g, RgbTmp* tmp, int t,
                                          RgbVis* gv, const double* vsv) {
  const KModelDesc* m = &dm->d;
  // bounding rectangles, one per object (an object that is not safely in front of the camera gets the whole image): the cube's
  // eight corners; a sphere's centre +- a conservative projected radius
  auto put = [&](int o, bool ok, real r0, real r1, real c0, real c1) {
    if (!ok) { g->box[o][0] = 0; g->box[o][1] = height - 1; g->box[o][2] = 0; g->box[o][3] = width - 1; return; }
    g->box[o][0] = (int)fmax(floor(r0) - 1, -1.0); g->box[o][1] = (int)fmin(ceil(r1) + 1, (real)height);
    g->box[o][2] = (int)fmax(floor(c0) - 1, -1.0); g->box[o][3] = (int)fmin(ceil(c1) + 1, (real)width);
  };
  if (t < 8) {
    const real loc[3] = {(t & 1 ? 1 : -1) * m->cube_half[0], (t & 2 ? 1 : -1) * m->cube_half[1], (t & 4 ? 1 : -1) * m->cube_half[2]};
    real P[3], row = 0, col = 0;
    mat_vec3(P, sc.cube_R, loc);
    P[0] += sc.cube_p[0]; P[1] += sc.cube_p[1]; P[2] += sc.cube_p[2];
    tmp->ok[t] = rgb_project(sc, P, height, width, row, col);
    tmp->row[t] = row; tmp->col[t] = col;
  } else if (t < 8 + KM_RGB_MAXSPH) {
    // the (t - 8)-th visible sphere (the list is built on the host; kmanip_create refuses models with more than four)
    const int s = t - 8 < dm->x.nvis ? dm->x.vis_sphere[t - 8] : -1;
    if (s >= 0) {
      const int ns = t - 8;
      const real rad = m->sphere_radius[s];
      const real oc[3] = {sc.cam_o[0] - sc.sph[s][0], sc.cam_o[1] - sc.sph[s][1], sc.cam_o[2] - sc.sph[s][2]};
      for (int c = 0; c < 3; c++) g->oc[ns][c] = (float)oc[c];
      g->cc[ns] = (float)(dot3(oc, oc) - rad * rad); g->ir[ns] = (float)(1.0 / rad);
      real row = 0, col = 0;
      const real zc = dot3(oc, sc.cam_z);                                  // depth of the centre along the optical axis
      const bool ok = rgb_project(sc, sc.sph[s], height, width, row, col) && zc - rad > 1e-3;
      const real pr = ok ? 1.5 * sc.focal * rad / (zc - rad) + 1.0 : 0.0;  // (off-axis spheres project to ellipses: generous)
      put(1 + ns, ok, row - pr, row + pr, col - pr, col + pr);
    }
  } else if (t < 16) {
    const int i = t - 12;
    const real* tr = m->table_rect;
    if (isfinite(tr[0]) && isfinite(tr[1]) && isfinite(tr[2]) && isfinite(tr[3])) {
      // corner i and its successor, counter-clockwise from (x_lo, y_lo)
      const real ax = (i == 0 || i == 3) ? tr[0] : tr[1], ay = i < 2 ? tr[2] : tr[3];
      const real bx = (i == 3 || i == 2) ? tr[0] : tr[1], by = (i == 0 || i == 3) ? tr[2] : tr[3];
      const real dz = m->table_z - sc.cam_o[2];
      const real Va[3] = {ax - sc.cam_o[0], ay - sc.cam_o[1], dz}, Vb[3] = {bx - sc.cam_o[0], by - sc.cam_o[1], dz};
      const real Vc[3] = {0.5 * (tr[0] + tr[1]) - sc.cam_o[0], 0.5 * (tr[2] + tr[3]) - sc.cam_o[1], dz};
      real n[3];
      cross3(n, Va, Vb);
      const real sgn = dot3(n, Vc) < 0 ? -1.0 : 1.0;
      const real a = sgn * dot3(n, sc.cam_x), b = sgn * dot3(n, sc.cam_y), c = -sgn * dot3(n, sc.cam_z);
      g->te_a[i] = (float)a; g->te_b[i] = (float)b; g->te_c[i] = (float)c;
      g->te_i[i] = g->te_a[i] != 0.0f ? -1.0f / g->te_a[i] : 0.0f;
    } else { g->te_a[i] = 0; g->te_b[i] = 0; g->te_c[i] = 1; g->te_i[i] = 0; }   // the infinite plane: always inside
  } else if (t == 16) {
    for (int c = 0; c < 3; c++) { g->o[c] = (float)sc.cam_o[c]; g->X[c] = (float)sc.cam_x[c]; g->Y[c] = (float)sc.cam_y[c]; g->Z[c] = (float)sc.cam_z[c]; }
    g->inv_f = (float)(1.0 / sc.focal); g->tz = (float)m->table_z; g->zfar = (float)m->cam_zfar;
    real rel[3] = {sc.cam_o[0] - sc.cube_p[0], sc.cam_o[1] - sc.cube_p[1], sc.cam_o[2] - sc.cube_p[2]}, v[3];
    matT_vec3(v, sc.cube_R, rel); for (int c = 0; c < 3; c++) g->ol[c] = (float)v[c];
    matT_vec3(v, sc.cube_R, sc.cam_x); for (int c = 0; c < 3; c++) g->DX[c] = (float)v[c];
    matT_vec3(v, sc.cube_R, sc.cam_y); for (int c = 0; c < 3; c++) g->DY[c] = (float)v[c];
    matT_vec3(v, sc.cube_R, sc.cam_z); for (int c = 0; c < 3; c++) g->DZ[c] = (float)v[c];
    for (int c = 0; c < 3; c++) g->half[c] = (float)m->cube_half[c];
    for (int c = 0; c < 9; c++) g->R[c] = (float)sc.cube_R[c];
    g->nsph = dm->x.nvis;
    g->tab_L = 0.3f * (0.57735026919f + 0.57735026919f + 0.70710678119f);    // sum_l max(0, L_l . (0,0,1)), scene.xml:11-13
    if constexpr (VIS) g->tab_L = (float)vsv[KM_VP_DIRECTIONAL] * g->tab_L;
  } else if (VIS && t == 17) {
    // material order of rgb_pixel's `mat`: 1 table, 2 cube, 3 robot
    const int base[3] = {KM_VP_TABLE_RGB, KM_VP_CUBE_RGB, KM_VP_ROBOT_RGB};
    for (int m2 = 0; m2 < 3; m2++)
      for (int c = 0; c < 3; c++) gv->col[m2][c] = (float)vsv[base[m2] + c];
    for (int c = 0; c < 3; c++) gv->k255[c] = (float)(255.0 * vsv[KM_VP_TABLE_RGB + c]);
    uint32_t b[3];
    for (int c = 0; c < 3; c++) b[c] = (uint32_t)floor(255.0 * vsv[KM_VP_BACKGROUND_RGB + c] + 0.5);
    gv->bg = b[0] | (b[1] << 8) | (b[2] << 16);
    gv->bgw[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[0] << 24);
    gv->bgw[1] = b[1] | (b[2] << 8) | (b[0] << 16) | (b[1] << 24);
    gv->bgw[2] = b[2] | (b[0] << 8) | (b[1] << 16) | (b[2] << 24);
    gv->amb = (float)vsv[KM_VP_AMBIENT]; gv->hl = (float)vsv[KM_VP_HEADLIGHT]; gv->ds = (float)vsv[KM_VP_DIRECTIONAL] * 0.3f;
  }
  __syncthreads();
  if (t == 0) {
    real r0 = 1e30, r1 = -1e30, c0 = 1e30, c1 = -1e30;
    bool ok = true;
    for (int k = 0; k < 8; k++) {
      ok = ok && tmp->ok[k];
      r0 = fmin(r0, tmp->row[k]); r1 = fmax(r1, tmp->row[k]); c0 = fmin(c0, tmp->col[k]); c1 = fmax(c1, tmp->col[k]);
    }
    put(0, ok, r0, r1, c0, c1);
    for (int k = 0; k < 4; k++) {
      int u = g->box[0][k];
      for (int o = 1; o <= g->nsph; o++) u = (k & 1) ? max(u, g->box[o][k]) : min(u, g->box[o][k]);
      g->ubox[k] = u;
    }
  }
}

// does the ray direction (dx, dy) pass through the table top?
__device__ __forceinline__ bool rgb_over_table(const RgbScene& g, float dx, float dy) {
  bool in = true;
#pragma unroll
  for (int i = 0; i < 4; i++) in = in && (g.te_a[i] * dx + (g.te_b[i] * dy + g.te_c[i])) > 0.0f;
  return in;
}
// the open interval of dx over which a row (dy) crosses the table top: lo >= hi = not at all
__device__ __forceinline__ void rgb_table_span(const RgbScene& g, float dy, float& lo, float& hi) {
  lo = -INFINITY; hi = INFINITY;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float e = g.te_b[i] * dy + g.te_c[i], a = g.te_a[i], x = e * g.te_i[i];
    if (a > 0.0f) lo = fmaxf(lo, x);
    else if (a < 0.0f) hi = fminf(hi, x);
    else if (!(e > 0.0f)) lo = INFINITY;
  }
}
