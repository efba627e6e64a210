// kmanip_dyn_constraints.hpp -- one of the phase headers kmanip_dyn_variant.hpp includes (inside the variant namespace) into each per-variant translation unit: frames, collision, impedance, constraint rows and the PGS solver.
#pragma once
// mju_makeFrame
__device__ __forceinline__ void make_frame(real* fr) {
  normalize3_fast(fr);
  real y[3] = {0, 0, 0};
  if (fr[1] < 0.5 && fr[1] > -0.5) y[1] = 1; else y[2] = 1;
  real t = dot3(fr, y);
  y[0] -= t * fr[0]; y[1] -= t * fr[1]; y[2] -= t * fr[2];
  normalize3_fast(y);
  fr[3] = y[0]; fr[4] = y[1]; fr[5] = y[2];
  cross3(fr + 6, fr, fr + 3);
}

// contact frame of every contact whose normal is the table normal (+z): mju_makeFrame((0,0,1)) = rows n, t1, t2
#define KM_PLANE_FRAME {0, 0, 1, 0, 1, 0, -1, 0, 0}
// narrow phase for the fixed candidate set, written into fixed slots: plane-box (first 4 corners below the
// table -> slots 0..3 in corner order), sphere-box (slots 4.., the first NSS penetrating spheres), plane-sphere (slots 4 + NSS..).
// One candidate per lane: lanes 0..7 test the cube corners (slot = rank among the penetrating corners, from the
// group's ballot bits), lanes 8..8+NSPH-1 their collision sphere against cube and table.
// the table top is a rectangle (kmanip.h table_rect): a point is over it while its x, y lie inside.  tr = the four bounds, fetched
// ONCE by the caller (one scalar load); `&` not `&&`: four compares, no branch per bound
__device__ __forceinline__ bool over_table(const real (&tr)[4], const real* p) {
  return (p[0] >= tr[0]) & (p[0] <= tr[1]) & (p[1] >= tr[2]) & (p[1] <= tr[3]);
}

// NEAR (the trailing mj_step1 of the two-arm kernels only): also report whether some collider is within KM_NEAR_MARGIN of the cube
// without touching it -- the onset of the coupled Newton loop is what k_sort_envs' last-step counters cannot see coming
#define KM_NEAR_MARGIN 0.015      // (the default of callers that pass none; the handle's value is KDeviceState::near_margin: kmanip_api.hip)
template <int NL, int G, bool NEAR = false>
__device__ __forceinline__ int collide_parallel(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub, real near_margin = KM_NEAR_MARGIN) {
  constexpr int NSPH = Dim<NL>::NSPH, NSS = Dim<NL>::NSS, NST = Dim<NL>::NST;
  static_assert(8 + NSPH <= G, "one lane per collision candidate");
  uint32_t mask = 0, act = 0;
  // (round 6) the cube's pose and this lane's candidate (sphere s = sub - 8: link, centre, radius, capsule segment) in one batch;
  // the candidate's link frame -- the one dependent read -- in a second
  const int sidx = sub >= 8 && sub - 8 < NSPH ? sub - 8 : 0;
  real cp[3] = {w.qpos[NL], w.qpos[NL + 1], w.qpos[NL + 2]}, cmat[9];
#pragma unroll
  for (int k = 0; k < 9; k++) cmat[k] = w.k.cube_mat[k];
  int lnk = lm.sph_link[sidx], nsph_ = lm.nsph;
  real slp[3] = {lm.sph_pos[sidx][0], lm.sph_pos[sidx][1], lm.sph_pos[sidx][2]}, sgp[3] = {lm.sph_seg[sidx][0], lm.sph_seg[sidx][1], lm.sph_seg[sidx][2]}, radp = lm.sph_rad[sidx];
  km_pin(cp); km_pin(cmat); km_pin(slp, sgp); km_pin(radp); km_pin_i(lnk, nsph_);
  real lmat[9], lpos[3];
#pragma unroll
  for (int k = 0; k < 9; k++) lmat[k] = w.k.xmat[lnk][k];
  lpos[0] = w.k.xpos[lnk][0]; lpos[1] = w.k.xpos[lnk][1]; lpos[2] = w.k.xpos[lnk][2];
  uint32_t lanc = lm.anc[lnk];
  const real tr[4] = {m->table_rect[0], m->table_rect[1], m->table_rect[2], m->table_rect[3]};
  bool below = false;
  real c[3] = {0, 0, 0}, dist = 0;
  if (sub < 8) {
    const real loc[3] = {(sub & 1 ? 1 : -1) * m->cube_half[0], (sub & 2 ? 1 : -1) * m->cube_half[1], (sub & 4 ? 1 : -1) * m->cube_half[2]};
    mat_vec3(c, cmat, loc);
    c[0] += cp[0]; c[1] += cp[1]; c[2] += cp[2];
    dist = c[2] - m->table_z;
    below = (dist < 0) & over_table(tr, c);
  }
  const unsigned long long bal = __ballot(below);
  const uint32_t m8 = (uint32_t)(bal >> ((threadIdx.x & 63) - sub)) & 0xFFu;
  if (below) {
    const int n = __popc(m8 & ((1u << sub) - 1u));
    if (n < 4) {
      const real fr[9] = KM_PLANE_FRAME;
#pragma unroll
      for (int k = 0; k < 9; k++) w.c_frame[n][k] = fr[k];
      w.c_dist[n] = dist;
      w.c_pos[n][0] = c[0]; w.c_pos[n][1] = c[1]; w.c_pos[n][2] = c[2] - 0.5 * dist;
      mask |= KM_CON_CUBE_TABLE(sub); act |= 1u << n;
    }
  }
  const int nsph = nsph_;
  const int s = sub - 8;
  bool hitc = false, hitt = false;
  real ctr[3] = {0, 0, 0}, ctrt[3] = {0, 0, 0}, nloc[3] = {0, 0, 0}, d1 = 0, d2 = 0, rad = 0;
  km_pin(lmat); km_pin(lpos); asm volatile("" : "+v"(lanc));
  if (sub >= 8 && sub < 8 + nsph) {
    real sl[3] = {slp[0], slp[1], slp[2]}, rel[3], loc[3], cl[3];
    mat_vec3(ctr, lmat, sl);
#pragma unroll
    for (int a = 0; a < 3; a++) ctr[a] += lpos[a];
    rad = radp;
    // table plane (geom1) - sphere (geom2): the end sphere itself (a capsule meets a plane in its end spheres)
    d2 = ctr[2] - m->table_z - rad;
    hitt = (d2 < 0) & over_table(tr, ctr);
    ctrt[0] = ctr[0]; ctrt[1] = ctr[1]; ctrt[2] = ctr[2];
    // capsule section (kmanip.h sphere_seg): against the cube the collider is the point of the link's segment closest to the
    // cube centre -- a sphere sliding along the link
    {
      const real sg[3] = {sgp[0], sgp[1], sgp[2]};
      real sw[3];
      mat_vec3(sw, lmat, sg);
      const real ss = dot3(sw, sw);
      if (ss > 0) {
        real t = ((cp[0] - ctr[0]) * sw[0] + (cp[1] - ctr[1]) * sw[1] + (cp[2] - ctr[2]) * sw[2]) / ss;
        t = fmin(fmax(t, 0.0), 1.0);
#pragma unroll
        for (int a = 0; a < 3; a++) ctr[a] += t * sw[a];
      }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) rel[a] = ctr[a] - cp[a];
    // sphere (geom1) - cube box (geom2)
    matT_vec3(loc, cmat, rel);
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; a++) { cl[a] = fmin(fmax(loc[a], -m->cube_half[a]), m->cube_half[a]); if (cl[a] != loc[a]) inside = false; }
    if (!inside) {
      nloc[0] = cl[0] - loc[0]; nloc[1] = cl[1] - loc[1]; nloc[2] = cl[2] - loc[2];
      real dn = normalize3_fast(nloc);
      d1 = dn - rad;
    } else {
      int best = 0; real bd = INFINITY;
#pragma unroll
      for (int a = 0; a < 3; a++) { real dd = m->cube_half[a] - fabs(loc[a]); if (dd < bd) { bd = dd; best = a; } }
      real sg = (best == 0 ? loc[0] : (best == 1 ? loc[1] : loc[2])) >= 0 ? -1.0 : 1.0;
      if (best == 0) nloc[0] = sg; else if (best == 1) nloc[1] = sg; else nloc[2] = sg;
      d1 = -bd - rad;
    }
    hitc = d1 < 0;
  }
  // the first NSS penetrating spheres of each kind (sphere order) get the slots: rank = penetrating spheres on lower lanes
  const uint32_t below_me = (1u << sub) - 1u;
  const uint32_t mc = (uint32_t)(__ballot(hitc) >> ((threadIdx.x & 63) - sub)) & below_me;
  const uint32_t mt = (uint32_t)(__ballot(hitt) >> ((threadIdx.x & 63) - sub)) & below_me;
  if (hitc && __popc(mc) < NSS) {
    const int n = 4 + __popc(mc);
    real fr[9];
    mat_vec3(fr, cmat, nloc);
    make_frame(fr);
#pragma unroll
    for (int k = 0; k < 9; k++) w.c_frame[n][k] = fr[k];
    w.c_dist[n] = d1;
#pragma unroll
    for (int a = 0; a < 3; a++) w.c_pos[n][a] = ctr[a] + fr[a] * (rad + 0.5 * d1);
    w.slot_sph[n] = s; w.slot_anc[n] = lanc;
    mask |= KM_CON_SPHERE_CUBE(s); act |= 1u << n;
  }
  if (hitt && __popc(mt) < NST) {
    const int n = 4 + NSS + __popc(mt);
    const real fr[9] = KM_PLANE_FRAME;
#pragma unroll
    for (int k = 0; k < 9; k++) w.c_frame[n][k] = fr[k];
    w.c_dist[n] = d2;
    w.c_pos[n][0] = ctrt[0]; w.c_pos[n][1] = ctrt[1]; w.c_pos[n][2] = ctrt[2] - (rad + 0.5 * d2);
    w.slot_sph[n] = s; w.slot_anc[n] = lanc;
    mask |= KM_CON_SPHERE_TABLE(s); act |= 1u << n;
  }
  mask = (uint32_t)gor<G>((int)mask);
  act = (uint32_t)gor<G>((int)act);
  if (sub == 0) {
    w.cact = act; w.contact_mask = mask;
    w.touch_ct = (mask & KM_CON_ANY_CUBE_TABLE) != 0;
  }
  if constexpr (NEAR) return gor<G>((int)(sub >= 8 && sub < 8 + nsph && d1 < near_margin));
  return 0;
}

// MuJoCo impedance d(r) from the staged, pre-clamped solimp constants: no divide, no pow (power is 1 or 2: kmanip_create
// refuses any other value; every reference model uses the default 2)
template <class IMP> __device__ __forceinline__ real impedance_c(const IMP& p, real pos) {
  // (round 6: the seven staged constants fetched together and the cases as selects -- as early returns each case read its own
  // constants from LDS behind its own branch, eight round trips in a row; same expressions, same value)
  real d0 = p.d0, dw = p.dw, iw = p.iw, mid = p.mid, imid = p.imid, i1mid = p.i1mid;
  int mode = p.mode;
  km_pin(d0, dw, iw, mid, imid, i1mid); km_pin_i(mode);
  const real x = fabs(pos) * iw;
  const real y = mode == 1 ? x : ((x <= mid) ? x * x * imid : 1 - (1 - x) * (1 - x) * i1mid);
  real r = d0 + y * (dw - d0);
  r = x <= 0 ? d0 : r;
  r = x >= 1 ? dw : r;
  return mode == 0 ? 0.5 * (d0 + dw) : r;
}
// the same from constants the caller fetched (together with its other inputs)
__device__ __forceinline__ real impedance_v(real d0, real dw, real iw, real mid, real imid, real i1mid, int mode, real pos) {
  const real x = fabs(pos) * iw;
  const real y = mode == 1 ? x : ((x <= mid) ? x * x * imid : 1 - (1 - x) * (1 - x) * i1mid);
  real r = d0 + y * (dw - d0);
  r = x <= 0 ? d0 : r;
  r = x >= 1 ? dw : r;
  return mode == 0 ? 0.5 * (d0 + dw) : r;
}
template <class IMP> __device__ __forceinline__ void stage_imp(IMP& p, const real* si) {
  p.d0 = fmin(fmax(si[0], MJ_MINIMP), MJ_MAXIMP); p.dw = fmin(fmax(si[1], MJ_MINIMP), MJ_MAXIMP);
  const real width = fmax(MJ_MINVAL, si[2]);
  p.mid = fmin(fmax(si[3], MJ_MINIMP), MJ_MAXIMP);
  p.iw = 1.0 / width; p.imid = 1.0 / p.mid; p.i1mid = 1.0 / (1 - p.mid);
  p.mode = (p.d0 == p.dw || width <= MJ_MINVAL) ? 0 : (fmax(1.0, si[4]) == 1 ? 1 : 2);
}
// MuJoCo impedance / reference acceleration parameters (general form; staging only)
__device__ __forceinline__ real impedance(const real* si, real pos) {
  real d0 = fmin(fmax(si[0], MJ_MINIMP), MJ_MAXIMP), dw = fmin(fmax(si[1], MJ_MINIMP), MJ_MAXIMP);
  real width = fmax(MJ_MINVAL, si[2]), mid = fmin(fmax(si[3], MJ_MINIMP), MJ_MAXIMP), power = fmax(1.0, si[4]);
  if (d0 == dw || width <= MJ_MINVAL) return 0.5 * (d0 + dw);
  real x = fabs(pos) / width, y;
  if (x >= 1) return dw;
  if (x <= 0) return d0;
  if (power == 1) y = x;
  else y = (x <= mid) ? x * x / mid : 1 - (1 - x) * (1 - x) / (1 - mid);   // power 2, MuJoCo's default (others refused at create)
  (void)power;
  return d0 + y * (dw - d0);
}
__device__ __forceinline__ void get_kb(const KModelDesc* m, const real* sr, const real* si, real& kk, real& bb) {
  real tc = fmax(sr[0], 2 * m->timestep), dr = sr[1];
  real dmax = fmin(fmax(si[1], MJ_MINIMP), MJ_MAXIMP);
  bb = 2 / (dmax * tc);
  kk = 1 / (dmax * dmax * tc * tc * dr * dr);
}

// linear/angular velocity Jacobian column of dof j for a world point `pt` fixed to body `body`
template <int NL>
__device__ __forceinline__ void point_jac_col(const Ws<NL>& w, const LModel<NL>& lm, int body, int j, const real* pt,
                                              real* jp, real* jr) {
  jp[0] = 0; jp[1] = 0; jp[2] = 0; jr[0] = 0; jr[1] = 0; jr[2] = 0;
  if (body < 0) return;
  if (body < NL) {
    if (j >= NL || !((lm.anc[body] >> j) & 1u)) return;
    if (lm.jtype[j] == KM_JNT_SLIDE) { jp[0] = w.k.axis[j][0]; jp[1] = w.k.axis[j][1]; jp[2] = w.k.axis[j][2]; }
    else {
      real ax[3] = {w.k.axis[j][0], w.k.axis[j][1], w.k.axis[j][2]};
      real r[3] = {pt[0] - w.k.xpos[j][0], pt[1] - w.k.xpos[j][1], pt[2] - w.k.xpos[j][2]};
      cross3(jp, ax, r);
      jr[0] = ax[0]; jr[1] = ax[1]; jr[2] = ax[2];
    }
    return;
  }
  if (j < NL) return;
  const int e = j - NL;
  if (e < 3) { jp[0] = e == 0; jp[1] = e == 1; jp[2] = e == 2; return; }
  const int k = e - 3;
  real col[3] = {w.k.cube_mat[k], w.k.cube_mat[3 + k], w.k.cube_mat[6 + k]};
  real r[3] = {pt[0] - w.qpos[NL], pt[1] - w.qpos[NL + 1], pt[2] - w.qpos[NL + 2]};
  cross3(jp, col, r);
  jr[0] = col[0]; jr[1] = col[1]; jr[2] = col[2];
}

// arm single-dof rows in mj_makeConstraint order (friction loss, then limits), enumerated by one lane
template <int NL>
__device__ __forceinline__ void scalar_rows_serial(Ws<NL>& w, const LModel<NL>& lm) {
  int n = 0;
  for (int j = 0; j < NL; j++) {
    real fl = lm.floss[j];
    if (fl > 0) { w.s_dof[n] = j; w.s_type[n] = 0; w.s_sign[n] = 1; w.s_pos[n] = 0; w.s_floss[n] = fl; n++; }
  }
  for (int j = 0; j < NL; j++) {
    real dl = w.qpos[j] - lm.range[j][0], du = lm.range[j][1] - w.qpos[j];
    if (dl < 0) { w.s_dof[n] = j; w.s_type[n] = 1; w.s_sign[n] = 1; w.s_pos[n] = dl; w.s_floss[n] = 0; n++; }
    if (du < 0) { w.s_dof[n] = j; w.s_type[n] = 1; w.s_sign[n] = -1; w.s_pos[n] = du; w.s_floss[n] = 0; n++; }
  }
  w.ns = n;
}

// Constraint assembly.  Arm single-dof rows: parameters in LDS (parallel over rows).  Contacts: this lane's
// Jacobian column of each basis row in registers (cr.jb), B = M^-1 J^T columns (cr.bb), then per-contact
// Gram / edge tables (group-uniform) in LDS.
template <int NL, int G>
__device__ __forceinline__ void build_constraints(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub,
                                                  CReg<NL>& cr, real invm) {
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC;
  for (int r = sub; r < w.ns; r += G) {
    const int j = w.s_dof[r];
    real Ad = w.Minv[j][j];
    real pos = w.s_pos[r];
    real imp = impedance_c(lm.imp[0], pos), kk = lm.kb[0][0], bb = lm.kb[0][1];
    const real R = fmax(MJ_MINVAL, (1 - imp) * frcp(imp) * lm.dofw[j]);      // efc_diagApprox = dof_invweight0, not the exact A_ii
    w.s_R[r] = R;
    w.s_den[r] = Ad + R;
    w.s_inv[r] = 1.0 / (Ad + R);
    w.s_aref[r] = -bb * (w.s_sign[r] * w.qvel[j]) - kk * imp * pos;
  }
  const uint32_t act = w.cact;
  // ---- J columns (needs kinematics, which the Gram tables will overwrite: finish all slots first)
#pragma unroll
  for (int c = 0; c < NC; c++) {
    cr.jb[c][0] = 0; cr.jb[c][1] = 0; cr.jb[c][2] = 0; cr.jb[c][3] = 0;
    if (((act >> c) & 1u) && sub < NV) {
      const int kind = slot_kind<NL>(c);
      const int link = kind == 0 ? -1 : lm.sph_link[w.slot_sph[c]];
      const int b1 = kind == 1 ? link : -1, b2 = kind == 2 ? link : NL;   // geom1 / geom2 bodies
      real pt[3] = {w.c_pos[c][0], w.c_pos[c][1], w.c_pos[c][2]};
      real p1[3], r1[3], p2[3], r2[3];
      point_jac_col<NL>(w, lm, b1, sub, pt, p1, r1);
      point_jac_col<NL>(w, lm, b2, sub, pt, p2, r2);
      real dl[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]}, dr[3] = {r2[0] - r1[0], r2[1] - r1[1], r2[2] - r1[2]};
      cr.jb[c][0] = dot3(w.c_frame[c], dl);
      cr.jb[c][1] = dot3(w.c_frame[c] + 3, dl);
      cr.jb[c][2] = dot3(w.c_frame[c] + 6, dl);
      cr.jb[c][3] = dot3(w.c_frame[c], dr);
    }
  }
  GSYNC();
  // ---- B = M^-1 J^T for the slots with arm dofs: arm lanes need the whole row -> stage through LDS;
  // cube lanes (and every lane of a table-cube slot) just scale by the diagonal
#pragma unroll
  for (int c = 4; c < NC; c++) {
    cr.bb[c - 4][0] = 0; cr.bb[c - 4][1] = 0; cr.bb[c - 4][2] = 0; cr.bb[c - 4][3] = 0;
    __builtin_amdgcn_sched_barrier(0);
    if ((act >> c) & 1u) {
      if (sub < NV) {
#pragma unroll
        for (int k = 0; k < 4; k++) w.stage[k][sub] = cr.jb[c][k];
      }
      GSYNC();
      if (sub < NL) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          real s = 0;
          for (int j = 0; j < NL; j++) s += w.Minv[sub][j] * w.stage[k][j];
          cr.bb[c - 4][k] = s;
        }
      } else if (sub < NV) {
#pragma unroll
        for (int k = 0; k < 4; k++) cr.bb[c - 4][k] = cr.jb[c][k] * invm;
      }
      GSYNC();
    }
  }
  // ---- Gram matrix + edge tables per slot (all lanes get identical sums; lane 0 stores)
  const real qv = sub < NV ? w.qvel[sub] : 0.0;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    __builtin_amdgcn_sched_barrier(0);
    if ((act >> c) & 1u) {
      const int kind = slot_kind<NL>(c);
      real Gm[4][4], vb[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        vb[k] = gsum<G>(cr.jb[c][k] * qv);
#pragma unroll
        for (int l = k; l < 4; l++) {
          const real bl = c < 4 ? cr.jb[c][l] * invm : cr.bb[c < 4 ? 0 : c - 4][l];
          Gm[k][l] = gsum<G>(cr.jb[c][k] * bl); Gm[l][k] = Gm[k][l];
        }
      }
      const bool cube = kind != 2;
      const real* fr = cube ? m->con_cube_friction : m->con_def_friction;
      const real* sr = cube ? m->con_cube_solref : m->con_def_solref;
      const real* si = cube ? m->con_cube_solimp : m->con_def_solimp;
#if KM_VAR_PAR
      const real fr0 = cube ? KM_EP_MU(w, m) : fr[0];
#else
      const real fr0 = fr[0];
#endif
      real mu[3] = {fr0, fr0, fr[1]};
      const real dist = w.c_dist[c];
      real imp = impedance_c(lm.imp[cube ? 1 : 0], dist), kk = lm.kb[cube ? 1 : 0][0], bb = lm.kb[cube ? 1 : 0][1];
      (void)sr; (void)si;
      const int ne = kind == 2 ? 4 : 6;
      real R = 0;
      ConRec& rc = w.rec[c];
#pragma unroll
      for (int e = 0; e < 6; e++) {
        const int k = e / 2 + 1;
        const real sm = (e & 1) ? -mu[k - 1] : mu[k - 1];
        real Ge[4];
#pragma unroll
        for (int l = 0; l < 4; l++) Ge[l] = Gm[l][0] + sm * Gm[l][k];        // J_l . M^-1 (J_0 + sm J_k)^T
        const real Ad = Ge[0] + sm * Ge[k];
        if (e == 0) R = 2 * fr0 * fr0 * fmax(MJ_MINVAL, (1 - imp) * frcp(imp) * KM_EP_SLOT_A(w, lm, kind, w.slot_sph[c]));
        const real vel = vb[0] + sm * vb[k];
        if (sub == 0) {
          rc.den[e] = Ad + R;
          rc.inv[e] = e < ne ? 1.0 / (Ad + R) : 0.0;
          rc.aref[e] = -bb * vel - kk * imp * dist;
          rc.f[e] = 0;
#pragma unroll
          for (int l = 0; l < 4; l++) w.p.Ge[c][e][l] = Ge[l];
        }
      }
      if (sub == 0) { rc.R = R; rc.mu[0] = mu[0]; rc.mu[1] = mu[1]; rc.mu[2] = mu[2]; }
    }
  }
  GSYNC();
}

// one Gauss-Seidel update of a non-negative / box-bounded row (returns delta f); inv = 1 / den
__device__ __forceinline__ real pgs_row(real Ja, real aref, real R, real den, real inv, real f, int type, real floss,
                                        real& improvement) {
  const real res = Ja - aref + R * f;
  real fn = f - res * inv;
  if (type == 0) fn = fmin(fmax(fn, -floss), floss);
  else fn = fmax(fn, 0.0);
  const real dlt = fn - f;
  improvement -= dlt * (res + 0.5 * den * dlt);
  return dlt;
}

#if KM_VAR_FRC
// rhs + qfrc_applied of one dof (the KM_VAR_FRC builds).  The sum is an addition of its own, never contracted into the servo force's
// arithmetic; a zero component leaves rhs as it is, to the sign of a zero (-0 + 0 would be +0), so that a buffer of zeros gives the
// default kernels' bits.
__device__ __forceinline__ real add_applied(real rhs, real f) {
#pragma clang fp contract(off)
  const real s = rhs + f;
  return f == 0.0 ? rhs : s;
}
#endif

// mj_step2 up to (not including) integration: actuation, qacc_smooth, warm start, PGS.  Returns this
// lane's component of qacc (lane `sub` owns dof `sub`).
template <int NL, int G>
__device__ __forceinline__ real solve_accel(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub, int actuation,
                                            CReg<NL>& cr, real invm) {
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC;
  // ---- actuation (position servos on actuator_length = q at mj_step1 time) and smooth acceleration
  if (sub < NV) {
    real rhs = -w.bias[sub];
    if (actuation && sub < NL) {
      real c = fmin(fmax(w.ctrl[sub], lm.ctrlrange[sub][0]), lm.ctrlrange[sub][1]);
      real force = KM_EP_KP(w, lm, sub) * c - KM_EP_KP(w, lm, sub) * w.qpos[sub];
      if (lm.forcelimited[sub]) force = fmin(fmax(force, lm.forcerange[sub][0]), lm.forcerange[sub][1]);
      rhs += force;
    }
#if KM_VAR_FRC
    if (actuation) rhs = add_applied(rhs, w.frc[sub]);      // qfrc_applied: every dof, outside the servo's clamps
#endif
    w.tmp[sub] = rhs;
  }
  GSYNC();
  real a_s = 0;
  if (sub < NL) { for (int j = 0; j < NL; j++) a_s += w.Minv[sub][j] * w.tmp[j]; }
  else if (sub < NV) a_s = w.tmp[sub] * invm;
  if (sub < NV) w.as[sub] = a_s;
  GSYNC();
  const int ns = w.ns;
  const uint32_t act = w.cact;
  const real warm = sub < NV ? w.warm[sub] : 0.0;
  // ---- the cube's friction-loss row owned by this lane (registers only)
  const bool my_row = sub >= NL && sub < NV && KM_EP_FLOSS(w, m) > 0;
  real my_f = 0, my_aref = 0, my_R = 1, my_den = 1, my_inv = 0;
  const real my_fl = KM_EP_FLOSS(w, m);
  if (my_row) {
    real imp = lm.imp0[0], bb = lm.kb[0][1];
    my_R = fmax(MJ_MINVAL, (1 - imp) * frcp(imp) * KM_EP_CUBEW(w, lm, sub < NL + 3 ? 0 : 1));
    my_den = invm + my_R;
    my_inv = 1.0 / my_den;
    my_aref = -bb * w.qvel[sub];
  }
  // ---- warm start: forces implied by qacc_warmstart, kept only if the dual cost is negative
  real cost_rows = 0, y = 0;
  for (int r = sub; r < ns; r += G) {
    const int j = w.s_dof[r];
    const real sg = w.s_sign[r], R = w.s_R[r], aref = w.s_aref[r];
    real jar = sg * w.warm[j] - aref, f;
    if (w.s_type[r] == 0) { const real fl = w.s_floss[r]; f = (jar <= -R * fl) ? fl : ((jar >= R * fl) ? -fl : -jar / R); }
    else f = jar < 0 ? -jar / R : 0.0;
    w.s_f[r] = f;
    cost_rows += 0.5 * R * f * f + f * (sg * w.as[j] - aref);
  }
  if (my_row) {
    real jar = warm - my_aref;
    my_f = (jar <= -my_R * my_fl) ? my_fl : ((jar >= my_R * my_fl) ? -my_fl : -jar / my_R);
    cost_rows += 0.5 * my_R * my_f * my_f + my_f * (a_s - my_aref);
    y += my_f;
  }
#pragma unroll
  for (int c = 0; c < NC; c++) {
    __builtin_amdgcn_sched_barrier(0);
    if ((act >> c) & 1u) {
      real wk[4], ak[4], F[4] = {0, 0, 0, 0};
      {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < 4; k++) { wk[k] = cr.jb[c][k] * warm; ak[k] = cr.jb[c][k] * a_s; }
        gsum_n<G, 4>(wk); gsum_n<G, 4>(ak);
      }
      ConRec& rc = w.rec[c];
      const real R = rc.R;
#pragma unroll
      for (int e = 0; e < 6; e++) {
        const int k = e / 2 + 1;
        const real sm = (e & 1) ? -rc.mu[k - 1] : rc.mu[k - 1];
        const real aref = rc.aref[e];
        real jar = wk[0] + sm * wk[k] - aref;
        real f = (rc.inv[e] != 0 && jar < 0) ? -jar / R : 0.0;
        if (sub == 0) { rc.f[e] = f; cost_rows += 0.5 * R * f * f + f * (ak[0] + sm * ak[k] - aref); }
        F[0] += f; F[k] += sm * f;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) y += cr.jb[c][k] * F[k];
    }
  }
  GSYNC();
  // y = J^T f (lane j), z = M^-1 y
  if (sub < NL) { for (int r = 0; r < ns; r++) if (w.s_dof[r] == sub) y += w.s_sign[r] * w.s_f[r]; }
  if (sub < NV) w.tmp[sub] = y;
  GSYNC();
  real z = 0;
  if (sub < NL) { for (int j = 0; j < NL; j++) z += w.Minv[sub][j] * w.tmp[j]; }
  else if (sub < NV) z = y * invm;
  const real cost = gsum<G>(0.5 * y * z + cost_rows);
  real a = a_s;
  if (cost > 0) {
    for (int r = sub; r < ns; r += G) w.s_f[r] = 0;
    for (int c = sub; c < NC; c += G) for (int e = 0; e < 6; e++) w.rec[c].f[e] = 0;
    my_f = 0;
  } else a += z;
  GSYNC();
  // ---- projected Gauss-Seidel in acceleration space: a = a_s + M^-1 J^T f kept distributed (lane = dof).
  // Row order = mj_makeConstraint order.  The cube's friction-loss rows touch only the diagonal block of
  // M^-1, so the owning lanes update them locally and simultaneously -- identical to one after another,
  // and no cross-lane traffic.  A row on an arm dof needs one broadcast; a contact needs four DPP row
  // reductions (its basis projections u = J a), then its pyramid edges run on precomputed Gram rows.
  const real scale = KM_EP_SCALE(w, lm);
  const int maxit = m->solver_iterations;
  const real tol = m->solver_tolerance;
  for (int iter = 0; iter < maxit; iter++) {
    real improvement = 0, imp_local = 0;
    for (int r = 0; r < ns; r++) {
      const int j = w.s_dof[r];
      const real sg = w.s_sign[r];
      const real f = w.s_f[r];
      const real mij = sub < NL ? w.Minv[sub][j] : 0.0;
      const real Ja = sg * __shfl(a, j, G);
      const real dlt = pgs_row(Ja, w.s_aref[r], w.s_R[r], w.s_den[r], w.s_inv[r], f, w.s_type[r], w.s_floss[r], improvement);
      w.s_f[r] = f + dlt;
      a += sg * mij * dlt;
    }
    if (my_row) {
      const real dlt = pgs_row(a, my_aref, my_R, my_den, my_inv, my_f, 0, my_fl, imp_local);
      my_f += dlt;
      a += dlt * invm;
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
      __builtin_amdgcn_sched_barrier(0);
    if ((act >> c) & 1u) {
        // group-uniform tables come from LDS as broadcast reads (no stores in between: freely scheduled)
        const ConRec& rr = w.rec[c];
        const real Rc = rr.R;
        real u[4], Dk[4] = {0, 0, 0, 0}, f[6];
        {
          // the four basis projections u = J a as INTERLEAVED group sums (round 4; bitwise the same sums as four gsum calls:
          // the products are rounded before the first addition either way)
#pragma clang fp contract(off)
#pragma unroll
          for (int k = 0; k < 4; k++) u[k] = cr.jb[c][k] * a;
          gsum_n<G, 4>(u);
        }
#pragma unroll
        for (int e = 0; e < 6; e++) {
          const int k = e / 2 + 1;
          if (slot_kind<NL>(c) == 2 && e >= 4) { f[e] = 0; continue; }        // condim-3 pair: 4 edges
          const real sm = (e & 1) ? -rr.mu[k - 1] : rr.mu[k - 1];
          const real f0 = rr.f[e];
          const real res = (u[0] + sm * u[k]) + (Rc * f0 - rr.aref[e]);
          const real fn = fmax(f0 - res * rr.inv[e], 0.0);
          const real dlt = fn - f0;
          improvement -= dlt * (res + 0.5 * rr.den[e] * dlt);
          f[e] = fn;
          Dk[0] += dlt; Dk[k] += sm * dlt;
#pragma unroll
          for (int l = 0; l < 4; l++) u[l] += w.p.Ge[c][e][l] * dlt;
        }
        if (sub == 0) {
#pragma unroll
          for (int e = 0; e < 6; e++) w.rec[c].f[e] = f[e];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) a += (c < 4 ? cr.jb[c][k] * invm : cr.bb[c < 4 ? 0 : c - 4][k]) * Dk[k];
      }
    }
    improvement += gsum<G>(imp_local);
    if (improvement * scale < tol) break;
  }
  return a;
}
