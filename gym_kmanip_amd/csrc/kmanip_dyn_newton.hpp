// kmanip_dyn_newton.hpp -- one of the phase headers kmanip_dyn_variant.hpp includes (inside the variant namespace) into each per-variant translation unit: Cholesky row kernels and the Newton solver.
#pragma once
// =============================================================================================
// Newton solver (MuJoCo's default solver, i.e. what the reference actually runs: no <option> element in
// any of its XML files).  Primal problem over qacc:  1/2 (a-a_s)^T M (a-a_s) + sum_i s_i(J_i a - aref_i).
// Lane d owns a_d, grad_d, the search component p_d and column d of the Hessian; the nv x nv Hessian lives
// in LDS (aliasing the dead kinematics) and is factored by a cooperative Cholesky; projections of the
// contact bases are DPP row reductions; the exact line search evaluates phi', phi'' with the rows strided
// over the lanes.  The minimiser is unique, so parity with the oracle does not depend on iteration counts.

// Dof subset of a Newton problem.  Arm and cube meet only in finger-cube contacts (slot kind 1); while none is active the
// primal cost is a SUM of an arm part (dofs 0..NL-1; rows: arm friction loss / limits, finger-table contacts) and a cube part
// (dofs NL..NV-1; rows: cube friction loss, table-cube contacts), i.e. two independent strictly convex minimisations with
// the same joint minimiser -- solved one after the other, each on its own block of the Hessian.  The hard solves of a batch
// are cube-table impacts (tens of active-set changes): they then cost 6 pivots per iteration instead of NV.
enum { KM_SUB_ALL = 0, KM_SUB_ARM = 1, KM_SUB_CUBE = 2 };
template <int NL, int S> struct SubSet {
  static constexpr int D0 = S == KM_SUB_CUBE ? NL : 0, D1 = S == KM_SUB_ARM ? NL : NL + 6;
  static constexpr int kind(int c) { return slot_kind<NL>(c); }
  static constexpr bool slot(int c) { return S == KM_SUB_ALL || (S == KM_SUB_ARM ? kind(c) == 2 : kind(c) == 0); }
  // columns of the Hessian a slot of this kind touches (its Jacobian is zero elsewhere), intersected with the subset
  static constexpr int c0(int c) { const int k = kind(c); const int lo = k == 0 ? NL : 0; return lo > D0 ? lo : D0; }
  static constexpr int c1(int c) { const int k = kind(c); const int hi = k == 2 ? NL : NL + 6; return hi < D1 ? hi : D1; }
};

// Cholesky of an SPD matrix held one ROW PER LANE in registers (h[j] = H[sub][j]), right-looking, in place, on the
// diagonal block [D0, D1): afterwards h[j] = L[sub][j] for D0 <= j <= sub (the j > sub entries are dead) and
// invd = 1 / L[sub][sub].  Lanes outside the block hold zeros and stay inert.
// Column k of L reaches the other rows through DPP row broadcasts: no LDS, no synchronisation.
template <int G, int N, int D0, int D1>
__device__ __forceinline__ void chol_rows(real (&h)[N], real& invd, int sub, int& bad) {
  static_for<D0, D1>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    real dk = gbcast<G, k>(h[k]);
    if (!(dk > 0)) { bad = 1; dk = 1; }
    const real inv = rsqrt_nr(dk);
    const real lik = h[k] * inv;
    h[k] = lik;
    if (sub == k) invd = inv;
    const BSrc<G> lsrc = bsrc<G>(lik);
    fnmac_cols<G, k + 1, D1>(h, lsrc, lik);
    if constexpr (k + 2 >= D1 && k + 1 < D1) dpp_settle(h[k + 1]);     // the next pivot's broadcast reads what the last run just wrote
  });
}
// x = (L L^T)^-1 b, b distributed one component per lane.  Forward substitution is column-oriented (z_k broadcast,
// rows below updated); the transposed solve uses the dot form (lane i contributes L[i][k] x_i, group sum).
template <int G, int N, int D0, int D1>
__device__ __forceinline__ real chol_solve_rows(const real (&h)[N], real invd, int sub, real b) {
  static_for<D0, D1>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const real t = b * invd;                         // lane k's t is z_k
    real upd = b;
    fnmac_b<G, k>(upd, bsrc<G>(t), h[k]);
    b = sub > k ? upd : (sub == k ? t : b);
  });
  real x = 0;
  static_for<D0, D1>([&](auto kc) {
    constexpr int k = D1 - 1 - (decltype(kc)::value - D0);
    const real s = gsum<G>(sub > k ? h[k] * x : 0.0);
    if (sub == k) x = (b - s) * invd;
  });
  return x;
}

// ---- One-row systems (round 3): the same right-looking Cholesky, but column k of L is MASKED to its strictly-lower part as
// it is formed (lik = sub > k ? h[k] * inv : 0), so rows on and above the pivot never change again and hold exact zeros there.
// Both triangular solves are then column-oriented -- one multiply and one broadcast-FMA per pivot, no lane tests, no lane
// reductions -- given row `sub` of L^T next to row `sub` of L.  Row `sub` of L^T is column `sub` of L, which lives in the
// OTHER lanes' registers; it arrives either from the factorisation's own broadcasts (UT: ut[j] += bcast_j(l) * [sub == k],
// (D1-D0)(D1-D0-1)/2 extra broadcast-FMAs: small blocks) or through one LDS transposition (chol_transpose: larger blocks).
// Round 2's transposed solve took one 16-lane reduction per pivot (12-20 instructions each).
// `sl` = this lane's dof index relative to the DPP row's first dof (two-row groups run a block that sits in one row with the
// other row inert: sl < 0 or rows of zeros); `live` = the lane's row holds the block (only those lanes report a bad pivot).
template <int N, int D0, int D1, int BASE, bool UT>
__device__ __forceinline__ void chol_rows1(real (&h)[N], real (&ut)[N], real& invd, int sl, bool live, int& bad) {
  invd = 0;
  if constexpr (UT) {
#pragma unroll
    for (int j = 0; j < N; j++) ut[j] = 0;
  }
  static_for<D0, D1>([&](auto kc) {
    constexpr int k = decltype(kc)::value, kl = k - BASE;
    const real dk = gbcast<16, kl>(h[k]);
    bad |= live && !(dk > 0);
    const real inv = rsqrt_nr(dk);
    const bool me = sl == kl;
    const real lik = sl > kl ? h[k] * inv : 0.0;
    h[k] = lik;
    invd = me ? inv : invd;
    if constexpr (UT) {
      const real isk = me ? 1.0 : 0.0;
      static_for<k + 1, D1>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        dppfma_pn<j - BASE, j == k + 1>(ut[j], lik, isk, h[j], lik, lik);      // ut[j] += L[j][k] [sub == k];  h[j] -= L[j][k] L[sub][k]
      });
    } else {
      static_for<k + 1, D1>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        dppfma1<true, j - BASE, j == k + 1>(h[j], lik, lik);
      });
    }
    if constexpr (k + 2 >= D1 && k + 1 < D1) dpp_settle(h[k + 1]);     // the next pivot's broadcast reads what the last run just wrote
  });
}
// ut[k] = L[k][sub] through LDS: lane i writes row i of L (exact zeros on and above the diagonal), lane s reads column s
template <int N, int D0, int D1, int BASE, class LT>
__device__ __forceinline__ void chol_transpose(LT& lt, const real (&h)[N], real (&ut)[N], int sl) {
  const int r = sl < 0 ? 0 : sl;                        // (lanes of an inert row write zeros over zeros)
#pragma unroll
  for (int k = D0; k < D1; k++) lt[r][k - D0] = h[k];
  GSYNC();
  // lanes outside the block read a column of the block too (finite numbers, never stale LDS): their invd = 0 then gives the
  // zero they need without a select per entry
  const int col = r + BASE - D0 < 0 ? 0 : (r + BASE - D0 > D1 - D0 - 1 ? D1 - D0 - 1 : r + BASE - D0);
#pragma unroll
  for (int k = D0; k < D1; k++) ut[k] = lt[k - BASE][col];
  GSYNC();
}
// x = (L L^T)^-1 b, b distributed one component per lane (zero outside the block)
template <int N, int D0, int D1, int BASE>
__device__ __forceinline__ real chol_solve_rows1(const real (&h)[N], const real (&ut)[N], real invd, real b) {
  static_for<D0, D1>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const real t = b * invd;                            // lane k's t is z_k (its b is final: h[j] = 0 for j >= sub)
    fnmac_bcast16<k - BASE>(b, t, h[k]);
  });
  real z = b * invd;
  static_for<D0, D1>([&](auto kc) {
    constexpr int k = D1 - 1 - (decltype(kc)::value - D0);
    const real t = z * invd;                            // lane k's t is x_k (ut[j] = 0 for j <= sub)
    fnmac_bcast16<k - BASE>(z, t, ut[k]);
  });
  return z * invd;
}

// s_i'(x) and s_i''(x) contributions of one row to the line-search derivatives
__device__ __forceinline__ void row_ls(int type, real x, real y, real R, real Dn, real fl, real& d1, real& d2) {
  if (type == 0) {
    if (x <= -R * fl) d1 += -fl * y;
    else if (x >= R * fl) d1 += fl * y;
    else { d1 += Dn * x * y; d2 += Dn * y * y; }
  } else if (x < 0) { d1 += Dn * x * y; d2 += Dn * y * y; }
}
// cost / force / quadratic-zone flag of one row
__device__ __forceinline__ real row_eval(int type, real x, real R, real Dn, real fl, real& f, int& quad) {
  if (type == 0) {
    if (x <= -R * fl) { f = fl; quad = 0; return fl * (-0.5 * R * fl - x); }
    if (x >= R * fl) { f = -fl; quad = 0; return fl * (-0.5 * R * fl + x); }
    f = -Dn * x; quad = 1; return 0.5 * Dn * x * x;
  }
  if (x < 0) { f = -Dn * x; quad = 1; return 0.5 * Dn * x * x; }
  f = 0; quad = 0; return 0;
}

// The six cube components of a lane-distributed vector, on every lane: linear part and the angular part turned
// into the world frame (the free joint's angular velocity is expressed in the body frame).
template <int NL, int G>
__device__ __forceinline__ void cube_part(const Ws<NL>& w, real x, real* lin, real* angw) {
  lin[0] = gbcast<G, NL>(x); lin[1] = gbcast<G, NL + 1>(x); lin[2] = gbcast<G, NL + 2>(x);
  const real ab[3] = {gbcast<G, NL + 3>(x), gbcast<G, NL + 4>(x), gbcast<G, NL + 5>(x)};
  mat_vec3(angw, w.k.cube_mat, ab);
}
// J_c x for a table-cube contact (slots 0..3: only the cube moves, plane frame): the velocity of the contact point
// read off in the frame -- no cross-lane reduction.  u = (normal, tangent 1, tangent 2, torsion).
template <int NL>
__device__ __forceinline__ void plane_proj(const Ws<NL>& w, int c, const real* lin, const real* angw, real* u) {
  const real r[3] = {w.c_pos[c][0] - w.qpos[NL], w.c_pos[c][1] - w.qpos[NL + 1], w.c_pos[c][2] - w.qpos[NL + 2]};
  real v[3];
  cross3(v, angw, r);
  v[0] += lin[0]; v[1] += lin[1]; v[2] += lin[2];
  u[0] = v[2]; u[1] = v[1]; u[2] = -v[0]; u[3] = angw[2];     // KM_PLANE_FRAME rows
}

// the same for the table-cube slot that lane `sub` owns (lanes 0..3; the others get slot 0's numbers, which they never use):
// ONE evaluation serves all four corner slots
template <int NL>
__device__ __forceinline__ void plane_proj_lane(const Ws<NL>& w, int sub, const real* lin, const real* angw, real* u) {
  plane_proj<NL>(w, sub < 4 ? sub : 0, lin, angw, u);
}

// Constraint assembly for Newton: like build_constraints but no B = M^-1 J^T / Gram tables -- only the
// first-edge diagonal (for MuJoCo's pyramidal regulariser) and the velocity projections (for aref).  The
// single-dof rows (friction loss, joint limits) of dof `sub` are built into this lane's registers: the primal
// cost is a sum over rows, so mj_makeConstraint's row order does not matter here (it does for PGS).
template <int NL, int G>
__device__ __forceinline__ void build_constraints_newton(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub,
                                                         CReg<NL>& cr, real invm) {
  SlotC& sc = cr.sc;
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC, NSPH = Dim<NL>::NSPH;
  cr.fl = 0; cr.Rf = 1; cr.Df = 1; cr.areff = 0; cr.sg = 0; cr.Rl = 1; cr.Dl = 1; cr.arefl = 0;
  const bool armlane = sub < NL, cubelane = sub >= NL && sub < NV;
  const int jl = armlane ? sub : 0, ce = cubelane ? sub - NL : 0;
  // ---- Round 6: EVERYTHING the assembly reads unconditionally is fetched here, at clamped addresses, in one go (km_pin: one wait
  // instead of one per input -- the phase was ~30 LDS round trips in a row with one wave per SIMD); the conditions select afterwards.
  const int si = sub < NL ? sub : NL - 1, sv = sub < NV ? sub : NV - 1, ck = ce >= 3 ? ce - 3 : 0;
  const int cs = sub < NC ? sub : NC - 1;                       // the contact slot this lane owns (slot lanes)
  real dofw = lm.dofw[si], cubew0 = KM_EP_CUBEW(w, lm, 0), cubew1 = KM_EP_CUBEW(w, lm, 1), qvs = w.qvel[sv], kk0 = lm.kb[0][0], bb0 = lm.kb[0][1];
  real floss = lm.floss[si], imp00 = lm.imp0[0], qps = w.qpos[si], rlo = lm.range[si][0], rhi = lm.range[si][1], distc = w.c_dist[cs];
  real ax[3] = {w.k.axis[jl][0], w.k.axis[jl][1], w.k.axis[jl][2]}, xo[3] = {w.k.xpos[jl][0], w.k.xpos[jl][1], w.k.xpos[jl][2]};
  real col0 = w.k.cube_mat[ck], col1 = w.k.cube_mat[3 + ck], col2 = w.k.cube_mat[6 + ck], cpos[3] = {w.qpos[NL], w.qpos[NL + 1], w.qpos[NL + 2]};
  real cm[9], cpc[4][3], cpl[3];                                // cube rotation; the four corner slots' contact points; this lane's corner
#pragma unroll
  for (int k = 0; k < 9; k++) cm[k] = w.k.cube_mat[k];
#pragma unroll
  for (int c = 0; c < 4; c++) { cpc[c][0] = w.c_pos[c][0]; cpc[c][1] = w.c_pos[c][1]; cpc[c][2] = w.c_pos[c][2]; }
  { const int cl = sub < 4 ? sub : 0; cpl[0] = w.c_pos[cl][0]; cpl[1] = w.c_pos[cl][1]; cpl[2] = w.c_pos[cl][2]; }
  int jt = lm.jtype[jl], sps = w.slot_sph[cs];
  uint32_t act = w.cact;
  km_pin(dofw, cubew0, cubew1, qvs, kk0, bb0); km_pin(floss, imp00, qps, rlo, rhi, distc);
  km_pin(ax, xo); km_pin(col0, col1, col2); km_pin(cpos); km_pin(cm); km_pin(cpc[0], cpc[1]); km_pin(cpc[2], cpc[3]); km_pin(cpl);
  km_pin_i(jt, sps); asm volatile("" : "+v"(act));
  if (sub < NV) {
    const real Ad = sub < NL ? dofw : (sub < NL + 3 ? cubew0 : cubew1);           // efc_diagApprox (qpos0 constants)
    const real qv = qvs;
    const real kk = kk0, bb = bb0;
    const real fl = sub < NL ? floss : KM_EP_FLOSS(w, m);
    if (fl > 0) {
      const real imp = imp00;
      cr.fl = fl; cr.Rf = fmax(MJ_MINVAL, (1 - imp) * frcp(imp) * Ad); cr.Df = frcp(cr.Rf); cr.areff = -bb * qv;
    }
    if (sub < NL) {
      const real dl = qps - rlo, du = rhi - qps;
      const real pos = dl < 0 ? dl : du;
      if (pos < 0) {                                       // (lower and upper cannot both be violated: range lo < hi)
        const real imp = impedance_c(lm.imp[0], pos);
        cr.sg = dl < 0 ? 1.0 : -1.0;
        cr.Rl = fmax(MJ_MINVAL, (1 - imp) * frcp(imp) * Ad);
        cr.Dl = frcp(cr.Rl);
        cr.arefl = -bb * (cr.sg * qv) - kk * imp * pos;
      }
    }
  }
  // ---- this lane's column of every active contact's Jacobian basis.  What a dof does to a point depends on the dof only
  // through a direction A and, for rotations, a point O on the axis (an arm hinge: joint axis and origin; an arm slider: its
  // axis; the cube: a world axis, or a body axis through the cube centre) -- fetched ONCE, unconditionally, above;
  // per slot the column is then a cross product and selects, no branches and no loads under conditions (sphere slots, which are
  // rarely active, fetch their contact point, frame and ancestor mask together inside their branch).
  const bool rot = armlane ? jt != KM_JNT_SLIDE : ce >= 3;
  real A[3], O[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const real cold = d == 0 ? col0 : (d == 1 ? col1 : col2);
    A[d] = armlane ? ax[d] : (ce >= 3 ? cold : (ce == d ? 1.0 : 0.0));
    O[d] = armlane ? xo[d] : cpos[d];
  }
#pragma unroll
  for (int c = 0; c < NC; c++) {
    cr.jb[c][0] = 0; cr.jb[c][1] = 0; cr.jb[c][2] = 0; cr.jb[c][3] = 0;
    if ((act >> c) & 1u) {                                 // (group-uniform)
      const int kind = slot_kind<NL>(c);
      // geom1 / geom2: kind 0 table (world) / cube, kind 1 sphere's link / cube, kind 2 table (world) / sphere's link.  A lane
      // belongs to at most one of the two bodies; its column is +J for geom2's body, -J for geom1's.
      real sgn = 0, cp[3], fr[9];
      if (kind == 0) {
        sgn = cubelane ? 1.0 : 0.0;
        cp[0] = cpc[c < 4 ? c : 0][0]; cp[1] = cpc[c < 4 ? c : 0][1]; cp[2] = cpc[c < 4 ? c : 0][2];
      } else {
        cp[0] = w.c_pos[c][0]; cp[1] = w.c_pos[c][1]; cp[2] = w.c_pos[c][2];
#pragma unroll
        for (int k = 0; k < 9; k++) fr[k] = w.c_frame[c][k];
        uint32_t am = w.slot_anc[c];
        km_pin(cp, fr); asm volatile("" : "+v"(am));
        const bool mine = armlane && ((am >> jl) & 1u);
        sgn = kind == 1 ? (mine ? -1.0 : (cubelane ? 1.0 : 0.0)) : (mine ? 1.0 : 0.0);
      }
      const real r[3] = {cp[0] - O[0], cp[1] - O[1], cp[2] - O[2]};
      real jp[3];
      cross3(jp, A, r);
#pragma unroll
      for (int d = 0; d < 3; d++) jp[d] = sgn * (rot ? jp[d] : A[d]);
      const real jr[3] = {rot ? sgn * A[0] : 0.0, rot ? sgn * A[1] : 0.0, rot ? sgn * A[2] : 0.0};
      if (kind == 0) {                                     // constant plane frame: rows n = +z, t1 = +y, t2 = -x
        cr.jb[c][0] = jp[2]; cr.jb[c][1] = jp[1]; cr.jb[c][2] = -jp[0]; cr.jb[c][3] = jr[2];
      } else {
        cr.jb[c][0] = dot3(fr, jp);
        cr.jb[c][1] = dot3(fr + 3, jp);
        cr.jb[c][2] = dot3(fr + 6, jp);
        cr.jb[c][3] = dot3(fr, jr);
      }
    }
  }
  // the slot lanes' solver constants: fetched now, while the projections below run (slot `sub` of a slot lane; clamped elsewhere)
  const int kindl = cs < 4 ? 0 : (cs < 4 + Dim<NL>::NSS ? 1 : 2), pset = kindl != 2 ? 1 : 0;
  const int spc = sps < 0 ? 0 : (sps >= NSPH ? NSPH - 1 : sps);            // (an inactive slot's sphere index is stale: clamped, never used)
  real sA = KM_EP_SLOT_A(w, lm, kindl, spc);                               // efc_diagApprox of the first pyramid edge (qpos0 constant; no M^-1 product)
  real mu_t = KM_EP_FRIC_T(w, lm, pset), mu_r = lm.fric[pset][1], kks = lm.kb[pset][0], bbs = lm.kb[pset][1];
  real i_d0 = lm.imp[pset].d0, i_dw = lm.imp[pset].dw, i_iw = lm.imp[pset].iw, i_mid = lm.imp[pset].mid, i_imid = lm.imp[pset].imid, i_i1 = lm.imp[pset].i1mid;
  int i_mode = lm.imp[pset].mode;
  const real qv = sub < NV ? qvs : 0.0;
  // the six cube components of qvel on every lane, the angular part in the world frame (cube_part with the rotation fetched above)
  real qlin[3], qangw[3];
  {
    qlin[0] = gbcast<G, NL>(qv); qlin[1] = gbcast<G, NL + 1>(qv); qlin[2] = gbcast<G, NL + 2>(qv);
    const real ab[3] = {gbcast<G, NL + 3>(qv), gbcast<G, NL + 4>(qv), gbcast<G, NL + 5>(qv)};
    mat_vec3(qangw, cm, ab);
  }
  // velocity projections of every active slot; lane c keeps slot c's
  real vb[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 9; k++) cr.cm[k] = cm[k];
  cr.pr[0] = cpl[0] - cpos[0]; cr.pr[1] = cpl[1] - cpos[1]; cr.pr[2] = cpl[2] - cpos[2];
  {                                                             // table-cube slots: lane c < 4 evaluates ITS corner (plane_proj)
    const real r[3] = {cr.pr[0], cr.pr[1], cr.pr[2]};
    real v[3];
    cross3(v, qangw, r);
    v[0] += qlin[0]; v[1] += qlin[1]; v[2] += qlin[2];
    vb[0] = v[2]; vb[1] = v[1]; vb[2] = -v[0]; vb[3] = qangw[2];     // KM_PLANE_FRAME rows
  }
  static_for<4, NC>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    if ((act >> c) & 1u) {
      constexpr int NK = slot_kind<NL>(c) == 2 ? 3 : 4;
      real pj[NK];
#pragma unroll
      for (int k = 0; k < NK; k++) pj[k] = cr.jb[c][k] * qv;
      gsum_n<G, NK>(pj);
#pragma unroll
      for (int k = 0; k < NK; k++) vb[k] = sub == c ? pj[k] : vb[k];
      if (slot_kind<NL>(c) == 2) vb[3] = sub == c ? 0.0 : vb[3];
    }
  });
  // the solver constants of slot `sub`, one slot per lane (all slots through ONE pass of the impedance / regulariser / reference
  // acceleration arithmetic instead of one unrolled copy per slot)
  km_pin(sA, mu_t, mu_r, kks, bbs, i_d0); km_pin(i_dw, i_iw, i_mid, i_imid, i_i1); km_pin_i(i_mode);
  sc.D = 0; sc.D3 = 0; sc.mu = 0; sc.mu3 = 0; sc.A[0] = 0; sc.A[1] = 0; sc.A[2] = 0; sc.A[3] = 0;
  if (sub < NC && ((act >> sub) & 1u)) {
    const int kind = kindl;
    const real Ad = sA;
    const real dist = distc;
    const real imp = impedance_v(i_d0, i_dw, i_iw, i_mid, i_imid, i_i1, i_mode, dist), kk = kks, bb = bbs;
    const real R = 2 * mu_t * mu_t * fmax(MJ_MINVAL, (1 - imp) * frcp(imp) * Ad), Dn = frcp(R);
    sc.D = Dn; sc.D3 = kind == 2 ? 0.0 : Dn; sc.mu = mu_t; sc.mu3 = mu_r;
    sc.A[0] = -bb * vb[0] - kk * imp * dist; sc.A[1] = -bb * vb[1]; sc.A[2] = -bb * vb[2]; sc.A[3] = -bb * vb[3];
  }
  GSYNC();
}

// M x for a vector distributed one component per lane: arm block from the lane's register row of M
// (components arrive by DPP row broadcast), cube block diagonal
template <int NL, int G>
__device__ __forceinline__ real mass_mul(const CReg<NL>& cr, int sub, real mdiag, real x) {
  real s = 0;
  const BSrc<G> xs = bsrc<G>(x);
  fmac_rowvec<G, 0, NL>(s, xs, [&](int j) { return cr.mrow[j]; });
  return sub < NL ? s : mdiag * x;
}

// =============================================================================================
// Slot-lane Newton (round 3; one- and two-row groups).  Lane c < NC of the group's FIRST DPP row owns contact slot c; what the
// other lanes need from it arrives as a row broadcast inside an FMA (two-row groups: of the copy v_permlane16_swap makes of the
// first row's registers, ONE swap pair per broadcast value whatever the number of slots).  Same mathematics and iterates as
// round 2's edge-distributed layout; the oracle mirrors neither, only the algorithm.

// All six pyramid edges of the slot this lane owns at the shifted projections X (x_e = X_0 +- mu_k X_k): the slot's cost, the
// force it applies along its four basis rows (F = sum_e f_e (1, +-mu_k)), and the Hessian weights of its active edges
// W = sum_{x_e < 0} D_e (1, +-mu_k)(1, +-mu_k)^T, stored (W00, W01, W02, W03, W11, W22, W33).  Branch-free; an inactive slot
// (D = D3 = 0) yields zeros.
// a register of the group's first DPP row as seen from both rows (one-row groups: itself)
template <int G> __device__ __forceinline__ real row0(real x) {
  if constexpr (G == 32) return bsrc<32>(x).e; else return x;
}

template <bool WEIGHTS>
__device__ __forceinline__ real slot_eval(const SlotC& sc, const real (&X)[4], real (&F)[4], real (&W)[7]) {
  const real t1 = sc.mu * X[1], t2 = sc.mu * X[2], t3 = sc.mu3 * X[3];
  const real x1p = X[0] + t1, x1m = X[0] - t1, x2p = X[0] + t2, x2m = X[0] - t2, x3p = X[0] + t3, x3m = X[0] - t3;
  const real m1p = fmin(x1p, 0.0), m1m = fmin(x1m, 0.0), m2p = fmin(x2p, 0.0), m2m = fmin(x2m, 0.0), m3p = fmin(x3p, 0.0), m3m = fmin(x3m, 0.0);
  const real s12 = (m1p + m1m) + (m2p + m2m), s3 = m3p + m3m;
  F[0] = -(sc.D * s12 + sc.D3 * s3);                         // f_e = -D x_e on the active edges
  F[1] = -(sc.mu * sc.D) * (m1p - m1m); F[2] = -(sc.mu * sc.D) * (m2p - m2m); F[3] = -(sc.mu3 * sc.D3) * (m3p - m3m);
  if constexpr (WEIGHTS) {
    const real d1p = x1p < 0 ? sc.D : 0.0, d1m = x1m < 0 ? sc.D : 0.0, d2p = x2p < 0 ? sc.D : 0.0, d2m = x2m < 0 ? sc.D : 0.0;
    const real d3p = x3p < 0 ? sc.D3 : 0.0, d3m = x3m < 0 ? sc.D3 : 0.0;
    W[0] = ((d1p + d1m) + (d2p + d2m)) + (d3p + d3m);
    W[1] = sc.mu * (d1p - d1m); W[2] = sc.mu * (d2p - d2m); W[3] = sc.mu3 * (d3p - d3m);
    W[4] = (sc.mu * sc.mu) * (d1p + d1m); W[5] = (sc.mu * sc.mu) * (d2p + d2m); W[6] = (sc.mu3 * sc.mu3) * (d3p + d3m);
  }
  return 0.5 * (sc.D * ((m1p * m1p + m1m * m1m) + (m2p * m2p + m2m * m2m)) + sc.D3 * (m3p * m3p + m3m * m3m));
}
// which of the slot's six edges are active at the shifted projections X (the comparisons slot_eval's weights W come from)
__device__ __forceinline__ int slot_edge_mask(const SlotC& sc, const real (&X)[4]) {
  const real t1 = sc.mu * X[1], t2 = sc.mu * X[2], t3 = sc.mu3 * X[3];
  return (int)(X[0] + t1 < 0) | (int)(X[0] - t1 < 0) << 1 | (int)(X[0] + t2 < 0) << 2 | (int)(X[0] - t2 < 0) << 3
         | (int)(X[0] + t3 < 0) << 4 | (int)(X[0] - t3 < 0) << 5;
}
// this slot's contribution to phi'(alpha) and phi''(alpha) along y (X already holds u + alpha y)
__device__ __forceinline__ void slot_ls(const SlotC& sc, const real (&X)[4], const real (&y)[4], real& e1, real& e2) {
  const real t1 = sc.mu * X[1], t2 = sc.mu * X[2], t3 = sc.mu3 * X[3], s1 = sc.mu * y[1], s2 = sc.mu * y[2], s3 = sc.mu3 * y[3];
  const real x1p = X[0] + t1, x1m = X[0] - t1, x2p = X[0] + t2, x2m = X[0] - t2, x3p = X[0] + t3, x3m = X[0] - t3;
  const real y1p = y[0] + s1, y1m = y[0] - s1, y2p = y[0] + s2, y2m = y[0] - s2, y3p = y[0] + s3, y3m = y[0] - s3;
  const real a = (fmin(x1p, 0.0) * y1p + fmin(x1m, 0.0) * y1m) + (fmin(x2p, 0.0) * y2p + fmin(x2m, 0.0) * y2m);
  const real a3 = fmin(x3p, 0.0) * y3p + fmin(x3m, 0.0) * y3m;
  e1 += sc.D * a + sc.D3 * a3;
  const real b = ((x1p < 0 ? y1p * y1p : 0.0) + (x1m < 0 ? y1m * y1m : 0.0)) + ((x2p < 0 ? y2p * y2p : 0.0) + (x2m < 0 ? y2m * y2m : 0.0));
  const real b3 = (x3p < 0 ? y3p * y3p : 0.0) + (x3m < 0 ? y3m * y3m : 0.0);
  e2 += sc.D * b + sc.D3 * b3;
}

// J_c v of every active slot of the subset, delivered to the lane that owns the slot (u of the other lanes / slots: finite
// numbers that meet D = 0).  Table-cube slots: lane c < 4 reads the contact point's velocity off the cube twist (one
// evaluation for all four); sphere slots: a group sum per basis row, kept by lane c.
template <int NL, int G, int S>
__device__ __forceinline__ void slot_project(const Ws<NL>& w, const CReg<NL>& cr, uint32_t act, int sub, real v, real (&u)[4]) {
  constexpr int NC = Dim<NL>::NC;
  using SS = SubSet<NL, S>;
  u[0] = 0; u[1] = 0; u[2] = 0; u[3] = 0;
  if constexpr (S != KM_SUB_ARM) {
    // cube_part + plane_proj_lane on the registers the constraint assembly left in cr (same operations, same values)
    const real lin[3] = {gbcast<G, NL>(v), gbcast<G, NL + 1>(v), gbcast<G, NL + 2>(v)};
    const real ab[3] = {gbcast<G, NL + 3>(v), gbcast<G, NL + 4>(v), gbcast<G, NL + 5>(v)};
    real angw[3], vv[3];
    mat_vec3(angw, cr.cm, ab);
    cross3(vv, angw, cr.pr);
    vv[0] += lin[0]; vv[1] += lin[1]; vv[2] += lin[2];
    u[0] = vv[2]; u[1] = vv[1]; u[2] = -vv[0]; u[3] = angw[2];     // KM_PLANE_FRAME rows
  }
  static_for<4, NC>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    if constexpr (SS::slot(c)) {
      if ((act >> c) & 1u) {
        constexpr int NK = slot_kind<NL>(c) == 2 ? 3 : 4;
        real pj[NK];
#pragma unroll
        for (int k = 0; k < NK; k++) pj[k] = cr.jb[c][k] * v;
        gsum_n<G, NK>(pj);
#pragma unroll
        for (int k = 0; k < NK; k++) u[k] = sub == c ? pj[k] : u[k];
        if (slot_kind<NL>(c) == 2) u[3] = sub == c ? 0.0 : u[3];
      }
    }
  });
}
// grad -= J^T F over the subset's active slots: the four force components of slot c arrive from lane c inside the FMAs
template <int NL, int G, int S>
__device__ __forceinline__ void slot_grad(const CReg<NL>& cr, uint32_t act, const real (&F)[4], real& grad) {
  constexpr int NC = Dim<NL>::NC;
  static_assert(NC <= 16, "the slot lanes sit in the group's first DPP row");
  using SS = SubSet<NL, S>;
  const real F0 = row0<G>(F[0]), F1 = row0<G>(F[1]), F2 = row0<G>(F[2]), F3 = row0<G>(F[3]);
  static_for<0, NC>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    if constexpr (SS::slot(c)) {
      if ((act >> c) & 1u) {
        real g2 = 0;
        if constexpr (slot_kind<NL>(c) == 2) dppfma_acc3<c>(g2, F0, cr.jb[c][0], F1, cr.jb[c][1], F2, cr.jb[c][2]);
        else dppfma_acc4<c>(g2, F0, cr.jb[c][0], F1, cr.jb[c][1], F2, cr.jb[c][2], F3, cr.jb[c][3]);
        grad -= g2;
      }
    }
  });
}
// does lane `sub` own a slot of the subset?
template <int NL, int S> __device__ __forceinline__ bool slot_lane_in(int sub) {
  constexpr int NC = Dim<NL>::NC, NSS = Dim<NL>::NSS;
  return S == KM_SUB_ALL ? sub < NC : (S == KM_SUB_ARM ? (sub >= 4 + NSS && sub < NC) : sub < 4);
}

// Newton state at a start point (all slots, both cost parts): u = J a - A on the slot lanes, gradient, the lanes' own rows,
// the slots' Hessian weights.  cs != nullptr: also this lane's share of the cost at a_s (MuJoCo's warm-start comparison).
template <int NL, int G, bool CS>
__device__ __forceinline__ void newton_eval_sl(const Ws<NL>& w, int sub, const CReg<NL>& cr, real a, real a_s, real Mr, real& grad, int& qf,
                                               int& ql, real (&u)[4], real (&W)[7], real& c0, real& c1, real& cs) {
  constexpr int NV = Dim<NL>::NV;
  const uint32_t act = w.cact;
  const SlotC& sc = cr.sc;
  slot_project<NL, G, KM_SUB_ALL>(w, cr, act, sub, a, u);
#pragma unroll
  for (int k = 0; k < 4; k++) u[k] -= sc.A[k];
  real F[4];
  const real cslot = slot_eval<true>(sc, u, F, W);
  real csl = 0;
  if constexpr (CS) {
    real us[4], Fs[4], Ws_[7];
    slot_project<NL, G, KM_SUB_ALL>(w, cr, act, sub, a_s, us);
#pragma unroll
    for (int k = 0; k < 4; k++) us[k] -= sc.A[k];
    csl = slot_eval<false>(sc, us, Fs, Ws_);
  }
  grad = Mr;
  qf = 0; ql = 0;
  {
    real co = 0.5 * (a - a_s) * Mr;
    if (cr.fl > 0) { real f; co += row_eval(0, a - cr.areff, cr.Rf, cr.Df, cr.fl, f, qf); grad -= f; }
    if (cr.sg != 0) { real f; co += row_eval(1, cr.sg * a - cr.arefl, cr.Rl, cr.Dl, 0.0, f, ql); grad -= cr.sg * f; }
    // (selects, not `if (..) c0 = ..; else c1 = ..`: the latter made the compiler index {c0, c1} in scratch memory)
    c0 = sub < NL ? co : 0.0; c1 = (sub >= NL && sub < NV) ? co : 0.0;
    if constexpr (CS) {                         // (the Gauss term vanishes at a_s)
      real f; int qd;
      if (cr.fl > 0) csl += row_eval(0, a_s - cr.areff, cr.Rf, cr.Df, cr.fl, f, qd);
      if (cr.sg != 0) csl += row_eval(1, cr.sg * a_s - cr.arefl, cr.Rl, cr.Dl, 0.0, f, qd);
    }
  }
  c1 += sub < 4 ? cslot : 0.0; c0 += sub < 4 ? 0.0 : cslot;   // table-cube slots belong to the cube part (lanes without a slot: cslot = 0)
  slot_grad<NL, G, KM_SUB_ALL>(cr, act, F, grad);
  cs = csl;
}

// Hessian row `sub` (block [D0, D1) of the subset) from the slots' weights: H += J_c^T W_c J_c, the weights of slot c arriving
// from lane c inside the FMAs that build t = W_c J_c[:, sub]
// CUBECOLS: only the cube's columns NL..NV-1 of every row (the partial refactorisation of newton_loop_sl; the entries are built by
// the same operations in the same order as in the full build, so they come out bitwise the same)
template <int NL, int G, int S, bool CUBECOLS = false>
__device__ __forceinline__ void newton_hessian_sl(const Ws<NL>& w, int sub, const CReg<NL>& cr, real mdiag, int qf, int ql,
                                                  const real (&W)[7], real (&h)[Dim<NL>::NV], bool in, uint32_t act, bool joint) {
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC, J0 = CUBECOLS ? NL : 0;
  using SS = SubSet<NL, S>;
  {
    real dg = sub < NL ? 0.0 : mdiag;
    if (qf) dg += cr.Df;
    if (ql) dg += cr.Dl;
    // dofs outside the problem: zero rows -- or, in the joint loop (whose pivots run over them too), identity rows
    const real idg = joint ? 1.0 : 0.0;
#pragma unroll
    for (int j = J0; j < NV; j++) h[j] = in ? (j < NL ? cr.mrow[j] : 0.0) + ((j == sub) ? dg : 0.0) : ((j == sub) ? idg : 0.0);
  }
  real Wb[7];
#pragma unroll
  for (int i = 0; i < 7; i++) Wb[i] = row0<G>(W[i]);
  static_for<0, NC>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    if constexpr (SS::slot(c)) {
      if ((act >> c) & 1u) {
        const real j0 = cr.jb[c][0], j1 = cr.jb[c][1], j2 = cr.jb[c][2], j3 = cr.jb[c][3];
        real t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        if constexpr (SS::kind(c) != 2) {
          dppfma_acc4<c>(t0, Wb[0], j0, Wb[1], j1, Wb[2], j2, Wb[3], j3);
          dppfma3<false, c, c, c>(t1, Wb[1], j0, t2, Wb[2], j0, t3, Wb[3], j0);
          dppfma3<false, c, c, c, false>(t1, Wb[4], j1, t2, Wb[5], j2, t3, Wb[6], j3);
        } else {                                                                // (condim-3 pairs have no torsion row)
          dppfma_acc3<c>(t0, Wb[0], j0, Wb[1], j1, Wb[2], j2);
          dppfma2<false, c, c>(t1, Wb[1], j0, t2, Wb[2], j0);
          dppfma2<false, c, c, false>(t1, Wb[4], j1, t2, Wb[5], j2);
        }
        // H[sub][j] += sum_k t_k(sub) * J_k[j]: lane j's basis entries arrive by row broadcast (only the columns the slot's
        // Jacobian can be nonzero in); DPP sources = the Jacobian columns (or their row copies), written long before: the
        // first run of a two-row group still waits for the swap that made the copies
        const BSrc<G> j0s = bsrc<G>(j0), j1s = bsrc<G>(j1), j2s = bsrc<G>(j2), j3s = bsrc<G>(j3);
        static_for<(SS::c0(c) > J0 ? SS::c0(c) : J0), SS::c1(c)>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          constexpr bool WT = G == 32 && j == SS::c0(c);
          if constexpr (SS::kind(c) != 2) dppfma_acc4<j & 15, WT>(h[j], bsel<G, j>(j0s), t0, bsel<G, j>(j1s), t1, bsel<G, j>(j2s), t2, bsel<G, j>(j3s), t3);
          else dppfma_acc3<j & 15, WT>(h[j], bsel<G, j>(j0s), t0, bsel<G, j>(j1s), t1, bsel<G, j>(j2s), t2);
        });
      }
    }
  });
}

// Newton iterations on one dof subset, from the point (a, Mr, grad, qf, ql, u, W) with cost `cost` (all of the subset).
// JOINT (S = KM_SUB_ALL only): the wave holds at least one coupled env.  Its uncoupled wave-mates would otherwise run their arm
// loops BEFORE and their cube loops AFTER the coupled env's 16-dof loop (different code paths: SIMD divergence serialises them --
// 0.1-0.2 M and 0.13-0.34 M clocks on top of the slowest waves of a launch); here every group runs ITS problems inside one
// instruction stream: the coupled env its whole problem, an uncoupled env (`two`) first its arm problem (cost `cost`), then its
// cube problem (`cost_b`), each as a 16-dof problem whose other dofs are inert (identity rows, zero gradient, no slots), with its
// own iteration counts; the arm problem's Woodbury direction is the one part that stays a branch of its own.  The inert pivots and
// the zero entries they meet change nothing in a block's arithmetic: an env's result does not depend on what its wave-mates
// are (tests compare shards and launch shapes bit for bit).
template <int NL, int G, int S, bool JOINT = false>
__device__ __forceinline__ void newton_loop_sl(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub, const CReg<NL>& cr,
                                               real mdiag, real a_s, real& a, real& Mr, real cost, real& grad, int& qf, int& ql,
                                               real (&u)[4], real (&W)[7], Prof& pf, bool two = false, real cost_b = 0, int iter0 = 0,
                                               int* resume = nullptr, real* rcost = nullptr, int* riter = nullptr) {
  static_assert(!JOINT || (S == KM_SUB_ALL && G == 16), "the joint loop is the whole-problem loop of the one-row groups");
  constexpr int NV = Dim<NL>::NV, NC = Dim<NL>::NC, NSS = Dim<NL>::NSS;
  using SS = SubSet<NL, S>;
  const SlotC& sc = cr.sc;
  // the problem this group is on (JOINT: run-time and per group), its slots, its dofs, the slot lanes that belong to it (their
  // cost counts, their u moves)
  int prob = (JOINT && two) ? (int)KM_SUB_ARM : S;
  uint32_t act = w.cact;
  bool in = sub >= SS::D0 && sub < SS::D1, slin = slot_lane_in<NL, S>(sub);
  // Partial refactorisation (round 4; one-row groups, whole-problem / joint loop).  Most iterations of a coupled env only move
  // edges of the cube's table contacts (the stiff ones): rows and columns of the ARM dofs -- the first NL pivots -- are then
  // exactly what the previous iteration factorised.  When no group of the wave has changed anything on its arm side (single-
  // dof rows of arm dofs, edge sets of the sphere slots) since the factor that sits in LDS (w.LT) was made, the iteration keeps
  // L's first NL columns, REPLAYS their updates on the cube block (the same FMAs on the same numbers in the same order as the
  // full factorisation, minus the pivots' reciprocal-square-root chains) and factorises only the cube's 6 x 6 Schur complement:
  // bitwise the result of the full path, so an env's bits still do not depend on its wave-mates -- whose state decides which
  // path the wave takes.  `sig0` = the arm-side signature of the cached factor, `invd_keep` its 1 / L_ii.
  int sig0 = 0;
  bool cache_ok = false;
  real invd_keep = 0;
  auto enter = [&](int pr) {
    constexpr uint32_t ARM_SLOTS = ((1u << NC) - 1u) & ~((1u << (4 + NSS)) - 1u);
    cache_ok = false;
    if constexpr (JOINT) {
      if (pr == KM_SUB_CUBE) {
        // a wave-mate's cube problem has identity rows on the arm dofs: the arm columns of ITS factor are known without a
        // factorisation (strictly-lower entries 0, 1 / L_ii = 1 -- and whatever 1 / L_ii a full pass would compute there only ever
        // multiplies the zero arm components of its right-hand side), so its first iteration need not force the wave onto the full path
#pragma unroll
        for (int k = 0; k < NL; k++) w.LT[sub][k] = 0;
        invd_keep = sub < NL ? 1.0 : 0.0; sig0 = 0; cache_ok = true;
      }
    }
    prob = pr;
    act = pr == KM_SUB_ARM ? (w.cact & ARM_SLOTS) : (w.cact & 0xFu);
    in = pr == KM_SUB_ARM ? sub < NL : (sub >= NL && sub < NV);
    slin = pr == KM_SUB_ARM ? (sub >= 4 + NSS && sub < NC) : sub < 4;
  };
  if (JOINT && two) enter(KM_SUB_ARM);
  const real scale = KM_EP_SCALE(w, lm);
  const real tol = m->solver_tolerance;
  const int maxit = m->solver_iterations;
  pf.ph(40);       // (what a group waited for wave-mates that ran a loop it does not -- SIMD divergence -- lands here)
  auto small = [&]() { const real g0 = in ? grad : 0.0; return km_sqrt(gsum<G>(g0 * g0)) * scale < tol; };
  if (small()) {
    if (!(JOINT && prob == KM_SUB_ARM)) return;
    enter(KM_SUB_CUBE); cost = cost_b;
    if (small()) return;
  }
  for (int iter = iter0; ; iter++) {
    if constexpr (JOINT) {
      // Round 5: the joint loop runs only while a COUPLED env of the wave is still iterating.  Its uncoupled mates ride along for
      // free until then; what is left of their problems afterwards (measured: a mate's arm + cube iterations in sequence outlast the
      // coupled env's by about one iteration per sub-step, at the whole-problem iteration's price) they finish in their own arm / cube
      // loops -- a third of the cost per iteration, and bit for bit the same iterates: an uncoupled env's arithmetic in here IS that
      // of its own loops (which is what keeps an env's bits independent of its wave-mates), so where an iteration runs changes nothing.
      // The hand-over carries the problem the group is on, its cost so far and its iteration count.
      if (!__any(!two)) { *resume = prob; *rcost = cost; *riter = iter; return; }
    }
#ifdef KM_PROFILE
    const bool lone_it = JOINT && __popcll(__ballot(1)) <= 16;       // this group iterates alone: its wave-mates have left the loop
    if constexpr (JOINT) pf.it_begin();
#endif
    real p = 0;
    // The arm problem's quadratic rows are usually just single-dof rows (the two slider friction-loss rows; now and then a
    // joint at its limit) -- no sphere on the table.  Its Hessian is then M + diag(delta) with at most two nonzero deltas, and
    // this sub-step already holds M^-1: by the Woodbury identity  p = -(y - M^-1[:,S] z),  y = M^-1 grad,
    // (diag(1/delta_S) + M^-1[S,S]) z = y_S  -- one row-times-vector product and a 2 x 2 solve instead of a 10-pivot
    // factorisation and two triangular solves.
    bool plain = false;
    uint32_t rows = 0;
    if (S == KM_SUB_ARM || (JOINT && prob == KM_SUB_ARM)) {
      const unsigned long long bq = __ballot(slin && W[0] != 0);              // a sphere-table slot with edges in their quadratic zone
      const unsigned long long bal = __ballot(in && (qf | ql));
      const int sh = (threadIdx.x & 63) - sub;
      constexpr uint32_t GM = G == 32 ? 0xFFFFFFFFu : 0xFFFFu;
      const bool cq = ((uint32_t)(bq >> sh) & GM) != 0;
      rows = (uint32_t)(bal >> sh) & GM;
      if constexpr (G == 32) {
        // two-arm models: M^-1 is block diagonal, so the identity holds per block -- up to two quadratic rows in EACH block,
        // every lane correcting with the rows of its own block
        const uint32_t lowm = lm.split ? (1u << lm.split) - 1u : 0xFFFFFFFFu;
        plain = !cq && __popc(rows & lowm) <= 2 && __popc(rows & ~lowm) <= 2;
        rows &= (sub < lm.split || !lm.split) ? lowm : ~lowm;
      } else plain = !cq && __popc(rows) <= 2;
    }
    if constexpr (KM_WORK_COUNTERS(NL)) {
      if (sub == 0) w.work += plain ? KM_WORK_PLAIN : (prob == KM_SUB_ALL ? KM_WORK_ALL : (prob == KM_SUB_ARM ? KM_WORK_ARM : KM_WORK_CUBE));
    }
    if (plain) {
      // everything the direction reads from LDS or from other lanes that does not depend on y is requested FIRST and together --
      // the row of M^-1, the 2 x 2 system's entries, the correction's two column entries, the two rows' weights -- so that the
      // path waits for one LDS round trip here and one more for y's two entries, not for eleven in a row
      const BSrc<G> gs = bsrc<G>(in ? grad : 0.0);
      const int row = sub < NL ? sub : 0;
      real mi[NL];
#pragma unroll
      for (int j = 0; j < NL; j++) mi[j] = w.Minv[row][j];
      const int i1 = rows ? __ffs(rows) - 1 : 0, i2 = (rows & (rows - 1)) ? __ffs(rows & (rows - 1)) - 1 : i1;
      const real m11 = w.Minv[i1][i1], m22 = w.Minv[i2][i2], a12 = w.Minv[i1][i2], r1 = w.Minv[row][i1], r2 = w.Minv[row][i2];
      const real dl = (qf ? cr.Df : 0.0) + (ql ? cr.Dl : 0.0);
      const real d1 = __shfl(dl, i1, G), d2 = __shfl(dl, i2, G);
      real y = 0;
      fmac_rowvec<G, 0, NL>(y, gs, [&](int j) { return mi[j]; });
      real corr = 0;
      if (rows) {
        const real y1 = __shfl(y, i1, G), y2 = __shfl(y, i2, G);
        const real a11 = frcp(d1) + m11;
        real z1, z2 = 0;
        if (i2 == i1) z1 = y1 * frcp(a11);
        else {
          const real a22 = frcp(d2) + m22;
          const real idet = frcp(a11 * a22 - a12 * a12);
          z1 = (a22 * y1 - a12 * y2) * idet;
          z2 = (a11 * y2 - a12 * y1) * idet;
        }
        corr = r1 * z1 + (i2 == i1 ? 0.0 : r2 * z2);
      }
      p = in ? -(y - corr) : 0.0;
      pf.ph(11 + 6 * S);
    } else {
      real h[NV];
      bool partial = false;
      int sig = 0;
      if constexpr (S == KM_SUB_ALL && G == 16) {
        // arm-side signature of this iteration's Hessian: quadratic-zone flags of the arm dofs' own rows, edge sets of the sphere slots
        // (an inactive slot's projections are arbitrary finite numbers: not part of the signature; a condim-3 pair has no torsion edges)
        sig = (in && sub < NL ? (qf | ql << 1) : 0)
              | ((slin && sub >= 4 && ((act >> sub) & 1u)) ? (slot_edge_mask(sc, u) & (sc.D3 != 0 ? 0x3F : 0xF)) << 2 : 0);
        const bool same = cache_ok && gor<G>((int)(sig != sig0)) == 0;
        partial = __all(same);                      // (the groups of the wave that are in this branch)
      }
      if constexpr (S == KM_SUB_ALL && G == 16) { if (prob == KM_SUB_ALL) pf.cnt(partial ? 41 : 42, 1); else pf.cnt(43, partial ? 1 : 0x10000); }
      if (partial) newton_hessian_sl<NL, G, S, true>(w, sub, cr, mdiag, qf, ql, W, h, in, act, JOINT);
      else newton_hessian_sl<NL, G, S>(w, sub, cr, mdiag, qf, ql, W, h, in, act, JOINT);
      pf.ph(9 + 6 * S);
      // ---- p = -H^-1 grad
      int hbad = 0;
      bool blocks = false;
      if constexpr (S == KM_SUB_ARM && G == 32) blocks = lm.split != 0;
      if (blocks) {
        // Two-arm models: the arm problem's Hessian has the inertia's two diagonal blocks (a finger / link sphere on the table
        // touches one arm only).  Each DPP row factorises and solves ONE block with the one-row code: lane c of row r takes over
        // row base_r + c of H (block-local columns) and that dof's gradient from the lane that built them, and hands the
        // direction back -- 13 wave shuffles around two 11-pivot solves side by side instead of one 20-pivot solve across rows.
        if constexpr (S == KM_SUB_ARM && G == 32) {
          constexpr int NB = KM_BLOCK_MAX;
          const int split = lm.split, lane0 = (threadIdx.x & 63) & ~31;
          const int row = (threadIdx.x >> 4) & 1, c = threadIdx.x & 15;
          const int base = row ? split : 0, nb = row ? NL - split : split;
          const bool on = c < nb;
          const int src = lane0 + (on ? base + c : 0);
          real mine[NB], loc[NB];                                  // my dof's row of H in ITS block's column order
#pragma unroll
          for (int k = 0; k < NB; k++) {
            const real lo = h[k], hi = split == 10 ? h[(10 + k) < NL ? 10 + k : NL - 1] : h[(11 + k) < NL ? 11 + k : NL - 1];
            mine[k] = sub < split ? lo : hi;
          }
          // (round 6) all twelve shuffles in flight together: taken one at a time, each pair of ds_bpermute was waited for before the
          // next was issued (twelve round trips per iteration of a two-arm env's arm problem)
          real sv[NB];
#pragma unroll
          for (int k = 0; k < NB; k++) sv[k] = __shfl(mine[k], src, 64);
          real gsrc = __shfl(in ? -grad : 0.0, src, 64);
          static_assert(NB == 11, "the pins below name eleven block columns");
          km_pin(sv[0], sv[1], sv[2], sv[3], sv[4], sv[5]); km_pin(sv[6], sv[7], sv[8], sv[9], sv[10], gsrc);
#pragma unroll
          for (int k = 0; k < NB; k++) loc[k] = (on && k < nb) ? sv[k] : ((!on && k == c) ? 1.0 : 0.0);
          real invl = 0, utl[NB];
          chol_rows1<NB, 0, NB, 0, true>(loc, utl, invl, c, true, hbad);
          if (__any(hbad)) { const int gb = gor<G>(hbad); if (gb && sub == 0) w.bad = 1; }
          pf.ph(10 + 6 * S);
          const real pl = chol_solve_rows1<NB, 0, NB, 0>(loc, utl, invl, on ? gsrc : 0.0);
          const int back = lane0 + (sub < split ? sub : 16 + (sub < NL ? sub - split : 0));
          const real pb = __shfl(pl, back, 64);
          p = in ? pb : 0.0;
        }
      } else {
        // blocks that sit inside one DPP row use the one-row code (single-arm models: every subset; two-arm models: the cube
        // block, dofs NL..NL+5 of the group's second row)
        constexpr bool onerow = G == 16 || (S == KM_SUB_CUBE && NL >= 16);
        real invd = 0;
        if constexpr (onerow) {
          constexpr int BASE = G == 16 ? 0 : 16, ND = SS::D1 - SS::D0;
          const int sl = sub - BASE;
          const bool live = G == 16 || sub >= 16;
          real ut[NV];
          if constexpr (ND <= 6) {
            chol_rows1<NV, SS::D0, SS::D1, BASE, true>(h, ut, invd, sl, live, hbad);
          } else if constexpr (S == KM_SUB_ALL && G == 16) {
            if (partial) {
              // L's arm columns from LDS (row `sub` of the factor: exact zeros on and above the diagonal), their updates replayed on
              // the cube columns, then the cube block's six pivots
#pragma unroll
              for (int k = 0; k < NL; k++) h[k] = w.LT[sub][k];
              static_for<0, NL>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                fnmac_cols<16, NL, NV, NV, true>(h, bsrc<16>(h[k]), h[k]);
              });
              dpp_settle(h[NL]);
              real invc = 0;
              chol_rows1<NV, NL, NV, 0, false>(h, ut, invc, sl, live, hbad);
              invd = sub < NL ? invd_keep : invc;
#pragma unroll
              for (int k = NL; k < NV; k++) w.LT[sub][k] = h[k];
              GSYNC();
#pragma unroll
              for (int k = 0; k < NV; k++) ut[k] = w.LT[k][sub];
              GSYNC();
            } else {
              chol_rows1<NV, SS::D0, SS::D1, BASE, false>(h, ut, invd, sl, live, hbad);
              chol_transpose<NV, SS::D0, SS::D1, BASE>(w.LT, h, ut, sl);
              invd_keep = invd; sig0 = sig; cache_ok = true;
            }
          } else {
            chol_rows1<NV, SS::D0, SS::D1, BASE, false>(h, ut, invd, sl, live, hbad);
            chol_transpose<NV, SS::D0, SS::D1, BASE>(w.LT, h, ut, sl);
          }
          if (hbad && sub == 0) w.bad = 1;
          pf.ph(10 + 6 * S);
          p = chol_solve_rows1<NV, SS::D0, SS::D1, BASE>(h, ut, invd, in ? -grad : 0.0);
        } else {
          chol_rows<G, NV, SS::D0, SS::D1>(h, invd, sub, hbad);
          if (hbad && sub == 0) w.bad = 1;
          pf.ph(10 + 6 * S);
          p = chol_solve_rows<G, NV, SS::D0, SS::D1>(h, invd, sub, in ? -grad : 0.0);
        }
      }
      pf.ph(11 + 6 * S);
    }
    // ---- exact line search on phi(alpha) = cost(a + alpha p)
    real Mp;
    if constexpr (S == KM_SUB_CUBE) Mp = mdiag * p; else Mp = mass_mul<NL, G>(cr, sub, mdiag, p);
    real s3[3] = {in ? p * Mr : 0.0, p * Mp, in ? p * grad : 0.0};
    gsum_n<G, 3>(s3);
    const real gp = s3[0], pMp = s3[1], d10 = s3[2];
    real y[4];
    slot_project<NL, G, S>(w, cr, act, sub, p, y);
    if (!slin) { y[0] = 0; y[1] = 0; y[2] = 0; y[3] = 0; }     // slots outside the subset do not move
    const real xf = a - cr.areff, xl = cr.sg * a - cr.arefl, yl = cr.sg * p;
    pf.ph(12 + 6 * S);
    real alpha = 0, lo = 0, hi = INFINITY;
    if (d10 < 0) {
      alpha = 1;
      for (int it = 0; it < 50; it++) {
        real e1 = 0, e2 = 0;
        if (in && cr.fl > 0) row_ls(0, xf + alpha * p, p, cr.Rf, cr.Df, cr.fl, e1, e2);
        if (in && cr.sg != 0) row_ls(1, xl + alpha * yl, yl, cr.Rl, cr.Dl, 0.0, e1, e2);
        const real X[4] = {u[0] + alpha * y[0], u[1] + alpha * y[1], u[2] + alpha * y[2], u[3] + alpha * y[3]};
        slot_ls(sc, X, y, e1, e2);
        real e12[2] = {e1, e2};
        gsum_n<G, 2>(e12);
        const real d1 = gp + alpha * pMp + e12[0];
        const real d2 = pMp + e12[1];
        if (fabs(d1) <= 1e-8 * fabs(d10)) break;        // MuJoCo's ls_tolerance is 1e-2; the outer Newton absorbs the rest
        if (d1 < 0) lo = alpha; else hi = alpha;
        if (hi - lo <= 1e-14 * hi) break;                 // bracket collapsed to roundoff
        if (it == 49) break;
        real an = alpha - d1 * frcp(d2);
        if (!(an > lo && an < hi)) an = isfinite(hi) ? 0.5 * (lo + hi) : 2 * alpha + 1;
        alpha = an;
      }
    }
    pf.ph(13 + 6 * S);
    // ---- advance the point and everything linear in it, evaluate
    a += alpha * p;
    Mr += alpha * Mp;
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] += alpha * y[k];
    real F[4];
    const real cslot = slot_eval<true>(sc, u, F, W);
    real cl = slin ? cslot : 0.0;
    if (in) {
      cl += 0.5 * (a - a_s) * Mr;
      grad = Mr;
      qf = 0; ql = 0;
      if (cr.fl > 0) { real f; cl += row_eval(0, a - cr.areff, cr.Rf, cr.Df, cr.fl, f, qf); grad -= f; }
      if (cr.sg != 0) { real f; cl += row_eval(1, cr.sg * a - cr.arefl, cr.Rl, cr.Dl, 0.0, f, ql); grad -= cr.sg * f; }
    }
    real gsl = grad;
    slot_grad<NL, G, S>(cr, act, F, gsl);
    if (in) grad = gsl;
    const real g1 = in ? grad : 0.0;
    real cg[2] = {cl, g1 * g1};
    gsum_n<G, 2>(cg);
    const real cost_new = cg[0];
    const real improvement = scale * (cost - cost_new), gradient = scale * km_sqrt(cg[1]);
    cost = cost_new;
    pf.ph(14 + 6 * S);
#ifdef KM_PROFILE
    if constexpr (JOINT) { if (prob == KM_SUB_ALL) { pf.cnt(lone_it ? 44 : 45, 1); pf.it_end(lone_it ? 46 : 47); } }
#endif
    if (improvement < tol || gradient < tol || w.bad || iter + 1 >= maxit) {
      if (!(JOINT && prob == KM_SUB_ARM)) break;
      enter(KM_SUB_CUBE); cost = cost_b;        // an uncoupled env of the joint loop: on to its cube problem
      if (small()) break;
      iter = -1;
    }
  }
}

template <int NL, int G>
__device__ __forceinline__ real solve_newton_sl(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub, CReg<NL>& cr, real a_s,
                                                real invm, Prof& pf) {
  constexpr int NV = Dim<NL>::NV;
  const uint32_t act = w.cact;
  const real warm = sub < NV ? w.warm[sub] : 0.0;
  const real mdiag = (sub >= NL && sub < NV) ? 1.0 / invm : 0.0;
  real grad; int qf, ql;
  real u[4], W[7];
  real c0, c1, csl;
  real a = warm;
  real Mr = mass_mul<NL, G>(cr, sub, mdiag, warm - a_s);
  newton_eval_sl<NL, G, true>(w, sub, cr, a, a_s, Mr, grad, qf, ql, u, W, c0, c1, csl);
  real c3[3] = {csl, c0, c1};
  gsum_n<G, 3>(c3);
  const real cs = c3[0];
  real cost0 = c3[1], cost1 = c3[2];
  pf.ph(8);
  if (!(cost0 + cost1 < cs)) {
    a = a_s; Mr = 0;
    real dummy;
    newton_eval_sl<NL, G, false>(w, sub, cr, a, a_s, Mr, grad, qf, ql, u, W, c0, c1, dummy);
    real c2[2] = {c0, c1};
    gsum_n<G, 2>(c2);
    cost0 = c2[0]; cost1 = c2[1];
    pf.ph(38);
  }
  constexpr uint32_t FC_MASK = ((1u << Dim<NL>::NSS) - 1u) << 4;           // sphere-cube slots couple arm and cube
  const bool coupled = (act & FC_MASK) != 0;                               // (group-uniform)
  if constexpr (G == 16) {
    // what this group still has to run in its own loops: its arm problem and then its cube problem (an uncoupled env in a wave
    // without a coupled one), or -- after a joint loop -- whatever the joint loop handed back (nothing for the coupled env itself)
    int resume = KM_SUB_ARM, riter = 0;
    real rcost = cost0;
    if (__any(coupled)) {
      // a coupled env in the wave: its whole-problem loop and the wave-mates' arm and cube loops share one instruction stream
      // for as long as the coupled env iterates
      resume = 0;
      newton_loop_sl<NL, G, KM_SUB_ALL, true>(w, lm, m, sub, cr, mdiag, a_s, a, Mr, coupled ? cost0 + cost1 : cost0, grad, qf, ql, u, W, pf, !coupled, cost1,
                                              0, &resume, &rcost, &riter);
    }
    if (resume == KM_SUB_ARM) newton_loop_sl<NL, G, KM_SUB_ARM>(w, lm, m, sub, cr, mdiag, a_s, a, Mr, rcost, grad, qf, ql, u, W, pf, false, 0, riter);
    if (resume != 0) newton_loop_sl<NL, G, KM_SUB_CUBE>(w, lm, m, sub, cr, mdiag, a_s, a, Mr, resume == KM_SUB_ARM ? cost1 : rcost, grad, qf, ql, u, W, pf,
                                                        false, 0, resume == KM_SUB_ARM ? 0 : riter);
  } else {
    // two-row groups keep the separate loops: their cube block runs the one-row code in the second DPP row while the whole
    // problem runs the two-row code -- different operation order, so a joint loop would make an env's bits depend on its wave-mates
    if (!coupled) newton_loop_sl<NL, G, KM_SUB_ARM>(w, lm, m, sub, cr, mdiag, a_s, a, Mr, cost0, grad, qf, ql, u, W, pf);
    if (coupled) newton_loop_sl<NL, G, KM_SUB_ALL>(w, lm, m, sub, cr, mdiag, a_s, a, Mr, cost0 + cost1, grad, qf, ql, u, W, pf);
    else newton_loop_sl<NL, G, KM_SUB_CUBE>(w, lm, m, sub, cr, mdiag, a_s, a, Mr, cost1, grad, qf, ql, u, W, pf);
  }
  return a;
}

template <int NL, int G>
__device__ __forceinline__ real solve_newton(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub, int actuation,
                                             CReg<NL>& cr, real invm, Prof& pf) {
  constexpr int NV = Dim<NL>::NV;
  // ---- actuation and smooth acceleration (as in the PGS path)
  // (round 6) the lane's inputs and its row of M^-1 in one batch in front of the exchange, the right-hand sides in one behind it
  const int si = sub < NL ? sub : NL - 1, sv = sub < NV ? sub : NV - 1;
  real bia = w.bias[sv], ctl = w.ctrl[si], cr0 = lm.ctrlrange[si][0], cr1 = lm.ctrlrange[si][1], kpv = KM_EP_KP(w, lm, si), qps = w.qpos[si];
  real fr0 = lm.forcerange[si][0], fr1 = lm.forcerange[si][1];
  int flim = lm.forcelimited[si];
  real mrow[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) mrow[j] = w.Minv[si][j];
#if KM_VAR_FRC
  real fap = w.frc[sv];          // qfrc_applied of this lane's dof, in the same batch
  km_pin(fap);
#endif
  km_pin(bia, ctl, cr0, cr1, kpv, qps); km_pin(fr0, fr1); km_pin_i(flim);
  real rhs = -bia;
  if (sub < NV) {
    if (actuation && sub < NL) {
      real c = fmin(fmax(ctl, cr0), cr1);
      real force = kpv * c - kpv * qps;
      if (flim) force = fmin(fmax(force, fr0), fr1);
      rhs += force;
    }
#if KM_VAR_FRC
    if (actuation) rhs = add_applied(rhs, fap);      // every dof, outside the servo's clamps
#endif
    w.tmp[sub] = rhs;
  }
  GSYNC();
  real tv[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) tv[j] = w.tmp[j];
  real a_s = 0;
  if (sub < NL) {
#pragma unroll
    for (int j = 0; j < NL; j++) a_s += mrow[j] * tv[j];
  } else if (sub < NV) a_s = rhs * invm;
  pf.ph(7);
  return solve_newton_sl<NL, G>(w, lm, m, sub, cr, a_s, invm, pf);
}
