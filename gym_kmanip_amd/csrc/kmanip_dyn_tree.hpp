// kmanip_dyn_tree.hpp -- one of the phase headers kmanip_dyn_variant.hpp includes (inside the variant namespace) into each per-variant translation unit: kinematic tree: FK, composite inertias, mass matrix, bias forces, M^-1.
#pragma once
// mj_kinematics, all links at once: lane i builds link i's transform in its parent (constant rotation times the
// planar joint rotation; one sincos per lane instead of NL in a row), then ceil(log2(depth)) rounds of pointer
// jumping compose it with the transform of the 2^k-th ancestor (staged in the link's own xmat/xpos slots).
// kin (optional, 15 doubles): the world frame of THIS lane's link as it was written to LDS -- rotation R[9], origin p[3], centre of
// mass c[3] (zeros on lanes without a link) -- so that the passes that follow need not read their own link back (round 6)
// One-row groups (G == 16, NL <= 10; lane = link): the staged transforms never leave the registers.  A round fetches the ancestor
// lane's R[9] and p[3] with a lane gather inside the group's 16 lanes (ds_bpermute: the LDS crossbar, no LDS memory) -- 24 dwords
// issued back to back behind ONE wait -- where it used to write 12 doubles to LDS, synchronise, read the ancestor's 12 and wait
// again; xmat / xpos reach LDS once, after the last round, with cpos / axis.  The gather sits OUTSIDE the `a >= 0` branch at a
// clamped source lane (a gather's source lane must be active; lanes of a group enter and leave this function together), the
// products and their order are the ones below, the jump tables stay run-time model data.
// lane (addr >> 2)'s copy of v
__device__ __forceinline__ real lane_gather(int addr, real v) {
  const int lo = __builtin_amdgcn_ds_bpermute(addr, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(addr, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// PINNED CONTRACTIONS.  Which product of a * b + c * d is rounded on its own and which is fused into the add is the compiler's
// choice -- it follows the operand order the optimiser leaves, and that order moves when the code around an expression moves (with
// the frames in registers, the three products of R * com came out the other way round: tools/ir_fma_order.py shows such a swap
// in the optimised IR).  The one-row paths that this file moved off LDS therefore spell their sums out, with contraction off, in
// the pairing the compiler gives dot3 / cross3 / mat_vec3 as written -- the bits the library has always produced:
//   a0 b0 + a1 b1 + a2 b2 = fma(a2, b2, fma(a0, b0, rnd(a1 b1)))        a b - c d = fma(a, b, -rnd(c d))
__device__ __forceinline__ real dot3_pinned(real a0, real b0, real a1, real b1, real a2, real b2) {
#pragma clang fp contract(off)
  const real m = a1 * b1;
  return __builtin_fma(a2, b2, __builtin_fma(a0, b0, m));
}
__device__ __forceinline__ real dot3_pinned(const real* a, const real* b) { return dot3_pinned(a[0], b[0], a[1], b[1], a[2], b[2]); }
__device__ __forceinline__ real diff2_pinned(real a, real b, real c, real d) {
#pragma clang fp contract(off)
  const real m = c * d;
  return __builtin_fma(a, b, -m);
}
__device__ __forceinline__ real sum2_pinned(real a, real b, real c, real d) {
#pragma clang fp contract(off)
  const real m = c * d;
  return __builtin_fma(a, b, m);
}
__device__ __forceinline__ void cross3_pinned(real* r, const real* a, const real* b) {
  const real x = diff2_pinned(a[1], b[2], a[2], b[1]), y = diff2_pinned(a[2], b[0], a[0], b[2]), z = diff2_pinned(a[0], b[1], a[1], b[0]);
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ void mat_vec3_pinned(real* r, const real* m, const real* v) {
  const real x = dot3_pinned(m[0], v[0], m[1], v[1], m[2], v[2]), y = dot3_pinned(m[3], v[0], m[4], v[1], m[5], v[2]), z = dot3_pinned(m[6], v[0], m[7], v[1], m[8], v[2]);
  r[0] = x; r[1] = y; r[2] = z;
}
template <int NL, int G>
__device__ __forceinline__ void fk_parallel(Ws<NL>& w, const LModel<NL>& lm, int sub, real* kin = nullptr) {
  constexpr bool ROW = G == 16 && NL <= 10;
  real R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, p[3] = {0, 0, 0};
  const bool on = sub < NL;
  // (round 6) everything the pass reads about this lane's link -- its coordinate, its constant frame in the parent, its joint
  // type, its jump table, its centre of mass -- in one batch: as written, each sat behind the branch that used it
  const int li = on ? sub : 0;
  real q = w.qpos[li], lp[3] = {lm.pos[li][0], lm.pos[li][1], lm.pos[li][2]}, lR[9], cl[3] = {lm.com[li][0], lm.com[li][1], lm.com[li][2]};
#pragma unroll
  for (int c = 0; c < 9; c++) lR[c] = lm.R[li][c];
  int jt = lm.jtype[li], jmp0 = lm.jump[0][li], jmp1 = lm.jump[1][li], jmp2 = lm.jump[2][li], jmp3 = lm.jump[3][li], rounds = lm.fk_rounds;
  km_pin(q); km_pin(lp, cl); km_pin(lR); km_pin_i(jt, rounds); km_pin_i(jmp0, jmp1); km_pin_i(jmp2, jmp3);
  if (on) {
    p[0] = lp[0]; p[1] = lp[1]; p[2] = lp[2];
    if (jt == KM_JNT_SLIDE) {
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = lR[c];
      p[0] += R[2] * q; p[1] += R[5] * q; p[2] += R[8] * q;
    } else {
      real sn, cs;
      km_sincos(q, &sn, &cs);
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const real c0 = lR[3 * a], c1 = lR[3 * a + 1];
        if constexpr (ROW) {
          R[3 * a] = sum2_pinned(cs, c0, sn, c1);
          R[3 * a + 1] = diff2_pinned(cs, c1, sn, c0);
        } else {
          R[3 * a] = cs * c0 + sn * c1;
          R[3 * a + 1] = cs * c1 - sn * c0;
        }
        R[3 * a + 2] = lR[3 * a + 2];
      }
    }
    if constexpr (!ROW) {
#pragma unroll
      for (int c = 0; c < 9; c++) w.k.xmat[sub][c] = R[c];
      w.k.xpos[sub][0] = p[0]; w.k.xpos[sub][1] = p[1]; w.k.xpos[sub][2] = p[2];
    }
  } else if (sub == NL) {
    real cq[4] = {w.qpos[NL + 3], w.qpos[NL + 4], w.qpos[NL + 5], w.qpos[NL + 6]}, cm[9];
    normalize4_fast(cq);
    quat2mat(cm, cq);
#pragma unroll
    for (int c = 0; c < 9; c++) w.k.cube_mat[c] = cm[c];
  }
  if constexpr (ROW) {
    const int nrounds = __builtin_amdgcn_readfirstlane(rounds);      // (one model, one value: a scalar loop)
    const int row4 = (threadIdx.x & 48) << 2;                        // byte address of the group's lane 0 in the gather's lane space
    for (int k = 0; k < nrounds; k++) {
      const int jk = k == 0 ? jmp0 : (k == 1 ? jmp1 : (k == 2 ? jmp2 : jmp3));
      const int a = on ? jk : -1;
      const int src = row4 + (((a >= 0 ? a : 0) & 15) << 2);
      real A[9], pa[3];
#pragma unroll
      for (int c = 0; c < 9; c++) A[c] = lane_gather(src, R[c]);
#pragma unroll
      for (int c = 0; c < 3; c++) pa[c] = lane_gather(src, p[c]);
      km_pin(pa, A);
      if (a >= 0) {
        real Rn[9], t[3];
        mat_vec3_pinned(t, A, p);
        p[0] = t[0] + pa[0]; p[1] = t[1] + pa[1]; p[2] = t[2] + pa[2];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) Rn[3 * i + j] = dot3_pinned(A[3 * i], R[j], A[3 * i + 1], R[3 + j], A[3 * i + 2], R[6 + j]);
#pragma unroll
        for (int c = 0; c < 9; c++) R[c] = Rn[c];
      }
    }
  } else {
  GSYNC();
  for (int k = 0; k < rounds; k++) {
    const int jk = k == 0 ? jmp0 : (k == 1 ? jmp1 : (k == 2 ? jmp2 : jmp3));
    const int a = on ? jk : -1;
    if (a >= 0) {
      real A[9], pa[3], Rn[9], t[3];
#pragma unroll
      for (int c = 0; c < 9; c++) A[c] = w.k.xmat[a][c];
      pa[0] = w.k.xpos[a][0]; pa[1] = w.k.xpos[a][1]; pa[2] = w.k.xpos[a][2];
      mat_vec3(t, A, p);
      p[0] = t[0] + pa[0]; p[1] = t[1] + pa[1]; p[2] = t[2] + pa[2];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rn[3 * i + j] = A[3 * i] * R[j] + A[3 * i + 1] * R[3 + j] + A[3 * i + 2] * R[6 + j];
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = Rn[c];
    }
    GSYNC();
    if (a >= 0) {
#pragma unroll
      for (int c = 0; c < 9; c++) w.k.xmat[sub][c] = R[c];
      w.k.xpos[sub][0] = p[0]; w.k.xpos[sub][1] = p[1]; w.k.xpos[sub][2] = p[2];
    }
    GSYNC();
  }
  }
  real cpo[3] = {0, 0, 0};
  if (on) {
    real cw[3];
    if constexpr (ROW) {
#pragma unroll
      for (int c = 0; c < 9; c++) w.k.xmat[sub][c] = R[c];
      w.k.xpos[sub][0] = p[0]; w.k.xpos[sub][1] = p[1]; w.k.xpos[sub][2] = p[2];
    }
    if constexpr (ROW) mat_vec3_pinned(cw, R, cl);
    else mat_vec3(cw, R, cl);
    cpo[0] = p[0] + cw[0]; cpo[1] = p[1] + cw[1]; cpo[2] = p[2] + cw[2];
    w.k.cpos[sub][0] = cpo[0]; w.k.cpos[sub][1] = cpo[1]; w.k.cpos[sub][2] = cpo[2];
    w.k.axis[sub][0] = R[2]; w.k.axis[sub][1] = R[5]; w.k.axis[sub][2] = R[8];
  }
  if (kin) {
#pragma unroll
    for (int c = 0; c < 9; c++) kin[c] = on ? R[c] : 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) { kin[9 + c] = on ? p[c] : 0.0; kin[12 + c] = cpo[c]; }
  }
  GSYNC();
}

// column j of the com Jacobian of body b (world frame): linear part jv, angular part jw
template <int NL>
__device__ __forceinline__ void com_jac_col(const Ws<NL>& w, const LModel<NL>& lm, int b, int j, real* jv, real* jw) {
  if (lm.jtype[j] == KM_JNT_SLIDE) {
    jv[0] = w.k.axis[j][0]; jv[1] = w.k.axis[j][1]; jv[2] = w.k.axis[j][2];
    jw[0] = 0; jw[1] = 0; jw[2] = 0;
  } else {
    real r[3] = {w.k.cpos[b][0] - w.k.xpos[j][0], w.k.cpos[b][1] - w.k.xpos[j][1], w.k.cpos[b][2] - w.k.xpos[j][2]};
    real ax[3] = {w.k.axis[j][0], w.k.axis[j][1], w.k.axis[j][2]};
    cross3(jv, ax, r);
    jw[0] = ax[0]; jw[1] = ax[1]; jw[2] = ax[2];
  }
}

// Composite-rigid-body mass matrix.  Lane b first writes body b's own (mass, first moment m*c, inertia about
// the world origin) -- 10 numbers; lane 0 then suffix-accumulates them up the tree (children into parents);
// lane j finally projects the unit-acceleration wrench of its composite onto every ancestor joint:
//   F = mc*a_O + alpha x h,  N_O = Io*alpha + h x a_O   (hinge: alpha = axis_j, a_O = o_j x axis_j; slide: a_O = axis_j)
//   M_ij = axis_i . (N_O - o_i x F)  (hinge i)   |   axis_i . F  (slide i)
template <int NL, int G>
__device__ __forceinline__ void composite_own(Ws<NL>& w, const LModel<NL>& lm, int sub) {
  for (int b = sub; b < NL; b += G) {
    const real mb = lm.mass[b];
    const real c[3] = {w.k.cpos[b][0], w.k.cpos[b][1], w.k.cpos[b][2]};
    const real* R = w.k.xmat[b];
    const real I0 = lm.inertia[b][0], I1 = lm.inertia[b][1], I2 = lm.inertia[b][2];
    const real cc = dot3(c, c);
    real* o = w.f.comp[b];
    o[0] = mb; o[1] = mb * c[0]; o[2] = mb * c[1]; o[3] = mb * c[2];
    // R diag(I) R^T + m (|c|^2 1 - c c^T), packed xx xy xz yy yz zz
    o[4] = R[0] * R[0] * I0 + R[1] * R[1] * I1 + R[2] * R[2] * I2 + mb * (cc - c[0] * c[0]);
    o[5] = R[0] * R[3] * I0 + R[1] * R[4] * I1 + R[2] * R[5] * I2 - mb * c[0] * c[1];
    o[6] = R[0] * R[6] * I0 + R[1] * R[7] * I1 + R[2] * R[8] * I2 - mb * c[0] * c[2];
    o[7] = R[3] * R[3] * I0 + R[4] * R[4] * I1 + R[5] * R[5] * I2 + mb * (cc - c[1] * c[1]);
    o[8] = R[3] * R[6] * I0 + R[4] * R[7] * I1 + R[5] * R[8] * I2 - mb * c[1] * c[2];
    o[9] = R[6] * R[6] * I0 + R[7] * R[7] * I1 + R[8] * R[8] * I2 + mb * (cc - c[2] * c[2]);
  }
}
// subtree sums, one link per lane: comp/FN of link i += those of its proper descendants (read-all, sync, write)
template <int NL, int G>
__device__ __forceinline__ void composite_accumulate(Ws<NL>& w, const LModel<NL>& lm, int sub) {
  real acc[16];
  const bool on = sub < NL;
  if (on) {
    if constexpr (NL <= 10) {
    // every candidate j at a compile-time address (all loads can be in flight together; no mask-driven pointer chase),
    // taken or not by its descendant bit.  Links are ordered parents-first, so descendants have larger indices.
    const uint32_t dm = lm.desc[sub];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const bool take = (dm >> j) & 1u;                 // (bit `sub` itself is set: the link's own contribution)
#pragma unroll
      for (int k = 0; k < 10; k++) { const real v = w.f.comp[j][k]; acc[k] += take ? v : 0.0; }
#pragma unroll
      for (int k = 0; k < 6; k++) { const real v = w.f.FN[j][k]; acc[10 + k] += take ? v : 0.0; }
    }
    } else {                                            // (the 20-link kernels sit at the 512-register limit: rolled mask walk)
#pragma unroll
      for (int k = 0; k < 10; k++) acc[k] = w.f.comp[sub][k];
#pragma unroll
      for (int k = 0; k < 6; k++) acc[10 + k] = w.f.FN[sub][k];
      for (uint32_t mk = lm.desc[sub] & ~(1u << sub); mk; mk &= mk - 1) {
        const int j = __ffs(mk) - 1;
#pragma unroll
        for (int k = 0; k < 10; k++) acc[k] += w.f.comp[j][k];
#pragma unroll
        for (int k = 0; k < 6; k++) acc[10 + k] += w.f.FN[j][k];
      }
    }
  }
  GSYNC();
  if (on) {
#pragma unroll
    for (int k = 0; k < 10; k++) w.f.comp[sub][k] = acc[k];
#pragma unroll
    for (int k = 0; k < 6; k++) w.f.FN[sub][k] = acc[10 + k];
  }
}
template <int NL, int G>
__device__ __forceinline__ void mass_matrix(Ws<NL>& w, const LModel<NL>& lm, int sub) {
  for (int j = sub; j < NL; j += G) {
    const real* o = w.f.comp[j];
    const real ax[3] = {w.k.axis[j][0], w.k.axis[j][1], w.k.axis[j][2]};
    const real oj[3] = {w.k.xpos[j][0], w.k.xpos[j][1], w.k.xpos[j][2]};
    const real h[3] = {o[1], o[2], o[3]};
    real F[3], N[3], t[3];
    if (lm.jtype[j] == KM_JNT_SLIDE) {
      F[0] = o[0] * ax[0]; F[1] = o[0] * ax[1]; F[2] = o[0] * ax[2];
      cross3(N, h, ax);
    } else {
      real aO[3];
      cross3(aO, oj, ax);
      cross3(t, ax, h);
      F[0] = o[0] * aO[0] + t[0]; F[1] = o[0] * aO[1] + t[1]; F[2] = o[0] * aO[2] + t[2];
      N[0] = o[4] * ax[0] + o[5] * ax[1] + o[6] * ax[2];
      N[1] = o[5] * ax[0] + o[7] * ax[1] + o[8] * ax[2];
      N[2] = o[6] * ax[0] + o[8] * ax[1] + o[9] * ax[2];
      cross3(t, h, aO);
      N[0] += t[0]; N[1] += t[1]; N[2] += t[2];
    }
    // rows i = ancestors of j (incl. j), every candidate i at a compile-time address and taken by its ancestor bit -- no
    // pointer chase up the tree through LDS; non-ancestors get the zero they need (the reader mirrors the triangle)
    const uint32_t am = lm.anc[j];
#pragma unroll KM_TREE_UNROLL(NL)
    for (int i = 0; i < NL; i++) {
      const real ai[3] = {w.k.axis[i][0], w.k.axis[i][1], w.k.axis[i][2]};
      const real oi[3] = {w.k.xpos[i][0], w.k.xpos[i][1], w.k.xpos[i][2]};
      cross3(t, oi, F);
      const real mo[3] = {N[0] - t[0], N[1] - t[1], N[2] - t[2]};
      const real val = lm.jtype[i] == KM_JNT_SLIDE ? dot3(ai, F) : dot3(ai, mo);
      w.Minv[i][j] = ((am >> i) & 1u) ? val : 0.0;
    }
  }
}
// One-row groups (NL <= 10, G = 16): composite inertias and subtree wrenches WITHOUT the LDS round trips.  Lane b builds link
// b's own ten composite numbers in registers, takes its bias wrench, and every lane sums over its descendants with
// broadcast-FMAs (acc_k += bcast_j(own_k) * [j in subtree(sub)], runs of four behind one pair of wait states): 160 LDS reads,
// 32 LDS writes and two synchronisations become 40 four-instruction runs.  Then the lane projects ITS composite's unit-
// acceleration wrench onto its ancestors' joints (column `sub` of M, rows through LDS for the row-per-lane inversion) and its
// subtree wrench onto its own joint (bias).
template <int NL, int W>
__device__ __forceinline__ void composite_mass_bias_rows(Ws<NL>& w, const LModel<NL>& lm, int li, int base, const real (&FN)[6], const real* kin = nullptr) {
  static_assert(W <= 16, "one DPP row per block");
  const bool on = li >= 0;
  const int b = on ? li : 0;
  // (round 6) the link's frame from fk_parallel's registers (kin; else one batch from LDS), its constants in one batch
  real Rk[9], oj[3], c[3];
  real massb = lm.mass[b], I0 = lm.inertia[b][0], I1 = lm.inertia[b][1], I2 = lm.inertia[b][2];
  int jtb = lm.jtype[b];
  uint32_t descb = lm.desc[b], ancb = lm.anc[b];
  if (kin) {
#pragma unroll
    for (int k = 0; k < 9; k++) Rk[k] = kin[k];
#pragma unroll
    for (int k = 0; k < 3; k++) { oj[k] = kin[9 + k]; c[k] = kin[12 + k]; }
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++) Rk[k] = w.k.xmat[b][k];
#pragma unroll
    for (int k = 0; k < 3; k++) { oj[k] = w.k.xpos[b][k]; c[k] = w.k.cpos[b][k]; }
    km_pin(Rk); km_pin(oj, c);
  }
  km_pin(massb, I0, I1, I2); km_pin_i(jtb); asm volatile("" : "+v"(descb), "+v"(ancb));
  real own[16];
  {
    const real mb = on ? massb : 0.0;
    const real* R = Rk;
    const real cc = dot3(c, c);
    own[0] = mb; own[1] = mb * c[0]; own[2] = mb * c[1]; own[3] = mb * c[2];
    // R diag(I) R^T + m (|c|^2 1 - c c^T), packed xx xy xz yy yz zz
    own[4] = R[0] * R[0] * I0 + R[1] * R[1] * I1 + R[2] * R[2] * I2 + mb * (cc - c[0] * c[0]);
    own[5] = R[0] * R[3] * I0 + R[1] * R[4] * I1 + R[2] * R[5] * I2 - mb * c[0] * c[1];
    own[6] = R[0] * R[6] * I0 + R[1] * R[7] * I1 + R[2] * R[8] * I2 - mb * c[0] * c[2];
    own[7] = R[3] * R[3] * I0 + R[4] * R[4] * I1 + R[5] * R[5] * I2 + mb * (cc - c[1] * c[1]);
    own[8] = R[3] * R[6] * I0 + R[4] * R[7] * I1 + R[5] * R[8] * I2 - mb * c[1] * c[2];
    own[9] = R[6] * R[6] * I0 + R[7] * R[7] * I1 + R[8] * R[8] * I2 + mb * (cc - c[2] * c[2]);
#pragma unroll
    for (int k = 0; k < 6; k++) own[10 + k] = FN[k];
    if (!on) {
#pragma unroll
      for (int k = 0; k < 16; k++) own[k] = 0;
    }
  }
  real acc[16];
#pragma unroll
  for (int k = 0; k < 16; k++) acc[k] = 0;
  const uint32_t dm = on ? descb >> base : 0u;   // row-local bits (the link's own bit is set: its own contribution)
  static_for<0, W>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const real take = ((dm >> j) & 1u) ? 1.0 : 0.0;
    constexpr bool WT = j == 0;                  // (the sources own[] are read again for every j: only the first pass can trail their writes)
    dppfma4<false, j, j, j, j, WT>(acc[0], own[0], take, acc[1], own[1], take, acc[2], own[2], take, acc[3], own[3], take);
    dppfma4<false, j, j, j, j, WT>(acc[4], own[4], take, acc[5], own[5], take, acc[6], own[6], take, acc[7], own[7], take);
    dppfma4<false, j, j, j, j, WT>(acc[8], own[8], take, acc[9], own[9], take, acc[10], own[10], take, acc[11], own[11], take);
    dppfma4<false, j, j, j, j, WT>(acc[12], own[12], take, acc[13], own[13], take, acc[14], own[14], take, acc[15], own[15], take);
  });
  if (on) {
    const int j = li;
    const real* o = acc;
    const real ax[3] = {Rk[2], Rk[5], Rk[8]};
    const real h[3] = {o[1], o[2], o[3]};
    real F[3], N[3], t[3];
    const bool slide = jtb == KM_JNT_SLIDE;
    if (slide) {
      F[0] = o[0] * ax[0]; F[1] = o[0] * ax[1]; F[2] = o[0] * ax[2];
      cross3(N, h, ax);
    } else {
      real aO[3];
      cross3(aO, oj, ax);
      cross3(t, ax, h);
      F[0] = o[0] * aO[0] + t[0]; F[1] = o[0] * aO[1] + t[1]; F[2] = o[0] * aO[2] + t[2];
      N[0] = o[4] * ax[0] + o[5] * ax[1] + o[6] * ax[2];
      N[1] = o[5] * ax[0] + o[7] * ax[1] + o[8] * ax[2];
      N[2] = o[6] * ax[0] + o[8] * ax[1] + o[9] * ax[2];
      cross3(t, h, aO);
      N[0] += t[0]; N[1] += t[1]; N[2] += t[2];
    }
    const uint32_t am = ancb;
    // Round 6: one basic block.  With the stores inside `if (i <= j)` the compiler sank each row's six LDS loads into that row's
    // conditional block: ten load -> wait -> compute -> store round trips in a row (one wave per SIMD: nothing hides them).  Now every
    // row's entry is stored unconditionally -- rows this lane does not own go to a scratch slot of its own (w.tmp[j], not live before
    // the solve) -- so nothing is conditional, and the scheduler issues the rows' loads together.  Same operations, same bits.
    real mcol[W];
    if constexpr (W == NL && NL <= 10) {
      // One-row groups (lane = link, base = 0): row i's joint axis, origin and type are lane i's OWN registers (ax, oj, jtb), so they
      // arrive by row broadcast.  Read from LDS -- whatever the scheduling hint below asked for -- the rows came out as a chain of
      // load -> wait -> compute steps: about a dozen exposed LDS round trips per call with one wave per SIMD.  Same values (the
      // LDS copies are these registers, stored by fk_parallel), same operations on them.  Lane i < NL is inside this branch: active.
      static_for<0, W>([&](auto cc) {
        constexpr int i = decltype(cc)::value;
        const real ai[3] = {gbcast<16, i>(ax[0]), gbcast<16, i>(ax[1]), gbcast<16, i>(ax[2])};
        const real oi[3] = {gbcast<16, i>(oj[0]), gbcast<16, i>(oj[1]), gbcast<16, i>(oj[2])};
        const int jti = dpp_i32<0x150 + i>(jtb);
        cross3_pinned(t, oi, F);
        const real mo[3] = {N[0] - t[0], N[1] - t[1], N[2] - t[2]};
        const real val = jti == KM_JNT_SLIDE ? dot3_pinned(ai, F) : dot3_pinned(ai, mo);
        mcol[i] = ((am >> i) & 1u) ? val : 0.0;
      });
    } else {
#pragma unroll
    for (int c = 0; c < W; c++) {
      const int i = base + c < NL ? base + c : NL - 1;      // rows of the block only: M has no entries between blocks (clamped: never stored)
      const real ai[3] = {w.k.axis[i][0], w.k.axis[i][1], w.k.axis[i][2]};
      const real oi[3] = {w.k.xpos[i][0], w.k.xpos[i][1], w.k.xpos[i][2]};
      cross3(t, oi, F);
      const real mo[3] = {N[0] - t[0], N[1] - t[1], N[2] - t[2]};
      const real val = lm.jtype[i] == KM_JNT_SLIDE ? dot3(ai, F) : dot3(ai, mo);
      mcol[c] = ((am >> i) & 1u) ? val : 0.0;
    }
    // (scheduling hint for the block above: all the rows' LDS reads first, then the arithmetic)
    __builtin_amdgcn_sched_group_barrier(0x100, 8 * W, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 64 * W, 0);
    }
#pragma unroll
    for (int c = 0; c < W; c++) {
      const int i = base + c;
      if (W != NL && i >= NL) continue;
      // both triangles: the inversion then reads plain rows; entry (a, b) is written by the lane of link max(a, b) only
      real* const up = i <= j ? &w.Minv[i][j] : &w.tmp[j];
      real* const lo = i <= j ? &w.Minv[j][i] : &w.tmp[j];
      *up = mcol[c];
      *lo = mcol[c];
    }
    // bias_j = axis_j . (subtree wrench about the joint)
    const real Fb[3] = {acc[10], acc[11], acc[12]};
    if (slide) w.bias[j] = dot3(ax, Fb);
    else {
      cross3(t, oj, Fb);
      const real mo[3] = {acc[13] - t[0], acc[14] - t[1], acc[15] - t[2]};
      w.bias[j] = dot3(ax, mo);
    }
  }
}

// lower triangle from the upper one (column j only wrote rows i <= j along its ancestor path)
template <int NL, int G>
__device__ __forceinline__ void mass_symmetrize(Ws<NL>& w, int sub) {
  for (int j = sub; j < NL; j += G)
    for (int i = j + 1; i < NL; i++) w.Minv[i][j] = w.Minv[j][i];
}

// ---------------------------------------------------------------------------------------------
// Velocity-product + gravity wrench of every body (then bias_j = sum_b J_bj^T wrench_b), one link per lane.  omega, alpha and the origin acceleration of a link are sums of per-link
// increments over its ancestors, so each lane first publishes its increment (LDS), then sums along its own
// ancestor mask in root-to-leaf order (the order of the serial recursion):
//   omega_i = sum_j wv_j,          wv_j = axis_j qvel_j (hinge)
//   alpha_i = sum_j cz_j (hinge),  cz_j = omega_parent(j) x wv_j
//   a_i     = -g + sum_j d_j,      d_j  = alpha_p x r_j + omega_p x (omega_p x r_j) (+ 2 cz_j for a slide)
template <int NL, int G>
__device__ __forceinline__ void bias_bodies_parallel(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub) {
  real* wvb = &w.f.bsc[0][0];           // [NL][3] each
  real* czb = wvb + 3 * NL;
  real* dbb = czb + 3 * NL;
  const bool on = sub < NL;
  const bool slide = on && lm.jtype[sub] == KM_JNT_SLIDE;
  const uint32_t up = on ? (lm.anc[sub] & ~(1u << sub)) : 0u;       // proper ancestors
  real ax[3] = {0, 0, 0};
  if (on) {
    const real qv = w.qvel[sub];
    ax[0] = w.k.axis[sub][0] * qv; ax[1] = w.k.axis[sub][1] * qv; ax[2] = w.k.axis[sub][2] * qv;
    wvb[3 * sub] = slide ? 0.0 : ax[0]; wvb[3 * sub + 1] = slide ? 0.0 : ax[1]; wvb[3 * sub + 2] = slide ? 0.0 : ax[2];
  }
  GSYNC();
  real wp[3] = {0, 0, 0}, cz[3] = {0, 0, 0};
  if (on) {
#pragma unroll KM_TREE_UNROLL(NL)
    for (int j = 0; j < NL; j++) {                                     // (static addresses, taken by the ancestor bit; root-to-leaf order)
      const bool take = (up >> j) & 1u;
      const real v0 = wvb[3 * j], v1 = wvb[3 * j + 1], v2 = wvb[3 * j + 2];
      wp[0] += take ? v0 : 0.0; wp[1] += take ? v1 : 0.0; wp[2] += take ? v2 : 0.0;
    }
    cross3(cz, wp, ax);
    czb[3 * sub] = slide ? 0.0 : cz[0]; czb[3 * sub + 1] = slide ? 0.0 : cz[1]; czb[3 * sub + 2] = slide ? 0.0 : cz[2];
  }
  GSYNC();
  real alp[3] = {0, 0, 0};
  if (on) {
#pragma unroll KM_TREE_UNROLL(NL)
    for (int j = 0; j < NL; j++) {
      const bool take = (up >> j) & 1u;
      const real v0 = czb[3 * j], v1 = czb[3 * j + 1], v2 = czb[3 * j + 2];
      alp[0] += take ? v0 : 0.0; alp[1] += take ? v1 : 0.0; alp[2] += take ? v2 : 0.0;
    }
    const int p = lm.parent[sub];
    real op[3] = {0, 0, 0};
    if (p >= 0) { op[0] = w.k.xpos[p][0]; op[1] = w.k.xpos[p][1]; op[2] = w.k.xpos[p][2]; }
    real r[3] = {w.k.xpos[sub][0] - op[0], w.k.xpos[sub][1] - op[1], w.k.xpos[sub][2] - op[2]}, t1[3], t2[3];
    cross3(t1, alp, r);
    cross3(t2, wp, r); cross3(t2, wp, t2);
#pragma unroll
    for (int c = 0; c < 3; c++) dbb[3 * sub + c] = t1[c] + t2[c] + (slide ? 2 * cz[c] : 0.0);
  }
  GSYNC();
  if (on) {
    real ai[3] = {-m->gravity[0], -m->gravity[1], -m->gravity[2]};
    const uint32_t am = lm.anc[sub];
#pragma unroll KM_TREE_UNROLL(NL)
    for (int j = 0; j < NL; j++) {
      const bool take = (am >> j) & 1u;
      const real v0 = dbb[3 * j], v1 = dbb[3 * j + 1], v2 = dbb[3 * j + 2];
      ai[0] += take ? v0 : 0.0; ai[1] += take ? v1 : 0.0; ai[2] += take ? v2 : 0.0;
    }
    real wi[3] = {wp[0], wp[1], wp[2]}, ali[3] = {alp[0], alp[1], alp[2]};
    if (!slide) {
#pragma unroll
      for (int c = 0; c < 3; c++) { wi[c] += ax[c]; ali[c] += cz[c]; }
    }
    const int i = sub;
    real cr[3] = {w.k.cpos[i][0] - w.k.xpos[i][0], w.k.cpos[i][1] - w.k.xpos[i][1], w.k.cpos[i][2] - w.k.xpos[i][2]}, t1[3], t2[3];
    cross3(t1, ali, cr);
    cross3(t2, wi, cr); cross3(t2, wi, t2);
    real wl[3], all[3], Iw[3], nl3[3], nw[3];
    matT_vec3(wl, w.k.xmat[i], wi);
    matT_vec3(all, w.k.xmat[i], ali);
#pragma unroll
    for (int c = 0; c < 3; c++) Iw[c] = lm.inertia[i][c] * wl[c];
    cross3(nl3, wl, Iw);
#pragma unroll
    for (int c = 0; c < 3; c++) nl3[c] += lm.inertia[i][c] * all[c];
    mat_vec3(nw, w.k.xmat[i], nl3);
    real Fi[3] = {lm.mass[i] * (ai[0] + t1[0] + t2[0]), lm.mass[i] * (ai[1] + t1[1] + t2[1]), lm.mass[i] * (ai[2] + t1[2] + t2[2])};
    real cpi[3] = {w.k.cpos[i][0], w.k.cpos[i][1], w.k.cpos[i][2]}, sh[3];
    cross3(sh, cpi, Fi);                       // shift the moment from the com to the world origin
#pragma unroll
    for (int c = 0; c < 3; c++) { w.f.FN[i][c] = Fi[c]; w.f.FN[i][3 + c] = nw[c] + sh[c]; }
  } else if (sub == NL) {
    // cube (free joint, qvel = [v_world, w_body]): bias = [-m g, w x I w]
    real wv[3] = {w.qvel[NL + 3], w.qvel[NL + 4], w.qvel[NL + 5]};
    real Iw[3] = {KM_EP_INERTIA(w, m, 0) * wv[0], KM_EP_INERTIA(w, m, 1) * wv[1], KM_EP_INERTIA(w, m, 2) * wv[2]}, t[3];
    cross3(t, wv, Iw);
#pragma unroll
    for (int c = 0; c < 3; c++) { w.bias[NL + c] = -KM_EP_MASS(w, m) * m->gravity[c]; w.bias[NL + 3 + c] = t[c]; }
  }
}

// One-row groups: the bias-wrench pass with the three ancestor sums as broadcast-FMAs (s += bcast_j(v) * [j in mask], link
// order = root-to-leaf order) instead of LDS publish / synchronise / read rounds; the link's wrench stays in registers (FN).
template <int NL, int G>
__device__ __forceinline__ void anc_sum3(uint32_t mask, const real* v, real* s) {      // (NL here = the row's width)
  static_for<0, NL>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const real take = ((mask >> j) & 1u) ? 1.0 : 0.0;
    dppfma3<false, j, j, j, j == 0>(s[0], v[0], take, s[1], v[1], take, s[2], v[2], take);
  });
}
// cube (free joint, qvel = [v_world, w_body]): bias = [-m g, w x I w]
template <int NL>
__device__ __forceinline__ void cube_bias(Ws<NL>& w, const KModelDesc* m) {
  real wc[3] = {w.qvel[NL + 3], w.qvel[NL + 4], w.qvel[NL + 5]};
  real Iw[3] = {KM_EP_INERTIA(w, m, 0) * wc[0], KM_EP_INERTIA(w, m, 1) * wc[1], KM_EP_INERTIA(w, m, 2) * wc[2]}, t[3];
  cross3(t, wc, Iw);
#pragma unroll
  for (int c = 0; c < 3; c++) { w.bias[NL + c] = -KM_EP_MASS(w, m) * m->gravity[c]; w.bias[NL + 3 + c] = t[c]; }
}
// W = links per DPP row.  One-row groups: the row holds the whole robot (li = sub, base = 0, W = NL).  Two-row groups with a
// block split (two-arm models): each row holds one block of the robot -- lane c of a row works on link li = base + c of ITS
// block, masks are taken relative to the block's first link, and both blocks go through the same instructions at once.
// kin != nullptr (one-row groups, lane = link): the link's own frame from fk_parallel's registers instead of LDS.
template <int NL, int W>
__device__ __forceinline__ void bias_bodies_rows(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int li, int base, bool cube_lane, real (&FN)[6],
                                                 const real* kin = nullptr) {
  static_assert(W <= 16, "one DPP row per block");
  constexpr int G = 16;
  const bool on = li >= 0;
  const int i = on ? li : 0;
  // (round 6) the link's constants and state in one batch; the parent's origin -- the one dependent read -- right behind it
  int jti = lm.jtype[i], pari = lm.parent[i];
  uint32_t anci = lm.anc[i];
  real qvi = w.qvel[i], in0 = lm.inertia[i][0], in1 = lm.inertia[i][1], in2 = lm.inertia[i][2], massi = lm.mass[i];
  real Rk[9], xo[3], cpi[3];
  if (kin) {
#pragma unroll
    for (int c = 0; c < 9; c++) Rk[c] = kin[c];
#pragma unroll
    for (int c = 0; c < 3; c++) { xo[c] = kin[9 + c]; cpi[c] = kin[12 + c]; }
  } else {
#pragma unroll
    for (int c = 0; c < 9; c++) Rk[c] = w.k.xmat[i][c];
#pragma unroll
    for (int c = 0; c < 3; c++) { xo[c] = w.k.xpos[i][c]; cpi[c] = w.k.cpos[i][c]; }
    km_pin(Rk); km_pin(xo, cpi);
  }
  km_pin_i(jti, pari); asm volatile("" : "+v"(anci)); km_pin(qvi, in0, in1, in2, massi);
  real op[3] = {0, 0, 0};
  { const int pc = pari >= 0 ? pari : 0; op[0] = w.k.xpos[pc][0]; op[1] = w.k.xpos[pc][1]; op[2] = w.k.xpos[pc][2]; }
  if (!(on && pari >= 0)) { op[0] = 0; op[1] = 0; op[2] = 0; }
  const bool slide = on && jti == KM_JNT_SLIDE;
  const uint32_t am = on ? anci >> base : 0u, up = am & ~(1u << (i - base));       // ancestors incl. self / proper ancestors (row-local bits)
  const real qv = on ? qvi : 0.0;
  const real ax[3] = {Rk[2] * qv, Rk[5] * qv, Rk[8] * qv};                           // (the joint axis = third column of the link's rotation)
  const real wv[3] = {(slide || !on) ? 0.0 : ax[0], (slide || !on) ? 0.0 : ax[1], (slide || !on) ? 0.0 : ax[2]};
  real wp[3] = {0, 0, 0}, cz[3], alp[3] = {0, 0, 0};
  anc_sum3<W, G>(up, wv, wp);
  cross3(cz, wp, ax);
  const real czv[3] = {(slide || !on) ? 0.0 : cz[0], (slide || !on) ? 0.0 : cz[1], (slide || !on) ? 0.0 : cz[2]};
  anc_sum3<W, G>(up, czv, alp);
  real r[3] = {xo[0] - op[0], xo[1] - op[1], xo[2] - op[2]}, t1[3], t2[3], db[3];
  cross3(t1, alp, r);
  cross3(t2, wp, r); cross3(t2, wp, t2);
#pragma unroll
  for (int c = 0; c < 3; c++) db[c] = on ? t1[c] + t2[c] + (slide ? 2 * cz[c] : 0.0) : 0.0;
  real ai[3] = {-m->gravity[0], -m->gravity[1], -m->gravity[2]};
  anc_sum3<W, G>(am, db, ai);
  if (on) {
    real wi[3] = {wp[0], wp[1], wp[2]}, ali[3] = {alp[0], alp[1], alp[2]};
    if (!slide) {
#pragma unroll
      for (int c = 0; c < 3; c++) { wi[c] += ax[c]; ali[c] += cz[c]; }
    }
    real cr[3] = {cpi[0] - xo[0], cpi[1] - xo[1], cpi[2] - xo[2]};
    cross3(t1, ali, cr);
    cross3(t2, wi, cr); cross3(t2, wi, t2);
    real wl[3], all[3], Iw[3], nl3[3], nw[3];
    const real inr[3] = {in0, in1, in2};
    matT_vec3(wl, Rk, wi);
    matT_vec3(all, Rk, ali);
#pragma unroll
    for (int c = 0; c < 3; c++) Iw[c] = inr[c] * wl[c];
    cross3(nl3, wl, Iw);
#pragma unroll
    for (int c = 0; c < 3; c++) nl3[c] += inr[c] * all[c];
    mat_vec3(nw, Rk, nl3);
    real Fi[3] = {massi * (ai[0] + t1[0] + t2[0]), massi * (ai[1] + t1[1] + t2[1]), massi * (ai[2] + t1[2] + t2[2])}, sh[3];
    cross3(sh, cpi, Fi);                       // shift the moment from the com to the world origin
#pragma unroll
    for (int c = 0; c < 3; c++) { FN[c] = Fi[c]; FN[3 + c] = nw[c] + sh[c]; }
  } else {
#pragma unroll
    for (int c = 0; c < 6; c++) FN[c] = 0;
    if (cube_lane) cube_bias<NL>(w, m);
  }
}

template <int NL, int G>
__device__ __forceinline__ void bias_project(Ws<NL>& w, const LModel<NL>& lm, int sub) {
  // FN[j] now holds the accumulated wrench of subtree(j) about the world origin
  for (int j = sub; j < NL; j += G) {
    const real aj[3] = {w.k.axis[j][0], w.k.axis[j][1], w.k.axis[j][2]};
    const real F[3] = {w.f.FN[j][0], w.f.FN[j][1], w.f.FN[j][2]};
    if (lm.jtype[j] == KM_JNT_SLIDE) w.bias[j] = dot3(aj, F);
    else {
      const real oj[3] = {w.k.xpos[j][0], w.k.xpos[j][1], w.k.xpos[j][2]};
      real t[3];
      cross3(t, oj, F);
      real mo[3] = {w.f.FN[j][3] - t[0], w.f.FN[j][4] - t[1], w.f.FN[j][5] - t[2]};
      w.bias[j] = dot3(aj, mo);
    }
  }
}

// upd[j] -= bcast_K(a[j]) * f for j in [J0, J1), j != K (Gauss-Jordan row update), runs of four / singles
template <int G, int K, int J0, int J1, int N>
__device__ __forceinline__ void gj_cols(real (&upd)[N], const real (&a)[N], real f) {
  if constexpr (G == 16 && J1 - J0 >= 4 && !(K >= J0 && K < J0 + 4)) {
    dppfma4<true, K, K, K, K>(upd[J0], a[J0], f, upd[J0 + 1], a[J0 + 1], f, upd[J0 + 2], a[J0 + 2], f, upd[J0 + 3], a[J0 + 3], f);
    gj_cols<G, K, J0 + 4, J1>(upd, a, f);
  } else if constexpr (J1 - J0 >= 1) {
    if constexpr (J0 != K) fnmac_b<G, K>(upd[J0], bsrc<G>(a[J0]), f);
    gj_cols<G, K, J0 + 1, J1>(upd, a, f);
  }
}

// Minv <- inverse of the SPD joint-space inertia held in Minv.  Lane i takes row i into registers and the
// group runs an in-place Gauss-Jordan sweep (no pivoting: every pivot of an SPD matrix is a positive Schur
// complement); row k reaches the other lanes through DPP row broadcasts, so there is no LDS traffic and no
// synchronisation inside the n^2 loop.
// In-place Gauss-Jordan sweep of the SPD matrix whose row `me` this lane holds in a[0..N) (one matrix per DPP row; no
// pivoting: every pivot of an SPD matrix is a positive Schur complement).  Row k reaches the other lanes through DPP row
// broadcasts, so there is no LDS traffic and no synchronisation inside the n^2 loop.
// a[j] -= bcast_K(a[j]) * f IN PLACE for j in [J0, J1), j != K: each instruction reads its own destination register through
// DPP (lane K's copy, before any lane writes it) -- no second register set, no selects.  Every run spends the two DPP wait
// states: a source may have been written by a plain select (the loads' masking before the first pivot, the pivot column's
// update) that the scheduler is free to place directly in front of the run.
template <int K, int J0, int J1, int N>
__device__ __forceinline__ void gj_cols_inplace(real (&a)[N], real f) {
#define KM_GJ1(I) "v_fmac_f64_dpp %" #I ", -%" #I ", %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
  if constexpr (J1 - J0 >= 4 && !(K >= J0 && K < J0 + 4)) {
    asm volatile("s_nop 1\n\t" KM_GJ1(0) KM_GJ1(1) KM_GJ1(2) KM_GJ1(3) : "+v"(a[J0]), "+v"(a[J0 + 1]), "+v"(a[J0 + 2]), "+v"(a[J0 + 3]) : "v"(f), "n"(K));
    gj_cols_inplace<K, J0 + 4, J1>(a, f);
  } else if constexpr (J1 - J0 >= 1) {
    if constexpr (J0 != K) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, -%0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(a[J0]) : "v"(f), "n"(K));
    gj_cols_inplace<K, J0 + 1, J1>(a, f);
  }
#undef KM_GJ1
}
template <int G, int N>
__device__ __forceinline__ void gj_invert_rows(real (&a)[N], int me_idx, int& bad) {
  static_for<0, N>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if constexpr (G == 16) {
      // one-row form (round 3): the pivot row scales itself through the same update as the others -- with f = 1 - d on the
      // pivot's own lane, a_kj - a_kj (1 - d) = a_kj d -- so a pivot costs one select for f and one for the pivot column
      // instead of two per column, and the update runs in place
      if constexpr (k > 0) dpp_settle(a[k]);           // (written by the previous pivot's runs: the broadcast below is compiler code)
      const real pk = gbcast<G, k>(a[k]);
      bad |= !(pk > 0);
      const real d = frcp(pk);
      const bool me = me_idx == k;
      const real f = me ? 1.0 - d : a[k] * d;
      gj_cols_inplace<k, 0, N>(a, f);
      a[k] = me ? d : -f;
    } else {
    real pk = gbcast<G, k>(a[k]);
    if (!(pk > 0)) { bad = 1; pk = 1; }
    const real d = frcp(pk);
    const real aik = a[k];
    const bool me = me_idx == k;
    // a_ij - (a_ik / p) a_kj for every column j != k, row k arriving by DPP: all columns of a pivot are independent, so
    // they go in runs of four behind one pair of wait states
    real upd[N];
    const real f = aik * d;
#pragma unroll
    for (int j = 0; j < N; j++) upd[j] = a[j];
    gj_cols<G, k, 0, N>(upd, a, f);
#pragma unroll
    for (int j = 0; j < N; j++) if (j != k) a[j] = me ? a[j] * d : upd[j];
    a[k] = me ? d : -aik * d;
    }
  });
}

// Two-arm models: the trees [0, split) and [split, NL) share no dof, so the inertia is two diagonal blocks.  Row r of the
// group inverts block r (lane c <-> link base + c, the mapping of the tree passes; M comes from and goes back to LDS by link
// index, so nothing has to be moved between lanes): two <= KM_BLOCK_MAX-pivot sweeps side by side with the one-row
// broadcasts, instead of one NL-pivot sweep across two rows.  Lanes and columns beyond a block's size carry identity rows.
// The same operations per block in the same order as the full sweep does them (the off-block entries it carries are exact
// zeros), so the result is bitwise the same.
template <int NL, int G>
__device__ __forceinline__ void invert_mass_blocks(Ws<NL>& w, int sub, CReg<NL>& cr, int split, Prof& pf) {
  constexpr int NB = KM_BLOCK_MAX;
  const int row = (threadIdx.x >> 4) & 1, c = threadIdx.x & 15;
  const int base = row ? split : 0, nb = row ? NL - split : split;
  const bool on = c < nb;
  const int li = base + c;
  real loc[NB];
  {
    // unconditional loads at clamped addresses, then selects on the values (conditional loads would each become a branch)
    const int rs = sub < NL ? sub : NL - 1, rl = on ? li : NL - 1;
    real full[NL], blk[NB];
#pragma unroll
    for (int j = 0; j < NL; j++) full[j] = w.Minv[rs][j];
#pragma unroll
    for (int k = 0; k < NB; k++) blk[k] = w.Minv[rl][base + k < NL ? base + k : NL - 1];
#pragma unroll
    for (int j = 0; j < NL; j++) cr.mrow[j] = sub < NL ? full[j] : 0.0;
#pragma unroll
    for (int k = 0; k < NB; k++) loc[k] = (on && k < nb) ? blk[k] : ((!on && k == c) ? 1.0 : 0.0);
  }
  GSYNC();
  pf.ph(39);
  int bad = 0;
  gj_invert_rows<16, NB>(loc, c, bad);
  if (__any(bad)) { const int gb = gor<G>(bad); if (gb && sub == 0) w.bad = 1; }      // (wave-uniform branch; never taken on sane models)
  if (on) {
#pragma unroll
    for (int j = 0; j < NL; j++) w.Minv[li][j] = 0.0;
#pragma unroll
    for (int k = 0; k < NB; k++) if (k < nb) w.Minv[li][base + k] = loc[k];
  }
  GSYNC();
}

template <int NL, int G>
__device__ __forceinline__ void invert_mass(Ws<NL>& w, int sub, CReg<NL>& cr, int split, Prof& pf) {
  if constexpr (G == 32) { if (split) { invert_mass_blocks<NL, G>(w, sub, cr, split, pf); return; } }
  real a[NL];
  if constexpr (G == 16) {                      // (composite_mass_bias_rows wrote both triangles: plain rows, unconditional loads)
    const int rs = sub < NL ? sub : NL - 1;
#pragma unroll
    for (int j = 0; j < NL; j++) a[j] = w.Minv[rs][j];
#pragma unroll
    for (int j = 0; j < NL; j++) a[j] = sub < NL ? a[j] : 0.0;
  } else {
#pragma unroll
    for (int j = 0; j < NL; j++) a[j] = sub < NL ? (j >= sub ? w.Minv[sub][j] : w.Minv[j][sub]) : 0.0;   // columns hold the upper triangle
  }
  GSYNC();
#pragma unroll
  for (int j = 0; j < NL; j++) cr.mrow[j] = a[j];
  int bad = 0;
  gj_invert_rows<G, NL>(a, sub, bad);
  if (bad && sub == 0) w.bad = 1;
  if (sub < NL) {
#pragma unroll
    for (int j = 0; j < NL; j++) w.Minv[sub][j] = a[j];
  }
  GSYNC();
}
