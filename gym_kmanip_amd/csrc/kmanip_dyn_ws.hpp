// kmanip_dyn_ws.hpp -- one of the phase headers kmanip_dyn_variant.hpp includes (inside the variant namespace) into each per-variant translation unit: per-env workspace (Dim, EnvP, LModel, ConRec, Ws, SlotC, CReg) and the lane-group reductions.
#pragma once
template <int NL> struct Dim {
  static constexpr int NV = NL + 6;
  static constexpr int NQ = NL + 7;
  static constexpr int NS = 2 * NL;               // arm single-dof rows: friction loss (<= nl) + limits (<= nl)
  static constexpr int NSPH = 6 * (NL / 10);      // collision-sphere CANDIDATES, one lane each: per arm two fingers, palm, three joint housings
  static constexpr int NSS = KM_SPHERE_SLOTS(NL); // sphere contacts KEPT per kind and sub-step (the first penetrating ones in sphere order)
  static constexpr int NST = KM_SPHERE_TABLE_SLOTS(NL);   // ... of the sphere-table kind
  static constexpr int NC = 4 + NSS + NST;        // contact SLOTS: 4 cube-table corners, NSS sphere-cube, NST sphere-table
  static constexpr int NCF = NSS + NST;           // slots that involve arm dofs
};
// compile-time kind of contact slot c: 0 = table(plane) - cube corner, 1 = sphere - cube, 2 = table - sphere.  WHICH sphere sits
// in a sphere slot is decided per sub-step by collide_parallel (Ws::slot_sph).
template <int NL> __device__ __forceinline__ constexpr int slot_kind(int c) { return c < 4 ? 0 : (c < 4 + Dim<NL>::NSS ? 1 : 2); }

// One env's physics parameters (KM_EP_*) and the constants derived from them (ep_derive), staged in LDS inside its Ws by the
// KM_VAR_PAR kernels: they replace the wave-uniform reads of the same model quantities (the KM_EP_* accessors below Ws).
template <int NL> struct EnvP {
  real p[KM_EP_N];                // cube mass, cube friction, cube frictionloss, kp scale
  real inertia[3];                // cube_inertia[k] * (mass / cube_mass)
  real cubew[2], scale, cornerA;  // LModel::cubew / scale / cornerA of this env
  real sphA[Dim<NL>::NSPH];       // LModel::sphA[0][*] (sphere on the cube) of this env
};

// Per-link model constants staged in LDS once per workgroup (lane-indexed reads stay on-chip); scalars
// and small fixed arrays are read straight from the global KModelDesc with wave-uniform (scalar) loads.
template <int NL>
struct alignas(16) LModel {
  int parent[NL], jtype[NL], forcelimited[NL];
  uint32_t anc[NL], desc[NL];
  int jump[4][NL], fk_rounds, split;
  real pos[NL][3], quat[NL][4], jaxis[NL][3], range[NL][2], floss[NL], kp[NL], ctrlrange[NL][2], forcerange[NL][2];
  real mass[NL], com[NL][3], inertia[NL][3], q_home[NL];
  real R[NL][9];        // constant rotation of each link in its parent (from link_quat)
  // soft-constraint constants of the two parameter sets (0 = default pairs / joint rows, 1 = pairs with the cube):
  // stiffness k, damping b (mj_makeImpedance / solref), impedance at zero distance
  real kb[2][2], imp0[2];
  // MuJoCo's qpos0-time constants (mj_setConst): efc_diagApprox of this link's single-dof rows (dof_invweight0), of the
  // FIRST pyramid edge of every contact pair (tran + mu^2 tran, tran = summed body_invweight0 of the pair: cornerA for a
  // cube corner on the table, sphA[0][s] for sphere s on the cube, sphA[1][s] for sphere s on the table), of the cube's
  // friction-loss rows (linear, angular), and the solvers' termination scale 1 / (meaninertia * nv)
  real dofw[NL], sphA[2][Dim<NL>::NSPH], cornerA, cubew[2], scale;
  // solimp of the two parameter sets, clamped like mj_makeImpedance clamps it, with the reciprocals the spline divides by
  // (mode 0: constant (d0 + dw) / 2; 1: linear; 2: MuJoCo's default quadratic spline)
  struct Imp { real d0, dw, iw, mid, imid, i1mid; int mode; } imp[2];
  // collision candidates (round 6): link, centre, radius and capsule segment of sphere s were per-lane GLOBAL loads in every
  // sub-step's narrow phase (and the link again, behind an LDS load, for every active sphere slot of the constraint assembly)
  real fric[2][2];      // (tangential, torsional) friction of pairs without / with the cube (con_def_friction, con_cube_friction)
  int sph_link[Dim<NL>::NSPH > 0 ? Dim<NL>::NSPH : 1], nsph;
  real sph_pos[Dim<NL>::NSPH > 0 ? Dim<NL>::NSPH : 1][3], sph_rad[Dim<NL>::NSPH > 0 ? Dim<NL>::NSPH : 1], sph_seg[Dim<NL>::NSPH > 0 ? Dim<NL>::NSPH : 1][3];
};

// friction coefficient k (0, 1: tangential, 2: torsional) of contact slot kind `kind`: pairs with the cube use the mixed cube
// parameters, finger-table pairs MuJoCo's defaults -- wave-uniform model scalars, not worth a slot in the LDS records
__device__ __forceinline__ real slot_mu(const KModelDesc* m, int kind, int k) {
  const real* fr = kind != 2 ? m->con_cube_friction : m->con_def_friction;
  return k < 2 ? fr[0] : fr[1];
}
// Solver view of one pyramidal contact (group-uniform scalars).  Basis index 0 = normal, 1..2 = tangents,
// 3 = torsion.  Edge e = 2*(k-1) + s uses J_0 + sm J_k with sm = (s ? -mu[k-1] : mu[k-1]).
struct ConRec {
  real mu[3];
  real R;          // regulariser shared by all edges (MuJoCo pyramidal rule)
  real D;          // 1 / R
  real inv[6];     // 1 / (A_ee + R); 0 for the unused edges of a condim-3 pair
  real den[6];     // A_ee + R
  real aref[6];    // reference acceleration of the edge
  real f[6];       // edge forces
};

// doubles of padding at the end of Ws (see the note on row strides in it); the KM_VAR_FRC builds' Ws::frc is 16 doubles = 128 bytes for
// the 10-link model, so their padding moves by 16 doubles to keep consecutive envs 128 bytes apart modulo the bank row
#define KM_WS_PAD(NL) ((NL) <= 10 ? (KM_VAR_PAR ? (KM_VAR_FRC ? 8 : 24) : (KM_VAR_FRC ? 25 : 9)) : 1)
template <int NL>
struct Ws {
  static constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ, NS = Dim<NL>::NS, NC = Dim<NL>::NC;
  real qpos[NQ], qvel[NV], ctrl[NL], warm[NV], qpos_ik[NL];
  union {
    // kinematics: live from fk() to the end of the contact-Jacobian build ...
    struct { real xpos[NL][3], xmat[NL][9], axis[NL][3], cpos[NL][3], cube_mat[9]; } k;
#if KM_VAR_SOLVER == KM_SOLVER_PGS
    // ... then the same bytes hold the per-edge Gram rows Ge[c][e][l] = J_l . M^-1 (J_0 + sm J_k)^T for PGS
    struct { real Ge[NC][6][4]; } p;
#endif
  };
  // Row strides of everything a lane reads or writes at [its index][k] are ODD numbers of doubles (round 5): ds_write_b64 banks
  // are (a / 4) mod 32 inside each 16-lane group and ds_read_b64 banks (a / 4) mod 64 inside each 32-lane half, so a stride of 10
  // (or 6) doubles puts lanes i and i + 8 of an env on one bank; and sizeof(Ws<10>) is 128 mod 256 bytes, which puts the two envs
  // of a 32-lane half on opposite halves of the bank row for every odd-stride and unit-stride access (KM_WS_PAD below).
  real Minv[NL][NL | 1];   // joint-space inertia, overwritten by its inverse
  union {
    struct { union { real bsc[NL][9]; real comp[NL][11]; }; real FN[NL][7]; } f;   // bias-pass scratch | composite inertias (10 used); bias wrenches (6 used)
#if KM_VAR_SOLVER == KM_SOLVER_PGS
    real stage[4][NV];                               // staging of basis rows for B = M^-1 J^T
    ConRec rec[NC];                                  // solver records (built last; Newton keeps a slot's constants in its lane)
#endif
  };
  real bias[NV], tmp[NV];
#if KM_VAR_SOLVER == KM_SOLVER_PGS
  real as[NV], tmp2[NV], tmp3[NV];
#endif
  int ns, bad, touch_ct;
  int work;                // Newton iterations of this control step, weighted by kind (KM_WORK_*): the cost predictor of k_sort_envs
  uint32_t contact_mask;   // KM_CON_* bits (which candidate pairs touch)
  uint32_t cact;           // active contact slots
  // single-dof constraint rows on ARM dofs (friction loss, then limits); the cube's friction-loss rows are
  // lane-local registers
#if KM_VAR_SOLVER == KM_SOLVER_PGS
  int s_dof[NS], s_type[NS], s_quad[NS];
  real s_sign[NS], s_pos[NS], s_f[NS], s_R[NS], s_aref[NS], s_den[NS], s_inv[NS], s_floss[NS];
#endif
#if KM_VAR_SOLVER == 1      // (Newton; the enum constants are not visible to the preprocessor)
  // the Cholesky factor of a one-row Newton system on its way from row-per-lane to column-per-lane (rows padded to an odd
  // number of doubles: the lanes' row writes then fall into different banks)
  real LT[NL <= 10 ? NL + 6 : 1][(NL <= 10 ? NL + 6 : 1) + 1];     // (one-row groups only)
#endif
  // contact geometry per slot
  real c_pos[NC][3], c_frame[NC][9], c_dist[NC];
  int slot_sph[NC];        // sphere index held by each active sphere slot (4..NC-1)
  uint32_t slot_anc[NC];   // ... and the ancestor mask of that sphere's link (round 6: the constraint assembly read it through two more dependent loads)
#if KM_VAR_PAR
  EnvP<NL> ep;             // this env's physics parameters (per env, never per wave slot)
#endif
#if KM_VAR_FRC
  real frc[NV];            // this env's row of KDeviceState::qfrc_applied (load_applied: once per launch; zeros if a component is not finite)
#endif
  real pad_[KM_WS_PAD(NL)];
};
static_assert(KM_VAR_NL != 10 || KM_VAR_SOLVER != 1 || sizeof(Ws<KM_VAR_NL>) % 256 == 128, "Ws<10>: consecutive envs 128 bytes apart modulo the 256-byte bank row");

// The model quantities an env's parameters change, as the kernels read them: the wave-uniform model values in the default build,
// the env's own (Ws::ep) in the KM_VAR_PAR build.
#if KM_VAR_PAR
#define KM_EP_MASS(w, m) ((w).ep.p[KM_EP_CUBE_MASS])
#define KM_EP_INERTIA(w, m, k) ((w).ep.inertia[k])
#define KM_EP_FLOSS(w, m) ((w).ep.p[KM_EP_CUBE_FRICTIONLOSS])
#define KM_EP_MU(w, m) ((w).ep.p[KM_EP_CUBE_FRICTION])
#define KM_EP_FRIC_T(w, lm, pset) ((pset) ? (w).ep.p[KM_EP_CUBE_FRICTION] : (lm).fric[0][0])
#define KM_EP_KP(w, lm, i) ((lm).kp[i] * (w).ep.p[KM_EP_KP_SCALE])
#define KM_EP_CUBEW(w, lm, k) ((w).ep.cubew[k])
#define KM_EP_SCALE(w, lm) ((w).ep.scale)
#define KM_EP_SLOT_A(w, lm, kind, sp) ((kind) == 0 ? (w).ep.cornerA : ((kind) == 2 ? (lm).sphA[1][sp] : (w).ep.sphA[sp]))
#else
#define KM_EP_MASS(w, m) ((m)->cube_mass)
#define KM_EP_INERTIA(w, m, k) ((m)->cube_inertia[k])
#define KM_EP_FLOSS(w, m) ((m)->cube_frictionloss)
#define KM_EP_MU(w, m) ((m)->con_cube_friction[0])
#define KM_EP_FRIC_T(w, lm, pset) ((lm).fric[pset][0])
#define KM_EP_KP(w, lm, i) ((lm).kp[i])
#define KM_EP_CUBEW(w, lm, k) ((lm).cubew[k])
#define KM_EP_SCALE(w, lm) ((lm).scale)
#define KM_EP_SLOT_A(w, lm, kind, sp) ((kind) == 0 ? (lm).cornerA : (lm).sphA[(kind) == 2][sp])
#endif

// One-row groups (round 3): lane c < NC OWNS contact slot c for the Newton solve -- its regulariser, friction coefficients and
// reference offsets live in that lane's registers, the slot's pyramid edges are evaluated there (all slots at once, one per
// lane), and what the other lanes need (four force components, seven Hessian weights) reaches them as row broadcasts folded
// into their FMAs.  Round 2 spread the EDGES over the lanes and exchanged projections and forces through LDS records /
// per-slot broadcasts, every lane redoing each slot's scalar arithmetic.
// x_e = (u_0 - A_0) +- mu_k (u_k - A_k), u = J_c a: A_0 = -b v_0 - k imp dist, A_k = -b v_k (v = J_c qvel).
struct SlotC {
  real D, D3;        // 1 / R of the slot's edges and of its torsion pair (0: condim-3 pair / inactive slot / lane owns no slot)
  real mu, mu3;      // tangential / torsional friction coefficient
  real A[4];
};

// this lane's column of every contact basis: J (jb) and M^-1 J^T (bb); compile-time indexed only
// (bb only for the slots that involve arm dofs: for table-cube slots M^-1 is diagonal, bb = jb * invm)
// Newton path only: mrow = this lane's row of the arm inertia M; the lane's OWN single-dof constraint rows
// (dof `sub`: friction loss and, when violated, its joint limit) -- no row tables in LDS.
template <int NL> struct CReg {
  real jb[Dim<NL>::NC][4];
  real bb[Dim<NL>::NCF][4];
  real mrow[NL];
  real fl, Rf, Df, areff;    // friction-loss row x = a - areff          (fl = 0: no row); Df = 1 / Rf
  real sg, Rl, Dl, arefl;    // limit row         x = sg * a - arefl     (sg = 0: no row); Dl = 1 / Rl
  SlotC sc;                  // one-row groups: the contact slot this lane owns
  // Newton path (round 6): the cube's rotation and this lane's corner contact point relative to the cube centre, fetched once per
  // sub-step by the constraint assembly -- every projection J_c v of the table-cube slots (two per start evaluation, one per Newton
  // iteration) re-read all twelve from LDS
  real cm[9], pr[3];
};

#define GSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// sum over the G lanes of a group, result identical (bitwise) in every lane.  16-lane rows use four DPP
// steps (row_mirror, row_half_mirror, two quad_perms) instead of ds_bpermute; G = 32 adds one swizzle.
// The additions below must NOT be contracted with a multiply in the caller's argument (gsum(x * y)): lane i would add
// the exact product to its partner's ROUNDED one and the lanes of a group would no longer hold the bitwise-identical
// sum -- which group-uniform control flow (line-search breaks, termination tests) relies on.  Contraction needs the
// `contract` flag on both operations, so switching it off for this body is enough.
template <int G> __device__ __forceinline__ real gsum(real v) {
#pragma clang fp contract(off)
  static_assert(G == 16 || G == 32, "lane group must be one or two DPP rows");
  v += dpp_f64<0x140>(v);   // row_mirror:      i <-> 15 - i
  v += dpp_f64<0x141>(v);   // row_half_mirror: i <-> 7 - i within each half row
  v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  if (G == 32) {
    const BSrc<32> r = bsrc<32>(v);                  // even-row sum and odd-row sum, each in both rows (v_permlane16_swap)
    v = r.e + r.o;                                   // same operands in the same order on every lane
  }
  return v;
}
// N group sums at once, step by step: the SAME operations per value as N gsum calls (bitwise the same results), but the chains
// interleave -- with one wave per SIMD a lone chain waits out every add's latency and the two wait states in front of each DPP read
template <int G, int N> __device__ __forceinline__ void gsum_n(real (&v)[N]) {
#pragma clang fp contract(off)
  static_assert(G == 16 || G == 32, "lane group must be one or two DPP rows");
  real t[N];
#pragma unroll
  for (int i = 0; i < N; i++) t[i] = dpp_f64<0x140>(v[i]);
#pragma unroll
  for (int i = 0; i < N; i++) v[i] += t[i];
#pragma unroll
  for (int i = 0; i < N; i++) t[i] = dpp_f64<0x141>(v[i]);
#pragma unroll
  for (int i = 0; i < N; i++) v[i] += t[i];
#pragma unroll
  for (int i = 0; i < N; i++) t[i] = dpp_f64<0xB1>(v[i]);
#pragma unroll
  for (int i = 0; i < N; i++) v[i] += t[i];
#pragma unroll
  for (int i = 0; i < N; i++) t[i] = dpp_f64<0x4E>(v[i]);
#pragma unroll
  for (int i = 0; i < N; i++) v[i] += t[i];
  if (G == 32) {
#pragma unroll
    for (int i = 0; i < N; i++) { const BSrc<32> r = bsrc<32>(v[i]); v[i] = r.e + r.o; }
  }
}
// OR over the G lanes of a group, every lane receiving it: the same four DPP steps as gsum (round 3; round 2 went through
// four or five dependent ds_bpermute round trips -- 12 of them per sub-step for the contact masks and the divergence flag)
template <int CTRL> __device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int G> __device__ __forceinline__ int gor(int v) {
  static_assert(G == 16 || G == 32, "lane group must be one or two DPP rows");
  v |= dpp_i32<0x140>(v);   // row_mirror
  v |= dpp_i32<0x141>(v);   // row_half_mirror
  v |= dpp_i32<0xB1>(v);    // quad_perm [1,0,3,2]
  v |= dpp_i32<0x4E>(v);    // quad_perm [2,3,0,1]
  if constexpr (G == 32) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    v = (int)(r[0] | r[1]);
  }
  return v;
}
