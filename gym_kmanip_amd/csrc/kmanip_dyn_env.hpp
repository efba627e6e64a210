// kmanip_dyn_env.hpp -- one of the phase headers kmanip_dyn_variant.hpp includes (inside the variant namespace) into each per-variant translation unit: step phases, obs / reward, per-env parameters, reset, state load / store, model staging, the entry and the slot rows of the state queries.
#pragma once
// everything mj_step1 computes that mj_step2 needs, at the state held in w.qpos / w.qvel
template <int NL, int G, int SOLVER>
__device__ __forceinline__ void step1_products(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub,
                                               CReg<NL>& cr, real invm, Prof& pf) {
  real kin[15];
  fk_parallel<NL, G>(w, lm, sub, G == 16 ? kin : nullptr);
  pf.ph(0);
  real FN[6];
  // two-row groups with a block split: row r of the group = block r of the robot (lane c <-> link base + c) for the two tree
  // passes; everything else keeps lane = dof
  const int split = G == 32 ? lm.split : 0;
  int bli = -1, bbase = 0;
  if constexpr (G == 32) {
    const int row = (threadIdx.x >> 4) & 1, c = threadIdx.x & 15;
    bbase = row ? split : 0;
    bli = (split && c < (row ? NL - split : split)) ? bbase + c : -1;
    if (split) {                                 // entries between the blocks: never written below, read as part of the rows
      for (int e = sub; e < (int)(sizeof(w.Minv) / sizeof(real)); e += G) (&w.Minv[0][0])[e] = 0.0;      // (the padded rows whole)
    }
  }
  if constexpr (G == 16) bias_bodies_rows<NL, NL>(w, lm, m, sub < NL ? sub : -1, 0, sub == NL, FN, kin);
  else if (split) {
    bias_bodies_rows<NL, KM_BLOCK_MAX>(w, lm, m, bli, bbase, false, FN);
    if (sub == NL) cube_bias<NL>(w, m);          // (lane NL also works on a link of the second block above)
  }
  else bias_bodies_parallel<NL, G>(w, lm, m, sub);
  pf.ph(1);
  collide_parallel<NL, G>(w, lm, m, sub);
  if constexpr (SOLVER != KM_SOLVER_NEWTON) { if (sub == 0) scalar_rows_serial<NL>(w, lm); }
  GSYNC();
  pf.ph(2);
  if constexpr (G == 16) {
    composite_mass_bias_rows<NL, NL>(w, lm, sub < NL ? sub : -1, 0, FN, kin);
  } else if (split) {
    composite_mass_bias_rows<NL, KM_BLOCK_MAX>(w, lm, bli, bbase, FN);
  } else {
    composite_own<NL, G>(w, lm, sub);      // (comp aliases the bias scratch: its last reader is before the barrier above)
    GSYNC();
    composite_accumulate<NL, G>(w, lm, sub);
    GSYNC();
    mass_matrix<NL, G>(w, lm, sub);
    bias_project<NL, G>(w, lm, sub);
  }
  GSYNC();
  pf.ph(3);
  invert_mass<NL, G>(w, sub, cr, lm.split, pf);
  pf.ph(4);
  if constexpr (SOLVER == KM_SOLVER_NEWTON) build_constraints_newton<NL, G>(w, lm, m, sub, cr, invm);
  else build_constraints<NL, G>(w, lm, m, sub, cr, invm);
  pf.ph(5);
}
template <int NL, int G, int SOLVER>
__device__ __forceinline__ real solve(Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub, int actuation,
                                      CReg<NL>& cr, real invm, Prof& pf) {
  if constexpr (SOLVER == KM_SOLVER_NEWTON) return solve_newton<NL, G>(w, lm, m, sub, actuation, cr, invm, pf);
  else {
    real a = solve_accel<NL, G>(w, lm, m, sub, actuation, cr, invm);
    pf.ph(6);
    return a;
  }
}

// mj_Euler: qvel += dt*qacc, then positions with the NEW velocity (semi-implicit); free-joint quaternion
// integrated on the group's lane 0
template <int NL, int G>
__device__ __forceinline__ void integrate(Ws<NL>& w, const KModelDesc* m, int sub, real a) {
  constexpr int NV = Dim<NL>::NV;
  const real dt = m->timestep;
  // (round 6) the lane's velocity / position and the cube's quaternion in one batch; the new angular velocity reaches lane 0 by row
  // broadcast instead of through LDS (one synchronisation and one round trip less in front of the quaternion's serial chain)
  const int sv = sub < NV ? sub : NV - 1, sq = sub < NL + 3 ? sub : NL + 2;
  real v0 = w.qvel[sv], qp = w.qpos[sq], q[4] = {w.qpos[NL + 3], w.qpos[NL + 4], w.qpos[NL + 5], w.qpos[NL + 6]};
  km_pin(v0, qp, q[0], q[1], q[2], q[3]);
  real v = 0;
  if (sub < NV) {
    v = v0 + dt * a;
    w.qvel[sub] = v;
    w.warm[sub] = a;
    if (sub < NL + 3) w.qpos[sub] = qp + dt * v;
  }
  real ax[3] = {gbcast<G, NL + 3>(v), gbcast<G, NL + 4>(v), gbcast<G, NL + 5>(v)};
  if (sub == 0) {
    real ang = dt * normalize3_fast(ax), qr[4], qn[4];
    axis_angle2quat(qr, ax, ang);
    normalize4_fast(q);
    qmul(qn, q, qr);
    normalize4_fast(qn);
    w.qpos[NL + 3] = qn[0]; w.qpos[NL + 4] = qn[1]; w.qpos[NL + 5] = qn[2]; w.qpos[NL + 6] = qn[3];
  }
  GSYNC();
}

// [-1, 1] clip of an observation component
__device__ __forceinline__ real clip1(real x) { return fmin(fmax(x, -1.0), 1.0); }

// get_observation, env_sim.py:110-146 (state keys; cameras are out of this kernel)
template <int NL, int G>
__device__ __forceinline__ void write_obs(const Ws<NL>& w, const LModel<NL>& lm, const KModelDesc* m, int sub, double* obs_row) {
  for (int i = sub; i < NL; i += G) {
    obs_row[i] = clip1((w.qpos[i] - lm.range[i][0]) / (lm.range[i][1] - lm.range[i][0]));
    obs_row[NL + i] = clip1(w.qvel[i] / m->max_q_vel);
  }
  for (int c = sub; c < 7; c += G) {
    if (c < 3) obs_row[2 * NL + c] = clip1((w.qpos[NL + c] - m->cube_spawn_lo[c]) / (m->cube_spawn_hi[c] - m->cube_spawn_lo[c]));
    else obs_row[2 * NL + c] = w.qpos[NL + c];
  }
}

// lo + (hi - lo) * u with the product rounded before the sum: the cube spawn is compared bit-for-bit with the oracle
__device__ __forceinline__ real lerp_unfused(real lo, real hi, real u) {
#pragma clang fp contract(off)
  const real d = hi - lo;
  const real p = d * u;
  return lo + p;
}

#if KM_VAR_PAR
// ---- per-env physics parameters.  ONE evaluation order for every derived constant, restated bit for bit by
// model.py with_env_params (the mass-derived ones without contraction: the host rounds every operation); cornerA / sphA[0] are
// build_lmodel's expressions, evaluated under the same contraction rules it is compiled with.
__device__ __forceinline__ real ep_inertia(const KModelDesc* m, real mass, int k) {
#pragma clang fp contract(off)
  return m->cube_inertia[k] * (mass / m->cube_mass);
}
// cube_invweight0[1] = mean_k 1 / I_k, meaninertia = (trace_robot + 3 m + (I_0 + I_1 + I_2)) / nv (the compiled value while the mass is
// the model's), as invweight0 in model.py sums them
__device__ __forceinline__ void ep_mass_consts(const KDeviceModel* dm, real mass, const real (&I)[3], int nv, real& cw1, real& mi) {
#pragma clang fp contract(off)
  cw1 = ((1.0 / I[0] + 1.0 / I[1]) + 1.0 / I[2]) / 3.0;
  mi = mass == dm->d.cube_mass ? dm->d.meaninertia : ((dm->trace_robot + 3.0 * mass) + ((I[0] + I[1]) + I[2])) / nv;
}
// this lane's cube diagonal of M^-1 (invm) for parameters p
template <int NL>
__device__ __forceinline__ real ep_invm(const KModelDesc* m, const real (&p)[KM_EP_N], int sub) {
  if (sub < NL || sub >= Dim<NL>::NV) return 0;
  return sub < NL + 3 ? 1.0 / p[KM_EP_CUBE_MASS] : 1.0 / ep_inertia(m, p[KM_EP_CUBE_MASS], sub - NL - 3);
}
// Ws::ep from the raw values p (every lane of the group holds the same p; lane 0 writes the scalars, lane s < NSPH sphA[s]).
// The caller synchronises the group before the values are read.
template <int NL>
__device__ __forceinline__ void ep_derive(Ws<NL>& w, const KDeviceModel* dm, const real (&p)[KM_EP_N], int sub) {
  const KModelDesc* m = &dm->d;
  const real mass = p[KM_EP_CUBE_MASS], muc = p[KM_EP_CUBE_FRICTION];
  const real cw = 1.0 / mass;
  if (sub == 0) {
    real I[3] = {ep_inertia(m, mass, 0), ep_inertia(m, mass, 1), ep_inertia(m, mass, 2)}, cw1, mi;
    ep_mass_consts(dm, mass, I, NL + 6, cw1, mi);
#pragma unroll
    for (int k = 0; k < KM_EP_N; k++) w.ep.p[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; k++) w.ep.inertia[k] = I[k];
    w.ep.cubew[0] = cw; w.ep.cubew[1] = cw1;
    w.ep.scale = 1.0 / (mi * (NL + 6));
    w.ep.cornerA = cw + muc * muc * cw;
  }
  if (sub < Dim<NL>::NSPH) {
    const real lw = sub < m->nsphere ? m->body_invweight0[m->sphere_link[sub]][0] : 0.0;
    w.ep.sphA[sub] = (cw + lw) + muc * muc * (cw + lw);
  }
}
// the env's values in force (KDeviceState::envp) -> Ws::ep and the lane's invm
template <int NL>
__device__ __forceinline__ void ep_load(Ws<NL>& w, const KDeviceModel* dm, const KDeviceState& st, int env, int sub, real& invm) {
  real p[KM_EP_N];
#pragma unroll
  for (int k = 0; k < KM_EP_N; k++) p[k] = st.envp[(size_t)k * st.num_envs + env];
  ep_derive<NL>(w, dm, p, sub);
  invm = ep_invm<NL>(&dm->d, p, sub);
}
#endif

// initialize_episode (env_sim.py:23-36) + mj_forward without actuation (dm_control after_reset).  The KM_VAR_PAR build in ranges
// mode first draws the env's parameters for the new episode (written back to KDeviceState::envp; invm follows them).
template <int NL, int G, int SOLVER>
__device__ __forceinline__ void reset_env(Ws<NL>& w, const LModel<NL>& lm, const KDeviceModel* dm, int sub, const KDeviceState& st,
                                          int env, int episode, CReg<NL>& cr, real& invm, Prof& pf) {
  const KModelDesc* m = &dm->d;
  const uint64_t seed = st.seed;
  const int64_t genv = st.env_id_offset + env;
  constexpr int NV = Dim<NL>::NV;
  if (sub < NV) { w.qvel[sub] = 0; w.warm[sub] = 0; }
  if (sub < NL) { w.qpos[sub] = lm.q_home[sub]; w.ctrl[sub] = lm.q_home[sub]; }
  if (sub == 0) {
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t ctr[4] = {(uint32_t)genv, (uint32_t)((uint64_t)genv >> 32), (uint32_t)episode, 0}, o[4];
    philox4x32_10(ctr, key, o);
    real u0 = u53(o[0], o[1]), u1 = u53(o[2], o[3]);
    ctr[3] = 1;
    philox4x32_10(ctr, key, o);
    real u2 = u53(o[0], o[1]);
    w.qpos[NL] = lerp_unfused(m->cube_spawn_lo[0], m->cube_spawn_hi[0], u0);
    w.qpos[NL + 1] = lerp_unfused(m->cube_spawn_lo[1], m->cube_spawn_hi[1], u1);
    w.qpos[NL + 2] = lerp_unfused(m->cube_spawn_lo[2], m->cube_spawn_hi[2], u2);
    for (int c = 0; c < 4; c++) w.qpos[NL + 3 + c] = m->cube_quat0[c];
    w.bad = 0;
  }
#if KM_VAR_PAR
  if (st.ep_range) {
    // p_k = lerp(lo_k, hi_k, u_k), u_k from counter word 3 = KM_EP_CTR3 + k / 2: words (0, 1) of the block for even k, (2, 3) for odd k
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t ctr[4] = {(uint32_t)genv, (uint32_t)((uint64_t)genv >> 32), (uint32_t)episode, KM_EP_CTR3}, o[4], o2[4];
    philox4x32_10(ctr, key, o);
    ctr[3] = KM_EP_CTR3 + 1;
    philox4x32_10(ctr, key, o2);
    const real u[KM_EP_N] = {u53(o[0], o[1]), u53(o[2], o[3]), u53(o2[0], o2[1]), u53(o2[2], o2[3])};
    real p[KM_EP_N];
#pragma unroll
    for (int k = 0; k < KM_EP_N; k++) {
      p[k] = lerp_unfused(st.ep_range[k], st.ep_range[KM_EP_N + k], u[k]);
      if (sub == 0) st.envp[(size_t)k * st.num_envs + env] = p[k];
    }
    ep_derive<NL>(w, dm, p, sub);
    invm = ep_invm<NL>(m, p, sub);
  }
#endif
  GSYNC();
  step1_products<NL, G, SOLVER>(w, lm, m, sub, cr, invm, pf);
  real a = solve<NL, G, SOLVER>(w, lm, m, sub, 0, cr, invm, pf);
  if (sub < NV) w.warm[sub] = a;
  GSYNC();
}

// contact points of slots that never became active are read (and multiplied by zero weights) by the slot-lane solver: give
// them finite values once per launch
template <int NL>
__device__ __forceinline__ void init_ws(Ws<NL>& w, int sub) {
  if (sub < Dim<NL>::NC) { w.c_pos[sub][0] = 0; w.c_pos[sub][1] = 0; w.c_pos[sub][2] = 0; w.c_dist[sub] = 0; }
}
// the env's state -> LDS, with the start of before_step: ctrl <- float32(ctrl) (env_sim.py:40) and qpos_ik <- qpos
template <int NL, int G>
__device__ __forceinline__ void load_state(Ws<NL>& w, const KDeviceState& st, int env, int sub) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  const int NE = st.num_envs;
  // (round 6) every column read of the env's state issued before the first is waited for: as loops, each HBM read was waited for
  // on its own (five to six round trips at the start of every wave)
  constexpr int KQ = (NQ + G - 1) / G, KV = (NV + G - 1) / G, KL = (NL + G - 1) / G;
  real q[KQ], v[KV], wm[KV], c[KL];
#pragma unroll
  for (int k = 0; k < KQ; k++) { const int i = sub + G * k; q[k] = st.qpos[(size_t)(i < NQ ? i : NQ - 1) * NE + env]; }
#pragma unroll
  for (int k = 0; k < KV; k++) { const int i = sub + G * k, ic = i < NV ? i : NV - 1; v[k] = st.qvel[(size_t)ic * NE + env]; wm[k] = st.warm[(size_t)ic * NE + env]; }
#pragma unroll
  for (int k = 0; k < KL; k++) { const int i = sub + G * k; c[k] = st.ctrl[(size_t)(i < NL ? i : NL - 1) * NE + env]; }
#pragma unroll
  for (int k = 0; k < KQ; k++) { const int i = sub + G * k; if (i < NQ) { w.qpos[i] = q[k]; if (i < NL) w.qpos_ik[i] = q[k]; } }
#pragma unroll
  for (int k = 0; k < KV; k++) { const int i = sub + G * k; if (i < NV) { w.qvel[i] = v[k]; w.warm[i] = wm[k]; } }
#pragma unroll
  for (int k = 0; k < KL; k++) { const int i = sub + G * k; if (i < NL) w.ctrl[i] = (real)(float)c[k]; }
  if (sub == 0) { w.bad = 0; w.work = 0; }
}
#if KM_VAR_FRC
// the env's row of KDeviceState::qfrc_applied -> Ws::frc, lane `sub` its own dof's component, once per launch.  Returns nonzero on
// every lane of the group if a component is not finite: the row is then stored as zeros and the caller treats the env as diverged
// before any solver runs (no loop ever iterates on a NaN input).  The caller synchronises the group before Ws::frc is read.
template <int NL, int G>
__device__ __forceinline__ int load_applied(Ws<NL>& w, const KDeviceState& st, int env, int sub) {
  constexpr int NV = Dim<NL>::NV;
  static_assert(NV <= G, "one dof per lane");
  const real f = st.qfrc_applied[(size_t)env * NV + (sub < NV ? sub : NV - 1)];
  const int bad = gor<G>(!isfinite(f));
  if (sub < NV) w.frc[sub] = bad ? 0.0 : f;
  return bad;
}
#endif
template <int NL> struct LdsIO {
  Ws<NL>& w; const KDeviceState& st; int env;
  __device__ __forceinline__ real qpos(int i) const { return w.qpos[i]; }
  __device__ __forceinline__ void set_ctrl(int i, real v) { w.ctrl[i] = v; }
  __device__ __forceinline__ void set_qpos_ik(int i, real v) { w.qpos_ik[i] = v; }
  __device__ __forceinline__ void set_diag(int arm, int nfev, int status) {
    st.ik_nfev[(size_t)arm * st.num_envs + env] = nfev; st.ik_status[(size_t)arm * st.num_envs + env] = status;
  }
};
template <int NL, int G>
__device__ __forceinline__ void store_state(const Ws<NL>& w, const KDeviceState& st, int env, int sub) {
  constexpr int NV = Dim<NL>::NV, NQ = Dim<NL>::NQ;
  const int NE = st.num_envs;
  for (int i = sub; i < NQ; i += G) st.qpos[(size_t)i * NE + env] = w.qpos[i];
  for (int i = sub; i < NV; i += G) { st.qvel[(size_t)i * NE + env] = w.qvel[i]; st.warm[(size_t)i * NE + env] = w.warm[i]; }
  for (int i = sub; i < NL; i += G) st.ctrl[(size_t)i * NE + env] = w.ctrl[i];
}

// per-link constants -> LDS: a flat copy of the image k_prepare_model built at kmanip_create (KDeviceModel::staged), one batch of
// 16-byte loads per lane, then a workgroup barrier (one wave: cheap)
template <int NL>
__device__ __forceinline__ void stage_model(LModel<NL>& lm, const KDeviceModel* dm) {
  static_assert(sizeof(LModel<NL>) % 16 == 0 && sizeof(LModel<NL>) <= KM_LMODEL_MAX, "the staged image is copied in 16-byte pieces");
  constexpr int N16 = (int)(sizeof(LModel<NL>) / 16);
  const uint4* src = reinterpret_cast<const uint4*>(dm->staged);
  uint4* dst = reinterpret_cast<uint4*>(&lm);
  uint4 v[(N16 + 63) / 64];
#pragma unroll
  for (int k = 0; k < (N16 + 63) / 64; k++) { const int i = threadIdx.x + 64 * k; v[k] = src[i < N16 ? i : N16 - 1]; }
#pragma unroll
  for (int k = 0; k < (N16 + 63) / 64; k++) { const int i = threadIdx.x + 64 * k; if (i < N16) dst[i] = v[k]; }
  __syncthreads();
}
// the image itself: per-link constants with all 64 lanes, the derived scalars on lane 0 (k_prepare_model only)
template <int NL>
__device__ __forceinline__ void build_lmodel(LModel<NL>& lm, const KDeviceModel* dm) {
  const KModelDesc* m = &dm->d;
  for (int i = threadIdx.x; i < NL; i += 64) {
    lm.parent[i] = m->link_parent[i]; lm.jtype[i] = m->jnt_type[i]; lm.forcelimited[i] = m->forcelimited[i];
    lm.anc[i] = dm->x.anc_mask[i]; lm.desc[i] = dm->x.desc_mask[i];
    for (int k = 0; k < 4; k++) lm.jump[k][i] = dm->x.jump[k][i];
    if (i == 0) {
      lm.fk_rounds = dm->x.fk_rounds; lm.split = dm->x.split;
      get_kb(m, m->con_def_solref, m->con_def_solimp, lm.kb[0][0], lm.kb[0][1]);
      get_kb(m, m->con_cube_solref, m->con_cube_solimp, lm.kb[1][0], lm.kb[1][1]);
      lm.imp0[0] = impedance(m->con_def_solimp, 0.0);
      lm.imp0[1] = impedance(m->con_cube_solimp, 0.0);
      stage_imp(lm.imp[0], m->con_def_solimp); stage_imp(lm.imp[1], m->con_cube_solimp);
      lm.cubew[0] = m->cube_invweight0[0]; lm.cubew[1] = m->cube_invweight0[1];
      lm.fric[0][0] = m->con_def_friction[0]; lm.fric[0][1] = m->con_def_friction[1];
      lm.fric[1][0] = m->con_cube_friction[0]; lm.fric[1][1] = m->con_cube_friction[1];
      lm.scale = 1.0 / (m->meaninertia * (NL + 6));
      const real muc = m->con_cube_friction[0], mud = m->con_def_friction[0], cw = m->cube_invweight0[0];
      lm.cornerA = cw + muc * muc * cw;
      for (int sp = 0; sp < Dim<NL>::NSPH; sp++) {
        const real lw = sp < m->nsphere ? m->body_invweight0[m->sphere_link[sp]][0] : 0.0;
        lm.sphA[0][sp] = (cw + lw) + muc * muc * (cw + lw);
        lm.sphA[1][sp] = lw + mud * mud * lw;
      }
    }
    if (i < Dim<NL>::NSPH) {           // (NSPH <= NL)
      const int sp = i < m->nsphere ? i : 0;          // (unused candidates: finite copies, never tested)
      lm.sph_link[i] = m->sphere_link[sp]; lm.sph_rad[i] = m->sphere_radius[sp];
      for (int c = 0; c < 3; c++) { lm.sph_pos[i][c] = m->sphere_pos[sp][c]; lm.sph_seg[i][c] = m->sphere_seg[sp][c]; }
      if (i == 0) lm.nsph = m->nsphere < Dim<NL>::NSPH ? m->nsphere : Dim<NL>::NSPH;
    }
    lm.dofw[i] = m->dof_invweight0[i];
    lm.floss[i] = m->frictionloss[i]; lm.kp[i] = m->kp[i]; lm.mass[i] = m->mass[i]; lm.q_home[i] = m->q_home[i];
    for (int c = 0; c < 3; c++) { lm.pos[i][c] = m->link_pos[i][c]; lm.jaxis[i][c] = m->jnt_axis[i][c]; lm.com[i][c] = m->com[i][c]; lm.inertia[i][c] = m->inertia[i][c]; }
    for (int c = 0; c < 4; c++) lm.quat[i][c] = m->link_quat[i][c];
    { real qn[4] = {m->link_quat[i][0], m->link_quat[i][1], m->link_quat[i][2], m->link_quat[i][3]}, Rm[9]; normalize4(qn); quat2mat(Rm, qn); for (int c = 0; c < 9; c++) lm.R[i][c] = Rm[c]; }
    for (int c = 0; c < 2; c++) { lm.range[i][c] = m->jnt_range[i][c]; lm.ctrlrange[i][c] = m->ctrlrange[i][c]; lm.forcerange[i][c] = m->forcerange[i][c]; }
  }
  __syncthreads();
}

// get_reward, env_sim.py:148-179, from the kinematics and contacts of a trailing mj_step1 (fk_parallel + collide_parallel)
template <int NL, int G>
__device__ __forceinline__ real env_reward(Ws<NL>& w, const KModelDesc* m, int sub) {
  constexpr int NV = Dim<NL>::NV;
  real v2 = gsum<G>(sub < NV ? w.qvel[sub] * w.qvel[sub] : 0.0);
  GSYNC();
  real rew = -m->reward_vel_penalty * km_sqrt(v2);
  for (int arm = 1; arm >= 0; arm--) {
    if (!m->arm_present[arm] || !m->arm_has_grip[arm]) continue;
    const int l = m->arm_site_link[arm];
    real so[3] = {m->arm_site_pos[arm][0], m->arm_site_pos[arm][1], m->arm_site_pos[arm][2]}, sp[3];
    mat_vec3(sp, w.k.xmat[l], so);
    real df[3] = {w.qpos[NL] - (sp[0] + w.k.xpos[l][0]), w.qpos[NL + 1] - (sp[1] + w.k.xpos[l][1]), w.qpos[NL + 2] - (sp[2] + w.k.xpos[l][2])};
    rew += m->reward_grip_dist * (1.0 / (km_sqrt(dot3(df, df)) + m->epsilon));
  }
  if (m->touch_reward_enabled && (w.contact_mask & KM_CON_FINGERS_CUBE(NL))) {      // a FINGER on the cube (palm / link spheres do not count)
    rew += m->reward_touch_cube;
    if (!w.touch_ct) rew += m->reward_lift_cube;
  }
  return rew;
}

// ---- the state queries (k_observe, kmanip_forces.hip, kmanip_kinematics.hip, kmanip_inverse.hip) and what k_step / k_reset share with them
// this lane's diagonal of M^-1 for the cube dof it owns (0 on every other lane), from the model's values ...
template <int NL>
__device__ __forceinline__ real cube_invm(const KModelDesc* m, int sub) {
  real invm = 0;
  if (sub >= NL && sub < Dim<NL>::NV) invm = sub < NL + 3 ? 1.0 / m->cube_mass : 1.0 / m->cube_inertia[sub - NL - 3];
  return invm;
}
// ... or, KM_VAR_PAR builds, from the env's own, staged into Ws::ep with it
template <int NL>
__device__ __forceinline__ void env_invm(Ws<NL>& w, const KDeviceModel* dm, const KDeviceState& st, int env, int sub, real& invm) {
#if KM_VAR_PAR
  ep_load<NL>(w, dm, st, env, sub, invm);
#else
  invm = cube_invm<NL>(&dm->d, sub);
#endif
}
// A non-finite loaded state, or a further reason `lb` of this lane's: the same flag on every lane of the group.  k_step reports such
// an env as diverged; a query gives status 1 and computes nothing (the kinematics of a non-finite state are garbage).
template <int NL, int G>
__device__ __forceinline__ int state_nonfinite(const Ws<NL>& w, int sub, int lb = 0) {
  for (int i = sub; i < Dim<NL>::NQ; i += G) lb |= !isfinite(w.qpos[i]);
  for (int i = sub; i < Dim<NL>::NV; i += G) lb |= !isfinite(w.qvel[i]);
  return gor<G>(lb);
}
// The entry of a query kernel, 64 / G envs per single-wave workgroup, in two parts around the exit of a group without an env (the
// kernel's own return: the whole group exits together).  query_env: the model staged (every lane: it ends in a workgroup barrier),
// lane group -> env behind the XCD-aware block mapping; false = no env.
template <int NL, int EPB>
__device__ __forceinline__ bool query_env(LModel<NL>& lm, const KDeviceModel* dm, const KDeviceState& st, int grp, int& env) {
  stage_model<NL>(lm, dm);
  env = xcd_block(blockIdx.x, gridDim.x) * EPB + grp;
  return grp < EPB && env < st.num_envs;
}
// query_load: the workspace initialised, the env's parameters (invm) and its state loaded (load_state: with float32(ctrl)).  The
// caller synchronises the group (GSYNC) before it reads the state.  (k_inverse spells the three calls out: it requests the
// caller's row between them.)
template <int NL, int G>
__device__ __forceinline__ void query_load(Ws<NL>& w, const KDeviceModel* dm, const KDeviceState& st, int env, int sub, real& invm) {
  init_ws<NL>(w, sub);
  env_invm<NL>(w, dm, st, env, sub, invm);
  load_state<NL, G>(w, st, env, sub);
}
// which KM_CON_* bit sits in contact slot c (< NC), -1 = none: corner slots hold the penetrating corners in corner order (the mask's
// low byte has exactly the kept ones), sphere slots name their sphere (sph = Ws::slot_sph of the slot)
template <int NL>
__device__ __forceinline__ int slot_contact_bit(int c, uint32_t act, uint32_t mask, int sph) {
  int bit = -1;
  if ((act >> c) & 1u) {
    if (c < 4) {
      uint32_t mm = mask & KM_CON_ANY_CUBE_TABLE;
      for (int k = 0; k < c; k++) mm &= mm - 1u;
      bit = __ffs((int)mm) - 1;
    } else bit = (c < 4 + Dim<NL>::NSS ? 8 : 20) + sph;
  }
  return bit;
}
// one env's slot rows of a query's outputs, lane = slot: the force and the bit and, for KForcesDev, the contact geometry.
// !ok or an empty slot (bit < 0): zeros, bit -1.
template <int NL, class Out>
__device__ __forceinline__ void write_slot_rows(const Out& out, size_t e, int sub, bool ok, const real (&F)[4], int bit,
                                                const real* fr = nullptr, const real* cp = nullptr, real dist = 0) {
  constexpr int NC = Dim<NL>::NC;
  if (sub >= NC) return;
  const size_t s = e * NC + sub;
  const bool on = ok && bit >= 0;
  if (out.contact_force) {
#pragma unroll
    for (int k = 0; k < 4; k++) out.contact_force[s * 4 + k] = on ? F[k] : 0.0;
  }
  if (out.contact_bit) out.contact_bit[s] = on ? bit : -1;
  if constexpr (std::is_same<Out, KForcesDev>::value) {
    if (out.contact_frame) {
#pragma unroll
      for (int k = 0; k < 9; k++) out.contact_frame[s * 9 + k] = on ? fr[k] : 0.0;
    }
    if (out.contact_pos) {
#pragma unroll
      for (int k = 0; k < 3; k++) out.contact_pos[s * 3 + k] = on ? cp[k] : 0.0;
    }
    if (out.contact_dist) out.contact_dist[s] = on ? dist : 0.0;
  }
}
