// kmanip_api.hip -- host side of the C ABI declared in include/kmanip.h.
// Owns the device model, the struct-of-arrays env state and the launch sequence of one control step: ONE k_step launch
//   (before_step's decode + IK, physics, reward, obs, done, auto-reset), preceded by k_sort_envs when the cost sort is on.
//   No CPU fallback exists: every entry point fails loudly without a HIP device.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "kmanip_device.hpp"

#define KM_VERSION "kmanip-hip 0.40 (gfx950, f64)"

static thread_local std::string g_create_error;

struct KHandle_ {
  KModelDesc desc;
  KDeviceModel* dmodel = nullptr;
  KDeviceState st{};
  int device = 0;
  int num_envs = 0;
  std::string err;
  std::vector<hipEvent_t> ev;   // 3 events per timed step: before k_step, after k_step, after the render
  std::vector<char> ev_render;  // the step rendered in the step (its third event was recorded)
  bool timing = false;
  int timing_every = 1;         // events around every timing_every-th step (the argument of kmanip_enable_timing)
  long timing_count = 0;
  double* rd_rec[2] = {nullptr, nullptr};   // kmanip_bind_reward_done_record: the two record buffers
  int rd_sel = 0;                           // kmanip_select_reward_done_record: the one the next kmanip_step fills
  int timed_steps = 0;
  double* qpos_snap[2] = {nullptr, nullptr};   // kmanip_snapshot_render_state: copies of qpos the renders can read instead of the live state
  int render_src = -1;                         // kmanip_set_render_source: -1 = live state, 0 / 1 = that snapshot
  bool last_step_timed = false; // the last kmanip_step recorded its events (the ring was not full): a render that follows may add its leg
  // render target bound to the step (BASELINE config 5: "depth render in the step"): kmanip_step then also renders
  int step_cam = -1, step_h = 0, step_w = 0;
  float* step_depth = nullptr;
  int epb_forced = 0;           // KMANIP_EPB = 1 | 2 | 4: envs per wave of the step / reset launches (diagnostics), 0 = km_pick_epb's choice
  // wave slots in predicted-cost order (k_sort_envs) for launches of several residency rounds; KMANIP_COST_SORT=0 / 1 overrides
  int32_t* slot_env = nullptr;
  bool cost_sort = false;
  KCostWeights cost_w{18, 1, 2000, 0, 0, 100};     // work units per: IK evaluation, Newton work unit, collider near the cube; bin width
  uint8_t* spread_flags[2] = {nullptr, nullptr};   // SPREAD (KDeviceState::spread_*): the two flag arrays, rotated by every single-step launch
  unsigned spread_k = 0;
  int last_epb = 0;             // envs per wave of the LAST step launch (a chunk launch always takes the full shape): what the slot -> env maps of kmanip_dbg_wave_clocks are rebuilt with
  // per-env physics parameters (kmanip_set_env_params): allocated by the first call that needs them; st.envp / st.ep_range
  // point at them while explicit values / ranges mode are in force
  double* envp_buf = nullptr;       // [KM_EP_N][N]
  double* ep_range_buf = nullptr;   // lo[KM_EP_N], hi[KM_EP_N]
  int* ep_flag = nullptr;           // validation result of kmanip_set_env_params
  // per-env visual parameters (kmanip_set_visual_params): `vis` is what the render launchers get (all NULL:
  // the default kernels); vis.vp points at vp_buf while explicit values are in force, vis.range at vp_range_buf in ranges mode
  KVisArgs vis{};
  double* vp_buf = nullptr;         // [KM_VP_N][N]
  double* vp_range_buf = nullptr;   // lo[KM_VP_N], hi[KM_VP_N]
  int* vp_flag = nullptr;           // validation result of kmanip_set_visual_params
  int32_t* ep_snap[2] = {nullptr, nullptr};   // the episode counters a snapshot took in ranges mode (a render of that slot draws from them)
  bool ep_snap_ok[2] = {false, false};
  // link capsules of the RGB / label renders (kmanip_set_render_links): the list in force and its device copy,
  // an argument of k_render_links; empty = the default kernels
  std::vector<KLinkCapsule> links;
  KLinkCapsule* links_buf = nullptr;   // [KM_MAX_LINK_CAPSULES], allocated by the first call that sets a list
  // kmanip_set_depth_links: while on AND the list is not empty the depth renders launch k_render_depth_links
  bool depth_links = false;
  // the state on the device (kmanip_get_state_dev / kmanip_set_state_dev / kmanip_copy_envs)
  unsigned long long* index_errors = nullptr;   // index entries outside 0 .. num_envs-1 those calls skipped (kmanip_state_index_errors)
  double* stage_buf = nullptr;                  // staging copy of a same-handle kmanip_copy_envs: [nq + nv + nu + nv + KM_EP_N][stage_cap]
  int32_t* stage_cnt = nullptr;                 //   doubles, then step_idx and episode [2][stage_cap]; allocated by the first such call
  int stage_cap = 0;
  std::vector<void*> allocs;
};

// Every entry point works on the handle's device and leaves the caller's current device as it found it (a
// multi-device process -- e.g. torch with several GPUs -- must not have its current device changed under it).
struct DevGuard {
  int prev = -1;
  bool ok = true;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
  }
  ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define KM_ENTER(h)                                                                         \
  DevGuard dev_guard_((h)->device);                                                         \
  if (!dev_guard_.ok) { (h)->err = "hipSetDevice failed"; return -1; }

// device scratch freed on every exit path
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  template <class T> T* as() const { return (T*)p; }
};

#define HIPCHK(h, call)                                                                     \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
      return (int)e_ ? (int)e_ : -1;                                                        \
    }                                                                                       \
  } while (0)

static int validate(const KModelDesc* d, std::string& err) {
  if (d->ik_max_nfev < 0) { err = "ik_max_nfev must be 0 (the reference's 100 n) or a positive cap"; return -1; }
  if (d->nlink != 10 && d->nlink != 20) { err = "nlink must be 10 or 20 (KManipSoloArm / DualArm / Torso)"; return -1; }
  if (d->nsphere < 0 || d->nsphere > KM_MAX_SPHERES || d->nsphere > 6 * (d->nlink / 10)) { err = "too many collision spheres (at most 6 per 10 links: one collision lane each)"; return -1; }
  for (int s = 0; s < d->nsphere; s++)
    if (d->sphere_link[s] < 0 || d->sphere_link[s] >= d->nlink || !(d->sphere_radius[s] > 0)) { err = "collision sphere on a missing link or with radius <= 0"; return -1; }
  if (d->obs_dim != 2 * d->nlink + 7) { err = "obs_dim != 2*nlink+7"; return -1; }
  // (+-INFINITY is the infinite plane; a NaN bound would pass the depth renderer's min-chain rectangle test)
  if (std::isnan(d->table_rect[0]) || std::isnan(d->table_rect[1]) || std::isnan(d->table_rect[2]) || std::isnan(d->table_rect[3]) ||
      !(d->table_rect[0] <= d->table_rect[1]) || !(d->table_rect[2] <= d->table_rect[3])) { err = "table_rect must be x_lo <= x_hi, y_lo <= y_hi (no NaN; +-INFINITY = infinite plane)"; return -1; }
  if (d->n_sub_steps < 1 || d->solver_iterations < 0) { err = "bad n_sub_steps / solver_iterations"; return -1; }
  for (const double* si : {d->con_def_solimp, d->con_cube_solimp}) {
    const double power = si[4] < 1 ? 1 : si[4];
    if (power != 1 && power != 2) { err = "solimp power must be 1 or 2 (MuJoCo's default is 2; the device impedance spline has no pow)"; return -1; }
  }
  for (int i = 0; i < d->nlink; i++)
    if (d->link_parent[i] >= i || d->link_parent[i] < -1) { err = "links must be ordered parents-first"; return -1; }
  int nik = 0;
  for (int a = 0; a < KM_MAX_ARMS; a++) {
    if (!d->arm_present[a]) continue;
    if (d->arm_nq[a] != 6 && d->arm_nq[a] != 7) { err = "arm_nq must be 6 or 7"; return -1; }
    if (nik && nik != d->arm_nq[a]) { err = "both arms must have the same number of IK unknowns"; return -1; }
    nik = d->arm_nq[a];
  }
  return 0;
}

// ancestor masks and IK chains (derived data, kept out of the ABI struct)
static void h_quat2mat(const double* q, double* m) {
  double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}

static int build_aux(const KModelDesc* d, KModelAux* x, std::string& err) {
  memset(x, 0, sizeof(*x));
  for (int i = 0; i < d->nlink; i++)
    if (d->jnt_axis[i][0] != 0 || d->jnt_axis[i][1] != 0 || d->jnt_axis[i][2] != 1) {
      err = "the IK kernel assumes joint axes along local z (true for every reference model: axis=\"0 0 1\")"; return -1;
    }
  for (int i = 0; i < d->nlink; i++) {
    uint32_t mk = 0;
    for (int j = i; j >= 0; j = d->link_parent[j]) mk |= 1u << j;
    x->anc_mask[i] = mk;
  }
  int depth = 1;
  for (int i = 0; i < d->nlink; i++) {
    int dep = 0;
    for (int j = i; j >= 0; j = d->link_parent[j]) { x->desc_mask[j] |= 1u << i; dep++; }
    if (dep > depth) depth = dep;
    for (int k = 0; k < 4; k++) {
      int a = i;
      for (int t = 0; t < (1 << k) && a >= 0; t++) a = d->link_parent[a];
      x->jump[k][i] = a;
    }
  }
  if (depth > 16) { err = "kinematic tree deeper than 16 links"; return -1; }
  x->fk_rounds = 0;
  while ((1 << x->fk_rounds) < depth) x->fk_rounds++;
  // block split of the joint-space inertia: the most balanced s such that no link >= s has an ancestor < s
  x->split = 0;
  if (!getenv("KMANIP_NO_BLOCK_SPLIT")) {
    int best = d->nlink + 1;
    for (int s = 1; s < d->nlink; s++) {
      bool ok = true;
      for (int i = s; i < d->nlink && ok; i++) ok = (x->anc_mask[i] & ((1u << s) - 1u)) == 0;
      const int big = s > d->nlink - s ? s : d->nlink - s;
      // only the two layouts the device code is written for (its row-per-block paths pick the second block's columns at
      // compile-time offsets 10 or 11): DualArm 10 + 10, Torso 11 + 9.  Any other forest runs the full two-row code (split = 0).
      if (ok && big <= KM_BLOCK_MAX && big < best && (s == 10 || s == 11)) { best = big; x->split = s; }
    }
  }
  if (x->split != 0 && x->split != 10 && x->split != 11) { err = "internal: block split other than 10 / 11"; return -1; }
  for (int i = 0; i < d->nlink; i++) {
    double q[4] = {d->link_quat[i][0], d->link_quat[i][1], d->link_quat[i][2], d->link_quat[i][3]};
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(n > 0)) { err = "zero link quaternion"; return -1; }
    for (int c = 0; c < 4; c++) q[c] /= n;
    h_quat2mat(q, x->link_R[i]);
  }
  for (int c = 0; c < KM_MAX_CAMS; c++) x->cam_tanhalf[c] = d->cam_present[c] ? tan(0.5 * d->cam_fovy[c] * (M_PI / 180.0)) : 1.0;
  for (int s = 0; s < d->nsphere; s++)
    if (d->sphere_visible[s]) {
      if (x->nvis == KM_RENDER_MAXVIS) { err = "the camera renders draw at most 4 visible spheres (the finger tips)"; return -1; }
      x->vis_sphere[x->nvis++] = s;
    }
  for (int a = 0; a < KM_MAX_ARMS; a++) {
    if (!d->arm_present[a]) continue;
    int chain[KM_MAX_LINKS], n = 0;
    for (int j = d->arm_site_link[a]; j >= 0; j = d->link_parent[j]) chain[n++] = j;
    if (n > KM_MAX_CHAIN) { err = "IK chain longer than KM_MAX_CHAIN"; return -1; }
    if (n > d->arm_nq[a] + 1) { err = "at most one fixed joint may follow the IK unknowns on the site's chain"; return -1; }
    x->chain_len[a] = n;
    h_quat2mat(d->arm_site_quat[a], x->site_R[a]);
    for (int k = 0; k < n; k++) {
      int l = chain[n - 1 - k];
      x->chain_link[a][k] = l;
      int xi = -1;
      for (int i = 0; i < d->arm_nq[a]; i++) if (d->arm_q_id[a][i] == l) xi = i;
      x->chain_xidx[a][k] = xi;
      h_quat2mat(d->link_quat[l], x->chain_R[a][k]);
      // the kernels rely on: unknown i sits at chain position i, fixed joints (if any) come after
      if ((k < d->arm_nq[a]) != (xi == k)) { err = "IK mask must be the leading links of the site's chain, in order"; return -1; }
    }
  }
  return 0;
}

// The arm of every sphere (KDeviceModel::sphere_arm; model.py sphere_arm restates it): sphere s belongs to arm a when its link is an
// ancestor-or-self of the arm's site link or of one of its gripper links.  Exactly one arm per sphere in every reference model.
// No desc is refused over this (kmanip_create accepts what it accepted before the labels): a sphere on several chains gets the
// lowest of those arms, one on none gets arm 0, as model.sphere_arm does without strict=True.
static void build_sphere_arm(const KModelDesc* d, uint8_t* out) {
  memset(out, 0, KM_MAX_SPHERES);
  for (int s = 0; s < d->nsphere; s++) {
    int found = -1;
    for (int a = 0; a < KM_MAX_ARMS && found < 0; a++) {
      if (!d->arm_present[a]) continue;
      const int leaf[3] = {d->arm_site_link[a], d->arm_grip_id[a][0], d->arm_grip_id[a][1]};
      bool on = false;
      for (int k = 0; k < 3 && !on; k++)
        for (int j = leaf[k]; j >= 0 && j < d->nlink && !on; j = d->link_parent[j]) on = j == d->sphere_link[s];
      if (on) found = a;
    }
    out[s] = (uint8_t)(found < 0 ? 0 : found);
  }
}

// the row arguments of kmanip_forward / kmanip_rollout / kmanip_feedback / kmanip_kinematics_rows / kmanip_site_cost (`what`; `in_t` / `out_t`: the names of its structs)
template <class In, class Out>
static int row_args(KHandle h, const char* what, const char* in_t, const char* out_t, const In* in, const Out* out, int n) {
  const std::string w = std::string(what) + ": ";
  if (!in) { h->err = w + "the " + in_t + " pointer is NULL"; return -1; }
  if (!out) { h->err = w + "the " + out_t + " pointer is NULL"; return -1; }
  if (n < 0) { h->err = w + "n is negative"; return -1; }
  if (!in->env_index && n > h->st.num_envs) { h->err = w + "more rows than envs need " + in_t + "::env_index"; return -1; }
  return 0;
}
// ... and of the two that step (kmanip_rollout / kmanip_feedback): row_args, then the step counts and the per-step flags
template <class In, class Out>
static int stepped_args(KHandle h, const char* what, const char* in_t, const char* out_t, const In* in, const Out* out, int n, int nstep,
                        int nsub) {
  if (row_args(h, what, in_t, out_t, in, out, n)) return -1;
  const std::string w = std::string(what) + ": ";
  if (nstep < 0) { h->err = w + "nstep is negative"; return -1; }
  if (nsub < 0) { h->err = w + "nsub is negative"; return -1; }
  if (in->ctrl_per_step && !in->ctrl) { h->err = w + "ctrl_per_step is set and " + in_t + "::ctrl is NULL"; return -1; }
  if (in->frc_per_step && !in->qfrc_applied) { h->err = w + "frc_per_step is set and " + in_t + "::qfrc_applied is NULL"; return -1; }
  return 0;
}

extern "C" {

int kmanip_model_desc_size(void) { return (int)sizeof(KModelDesc); }

// ---- per-env physics parameters (include/kmanip.h KM_EP_*)
// robot part of trace(M(qpos0)), in the order model.py with_env_params restates (no contraction: the host rounds every operation)
static double trace_robot_of(const KModelDesc& d) {
#pragma clang fp contract(off)
  const double nv = d.nlink + 6;
  return d.meaninertia * nv - (3.0 * d.cube_mass + ((d.cube_inertia[0] + d.cube_inertia[1]) + d.cube_inertia[2]));
}
// (the limits every parameter value must meet, the ranges' lo and hi as well: ep_value_ok of kmanip_device.hpp)
__global__ void k_ep_validate(const double* __restrict__ p, int n, int* __restrict__ bad) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool ok = true;
    for (int k = 0; k < KM_EP_N; k++) ok = ok && ep_value_ok(k, p[(size_t)k * n + i]);
    if (!ok) atomicOr(bad, 1);
  }
}
__global__ void k_ep_fill(double* __restrict__ p, int n, double v0, double v1, double v2, double v3) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    p[i] = v0; p[(size_t)n + i] = v1; p[2 * (size_t)n + i] = v2; p[3 * (size_t)n + i] = v3;
  }
}
static int ep_grid(int n) { return (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024; }

// ---- per-env visual parameters (include/kmanip.h KM_VP_*)
__host__ __device__ static inline double vp_default(int k) {
  if (k < KM_VP_TABLE_RGB) return k == KM_VP_CUBE_RGB ? 1.0 : 0.0;                 // cube 1 0 0
  if (k < KM_VP_ROBOT_RGB) return 0.2;                                             // table .2 .2 .2
  if (k < KM_VP_BACKGROUND_RGB) return 0.647059;                                   // finger spheres
  if (k < KM_VP_AMBIENT) return 0.0;                                               // background black
  if (k == KM_VP_AMBIENT || k == KM_VP_HEADLIGHT) return 0.4;
  if (k == KM_VP_DIRECTIONAL) return 1.0;
  return 0.0;                                                                      // camera offset
}
// the limits every value must meet (the ranges' lo and hi as well): colours in [0, 1], light terms >= 0, |offset| <= 0.25 m, finite
__host__ __device__ static inline bool vp_value_ok(int k, double v) {
  if (!(v - v == 0.0)) return false;           // NaN or infinite
  if (k < KM_VP_AMBIENT) return v >= 0.0 && v <= 1.0;
  if (k < KM_VP_CAM_OFFSET) return v >= 0.0;
  return v >= -0.25 && v <= 0.25;
}
__global__ void k_vp_validate(const double* __restrict__ p, int n, int* __restrict__ bad) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool ok = true;
    for (int k = 0; k < KM_VP_N; k++) ok = ok && vp_value_ok(k, p[(size_t)k * n + i]);
    if (!ok) atomicOr(bad, 1);
  }
}
__global__ void k_vp_fill_defaults(double* __restrict__ p, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    for (int k = 0; k < KM_VP_N; k++) p[(size_t)k * n + i] = vp_default(k);
}
const char* kmanip_version(void) { return KM_VERSION; }

int kmanip_create(const KModelDesc* desc, int num_envs, int device, uint64_t seed, int64_t env_id_offset, KHandle* out) {
  if (!desc || !out || num_envs <= 0) { g_create_error = "kmanip_create: bad arguments"; return -1; }
  KHandle_* h = new (std::nothrow) KHandle_();
  if (!h) { g_create_error = "out of memory"; return -1; }
  h->desc = *desc;
  h->device = device;
  h->num_envs = num_envs;
  KDeviceModel hm;
  hm.d = *desc;
  if (validate(desc, h->err) != 0 || build_aux(desc, &hm.x, h->err) != 0) { g_create_error = h->err; delete h; return -2; }
  // solver_iterations = 0 means no iteration: qacc is the solver's start point (MuJoCo's `while (iter < opt.iterations)`; the PGS
  // loop's `iter < maxit`).  The Newton loop tests its cap only after an iteration, so a Newton model with a cap of 0 gets an
  // infinite tolerance in the DEVICE copy instead: the loop's entry test (scaled gradient < tolerance) then accepts every start
  // point, of every problem of every kernel that holds the loop, and the kernels themselves stay as they are (a test of the cap
  // inside the loop, one scalar compare, moved the step time by 0.5-1 %: DESIGN.md section 32).  h->desc keeps the caller's value.
  if (desc->solver == KM_SOLVER_NEWTON && desc->solver_iterations == 0) hm.d.solver_tolerance = INFINITY;
  hm.trace_robot = trace_robot_of(*desc);
  build_sphere_arm(desc, hm.sphere_arm);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || device >= ndev) {
    g_create_error = std::string("kmanip_create: no usable HIP device (") + hipGetErrorString(e) + "); this library has no CPU path";
    delete h; return -3;
  }
#define CR(call) do { hipError_t e2 = (call); if (e2 != hipSuccess) { g_create_error = std::string(#call) + ": " + hipGetErrorString(e2); kmanip_destroy(h); return -4; } } while (0)
  DevGuard dev_guard_(device);
  if (!dev_guard_.ok) { g_create_error = "kmanip_create: hipSetDevice failed"; delete h; return -4; }
  const int nl = desc->nlink, nv = nl + 6, nq = nl + 7;
  const size_t N = (size_t)num_envs;
  auto dalloc = [&](void** p, size_t bytes) -> hipError_t {
    hipError_t r = hipMalloc(p, bytes);
    if (r == hipSuccess) { h->allocs.push_back(*p); r = hipMemset(*p, 0, bytes); }
    return r;
  };
  CR(dalloc((void**)&h->dmodel, sizeof(KDeviceModel)));
  CR(hipMemcpy(h->dmodel, &hm, sizeof(KDeviceModel), hipMemcpyHostToDevice));
  kmanip_launch_prepare_model(h->dmodel, *desc, nullptr);       // the kernels' LDS image of the model constants, built once (KDeviceModel::staged)
  CR(hipGetLastError());
  CR(dalloc((void**)&h->st.qpos, sizeof(double) * nq * N));
  CR(dalloc((void**)&h->st.qvel, sizeof(double) * nv * N));
  CR(dalloc((void**)&h->st.ctrl, sizeof(double) * nl * N));
  CR(dalloc((void**)&h->st.warm, sizeof(double) * nv * N));
  CR(dalloc((void**)&h->st.step_idx, sizeof(int32_t) * N));
  CR(dalloc((void**)&h->st.episode, sizeof(int32_t) * N));
  CR(dalloc((void**)&h->st.contact_mask, sizeof(uint32_t) * N));
  CR(dalloc((void**)&h->st.ik_nfev, sizeof(int32_t) * 2 * N));
  CR(dalloc((void**)&h->st.ik_status, sizeof(int32_t) * 2 * N));
  // episode counter starts at -1 so that the first reset is episode 0 (matches the oracle's ko_reset(..., 0))
  CR(hipMemset(h->st.episode, 0xFF, sizeof(int32_t) * N));
  h->st.num_envs = num_envs;
  h->st.env_id_offset = env_id_offset;
  h->st.seed = seed;
  h->st.sim_time = nullptr;
  h->st.rd_rec = nullptr;
  h->st.control_dt = desc->n_sub_steps * desc->timestep;
  if (const char* e = getenv("KMANIP_EPB")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) h->epb_forced = v; }
  h->st.slot_env = nullptr;
  h->st.wave_clk = nullptr;
  h->st.spread_in = nullptr; h->st.spread_out = nullptr;
  // "near the cube": what flags an env heavy (SPREAD) / sets the sort's proximity bit (k_sort_envs).  Swept on one box
  // (profiles/r05_near_margin.txt): the single-arm launch is best at 1.5 cm (7.18 M; 1 cm 7.17, 2.5 cm 7.14, 0 = in contact only 7.01);
  // the two-arm sort at 2.5-3 cm on the DualArm (3.91 -> 3.97 M) and flat on the Torso (4.86 / 4.85 / 4.83 M at 1.5 / 2.5 / 4 cm)
  h->st.near_margin = nl > 10 ? 0.025 : 0.015;
  {
    // more waves than SIMD slots (1024) at two envs per wave: the two-arm models (their kernels carry the work counters the
    // order is predicted from; the single-arm kernel ships without them -- KMANIP_COST_SORT=1 still sorts it by its IK counts)
    h->cost_sort = nl > 10 && num_envs > 2048;
    if (const char* e = getenv("KMANIP_COST_SORT")) h->cost_sort = e[0] == '1';
  }
  {
    // Which envs share a wave (the single-arm Newton kernel at widths whose launch is about one residency round of multi-env waves).
    // Every step notes which envs end it with a collider on or within 1.5 cm of the cube ("heavy": 12 % of the envs, 99 % of the
    // next step's coupled ones); the next launch uses that to choose its wave-mates.  An env's bits do not depend on its slot or
    // its wave-mates (tests), so this is scheduling only.
    //  * SPREAD (default at >= 2048 envs: two or four envs per wave; KMANIP_SPREAD=0 turns it off): flags, one byte per env
    //    (KDeviceState::spread_*: bit 0 heavy; bits 1-2 a cost score of the others: a cube that does not rest on four corners, a
    //    sphere on the table).  A wave reads the 64 flags of its block of 64 consecutive envs (three ballots) and the block's waves
    //    deal its envs out (spread_pick): the j-th heavy env to lane group 0 of wave j, so that no wave holds two heavy ones (a wave
    //    with two coupled envs runs the joint loop for the longer of their iteration counts: those waves ended the launches); the
    //    others in ascending score order, so that the heavy waves' other groups take the block's plainest envs and envs of a kind
    //    sit together in the later waves.  k_step 0.5896 -> 0.5690 ms at 4096 envs (heavy-only flags 0.5751, + table bit 0.5716),
    //    0.5361 -> 0.5302 ms at 2048 (profiles/r05_spread_dispatch.txt).  A permutation INSIDE each block whatever the flags
    //    say: the cache lines a block touches are those of the identity map (a first version dealt from launch-wide lists filled by
    //    atomics in completion order: 0.5853 ms, HBM traffic 5.6 -> 17 MB a launch; a heavy-first dispatch with a wave to each heavy
    //    env lost too: DESIGN.md 3.2).
    //  * the cost sort (above) or KMANIP_SPREAD=0: the sorted slot order (a map of its own) / the identity map.
    const bool single_newton = nl == 10 && desc->solver == KM_SOLVER_NEWTON;
    bool spread = single_newton && num_envs >= 2048 && num_envs % 64 == 0 && !h->cost_sort;
    if (const char* e = getenv("KMANIP_SPREAD")) spread = spread && e[0] == '1';
    if (spread) for (int t = 0; t < 2; t++) CR(dalloc((void**)&h->spread_flags[t], (size_t)num_envs));
  }
  if (const char* e = getenv("KMANIP_WAVE_CLOCKS")) if (e[0] == '1') CR(dalloc((void**)&h->st.wave_clk, sizeof(unsigned long long) * N));
  CR(dalloc((void**)&h->slot_env, sizeof(int32_t) * N));
  CR(dalloc((void**)&h->st.work, sizeof(int32_t) * N));
  CR(dalloc((void**)&h->index_errors, sizeof(unsigned long long)));
  // the initialisation above ran on the null stream; the caller's (non-blocking) streams must not start before it
  CR(hipDeviceSynchronize());
#undef CR
  *out = h;
  return 0;
}

void kmanip_destroy(KHandle h) {
  if (!h) return;
  DevGuard dev_guard_(h->device);
  for (void* p : h->allocs) (void)hipFree(p);
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  delete h;
}

const char* kmanip_last_error(KHandle h) { return h ? h->err.c_str() : g_create_error.c_str(); }
int kmanip_num_envs(KHandle h) { return h ? h->num_envs : 0; }

int kmanip_reset(KHandle h, const uint8_t* mask_dev, double* obs_dev, void* stream) {
  if (!h) return -1;
  KM_ENTER(h);
  kmanip_launch_reset(h->dmodel, h->desc, h->st, mask_dev, obs_dev, km_pick_epb(h->num_envs, h->desc.nlink <= 10 ? 4 : 2, h->epb_forced),
                      (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// Diagnostics (include/kmanip_debug.h, not part of the boundary; KMANIP_WAVE_CLOCKS=1 at create): per wave slot, the ticks its wave spent in the last
// k_step and the env it held, and every env's work counter -- HOST arrays of num_envs entries each.  Synchronous.
int kmanip_dbg_wave_clocks(KHandle h, unsigned long long* clk, int32_t* slot_env, int32_t* work) {
  if (!h) return -1;
  if (clk && !h->st.wave_clk) { h->err = "kmanip_dbg_wave_clocks: clk needs KMANIP_WAVE_CLOCKS=1 at create"; return -1; }
  KM_ENTER(h);
  HIPCHK(h, hipDeviceSynchronize());
  const size_t N = (size_t)h->num_envs;
  if (clk) HIPCHK(h, hipMemcpy(clk, h->st.wave_clk, sizeof(unsigned long long) * N, hipMemcpyDeviceToHost));
  if (slot_env) {
    if (h->spread_flags[0]) {
      // SPREAD: the LAST launch's map from the flags it read (slot = wave index in slot space x envs per wave + lane group)
      std::vector<uint8_t> fl(N);
      HIPCHK(h, hipMemcpy(fl.data(), h->spread_flags[(h->spread_k + 1) & 1], N, hipMemcpyDeviceToHost));
      const int epb = h->last_epb ? h->last_epb : km_step_epb(h->num_envs, 4, 1, h->epb_forced);      // (a chunk launch at 2048 envs runs four envs per wave, a step two)
      for (size_t blk = 0; blk < N / 64; blk++) {
        unsigned long long M = 0, S1 = 0, S2 = 0;
        for (int i = 0; i < 64; i++) {
          const unsigned long long f = fl[blk * 64 + i];
          M |= (f & 1) << i; S1 |= ((f >> 1) & 1) << i; S2 |= ((f >> 2) & 1) << i;
        }
        for (int j = 0; j < 64 / epb; j++)
          for (int g = 0; g < epb; g++) slot_env[blk * 64 + j * epb + g] = (int32_t)(blk * 64) + spread_pick(M, S1, S2, j, g, epb);
      }
    } else if (h->cost_sort) HIPCHK(h, hipMemcpy(slot_env, h->slot_env, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    else for (size_t i = 0; i < N; i++) slot_env[i] = (int32_t)i;                     // the identity map
  }
  if (work) HIPCHK(h, hipMemcpy(work, h->st.work, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  return 0;
}

int kmanip_observe(KHandle h, double* obs_dev, double* reward_dev, void* stream) {
  if (!h) { g_create_error = "kmanip_observe: null handle"; return -1; }
  KM_ENTER(h);
  kmanip_launch_observe(h->dmodel, h->desc, h->st, obs_dev, reward_dev, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// nothing requested of kmanip_forces / kmanip_forward: the call succeeds and launches nothing
static bool forces_out_empty(const KForcesDev& o) {
  return !o.qacc && !o.qfrc_constraint && !o.qfrc_actuator && !o.contact_force && !o.contact_bit && !o.contact_frame && !o.contact_pos &&
         !o.contact_dist && !o.contact_mask && !o.status;
}

// mj_forward with actuation at every env's current state: qacc, joint forces, contact forces (include/kmanip.h KForcesDev;
// kmanip_forces.hip).  One launch; the handle is only read.
int kmanip_forces(KHandle h, const KForcesDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_forces: null handle"; return -1; }
  if (!out) { h->err = "kmanip_forces: the KForcesDev pointer is NULL"; return -1; }
  if (h->desc.solver != KM_SOLVER_NEWTON) { h->err = "kmanip_forces: contact forces need the Newton solver"; return -1; }
  if (forces_out_empty(*out)) return 0;
  KM_ENTER(h);
  kmanip_launch_forces(h->dmodel, h->desc, h->st, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// link and site poses, site Jacobians, M and bias forces of every env's current state (include/kmanip.h KKinDev;
// kmanip_kinematics.hip).  One launch; the handle is only read; either solver.
int kmanip_kinematics(KHandle h, const KKinDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_kinematics: null handle"; return -1; }
  if (!out) { h->err = "kmanip_kinematics: the KKinDev pointer is NULL"; return -1; }
  if (!out->link_xpos && !out->link_xmat && !out->site_xpos && !out->site_xmat && !out->site_jacp && !out->site_jacr && !out->site_vel &&
      !out->qM && !out->qfrc_bias && !out->status) return 0;
  KM_ENTER(h);
  kmanip_launch_kinematics(h->dmodel, h->desc, h->st, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// mj_inverse at a given acceleration: qfrc_inverse, J^T f and the contact forces at that acceleration (include/kmanip.h KInverseIn /
// KInverseDev; kmanip_inverse.hip).  One launch; the handle is only read; either solver.
int kmanip_inverse(KHandle h, const KInverseIn* in, const KInverseDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_inverse: null handle"; return -1; }
  if (!in) { h->err = "kmanip_inverse: the KInverseIn pointer is NULL"; return -1; }
  if (!out) { h->err = "kmanip_inverse: the KInverseDev pointer is NULL"; return -1; }
  if (!in->qacc) { h->err = "kmanip_inverse: KInverseIn::qacc is NULL"; return -1; }
  if (!out->qfrc_inverse && !out->qfrc_constraint && !out->contact_force && !out->contact_bit && !out->contact_mask && !out->status) return 0;
  KM_ENTER(h);
  kmanip_launch_inverse(h->dmodel, h->desc, h->st, *in, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// mj_forward at rows the caller passes: kmanip_forces' outputs for n hypothetical states, each naming the env whose model parameters
// and unnamed fields it takes (include/kmanip.h KForwardIn; kmanip_forward.hip).  One launch; the handle is only read.
int kmanip_forward(KHandle h, const KForwardIn* in, int n, const KForcesDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_forward: null handle"; return -1; }
  if (row_args(h, "kmanip_forward", "KForwardIn", "KForcesDev", in, out, n)) return -1;
  if (h->desc.solver != KM_SOLVER_NEWTON) { h->err = "kmanip_forward: contact forces need the Newton solver"; return -1; }
  if (n == 0) return 0;
  if (forces_out_empty(*out)) return 0;
  KM_ENTER(h);
  kmanip_launch_forward(h->dmodel, h->desc, h->st, *in, n, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// kmanip_kinematics at rows the caller passes (include/kmanip.h KKinRowsIn; kmanip_sitekin.hip).  One launch; the
// handle is only read; either solver.
int kmanip_kinematics_rows(KHandle h, const KKinRowsIn* in, int n, const KKinDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_kinematics_rows: null handle"; return -1; }
  if (row_args(h, "kmanip_kinematics_rows", "KKinRowsIn", "KKinDev", in, out, n)) return -1;
  if (n == 0) return 0;
  if (!out->link_xpos && !out->link_xmat && !out->site_xpos && !out->site_xmat && !out->site_jacp && !out->site_jacr && !out->site_vel &&
      !out->qM && !out->qfrc_bias && !out->status) return 0;
  KM_ENTER(h);
  kmanip_launch_kinrows(h->dmodel, h->desc, h->st, *in, n, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// the site-pose cost of n rows, its gradient and Gauss-Newton Hessian (include/kmanip.h KSiteCostIn / KSiteCostDev; kmanip_sitekin.hip;
// DESIGN.md section 40).  One launch; the handle is only read; either solver.
int kmanip_site_cost(KHandle h, const KSiteCostIn* in, int n, const KSiteCostDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_site_cost: null handle"; return -1; }
  if (row_args(h, "kmanip_site_cost", "KSiteCostIn", "KSiteCostDev", in, out, n)) return -1;
  if (!in->target_pos) { h->err = "kmanip_site_cost: KSiteCostIn::target_pos is NULL"; return -1; }
  if (!in->weight) { h->err = "kmanip_site_cost: KSiteCostIn::weight is NULL"; return -1; }
  if (n == 0) return 0;
  if (!out->cost && !out->lx && !out->lxx && !out->site_xpos && !out->resid && !out->status) return 0;
  KM_ENTER(h);
  kmanip_launch_sitecost(h->dmodel, h->desc, h->st, *in, n, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// MuJoCo's rollout at rows the caller passes: nstep steps of nsub sub-steps from each row's state under the caller's ctrl (and force),
// held or per step, the state after every step recorded at the row (include/kmanip.h KRolloutIn / KRolloutDev; kmanip_rollout.hip;
// DESIGN.md section 27).  One launch; the handle is only read; the handle's solver.
int kmanip_rollout(KHandle h, const KRolloutIn* in, int n, int nstep, int nsub, const KRolloutDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_rollout: null handle"; return -1; }
  if (stepped_args(h, "kmanip_rollout", "KRolloutIn", "KRolloutDev", in, out, n, nstep, nsub)) return -1;
  if (n == 0 || nstep == 0) return 0;
  if (!out->qpos && !out->qvel && !out->qacc_warm && !out->contact_mask && !out->reward && !out->status && !out->steps_done) return 0;
  KM_ENTER(h);
  kmanip_launch_rollout(h->dmodel, h->desc, h->st, *in, n, nstep, nsub ? nsub : h->desc.n_sub_steps, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// kmanip_rollout with the policy u = ctrl + gain (state - reference) evaluated at every step boundary on the device (include/kmanip.h
// KFeedbackIn / KFeedbackDev; kmanip_rollout.hip built with KM_VAR_FB; DESIGN.md sections 29 and 30).  One launch; the handle is only
// read; the handle's solver.
int kmanip_feedback(KHandle h, const KFeedbackIn* in, int n, int nstep, int nsub, const KFeedbackDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_feedback: null handle"; return -1; }
  if (stepped_args(h, "kmanip_feedback", "KFeedbackIn", "KFeedbackDev", in, out, n, nstep, nsub)) return -1;
  if (!in->qpos_ref) { h->err = "kmanip_feedback: KFeedbackIn::qpos_ref is NULL"; return -1; }
  if (!in->qvel_ref) { h->err = "kmanip_feedback: KFeedbackIn::qvel_ref is NULL"; return -1; }
  if (!in->gain_t) { h->err = "kmanip_feedback: KFeedbackIn::gain_t is NULL"; return -1; }
  if (in->ng <= 0) { h->err = "kmanip_feedback: ng is not positive"; return -1; }
  if (!in->gain_index && in->ng < n) { h->err = "kmanip_feedback: more rows than gain trajectories need KFeedbackIn::gain_index"; return -1; }
  if (n == 0 || nstep == 0) return 0;
  if (!out->qpos && !out->qvel && !out->qacc_warm && !out->contact_mask && !out->reward && !out->status && !out->steps_done && !out->ctrl) return 0;
  KM_ENTER(h);
  kmanip_launch_feedback(h->dmodel, h->desc, h->st, *in, n, nstep, nsub ? nsub : h->desc.n_sub_steps, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// kmanip_feedback with the policy's output clamped to a box (include/kmanip.h KFeedbackBoxIn; kmanip_rollout.hip built with KM_VAR_FB=2,
// the kmanip_boxfb_* objects).  One launch; the handle is only read; the handle's solver.
int kmanip_feedback_box(KHandle h, const KFeedbackBoxIn* in, int n, int nstep, int nsub, const KFeedbackDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_feedback_box: null handle"; return -1; }
  if (stepped_args(h, "kmanip_feedback_box", "KFeedbackBoxIn", "KFeedbackDev", in, out, n, nstep, nsub)) return -1;
  if (!in->qpos_ref) { h->err = "kmanip_feedback_box: KFeedbackBoxIn::qpos_ref is NULL"; return -1; }
  if (!in->qvel_ref) { h->err = "kmanip_feedback_box: KFeedbackBoxIn::qvel_ref is NULL"; return -1; }
  if (!in->gain_t) { h->err = "kmanip_feedback_box: KFeedbackBoxIn::gain_t is NULL"; return -1; }
  if (!in->lo) { h->err = "kmanip_feedback_box: KFeedbackBoxIn::lo is NULL"; return -1; }
  if (!in->hi) { h->err = "kmanip_feedback_box: KFeedbackBoxIn::hi is NULL"; return -1; }
  if (in->ng <= 0) { h->err = "kmanip_feedback_box: ng is not positive"; return -1; }
  if (!in->gain_index && in->ng < n) { h->err = "kmanip_feedback_box: more rows than gain trajectories need KFeedbackBoxIn::gain_index"; return -1; }
  if (n == 0 || nstep == 0) return 0;
  if (!out->qpos && !out->qvel && !out->qacc_warm && !out->contact_mask && !out->reward && !out->status && !out->steps_done && !out->ctrl) return 0;
  KM_ENTER(h);
  kmanip_launch_boxfb(h->dmodel, h->desc, h->st, *in, n, nstep, nsub ? nsub : h->desc.n_sub_steps, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// MuJoCo's mjd_transitionFD at rows the caller passes (include/kmanip.h KTransFdIn / KTransFdDev; kmanip_transfd.hip; DESIGN.md section
// 31).  Two launches ordered by the stream: the nominal rows through kmanip_rollout's kernel, then the column pairs, which read the
// nominal qacc_warm the first wrote.  The handle is only read; the handle's solver.
int kmanip_transition_fd(KHandle h, const KTransFdIn* in, int n, int nsub, const KTransFdDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_transition_fd: null handle"; return -1; }
  if (row_args(h, "kmanip_transition_fd", "KTransFdIn", "KTransFdDev", in, out, n)) return -1;
  if (nsub < 0) { h->err = "kmanip_transition_fd: nsub is negative"; return -1; }
  const int wrt = in->wrt, nv = h->desc.nlink + 6, nu = h->desc.nlink;
  if (wrt & ~(KM_WRT_QPOS | KM_WRT_QVEL | KM_WRT_CTRL | KM_WRT_FRC)) { h->err = "kmanip_transition_fd: wrt has bits outside KM_WRT_*"; return -1; }
  if (!(in->eps - in->eps == 0.0) || !(in->eps > 0.0)) { h->err = "kmanip_transition_fd: eps is not a finite positive number"; return -1; }
  if (!(in->warm_offset - in->warm_offset == 0.0)) { h->err = "kmanip_transition_fd: warm_offset is not finite"; return -1; }
  if (n == 0) return 0;                // (tensors of no rows have no address: nothing below is asked of them)
  if (wrt && !out->deriv_t) { h->err = "kmanip_transition_fd: wrt is set and KTransFdDev::deriv_t is NULL"; return -1; }
  if (wrt && !in->qacc_warm && !out->qacc_warm) {
    h->err = "kmanip_transition_fd: without KTransFdIn::qacc_warm the perturbed rows start from KTransFdDev::qacc_warm, which is NULL";
    return -1;
  }
  const int ncol = ((wrt & KM_WRT_QPOS) ? nv : 0) + ((wrt & KM_WRT_QVEL) ? nv : 0) + ((wrt & KM_WRT_CTRL) ? nu : 0) + ((wrt & KM_WRT_FRC) ? nv : 0);
  if (2LL * ncol * n > 2147483647LL) { h->err = "kmanip_transition_fd: 2 ncol n perturbed rows are more than an int counts"; return -1; }
  const int ns = nsub ? nsub : h->desc.n_sub_steps;
  const hipStream_t s = (hipStream_t)stream;
  const bool nominal = out->qpos || out->qvel || out->qacc_warm || out->contact_mask || out->status;
  if (!nominal && !wrt) return 0;
  KM_ENTER(h);
  if (nominal) {
    const KRolloutIn ri = {in->env_index, in->qpos, in->qvel, in->qacc_warm, in->ctrl, in->qfrc_applied, 0, 0};
    const KRolloutDev ro = {out->qpos, out->qvel, out->qacc_warm, out->contact_mask, nullptr, out->status, nullptr};
    kmanip_launch_rollout(h->dmodel, h->desc, h->st, ri, n, 1, ns, ro, s);
    HIPCHK(h, hipGetLastError());
  }
  if (wrt) {
    // tangent_perturb's rotation columns: cos and sin of eps / 2, once, on the host
    kmanip_launch_transfd(h->dmodel, h->desc, h->st, *in, n, ncol, ns, cos(0.5 * in->eps), sin(0.5 * in->eps), *out, s);
    HIPCHK(h, hipGetLastError());
  }
  return 0;
}

// Centred finite differences of ONE step in the per-env physics parameters at rows the caller passes (include/kmanip.h KParamFdIn /
// KParamFdDev; kmanip_paramfd.hip).  One launch; the handle is only read; the handle's solver; always a
// per-env parameter build, on a handle without parameters over the compiled model's values.
int kmanip_param_fd(KHandle h, const KParamFdIn* in, int n, int nsub, const KParamFdDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_param_fd: null handle"; return -1; }
  if (row_args(h, "kmanip_param_fd", "KParamFdIn", "KParamFdDev", in, out, n)) return -1;
  if (nsub < 0) { h->err = "kmanip_param_fd: nsub is negative"; return -1; }
  const int wrt = in->wrt;
  if (wrt & ~((1 << KM_EP_N) - 1)) { h->err = "kmanip_param_fd: wrt has bits outside the KM_EP_* parameters"; return -1; }
  if (!(in->warm_offset - in->warm_offset == 0.0)) { h->err = "kmanip_param_fd: warm_offset is not finite"; return -1; }
  int npar = 0;
  for (int k = 0; k < KM_EP_N; k++) {
    if (!((wrt >> k) & 1)) continue;
    npar++;
    if (!(in->eps[k] - in->eps[k] == 0.0) || !(in->eps[k] > 0.0)) {
      h->err = "kmanip_param_fd: eps[" + std::to_string(k) + "] of a selected parameter is not a finite positive number";
      return -1;
    }
  }
  if (n == 0 || wrt == 0) return 0;    // (tensors of no rows have no address: nothing below is asked of them)
  if (!out->deriv_t) { h->err = "kmanip_param_fd: wrt is set and KParamFdDev::deriv_t is NULL"; return -1; }
  if (2LL * npar * n > 2147483647LL) { h->err = "kmanip_param_fd: 2 npar n perturbed rows are more than an int counts"; return -1; }
  KM_ENTER(h);
  const KModelDesc& d = h->desc;
  const KEnvParamDefaults model{{d.cube_mass, d.con_cube_friction[0], d.cube_frictionloss, 1.0}};
  kmanip_launch_paramfd(h->dmodel, h->desc, h->st, *in, model, n, npar, nsub ? nsub : d.n_sub_steps, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The backward pass of iLQR for n problems of T steps (include/kmanip.h KLqrIn / KLqrDev; kmanip_lqr.hip).  One
// launch; the handle gives the device and the size class and is only read.
int kmanip_lqr_backward(KHandle h, const KLqrIn* in, int n, int T, const KLqrDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_lqr_backward: null handle"; return -1; }
  if (!in) { h->err = "kmanip_lqr_backward: the KLqrIn pointer is NULL"; return -1; }
  if (!out) { h->err = "kmanip_lqr_backward: the KLqrDev pointer is NULL"; return -1; }
  if (n < 0) { h->err = "kmanip_lqr_backward: n is negative"; return -1; }
  if (T < 0) { h->err = "kmanip_lqr_backward: T is negative"; return -1; }
  if (n == 0 || T == 0) return 0;      // (tensors of no problems or no steps have no address: nothing below is asked of them)
  if (!in->a_t) { h->err = "kmanip_lqr_backward: KLqrIn::a_t is NULL"; return -1; }
  if (!in->b_t) { h->err = "kmanip_lqr_backward: KLqrIn::b_t is NULL"; return -1; }
  if (!in->lx) { h->err = "kmanip_lqr_backward: KLqrIn::lx is NULL"; return -1; }
  if (!in->lu) { h->err = "kmanip_lqr_backward: KLqrIn::lu is NULL"; return -1; }
  if (!in->lxx) { h->err = "kmanip_lqr_backward: KLqrIn::lxx is NULL"; return -1; }
  if (!in->luu) { h->err = "kmanip_lqr_backward: KLqrIn::luu is NULL"; return -1; }
  const int64_t nx = h->desc.nlink <= 10 ? 32 : 52, nu = h->desc.nlink <= 10 ? 10 : 20;      // (kmanip_lqr.hip's two classes)
  if (in->a_stride != 0 && in->a_stride < nx * nx) { h->err = "kmanip_lqr_backward: a_stride is smaller than an [nx, nx] block"; return -1; }
  if (in->b_stride != 0 && in->b_stride < nu * nx) { h->err = "kmanip_lqr_backward: b_stride is smaller than an [nu, nx] block"; return -1; }
  if ((long long)n * T > 2147483647LL) { h->err = "kmanip_lqr_backward: n * T steps are more than an int counts"; return -1; }
  if (!out->k && !out->gain_t && !out->dv && !out->status && !out->fail_step) return 0;
  KLqrIn li = *in;
  if (!li.a_stride) li.a_stride = nx * nx;
  if (!li.b_stride) li.b_stride = nu * nx;
  KM_ENTER(h);
  kmanip_launch_lqr_backward(h->desc, li, n, T, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The backward pass of control-limited DDP for n problems of T steps (include/kmanip.h KLqrBoxIn / KLqrBoxDev; kmanip_lqr_box.hip;
// DESIGN.md section 39).  One launch; the handle gives the device and the size class and is only read.
int kmanip_lqr_backward_box(KHandle h, const KLqrBoxIn* in, int n, int T, const KLqrBoxDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_lqr_backward_box: null handle"; return -1; }
  if (!in) { h->err = "kmanip_lqr_backward_box: the KLqrBoxIn pointer is NULL"; return -1; }
  if (!out) { h->err = "kmanip_lqr_backward_box: the KLqrBoxDev pointer is NULL"; return -1; }
  if (n < 0) { h->err = "kmanip_lqr_backward_box: n is negative"; return -1; }
  if (T < 0) { h->err = "kmanip_lqr_backward_box: T is negative"; return -1; }
  if (n == 0 || T == 0) return 0;      // (tensors of no problems or no steps have no address: nothing below is asked of them)
  const KLqrIn& l = in->lqr;
  if (!l.a_t) { h->err = "kmanip_lqr_backward_box: KLqrIn::a_t is NULL"; return -1; }
  if (!l.b_t) { h->err = "kmanip_lqr_backward_box: KLqrIn::b_t is NULL"; return -1; }
  if (!l.lx) { h->err = "kmanip_lqr_backward_box: KLqrIn::lx is NULL"; return -1; }
  if (!l.lu) { h->err = "kmanip_lqr_backward_box: KLqrIn::lu is NULL"; return -1; }
  if (!l.lxx) { h->err = "kmanip_lqr_backward_box: KLqrIn::lxx is NULL"; return -1; }
  if (!l.luu) { h->err = "kmanip_lqr_backward_box: KLqrIn::luu is NULL"; return -1; }
  if (!in->u) { h->err = "kmanip_lqr_backward_box: KLqrBoxIn::u is NULL"; return -1; }
  if (!in->lo) { h->err = "kmanip_lqr_backward_box: KLqrBoxIn::lo is NULL"; return -1; }
  if (!in->hi) { h->err = "kmanip_lqr_backward_box: KLqrBoxIn::hi is NULL"; return -1; }
  const int64_t nx = h->desc.nlink <= 10 ? 32 : 52, nu = h->desc.nlink <= 10 ? 10 : 20;      // (kmanip_lqr_box.hip's two classes)
  if (l.a_stride != 0 && l.a_stride < nx * nx) { h->err = "kmanip_lqr_backward_box: a_stride is smaller than an [nx, nx] block"; return -1; }
  if (l.b_stride != 0 && l.b_stride < nu * nx) { h->err = "kmanip_lqr_backward_box: b_stride is smaller than an [nu, nx] block"; return -1; }
  if ((long long)n * T > 2147483647LL) { h->err = "kmanip_lqr_backward_box: n * T steps are more than an int counts"; return -1; }
  const KLqrDev& o = out->lqr;
  if (!o.k && !o.gain_t && !o.dv && !o.status && !o.fail_step && !out->clamped && !out->qp_iters) return 0;
  KLqrBoxIn li = *in;
  if (!li.lqr.a_stride) li.lqr.a_stride = nx * nx;
  if (!li.lqr.b_stride) li.lqr.b_stride = nu * nx;
  KM_ENTER(h);
  kmanip_launch_lqr_backward_box(h->desc, li, n, T, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The adjoint sweep of a rollout for n problems of T steps and m cotangent vectors each (include/kmanip.h KAdjointIn / KAdjointDev;
// kmanip_adjoint.hip).  One launch; the handle gives the device and the size class and is only read.
int kmanip_adjoint(KHandle h, const KAdjointIn* in, int n, int T, int m, const KAdjointDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_adjoint: null handle"; return -1; }
  if (!in) { h->err = "kmanip_adjoint: the KAdjointIn pointer is NULL"; return -1; }
  if (!out) { h->err = "kmanip_adjoint: the KAdjointDev pointer is NULL"; return -1; }
  if (n < 0) { h->err = "kmanip_adjoint: n is negative"; return -1; }
  if (T < 0) { h->err = "kmanip_adjoint: T is negative"; return -1; }
  if (m < 0) { h->err = "kmanip_adjoint: m is negative"; return -1; }
  if (n == 0 || T == 0 || m == 0) return 0;      // (tensors of no problems, steps or vectors have no address: nothing below is asked of them)
  if (!in->a_t) { h->err = "kmanip_adjoint: KAdjointIn::a_t is NULL"; return -1; }
  if (!in->b_t) { h->err = "kmanip_adjoint: KAdjointIn::b_t is NULL"; return -1; }
  if (!in->gx) { h->err = "kmanip_adjoint: KAdjointIn::gx is NULL"; return -1; }
  const int64_t nx = h->desc.nlink <= 10 ? 32 : 52, nu = h->desc.nlink <= 10 ? 10 : 20;      // (kmanip_adjoint.hip's two classes)
  if (in->a_stride != 0 && in->a_stride < nx * nx) { h->err = "kmanip_adjoint: a_stride is smaller than an [nx, nx] block"; return -1; }
  if (in->b_stride != 0 && in->b_stride < nu * nx) { h->err = "kmanip_adjoint: b_stride is smaller than an [nu, nx] block"; return -1; }
  if ((long long)n * m > 2147483647LL || (long long)n * m * T > 2147483647LL) { h->err = "kmanip_adjoint: n * m * T row steps are more than an int counts"; return -1; }
  if (!out->lam && !out->mu) return 0;
  KAdjointIn ai = *in;
  if (!ai.a_stride) ai.a_stride = nx * nx;
  if (!ai.b_stride) ai.b_stride = nu * nx;
  KM_ENTER(h);
  kmanip_launch_adjoint(h->desc, ai, n, T, m, *out, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// One helper of the kernels' math headers over n rows (include/kmanip_debug.h; kmanip_mathprobe.hip).  One
// launch; the handle gives the device and is only read.
int kmanip_dbg_math(KHandle h, int fn, int n, const double* in_dev, int in_cols, double* out_dev, int out_cols, void* stream) {
  if (!h) { g_create_error = "kmanip_dbg_math: null handle"; return -1; }
  int ic = 0, oc = 0;
  if (!kmanip_math_probe_cols(fn, &ic, &oc)) { h->err = "kmanip_dbg_math: no such function"; return -1; }
  if (in_cols != ic) { h->err = "kmanip_dbg_math: in_cols is not the function's argument count"; return -1; }
  if (out_cols != oc) { h->err = "kmanip_dbg_math: out_cols is not the function's result count"; return -1; }
  if (n < 0) { h->err = "kmanip_dbg_math: n is negative"; return -1; }
  if (n == 0) return 0;
  if (!in_dev) { h->err = "kmanip_dbg_math: in_dev is NULL"; return -1; }
  if (!out_dev) { h->err = "kmanip_dbg_math: out_dev is NULL"; return -1; }
  KM_ENTER(h);
  kmanip_launch_math_probe(fn, n, in_dev, out_dev, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// the render launchers' visual inputs for a render of source `src` (-1 live state, 0 / 1 a snapshot): in ranges mode the draw
// uses the episode counters of that source (a snapshot taken before ranges mode was on has none: the live ones)
static KVisArgs vis_args(KHandle h, int src) {
  KVisArgs v = h->vis;
  if (v.range) v.episode = (src >= 0 && h->ep_snap_ok[src]) ? h->ep_snap[src] : h->st.episode;
  return v;
}

// the state a render reads: the live one, or the snapshot kmanip_set_render_source chose
static KDeviceState render_state(KHandle h) {
  KDeviceState st = h->st;
  if (h->render_src >= 0) st.qpos = h->qpos_snap[h->render_src];
  return st;
}
// the handle's capsule list as the launchers take it; for the depth renders and the point clouds only while the depth flag is on
static KLinkArgs link_args(KHandle h) { return KLinkArgs{h->links_buf, (int)h->links.size()}; }
static KLinkArgs depth_link_args(KHandle h) { return h->depth_links && !h->links.empty() ? link_args(h) : KLinkArgs{nullptr, 0}; }

// the end of an RGB / label render entry.  Kernel timing (kmanip_enable_timing): the camera observations rendered right after a timed step are that step's render leg --
// its start is the event the step recorded after k_step, so the render costs the stream ONE more event, not a pair around it
// (a render of a SNAPSHOT runs behind the steps, on a stream of its own: it is no leg of the step's stream)
static int render_done(KHandle h, void* stream) {
  if (h->timing && h->render_src < 0 && h->last_step_timed && h->timed_steps > 0 && !h->ev_render[h->timed_steps - 1]) {
    HIPCHK(h, hipEventRecord(h->ev[3 * (size_t)(h->timed_steps - 1) + 2], (hipStream_t)stream));
    h->ev_render[h->timed_steps - 1] = 1;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

static int step_impl(KHandle h, int nchunk, const float* act_dev, double* obs_dev, double* reward_dev, uint8_t* done_dev, void* stream) {
  if (!h) { g_create_error = "kmanip_step: null handle"; return -1; }
  if (!act_dev || !obs_dev || !reward_dev || !done_dev) { h->err = "kmanip_step: null buffer"; return -1; }
  KM_ENTER(h);
  hipStream_t s = (hipStream_t)stream;
  const bool tm = h->timing && (h->timing_count++ % h->timing_every) == 0 && h->timed_steps < KM_TIMING_SLOTS;
  h->last_step_timed = tm;
  hipEvent_t* ev = tm ? &h->ev[3 * (size_t)h->timed_steps] : nullptr;
  // ONE launch: before_step (decode + IK) runs inside k_step, so that no device-wide barrier sits between an env's IK and
  // its physics
  h->st.rd_rec = nullptr;
  if (nchunk == 1 && h->rd_rec[0]) h->st.rd_rec = h->rd_rec[h->rd_sel];     // (the CALLER alternates: kmanip_select_reward_done_record)
  h->st.slot_env = nullptr;
  if (h->cost_sort) {                        // (one small launch: counting sort of the envs by their last step's diagnostics)
    kmanip_launch_sort_envs(h->st, h->slot_env, h->cost_w, s);
    h->st.slot_env = h->slot_env;
  }
  h->st.spread_in = nullptr; h->st.spread_out = nullptr;
  if (h->spread_flags[0]) {       // SPREAD: this launch (one step or a chunk of them) reads the flags the last launch wrote, and writes the other array
    h->st.spread_in = h->spread_flags[h->spread_k & 1]; h->st.spread_out = h->spread_flags[(h->spread_k + 1) & 1];
    h->spread_k++;
  }
  h->last_epb = km_step_epb(h->num_envs, h->desc.nlink <= 10 ? 4 : 2, nchunk, h->epb_forced);
  if (tm) HIPCHK(h, hipEventRecord(ev[0], s));        // (two events per step, each costs the stream a barrier packet)
  kmanip_launch_step(h->dmodel, h->desc, h->st, act_dev, obs_dev, reward_dev, done_dev, nchunk, h->last_epb, s);
  if (tm) HIPCHK(h, hipEventRecord(ev[1], s));
  const bool render = h->step_depth && nchunk == 1;
  if (render) {                           // the observation's camera branch (env_sim.py:140-145) of the state just produced
    const KLinkArgs links = depth_link_args(h);
    if (links.n > 0) kmanip_launch_render_depth_links(h->dmodel, h->st, h->step_cam, h->step_h, h->step_w, h->step_depth, links, vis_args(h, -1), s);
    else
      kmanip_launch_render_depth(h->dmodel, h->st, h->step_cam, h->step_h, h->step_w, h->step_depth, vis_args(h, -1), s);
  }
  if (tm) {
    if (render) HIPCHK(h, hipEventRecord(ev[2], s));
    h->ev_render[h->timed_steps] = render;
    h->timed_steps++;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_step(KHandle h, const float* act_dev, double* obs_dev, double* reward_dev, uint8_t* done_dev, void* stream) {
  return step_impl(h, 1, act_dev, obs_dev, reward_dev, done_dev, stream);
}

int kmanip_step_chunk(KHandle h, int nsteps, const float* act_dev, double* obs_dev, double* reward_dev, uint8_t* done_dev, void* stream) {
  if (nsteps <= 0) { if (h) h->err = "kmanip_step_chunk: nsteps must be positive"; return -1; }
  return step_impl(h, nsteps, act_dev, obs_dev, reward_dev, done_dev, stream);
}

int kmanip_render_depth(KHandle h, int cam, int height, int width, float* depth_dev, void* stream) {
  if (!h || !depth_dev || cam < 0 || cam >= KM_MAX_CAMS || height <= 0 || width <= 0) { if (h) h->err = "kmanip_render_depth: bad arguments"; return -1; }
  if (!h->desc.cam_present[cam]) { h->err = "kmanip_render_depth: this model has no such camera"; return -1; }
  KM_ENTER(h);
  const KDeviceState st = render_state(h);
  const KLinkArgs links = depth_link_args(h);
  if (links.n > 0) kmanip_launch_render_depth_links(h->dmodel, st, cam, height, width, depth_dev, links, vis_args(h, h->render_src), (hipStream_t)stream);
  else
    kmanip_launch_render_depth(h->dmodel, st, cam, height, width, depth_dev, vis_args(h, h->render_src), (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_get_camera_poses(KHandle h, int cam, double* pose_dev, void* stream) {
  if (!h) { g_create_error = "kmanip_get_camera_poses: null handle"; return -1; }
  if (!pose_dev) { h->err = "kmanip_get_camera_poses: pose_dev is NULL"; return -1; }
  if (cam < 0 || cam >= KM_MAX_CAMS || !h->desc.cam_present[cam]) { h->err = "kmanip_get_camera_poses: this model has no such camera"; return -1; }
  KM_ENTER(h);
  const KDeviceState st = render_state(h);
  kmanip_launch_camera_poses(h->dmodel, st, cam, pose_dev, vis_args(h, h->render_src), (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_render_points(KHandle h, int cam, int height, int width, int frame, float* xyz_dev, float* depth_dev, void* stream) {
  if (!h) { g_create_error = "kmanip_render_points: null handle"; return -1; }
  if (!xyz_dev) { h->err = "kmanip_render_points: xyz_dev is NULL"; return -1; }
  if (cam < 0 || cam >= KM_MAX_CAMS || !h->desc.cam_present[cam]) { h->err = "kmanip_render_points: this model has no such camera"; return -1; }
  if (height <= 0 || width <= 0) { h->err = "kmanip_render_points: height and width must be positive"; return -1; }
  if (frame != KM_POINTS_CAMERA && frame != KM_POINTS_WORLD) { h->err = "kmanip_render_points: frame must be KM_POINTS_CAMERA or KM_POINTS_WORLD"; return -1; }
  KM_ENTER(h);
  const KDeviceState st = render_state(h);
  kmanip_launch_render_points(h->dmodel, st, cam, height, width, frame == KM_POINTS_WORLD, xyz_dev, depth_dev, depth_link_args(h), vis_args(h, h->render_src),
                              (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_snapshot_render_state(KHandle h, int slot, void* stream) {
  if (!h) { g_create_error = "kmanip_snapshot_render_state: null handle"; return -1; }
  if (slot < 0 || slot > 1) { h->err = "kmanip_snapshot_render_state: slot must be 0 or 1"; return -1; }
  KM_ENTER(h);
  const size_t bytes = sizeof(double) * (size_t)(h->desc.nlink + 7) * h->num_envs;
  if (!h->qpos_snap[slot]) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, bytes));
    h->allocs.push_back(p);
    h->qpos_snap[slot] = (double*)p;
  }
  HIPCHK(h, hipMemcpyAsync(h->qpos_snap[slot], h->st.qpos, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  // visual ranges mode: the draw of the snapshot's images uses the episode of the snapshot's step, not of a later auto-reset
  h->ep_snap_ok[slot] = false;
  if (h->vis.range) {
    if (!h->ep_snap[slot]) {
      void* p = nullptr;
      HIPCHK(h, hipMalloc(&p, sizeof(int32_t) * (size_t)h->num_envs));
      h->allocs.push_back(p);
      h->ep_snap[slot] = (int32_t*)p;
    }
    HIPCHK(h, hipMemcpyAsync(h->ep_snap[slot], h->st.episode, sizeof(int32_t) * (size_t)h->num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    h->ep_snap_ok[slot] = true;
  }
  return 0;
}

int kmanip_set_render_source(KHandle h, int slot) {
  if (!h) { g_create_error = "kmanip_set_render_source: null handle"; return -1; }
  if (slot < -1 || slot > 1) { h->err = "kmanip_set_render_source: slot must be -1 (live state), 0 or 1"; return -1; }
  if (slot >= 0 && !h->qpos_snap[slot]) { h->err = "kmanip_set_render_source: no snapshot was taken into that slot"; return -1; }
  h->render_src = slot;
  return 0;
}

int kmanip_render_rgb_multi(KHandle h, int ncam, const int* cams, const int* heights, const int* widths, uint8_t* const* rgb_dev,
                            void* stream) {
  if (!h) { g_create_error = "kmanip_render_rgb: null handle"; return -1; }
  if (ncam <= 0 || ncam > KM_MAX_CAMS || !cams || !heights || !widths || !rgb_dev) { h->err = "kmanip_render_rgb: bad arguments"; return -1; }
  KRenderJobs jobs;
  jobs.n = ncam;
  for (int i = 0; i < ncam; i++) {
    if (!rgb_dev[i] || cams[i] < 0 || cams[i] >= KM_MAX_CAMS || heights[i] <= 0 || widths[i] <= 0) { h->err = "kmanip_render_rgb: bad arguments"; return -1; }
    if (!h->desc.cam_present[cams[i]]) { h->err = "kmanip_render_rgb: this model has no such camera"; return -1; }
    jobs.cam[i] = cams[i]; jobs.height[i] = heights[i]; jobs.width[i] = widths[i]; jobs.rgb[i] = rgb_dev[i];
  }
  KM_ENTER(h);
  const KDeviceState st = render_state(h);
  if (!h->links.empty()) {
    // link capsules: the kernel that draws them, with no label output
    KLabelJobs lj{};
    lj.n = ncam;
    for (int i = 0; i < ncam; i++) { lj.cam[i] = jobs.cam[i]; lj.height[i] = jobs.height[i]; lj.width[i] = jobs.width[i]; lj.rgb[i] = jobs.rgb[i]; lj.seg[i] = nullptr; }
    kmanip_launch_render_links(h->dmodel, st, lj, true, link_args(h), vis_args(h, h->render_src), (hipStream_t)stream);
  } else
    kmanip_launch_render_rgb(h->dmodel, st, jobs, vis_args(h, h->render_src), (hipStream_t)stream);
  return render_done(h, stream);
}

int kmanip_render_rgb(KHandle h, int cam, int height, int width, uint8_t* rgb_dev, void* stream) {
  return kmanip_render_rgb_multi(h, 1, &cam, &height, &width, &rgb_dev, stream);
}

int kmanip_render_labels_multi(KHandle h, int ncam, const int* cams, const int* heights, const int* widths, uint8_t* const* rgb_dev,
                               uint8_t* const* seg_dev, void* stream) {
  if (!h) { g_create_error = "kmanip_render_labels: null handle"; return -1; }
  if (ncam <= 0 || ncam > KM_MAX_CAMS || !cams || !heights || !widths || (!rgb_dev && !seg_dev)) { h->err = "kmanip_render_labels: bad arguments"; return -1; }
  KLabelJobs jobs;
  jobs.n = ncam;
  int nrgb = 0, nseg = 0;
  for (int i = 0; i < ncam; i++) {
    uint8_t* const r = rgb_dev ? rgb_dev[i] : nullptr;
    uint8_t* const g = seg_dev ? seg_dev[i] : nullptr;
    if (!r && !g) { h->err = "kmanip_render_labels: a job needs rgb_dev[i] or seg_dev[i]"; return -1; }
    if (cams[i] < 0 || cams[i] >= KM_MAX_CAMS || heights[i] <= 0 || widths[i] <= 0) { h->err = "kmanip_render_labels: bad arguments"; return -1; }
    if (!h->desc.cam_present[cams[i]]) { h->err = "kmanip_render_labels: this model has no such camera"; return -1; }
    jobs.cam[i] = cams[i]; jobs.height[i] = heights[i]; jobs.width[i] = widths[i]; jobs.rgb[i] = r; jobs.seg[i] = g;
    nrgb += r != nullptr; nseg += g != nullptr;
  }
  // no label wanted anywhere: this is the RGB render
  if (nseg == 0) return kmanip_render_rgb_multi(h, ncam, cams, heights, widths, rgb_dev, stream);
  KM_ENTER(h);
  const KDeviceState st = render_state(h);
  // labels only in every job: the kernel that does not shade; anything else: the one that writes what each job asks for
  if (!h->links.empty())
    kmanip_launch_render_links(h->dmodel, st, jobs, nrgb > 0, link_args(h), vis_args(h, h->render_src), (hipStream_t)stream);
  else
    kmanip_launch_render_labels(h->dmodel, st, jobs, nrgb > 0, vis_args(h, h->render_src), (hipStream_t)stream);
  return render_done(h, stream);
}

int kmanip_render_seg(KHandle h, int cam, int height, int width, uint8_t* seg_dev, void* stream) {
  return kmanip_render_labels_multi(h, 1, &cam, &height, &width, nullptr, &seg_dev, stream);
}

int kmanip_set_render_links(KHandle h, int n, const KLinkCapsule* caps) {
  if (!h) { g_create_error = "kmanip_set_render_links: null handle"; return -1; }
  if (n < 0 || n > KM_MAX_LINK_CAPSULES) { h->err = "kmanip_set_render_links: n must be 0 .. " + std::to_string(KM_MAX_LINK_CAPSULES); return -1; }
  if (n > 0 && !caps) { h->err = "kmanip_set_render_links: caps is NULL with n > 0"; return -1; }
  auto finite = [](double v) { return v - v == 0.0; };
  for (int k = 0; k < n; k++) {
    const KLinkCapsule& c = caps[k];
    const char* what = nullptr;
    if (c.link < 0 || c.link >= h->desc.nlink) what = "link out of range";
    else if (c.label != KM_SEG_ROBOT_R && c.label != KM_SEG_ROBOT_L) what = "label must be KM_SEG_ROBOT_R or KM_SEG_ROBOT_L";
    else if (!finite(c.radius) || !(c.radius > 0)) what = "radius must be finite and > 0";
    else for (int q = 0; q < 3; q++) if (!finite(c.p0[q]) || !finite(c.seg[q])) what = "p0 and seg must be finite";
    if (what) { h->err = "kmanip_set_render_links: capsule " + std::to_string(k) + ": " + what; return -2; }
  }
  KM_ENTER(h);
  // a render in flight on any stream may read the list: every change waits for the device
  HIPCHK(h, hipDeviceSynchronize());
  if (n == 0) { h->links.clear(); return 0; }
  if (!h->links_buf) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, sizeof(KLinkCapsule) * KM_MAX_LINK_CAPSULES));
    h->allocs.push_back(p);
    h->links_buf = (KLinkCapsule*)p;
  }
  std::vector<KLinkCapsule> list(caps, caps + n);
  for (auto& c : list) c.pad_ = 0;
  HIPCHK(h, hipMemcpy(h->links_buf, list.data(), sizeof(KLinkCapsule) * n, hipMemcpyHostToDevice));
  HIPCHK(h, hipDeviceSynchronize());
  h->links.swap(list);
  return 0;
}

int kmanip_get_render_links(KHandle h, int* n, KLinkCapsule* caps) {
  if (!h) { g_create_error = "kmanip_get_render_links: null handle"; return -1; }
  if (!n) { h->err = "kmanip_get_render_links: n is NULL"; return -1; }
  *n = (int)h->links.size();
  if (caps) for (size_t k = 0; k < h->links.size(); k++) caps[k] = h->links[k];
  return 0;
}

int kmanip_set_depth_links(KHandle h, int on) {
  if (!h) { g_create_error = "kmanip_set_depth_links: null handle"; return -1; }
  KM_ENTER(h);
  // like a change of the list: a render in flight keeps what it was launched with, and the device is idle when this returns
  HIPCHK(h, hipDeviceSynchronize());
  h->depth_links = on != 0;
  return 0;
}

int kmanip_get_depth_links(KHandle h, int* on) {
  if (!h) { g_create_error = "kmanip_get_depth_links: null handle"; return -1; }
  if (!on) { h->err = "kmanip_get_depth_links: on is NULL"; return -1; }
  *on = h->depth_links ? 1 : 0;
  return 0;
}

int kmanip_bind_step_depth(KHandle h, int cam, int height, int width, float* depth_dev) {
  if (!h) { g_create_error = "kmanip_bind_step_depth: null handle"; return -1; }
  if (!depth_dev) { h->step_depth = nullptr; h->step_cam = -1; return 0; }
  if (cam < 0 || cam >= KM_MAX_CAMS || height <= 0 || width <= 0 || !h->desc.cam_present[cam]) { h->err = "kmanip_bind_step_depth: bad camera / size"; return -1; }
  h->step_cam = cam; h->step_h = height; h->step_w = width; h->step_depth = depth_dev;
  return 0;
}

int kmanip_scripted_action(KHandle h, float* act_dev, void* stream) {
  if (!h || !act_dev) { if (h) h->err = "kmanip_scripted_action: null buffer"; return -1; }
  if (!h->desc.arm_present[0] || h->desc.act_col[KM_ACT_EER_POS] < 0) {
    h->err = "kmanip_scripted_action: this env id has no eer_pos action (the scripted policy drives the right EE delta)"; return -1;
  }
  KM_ENTER(h);
  kmanip_launch_scripted_action(h->dmodel, h->st, act_dev, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_sample_action(KHandle h, float* act_dev, int ahead, void* stream) {
  if (!h || !act_dev || ahead < 0) { if (h) h->err = "kmanip_sample_action: null buffer / negative ahead"; return -1; }
  if (h->desc.act_dim > 16) { h->err = "kmanip_sample_action: act_dim > 16"; return -1; }
  KM_ENTER(h);
  kmanip_launch_sample_action(h->dmodel, h->st, act_dev, ahead, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_enable_timing(KHandle h, int enable) {
  if (!h) return -1;
  KM_ENTER(h);
  if (enable && h->ev.empty()) {
    h->ev.resize(3 * KM_TIMING_SLOTS, nullptr);
    h->ev_render.assign(KM_TIMING_SLOTS, 0);
    for (auto& e : h->ev) HIPCHK(h, hipEventCreate(&e));
  }
  h->timing = enable != 0;
  h->timing_every = enable > 1 ? enable : 1;
  h->timing_count = 0;
  h->timed_steps = 0;
  return 0;
}
int kmanip_timing_summary(KHandle h, double* ik_ms_sum, double* dyn_ms_sum, double* render_ms_sum, int32_t* nsteps) {
  if (!h) return -1;
  KM_ENTER(h);
  HIPCHK(h, hipDeviceSynchronize());
  double dyn = 0, ren = 0;
  for (int k = 0; k < h->timed_steps; k++) {
    float md = 0, mr = 0;
    HIPCHK(h, hipEventElapsedTime(&md, h->ev[3 * k], h->ev[3 * k + 1]));
    if (h->ev_render[k]) HIPCHK(h, hipEventElapsedTime(&mr, h->ev[3 * k + 1], h->ev[3 * k + 2]));
    dyn += md; ren += mr;
  }
  if (ik_ms_sum) *ik_ms_sum = 0;      // (before_step runs inside k_step: its time is part of dyn_ms_sum)
  if (dyn_ms_sum) *dyn_ms_sum = dyn;
  if (render_ms_sum) *render_ms_sum = ren;
  if (nsteps) *nsteps = h->timed_steps;
  h->timed_steps = 0;
  return 0;
}

// env-major host <-> component-major device transposes
static int pull(KHandle h, const double* dev, double* host, int ncomp) {
  if (!host) return 0;
  const size_t N = (size_t)h->num_envs;
  std::vector<double> tmp(N * ncomp);
  HIPCHK(h, hipMemcpy(tmp.data(), dev, sizeof(double) * N * ncomp, hipMemcpyDeviceToHost));
  for (size_t e = 0; e < N; e++) for (int k = 0; k < ncomp; k++) host[e * ncomp + k] = tmp[(size_t)k * N + e];
  return 0;
}
static int push(KHandle h, double* dev, const double* host, int ncomp) {
  if (!host) return 0;
  const size_t N = (size_t)h->num_envs;
  std::vector<double> tmp(N * ncomp);
  for (size_t e = 0; e < N; e++) for (int k = 0; k < ncomp; k++) tmp[(size_t)k * N + e] = host[e * ncomp + k];
  HIPCHK(h, hipMemcpy(dev, tmp.data(), sizeof(double) * N * ncomp, hipMemcpyHostToDevice));
  return 0;
}

int kmanip_get_state(KHandle h, double* qpos, double* qvel, double* ctrl, double* qacc_warm, int32_t* step_idx) {
  if (!h) return -1;
  KM_ENTER(h);
  HIPCHK(h, hipDeviceSynchronize());
  const int nl = h->desc.nlink;
  int rc = 0;
  if ((rc = pull(h, h->st.qpos, qpos, nl + 7))) return rc;
  if ((rc = pull(h, h->st.qvel, qvel, nl + 6))) return rc;
  if ((rc = pull(h, h->st.ctrl, ctrl, nl))) return rc;
  if ((rc = pull(h, h->st.warm, qacc_warm, nl + 6))) return rc;
  if (step_idx) HIPCHK(h, hipMemcpy(step_idx, h->st.step_idx, sizeof(int32_t) * h->num_envs, hipMemcpyDeviceToHost));
  return 0;
}
int kmanip_set_state(KHandle h, const double* qpos, const double* qvel, const double* ctrl, const double* qacc_warm,
                     const int32_t* step_idx) {
  if (!h) return -1;
  KM_ENTER(h);
  HIPCHK(h, hipDeviceSynchronize());
  const int nl = h->desc.nlink;
  int rc = 0;
  if ((rc = push(h, h->st.qpos, qpos, nl + 7))) return rc;
  if ((rc = push(h, h->st.qvel, qvel, nl + 6))) return rc;
  if ((rc = push(h, h->st.ctrl, ctrl, nl))) return rc;
  if ((rc = push(h, h->st.warm, qacc_warm, nl + 6))) return rc;
  if (step_idx) HIPCHK(h, hipMemcpy(h->st.step_idx, step_idx, sizeof(int32_t) * h->num_envs, hipMemcpyHostToDevice));
  HIPCHK(h, hipDeviceSynchronize());      // pageable-memory copies may return early; order them before the caller's streams
  return 0;
}

int kmanip_get_episode(KHandle h, int32_t* episode) {
  if (!h || !episode) { if (h) h->err = "kmanip_get_episode: null pointer"; return -1; }
  KM_ENTER(h);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(episode, h->st.episode, sizeof(int32_t) * h->num_envs, hipMemcpyDeviceToHost));
  return 0;
}
int kmanip_set_episode(KHandle h, const int32_t* episode) {
  if (!h || !episode) { if (h) h->err = "kmanip_set_episode: null pointer"; return -1; }
  KM_ENTER(h);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(h->st.episode, episode, sizeof(int32_t) * h->num_envs, hipMemcpyHostToDevice));
  HIPCHK(h, hipDeviceSynchronize());
  return 0;
}

int kmanip_bind_sim_time(KHandle h, double* sim_time_dev) {
  if (!h) return -1;
  h->st.sim_time = sim_time_dev;
  return 0;
}

int kmanip_bind_applied_force(KHandle h, const double* qfrc_dev) {
  if (!h) return -1;
  h->st.qfrc_applied = qfrc_dev;
  return 0;
}

int kmanip_bind_reward_done_record(KHandle h, double* rec0_dev, double* rec1_dev) {
  if (!h) return -1;
  if ((rec0_dev == nullptr) != (rec1_dev == nullptr)) { h->err = "kmanip_bind_reward_done_record: two buffers or none"; return -1; }
  h->rd_rec[0] = rec0_dev; h->rd_rec[1] = rec1_dev; h->rd_sel = 0;
  return 0;
}

int kmanip_select_reward_done_record(KHandle h, int index) {
  if (!h) return -1;
  if (index < 0 || index > 1 || !h->rd_rec[0]) { h->err = "kmanip_select_reward_done_record: index 0 / 1 of two bound buffers"; return -1; }
  h->rd_sel = index;
  return 0;
}

// the compiled model's values (mass, tangential cube friction, cube frictionloss, kp scale 1) into p [KM_EP_N][N]
static void ep_fill_model(KHandle h, double* p, hipStream_t stream) {
  const KModelDesc& d = h->desc;
  hipLaunchKernelGGL(k_ep_fill, dim3(ep_grid(h->num_envs)), dim3(256), 0, stream, p, h->num_envs, d.cube_mass, d.con_cube_friction[0],
                     d.cube_frictionloss, 1.0);
}
static hipError_t ep_alloc(KHandle h) {
  auto one = [&](void** p, size_t bytes) -> hipError_t {
    if (*p) return hipSuccess;
    hipError_t r = hipMalloc(p, bytes);
    if (r == hipSuccess) h->allocs.push_back(*p);
    return r;
  };
  hipError_t r = one((void**)&h->envp_buf, sizeof(double) * KM_EP_N * (size_t)h->num_envs);
  if (r == hipSuccess) r = one((void**)&h->ep_range_buf, sizeof(double) * 2 * KM_EP_N);
  if (r == hipSuccess) r = one((void**)&h->ep_flag, sizeof(int));
  return r;
}

int kmanip_set_env_params(KHandle h, const double* params_dev, void* stream) {
  if (!h) return -1;
  KM_ENTER(h);
  if (!params_dev) { h->st.envp = nullptr; h->st.ep_range = nullptr; return 0; }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(h, ep_alloc(h));
  int bad = 0;
  HIPCHK(h, hipMemsetAsync(h->ep_flag, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_ep_validate, dim3(ep_grid(h->num_envs)), dim3(256), 0, s, params_dev, h->num_envs, h->ep_flag);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(&bad, h->ep_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (bad) {
    h->err = "kmanip_set_env_params: every env needs cube mass > 0, cube friction >= 0, cube frictionloss >= 0, kp scale > 0, all finite";
    return -2;
  }
  // the parameter buffer may be read by a step in flight on any stream (as in kmanip_set_env_param_ranges)
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(h->envp_buf, params_dev, sizeof(double) * KM_EP_N * (size_t)h->num_envs, hipMemcpyDeviceToDevice));
  HIPCHK(h, hipDeviceSynchronize());
  h->st.envp = h->envp_buf;
  h->st.ep_range = nullptr;
  return 0;
}

int kmanip_get_env_params(KHandle h, double* params_dev, void* stream) {
  if (!h || !params_dev) { if (h) h->err = "kmanip_get_env_params: params_dev is NULL"; return -1; }
  KM_ENTER(h);
  hipStream_t s = (hipStream_t)stream;
  if (h->st.envp) HIPCHK(h, hipMemcpyAsync(params_dev, h->st.envp, sizeof(double) * KM_EP_N * (size_t)h->num_envs, hipMemcpyDeviceToDevice, s));
  else ep_fill_model(h, params_dev, s);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_set_env_param_ranges(KHandle h, const double* lo, const double* hi) {
  if (!h) return -1;
  if (!lo && !hi) { h->st.ep_range = nullptr; return 0; }
  if (!lo || !hi) { h->err = "kmanip_set_env_param_ranges: lo and hi must both be NULL or both be set"; return -1; }
  for (int k = 0; k < KM_EP_N; k++) {
    if (!ep_value_ok(k, lo[k]) || !ep_value_ok(k, hi[k]) || lo[k] > hi[k]) {
      h->err = "kmanip_set_env_param_ranges: parameter " + std::to_string(k) + " needs finite lo <= hi within its limits "
               "(cube mass > 0, cube friction >= 0, cube frictionloss >= 0, kp scale > 0)";
      return -2;
    }
  }
  KM_ENTER(h);
  HIPCHK(h, ep_alloc(h));
  // the range buffer may be read by a step in flight on any stream
  HIPCHK(h, hipDeviceSynchronize());
  double r[2 * KM_EP_N];
  for (int k = 0; k < KM_EP_N; k++) { r[k] = lo[k]; r[KM_EP_N + k] = hi[k]; }
  HIPCHK(h, hipMemcpy(h->ep_range_buf, r, sizeof r, hipMemcpyHostToDevice));
  if (!h->st.envp) {          // until an env's next reset it keeps the values in force: the compiled model's
    ep_fill_model(h, h->envp_buf, nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipDeviceSynchronize());
  }
  h->st.envp = h->envp_buf;
  h->st.ep_range = h->ep_range_buf;
  return 0;
}

static hipError_t vp_alloc(KHandle h) {
  auto one = [&](void** p, size_t bytes) -> hipError_t {
    if (*p) return hipSuccess;
    hipError_t r = hipMalloc(p, bytes);
    if (r == hipSuccess) h->allocs.push_back(*p);
    return r;
  };
  hipError_t r = one((void**)&h->vp_buf, sizeof(double) * KM_VP_N * (size_t)h->num_envs);
  if (r == hipSuccess) r = one((void**)&h->vp_range_buf, sizeof(double) * 2 * KM_VP_N);
  if (r == hipSuccess) r = one((void**)&h->vp_flag, sizeof(int));
  return r;
}

int kmanip_set_visual_params(KHandle h, const double* params_dev, void* stream) {
  if (!h) return -1;
  KM_ENTER(h);
  // a render in flight on any stream may read the buffers: every change waits for the device
  if (!params_dev) { HIPCHK(h, hipDeviceSynchronize()); h->vis = KVisArgs{}; return 0; }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(h, vp_alloc(h));
  int bad = 0;
  HIPCHK(h, hipMemsetAsync(h->vp_flag, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_vp_validate, dim3(ep_grid(h->num_envs)), dim3(256), 0, s, params_dev, h->num_envs, h->vp_flag);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(&bad, h->vp_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (bad) {
    h->err = "kmanip_set_visual_params: every env needs colours in [0, 1], finite light terms >= 0 and camera offsets within +-0.25 m";
    return -2;
  }
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(h->vp_buf, params_dev, sizeof(double) * KM_VP_N * (size_t)h->num_envs, hipMemcpyDeviceToDevice));
  HIPCHK(h, hipDeviceSynchronize());
  h->vis = KVisArgs{h->vp_buf, nullptr, nullptr};
  return 0;
}

int kmanip_get_visual_params(KHandle h, double* params_dev, void* stream) {
  if (!h || !params_dev) { if (h) h->err = "kmanip_get_visual_params: params_dev is NULL"; return -1; }
  KM_ENTER(h);
  hipStream_t s = (hipStream_t)stream;
  if (h->vis.range) kmanip_launch_vp_draw(h->st, vis_args(h, -1), params_dev, s);
  else if (h->vis.vp) HIPCHK(h, hipMemcpyAsync(params_dev, h->vis.vp, sizeof(double) * KM_VP_N * (size_t)h->num_envs, hipMemcpyDeviceToDevice, s));
  else hipLaunchKernelGGL(k_vp_fill_defaults, dim3(ep_grid(h->num_envs)), dim3(256), 0, s, params_dev, h->num_envs);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_set_visual_param_ranges(KHandle h, const double* lo, const double* hi) {
  if (!h) return -1;
  if (!lo && !hi) {
    if (!h->vis.range) return 0;
    // ranges mode off: every env keeps its current episode's draw, as explicit values
    KM_ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());
    kmanip_launch_vp_draw(h->st, vis_args(h, -1), h->vp_buf, nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipDeviceSynchronize());
    h->vis = KVisArgs{h->vp_buf, nullptr, nullptr};
    return 0;
  }
  if (!lo || !hi) { h->err = "kmanip_set_visual_param_ranges: lo and hi must both be NULL or both be set"; return -1; }
  for (int k = 0; k < KM_VP_N; k++) {
    if (!vp_value_ok(k, lo[k]) || !vp_value_ok(k, hi[k]) || lo[k] > hi[k]) {
      h->err = "kmanip_set_visual_param_ranges: parameter " + std::to_string(k) + " needs finite lo <= hi within its limits "
               "(colours in [0, 1], light terms >= 0, camera offsets within +-0.25 m)";
      return -2;
    }
  }
  KM_ENTER(h);
  HIPCHK(h, vp_alloc(h));
  HIPCHK(h, hipDeviceSynchronize());
  double r[2 * KM_VP_N];
  for (int k = 0; k < KM_VP_N; k++) { r[k] = lo[k]; r[KM_VP_N + k] = hi[k]; }
  HIPCHK(h, hipMemcpy(h->vp_range_buf, r, sizeof r, hipMemcpyHostToDevice));
  HIPCHK(h, hipDeviceSynchronize());
  h->vis = KVisArgs{nullptr, h->vp_range_buf, nullptr};
  h->ep_snap_ok[0] = h->ep_snap_ok[1] = false;
  return 0;
}

int kmanip_set_seed(KHandle h, uint64_t seed, int restart_episodes) {
  if (!h) return -1;
  KM_ENTER(h);
  h->st.seed = seed;
  if (restart_episodes) {
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemset(h->st.episode, 0xFF, sizeof(int32_t) * (size_t)h->num_envs));   // -1: the next reset is episode 0
    HIPCHK(h, hipDeviceSynchronize());
  }
  return 0;
}

int kmanip_get_counters(KHandle h, int32_t* step_idx_dev, int32_t* episode_dev, void* stream) {
  if (!h) return -1;
  KM_ENTER(h);
  const size_t bytes = sizeof(int32_t) * (size_t)h->num_envs;
  if (step_idx_dev) HIPCHK(h, hipMemcpyAsync(step_idx_dev, h->st.step_idx, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (episode_dev) HIPCHK(h, hipMemcpyAsync(episode_dev, h->st.episode, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int kmanip_get_diag(KHandle h, uint32_t* contact_mask, int32_t* ik_nfev, int32_t* ik_status) {
  if (!h) return -1;
  KM_ENTER(h);
  HIPCHK(h, hipDeviceSynchronize());
  const size_t N = (size_t)h->num_envs;
  if (contact_mask) HIPCHK(h, hipMemcpy(contact_mask, h->st.contact_mask, sizeof(uint32_t) * N, hipMemcpyDeviceToHost));
  std::vector<int32_t> tmp(2 * N);
  if (ik_nfev) {
    HIPCHK(h, hipMemcpy(tmp.data(), h->st.ik_nfev, sizeof(int32_t) * 2 * N, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < N; e++) { ik_nfev[2 * e] = tmp[e]; ik_nfev[2 * e + 1] = tmp[N + e]; }
  }
  if (ik_status) {
    HIPCHK(h, hipMemcpy(tmp.data(), h->st.ik_status, sizeof(int32_t) * 2 * N, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < N; e++) { ik_status[2 * e] = tmp[e]; ik_status[2 * e + 1] = tmp[N + e]; }
  }
  return 0;
}

int kmanip_ik(KHandle h, int arm, int n, double* qpos, const double* goal_pos, const double* goal_quat, double* q_out,
              int32_t* nfev, int32_t* status) {
  if (!h) { g_create_error = "kmanip_ik: null handle"; return -1; }
  if (arm < 0 || arm >= KM_MAX_ARMS || !h->desc.arm_present[arm] || n <= 0 || !qpos || !goal_pos || !goal_quat || !q_out) {
    h->err = "kmanip_ik: bad arguments"; return -1;
  }
  KM_ENTER(h);
  const int nq = h->desc.nlink + 7, nik = h->desc.arm_nq[arm];
  DevBuf dq, dgp, dgq, dqo, dnf, dst;        // freed on every exit path
  HIPCHK(h, hipMalloc(&dq.p, sizeof(double) * n * nq));
  HIPCHK(h, hipMalloc(&dgp.p, sizeof(double) * n * 3));
  HIPCHK(h, hipMalloc(&dgq.p, sizeof(double) * n * 4));
  HIPCHK(h, hipMalloc(&dqo.p, sizeof(double) * n * nik));
  HIPCHK(h, hipMalloc(&dnf.p, sizeof(int32_t) * n));
  HIPCHK(h, hipMalloc(&dst.p, sizeof(int32_t) * n));
  HIPCHK(h, hipMemcpy(dq.p, qpos, sizeof(double) * n * nq, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dgp.p, goal_pos, sizeof(double) * n * 3, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dgq.p, goal_quat, sizeof(double) * n * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipDeviceSynchronize());
  kmanip_launch_ik_coop_standalone(h->dmodel, h->desc, arm, n, dq.as<double>(), dgp.as<double>(), dgq.as<double>(), dqo.as<double>(), dnf.as<int32_t>(), dst.as<int32_t>(), nullptr);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(qpos, dq.p, sizeof(double) * n * nq, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(q_out, dqo.p, sizeof(double) * n * nik, hipMemcpyDeviceToHost));
  if (nfev) HIPCHK(h, hipMemcpy(nfev, dnf.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (status) HIPCHK(h, hipMemcpy(status, dst.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return 0;
}

int kmanip_ik_eval(KHandle h, int arm, int n, const double* qpos, const double* goal_pos, const double* goal_quat,
                   double* res, double* jac) {
  if (!h) { g_create_error = "kmanip_ik_eval: null handle"; return -1; }
  if (arm < 0 || arm >= KM_MAX_ARMS || !h->desc.arm_present[arm] || n <= 0 || !qpos || !goal_pos || !goal_quat || !res || !jac) {
    h->err = "kmanip_ik_eval: bad arguments"; return -1;
  }
  KM_ENTER(h);
  const int nq = h->desc.nlink + 7, nik = h->desc.arm_nq[arm], mrow = 6 + 2 * nik;
  DevBuf dq, dgp, dgq, dres, djac;
  HIPCHK(h, hipMalloc(&dq.p, sizeof(double) * n * nq));
  HIPCHK(h, hipMalloc(&dgp.p, sizeof(double) * n * 3));
  HIPCHK(h, hipMalloc(&dgq.p, sizeof(double) * n * 4));
  HIPCHK(h, hipMalloc(&dres.p, sizeof(double) * n * mrow));
  HIPCHK(h, hipMalloc(&djac.p, sizeof(double) * n * mrow * nik));
  HIPCHK(h, hipMemcpy(dq.p, qpos, sizeof(double) * n * nq, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dgp.p, goal_pos, sizeof(double) * n * 3, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dgq.p, goal_quat, sizeof(double) * n * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipDeviceSynchronize());
  kmanip_launch_ik_eval_coop(h->dmodel, h->desc, arm, n, dq.as<double>(), dgp.as<double>(), dgq.as<double>(), dres.as<double>(), djac.as<double>(), nullptr);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(res, dres.p, sizeof(double) * n * mrow, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(jac, djac.p, sizeof(double) * n * mrow * nik, hipMemcpyDeviceToHost));
  return 0;
}

// ---- the state on the device (include/kmanip.h KStateDev; kmanip_state.hip)
// the handle's live state as one side of a transfer (episode / sim_time: NULL where the call does not write them)
static KStateSide state_side(KHandle h, const int32_t* index) {
  KStateSide s{};
  s.f[0] = h->st.qpos; s.f[1] = h->st.qvel; s.f[2] = h->st.ctrl; s.f[3] = h->st.warm; s.f[4] = h->st.envp;
  s.step = h->st.step_idx; s.episode = h->st.episode;
  s.index = index;
  s.sim_time = h->st.sim_time; s.control_dt = h->st.control_dt;
  s.stride = s.range = h->num_envs;
  return s;
}
static int state_dev_args(KHandle h, const char* what, const int32_t* index, int n, const KStateDev* io) {
  if (!io) { h->err = std::string(what) + ": the KStateDev pointer is NULL"; return -1; }
  if (n < 0) { h->err = std::string(what) + ": n must be >= 0"; return -1; }
  if (!index && n > h->num_envs) { h->err = std::string(what) + ": n > num_envs with a NULL index"; return -1; }
  return 0;
}
static KStateSide tensor_side(const KStateDev* io, const int32_t* index) {
  KStateSide t{};
  t.f[0] = io->qpos; t.f[1] = io->qvel; t.f[2] = io->ctrl; t.f[3] = io->qacc_warm;
  t.step = io->step_idx; t.episode = io->episode;
  t.index = index;
  return t;
}

int kmanip_get_state_dev(KHandle h, const int32_t* env_index_dev, int n, const KStateDev* out, void* stream) {
  if (!h) { g_create_error = "kmanip_get_state_dev: null handle"; return -1; }
  if (state_dev_args(h, "kmanip_get_state_dev", env_index_dev, n, out)) return -1;
  if (n == 0) return 0;
  KM_ENTER(h);
  kmanip_launch_state_io(h->desc, state_side(h, nullptr), tensor_side(out, env_index_dev), n, false, h->index_errors, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_set_state_dev(KHandle h, const int32_t* env_index_dev, int n, const KStateDev* in, void* stream) {
  if (!h) { g_create_error = "kmanip_set_state_dev: null handle"; return -1; }
  if (state_dev_args(h, "kmanip_set_state_dev", env_index_dev, n, in)) return -1;
  if (n == 0) return 0;
  KM_ENTER(h);
  kmanip_launch_state_io(h->desc, state_side(h, nullptr), tensor_side(in, env_index_dev), n, true, h->index_errors, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int kmanip_copy_envs(KHandle dst, const int32_t* dst_index_dev, KHandle src, const int32_t* src_index_dev, int n, unsigned flags, void* stream) {
  if (!dst) { g_create_error = "kmanip_copy_envs: null destination handle"; return -1; }
  if (!src) { dst->err = "kmanip_copy_envs: null source handle"; return -1; }
  if (n < 0) { dst->err = "kmanip_copy_envs: n must be >= 0"; return -1; }
  if (flags & ~(unsigned)(KM_COPY_EPISODE | KM_COPY_ENV_PARAMS)) { dst->err = "kmanip_copy_envs: unknown flag"; return -1; }
  if ((!dst_index_dev && n > dst->num_envs) || (!src_index_dev && n > src->num_envs)) { dst->err = "kmanip_copy_envs: n > num_envs with a NULL index"; return -1; }
  if (dst->device != src->device) { dst->err = "kmanip_copy_envs: the two handles are on different devices"; return -1; }
  if (memcmp(&dst->desc, &src->desc, sizeof(KModelDesc)) != 0) { dst->err = "kmanip_copy_envs: the two handles were created from different KModelDesc"; return -1; }
  bool params = false;
  if (flags & KM_COPY_ENV_PARAMS) {
    if (src->st.envp && !dst->st.envp) { dst->err = "kmanip_copy_envs: destination has no per-env parameters: call kmanip_set_env_params first"; return -2; }
    params = dst->st.envp != nullptr;           // (neither has them: the flag does nothing)
  }
  if (n == 0) return 0;
  KM_ENTER(dst);
  hipStream_t s = (hipStream_t)stream;
  const KModelDesc& d = dst->desc;
  const KEnvParamDefaults model{{d.cube_mass, d.con_cube_friction[0], d.cube_frictionloss, 1.0}};
  KStateSide to = state_side(dst, dst_index_dev), from = state_side(src, src_index_dev);
  if (!(flags & KM_COPY_EPISODE)) to.episode = nullptr;
  if (dst != src) {
    kmanip_launch_state_gather(d, to, from, n, params, model, dst->index_errors, s);
    HIPCHK(dst, hipGetLastError());
    return 0;
  }
  // Same handle: every source row is read before any is written -- rows 0 .. n-1 go into the staging copy (first launch, nothing
  // counted), and from there into their destination envs (second launch: both indices checked, bad entries counted once).
  if (dst->stage_cap < n) {
    // (the first such call, or one with more entries than any before: the only path here that allocates, and so synchronises)
    const int cap = n > dst->num_envs ? n : dst->num_envs;
    const int comps = 4 * d.nlink + 19 + KM_EP_N;
    HIPCHK(dst, hipDeviceSynchronize());
    void* pd = nullptr; void* pi = nullptr;
    HIPCHK(dst, hipMalloc(&pd, sizeof(double) * (size_t)comps * cap));
    dst->allocs.push_back(pd);
    HIPCHK(dst, hipMalloc(&pi, sizeof(int32_t) * 2 * (size_t)cap));
    dst->allocs.push_back(pi);
    dst->stage_buf = (double*)pd; dst->stage_cnt = (int32_t*)pi; dst->stage_cap = cap;     // (a smaller one stays in allocs until kmanip_destroy)
  }
  KStateSide stage{};
  {
    const size_t cap = (size_t)dst->stage_cap;
    const int K[KS_NFIELD] = {d.nlink + 7, d.nlink + 6, d.nlink, d.nlink + 6, KM_EP_N};
    double* p = dst->stage_buf;
    for (int f = 0; f < KS_NFIELD; f++) { stage.f[f] = p; p += (size_t)K[f] * cap; }
    stage.step = dst->stage_cnt; stage.episode = dst->stage_cnt + cap;
    stage.stride = stage.range = dst->stage_cap;
    stage.staged = 1;
  }
  kmanip_launch_state_gather(d, stage, from, n, params, model, nullptr, s);
  stage.index = src_index_dev; stage.range = src->num_envs;          // (checked again, so that a bad source entry is skipped and counted here)
  kmanip_launch_state_gather(d, to, stage, n, params, model, dst->index_errors, s);
  HIPCHK(dst, hipGetLastError());
  return 0;
}

int kmanip_state_index_errors(KHandle h, int64_t* count) {
  if (!h) { g_create_error = "kmanip_state_index_errors: null handle"; return -1; }
  if (!count) { h->err = "kmanip_state_index_errors: count is NULL"; return -1; }
  KM_ENTER(h);
  unsigned long long c = 0;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(&c, h->index_errors, sizeof c, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->index_errors, 0, sizeof c));
  HIPCHK(h, hipDeviceSynchronize());
  *count = (int64_t)c;
  return 0;
}

}  // extern "C"
