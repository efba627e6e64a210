// kmanip_render_points.hip -- camera geometry out of the library:
//   k_camera_poses  : MuJoCo's cam_xpos / cam_xmat of one camera, per env, as the renders build it (kmanip_get_camera_poses)
//   k_render_points : the float64 depth ray cast with the pixel's point stored as float32 XYZ in the camera or the world frame, and
//                     the depth image from the same launch if wanted (kmanip_render_points)
// A translation unit of its own with its own copy of the pixel loop, as kmanip_render_labels.hip, kmanip_render_links.hip and
// kmanip_render_depth_links.hip are: the code the compiler emits for the existing render kernels does not change (section 16 says
// why it is a copy).  The loop is k_render_depth_links' (kmanip_render_depth_links.hip) line for line, the capsule block behind
// `if constexpr (LINKS)`; a change to a hit test there or in k_render_depth (kmanip_render.hip) belongs here too --
// tests/test_points_gpu.py holds the depth of this kernel to kmanip_render_depth's.
#include "kmanip_render_scene.hpp"

// ---- camera poses -----------------------------------------------------------------------------------------------------
// One workgroup of 128 lanes per env (what render_fk's lane roles need: links 0.., spheres 64.., visual parameters 96..): the FK and
// the camera frame of the renders, then twelve lanes store.  Launch-latency sized.
template <bool VIS, class... VA>
__global__ __launch_bounds__(128) void k_camera_poses(const KDeviceModel* __restrict__ dm, KDeviceState st, int cam, double* __restrict__ pose, VA... vargs) {
  static_assert(sizeof...(VA) == (VIS ? 1 : 0), "the VIS kernel takes one KVisArgs, the default kernel none");
  __shared__ RenderScene sc;
  __shared__ double vsv_[KM_VP_N];           // (VIS only)
  KVisArgs va{};
  double* vsv = nullptr;
  if constexpr (VIS) { ((va = vargs), ...); vsv = vsv_; }
  const int env = blockIdx.x;
  RenderPre pre;
  render_fk<VIS>(dm, st, env, cam, &sc, pre, va, vsv);
  render_camera<VIS>(dm, st, env, cam, 2, &sc, pre, vsv);       // (the height only scales sc.focal, which is not read here)
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 12) {
    // origin, then the row-major matrix whose columns are the camera's x, y, z axes
    real v;
    if (t < 3) v = sc.cam_o[t];
    else {
      const int r = (t - 3) / 3, c = (t - 3) - 3 * r;
      v = c == 0 ? sc.cam_x[r] : (c == 1 ? sc.cam_y[r] : sc.cam_z[r]);
    }
    pose[(size_t)env * 12 + t] = v;
  }
}

void kmanip_launch_camera_poses(const KDeviceModel* dm, const KDeviceState& st, int cam, double* pose, const KVisArgs& vis, hipStream_t stream) {
  const dim3 grid(st.num_envs), block(128);
  if (km_vis_on(vis)) k_camera_poses<true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, cam, pose, vis);
  else k_camera_poses<false><<<grid, block, 0, stream>>>(dm, st, cam, pose);
}

// ---- points -----------------------------------------------------------------------------------------------------------
// (k_render_depth_links' DepthLinkScene / DepthCap / dl_uniform / depth_link_setup: private copies, see the head of the file)
struct PointScene { real ol[3], DX[3], DY[3], DZ[3]; real oc[KM_RENDER_MAXVIS][3], cc[KM_RENDER_MAXVIS]; int nvis; };

struct alignas(16) PointCap {
  real u[3], oa[3];
  real ou, len;                // oa.u, |B - A|
  real c, ca, cb;              // oa.oa - ou^2 - r^2; the end spheres' |oa|^2 - r^2, |ob|^2 - r^2
  int box[4];                  // screen rectangle r0, r1, c0, c1 (inclusive); r0 > r1: never tested
};
#define KM_PT_LANE0 72                 // one capsule per lane of the second wave (lanes 72 .. 95: idle after the FK)
static_assert(KM_PT_LANE0 >= 64 + KM_RENDER_MAXVIS && KM_PT_LANE0 + KM_MAX_LINK_CAPSULES <= 128, "one capsule per lane of the second wave");
static_assert(KM_MAX_LINK_CAPSULES <= 32, "the capsule masks are one uint32_t");

// a wave-uniform value moved into a scalar register pair (U = false: left where it is)
template <bool U>
__device__ __forceinline__ real pt_uniform(real x) {
  if constexpr (!U) return x;
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return __builtin_bit_cast(real, (uint64_t)hi << 32 | lo);
}

// a pixel's point: three floats at a 4-byte aligned address, stored as ONE 12-byte access
struct __attribute__((packed, aligned(4))) PointXYZ { float x, y, z; };

// capsule k of the list: ray constants and screen rectangle (depth_link_setup of kmanip_render_depth_links.hip)
__device__ __forceinline__ void point_link_setup(const RenderScene& sc, const KLinkCapsule& cp, int cam, int height, int width, PointCap* dc) {
  const int l = cp.link;
  const real rad = cp.radius;
  real v[3], A[3], B[3], sv[3];
  mat_vec3(v, sc.xmat[l], cp.p0);
  mat_vec3(sv, sc.xmat[l], cp.seg);
  for (int c = 0; c < 3; c++) { A[c] = sc.xpos[l][c] + v[c]; B[c] = A[c] + sv[c]; }
  const real L = sqrt(dot3(sv, sv));
  real u[3] = {0, 0, 1};
  if (L > 0) { for (int c = 0; c < 3; c++) u[c] = sv[c] / L; }
  real oa[3], ob[3];
  for (int c = 0; c < 3; c++) { oa[c] = sc.cam_o[c] - A[c]; ob[c] = sc.cam_o[c] - B[c]; }
  const real ou = dot3(oa, u), r2 = rad * rad;
  for (int c = 0; c < 3; c++) { dc->u[c] = u[c]; dc->oa[c] = oa[c]; }
  dc->ou = ou; dc->len = L;
  dc->c = dot3(oa, oa) - ou * ou - r2;
  dc->ca = dot3(oa, oa) - r2;
  dc->cb = dot3(ob, ob) - r2;
  int* box = dc->box;
  const real za = dot3(oa, sc.cam_z), zb = dot3(ob, sc.cam_z);               // depth of the end points along the optical axis
  if (!(cp.cam_mask >> cam & 1u) || (za + rad <= 0 && zb + rad <= 0)) { box[0] = height; box[1] = -1; box[2] = width; box[3] = -1; return; }
  real r0 = 1e30, r1 = -1e30, c0 = 1e30, c1 = -1e30;
  bool ok = true;
  for (int e = 0; e < 2; e++) {
    const real* E = e ? B : A;
    const real zc = e ? zb : za;
    real row = 0, col = 0;
    const bool oke = rgb_project(sc, E, height, width, row, col) && zc - rad > 1e-3;
    const real pr = oke ? 1.5 * sc.focal * rad / (zc - rad) + 1.0 : 0.0;     // (rgb_scene's generous radius)
    ok = ok && oke;
    r0 = fmin(r0, row - pr); r1 = fmax(r1, row + pr); c0 = fmin(c0, col - pr); c1 = fmax(c1, col + pr);
  }
  if (!ok) { box[0] = 0; box[1] = height - 1; box[2] = 0; box[3] = width - 1; return; }
  box[0] = (int)fmin(fmax(floor(r0) - 1, -1.0), (real)height); box[1] = (int)fmax(fmin(ceil(r1) + 1, (real)height), -1.0);
  box[2] = (int)fmin(fmax(floor(c0) - 1, -1.0), (real)width); box[3] = (int)fmax(fmin(ceil(c1) + 1, (real)width), -1.0);
}

// The pixel's ray is o + t d, d = X dx + Y dy - Z with dx = (c + 0.5 - W/2) / f, dy = -(r + 0.5 - H/2) / f; D = the depth the depth
// render computes (nearest hit, clipped to [znear, zfar] in float64, no hit = zfar).  Stored per pixel:
//   camera frame  (float)(D dx), (float)(D dy), (float)(-D)
//   world frame   (float)(o + D d), in float64 and rounded once -- d is the direction the ray cast itself used
//   depth (if wanted)  (float)D: casting and clamping are monotonic, so this is kmanip_render_depth's clamp of the cast
// LINKS = false: the scene of k_render_depth; LINKS = true: plus the capsules of `la`, as k_render_depth_links tests them.
template <bool COLFIXED, bool VIS, bool LINKS, class... VA>
__global__ __launch_bounds__(256, 4) void k_render_points(const KDeviceModel* __restrict__ dm, KDeviceState st, int cam, int height, int width, int world,
                                                       float* __restrict__ xyz, float* __restrict__ depth, KLinkArgs la, VA... vargs) {
  static_assert(sizeof...(VA) == (VIS ? 1 : 0), "the VIS kernel takes one KVisArgs, the default kernel none");
  __shared__ RenderScene sc;
  __shared__ PointScene ds;
  __shared__ PointCap caps[LINKS ? KM_MAX_LINK_CAPSULES : 1];
  __shared__ double vsv_[KM_VP_N];           // (VIS only: the default kernel never references it)
  KVisArgs va{};
  double* vsv = nullptr;
  if constexpr (VIS) { ((va = vargs), ...); vsv = vsv_; }
  const KModelDesc* m = &dm->d;
  const int env = blockIdx.x;
  const int ncap = LINKS ? (la.n < KM_MAX_LINK_CAPSULES ? la.n : KM_MAX_LINK_CAPSULES) : 0;
  // model scalars of the pixel loop: wave-uniform reads, issued in front of the set-up
  const real zfar = m->cam_zfar, znear = m->cam_znear, tabz = m->table_z;
  const real rx0 = m->table_rect[0], rx1 = m->table_rect[1], ry0 = m->table_rect[2], ry1 = m->table_rect[3];
  const real hf0 = m->cube_half[0], hf1 = m->cube_half[1], hf2 = m->cube_half[2];
  // the capsule of this lane, read with the kinematics' inputs (used after the FK's barriers)
  const int ck = (int)threadIdx.x - KM_PT_LANE0;
  const bool cap_lane = LINKS && ck >= 0 && ck < ncap;
  KLinkCapsule cp{};
  if constexpr (LINKS) cp = la.caps[cap_lane ? ck : 0];
  RenderPre pre;
  render_fk<VIS>(dm, st, env, cam, &sc, pre, va, vsv);
  render_camera<VIS>(dm, st, env, cam, height, &sc, pre, vsv);
  __syncthreads();
  if (threadIdx.x < 4) {
    // ray origin and basis in the cube frame, one vector per lane
    const int k = threadIdx.x;
    const real rel[3] = {sc.cam_o[0] - sc.cube_p[0], sc.cam_o[1] - sc.cube_p[1], sc.cam_o[2] - sc.cube_p[2]};
    const real* src = k == 0 ? rel : (k == 1 ? sc.cam_x : (k == 2 ? sc.cam_y : sc.cam_z));
    real* dst = k == 0 ? ds.ol : (k == 1 ? ds.DX : (k == 2 ? ds.DY : ds.DZ));
    matT_vec3(dst, sc.cube_R, src);
  } else if (threadIdx.x >= 64 && threadIdx.x < 64 + KM_RENDER_MAXVIS) {
    const int ns = threadIdx.x - 64;
    if (ns == 0) ds.nvis = dm->x.nvis;
    if (ns < dm->x.nvis) {
      const int sp = dm->x.vis_sphere[ns];
      const real rad = m->sphere_radius[sp];
      const real oc[3] = {sc.cam_o[0] - sc.sph[sp][0], sc.cam_o[1] - sc.sph[sp][1], sc.cam_o[2] - sc.sph[sp][2]};
      ds.oc[ns][0] = oc[0]; ds.oc[ns][1] = oc[1]; ds.oc[ns][2] = oc[2];
      ds.cc[ns] = dot3(oc, oc) - rad * rad;
    }
  } else if (cap_lane) point_link_setup(sc, cp, cam, height, width, &caps[ck]);
  __syncthreads();
  // ---- everything the pixel loop reads of the scene without capsules, in registers.  Which of the wave-uniform values go into
  // scalar registers is chosen per instantiation so that neither register file spills inside the loop at four waves per SIMD: with
  // capsules all of them, as in k_render_depth_links (the record's 22 vector registers); without capsules none in the COLFIXED loop
  // (k_render_depth's registers) and the sphere constants alone in the general one (all forty in scalar registers spilled those, and
  // their reloads in the loop cost a lone wave more than the stores)
  constexpr bool UA = LINKS && COLFIXED, UD = LINKS, US = LINKS || !COLFIXED;     // (camera basis and origin; cube-frame basis; spheres)
  const real oz = pt_uniform<UA>(sc.cam_o[2]);
  const real k0 = pt_uniform<UA>(tabz - sc.cam_o[2]), ox = pt_uniform<UA>(sc.cam_o[0]), oy = pt_uniform<UA>(sc.cam_o[1]);
  real X[3], Y[3], Z[3], ol[3], DX[3], DY[3], DZ[3];
  const real hf[3] = {hf0, hf1, hf2};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    X[c] = pt_uniform<UA>(sc.cam_x[c]); Y[c] = pt_uniform<UA>(sc.cam_y[c]); Z[c] = pt_uniform<UA>(sc.cam_z[c]);
    ol[c] = ds.ol[c]; DX[c] = pt_uniform<UD>(ds.DX[c]); DY[c] = pt_uniform<UD>(ds.DY[c]); DZ[c] = pt_uniform<UD>(ds.DZ[c]);
  }
  // |camera - cube centre|^2 - (bounding radius)^2, the radius padded by a relative 1e-9 so that roundoff never rejects a grazing ray
  const real cube_cc = (ol[0] * ol[0] + ol[1] * ol[1] + ol[2] * ol[2]) - (hf[0] * hf[0] + hf[1] * hf[1] + hf[2] * hf[2]) * (1.0 + 1e-9);
  const int nvis = ds.nvis;
  real soc[KM_RENDER_MAXVIS][3], scc[KM_RENDER_MAXVIS];
#pragma unroll
  for (int s = 0; s < KM_RENDER_MAXVIS; s++) {
    const int k = s < nvis ? s : 0;                      // (unused entries: finite copies, never tested)
    soc[s][0] = pt_uniform<US>(ds.oc[k][0]); soc[s][1] = pt_uniform<US>(ds.oc[k][1]); soc[s][2] = pt_uniform<US>(ds.oc[k][2]); scc[s] = pt_uniform<US>(ds.cc[k]);
  }
  const int npix = height * width;
  const real inv_f = 1.0 / sc.focal, hw = 0.5 * width, hh = 0.5 * height;
  int r = threadIdx.x / width, c = threadIdx.x - r * width;         // row / column advance incrementally (no division in the loop)
  const int dr = blockDim.x / width, dc = blockDim.x - dr * width;
  // ---- the capsules' rectangles: lane k of each wave keeps capsule k's row range; COLFIXED: bit k of colmask = this lane's column
  // is inside capsule k's column range
  const int wl = threadIdx.x & 63;
  int krow0 = height, krow1 = -1;                        // (lanes without a capsule: an empty range)
  uint32_t colmask = 0;
  if constexpr (LINKS) {
    if (wl < ncap) { krow0 = caps[wl].box[0]; krow1 = caps[wl].box[1]; }
    if constexpr (COLFIXED) {
      for (int k = 0; k < ncap; k++) colmask |= (uint32_t)(c >= caps[k].box[2] && c <= caps[k].box[3]) << k;
    }
  }
  // (COLFIXED: the wave's rows of a pass, scalar: its first lane's row and the rows 64 lanes span)
  int rw = __builtin_amdgcn_readfirstlane(r);
  const int rspan = COLFIXED ? (width < 64 ? 64 / width : 1) - 1 : 0;
  constexpr bool colfixed = COLFIXED;
  const real dxl = (c + 0.5 - hw) * inv_f;
  real ex[3], bx[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { ex[a] = X[a] * dxl - Z[a]; bx[a] = DX[a] * dxl - DZ[a]; }
  const real rel[3] = {sc.cam_o[0] - sc.cube_p[0], sc.cam_o[1] - sc.cube_p[1], sc.cam_o[2] - sc.cube_p[2]};   // (|rel| = |ol|)
  real A0 = 0, A1 = 0, A2 = 0, B0 = 0, B1 = 0, S0[KM_RENDER_MAXVIS], S1[KM_RENDER_MAXVIS];
#pragma unroll
  for (int s = 0; s < KM_RENDER_MAXVIS; s++) { S0[s] = 0; S1[s] = 0; }
  if constexpr (colfixed) {
    A0 = dot3(ex, ex); A1 = 2.0 * dot3(ex, Y); A2 = dot3(Y, Y);
    B0 = dot3(ex, rel); B1 = dot3(Y, rel);
#pragma unroll
    for (int s = 0; s < KM_RENDER_MAXVIS; s++) { S0[s] = dot3(ex, soc[s]); S1[s] = dot3(Y, soc[s]); }
  }
  // table rectangle by centre and half-widths (an unbounded side: the four-edge form below)
  const bool centred = isfinite(rx0) && isfinite(rx1) && isfinite(ry0) && isfinite(ry1);
  const real tcx = centred ? 0.5 * (rx0 + rx1) : 0.0, tcy = centred ? 0.5 * (ry0 + ry1) : 0.0;
  const real thx = 0.5 * (rx1 - rx0), thy = 0.5 * (ry1 - ry0);
  const real oxc = ox - tcx, oyc = oy - tcy;
  const real row0 = hh - 0.5;                            // dy = (row0 - r) / f
  real rd = (real)r;
  const real drd = (real)dr;
  real dyc = (row0 - rd) * inv_f;
  const real ddy = drd * inv_f;
  real zfv = zfar;
  asm volatile("" : "+v"(zfv));                          // (kept in a register pair: the selects below cannot take it from SGPRs next to VCC)
  auto rcp1 = [](real x) { real q = __builtin_amdgcn_rcp(x); return q + q * (1.0 - x * q); };
  // sqrt(x), x > 0, to 2^-46: v_rsq_f64 (2^-23) and one coupled step (g ~ sqrt x, h ~ 1 / (2 sqrt x): g += g (1/2 - g h)).
  // x = 0 gives NaN, which fails the comparisons of the hit it would have been (a ray tangent to a sphere to the last bit)
  auto sqrt1 = [](real x) { const real y = __builtin_amdgcn_rsq(x); const real g = x * y, h = 0.5 * y; return g + g * (0.5 - g * h); };
  // (a wave-uniform trip count: the loop control is scalar, the lane's pixel index one add)
  const int nit = (npix + (int)blockDim.x - 1) / (int)blockDim.x;
  PointXYZ* __restrict__ op = reinterpret_cast<PointXYZ*>(xyz) + (size_t)env * npix + threadIdx.x;
  const bool wd = depth != nullptr;                      // (wave-uniform: the depth store is behind a scalar branch)
  float* __restrict__ dp = (wd ? depth : xyz) + (size_t)env * npix + threadIdx.x;      // (advances with op; never written unless wd)
  const int pstep = blockDim.x;
  int p = threadIdx.x;
  for (int it = 0; it < nit; it++, p += pstep, op += pstep, dp += pstep) {
    // the capsules whose row range meets this wave's rows of the pass (every lane is active here: the ballot is the whole wave's)
    uint32_t wcaps = 0;
    if constexpr (LINKS) {
      int rwa, rwb;
      if constexpr (colfixed) { rwa = rw; rwb = rw + rspan; rw += dr; }
      else { rwa = __builtin_amdgcn_readfirstlane(r); rwb = __builtin_amdgcn_readlane(r, 63); }
      wcaps = (uint32_t)__ballot(rwb >= krow0 && rwa <= krow1);
    }
    const int rpix = r, cpix = c;                        // (general: this pixel's row and column, before they advance)
    real dx, dy, d0, d1, d2, a2, bc;
    if constexpr (colfixed) {
      dx = dxl; dy = dyc; dyc -= ddy;
      d0 = __builtin_fma(Y[0], dy, ex[0]); d1 = __builtin_fma(Y[1], dy, ex[1]); d2 = __builtin_fma(Y[2], dy, ex[2]);
      a2 = __builtin_fma(dy, __builtin_fma(dy, A2, A1), A0);
      bc = __builtin_fma(dy, B1, B0);
    } else {
      dx = (c + 0.5 - hw) * inv_f; dy = -(r + 0.5 - hh) * inv_f;
      c += dc; r += dr;
      if (c >= width) { c -= width; r++; }
      d0 = X[0] * dx + Y[0] * dy - Z[0]; d1 = X[1] * dx + Y[1] * dy - Z[1]; d2 = X[2] * dx + Y[2] * dy - Z[2];
      a2 = d0 * d0 + d1 * d1 + d2 * d2;
      bc = d0 * rel[0] + d1 * rel[1] + d2 * rel[2];
    }
    // table top: the rectangle table_rect at z = table_z.  d2 == 0 makes t infinite or NaN, which fails `t > 0 && t < zfar`; the
    // rectangle test is then never looked at (table_rect holds no NaN: kmanip_create checks)
    real best = zfv;
    {
      const real t = k0 * rcp1(d2);
      real in;
      if (centred) {
        const real hx = __builtin_fma(t, d0, oxc), hy = __builtin_fma(t, d1, oyc);
        in = fmin(thx - fabs(hx), thy - fabs(hy));
      } else {
        const real hx = __builtin_fma(t, d0, ox), hy = __builtin_fma(t, d1, oy);
        in = fmin(fmin(hx - rx0, rx1 - hx), fmin(hy - ry0, ry1 - hy));
      }
      if (t > 0 && t < zfar && in >= 0) best = t;
    }
    // cube box: slab test in the cube frame -- only for rays that meet the box's bounding sphere
    if (bc * bc - a2 * cube_cc >= 0) {
      real dlv[3];
#pragma unroll
      for (int a = 0; a < 3; a++) dlv[a] = colfixed ? __builtin_fma(DY[a], dy, bx[a]) : DX[a] * dx + DY[a] * dy - DZ[a];
      real t0 = -INFINITY, t1 = INFINITY;
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const real dl = dlv[a];
        if (dl != 0) {
          const real inv = rcp1(dl);
          const real ta = (-hf[a] - ol[a]) * inv, tb = (hf[a] - ol[a]) * inv;
          t0 = fmax(t0, fmin(ta, tb)); t1 = fmin(t1, fmax(ta, tb));
        } else if (ol[a] < -hf[a] || ol[a] > hf[a]) ok = false;
      }
      if (ok && t0 <= t1 && t1 > 0) {
        const real t = t0 > 0 ? t0 : t1;
        if (t < best) best = t;
      }
    }
    // the visible spheres (finger tips)
    const real ia2 = rcp1(a2);
#pragma unroll
    for (int s = 0; s < KM_RENDER_MAXVIS; s++) {
      if (s < nvis) {
        const real b = colfixed ? __builtin_fma(dy, S1[s], S0[s]) : d0 * soc[s][0] + d1 * soc[s][1] + d2 * soc[s][2];
        const real disc = b * b - a2 * scc[s];
        if (disc >= 0) {
          // nearest root; compared before the division: t < best  <=>  -b - sqrt(disc) < best * a2  (a2 > 0)
          const real num = -b - sqrt1(disc);
          if (num > 0 && num < best * a2) best = num * ia2;
        }
      }
    }
    // the link capsules, in list order: a scalar loop over the capsules this wave can meet
    if constexpr (LINKS) {
      while (wcaps) {
        const int k = __builtin_ctz(wcaps);
        wcaps &= wcaps - 1;
        const PointCap& q = caps[k];
        bool in;
        if constexpr (colfixed) in = colmask >> k & 1u;                                   // (rows: the wave's test above)
        else {
          const int b0 = q.box[0], b1 = q.box[1], b2 = q.box[2], b3 = q.box[3];         // (one read, no short-circuit chain of four)
          in = (rpix >= b0) & (rpix <= b1) & (cpix >= b2) & (cpix <= b3);
        }
        if (in) {
          // the record's reads, together and ahead of the arithmetic
          const real u0 = q.u[0], u1 = q.u[1], u2 = q.u[2], a0 = q.oa[0], a1 = q.oa[1], a2o = q.oa[2];
          const real ou = q.ou, len = q.len, cc = q.c, ca = q.ca, cb = q.cb;
          const real du = __builtin_fma(d0, u0, __builtin_fma(d1, u1, d2 * u2));
          const real dou = __builtin_fma(d0, a0, __builtin_fma(d1, a1, d2 * a2o));
          const real a = __builtin_fma(-du, du, a2), b = __builtin_fma(-du, ou, dou);
          const real h = __builtin_fma(b, b, -(a * cc));
          real num = INFINITY;                             // t |d|^2 of the end spheres' entry root, or of the body's t
          bool body = false;
          if (h >= 0) {
            const real tb = (-b - sqrt1(h)) * rcp1(a);
            const real sb = __builtin_fma(tb, du, ou);
            body = sb > 0 && sb < len;                     // (a = 0, the ray along the axis: tb is not finite, the test fails)
            if (body) num = tb * a2;
          }
          if (!body) {
            const real bb = __builtin_fma(-len, du, dou);                                 // d.ob, ob = oa - L u
            const real da = __builtin_fma(dou, dou, -(a2 * ca)), db = __builtin_fma(bb, bb, -(a2 * cb));
            const real na = da >= 0 ? -dou - sqrt1(da) : INFINITY, nb = db >= 0 ? -bb - sqrt1(db) : INFINITY;
            num = nb < na ? nb : na;
          }
          if (num > 0 && num < best * a2) best = num * ia2;
        }
      }
    }
    // ---- the pixel's point.  D: the clipped depth, float64.  best starts at zfar and only ever takes a smaller value (the table's
    // t < zfar, every other hit t < best), and it is never NaN (only comparisons that held assigned it): the clip is its lower half
    const real D = fmax(best, znear);
    if (COLFIXED || p < npix) {                          // (COLFIXED launches: npix is a multiple of the workgroup, checked by the launcher)
      PointXYZ P;
      if (world) {
        P.x = (float)__builtin_fma(D, d0, ox); P.y = (float)__builtin_fma(D, d1, oy); P.z = (float)__builtin_fma(D, d2, oz);
      } else {
        P.x = (float)(D * dx); P.y = (float)(D * dy); P.z = (float)(-D);
      }
      *op = P;
      if (wd) *dp = (float)D;
    }
  }
}

template <bool COLFIXED, bool LINKS>
static void launch_points(const KDeviceModel* dm, const KDeviceState& st, int cam, int height, int width, int world, float* xyz, float* depth,
                          const KLinkArgs& links, const KVisArgs& vis, hipStream_t stream) {
  const dim3 grid(st.num_envs), block(128);
  if (km_vis_on(vis)) k_render_points<COLFIXED, true, LINKS, KVisArgs><<<grid, block, 0, stream>>>(dm, st, cam, height, width, world, xyz, depth, links, vis);
  else k_render_points<COLFIXED, false, LINKS><<<grid, block, 0, stream>>>(dm, st, cam, height, width, world, xyz, depth, links);
}

void kmanip_launch_render_points(const KDeviceModel* dm, const KDeviceState& st, int cam, int height, int width, int world, float* xyz, float* depth,
                                 const KLinkArgs& links, const KVisArgs& vis, hipStream_t stream) {
  // k_render_depth's launch: 128 lanes per env, and its rule for the COLFIXED instantiation; links.n == 0: the scene without capsules
  const bool colfixed = width > 0 && 128 % width == 0 && (height * width) % 128 == 0;
  const bool wl = links.n > 0;
  if (colfixed) {
    if (wl) launch_points<true, true>(dm, st, cam, height, width, world, xyz, depth, links, vis, stream);
    else launch_points<true, false>(dm, st, cam, height, width, world, xyz, depth, links, vis, stream);
  } else {
    if (wl) launch_points<false, true>(dm, st, cam, height, width, world, xyz, depth, links, vis, stream);
    else launch_points<false, false>(dm, st, cam, height, width, world, xyz, depth, links, vis, stream);
  }
}
