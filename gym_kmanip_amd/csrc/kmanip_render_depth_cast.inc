// kmanip_render_depth_cast.inc -- the float64 depth ray cast, written once (DESIGN.md section 35).  A source fragment, not a header: no
// include guard, included exactly once by each of kmanip_render.hip, kmanip_render_depth_links.hip and kmanip_render_points.hip,
// behind kmanip_render_depth_cast.hpp and with KM_CAST_MODE set.  It spells ONE kernel, from its `template` line to its closing brace:
//   KM_CAST_DEPTH        k_render_depth<COLFIXED, VIS>              the scene (table, cube, visible spheres), a depth image
//   KM_CAST_DEPTH_LINKS  k_render_depth_links<COLFIXED, VIS>        plus the capsules of `la` in list order, a depth image
//   KM_CAST_POINTS       k_render_points<COLFIXED, VIS, LINKS>      either scene; the pixel's point and, if wanted, the depth image
// Only what differs between the three stands in #if regions (the signature, the scalar-register policy, the output pointers, the
// store), so that each object sees, after preprocessing, the statements of its own kernel in the order it had them: the three files'
// device code is, instruction for instruction, what their own copies of this text compiled to.  LINKS is a constant of the two depth
// kernels and a template parameter of k_render_points; the statements behind `if constexpr (LINKS)` are discarded where it is false.
//
// float64 ray maths (the parity bar against the float64 oracle is 1e-6 m; float32 intersection arithmetic cancels to ~1e-5 m).
// Round 4: the pixel loop was bound by what it FETCHED per pixel, not by its arithmetic -- scene constants re-read from LDS and
// model scalars from global memory inside the loop, a walk over all twelve collider spheres testing each one's `visible` flag.
// Now the per-env scene a ray meets is hoisted into registers once (camera basis and the same basis turned into the cube frame,
// so the slab test's direction is linear in the pixel coordinates; the visible spheres' centres from the host-built list), the
// divides are reciprocal + Newton steps, and nothing but the image is touched inside the loop.  (A float32 pre-classification
// with a float64 evaluation of the winner was built and measured first: 12 % of the pixels fell within its margins, i.e. nearly
// every wave ran both paths -- 0.155 ms against round 3's 0.089; dropped.)
//
// The capsules (DESIGN.md section 15) come after the visible spheres, in list order; a later object wins only where it is strictly
// nearer.  The capsule ray test is DESIGN.md section 14's, in float64 and in the direct form of the reference
// (tests/tools/link_oracle.py): body du = d.u, a = |d|^2 - du^2, b = d.oa - du ou, h = b^2 - a c, t = (-b - sqrt h) / a while
// 0 < ou + t du < L; otherwise the smaller entry root of the two end spheres (d.ob = d.oa - L du); only t > 0 counts.
// Culling: a capsule's arithmetic runs only for pixels inside its rectangle.  Lane k of every wave keeps capsule k's row range in two
// registers; per pass the wave's own row range is scalar, so one compare pair and its lane mask (a ballot) give the set of
// capsules the wave can meet as a scalar, and the loop below visits only those.  In the 64-wide COLFIXED case a wave is one image
// row and that test is exact; a lane's column test is one bit of a mask computed once (COLFIXED: the lane keeps its column) or a
// compare against the record's rectangle (general).
//
// k_render_points (DESIGN.md section 16): the pixel's ray is o + t d, d = X dx + Y dy - Z with dx = (c + 0.5 - W/2) / f,
// dy = -(r + 0.5 - H/2) / f; D = the depth the depth render computes (nearest hit, clipped to [znear, zfar] in float64, no hit =
// zfar).  Stored per pixel:
//   camera frame  (float)(D dx), (float)(D dy), (float)(-D)
//   world frame   (float)(o + D d), in float64 and rounded once -- d is the direction the ray cast itself used
//   depth (if wanted)  (float)D: casting and clamping are monotonic, so this is kmanip_render_depth's clamp of the cast
//
// COLFIXED: blockDim.x is a whole number of image rows (the launcher knows).  VIS = false: the default kernel (no VA);
// VIS = true: VA = KVisArgs, one more argument, and the camera offset applied
#if KM_CAST_MODE == KM_CAST_POINTS
template <bool COLFIXED, bool VIS, bool LINKS, class... VA>
__global__ __launch_bounds__(256, 4) void k_render_points(const KDeviceModel* __restrict__ dm, KDeviceState st, int cam, int height, int width, int world,
                                                       float* __restrict__ xyz, float* __restrict__ depth, KLinkArgs la, VA... vargs) {
#elif KM_CAST_MODE == KM_CAST_DEPTH_LINKS
template <bool COLFIXED, bool VIS, class... VA>
__global__ __launch_bounds__(256, 4) void k_render_depth_links(const KDeviceModel* __restrict__ dm, KDeviceState st, int cam, int height, int width,
                                                            float* __restrict__ depth, KLinkArgs la, VA... vargs) {
  constexpr bool LINKS = true;
#else
template <bool COLFIXED, bool VIS, class... VA>
__global__ __launch_bounds__(256, 4) void k_render_depth(const KDeviceModel* __restrict__ dm, KDeviceState st, int cam, int height, int width,
                                                      float* __restrict__ depth, VA... vargs) {
  constexpr bool LINKS = false;
  const KLinkArgs la{nullptr, 0};            // (no list: what the discarded statements below name)
#endif
  static_assert(sizeof...(VA) == (VIS ? 1 : 0), "the VIS kernel takes one KVisArgs, the default kernel none");
  __shared__ RenderScene sc;
  __shared__ DepthScene ds;
  __shared__ DepthCap caps[LINKS ? KM_MAX_LINK_CAPSULES : 1];      // (LINKS only: never referenced without, and no LDS there)
  __shared__ double vsv_[KM_VP_N];           // (VIS only: the default kernel never references it)
  KVisArgs va{};
  double* vsv = nullptr;
  if constexpr (VIS) { ((va = vargs), ...); vsv = vsv_; }
  const KModelDesc* m = &dm->d;
  const int env = blockIdx.x;
  const int ncap = LINKS ? (la.n < KM_MAX_LINK_CAPSULES ? la.n : KM_MAX_LINK_CAPSULES) : 0;
  // model scalars of the pixel loop: wave-uniform reads, issued in front of the set-up (they used to start after its last barrier)
  const real zfar = m->cam_zfar, znear = m->cam_znear, tabz = m->table_z;
  const real rx0 = m->table_rect[0], rx1 = m->table_rect[1], ry0 = m->table_rect[2], ry1 = m->table_rect[3];
  const real hf0 = m->cube_half[0], hf1 = m->cube_half[1], hf2 = m->cube_half[2];
  // the capsule of this lane, read with the kinematics' inputs (used after the FK's barriers)
  const int ck = (int)threadIdx.x - KM_CAP_LANE0;
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
  } else if (cap_lane) depth_link_setup(sc, cp, cam, height, width, &caps[ck]);
  __syncthreads();
  // ---- everything the pixel loop reads of the scene without capsules, in registers.  Which of the wave-uniform values go into
  // scalar registers (depth_uniform) is chosen per kernel so that neither register file spills inside the loop at four waves per
  // SIMD: with capsules all of them (the record's 22 vector registers); without capsules none in k_render_depth and in
  // k_render_points' COLFIXED loop, and the sphere constants alone in k_render_points' general one (all forty in scalar registers
  // spilled those, and their reloads in the loop cost a lone wave more than the stores)
#if KM_CAST_MODE == KM_CAST_POINTS
  constexpr bool UA = LINKS && COLFIXED, UD = LINKS, US = LINKS || !COLFIXED;     // (camera basis and origin; cube-frame basis; spheres)
#else
  constexpr bool UA = LINKS, UD = LINKS, US = LINKS;
#endif
  [[maybe_unused]] const real oz = depth_uniform<UA>(sc.cam_o[2]);                // (k_render_points' world frame)
  const real k0 = depth_uniform<UA>(tabz - sc.cam_o[2]), ox = depth_uniform<UA>(sc.cam_o[0]), oy = depth_uniform<UA>(sc.cam_o[1]);
  real X[3], Y[3], Z[3], ol[3], DX[3], DY[3], DZ[3];
  const real hf[3] = {hf0, hf1, hf2};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    X[c] = depth_uniform<UA>(sc.cam_x[c]); Y[c] = depth_uniform<UA>(sc.cam_y[c]); Z[c] = depth_uniform<UA>(sc.cam_z[c]);
    ol[c] = ds.ol[c]; DX[c] = depth_uniform<UD>(ds.DX[c]); DY[c] = depth_uniform<UD>(ds.DY[c]); DZ[c] = depth_uniform<UD>(ds.DZ[c]);
  }
  // |camera - cube centre|^2 - (bounding radius)^2, the radius padded by a relative 1e-9 so that roundoff never rejects a grazing ray
  const real cube_cc = (ol[0] * ol[0] + ol[1] * ol[1] + ol[2] * ol[2]) - (hf[0] * hf[0] + hf[1] * hf[1] + hf[2] * hf[2]) * (1.0 + 1e-9);
  const int nvis = ds.nvis;
  real soc[KM_RENDER_MAXVIS][3], scc[KM_RENDER_MAXVIS];
#pragma unroll
  for (int s = 0; s < KM_RENDER_MAXVIS; s++) {
    const int k = s < nvis ? s : 0;                      // (unused entries: finite copies, never tested)
    soc[s][0] = depth_uniform<US>(ds.oc[k][0]); soc[s][1] = depth_uniform<US>(ds.oc[k][1]); soc[s][2] = depth_uniform<US>(ds.oc[k][2]);
    scc[s] = depth_uniform<US>(ds.cc[k]);
  }
  const int npix = height * width;
  const real inv_f = 1.0 / sc.focal, hw = 0.5 * width, hh = 0.5 * height;
#if KM_CAST_MODE != KM_CAST_POINTS
  float* __restrict__ out = depth + (size_t)env * npix;
#endif
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
  // Round 5: when the workgroup's stride is a whole number of image rows (64-wide images: 128 lanes = two rows) a lane keeps its
  // COLUMN for the whole loop, so everything that is linear in the pixel coordinates has a per-lane constant part.
  // The loop is bound by the NUMBER of float64 instructions a pixel issues (a wave is one image row): what a ray rarely needs is
  // computed where it is needed -- the direction in the cube frame and the slab reciprocals behind the bounding-sphere test (itself
  // in the world frame: a rotation changes neither dot product), reciprocals take one Newton step (v_rcp_f64 is good to 2^-23: one
  // step gives 2^-46, the depth bar is 1e-6 m), and the depth image's final clamp is one v_med3_f32 after the conversion (rounding
  // is monotonic).
  // Round 6 (column kept): the ray direction is d = e + Y dy with e fixed per lane, so every dot product with d is ONE FMA in dy
  // against two per-lane constants (|d|^2: two) instead of three; dy itself advances by a constant; the table's rectangle is
  // tested as half-width minus |offset from its centre| (three instructions for the four edges' seven).
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
#if KM_CAST_MODE != KM_CAST_POINTS
  const float znf = (float)znear, zff = (float)zfar;
#endif
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
  const int pstep = blockDim.x;
  int p = threadIdx.x;
  // ---- the lane's output pointers; they advance with p
#if KM_CAST_MODE == KM_CAST_POINTS
  PointXYZ* __restrict__ op = reinterpret_cast<PointXYZ*>(xyz) + (size_t)env * npix + threadIdx.x;
  const bool wd = depth != nullptr;                      // (wave-uniform: the depth store is behind a scalar branch)
  float* __restrict__ dp = (wd ? depth : xyz) + (size_t)env * npix + threadIdx.x;      // (never written unless wd)
  for (int it = 0; it < nit; it++, p += pstep, op += pstep, dp += pstep) {
#else
  float* __restrict__ op = out + threadIdx.x;
  for (int it = 0; it < nit; it++, p += pstep, op += pstep) {
#endif
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
    // cube box: slab test in the cube frame -- only for rays that meet the box's bounding sphere (a wave is one image row or two,
    // so the test is coherent)
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
    // the visible spheres (finger tips): from the gripper camera they fill most of the image, so nearly every wave (one image
    // row) takes the hit path of every sphere -- 1 / |d|^2 once per pixel, a one-step square root
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
        const DepthCap& q = caps[k];
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
    // ---- the store (COLFIXED launches: npix is a multiple of the workgroup, checked by the launcher)
#if KM_CAST_MODE == KM_CAST_POINTS
    // the pixel's point.  D: the clipped depth, float64.  best starts at zfar and only ever takes a smaller value (the table's
    // t < zfar, every other hit t < best), and it is never NaN (only comparisons that held assigned it): the clip is its lower half
    const real D = fmax(best, znear);
    if (COLFIXED || p < npix) {
      PointXYZ P;
      if (world) {
        P.x = (float)__builtin_fma(D, d0, ox); P.y = (float)__builtin_fma(D, d1, oy); P.z = (float)__builtin_fma(D, d2, oz);
      } else {
        P.x = (float)(D * dx); P.y = (float)(D * dy); P.z = (float)(-D);
      }
      *op = P;
      if (wd) *dp = (float)D;
    }
#else
    if (COLFIXED || p < npix) *op = __builtin_amdgcn_fmed3f((float)best, znf, zff);
#endif
  }
}
