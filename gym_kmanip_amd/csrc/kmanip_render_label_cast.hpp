// kmanip_render_label_cast.hpp -- the RGB / label ray cast of the segmentation kernels, written once for the
// two kernels that run it: k_render_labels (kmanip_render_labels.hip, section 13) and k_render_links (kmanip_render_links.hip,
// section 14), which is k_render_labels plus a per-handle list of link capsules (kmanip_set_render_links).  Only those two
// translation units include this header.  k_render_rgb (kmanip_render.hip) and rgb_pixel keep their own code: bench.py times that
// kernel and its device code is pinned (section 33 says why it stays apart), so a change to a hit test there belongs here too.
#pragma once
#include "kmanip_render_scene.hpp"

// float32 view of the capsules for the pixel loop, built by lanes 128 .. 128 + n - 1 from the float64 RenderScene.  Everything is
// relative to the camera origin o; A, B the world end points of the axis, u = (B - A) / |B - A|.
struct LinkScene {
  float oa[KM_MAX_LINK_CAPSULES][3], ob[KM_MAX_LINK_CAPSULES][3];   // o - A, o - B
  float u[KM_MAX_LINK_CAPSULES][3];
  float op[KM_MAX_LINK_CAPSULES][3];                                // oa - (oa.u) u: the part of oa across the axis
  float ou[KM_MAX_LINK_CAPSULES], len[KM_MAX_LINK_CAPSULES];        // oa.u, |B - A|
  float c[KM_MAX_LINK_CAPSULES];                                    // |op|^2 - r^2 = oa.oa - ou^2 - r^2
  float ca[KM_MAX_LINK_CAPSULES], cb[KM_MAX_LINK_CAPSULES];         // the end spheres: |oa|^2 - r^2, |ob|^2 - r^2 (+INFINITY: not tested)
  float ir[KM_MAX_LINK_CAPSULES];                                   // 1 / r
  int box[KM_MAX_LINK_CAPSULES][4];                                 // screen rectangle r0, r1, c0, c1 (inclusive); r0 > r1: never tested
  uint32_t lab[KM_MAX_LINK_CAPSULES];                               // KM_SEG_ROBOT_R / KM_SEG_ROBOT_L
};
#define KM_LINK_LANE0 128              // the third wave is idle during the set-up: one capsule per lane
#define KM_LINK_BIT0 (1 + KM_RGB_MAXSPH)   // object mask: bit 0 the cube, bits 1-4 the spheres, bits 5-28 the capsules
static_assert(KM_LINK_BIT0 + KM_MAX_LINK_CAPSULES <= 32, "the object mask is one uint32_t");
static_assert(KM_LINK_LANE0 + KM_MAX_LINK_CAPSULES <= 192, "one capsule per lane of the third wave");

// Capsule k of the list: ray constants and screen rectangle (float64 throughout, rounded once).  The rectangle is the union of the
// two end spheres' rectangles, each as rgb_scene computes a sphere's (the bounding box of a convex hull is that of its
// generators); either end not safely in front of the camera: the whole image; the camera not in cam_mask: empty.
// An end sphere that IS a visible finger sphere (same centre, same radius: the default list's finger capsules end in one) is not
// tested again: the sphere is tested first and keeps the tie, and in float32 the second evaluation would differ from the first
// by an ulp and win it at random.  Its |oe|^2 - r^2 is stored as +INFINITY: the discriminant is then negative for every ray.
__device__ __forceinline__ void link_setup(const KDeviceModel* dm, const RenderScene& sc, const KLinkCapsule& cp, int k, int cam, int height, int width,
                                           LinkScene* ls) {
  const int l = cp.link;
  const real rad = cp.radius;
  real v[3], A[3], B[3], sv[3];
  mat_vec3(v, sc.xmat[l], cp.p0);
  mat_vec3(sv, sc.xmat[l], cp.seg);
  for (int c = 0; c < 3; c++) { A[c] = sc.xpos[l][c] + v[c]; B[c] = A[c] + sv[c]; }
  const real L = sqrt(dot3(sv, sv));
  real u[3] = {0, 0, 1};
  if (L > 0) { for (int c = 0; c < 3; c++) u[c] = sv[c] / L; }
  real oa[3], ob[3], op[3];
  for (int c = 0; c < 3; c++) { oa[c] = sc.cam_o[c] - A[c]; ob[c] = sc.cam_o[c] - B[c]; }
  const real ou = dot3(oa, u);
  for (int c = 0; c < 3; c++) op[c] = oa[c] - ou * u[c];
  for (int c = 0; c < 3; c++) { ls->oa[k][c] = (float)oa[c]; ls->ob[k][c] = (float)ob[c]; ls->u[k][c] = (float)u[c]; ls->op[k][c] = (float)op[c]; }
  ls->ou[k] = (float)ou; ls->len[k] = (float)L;
  ls->c[k] = (float)(dot3(op, op) - rad * rad);
  bool dup[2] = {false, false};
  for (int i = 0; i < dm->x.nvis; i++) {
    const int s = dm->x.vis_sphere[i];
    if (dm->d.sphere_radius[s] != rad) continue;
    const real da[3] = {A[0] - sc.sph[s][0], A[1] - sc.sph[s][1], A[2] - sc.sph[s][2]};
    const real db[3] = {B[0] - sc.sph[s][0], B[1] - sc.sph[s][1], B[2] - sc.sph[s][2]};
    dup[0] = dup[0] || dot3(da, da) < 1e-18;             // (1 nm: the two centres come from the same inputs by the same operations)
    dup[1] = dup[1] || dot3(db, db) < 1e-18;
  }
  ls->ca[k] = dup[0] ? INFINITY : (float)(dot3(oa, oa) - rad * rad);
  ls->cb[k] = dup[1] ? INFINITY : (float)(dot3(ob, ob) - rad * rad);
  ls->ir[k] = (float)(1.0 / rad);
  ls->lab[k] = (uint32_t)cp.label;
  int* box = ls->box[k];
  if (!(cp.cam_mask >> cam & 1u)) { box[0] = 1; box[1] = 0; box[2] = 1; box[3] = 0; return; }
  real r0 = 1e30, r1 = -1e30, c0 = 1e30, c1 = -1e30;
  bool ok = true;
  for (int e = 0; e < 2; e++) {
    const real* E = e ? B : A;
    const real* oe = e ? ob : oa;
    real row = 0, col = 0;
    const real zc = dot3(oe, sc.cam_z);                                    // depth of the centre along the optical axis
    const bool oke = rgb_project(sc, E, height, width, row, col) && zc - rad > 1e-3;
    const real pr = oke ? 1.5 * sc.focal * rad / (zc - rad) + 1.0 : 0.0;   // (rgb_scene's generous radius)
    ok = ok && oke;
    r0 = fmin(r0, row - pr); r1 = fmax(r1, row + pr); c0 = fmin(c0, col - pr); c1 = fmax(c1, col + pr);
  }
  if (!ok) { box[0] = 0; box[1] = height - 1; box[2] = 0; box[3] = width - 1; return; }
  box[0] = (int)fmin(fmax(floor(r0) - 1, -1.0), (real)height); box[1] = (int)fmax(fmin(ceil(r1) + 1, (real)height), -1.0);
  box[2] = (int)fmin(fmax(floor(c0) - 1, -1.0), (real)width); box[3] = (int)fmax(fmin(ceil(c1) + 1, (real)width), -1.0);
}

// rgb_pixel (kmanip_render_scene.hpp) for the label kernels: the same ray cast, line for line, which also hands out the pixel's
// KM_SEG_* value -- `mat` with a robot pixel replaced by byte s of `slab` (KM_SEG_ROBOT_R + arm of visible sphere s) or by the
// capsule's label.  SHADE = false (no RGB output): classification only -- no normals, no rsq, no light terms; returns 0.  A copy,
// not a parameter of rgb_pixel: with the parameter the RGB kernels' code moved by two instructions, and their
// code does not change.  LINKS: the capsules of `lc` are tested after the spheres (bit KM_LINK_BIT0 + k of `objs`: capsule k of the
// list; LINKS = false never reads lc).  The capsule arithmetic is written with explicit fused multiply-adds, so that every
// instantiation (shading or not, VIS or not) rounds a ray's hit distance identically: the labels-only kernel and the RGB kernel
// classify alike.
template <bool VIS, bool SHADE, bool LINKS>
__device__ __forceinline__ uint32_t label_pixel(const RgbScene& g, const RgbVis* gv, const LinkScene* lcp, int ncap, float dx, float dy, uint32_t objs,
                                                bool tab, uint32_t slab, uint32_t& lab) {
  const float dz = g.X[2] * dx + g.Y[2] * dy - g.Z[2];
  const float dd = dx * dx + dy * dy + 1.0f;                   // |d|^2: the camera axes are orthonormal
  float best = g.zfar;
  int mat = 0;
  uint32_t rob = 0;
  float n0 = 0, n1 = 0, n2 = 1;
  if (tab && dz != 0.0f) { const float t = (g.tz - g.o[2]) * __builtin_amdgcn_rcpf(dz); if (t > 0 && t < best) { best = t; mat = 1; } }
  const float d0 = g.X[0] * dx + g.Y[0] * dy - g.Z[0], d1 = g.X[1] * dx + g.Y[1] * dy - g.Z[1];
  if (objs & 1u) {
    // cube box: slab test in the cube frame; the ray direction there is linear in (dx, dy)
    float t0 = -INFINITY, t1 = INFINITY, s0 = 0, s1 = 0;
    int a0 = 0, a1 = 0;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float dl = g.DX[a] * dx + g.DY[a] * dy - g.DZ[a], h = g.half[a], o = g.ol[a];
      if (dl != 0.0f) {
        const float inv = __builtin_amdgcn_rcpf(dl);
        float ta = (-h - o) * inv, tb = (h - o) * inv, sa = -1, sb = 1;
        if (ta > tb) { const float s = ta; ta = tb; tb = s; sa = 1; sb = -1; }
        if (ta > t0) { t0 = ta; a0 = a; s0 = sa; }
        if (tb < t1) { t1 = tb; a1 = a; s1 = sb; }
      } else if (o < -h || o > h) ok = false;
    }
    if (ok && t0 <= t1 && t1 > 0) {
      const bool front = t0 > 0;
      const float t = front ? t0 : t1;
      if (t < best) {
        best = t; mat = 2;
        if constexpr (SHADE) {
          const int ax = front ? a0 : a1;
          const float sg = front ? s0 : s1;
          n0 = sg * g.R[ax]; n1 = sg * g.R[3 + ax]; n2 = sg * g.R[6 + ax];
        }
      }
    }
  }
  for (int s = 0; s < g.nsph; s++) {
    if (objs >> (1 + s) & 1u) {
      const float b = d0 * g.oc[s][0] + d1 * g.oc[s][1] + dz * g.oc[s][2], disc = b * b - dd * g.cc[s];
      if (disc >= 0) {
        const float t = (-b - __builtin_sqrtf(disc)) * __builtin_amdgcn_rcpf(dd);
        if (t > 0 && t < best) {
          best = t; mat = 3;
          rob = (slab >> (8 * s)) & 0xFFu;
          if constexpr (SHADE) { n0 = (g.oc[s][0] + t * d0) * g.ir[s]; n1 = (g.oc[s][1] + t * d1) * g.ir[s]; n2 = (g.oc[s][2] + t * dz) * g.ir[s]; }
        }
      }
    }
  }
  if constexpr (LINKS) {
    const LinkScene& lc = *lcp;
    if (objs >> KM_LINK_BIT0) {
      const float idd = __builtin_amdgcn_rcpf(dd);
      for (int k = 0; k < ncap; k++) {
        if (!(objs >> (KM_LINK_BIT0 + k) & 1u)) continue;
        const float u0 = lc.u[k][0], u1 = lc.u[k][1], u2 = lc.u[k][2], ou = lc.ou[k];
        const float du = __builtin_fmaf(d0, u0, __builtin_fmaf(d1, u1, dz * u2));
        // body: the ray against the infinite cylinder, in the plane across the axis (dp = d - (d.u) u: no cancellation in a)
        const float p0 = __builtin_fmaf(-du, u0, d0), p1 = __builtin_fmaf(-du, u1, d1), p2 = __builtin_fmaf(-du, u2, dz);
        const float a = __builtin_fmaf(p0, p0, __builtin_fmaf(p1, p1, p2 * p2));
        const float b = __builtin_fmaf(d0, lc.op[k][0], __builtin_fmaf(d1, lc.op[k][1], dz * lc.op[k][2]));
        const float h = __builtin_fmaf(b, b, -(a * lc.c[k]));
        float t = INFINITY;
        bool body = false;
        if (h >= 0) {
          const float tb = (-b - __builtin_sqrtf(h)) * __builtin_amdgcn_rcpf(a);
          const float sb = __builtin_fmaf(tb, du, ou);
          body = sb > 0 && sb < lc.len[k];                     // (a = 0, the ray along the axis: tb is not finite, the test fails)
          if (body) t = tb;
        }
        if (!body) {
          // the end spheres' entry roots, as for the finger spheres
          const float ba = __builtin_fmaf(d0, lc.oa[k][0], __builtin_fmaf(d1, lc.oa[k][1], dz * lc.oa[k][2]));
          const float bb = __builtin_fmaf(d0, lc.ob[k][0], __builtin_fmaf(d1, lc.ob[k][1], dz * lc.ob[k][2]));
          const float da = __builtin_fmaf(ba, ba, -(dd * lc.ca[k])), db = __builtin_fmaf(bb, bb, -(dd * lc.cb[k]));
          const float ta = da >= 0 ? (-ba - __builtin_sqrtf(da)) * idd : INFINITY;
          const float tb = db >= 0 ? (-bb - __builtin_sqrtf(db)) * idd : INFINITY;
          t = tb < ta ? tb : ta;
        }
        if (t > 0 && t < best) {
          best = t; mat = 3;
          rob = lc.lab[k];
          if constexpr (SHADE) {
            // (P - (A + clamp(s, 0, L) u)) / r with s = (P - A).u and P - A = oa + t d
            const float s = __builtin_amdgcn_fmed3f(__builtin_fmaf(t, du, ou), 0.0f, lc.len[k]), ir = lc.ir[k];
            n0 = (__builtin_fmaf(t, d0, lc.oa[k][0]) - s * u0) * ir;
            n1 = (__builtin_fmaf(t, d1, lc.oa[k][1]) - s * u1) * ir;
            n2 = (__builtin_fmaf(t, dz, lc.oa[k][2]) - s * u2) * ir;
          }
        }
      }
    }
  }
  lab = mat == 3 ? rob : (uint32_t)mat;
  if constexpr (!SHADE) return 0u;
  if constexpr (VIS) {
    if (mat == 0) return gv->bg;
  } else {
    if (mat == 0) return 0u;
  }
  const float rs = __builtin_amdgcn_rsqf(dd);
  float I;
  if constexpr (VIS) {
    // the env's light terms (at their defaults these are the default kernel's operations on the same values)
    if (mat == 1) I = gv->amb + gv->hl * fmaxf(0.0f, -dz * rs) + g.tab_L;
    else {
      const float r3 = 0.57735026919f, r2 = 0.70710678119f;
      I = gv->amb + gv->hl * fmaxf(0.0f, -(n0 * d0 + n1 * d1 + n2 * dz) * rs)
          + gv->ds * (fmaxf(0.0f, (-n0 - n1 + n2) * r3) + fmaxf(0.0f, (n0 - n1 + n2) * r3) + fmaxf(0.0f, (n1 + n2) * r2));
    }
    I = fminf(I, 1.0f) * 255.0f;
    const float* col = gv->col[mat - 1];
    return (uint32_t)(col[0] * I + 0.5f) | ((uint32_t)(col[1] * I + 0.5f) << 8) | ((uint32_t)(col[2] * I + 0.5f) << 16);
  }
  if (mat == 1) I = 0.4f + 0.4f * fmaxf(0.0f, -dz * rs) + g.tab_L;
  else {
    const float r3 = 0.57735026919f, r2 = 0.70710678119f;
    I = 0.4f + 0.4f * fmaxf(0.0f, -(n0 * d0 + n1 * d1 + n2 * dz) * rs)
        + 0.3f * (fmaxf(0.0f, (-n0 - n1 + n2) * r3) + fmaxf(0.0f, (n0 - n1 + n2) * r3) + fmaxf(0.0f, (n1 + n2) * r2));
  }
  I = fminf(I, 1.0f) * 255.0f;
  if (mat == 1) { const uint32_t v = (uint32_t)(0.2f * I + 0.5f); return v | (v << 8) | (v << 16); }
  if (mat == 2) return (uint32_t)(I + 0.5f);                                         // cube: rgba 1 0 0
  const uint32_t v = (uint32_t)(0.647059f * I + 0.5f);
  return v | (v << 8) | (v << 16);
}

// ---- segmentation labels, with link capsules (section 14) ---------------------------------------
// The ray cast of k_render_rgb with one more output: uint8 [num_envs, h, w] KM_SEG_* labels per job, next to (RGB) or instead of
// (RGB = false) the RGB bytes.  Same set-up, same 64 x 4 tiles, same per-pixel device code; a quad's four labels are one dword.
// A job's rgb / seg pointer may be NULL in the RGB = true kernel (a launch of mixed jobs): that output is then not written.
// RGB = false never shades: the classification alone decides a label.
// LINKS: the handle's capsule list `la` is drawn: the same set-up plus one capsule per lane of the third wave, the same table-only
// and background paths outside the union rectangle, which then also holds the capsules' rectangles.  LINKS = false reads nothing of
// `la` and has no LinkScene in LDS.
template <bool VIS, bool RGB, bool LINKS>
__device__ __forceinline__ void label_cast(const KDeviceModel* __restrict__ dm, const KDeviceState& st, const KLabelJobs& jobs, const KLinkArgs& la,
                                           const KVisArgs& va) {
  __shared__ RenderScene sc;
  __shared__ alignas(8) RgbScene g;
  __shared__ RgbTmp tmp;
  __shared__ RgbVis gv_;
  __shared__ double vsv_[KM_VP_N];
  __shared__ LinkScene lc_;                  // (LINKS only: the kernels without a list never reference it)
  __shared__ uint32_t slab_;                 // byte s: KM_SEG_ROBOT_R + arm of visible sphere s
  RgbVis* gv = nullptr;
  double* vsv = nullptr;
  LinkScene* lcp = nullptr;
  if constexpr (VIS) { gv = &gv_; vsv = vsv_; }
  if constexpr (LINKS) lcp = &lc_;
  const int env = blockIdx.x, job = blockIdx.y;
  const int cam = jobs.cam[job], height = jobs.height[job], width = jobs.width[job];
  uint8_t* __restrict__ rgb = RGB ? jobs.rgb[job] : nullptr;
  uint8_t* __restrict__ seg = jobs.seg[job];
  const int ncap = LINKS ? la.n : 0;
  // the capsule of this lane, read with the kinematics' inputs (used after the FK's barriers)
  const int ck = (int)threadIdx.x - KM_LINK_LANE0;
  const bool cap_lane = LINKS && ck >= 0 && ck < ncap;
  KLinkCapsule cp{};
  if constexpr (LINKS) cp = la.caps[cap_lane ? ck : 0];
  RenderPre pre;
  render_fk<VIS>(dm, st, env, cam, &sc, pre, va, vsv);
  render_camera<VIS>(dm, st, env, cam, height, &sc, pre, vsv);
  __syncthreads();
  if constexpr (LINKS) {
    if (cap_lane) link_setup(dm, sc, cp, ck, cam, height, width, lcp);     // (written before rgb_scene's barrier, read after it)
  }
  rgb_scene<VIS>(dm, sc, height, width, &g, &tmp, threadIdx.x, gv, vsv);
  if constexpr (LINKS) {
    if (threadIdx.x == 0) {
      // the capsules' rectangles into the union (lane 0 has just written it); an empty rectangle takes no part
      for (int k = 0; k < ncap; k++) {
        const int* b = lcp->box[k];
        if (b[0] > b[1] || b[2] > b[3]) continue;
        g.ubox[0] = min(g.ubox[0], b[0]); g.ubox[1] = max(g.ubox[1], b[1]);
        g.ubox[2] = min(g.ubox[2], b[2]); g.ubox[3] = max(g.ubox[3], b[3]);
      }
    }
  }
  if (threadIdx.x == 64) {
    uint32_t v = 0;
    for (int k = 0; k < dm->x.nvis; k++) v |= (uint32_t)(KM_SEG_ROBOT_R + dm->sphere_arm[dm->x.vis_sphere[k]]) << (8 * k);
    slab_ = v;
  }
  __syncthreads();
  const uint32_t slab = __builtin_amdgcn_readfirstlane(slab_);
  const int npix = height * width;
  const float hw = 0.5f * width, hh = 0.5f * height, inv_f = g.inv_f;
  uint8_t* out = rgb ? rgb + (size_t)env * npix * 3 : nullptr;
  uint8_t* lout = seg ? seg + (size_t)env * npix : nullptr;
  if ((width & 3) == 0) {
    const int wq = width >> 2, tcols = (wq + 15) >> 4, ntile = tcols * ((height + 15) >> 4);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    uint32_t* lab32 = reinterpret_cast<uint32_t*>(lout);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int tr = 0, tc = 0;
    const float k0 = g.tz - g.o[2], sg = k0 < 0.0f ? -1.0f : 1.0f, thr = k0 != 0.0f ? fabsf(k0) / g.zfar : INFINITY;
    const float Xzs = sg * g.X[2], Yzs = sg * g.Y[2], Zzs = sg * g.Z[2];
    float lam = 0, c1 = 0;
    if constexpr (RGB) { lam = VIS ? -gv->hl * sg : -0.4f * sg; c1 = VIS ? gv->amb + g.tab_L : 0.4f + g.tab_L; }
    const int nobj = g.nsph;
    float kr = 0, kg = 0, kb = 0;
    uint32_t bg0 = 0, bg1 = 0, bg2 = 0;
    if constexpr (VIS && RGB) {
      kr = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gv->k255[0])));
      kg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gv->k255[1])));
      kb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gv->k255[2])));
      bg0 = __builtin_amdgcn_readfirstlane(gv->bgw[0]); bg1 = __builtin_amdgcn_readfirstlane(gv->bgw[1]);
      bg2 = __builtin_amdgcn_readfirstlane(gv->bgw[2]);
    }
    float lo = 0, hi = 0, dy = 0, rz = 0, rd = 0;
    bool row_ok = false;
    for (int tile = 0; tile < ntile; tile++) {
      const int r = (tr << 4) + ty, qc = (tc << 4) + tx, c = qc << 2, q = r * wq + qc;
      if (tc == 0) {
        dy = -(r + 0.5f - hh) * inv_f;
        rgb_table_span(g, dy, lo, hi);
        rz = Yzs * dy - Zzs; rd = dy * dy + 1.0f;
        const float xa = fmaxf(lo, (0.5f - hw) * inv_f) - inv_f, xb = fminf(hi, (width - 0.5f - hw) * inv_f) + inv_f;
        row_ok = (Xzs * xa + rz > thr) && (Xzs * xb + rz > thr);
      }
      if (++tc == tcols) { tc = 0; tr++; }
      if (r >= height || qc >= wq) continue;
      const float dx0 = (c + 0.5f - hw) * inv_f;
      uint32_t w0 = 0, w1 = 0, w2 = 0, lw;
      if (r >= g.ubox[0] && r <= g.ubox[1] && c + 3 >= g.ubox[2] && c <= g.ubox[3]) {
        uint32_t objs = 0;
        for (int o = 0; o <= nobj; o++)
          objs |= (uint32_t)(r >= g.box[o][0] && r <= g.box[o][1] && c + 3 >= g.box[o][2] && c <= g.box[o][3]) << o;
        if constexpr (LINKS) {
          for (int k = 0; k < ncap; k++)
            objs |= (uint32_t)(r >= lcp->box[k][0] && r <= lcp->box[k][1] && c + 3 >= lcp->box[k][2] && c <= lcp->box[k][3]) << (KM_LINK_BIT0 + k);
        }
        uint32_t px[4], lb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float dx = (c + i + 0.5f - hw) * inv_f;
          px[i] = label_pixel<VIS, RGB, LINKS>(g, gv, lcp, ncap, dx, dy, objs, dx > lo && dx < hi, slab, lb[i]);
        }
        if constexpr (RGB) { w0 = px[0] | (px[1] << 24); w1 = (px[1] >> 8) | (px[2] << 16); w2 = (px[2] >> 16) | (px[3] << 8); }
        lw = lb[0] | (lb[1] << 8) | (lb[2] << 16) | (lb[3] << 24);
      } else if (!(dx0 + 3.0f * inv_f > lo && dx0 < hi)) {
        if constexpr (VIS && RGB) { w0 = bg0; w1 = bg1; w2 = bg2; }
        lw = 0u;                                                                        // beside the table: background
      } else {
        // outside every rectangle: table or background, by the tests the RGB table path makes anyway
        const bool whole = row_ok && dx0 > lo && dx0 + 3.0f * inv_f < hi;
        lw = 0x01010101u * KM_SEG_TABLE;
        if constexpr (!RGB) {
          if (!whole) {
            lw = 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const float dx = (c + i + 0.5f - hw) * inv_f;
              const float sdz = Xzs * dx + rz;
              lw |= (uint32_t)(sdz > thr && dx > lo && dx < hi) << (8 * i);
            }
          }
        } else if constexpr (VIS) {
          uint32_t px[4];
          auto shade = [&](float dx, float& sdz) {
            sdz = Xzs * dx + rz;
            const float dd = dx * dx + rd;
            const float a = __builtin_amdgcn_fmed3f(sdz * __builtin_amdgcn_rsqf(dd) * lam, 0.0f, 1.0f);
            const float I = __builtin_amdgcn_fmed3f(a + c1, 0.0f, 1.0f);
            return (uint32_t)(I * kr + 0.5f) | ((uint32_t)(I * kg + 0.5f) << 8) | ((uint32_t)(I * kb + 0.5f) << 16);
          };
          if (whole) {
#pragma unroll
            for (int i = 0; i < 4; i++) { float sdz; px[i] = shade(dx0 + (float)i * inv_f, sdz); }
          } else {
            const uint32_t bgp = bg0 & 0xFFFFFFu;
            lw = 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const float dx = (c + i + 0.5f - hw) * inv_f;
              float sdz;
              const uint32_t v = shade(dx, sdz);
              const bool on = sdz > thr && dx > lo && dx < hi;
              px[i] = on ? v : bgp;
              lw |= (uint32_t)on << (8 * i);
            }
          }
          w0 = __builtin_amdgcn_perm(px[1], px[0], 0x04020100u);
          w1 = __builtin_amdgcn_perm(px[2], px[1], 0x05040201u);
          w2 = __builtin_amdgcn_perm(px[3], px[2], 0x06050402u);
        } else {
          uint32_t v[4];
          if (whole) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const float dx = dx0 + (float)i * inv_f;
              const float sdz = Xzs * dx + rz, dd = dx * dx + rd;
              const float a = __builtin_amdgcn_fmed3f(sdz * __builtin_amdgcn_rsqf(dd) * lam, 0.0f, 1.0f);
              v[i] = (uint32_t)(__builtin_amdgcn_fmed3f(a + c1, 0.0f, 1.0f) * 51.0f + 0.5f);
            }
          } else {
            lw = 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const float dx = (c + i + 0.5f - hw) * inv_f;
              const float sdz = Xzs * dx + rz, dd = dx * dx + rd;
              const float a = __builtin_amdgcn_fmed3f(sdz * __builtin_amdgcn_rsqf(dd) * lam, 0.0f, 1.0f);
              const float I = __builtin_amdgcn_fmed3f(a + c1, 0.0f, 1.0f);
              const bool on = sdz > thr && dx > lo && dx < hi;
              v[i] = on ? (uint32_t)(51.0f * I + 0.5f) : 0u;
              lw |= (uint32_t)on << (8 * i);
            }
          }
          w0 = __builtin_amdgcn_perm(v[1], v[0], 0x04000000u);
          w1 = __builtin_amdgcn_perm(v[2], v[1], 0x04040000u);
          w2 = __builtin_amdgcn_perm(v[3], v[2], 0x04040400u);
        }
      }
      if constexpr (RGB) {
        if (out32) { out32[3 * q] = w0; out32[3 * q + 1] = w1; out32[3 * q + 2] = w2; }
        if (lab32) lab32[q] = lw;
      } else lab32[q] = lw;                                                             // (one global_store_dword: 64 contiguous bytes a tile row)
    }
  } else {
    for (int p = threadIdx.x; p < npix; p += blockDim.x) {
      const int r = p / width, c = p - r * width;
      uint32_t objs = 0;
      for (int o = 0; o <= g.nsph; o++)
        objs |= (uint32_t)(r >= g.box[o][0] && r <= g.box[o][1] && c >= g.box[o][2] && c <= g.box[o][3]) << o;
      if constexpr (LINKS) {
        for (int k = 0; k < ncap; k++)
          objs |= (uint32_t)(r >= lcp->box[k][0] && r <= lcp->box[k][1] && c >= lcp->box[k][2] && c <= lcp->box[k][3]) << (KM_LINK_BIT0 + k);
      }
      const float dx = (c + 0.5f - hw) * inv_f, dy = -(r + 0.5f - hh) * inv_f;
      uint32_t lb;
      const uint32_t v = label_pixel<VIS, RGB, LINKS>(g, gv, lcp, ncap, dx, dy, objs, rgb_over_table(g, dx, dy), slab, lb);
      if constexpr (RGB) {
        if (out) { out[3 * (size_t)p] = (uint8_t)v; out[3 * (size_t)p + 1] = (uint8_t)(v >> 8); out[3 * (size_t)p + 2] = (uint8_t)(v >> 16); }
        if (lout) lout[p] = (uint8_t)lb;
      } else lout[p] = (uint8_t)lb;
    }
  }
}
