// kmanip_render_labels.hip -- per-pixel segmentation labels of the RGB ray cast: k_render_labels writes
// uint8 [num_envs, h, w] KM_SEG_* labels next to, or instead of, the bytes k_render_rgb writes, from one ray cast.  A translation
// unit of its own: compiled into kmanip_render.hip, the new kernels changed the code the compiler emits for k_render_rgb's shared
// set-up, and that kernel's code does not change.
#include "kmanip_render_scene.hpp"

// rgb_pixel for the label kernel: the same ray cast, line for line, which also hands out the pixel's KM_SEG_* value -- `mat` with a
// robot pixel replaced by byte s of `slab` (KM_SEG_ROBOT_R + arm of visible sphere s).  SHADE = false (no RGB output):
// classification only -- no normals, no rsq, no light terms; returns 0.  A copy, not a parameter of rgb_pixel: with the parameter
// the RGB kernels' code moved by two instructions, and their code does not change.
template <bool VIS, bool SHADE>
__device__ __forceinline__ uint32_t seg_pixel(const RgbScene& g, const RgbVis* gv, float dx, float dy, uint32_t objs, bool tab,
                                              uint32_t slab, uint32_t& lab) {
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

// ---- segmentation labels ----------------------------------------------------------------------
// The ray cast of k_render_rgb with one more output: uint8 [num_envs, h, w] KM_SEG_* labels per job, next to (RGB) or instead of
// (RGB = false) the RGB bytes.  Same set-up, same 64 x 4 tiles, same per-pixel device code; a quad's four labels are one dword.
// A job's rgb / seg pointer may be NULL in the RGB = true kernel (a launch of mixed jobs): that output is then not written.
// RGB = false never shades: the classification alone decides a label.
template <bool VIS, bool RGB, class... VA>
__global__ __launch_bounds__(256) void k_render_labels(const KDeviceModel* __restrict__ dm, KDeviceState st, KLabelJobs jobs, VA... vargs) {
  static_assert(sizeof...(VA) == (VIS ? 1 : 0), "the VIS kernel takes one KVisArgs, the default kernel none");
  __shared__ RenderScene sc;
  __shared__ alignas(8) RgbScene g;
  __shared__ RgbTmp tmp;
  __shared__ RgbVis gv_;
  __shared__ double vsv_[KM_VP_N];
  __shared__ uint32_t slab_;                 // byte s: KM_SEG_ROBOT_R + arm of visible sphere s
  KVisArgs va{};
  RgbVis* gv = nullptr;
  double* vsv = nullptr;
  if constexpr (VIS) { ((va = vargs), ...); gv = &gv_; vsv = vsv_; }
  const int env = blockIdx.x, job = blockIdx.y;
  const int cam = jobs.cam[job], height = jobs.height[job], width = jobs.width[job];
  uint8_t* __restrict__ rgb = RGB ? jobs.rgb[job] : nullptr;
  uint8_t* __restrict__ seg = jobs.seg[job];
  RenderPre pre;
  render_fk<VIS>(dm, st, env, cam, &sc, pre, va, vsv);
  render_camera<VIS>(dm, st, env, cam, height, &sc, pre, vsv);
  __syncthreads();
  rgb_scene<VIS>(dm, sc, height, width, &g, &tmp, threadIdx.x, gv, vsv);
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
        uint32_t px[4], lb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float dx = (c + i + 0.5f - hw) * inv_f;
          px[i] = seg_pixel<VIS, RGB>(g, gv, dx, dy, objs, dx > lo && dx < hi, slab, lb[i]);
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
      const float dx = (c + 0.5f - hw) * inv_f, dy = -(r + 0.5f - hh) * inv_f;
      uint32_t lb;
      const uint32_t v = seg_pixel<VIS, RGB>(g, gv, dx, dy, objs, rgb_over_table(g, dx, dy), slab, lb);
      if constexpr (RGB) {
        if (out) { out[3 * (size_t)p] = (uint8_t)v; out[3 * (size_t)p + 1] = (uint8_t)(v >> 8); out[3 * (size_t)p + 2] = (uint8_t)(v >> 16); }
        if (lout) lout[p] = (uint8_t)lb;
      } else lout[p] = (uint8_t)lb;
    }
  }
}

void kmanip_launch_render_labels(const KDeviceModel* dm, const KDeviceState& st, const KLabelJobs& jobs, bool rgb, const KVisArgs& vis, hipStream_t stream) {
  const dim3 grid(st.num_envs, jobs.n), block(256);
  if (km_vis_on(vis)) {
    if (rgb) k_render_labels<true, true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, jobs, vis);
    else k_render_labels<true, false, KVisArgs><<<grid, block, 0, stream>>>(dm, st, jobs, vis);
  } else {
    if (rgb) k_render_labels<false, true><<<grid, block, 0, stream>>>(dm, st, jobs);
    else k_render_labels<false, false><<<grid, block, 0, stream>>>(dm, st, jobs);
  }
}
