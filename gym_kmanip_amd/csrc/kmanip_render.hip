// kmanip_render.hip -- camera renders of every env's current state: float32 depth (BASELINE.json config 5) and uint8 RGB
// (the camera observations of the *Vision env ids and KManipEnv.render()).
//
// Replaces the camera branch of KManipTask.get_observation / KManipEnvSim.k_render (reference
// gym_kmanip/env_sim.py:140-145,187-188 -> dm_control physics.render(height, width, camera_id)).  Cameras are the
// reference's four, all mode="targetbody": grip_r / grip_l on the hand links tracking the EE site body (fovy 20:
// arm_r_body.xml:68, arm_l_body.xml:68, torso_body.xml:104,173) and the world-fixed top / head tracking the table
// (fovy 78: _env_solo_arm.xml:14-15 and siblings).  The rendered scene is the build's surrogate geometry = its collision
// primitives (cube box, table plane, finger spheres): the reference's robot meshes are absent from the checkout
// (DESIGN.md section 5), so pixel parity with MuJoCo's OpenGL renderer is not defined; parity is against the oracle's
// restatement of the same ray caster.
//   depth : metres along the optical axis, clipped to [znear, zfar], no hit = zfar
//   rgb   : Lambert shading of the reference's material colours (cube rgba 1 0 0, table rgba .2 .2 .2: scene.xml:15,20)
//           under the reference's lights (scene.xml:8-13: headlight ambient 0.4 + MuJoCo's default headlight diffuse 0.4,
//           three directional lights of diffuse 0.3), no specular / shadows / fog; background black
//
// One workgroup (256 lanes) per env.  Forward kinematics run one link per lane with ceil(log2(depth)) rounds of pointer
// jumping through LDS (the same scheme as k_step's fk_parallel), lane 0 builds the camera frame, then the lanes ray-cast.
//   depth (k_render_depth): 128 lanes per env, pixels p = lane, lane + 128, ...; float64 ray maths -- the depth parity bar
//     against the float64 oracle is 1e-6 m, which float32 intersection arithmetic (cancellation ~1e-5 m) would not meet.  The
//     kernel's text is kmanip_render_depth_cast.inc, included below.
//   rgb (k_render_rgb, round 3): the *Vision observations are 480 x 640 x 3 + 40 x 60 x 3 bytes per env-step (__init__.py:
//     158-161), 929 KB -- the one genuinely HBM-sized output of the path.  Round 2 cast every pixel in float64 (~150 FP64
//     operations per pixel: 5 x the time the stores need) and wrote three separate bytes per pixel.  Now: (1) float32 ray
//     maths (the parity bar is one grey level); (2) the cube and the visible spheres are projected to screen-space bounding
//     rectangles once per env, and a pixel outside all of them can only see the table plane or the background: ~15
//     operations (most of a head / top image); (3) a lane shades FOUR consecutive pixels of a row and stores their 12 bytes as
//     three dwords (768 contiguous bytes per wave-instruction group); (4) the per-ray divides of the slab and plane tests are
//     v_rcp_f32 on quantities that are linear in the pixel coordinates.
// Visual parameters (kmanip_set_visual_params / _ranges): every kernel has a VIS instantiation with one more
// argument (KVisArgs), launched only while the handle has visual parameters; VIS = false is the default kernel, unchanged.  In the
// VIS build a few lanes of the second wave load the env's KM_VP_N values (or evaluate their Philox draw) into LDS while the FK
// loads are in flight; lane 0 adds the camera offset when it builds the camera frame, and the RGB kernel shades with the env's
// colours and light terms (RgbVis).
#include "kmanip_render_depth_cast.hpp"

// ---- depth (BASELINE config 5) -------------------------------------------------------------------------------------
// k_render_depth is the float64 depth ray cast of kmanip_render_depth_cast.inc, the one text k_render_depth_links and
// k_render_points are built from too; what rounds 4 to 6 did to its pixel loop is told there.
#define KM_CAST_MODE KM_CAST_DEPTH
#include "kmanip_render_depth_cast.inc"

// one pixel, float32: grey level * 255 of the three channels packed r | g << 8 | b << 16
// (kmanip_render_label_cast.hpp keeps a copy, label_pixel, that also returns the material and tests the link capsules, and its quad
// loop repeats k_render_rgb's table path: a change to the hit tests or the shading here belongs there too -- DESIGN.md sections 13
// and 33 say why it is a copy; tests/test_label_render_gpu.py holds the two to each other byte for byte)
template <bool VIS>
__device__ __forceinline__ uint32_t rgb_pixel(const RgbScene& g, const RgbVis* gv, float dx, float dy, uint32_t objs, bool tab) {
  const float dz = g.X[2] * dx + g.Y[2] * dy - g.Z[2];
  const float dd = dx * dx + dy * dy + 1.0f;                   // |d|^2: the camera axes are orthonormal
  float best = g.zfar;
  int mat = 0;
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
        const int ax = front ? a0 : a1;
        const float sg = front ? s0 : s1;
        n0 = sg * g.R[ax]; n1 = sg * g.R[3 + ax]; n2 = sg * g.R[6 + ax];
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
          n0 = (g.oc[s][0] + t * d0) * g.ir[s]; n1 = (g.oc[s][1] + t * d1) * g.ir[s]; n2 = (g.oc[s][2] + t * dz) * g.ir[s];
        }
      }
    }
  }
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

// grid = envs x jobs: blockIdx.y picks the camera / resolution / output buffer (all the cameras of a *Vision observation in one launch)
// VIS = false: the default kernel (no VA); VIS = true: VA = KVisArgs, one more argument, the env's colours / lights / camera offset
template <bool VIS, class... VA>
__global__ __launch_bounds__(256) void k_render_rgb(const KDeviceModel* __restrict__ dm, KDeviceState st, KRenderJobs jobs, VA... vargs) {
  static_assert(sizeof...(VA) == (VIS ? 1 : 0), "the VIS kernel takes one KVisArgs, the default kernel none");
  __shared__ RenderScene sc;
  __shared__ alignas(8) RgbScene g;     // (a kernel template's LDS objects keep their declared alignment: 8 is what the default had)
  __shared__ RgbTmp tmp;
  __shared__ RgbVis gv_;                     // (VIS only: the default kernel never references these two)
  __shared__ double vsv_[KM_VP_N];
  KVisArgs va{};
  RgbVis* gv = nullptr;
  double* vsv = nullptr;
  if constexpr (VIS) { ((va = vargs), ...); gv = &gv_; vsv = vsv_; }
  const int env = blockIdx.x, job = blockIdx.y;
  const int cam = jobs.cam[job], height = jobs.height[job], width = jobs.width[job];
  uint8_t* __restrict__ rgb = jobs.rgb[job];
  RenderPre pre;
  render_fk<VIS>(dm, st, env, cam, &sc, pre, va, vsv);
  render_camera<VIS>(dm, st, env, cam, height, &sc, pre, vsv);
  __syncthreads();
  rgb_scene<VIS>(dm, sc, height, width, &g, &tmp, threadIdx.x, gv, vsv);
  __syncthreads();
  const int npix = height * width;
  const float hw = 0.5f * width, hh = 0.5f * height, inv_f = g.inv_f;
  uint8_t* out = rgb + (size_t)env * npix * 3;
  if ((width & 3) == 0) {
    // four consecutive pixels of a row per lane: 12 bytes = three dwords.  A wave covers a 64 x 4 pixel tile (16 quads x 4 rows:
    // 192 contiguous bytes a row) rather than 256 pixels of one row, so that fewer waves straddle the objects' rectangles and
    // run both the full and the table-only path; the block walks 64 x 16 pixel tiles, tile row and column advancing
    // incrementally (no integer division)
    const int wq = width >> 2, tcols = (wq + 15) >> 4, ntile = tcols * ((height + 15) >> 4);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int tr = 0, tc = 0;
    // Outside every bounding rectangle a ray can only meet the table plane, and the shaded grey needs no hit distance: with
    // s = sign(tz - o_z), the hit test 0 < (tz - o_z) / dz < zfar is  s dz > |tz - o_z| / zfar, and the Lambert term
    // 0.4 max(0, -dz / |d|) is clamp(s dz * rsq(|d|^2) * (-0.4 s)).  ~14 operations a pixel, one of them transcendental
    const float k0 = g.tz - g.o[2], sg = k0 < 0.0f ? -1.0f : 1.0f, thr = k0 != 0.0f ? fabsf(k0) / g.zfar : INFINITY;
    const float Xzs = sg * g.X[2], Yzs = sg * g.Y[2], Zzs = sg * g.Z[2];
    const float lam = VIS ? -gv->hl * sg : -0.4f * sg, c1 = VIS ? gv->amb + g.tab_L : 0.4f + g.tab_L;
    const int nobj = g.nsph;
    // VIS: the table's three channel factors and the background's packed dwords, wave-uniform
    float kr = 0, kg = 0, kb = 0;
    uint32_t bg0 = 0, bg1 = 0, bg2 = 0;
    if constexpr (VIS) {
      kr = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gv->k255[0])));
      kg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gv->k255[1])));
      kb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gv->k255[2])));
      bg0 = __builtin_amdgcn_readfirstlane(gv->bgw[0]); bg1 = __builtin_amdgcn_readfirstlane(gv->bgw[1]);
      bg2 = __builtin_amdgcn_readfirstlane(gv->bgw[2]);
    }
    // Round 5: the loop was bound by instruction issue, not by its stores (~95 instructions a quad: 0.38 of its 0.45 ms).  A lane
    // keeps its image row while the block walks the tile columns, so the row's table span (20 instructions) and its ray constants
    // are computed once per tile ROW; and a quad that lies wholly inside the span and above the horizon -- nearly all of them --
    // shades its four pixels without the three per-pixel tests.
    float lo = 0, hi = 0, dy = 0, rz = 0, rd = 0;
    bool row_ok = false;              // every pixel of this row that is inside the span also passes the horizon test
    for (int tile = 0; tile < ntile; tile++) {
      const int r = (tr << 4) + ty, qc = (tc << 4) + tx, c = qc << 2, q = r * wq + qc;
      if (tc == 0) {
        dy = -(r + 0.5f - hh) * inv_f;
        rgb_table_span(g, dy, lo, hi);
        rz = Yzs * dy - Zzs; rd = dy * dy + 1.0f;
        // s dz is linear in dx: above the threshold on the whole clipped span iff it is at both ends (+- a pixel of slack)
        const float xa = fmaxf(lo, (0.5f - hw) * inv_f) - inv_f, xb = fminf(hi, (width - 0.5f - hw) * inv_f) + inv_f;
        row_ok = (Xzs * xa + rz > thr) && (Xzs * xb + rz > thr);
      }
      if (++tc == tcols) { tc = 0; tr++; }
      if (r >= height || qc >= wq) continue;
      const float dx0 = (c + 0.5f - hw) * inv_f;
      uint32_t w0, w1, w2;
      if (r >= g.ubox[0] && r <= g.ubox[1] && c + 3 >= g.ubox[2] && c <= g.ubox[3]) {
        uint32_t objs = 0;                                  // objects whose bounding rectangle this quad touches
        for (int o = 0; o <= nobj; o++)
          objs |= (uint32_t)(r >= g.box[o][0] && r <= g.box[o][1] && c + 3 >= g.box[o][2] && c <= g.box[o][3]) << o;
        uint32_t px[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { const float dx = (c + i + 0.5f - hw) * inv_f; px[i] = rgb_pixel<VIS>(g, gv, dx, dy, objs, dx > lo && dx < hi); }
        w0 = px[0] | (px[1] << 24); w1 = (px[1] >> 8) | (px[2] << 16); w2 = (px[2] >> 16) | (px[3] << 8);
      } else if (!(dx0 + 3.0f * inv_f > lo && dx0 < hi)) {
        if constexpr (VIS) { w0 = bg0; w1 = bg1; w2 = bg2; }
        else { w0 = 0; w1 = 0; w2 = 0; }                                               // beside the table: background
      } else if constexpr (VIS) {
        // per-env table colour: three channel values a pixel (one FMA and one conversion each, the default's rounding), packed
        // r | g << 8 | b << 16 and the quad's three dwords cut from the four packed pixels with one v_perm each
        // (the same two cases as the default below: the whole quad is table, or each pixel is tested)
        uint32_t px[4];
        auto shade = [&](float dx, float& sdz) {
          sdz = Xzs * dx + rz;
          const float dd = dx * dx + rd;
          const float a = __builtin_amdgcn_fmed3f(sdz * __builtin_amdgcn_rsqf(dd) * lam, 0.0f, 1.0f);
          const float I = __builtin_amdgcn_fmed3f(a + c1, 0.0f, 1.0f);
          return (uint32_t)(I * kr + 0.5f) | ((uint32_t)(I * kg + 0.5f) << 8) | ((uint32_t)(I * kb + 0.5f) << 16);
        };
        if (row_ok && dx0 > lo && dx0 + 3.0f * inv_f < hi) {
#pragma unroll
          for (int i = 0; i < 4; i++) { float sdz; px[i] = shade(dx0 + (float)i * inv_f, sdz); }
        } else {
          const uint32_t bgp = bg0 & 0xFFFFFFu;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const float dx = (c + i + 0.5f - hw) * inv_f;
            float sdz;
            const uint32_t v = shade(dx, sdz);
            px[i] = (sdz > thr && dx > lo && dx < hi) ? v : bgp;
          }
        }
        w0 = __builtin_amdgcn_perm(px[1], px[0], 0x04020100u);                       // r0 g0 b0 r1
        w1 = __builtin_amdgcn_perm(px[2], px[1], 0x05040201u);                       // g1 b1 r2 g2
        w2 = __builtin_amdgcn_perm(px[3], px[2], 0x06050402u);                       // b2 r3 g3 b3
      } else {
        uint32_t v[4];
        if (row_ok && dx0 > lo && dx0 + 3.0f * inv_f < hi) {                  // the whole quad is table: no per-pixel tests
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const float dx = dx0 + (float)i * inv_f;
            const float sdz = Xzs * dx + rz, dd = dx * dx + rd;
            const float a = __builtin_amdgcn_fmed3f(sdz * __builtin_amdgcn_rsqf(dd) * lam, 0.0f, 1.0f);
            v[i] = (uint32_t)(__builtin_amdgcn_fmed3f(a + c1, 0.0f, 1.0f) * 51.0f + 0.5f);  // table rgba .2 .2 .2: 255 * 0.2 = 51
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const float dx = (c + i + 0.5f - hw) * inv_f;
            const float sdz = Xzs * dx + rz, dd = dx * dx + rd;
            const float a = __builtin_amdgcn_fmed3f(sdz * __builtin_amdgcn_rsqf(dd) * lam, 0.0f, 1.0f);
            const float I = __builtin_amdgcn_fmed3f(a + c1, 0.0f, 1.0f);
            v[i] = (sdz > thr && dx > lo && dx < hi) ? (uint32_t)(51.0f * I + 0.5f) : 0u;
          }
        }
        // grey pixels: the three dwords are byte replications of the four values
        w0 = __builtin_amdgcn_perm(v[1], v[0], 0x04000000u);                         // v0 v0 v0 v1
        w1 = __builtin_amdgcn_perm(v[2], v[1], 0x04040000u);                         // v1 v1 v2 v2
        w2 = __builtin_amdgcn_perm(v[3], v[2], 0x04040400u);                         // v2 v3 v3 v3
      }
      out32[3 * q] = w0; out32[3 * q + 1] = w1; out32[3 * q + 2] = w2;       // (one global_store_dwordx3; non-temporal stores measured 11 % slower)
    }
  } else {
    for (int p = threadIdx.x; p < npix; p += blockDim.x) {
      const int r = p / width, c = p - r * width;
      uint32_t objs = 0;
      for (int o = 0; o <= g.nsph; o++)
        objs |= (uint32_t)(r >= g.box[o][0] && r <= g.box[o][1] && c >= g.box[o][2] && c <= g.box[o][3]) << o;
      const float dx = (c + 0.5f - hw) * inv_f, dy = -(r + 0.5f - hh) * inv_f;
      const uint32_t v = rgb_pixel<VIS>(g, gv, dx, dy, objs, rgb_over_table(g, dx, dy));
      out[3 * (size_t)p] = (uint8_t)v; out[3 * (size_t)p + 1] = (uint8_t)(v >> 8); out[3 * (size_t)p + 2] = (uint8_t)(v >> 16);
    }
  }
}

// ranges mode's values of every env's current episode (kmanip_get_visual_params): the draw the VIS kernels evaluate
__global__ void k_vp_draw(uint64_t seed, int64_t env_id_offset, int n, KVisArgs va, double* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * ((KM_VP_N + 1) / 2); i += gridDim.x * blockDim.x) {
    const int env = i % n, j = i / n;
    double o[2];
    km_vp_draw_pair(seed, env_id_offset + env, va.episode[env], j, va.range, o);
    out[(size_t)(2 * j) * n + env] = o[0];
    if (2 * j + 1 < KM_VP_N) out[(size_t)(2 * j + 1) * n + env] = o[1];
  }
}
void kmanip_launch_vp_draw(const KDeviceState& st, const KVisArgs& vis, double* out, hipStream_t stream) {
  const int n = st.num_envs, tot = n * ((KM_VP_N + 1) / 2), grid = (tot + 255) / 256 < 1024 ? (tot + 255) / 256 : 1024;
  hipLaunchKernelGGL(k_vp_draw, dim3(grid), dim3(256), 0, stream, st.seed, st.env_id_offset, n, vis, out);
}

void kmanip_launch_render_depth(const KDeviceModel* dm, const KDeviceState& st, int cam, int height, int width, float* depth,
                                const KVisArgs& vis, hipStream_t stream) {
  // 128 lanes per env: two waves -- 2048 envs x 2 waves fill the chip's 4096 wave slots (120 registers: four waves per SIMD) in one round
  const dim3 grid(st.num_envs), block(128);
  const bool colfixed = width > 0 && 128 % width == 0 && (height * width) % 128 == 0;
  if (km_vis_on(vis)) {
    if (colfixed) k_render_depth<true, true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth, vis);
    else k_render_depth<false, true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth, vis);
  } else {
    if (colfixed) k_render_depth<true, false><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth);
    else k_render_depth<false, false><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth);
  }
}
void kmanip_launch_render_rgb(const KDeviceModel* dm, const KDeviceState& st, const KRenderJobs& jobs, const KVisArgs& vis, hipStream_t stream) {
  const dim3 grid(st.num_envs, jobs.n), block(256);
  if (km_vis_on(vis)) k_render_rgb<true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, jobs, vis);
  else k_render_rgb<false><<<grid, block, 0, stream>>>(dm, st, jobs);
}
