// kmanip_render_points.hip -- camera geometry out of the library:
//   k_camera_poses  : MuJoCo's cam_xpos / cam_xmat of one camera, per env, as the renders build it (kmanip_get_camera_poses)
//   k_render_points : the float64 depth ray cast with the pixel's point stored as float32 XYZ in the camera or the world frame, and
//                     the depth image from the same launch if wanted (kmanip_render_points)
// A translation unit of its own, as kmanip_render_labels.hip, kmanip_render_links.hip and kmanip_render_depth_links.hip are.  The
// cast of k_render_points lives in kmanip_render_depth_cast.inc, the one text k_render_depth and k_render_depth_links are built from
// too, and its scene struct, capsule record and capsule set-up in kmanip_render_depth_cast.hpp; what is this
// kernel's alone there -- its signature, its scalar-register policy and its store -- stands in that text's #if regions.
// tests/test_points_gpu.py holds the depth of this kernel to kmanip_render_depth's.
#include "kmanip_render_depth_cast.hpp"

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
// a pixel's point: three floats at a 4-byte aligned address, stored as ONE 12-byte access
struct __attribute__((packed, aligned(4))) PointXYZ { float x, y, z; };

// LINKS = false: the scene of k_render_depth; LINKS = true: plus the capsules of `la`, as k_render_depth_links tests them.
#define KM_CAST_MODE KM_CAST_POINTS
#include "kmanip_render_depth_cast.inc"

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
