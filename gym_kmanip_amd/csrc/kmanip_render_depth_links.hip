// kmanip_render_depth_links.hip -- the float64 depth ray cast with the arm links drawn as capsules:
// k_render_depth_links is k_render_depth plus the handle's capsule list (kmanip_set_render_links), launched instead of
// k_render_depth while the handle's depth flag is on (kmanip_set_depth_links) and the list is not empty.  The cast lives in
// kmanip_render_depth_cast.inc, the one text k_render_depth and k_render_points are built from too, and
// its scene struct, capsule record and capsule set-up in kmanip_render_depth_cast.hpp; this file names the kernel and launches it.
// A translation unit of its own, as kmanip_render_labels.hip and kmanip_render_links.hip are.
#include "kmanip_render_depth_cast.hpp"

#define KM_CAST_MODE KM_CAST_DEPTH_LINKS
#include "kmanip_render_depth_cast.inc"

void kmanip_launch_render_depth_links(const KDeviceModel* dm, const KDeviceState& st, int cam, int height, int width, float* depth,
                                      const KLinkArgs& links, const KVisArgs& vis, hipStream_t stream) {
  // k_render_depth's launch: 128 lanes per env, and its rule for the COLFIXED instantiation
  const dim3 grid(st.num_envs), block(128);
  const bool colfixed = width > 0 && 128 % width == 0 && (height * width) % 128 == 0;
  if (km_vis_on(vis)) {
    if (colfixed) k_render_depth_links<true, true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth, links, vis);
    else k_render_depth_links<false, true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth, links, vis);
  } else {
    if (colfixed) k_render_depth_links<true, false><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth, links);
    else k_render_depth_links<false, false><<<grid, block, 0, stream>>>(dm, st, cam, height, width, depth, links);
  }
}
