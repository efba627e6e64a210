// kmanip_render_links.hip -- the RGB / label ray cast with the arm links drawn as capsules: k_render_links
// is k_render_labels plus a per-handle list of link capsules (kmanip_set_render_links), launched instead of k_render_rgb /
// k_render_labels while a handle has such a list.  A translation unit of its own, as kmanip_render_labels.hip is: the code the
// compiler emits for the other render kernels does not change.  The ray cast itself is label_cast<.., LINKS = true> of
// kmanip_render_label_cast.hpp, shared with k_render_labels.
#include "kmanip_render_label_cast.hpp"

template <bool VIS, bool RGB, class... VA>
__global__ __launch_bounds__(256) void k_render_links(const KDeviceModel* __restrict__ dm, KDeviceState st, KLabelJobs jobs, KLinkArgs la, VA... vargs) {
  static_assert(sizeof...(VA) == (VIS ? 1 : 0), "the VIS kernel takes one KVisArgs, the default kernel none");
  KVisArgs va{};
  if constexpr (VIS) ((va = vargs), ...);
  label_cast<VIS, RGB, true>(dm, st, jobs, la, va);
}

void kmanip_launch_render_links(const KDeviceModel* dm, const KDeviceState& st, const KLabelJobs& jobs, bool rgb, const KLinkArgs& links, const KVisArgs& vis,
                                hipStream_t stream) {
  const dim3 grid(st.num_envs, jobs.n), block(256);
  if (km_vis_on(vis)) {
    if (rgb) k_render_links<true, true, KVisArgs><<<grid, block, 0, stream>>>(dm, st, jobs, links, vis);
    else k_render_links<true, false, KVisArgs><<<grid, block, 0, stream>>>(dm, st, jobs, links, vis);
  } else {
    if (rgb) k_render_links<false, true><<<grid, block, 0, stream>>>(dm, st, jobs, links);
    else k_render_links<false, false><<<grid, block, 0, stream>>>(dm, st, jobs, links);
  }
}
