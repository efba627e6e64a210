// kmanip_render_labels.hip -- per-pixel segmentation labels of the RGB ray cast: k_render_labels writes
// uint8 [num_envs, h, w] KM_SEG_* labels next to, or instead of, the bytes k_render_rgb writes, from one ray cast.  A translation
// unit of its own: compiled into kmanip_render.hip, the new kernels changed the code the compiler emits for k_render_rgb's shared
// set-up, and that kernel's code does not change.  The ray cast itself is label_cast<.., LINKS = false> of
// kmanip_render_label_cast.hpp, shared with k_render_links.
#include "kmanip_render_label_cast.hpp"

template <bool VIS, bool RGB, class... VA>
__global__ __launch_bounds__(256) void k_render_labels(const KDeviceModel* __restrict__ dm, KDeviceState st, KLabelJobs jobs, VA... vargs) {
  static_assert(sizeof...(VA) == (VIS ? 1 : 0), "the VIS kernel takes one KVisArgs, the default kernel none");
  KVisArgs va{};
  if constexpr (VIS) ((va = vargs), ...);
  label_cast<VIS, RGB, false>(dm, st, jobs, KLinkArgs{nullptr, 0}, va);
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
