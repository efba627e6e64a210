// kmanip_render_depth_cast.hpp -- what the float64 depth ray cast keeps outside its kernel, written once for
// the three kernels that run it: k_render_depth (kmanip_render.hip), k_render_depth_links (kmanip_render_depth_links.hip, section 15)
// and k_render_points (kmanip_render_points.hip, section 16).  The kernel itself is kmanip_render_depth_cast.inc, a source fragment
// each of those three files includes once with KM_CAST_MODE set to the kernel it wants; only those three include this header.
#pragma once
#include "kmanip_render_scene.hpp"

// KM_CAST_MODE of the including file: which kernel kmanip_render_depth_cast.inc spells
#define KM_CAST_DEPTH 0                // k_render_depth: the scene without capsules, a depth image
#define KM_CAST_DEPTH_LINKS 1          // k_render_depth_links: plus the capsule list, a depth image
#define KM_CAST_POINTS 2               // k_render_points<.., LINKS, ..>: either scene, points and, if wanted, the depth image

// what the pixel loop reads of the scene beyond RenderScene: the ray origin and the camera basis in the cube frame (so that the slab
// test's direction is linear in the pixel coordinates), and the visible spheres' centres from the host-built list
struct DepthScene { real ol[3], DX[3], DY[3], DZ[3]; real oc[KM_RENDER_MAXVIS][3], cc[KM_RENDER_MAXVIS]; int nvis; };

// One capsule as the pixel loop reads it: float64, relative to the camera origin o.  A, B the world end points of the axis,
// u = (B - A) / |B - A|, oa = o - A.  One contiguous record per capsule: a hit path reads it with a handful of wide LDS reads at one
// wave-uniform address (a broadcast), issued together.
struct alignas(16) DepthCap {
  real u[3], oa[3];
  real ou, len;                // oa.u, |B - A|
  real c, ca, cb;              // oa.oa - ou^2 - r^2; the end spheres' |oa|^2 - r^2, |ob|^2 - r^2
  int box[4];                  // screen rectangle r0, r1, c0, c1 (inclusive); r0 > r1: never tested
};
#define KM_CAP_LANE0 72                // lanes 72 .. 95 are idle after the FK (64 .. 67 place the spheres, 96 .. read the visual parameters
                                       // before it): one capsule per lane
static_assert(KM_CAP_LANE0 >= 64 + KM_RENDER_MAXVIS && KM_CAP_LANE0 + KM_MAX_LINK_CAPSULES <= 128, "one capsule per lane of the second wave");
static_assert(KM_MAX_LINK_CAPSULES <= 32, "the capsule masks are one uint32_t");

// A value every lane of the wave holds alike (read from LDS at a wave-uniform address), moved into a scalar register pair: with
// capsules the pixel loop keeps some forty such values next to a capsule's record, and as vector registers they do not fit four
// waves per SIMD.  U = false: left where it is.
template <bool U>
__device__ __forceinline__ real depth_uniform(real x) {
  if constexpr (!U) return x;
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return __builtin_bit_cast(real, (uint64_t)hi << 32 | lo);
}

// Capsule k of the list: ray constants and screen rectangle.  The rectangle follows link_setup of kmanip_render_label_cast.hpp: the
// union of the two end spheres' rectangles with rgb_scene's generous radius (the bounding box of a convex hull is that of its
// generators); either end not safely in front of the camera: the whole image; the camera not in cam_mask: empty.  One case more:
// both ends at or behind the camera plane by more than the radius (zc + r <= 0).  Every point of the capsule then has depth <= 0
// along the optical axis, a ray's t IS that depth (the direction's component along the axis is 1), and only t > 0 counts: the
// capsule can never be hit and gets the empty rectangle.  From a gripper camera that is most of the arm.
__device__ __forceinline__ void depth_link_setup(const RenderScene& sc, const KLinkCapsule& cp, int cam, int height, int width, DepthCap* dc) {
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
  if (!(cp.cam_mask >> cam & 1u) || (za + rad <= 0 && zb + rad <= 0)) { box[0] = height; box[1] = -1; box[2] = width; box[3] = -1; return; }   // (below every row a wave can hold)
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
