// kmanip_actor_opt.hip -- the optimiser step of kmanip_actor's MLP (include/kmanip.h KActorAdamIn ...): the
// gradient norm and its clip, Adam, and BOTH PACKED BUFFERS rewritten while the new weights are in registers, so that no repack follows.
// Float64 per element, each stored value rounded to float32 once; no atomics: the same call gives the same bytes.
//
// k_actor_gradnorm: the seven gradient tensors as one concatenation, cut into `nb` slices of `per` elements.  A block of 256 threads
// sums its slice's g^2 in float64 -- thread i the elements i, i + 256, ... ascending, then __shfl_xor within a wave (32 .. 1), then the
// waves through LDS, ascending -- and writes one partial.  EVERY WAVE of k_actor_adam sums the partials again in ascending order (at
// most KM_ACTOR_ADAM_WS_DOUBLES uniform loads): there is no third launch, and every wave has the same bits of the norm.
//
// k_actor_adam: ONE WAVE OWNS ONE WORK ITEM (blocks of one wave).
//   A 16 x 16 TILE (t2, t) of a weight matrix, over the REAL K-blocks only: the zero blocks that pad a layer to KM_ACTOR_KGROUP are never
//   touched.  Lane l holds W[16 t2 + l % 16][16 t + 4 (l / 16) + 0..3] -- exactly its float4 of block (t2, t) in k_actor_pack's layout.  It
//   loads p, g, m, v of those four elements, each array as one 16-byte access where the row length is a multiple of 4 and that array's
//   pointer is 16-byte aligned (the test is wave-uniform and per array: the v half of the state often is not), else as guarded scalars;
//   updates them; stores p, m, v back row-major the same way; and stores the new float4 -- zeros where the guard fails -- to `packed`:
//   one coalesced 1 KB wave store.  For W1 and W2 the same tile is block (t, t2) of W^T in `packed_t`, whose lane l' wants
//   W[16 t2 + 4 (l' / 16) + c'][16 t + l' % 16]: the tile goes through a 16 x 17 LDS tile of the wave (four scalar writes, four scalar
//   reads a lane, the odd row length keeps both free of bank conflicts beyond two-way) and leaves as a second coalesced 1 KB store.
//   The alternative without LDS costs more: a source lane's four components go to four different destination lanes for each c', so the
//   selection cannot be made at the source -- 16 ds_bpermutes and 12 selects against 8 LDS accesses and one wave barrier.
//   A BIAS: lane j < 4 ot updates b[4 j .. 4 j + 3] and stores the float4 to the layer's padded bias block of `packed` (packed_t's bias
//   blocks are zeros and stay).  log_std: lane j < out_dim, no packed copy.
#include "kmanip_actor_layer.hpp"

#define KM_ADAM_NORM_SLICE 4096     // a block of k_actor_gradnorm takes at least this many elements

KActorAdamPlan kmanip_actor_adam_plan(const KActorDesc& d, bool with_log_std) {
  KActorAdamPlan ap;
  ap.p = kmanip_actor_plan(d);
  ap.t = kmanip_actor_grad_plan(d, 0).t;
  int item = 0, at = 0;
  for (int l = 0; l < 3; l++) {
    ap.rkb[l] = (ap.p.in[l] + 15) / 16;
    ap.item0[l] = item; item += ap.p.ot[l] * ap.rkb[l];
  }
  for (int l = 0; l < 3; l++) { ap.item0[3 + l] = item; item += 1; }
  ap.item0[6] = item; item += with_log_std ? 1 : 0;
  ap.item0[7] = item;
  for (int l = 0; l < 3; l++) {
    ap.off[2 * l] = at; at += ap.p.out[l] * ap.p.in[l];
    ap.off[2 * l + 1] = at; at += ap.p.out[l];
  }
  ap.off[6] = at; at += d.out_dim;
  ap.total = at;
  const int elems = with_log_std ? at : ap.off[6];
  ap.nb = std::min(KM_ACTOR_ADAM_WS_DOUBLES, (elems + KM_ADAM_NORM_SLICE - 1) / KM_ADAM_NORM_SLICE);
  ap.per = (elems + ap.nb - 1) / ap.nb;
  return ap;
}

struct KActorAdamPtrs { const float* g[7]; float* p[7]; };

__global__ __launch_bounds__(256) void k_actor_gradnorm(KActorAdamPlan ap, KActorAdamPtrs ptr, int elems, double* __restrict__ ws) {
#pragma clang fp contract(off)
  const int lo = blockIdx.x * ap.per, hi = min(elems, lo + ap.per);
  double s = 0.0;
  for (int e = lo + (int)threadIdx.x; e < hi; e += 256) {
    const float* gp = ptr.g[0];                                      // (selects, not an indexed array: the tensor varies by lane)
    int base = 0;
#pragma unroll
    for (int j = 1; j < 7; j++)
      if (e >= ap.off[j]) { gp = ptr.g[j]; base = ap.off[j]; }
    const double g = (double)gp[e - base];
    s = s + g * g;
  }
  __shared__ double part[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// four elements a[at + 0..3] of a row whose columns k0 .. k0 + 3 lie below `in` where they exist at all (rowok: the row does)
__device__ __forceinline__ f4 adam_load(const float* __restrict__ a, size_t at, bool vec, bool rowok, int k0, int in) {
  f4 r = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if (rowok && k0 < in) r = *(const f4*)(a + at);
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (rowok && k0 + c < in) r[c] = a[at + c];
  }
  return r;
}
__device__ __forceinline__ void adam_store(float* __restrict__ a, size_t at, bool vec, bool rowok, int k0, int in, f4 r) {
  if (vec) {
    if (rowok && k0 < in) *(f4*)(a + at) = r;
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (rowok && k0 + c < in) a[at + c] = r[c];
  }
}

// Adam on one element: g already widened and clipped
__device__ __forceinline__ void adam_elem(const KActorAdamHyper& hy, double c, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  const double gd = c * (double)g;
  m = (float)(hy.beta1 * (double)m + hy.omb1 * gd);
  v = (float)(hy.beta2 * (double)v + (hy.omb2 * gd) * gd);
  p = (float)((double)p - hy.step_size * ((double)m / (sqrt((double)v) / hy.sqrt_bc2 + hy.eps)));
}

__global__ __launch_bounds__(64) void k_actor_adam(KActorAdamPlan ap, KActorAdamHyper hy, KActorAdamPtrs ptr, float* __restrict__ state,
                                                  float* __restrict__ packed, float* __restrict__ packed_t, const double* __restrict__ ws,
                                                  int use_norm, double* __restrict__ gnorm) {
  __shared__ float tile[16 * 17];
  const int lane = threadIdx.x, item = blockIdx.x;
  // ---- the clip factor: every wave sums the partials in the same ascending order
  double c = 1.0;
  if (use_norm) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int b = 0; b < ap.nb; b++) s = s + ws[b];
    const double norm = sqrt(s);
    if (hy.max_norm > 0.0) c = fmin(1.0, hy.max_norm / (norm + 1e-6));
    if (item == 0 && lane == 0 && gnorm) *gnorm = norm;
  }
  int k = 0;                                                         // the item's kind: 0..2 a tile of W_k, 3..5 bias k - 3, 6 log_std
#pragma unroll
  for (int j = 1; j < 7; j++)
    if (item >= ap.item0[j]) k = j;
  if (k < 3) {
    const int l = k, local = item - ap.item0[l], t2 = local / ap.rkb[l], t = local - t2 * ap.rkb[l];
    const int in = ap.p.in[l], out = ap.p.out[l];
    const int r = 16 * t2 + (lane & 15), k0 = 16 * t + 4 * (lane >> 4);
    const bool rowok = r < out;
    const size_t at = (size_t)r * in + k0;
    const float* gp = ptr.g[2 * l];
    float *pp = ptr.p[2 * l], *mp = state + ap.off[2 * l], *vp = mp + ap.total;
    const bool row4 = (in & 3) == 0;
    const bool vg = row4 && !((uintptr_t)gp & 15), vpp = row4 && !((uintptr_t)pp & 15), vm = row4 && !((uintptr_t)mp & 15), vv = row4 && !((uintptr_t)vp & 15);
    const f4 g = adam_load(gp, at, vg, rowok, k0, in);
    f4 p = adam_load(pp, at, vpp, rowok, k0, in), m = adam_load(mp, at, vm, rowok, k0, in), v = adam_load(vp, at, vv, rowok, k0, in);
#pragma unroll
    for (int cc = 0; cc < 4; cc++)
      if (rowok && k0 + cc < in) {                                   // (beyond the guard p stays 0: the packed padding)
        float pe = p[cc], me = m[cc], ve = v[cc];
        adam_elem(hy, c, g[cc], pe, me, ve);
        p[cc] = pe; m[cc] = me; v[cc] = ve;
      }
    adam_store(pp, at, vpp, rowok, k0, in, p);
    adam_store(mp, at, vm, rowok, k0, in, m);
    adam_store(vp, at, vv, rowok, k0, in, v);
    ((f4*)packed)[ap.p.w4[l] + (size_t)(t2 * ap.p.kb[l] + t) * 64 + lane] = p;
    if (l > 0) {                                                     // W2^T is layer 0 of the transposed buffer, W1^T layer 1
      const int lt = 2 - l;
#pragma unroll
      for (int cc = 0; cc < 4; cc++) tile[(lane & 15) * 17 + 4 * (lane >> 4) + cc] = p[cc];
      __syncthreads();                                               // (one wave a block: a wave barrier)
      f4 q;
#pragma unroll
      for (int cc = 0; cc < 4; cc++) q[cc] = tile[(4 * (lane >> 4) + cc) * 17 + (lane & 15)];
      ((f4*)packed_t)[ap.t.w4[lt] + (size_t)(t * ap.t.kb[lt] + t2) * 64 + lane] = q;
    }
  } else if (k < 6) {
    const int l = k - 3, out = ap.p.out[l];
    if (lane < 4 * ap.p.ot[l]) {
      const float* gp = ptr.g[2 * l + 1];
      float *pp = ptr.p[2 * l + 1], *mp = state + ap.off[2 * l + 1], *vp = mp + ap.total;
      f4 p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int cc = 0; cc < 4; cc++) {
        const int j = 4 * lane + cc;
        if (j < out) {
          float pe = pp[j], me = mp[j], ve = vp[j];
          adam_elem(hy, c, gp[j], pe, me, ve);
          pp[j] = pe; mp[j] = me; vp[j] = ve;
          p[cc] = pe;
        }
      }
      ((f4*)packed)[ap.p.b4[l] + lane] = p;
    }
  } else if (lane < ap.p.out[2]) {
    float *pp = ptr.p[6], *mp = state + ap.off[6], *vp = mp + ap.total;
    float pe = pp[lane], me = mp[lane], ve = vp[lane];
    adam_elem(hy, c, ptr.g[6][lane], pe, me, ve);
    pp[lane] = pe; mp[lane] = me; vp[lane] = ve;
  }
}

void kmanip_launch_actor_adam(const KActorDesc& d, const KActorAdamIn& in, const KActorParams& params, float* state, float* packed, float* packed_t,
                              double* ws, double* gnorm, hipStream_t stream) {
  const bool ls = in.glog_std != nullptr, use_norm = in.max_grad_norm > 0.0 || gnorm;
  const KActorAdamPlan ap = kmanip_actor_adam_plan(d, ls);
  const KActorAdamPtrs ptr = {{in.gw0, in.gb0, in.gw1, in.gb1, in.gw2, in.gb2, in.glog_std},
                              {params.w0, params.b0, params.w1, params.b1, params.w2, params.b2, params.log_std}};
  const double bc1 = 1.0 - std::pow(in.beta1, (double)in.step), bc2 = 1.0 - std::pow(in.beta2, (double)in.step);
  const KActorAdamHyper hy = {in.beta1, 1.0 - in.beta1, in.beta2, 1.0 - in.beta2, in.lr / bc1, std::sqrt(bc2), in.eps, in.max_grad_norm};
  if (use_norm) hipLaunchKernelGGL(k_actor_gradnorm, dim3(ap.nb), dim3(256), 0, stream, ap, ptr, ls ? ap.total : ap.off[6], ws);
  hipLaunchKernelGGL(k_actor_adam, dim3(ap.item0[7]), dim3(64), 0, stream, ap, hy, ptr, state, packed, packed_t, ws, use_norm ? 1 : 0, gnorm);
}
