// kmanip_actor_bfloat.hip -- k_actor_bf16: k_actor's network (kmanip_actor.hip) with bf16 weights and bf16 activations between the layers
// on v_mfma_f32_16x16x32_bf16 (gfx950, wave64; float32 biases, float32 accumulation, a float32 mean), and k_actor_pack_bf16, which
// rounds torch's row-major float32 nn.Linear tensors to nearest-even bf16 and lays them out for it (include/kmanip.h
// kmanip_actor_bf16).  The rows, the observation read, the status and the Gaussian head are k_actor's own source
// (kmanip_actor_head.hpp).
//
// ONE WAVE OWNS A TILE OF 16 ROWS and computes the transpose, as k_actor does: the weights are the A operand (16 units x 32 k), the
// activations the B operand (32 k x 16 envs).  Operand layouts of the instruction, lane l = (g = l / 16, n = l % 16):
//   A: eight bf16, A[n][8 g + 0..7]      B: eight bf16, B[8 g + 0..7][n]      D: VGPR r holds D[4 g + r][n]
// D is the float32 layout of k_actor: output tile t leaves lane group g with units 16 t + 4 g + r of env n in VGPR r.  A K-step gives
// lane group g EIGHT k-slots, so the four accumulators of tile 2 s followed by the four of tile 2 s + 1, each pair rounded by one
// v_cvt_pk_bf16_f32, ARE lane group g's B operand of K-step s of the next layer -- provided that step's A operand brings, in slot j of
// lane group g, the weight column  32 s + 4 g + j  (j < 4)  or  32 s + 16 + 4 g + (j - 4)  (j >= 4).  k_actor_pack_bf16 stores the
// weights in exactly that order.  The identity needs only that slot (g, j) of A meets slot (g, j) of B.  Between layers there is no
// LDS, no barrier and no shuffle; a layer's output is rounded to its NT / 2 operands once; an odd tile count pairs its last tile with
// a zero tile.  The first layer's operand is built the same way from the observation.
// THE PACKED BUFFER (kmanip_actor_bf16_plan), in 16-byte entries: per layer the weight blocks, then the float32 bias padded to whole
// tiles.  Block (output tile t2, K-step s) is 64 consecutive entries in lane order; a layer's K-steps are padded with zero blocks to a
// multiple of KM_ACTOR_BF16_KGROUP, the unit the hot loop guards by.  Every weight access is an unguarded, aligned 1 KB wave load.
// THE LOADS RUN ONE OUTPUT TILE AHEAD: two buffers of the layer's K-steps (at most 8 x 4 VGPRs each); tile t2 + 1's loads are issued
// before tile t2's MFMAs, which then wait for their own buffer alone.
#include "kmanip_actor_head.hpp"
#include "kmanip_actor_bfloat.hpp"   // bf8, actor_layer_bf16, actor_bf16_operands: shared with k_actor_bwd_bf16

KActorBf16Plan kmanip_actor_bf16_plan(const KActorDesc& d) {
  KActorBf16Plan p;
  const int dims[4] = {d.in_dim, d.hidden[0], d.hidden[1], d.out_dim};
  int at = 0;
  for (int l = 0; l < 3; l++) {
    p.in[l] = dims[l]; p.out[l] = dims[l + 1];
    p.ks[l] = ((dims[l] + 31) / 32 + KG - 1) / KG * KG;
    p.ot[l] = (dims[l + 1] + 15) / 16;
    p.w16[l] = at; at += p.ot[l] * p.ks[l] * 64;
    p.b16[l] = at; at += p.ot[l] * 4;
  }
  p.total16 = at;
  return p;
}

// one 16-byte entry of the packed layer per thread: the weight blocks (eight bf16, nearest-even), then the padded float32 bias
__global__ __launch_bounds__(256) void k_actor_pack_bf16(const float* __restrict__ w, const float* __restrict__ b, int in, int out, int ks, int ot,
                                                         f4* __restrict__ wdst, f4* __restrict__ bdst) {
  const int i = blockIdx.x * 256 + threadIdx.x, nw = ot * ks * 64;
  if (i < nw) {
    const int lane = i & 63, blk = i >> 6, t2 = blk / ks, s = blk - t2 * ks;
    const int r = 16 * t2 + (lane & 15), k0 = 32 * s + 4 * (lane >> 4);
    bf8 v;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int k = k0 + (j < 4 ? j : 12 + j);                       // 4 g + 0..3, then 16 + 4 g + 0..3
      v[j] = (__bf16)(r < out && k < in ? w[(size_t)r * in + k] : 0.f);
    }
    ((bf8*)wdst)[i] = v;
  } else if (i < nw + ot * 4) {
    const int j = i - nw;
    f4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (4 * j + c < out) v[c] = b[4 * j + c];
    bdst[j] = v;
  }
}

void kmanip_launch_actor_bf16_pack(const KActorDesc& d, const KActorWeights& wt, void* packed, hipStream_t stream) {
  const KActorBf16Plan p = kmanip_actor_bf16_plan(d);
  const float* w[3] = {wt.w0, wt.w1, wt.w2};
  const float* b[3] = {wt.b0, wt.b1, wt.b2};
  f4* pk = (f4*)packed;
  for (int l = 0; l < 3; l++) {
    const int n16 = p.ot[l] * p.ks[l] * 64 + p.ot[l] * 4;
    hipLaunchKernelGGL(k_actor_pack_bf16, dim3((n16 + 255) / 256), dim3(256), 0, stream, w[l], b[l], p.in[l], p.out[l], p.ks[l], p.ot[l],
                       pk + p.w16[l], pk + p.b16[l]);
  }
}

template <int NT>
__global__ __launch_bounds__(64) void k_actor_bf16(KDeviceState st, KActorDesc d, KActorBf16Plan p, const f4* __restrict__ pk, KActorIn in, int n,
                                                   KActorDev out) {
  static_assert(NT >= 4 && NT % 2 == 0, "the first layer reads up to 64 inputs: two K-steps; tiles pair up");
  const int lane = threadIdx.x, g = lane >> 4;
  const int id = d.in_dim;
  const ActorRow rw = actor_row(st, in, n, lane);
  // ---- the first layer's B operand: obs[row][32 s + 4 g + 0..3] and obs[row][32 s + 16 + 4 g + 0..3], float32 as k_actor's, then bf16
  bf8 x[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
#pragma unroll
    for (int j = 0; j < 8; j++) x[s][j] = (__bf16)actor_obs(in, rw, id, 32 * s + 4 * g + (j < 4 ? j : 12 + j));
  }
  f4 h[NT], y[1];
  bf8 x1[NT / 2], x2[NT / 2];
  actor_layer_bf16<2, NT, true>(pk, p.w16[0], p.b16[0], p.ks[0], p.ot[0], d.activation, x, h, lane);
  actor_bf16_operands<NT>(h, x1);
  actor_layer_bf16<NT / 2, NT, true>(pk, p.w16[1], p.b16[1], p.ks[1], p.ot[1], d.activation, x1, h, lane);
  actor_bf16_operands<NT>(h, x2);
  actor_layer_bf16<NT / 2, 1, false>(pk, p.w16[2], p.b16[2], p.ks[2], 1, d.activation, x2, y, lane);
  actor_head(st, in, out, d.out_dim, rw, g, y[0]);
}

void kmanip_launch_actor_bf16(const KDeviceState& st, const KActorDesc& d, const void* packed, const KActorIn& in, int n, const KActorDev& out,
                              hipStream_t stream) {
  const KActorBf16Plan p = kmanip_actor_bf16_plan(d);
  const dim3 grid((n + 15) / 16), block(64);
  const f4* pk = (const f4*)packed;
  if (d.hidden[0] <= 64 && d.hidden[1] <= 64) hipLaunchKernelGGL(k_actor_bf16<4>, grid, block, 0, stream, st, d, p, pk, in, n, out);
  else hipLaunchKernelGGL(k_actor_bf16<16>, grid, block, 0, stream, st, d, p, pk, in, n, out);
}
