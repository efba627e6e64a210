// kmanip_actor.hip -- k_actor: a state-based MLP policy  in_dim -> H1 -> H2 -> out_dim  for rows of envs, on the matrix cores
// (gfx950, wave64; float32 weights, float32 accumulation on v_mfma_f32_16x16x4_f32), with a Gaussian head whose noise is a function
// of (seed, env, episode, step); and k_actor_pack, which lays torch's row-major nn.Linear tensors out for it (include/kmanip.h
// KActorDesc ...).
//
// ONE WAVE OWNS A TILE OF 16 ROWS and computes the TRANSPOSE, Y^T[unit][env] = W[unit][k] X^T[k][env]: the weights are the A operand
// (16 units x 4 k), the activations the B operand (4 k x 16 envs), the 16 envs the N columns.  Operand layouts of the instruction:
//   A: lane l holds A[l % 16][l / 16]      B: lane l holds B[l / 16][l % 16]      D: VGPR r of lane l holds D[4 (l / 16) + r][l % 16]
// so a 16-unit output tile t leaves lane group g = l / 16 with units 16 t + 4 g + r of env l % 16 in VGPR r -- and the B operand of
// a K-step wants lane group g to hold k = g.  VGPR r of output tile t therefore IS the B operand of the next layer's K-step (t, r),
// provided that step's A operand supplies the weight columns k = 16 t + 4 g + r: the order of a dot product's terms is free, and
// k_actor_pack stores the weights in exactly that order.  Between layers there is no LDS, no barrier and no shuffle; the activation
// is applied to the accumulators in place.  The first layer's B operand is built the same way from the observation (each lane reads
// obs[row][16 t + 4 g + 0..3]), the last layer is one tile whose lane (g, n) ends with outputs 4 g .. 4 g + 3 of env n and does that
// env's head work itself.
// THE PACKED BUFFER (kmanip_actor_plan): per layer the weight blocks, then the bias padded to whole tiles.  Block (output tile t2,
// K-block t) is 64 consecutive float4s in lane order, lane l's float4 = W[16 t2 + l % 16][16 t + 4 (l / 16) + 0..3], zero beyond the
// layer's real rows and columns; a layer's K-blocks are padded with zero blocks to a multiple of KM_ACTOR_KGROUP, the unit the hot
// loop loads and guards by (the activation tiles they meet are zero too).  Every weight access of k_actor is an unguarded, aligned,
// fully coalesced 1 KB wave load.
// Two instantiations: NT = 4 tiles a layer (both hidden sizes <= 64; no K guard at all) and NT = 16 (<= 256: 64 accumulator VGPRs a
// layer, two layers live).  Every tile loop is fully unrolled -- the accumulators are registers, never indexed at run time -- and
// guarded by wave-uniform tests against the layer's real tile counts.
// A row's results depend on that row's env and inputs only: a column of the product never meets another column.
#include "kmanip_actor_head.hpp"    // actor_row, actor_obs, actor_head: shared with k_actor_bf16; f4, actor_layer: with k_actor_bwd

KActorPlan kmanip_actor_plan(const KActorDesc& d) {
  KActorPlan p;
  const int dims[4] = {d.in_dim, d.hidden[0], d.hidden[1], d.out_dim};
  int at = 0;
  for (int l = 0; l < 3; l++) {
    p.in[l] = dims[l]; p.out[l] = dims[l + 1];
    p.kb[l] = ((dims[l] + 15) / 16 + KM_ACTOR_KGROUP - 1) / KM_ACTOR_KGROUP * KM_ACTOR_KGROUP;
    p.ot[l] = (dims[l + 1] + 15) / 16;
    p.w4[l] = at; at += p.ot[l] * p.kb[l] * 64;
    p.b4[l] = at; at += p.ot[l] * 4;
  }
  p.total4 = at;
  return p;
}

// one float4 of the packed layer per thread: the weight blocks, then the padded bias
__global__ __launch_bounds__(256) void k_actor_pack(const float* __restrict__ w, const float* __restrict__ b, int in, int out, int kb, int ot,
                                                    f4* __restrict__ wdst, f4* __restrict__ bdst) {
  const int i = blockIdx.x * 256 + threadIdx.x, nw = ot * kb * 64;
  f4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < nw) {
    const int lane = i & 63, blk = i >> 6, t2 = blk / kb, t = blk - t2 * kb;
    const int r = 16 * t2 + (lane & 15), k0 = 16 * t + 4 * (lane >> 4);
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (r < out && k0 + c < in) v[c] = w[(size_t)r * in + k0 + c];
    wdst[i] = v;
  } else if (i < nw + ot * 4) {
    const int j = i - nw;
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (4 * j + c < out) v[c] = b[4 * j + c];
    bdst[j] = v;
  }
}

void kmanip_launch_actor_pack(const KActorDesc& d, const KActorWeights& wt, float* packed, hipStream_t stream) {
  const KActorPlan p = kmanip_actor_plan(d);
  const float* w[3] = {wt.w0, wt.w1, wt.w2};
  const float* b[3] = {wt.b0, wt.b1, wt.b2};
  f4* pk = (f4*)packed;
  for (int l = 0; l < 3; l++) {
    const int n4 = p.ot[l] * p.kb[l] * 64 + p.ot[l] * 4;
    hipLaunchKernelGGL(k_actor_pack, dim3((n4 + 255) / 256), dim3(256), 0, stream, w[l], b[l], p.in[l], p.out[l], p.kb[l], p.ot[l], pk + p.w4[l],
                       pk + p.b4[l]);
  }
}

template <int NT>
__global__ __launch_bounds__(64) void k_actor(KDeviceState st, KActorDesc d, KActorPlan p, const float* __restrict__ packed, KActorIn in, int n,
                                              KActorDev out) {
  static_assert(NT >= 4, "the first layer reads up to 64 inputs: four tiles");
  const f4* pk = (const f4*)packed;
  const int lane = threadIdx.x, g = lane >> 4;
  const int id = d.in_dim;
  const ActorRow rw = actor_row(st, in, n, lane);                    // the row's env: kmanip_actor_head.hpp
  // ---- the first layer's B operand: obs[row][16 t + 4 g + 0..3], normalised in float64, cast once
  f4 x[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
#pragma unroll
    for (int c = 0; c < 4; c++) x[t][c] = actor_obs(in, rw, id, 16 * t + 4 * g + c);
  }
  f4 h1[NT], h2[NT], y[1];
  actor_layer<4, NT, true>(pk, p.w4[0], p.b4[0], p.kb[0], p.ot[0], d.activation, x, h1, lane);
  actor_layer<NT, NT, true>(pk, p.w4[1], p.b4[1], p.kb[1], p.ot[1], d.activation, h1, h2, lane);
  actor_layer<NT, 1, false>(pk, p.w4[2], p.b4[2], p.kb[2], 1, d.activation, h2, y, lane);
  // ---- lane (g, n): outputs 4 g .. 4 g + 3 of its row: the mean, the status and the Gaussian head
  actor_head(st, in, out, d.out_dim, rw, g, y[0]);
}

void kmanip_launch_actor(const KDeviceState& st, const KActorDesc& d, const float* packed, const KActorIn& in, int n, const KActorDev& out,
                         hipStream_t stream) {
  const KActorPlan p = kmanip_actor_plan(d);
  const dim3 grid((n + 15) / 16), block(64);
  if (d.hidden[0] <= 64 && d.hidden[1] <= 64) hipLaunchKernelGGL(k_actor<4>, grid, block, 0, stream, st, d, p, packed, in, n, out);
  else hipLaunchKernelGGL(k_actor<16>, grid, block, 0, stream, st, d, p, packed, in, n, out);
}
