// kmanip_actor_layer.hpp -- one layer of the MLP on a wave's tile of 16 rows, shared by k_actor (kmanip_actor.hip) and k_actor_bwd
// (kmanip_actor_grad.hip): the forward of both is this code on the same packed buffer, so the two agree to the bit.  The operand
// layouts and the packed buffer are described at the head of kmanip_actor.hip.
#pragma once
#include "kmanip_device.hpp"

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float actor_activate(float v, int activation) { return activation == KM_ACTOR_TANH ? tanhf(v) : fmaxf(v, 0.f); }

// One layer of the wave's tile: y[t2] (VGPR r of lane group g: unit 16 t2 + 4 g + r) from x[t] in the same layout.  NI / NO: the tile
// arrays' sizes; kb / ot: the layer's K-blocks (a multiple of KM_ACTOR_KGROUP) and output tiles.  Tiles of y beyond ot are zero: the
// next layer's padded K-blocks read them.
template <int NI, int NO, bool ACT>
__device__ __forceinline__ void actor_layer(const f4* __restrict__ pk, int w4, int b4, int kb, int ot, int activation, const f4 (&x)[NI], f4 (&y)[NO],
                                            int lane) {
  static_assert(NI % KM_ACTOR_KGROUP == 0, "whole K groups");
  const int g = lane >> 4;
#pragma unroll
  for (int t2 = 0; t2 < NO; t2++) {
    y[t2] = f4{0.f, 0.f, 0.f, 0.f};
    if (t2 < ot) {
      f4 acc = pk[b4 + 4 * t2 + g];                                 // the bias initialises the accumulator: units 16 t2 + 4 g + 0..3
      const f4* wr = pk + w4 + (size_t)t2 * kb * 64 + lane;
#pragma unroll
      for (int q = 0; q < NI / KM_ACTOR_KGROUP; q++) {
        if (q == 0 || KM_ACTOR_KGROUP * q < kb) {
          f4 w[KM_ACTOR_KGROUP];
#pragma unroll
          for (int j = 0; j < KM_ACTOR_KGROUP; j++) w[j] = wr[(KM_ACTOR_KGROUP * q + j) * 64];
#pragma unroll
          for (int j = 0; j < KM_ACTOR_KGROUP; j++) {
            const f4 xb = x[KM_ACTOR_KGROUP * q + j];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j].x, xb.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j].y, xb.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j].z, xb.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j].w, xb.w, acc, 0, 0, 0);
          }
        }
      }
      if (ACT) {
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c] = actor_activate(acc[c], activation);
      }
      y[t2] = acc;
    }
  }
}
