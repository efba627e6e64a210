// kmanip_actor_bfloat.hpp -- one layer of the MLP on a wave's tile of 16 rows on v_mfma_f32_16x16x32_bf16 and the hand-over between
// layers, shared by k_actor_bf16 (kmanip_actor_bfloat.hip) and k_actor_bwd_bf16 (kmanip_actor_grad_bfloat.hip): the forward of both is
// this code on the same packed buffer, so the two agree to the bit.  The operand layouts and the packed buffer are described at the
// head of kmanip_actor_bfloat.hip.
#pragma once
#include "kmanip_actor_layer.hpp"

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
#define KG KM_ACTOR_BF16_KGROUP

// the K-steps of output tile t2 into one buffer: groups of KG, guarded as the MFMAs that read them are
template <int NK>
__device__ __forceinline__ void actor_bf16_load(const bf8* __restrict__ wr, int ks, bf8 (&w)[NK]) {
#pragma unroll
  for (int q = 0; q < NK / KG; q++) {
    if (q == 0 || KG * q < ks) {
#pragma unroll
      for (int j = 0; j < KG; j++) w[KG * q + j] = wr[(KG * q + j) * 64];
    }
  }
}

// One layer of the wave's tile: y[t2] (VGPR r of lane group g: unit 16 t2 + 4 g + r, float32, activated) from the NK K-step operands x.
// ks / ot: the layer's K-steps (a multiple of KG) and output tiles.  Tiles of y beyond ot are zero: the next layer's padded K-steps
// read them.
template <int NK, int NO, bool ACT>
__device__ __forceinline__ void actor_layer_bf16(const f4* __restrict__ pk, int w16, int b16, int ks, int ot, int activation, const bf8 (&x)[NK],
                                                 f4 (&y)[NO], int lane) {
  static_assert(NK % KG == 0, "whole K groups");
  const int g = lane >> 4;
  const bf8* wr = (const bf8*)pk + w16 + lane;
  bf8 w[2][NK];
  actor_bf16_load<NK>(wr, ks, w[0]);
#pragma unroll
  for (int t2 = 0; t2 < NO; t2++) {
    y[t2] = f4{0.f, 0.f, 0.f, 0.f};
    if (t2 < ot) {
      if (t2 + 1 < NO && t2 + 1 < ot) actor_bf16_load<NK>(wr + (size_t)(t2 + 1) * ks * 64, ks, w[(t2 + 1) & 1]);      // one tile ahead
      f4 acc = pk[b16 + 4 * t2 + g];                                // the bias initialises the accumulator: units 16 t2 + 4 g + 0..3
#pragma unroll
      for (int q = 0; q < NK / KG; q++) {
        if (q == 0 || KG * q < ks) {
#pragma unroll
          for (int j = 0; j < KG; j++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[t2 & 1][KG * q + j], x[KG * q + j], acc, 0, 0, 0);
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

// The hand-over: tiles 2 s and 2 s + 1 of a layer's float32 output, rounded to nearest-even bf16, are K-step s of the next layer.
template <int NO>
__device__ __forceinline__ void actor_bf16_operands(const f4 (&y)[NO], bf8 (&x)[NO / 2]) {
#pragma unroll
  for (int s = 0; s < NO / 2; s++) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      x[s][c] = (__bf16)y[2 * s][c];
      x[s][4 + c] = (__bf16)y[2 * s + 1][c];
    }
  }
}
