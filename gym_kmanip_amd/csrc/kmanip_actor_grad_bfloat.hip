// kmanip_actor_grad_bfloat.hip -- kmanip_actor_grad_bf16: the loss gradients of the bf16 network kmanip_actor_bf16 evaluates, with bf16
// operands on v_mfma_f32_16x16x32_bf16 in every product (gfx950, wave64; float32 accumulation, float32 partials and results;
// include/kmanip.h kmanip_actor_grad_bf16 has the definition).  Three launches a call, no atomics: the same call
// gives the same bytes.  The rows, the observation read and the three heads are k_actor_bwd's own source (kmanip_actor_grad_head.hpp);
// the layers and the hand-over are k_actor_bf16's (kmanip_actor_bfloat.hpp), so the forward is kmanip_actor_bf16's to the bit.
//
// k_actor_pack_t_bf16: W2^T and W1^T rounded to nearest-even bf16 in k_actor_pack_bf16's block order for the network out_dim ->
// hidden[1] -> hidden[0], each with a float32 bias block of zeros, so that actor_layer_bf16 runs the transposed chain unchanged.
//
// k_actor_bwd_bf16<NT>: ONE WAVE OWNS 16 ROWS.  It recomputes x^, h1^, h2^ (kept as the NT / 2 bf16 operands they are: act' is taken
// from the rounded value) and the float32 mean, runs the head, and then the transposed chain with the same hand-over: tiles 2 s and
// 2 s + 1 of dz, rounded pairwise, are K-step s of W^T dz.  dz3^ enters as one K-step: its tile paired with a zero tile, then a zero
// step.  No LDS, no barrier, no scratch.
// THE STORES: x^, h1^, h2^, dz1^, dz2^, dz3^ go to the workspace unit-major in bf16, ws[unit][row], rows padded to 32.  In the D layout
// a lane holds units 4 g .. 4 g + 3 of ONE row: stored as they are that is 2-byte scattered stores.  Instead lanes n and n ^ 1 (rows n
// and n + 1, one quad_perm DPP move) exchange one packed pair each: the even lane ends with units 4 g, 4 g + 1 of both rows, the odd
// lane with units 4 g + 2, 4 g + 3, and each writes two 4-byte words {row n, row n + 1}.  Per store instruction the eight lanes of a
// unit cover one whole 32-byte segment.  The PPO head's log_std terms stay float32, as k_actor_bwd stores them.
//
// k_actor_wgrad_bf16: dW_l = dz_l^ . h_(l-1)^^T with the rows as K, 32 a step.  From unit-major bf16 storage A (the dz tile) and every
// B (an input tile) are the same access: lane (g, n) reads [16 tile + n][k0 + 8 g + 0..7] as one 16-byte load.  A wave owns one dz
// tile against up to EIGHT input tiles (their count is a template argument of the loop); every wave also multiplies the dz tile
// with a ones operand, and the wave of the first group stores that: the bias gradient.  The row loop is NOT unrolled, so the loads are double buffered by hand: two steps a trip, the loads of step i + 1 issued
// before the MFMAs of step i.  The log_std work item is k_actor_wgrad's float32 ones-product over the float32 terms.  The partial
// tiles have k_actor_wgrad's layout: k_actor_grad_reduce (kmanip_actor_grad.hip) is launched unchanged.
#include "kmanip_actor_grad_head.hpp"
#include "kmanip_actor_bfloat.hpp"

typedef int i4 __attribute__((ext_vector_type(4)));

#define KM_AGRAD_SPLIT_ROWS 256   // a K-split holds at least this many rows ...
#define KM_AGRAD_MAX_SPLITS 64    // ... and there are at most this many (as kmanip_actor_grad.hip)
#define KM_AGRAD_BF16_GROUP 8     // input tiles a wave of k_actor_wgrad_bf16 takes against its dz tile

KActorGradBf16Plan kmanip_actor_grad_bf16_plan(const KActorDesc& d, int n) {
  KActorGradBf16Plan bp = {};
  const KActorDesc td = {d.out_dim, {d.hidden[1], d.hidden[0]}, d.in_dim, d.activation};
  bp.t = kmanip_actor_bf16_plan(td);                  // layers 0 and 1 are W2^T and W1^T; the third is not stored
  bp.t.total16 = bp.t.w16[2];
  KActorGradPlan& gp = bp.g;
  const int steps = n > 32 ? (n + 31) / 32 : 1;
  gp.np = 32 * steps;
  gp.splits = n == 0 ? 0 : std::min(KM_AGRAD_MAX_SPLITS, (gp.np + KM_AGRAD_SPLIT_ROWS - 1) / KM_AGRAD_SPLIT_ROWS);
  gp.len = 32 * ((steps + std::max(gp.splits, 1) - 1) / std::max(gp.splits, 1));
  const int it0 = (d.in_dim + 15) / 16, t1 = d.hidden[0] / 16, t2 = d.hidden[1] / 16;
  const int units[KM_AGRAD_ARRAYS] = {16 * it0, 16 * t1, 16 * t2, 16 * t1, 16 * t2, 16, 16};      // x h1 h2 dz1 dz2 dz3 (bf16); log_std terms
  size_t at = 0;                                      // in 4-byte words: np is even, so every array begins on a 64-byte boundary
  for (int a = 0; a < KM_AGRAD_ARRAYS; a++) { gp.off[a] = at; at += (size_t)units[a] * gp.np / (a < 6 ? 2 : 1); }
  const int ot[4] = {t1, t2, 1, 1}, it[4] = {it0, t1, t2, 0}, dz[4] = {3, 4, 5, 6}, h[4] = {0, 1, 2, 0};
  int item = 0, tile = 0, bias = 0;
  for (int l = 0; l < 4; l++) {
    gp.ot[l] = ot[l]; gp.it[l] = it[l]; gp.itg[l] = std::max(1, (it[l] + KM_AGRAD_BF16_GROUP - 1) / KM_AGRAD_BF16_GROUP);
    gp.dz[l] = gp.off[dz[l]]; gp.h[l] = gp.off[h[l]];
    gp.item0[l] = item; item += ot[l] * gp.itg[l];
    gp.tile0[l] = tile; tile += ot[l] * it[l];
    gp.bias0[l] = bias; bias += 16 * ot[l];
  }
  gp.item0[4] = item; gp.tiles = tile; gp.biases = bias;
  gp.part = at;
  gp.total = at + (size_t)gp.splits * ((size_t)tile * 256 + bias);
  return bp;
}

// one 16-byte entry of a transposed packed layer per thread: slot j of lane l of block (t2, s) is W^T[16 t2 + l % 16][k] = W[k][16 t2 +
// l % 16] with k = 32 s + 4 (l / 16) + j (j < 4) or 32 s + 16 + 4 (l / 16) + (j - 4), W row-major [wout, win]; then a bias of zeros
__global__ __launch_bounds__(256) void k_actor_pack_t_bf16(const float* __restrict__ w, int win, int wout, int ks, int ot, f4* __restrict__ wdst,
                                                           f4* __restrict__ bdst) {
  const int i = blockIdx.x * 256 + threadIdx.x, nw = ot * ks * 64;
  if (i < nw) {
    const int lane = i & 63, blk = i >> 6, t2 = blk / ks, s = blk - t2 * ks;
    const int r = 16 * t2 + (lane & 15), k0 = 32 * s + 4 * (lane >> 4);
    bf8 v;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int k = k0 + (j < 4 ? j : 12 + j);
      v[j] = (__bf16)(r < win && k < wout ? w[(size_t)k * win + r] : 0.f);
    }
    ((bf8*)wdst)[i] = v;
  } else if (i < nw + ot * 4) bdst[i - nw] = f4{0.f, 0.f, 0.f, 0.f};
}

void kmanip_launch_actor_grad_bf16_pack(const KActorDesc& d, const KActorWeights& wt, void* packed_t, hipStream_t stream) {
  const KActorBf16Plan p = kmanip_actor_grad_bf16_plan(d, 0).t;
  const float* w[2] = {wt.w2, wt.w1};
  f4* pk = (f4*)packed_t;
  for (int l = 0; l < 2; l++) {
    const int n16 = p.ot[l] * p.ks[l] * 64 + p.ot[l] * 4;
    hipLaunchKernelGGL(k_actor_pack_t_bf16, dim3((n16 + 255) / 256), dim3(256), 0, stream, w[l], p.out[l], p.in[l], p.ks[l], p.ot[l], pk + p.w16[l],
                       pk + p.b16[l]);
  }
}

// Tiles [0, tiles) of an array held as K-step operands (slots 0..3 of v[s]: tile 2 s, slots 4..7: tile 2 s + 1; lane (g, n): units
// 4 g + 0..3 of row n) to ws[unit][row] in bf16.  `arr`: the array's first word; row0: the wave's first row.  Lanes n and n ^ 1 swap one
// packed pair: the even lane then holds units 4 g, 4 g + 1 of rows n, n + 1, the odd lane units 4 g + 2, 4 g + 3 of rows n - 1, n.
// Every lane of the wave calls it (`tiles` is wave-uniform).
template <int NK>
__device__ __forceinline__ void agrad_store_bf16(float* __restrict__ arr, size_t np, size_t row0, int tiles, const bf8 (&v)[NK], int lane) {
  const bool odd = lane & 1;
  int* dst = (int*)arr + ((size_t)(4 * (lane >> 4) + (odd ? 2 : 0)) * np + row0 + (lane & 14)) / 2;
#pragma unroll
  for (int s = 0; s < NK; s++) {
    const i4 dw = __builtin_bit_cast(i4, v[s]);
#pragma unroll
    for (int half = 0; half < 2; half++) {
      if (2 * s + half < tiles) {
        const int a = dw[2 * half], b = dw[2 * half + 1];              // (units 4 g, 4 g + 1) and (4 g + 2, 4 g + 3) of this lane's row
        const int recv = __builtin_amdgcn_update_dpp(0, odd ? a : b, 0xB1, 0xF, 0xF, true);      // quad_perm [1, 0, 3, 2]
        const int mine = odd ? b : a, lo = odd ? recv : mine, hi = odd ? mine : recv;             // lo: the even row, hi: the odd row
        int* at = dst + (size_t)8 * (2 * s + half) * np;
        at[0] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);            // the pair's first unit, rows n, n + 1
        at[np / 2] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);       // its second unit
      }
    }
  }
}

// dz[t] *= act'(h^), act' from the rounded activation widened to float32; h as the operands the next layer read
template <int NT>
__device__ __forceinline__ void agrad_dact_bf16(f4 (&dz)[NT], const bf8 (&h)[NT / 2], int activation) {
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const float hv = (float)h[t / 2][4 * (t & 1) + c];
      dz[t][c] = activation == KM_ACTOR_TANH ? dz[t][c] * (1.f - hv * hv) : (hv > 0.f ? dz[t][c] : 0.f);
    }
}

template <int NT>
__global__ __launch_bounds__(64) void k_actor_bwd_bf16(KActorDesc d, KActorBf16Plan p, KActorGradBf16Plan bp, const f4* __restrict__ pk,
                                                       const f4* __restrict__ pkt, KActorGradIn in, int n, float* __restrict__ ws, KActorGradDev out) {
  static_assert(NT >= 4 && NT % 2 == 0, "the first layer reads up to 64 inputs: two K-steps; tiles pair up");
  const KActorGradPlan& gp = bp.g;
  const int lane = threadIdx.x, g = lane >> 4;
  const int id = d.in_dim, od = d.out_dim;
  const AgradRow rw = agrad_row(in, n, lane);
  const size_t np = gp.np, row0 = (size_t)blockIdx.x * 16;           // (row < np: the grid is np / 16 waves)
  // ---- the forward, as k_actor_bf16 has it
  bf8 x[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
#pragma unroll
    for (int j = 0; j < 8; j++) x[s][j] = (__bf16)agrad_obs(in, rw, id, 32 * s + 4 * g + (j < 4 ? j : 12 + j));
  }
  agrad_store_bf16<2>(ws + gp.off[0], np, row0, gp.it[0], x, lane);
  f4 h[NT], y[1];
  bf8 x1[NT / 2], x2[NT / 2], dzo[NT / 2];
  actor_layer_bf16<2, NT, true>(pk, p.w16[0], p.b16[0], p.ks[0], p.ot[0], d.activation, x, h, lane);
  actor_bf16_operands<NT>(h, x1);
  agrad_store_bf16<NT / 2>(ws + gp.off[1], np, row0, gp.it[1], x1, lane);
  actor_layer_bf16<NT / 2, NT, true>(pk, p.w16[1], p.b16[1], p.ks[1], p.ot[1], d.activation, x1, h, lane);
  actor_bf16_operands<NT>(h, x2);
  agrad_store_bf16<NT / 2>(ws + gp.off[2], np, row0, gp.it[2], x2, lane);
  actor_layer_bf16<NT / 2, 1, false>(pk, p.w16[2], p.b16[2], p.ks[2], 1, d.activation, x2, y, lane);
  // ---- the head (kmanip_actor_grad_head.hpp); the log_std terms stay float32
  f4 gm, lt;
  agrad_head(in, out, od, rw, g, y[0], gm, lt);
#pragma unroll
  for (int c = 0; c < 4; c++) ws[gp.off[6] + (size_t)(4 * g + c) * np + rw.row] = lt[c];
  // ---- the data gradients: dz3^ = bf16(gmean), dz2 = (W2^T^ dz3^) act'(h2^), dz1 = (W1^T^ dz2^) act'(h1^), each rounded once
  bf8 dz3[2];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dz3[0][j] = (__bf16)(j < 4 ? gm[j & 3] : 0.f);                     // one K-step: the tile paired with a zero tile; then the zero step
    dz3[1][j] = (__bf16)0.f;
  }
  agrad_store_bf16<2>(ws + gp.off[5], np, row0, 1, dz3, lane);
  actor_layer_bf16<2, NT, false>(pkt, bp.t.w16[0], bp.t.b16[0], bp.t.ks[0], bp.t.ot[0], d.activation, dz3, h, lane);
  agrad_dact_bf16<NT>(h, x2, d.activation);
  actor_bf16_operands<NT>(h, dzo);
  agrad_store_bf16<NT / 2>(ws + gp.off[4], np, row0, bp.t.ot[0], dzo, lane);
  actor_layer_bf16<NT / 2, NT, false>(pkt, bp.t.w16[1], bp.t.b16[1], bp.t.ks[1], bp.t.ot[1], d.activation, dzo, h, lane);
  agrad_dact_bf16<NT>(h, x1, d.activation);
  actor_bf16_operands<NT>(h, dzo);
  agrad_store_bf16<NT / 2>(ws + gp.off[3], np, row0, bp.t.ot[1], dzo, lane);
}

// The K loop of one work item with NB input tiles, a compile-time count (no guard inside the loop: a guarded load makes the compiler
// wait for every load in flight before each MFMA).  Step i: rows 32 i .. 32 i + 31 from a and b, which point at this lane's eight
// bf16 of the first step; input tile j is 16 j np elements further.  acc[j]: the tile's partial; accb: the product with ones.
template <int NB>
__device__ __forceinline__ void agrad_wgrad_tiles(const __bf16* __restrict__ a, const __bf16* __restrict__ b, size_t np, int steps,
                                                  f4 (&acc)[KM_AGRAD_BF16_GROUP], f4& accb) {
  bf8 ones, av[2], bv[2][NB];
#pragma unroll
  for (int j = 0; j < 8; j++) ones[j] = (__bf16)1.f;
  auto load = [&](int buf, int i) {
    av[buf] = *(const bf8*)(a + 32 * i);
#pragma unroll
    for (int j = 0; j < NB; j++) bv[buf][j] = *(const bf8*)(b + (size_t)16 * j * np + 32 * i);
  };
  auto mma = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NB; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[buf], bv[buf][j], acc[j], 0, 0, 0);
    accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[buf], ones, accb, 0, 0, 0);
  };
  if (steps > 0) load(0, 0);
  int i = 0;
  for (; i + 2 <= steps; i += 2) {                                     // two steps a trip: each buffer's loads go out a step before its MFMAs
    load(1, i + 1);
    mma(0);
    if (i + 2 < steps) load(0, i + 2);
    mma(1);
  }
  if (i < steps) mma(0);                                               // an odd count: the last step is already in buffer 0
}

// blockIdx.x: work item (layer, dz tile, group of eight input tiles); blockIdx.y: K-split
__global__ __launch_bounds__(64) void k_actor_wgrad_bf16(KActorGradPlan gp, float* __restrict__ ws) {
  const int lane = threadIdx.x, g = lane >> 4, split = blockIdx.y;
  int l = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if ((int)blockIdx.x >= gp.item0[k]) l = k;
  const int local = blockIdx.x - gp.item0[l], to = local / gp.itg[l], q = local - to * gp.itg[l], it = gp.it[l];
  const size_t np = gp.np;
  const int k0 = split * gp.len, rows = max(0, min(gp.np, k0 + gp.len) - k0);      // a multiple of 32 (an empty split writes zeros)
  float* part = ws + gp.part + (size_t)split * ((size_t)gp.tiles * 256 + gp.biases);
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  f4 accb = zero;
  if (l == 3) {                                                        // the log_std terms: float32, the product with ones as k_actor_wgrad has it
    const float* a = ws + gp.dz[3] + (size_t)(lane & 15) * np + 4 * g + k0;
    for (int i = 0; i < rows / 16; i++) {
      const f4 av = *(const f4*)(a + 16 * i);
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, 1.f, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, 1.f, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, 1.f, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, 1.f, accb, 0, 0, 0);
    }
    if ((lane & 15) == 0) *(f4*)(part + (size_t)gp.tiles * 256 + gp.bias0[3] + 4 * g) = accb;
    return;
  }
  const __bf16* a = (const __bf16*)(ws + gp.dz[l]) + (size_t)(16 * to + (lane & 15)) * np + 8 * g + k0;
  const __bf16* b = (const __bf16*)(ws + gp.h[l]) + (size_t)(16 * KM_AGRAD_BF16_GROUP * q + (lane & 15)) * np + 8 * g + k0;
  const int nb = min(KM_AGRAD_BF16_GROUP, it - KM_AGRAD_BF16_GROUP * q), steps = rows / 32;
  f4 acc[KM_AGRAD_BF16_GROUP];
#pragma unroll
  for (int j = 0; j < KM_AGRAD_BF16_GROUP; j++) acc[j] = zero;
  switch (nb) {                                                        // (wave-uniform)
    case 1: agrad_wgrad_tiles<1>(a, b, np, steps, acc, accb); break;
    case 2: agrad_wgrad_tiles<2>(a, b, np, steps, acc, accb); break;
    case 3: agrad_wgrad_tiles<3>(a, b, np, steps, acc, accb); break;
    case 4: agrad_wgrad_tiles<4>(a, b, np, steps, acc, accb); break;
    case 5: agrad_wgrad_tiles<5>(a, b, np, steps, acc, accb); break;
    case 6: agrad_wgrad_tiles<6>(a, b, np, steps, acc, accb); break;
    case 7: agrad_wgrad_tiles<7>(a, b, np, steps, acc, accb); break;
    default: agrad_wgrad_tiles<8>(a, b, np, steps, acc, accb); break;
  }
#pragma unroll
  for (int j = 0; j < KM_AGRAD_BF16_GROUP; j++)
    if (j < nb) *(f4*)(part + (size_t)(gp.tile0[l] + to * it + KM_AGRAD_BF16_GROUP * q + j) * 256 + 4 * lane) = acc[j];
  if (q == 0 && (lane & 15) == 0) *(f4*)(part + (size_t)gp.tiles * 256 + gp.bias0[l] + 16 * to + 4 * g) = accb;
}

void kmanip_launch_actor_grad_bf16(const KActorDesc& d, const void* packed, const void* packed_t, const KActorGradIn& in, int n, void* workspace,
                                   const KActorGradDev& out, hipStream_t stream) {
  const KActorBf16Plan p = kmanip_actor_bf16_plan(d);
  const KActorGradBf16Plan bp = kmanip_actor_grad_bf16_plan(d, n);
  const f4 *pk = (const f4*)packed, *pkt = (const f4*)packed_t;
  float* ws = (float*)workspace;
  if (n > 0) {
    const dim3 grid(bp.g.np / 16), block(64);
    if (d.hidden[0] <= 64 && d.hidden[1] <= 64) hipLaunchKernelGGL(k_actor_bwd_bf16<4>, grid, block, 0, stream, d, p, bp, pk, pkt, in, n, ws, out);
    else hipLaunchKernelGGL(k_actor_bwd_bf16<16>, grid, block, 0, stream, d, p, bp, pk, pkt, in, n, ws, out);
    const int items = in.head == KM_AGRAD_PPO_CLIP ? bp.g.item0[4] : bp.g.item0[3];
    hipLaunchKernelGGL(k_actor_wgrad_bf16, dim3(items, bp.g.splits), block, 0, stream, bp.g, ws);
  }
  kmanip_launch_actor_grad_reduce(d, bp.g, in.head, ws, out, stream);
}
