// kmanip_actor_grad.hip -- the loss gradients of kmanip_actor's MLP in its weights, biases and log_std, for rows of a rollout buffer,
// on the matrix cores (gfx950, wave64; float32 on v_mfma_f32_16x16x4_f32, float32 accumulation; include/kmanip.h KActorGradIn ...;
// DESIGN.md section 46).  Three launches a call, no atomics anywhere: the same call gives the same bytes.
//
// k_actor_bwd<NT>: ONE WAVE OWNS 16 ROWS, as in k_actor.  It recomputes the forward with k_actor's own actor_layer on the same packed
// buffer (x, h1, h2 stay in registers), runs the loss head in lane (g, n) on outputs 4 g .. 4 g + 3 of row n in float64, and then the
// data-gradient chain with the SAME register-resident hand-over, transposed: a D-layout tile of dz (VGPR r of lane group g: output unit
// 16 t + 4 g + r) is the B operand of K-step (t, r) of W^T dz, provided the A operand brings W^T's columns in that order -- which is
// k_actor_pack's layout fed with W^T.  k_actor_pack_t writes that second buffer (W2^T, then W1^T, each with a zero bias, so that
// actor_layer's bias load initialises the accumulator with zeros).  No LDS, no barrier, no shuffle between layers; act' is applied to
// the accumulators in place from the activated value.  The wave stores x, h1, h2, dz1, dz2, dz3 and the PPO head's log_std terms to
// the workspace UNIT-MAJOR, ws[unit][row] with the rows padded to 16: for a fixed VGPR, 16 consecutive lanes write 16 consecutive
// floats.  A row beyond n or with a record index out of range has dz = 0 in every layer: it adds exact zeros to every sum.
//
// k_actor_wgrad: dW_l = dz_l . h_(l-1)^T is a GEMM whose K dimension is the rows.  From unit-major storage both operands are the same
// access -- lane l reads [16 tile + l % 16][k0 + 4 (l / 16) + 0..3] as one float4: four K-steps, the K order within the group permuted
// alike for A and B.  A wave owns one dz tile against up to four h tiles (the A loads are reused four times); the wave of the first
// group of h tiles also multiplies the dz tile with a ones operand: the bias gradient, the row sums of dz.  The log_std gradient is
// the same row sum over the stored terms, one more work item.  K is split over KActorGradPlan::splits workgroups, a function of n
// only; each writes its partial tiles (D layout as it leaves the registers) to the workspace.
//
// k_actor_grad_reduce: one thread per element of the seven gradient tensors sums the partials in ascending split order and writes
// the row-major tensors without the tile padding.  With no splits (n == 0) it writes zeros.
#include "kmanip_actor_grad_head.hpp"   // agrad_row, agrad_obs, agrad_head: shared with k_actor_bwd_bf16; f4, actor_layer: with k_actor

#define KM_AGRAD_SPLIT_ROWS 256   // a K-split holds at least this many rows ...
#define KM_AGRAD_MAX_SPLITS 64    // ... and there are at most this many

KActorGradPlan kmanip_actor_grad_plan(const KActorDesc& d, int n) {
  KActorGradPlan gp;
  const KActorDesc td = {d.out_dim, {d.hidden[1], d.hidden[0]}, d.in_dim, d.activation};
  gp.t = kmanip_actor_plan(td);                       // layers 0 and 1 are W2^T and W1^T; the third is not stored
  gp.t.total4 = gp.t.w4[2];
  const int tiles_n = n > 16 ? (n + 15) / 16 : 1;
  gp.np = 16 * tiles_n;
  gp.splits = n == 0 ? 0 : std::min(KM_AGRAD_MAX_SPLITS, (gp.np + KM_AGRAD_SPLIT_ROWS - 1) / KM_AGRAD_SPLIT_ROWS);
  gp.len = 16 * ((tiles_n + std::max(gp.splits, 1) - 1) / std::max(gp.splits, 1));
  const int it0 = (d.in_dim + 15) / 16, t1 = d.hidden[0] / 16, t2 = d.hidden[1] / 16;
  const int units[KM_AGRAD_ARRAYS] = {16 * it0, 16 * t1, 16 * t2, 16 * t1, 16 * t2, 16, 16};      // x h1 h2 dz1 dz2 dz3 log_std terms
  size_t at = 0;
  for (int a = 0; a < KM_AGRAD_ARRAYS; a++) { gp.off[a] = at; at += (size_t)units[a] * gp.np; }
  // work items: layer l = 0..2 is dW_l, db_l from dz_(l+1) and the layer's input; 3 is the log_std row sum
  const int ot[4] = {t1, t2, 1, 1}, it[4] = {it0, t1, t2, 0}, dz[4] = {3, 4, 5, 6}, h[4] = {0, 1, 2, 0};
  int item = 0, tile = 0, bias = 0;
  for (int l = 0; l < 4; l++) {
    gp.ot[l] = ot[l]; gp.it[l] = it[l]; gp.itg[l] = std::max(1, (it[l] + 3) / 4);
    gp.dz[l] = gp.off[dz[l]]; gp.h[l] = gp.off[h[l]];
    gp.item0[l] = item; item += ot[l] * gp.itg[l];
    gp.tile0[l] = tile; tile += ot[l] * it[l];
    gp.bias0[l] = bias; bias += 16 * ot[l];
  }
  gp.item0[4] = item; gp.tiles = tile; gp.biases = bias;
  gp.part = at;
  gp.total = at + (size_t)gp.splits * ((size_t)tile * 256 + bias);
  return gp;
}

// one float4 of a transposed packed layer per thread: lane l's float4 of block (t2, t) is W^T[16 t2 + l % 16][16 t + 4 (l / 16) + 0..3]
// = W[16 t + 4 (l / 16) + 0..3][16 t2 + l % 16], W row-major [wout, win]; then a bias of zeros
__global__ __launch_bounds__(256) void k_actor_pack_t(const float* __restrict__ w, int win, int wout, int kb, int ot, f4* __restrict__ wdst,
                                                      f4* __restrict__ bdst) {
  const int i = blockIdx.x * 256 + threadIdx.x, nw = ot * kb * 64;
  f4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < nw) {
    const int lane = i & 63, blk = i >> 6, t2 = blk / kb, t = blk - t2 * kb;
    const int r = 16 * t2 + (lane & 15), k0 = 16 * t + 4 * (lane >> 4);
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (r < win && k0 + c < wout) v[c] = w[(size_t)(k0 + c) * win + r];
    wdst[i] = v;
  } else if (i < nw + ot * 4) bdst[i - nw] = v;
}

void kmanip_launch_actor_grad_pack(const KActorDesc& d, const KActorWeights& wt, float* packed_t, hipStream_t stream) {
  const KActorPlan p = kmanip_actor_grad_plan(d, 0).t;
  const float* w[2] = {wt.w2, wt.w1};
  f4* pk = (f4*)packed_t;
  for (int l = 0; l < 2; l++) {
    const int n4 = p.ot[l] * p.kb[l] * 64 + p.ot[l] * 4;
    hipLaunchKernelGGL(k_actor_pack_t, dim3((n4 + 255) / 256), dim3(256), 0, stream, w[l], p.out[l], p.in[l], p.kb[l], p.ot[l], pk + p.w4[l],
                       pk + p.b4[l]);
  }
}

// tiles [0, tiles) of a D-layout array to ws[unit][row]
template <int NTL>
__device__ __forceinline__ void agrad_store(float* __restrict__ base, size_t np, size_t rowpos, int tiles, const f4 (&v)[NTL], int g) {
#pragma unroll
  for (int t = 0; t < NTL; t++)
    if (t < tiles) {
#pragma unroll
      for (int c = 0; c < 4; c++) base[(size_t)(16 * t + 4 * g + c) * np + rowpos] = v[t][c];
    }
}

// dz[t] *= act'(h[t]), act' from the activated value
template <int NTL>
__device__ __forceinline__ void agrad_dact(f4 (&dz)[NTL], const f4 (&h)[NTL], int activation) {
#pragma unroll
  for (int t = 0; t < NTL; t++)
#pragma unroll
    for (int c = 0; c < 4; c++) dz[t][c] = activation == KM_ACTOR_TANH ? dz[t][c] * (1.f - h[t][c] * h[t][c]) : (h[t][c] > 0.f ? dz[t][c] : 0.f);
}

template <int NT>
__global__ __launch_bounds__(64) void k_actor_bwd(KActorDesc d, KActorPlan p, KActorGradPlan gp, const float* __restrict__ packed,
                                                  const float* __restrict__ packed_t, KActorGradIn in, int n, float* __restrict__ ws, KActorGradDev out) {
  static_assert(NT >= 4, "the first layer reads up to 64 inputs: four tiles");
  const f4 *pk = (const f4*)packed, *pkt = (const f4*)packed_t;
  const int lane = threadIdx.x, g = lane >> 4;
  const int id = d.in_dim, od = d.out_dim;
  const AgradRow rw = agrad_row(in, n, lane);
  const size_t np = gp.np, rowpos = rw.row;                          // (row < np: the grid is np / 16 waves)
  // ---- the forward, as k_actor has it
  f4 x[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
#pragma unroll
    for (int c = 0; c < 4; c++) x[t][c] = agrad_obs(in, rw, id, 16 * t + 4 * g + c);
  }
  f4 h1[NT], h2[NT], y[1];
  actor_layer<4, NT, true>(pk, p.w4[0], p.b4[0], p.kb[0], p.ot[0], d.activation, x, h1, lane);
  agrad_store<4>(ws + gp.off[0], np, rowpos, gp.it[0], x, g);
  actor_layer<NT, NT, true>(pk, p.w4[1], p.b4[1], p.kb[1], p.ot[1], d.activation, h1, h2, lane);
  actor_layer<NT, 1, false>(pk, p.w4[2], p.b4[2], p.kb[2], 1, d.activation, h2, y, lane);
  // ---- the head (kmanip_actor_grad_head.hpp): dL/dmean and the log_std terms coef (u^2 - 1)
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  f4 gm[1], lt[1];
  agrad_head(in, out, od, rw, g, y[0], gm[0], lt[0]);
  agrad_store<1>(ws + gp.off[5], np, rowpos, 1, gm, g);
  agrad_store<1>(ws + gp.off[6], np, rowpos, 1, lt, g);
  const f4 dz3[4] = {gm[0], zero, zero, zero};                       // one K group: the tile and three of zeros against the zero blocks
  // ---- the data gradients: dz2 = (W2^T dz3) act'(h2), dz1 = (W1^T dz2) act'(h1)
  f4 dz2[NT], dz1[NT];
  actor_layer<4, NT, false>(pkt, gp.t.w4[0], gp.t.b4[0], gp.t.kb[0], gp.t.ot[0], d.activation, dz3, dz2, lane);
  agrad_dact<NT>(dz2, h2, d.activation);
  agrad_store<NT>(ws + gp.off[2], np, rowpos, gp.t.ot[0], h2, g);
  agrad_store<NT>(ws + gp.off[4], np, rowpos, gp.t.ot[0], dz2, g);
  actor_layer<NT, NT, false>(pkt, gp.t.w4[1], gp.t.b4[1], gp.t.kb[1], gp.t.ot[1], d.activation, dz2, dz1, lane);
  agrad_dact<NT>(dz1, h1, d.activation);
  agrad_store<NT>(ws + gp.off[1], np, rowpos, gp.t.ot[1], h1, g);
  agrad_store<NT>(ws + gp.off[3], np, rowpos, gp.t.ot[1], dz1, g);
}

// blockIdx.x: work item (layer, dz tile, group of four h tiles); blockIdx.y: K-split
__global__ __launch_bounds__(64) void k_actor_wgrad(KActorGradPlan gp, float* __restrict__ ws) {
  const int lane = threadIdx.x, g = lane >> 4, split = blockIdx.y;
  int l = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if ((int)blockIdx.x >= gp.item0[k]) l = k;
  const int local = blockIdx.x - gp.item0[l], to = local / gp.itg[l], q = local - to * gp.itg[l], it = gp.it[l];
  const size_t np = gp.np;
  const float* a = ws + gp.dz[l] + (size_t)(16 * to + (lane & 15)) * np + 4 * g;
  const float* b = ws + gp.h[l] + (size_t)(64 * q + (lane & 15)) * np + 4 * g;
  const int k0 = split * gp.len, groups = max(0, min(gp.np, k0 + gp.len) - k0) / 16;     // (an empty split writes zeros)
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  f4 acc[4] = {zero, zero, zero, zero}, accb = zero;
  for (int i = 0; i < groups; i++) {
    const int k = k0 + 16 * i;
    const f4 av = *(const f4*)(a + k);
    f4 bv[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (4 * q + j < it) bv[j] = *(const f4*)(b + (size_t)16 * j * np + k);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (4 * q + j < it) {
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv[j].x, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv[j].y, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv[j].z, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv[j].w, acc[j], 0, 0, 0);
      }
    if (q == 0) {                                                    // the row sums of dz: every column of the product with ones
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, 1.f, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, 1.f, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, 1.f, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, 1.f, accb, 0, 0, 0);
    }
  }
  float* part = ws + gp.part + (size_t)split * ((size_t)gp.tiles * 256 + gp.biases);
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (4 * q + j < it) *(f4*)(part + (size_t)(gp.tile0[l] + to * it + 4 * q + j) * 256 + 4 * lane) = acc[j];
  if (q == 0 && (lane & 15) == 0) *(f4*)(part + (size_t)gp.tiles * 256 + gp.bias0[l] + 16 * to + 4 * g) = accb;
}

// element e of the concatenation w0 b0 w1 b1 w2 b2 log_std: the partials of its tile entry in ascending split order
__global__ __launch_bounds__(256) void k_actor_grad_reduce(KActorDesc d, KActorGradPlan gp, int head, const float* __restrict__ ws, KActorGradDev out) {
  const int dims[4] = {d.in_dim, d.hidden[0], d.hidden[1], d.out_dim};
  float* const wdst[3] = {out.w0, out.w1, out.w2};
  float* const bdst[4] = {out.b0, out.b1, out.b2, out.log_std};
  int e = blockIdx.x * 256 + threadIdx.x;
  float* dst = nullptr;
  size_t src = 0;
  bool found = false;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const int in = l < 3 ? dims[l] : 0, on = l < 3 ? dims[l + 1] : (head == KM_AGRAD_PPO_CLIP ? d.out_dim : 0);
    if (!found && e < on * in) {
      const int r = e / in, c = e - r * in;
      dst = wdst[l < 3 ? l : 0] + e;
      src = (size_t)(gp.tile0[l] + (r >> 4) * gp.it[l] + (c >> 4)) * 256 + 4 * ((c & 15) + 16 * ((r & 15) >> 2)) + (r & 3);
      found = true;
    }
    if (!found) e -= on * in;
    if (!found && e < on) {
      dst = bdst[l] + e;
      src = (size_t)gp.tiles * 256 + gp.bias0[l] + e;
      found = true;
    }
    if (!found) e -= on;
  }
  if (!found) return;
  const size_t stride = (size_t)gp.tiles * 256 + gp.biases;
  const float* part = ws + gp.part + src;
  float sum = 0.f;
  for (int s = 0; s < gp.splits; s++) sum += part[(size_t)s * stride];
  *dst = sum;
}

void kmanip_launch_actor_grad(const KActorDesc& d, const float* packed, const float* packed_t, const KActorGradIn& in, int n, float* ws,
                              const KActorGradDev& out, hipStream_t stream) {
  const KActorPlan p = kmanip_actor_plan(d);
  const KActorGradPlan gp = kmanip_actor_grad_plan(d, n);
  if (n > 0) {
    const dim3 grid(gp.np / 16), block(64);
    if (d.hidden[0] <= 64 && d.hidden[1] <= 64) hipLaunchKernelGGL(k_actor_bwd<4>, grid, block, 0, stream, d, p, gp, packed, packed_t, in, n, ws, out);
    else hipLaunchKernelGGL(k_actor_bwd<16>, grid, block, 0, stream, d, p, gp, packed, packed_t, in, n, ws, out);
    const int items = in.head == KM_AGRAD_PPO_CLIP ? gp.item0[4] : gp.item0[3];
    hipLaunchKernelGGL(k_actor_wgrad, dim3(items, gp.splits), block, 0, stream, gp, ws);
  }
  kmanip_launch_actor_grad_reduce(d, gp, in.head, ws, out, stream);
}

void kmanip_launch_actor_grad_reduce(const KActorDesc& d, const KActorGradPlan& gp, int head, const float* ws, const KActorGradDev& out,
                                     hipStream_t stream) {
  const int elems = d.hidden[0] * (d.in_dim + 1) + d.hidden[1] * (d.hidden[0] + 1) + d.out_dim * (d.hidden[1] + 2);
  hipLaunchKernelGGL(k_actor_grad_reduce, dim3((elems + 255) / 256), dim3(256), 0, stream, d, gp, head, ws, out);
}
