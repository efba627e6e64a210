// kmanip_gae.hip -- generalised advantage estimation and value targets of a collect() buffer (include/kmanip.h KGaeIn ...; DESIGN.md
// section 48), float64 throughout, no atomics: the same call gives the same bytes.
//
// A DONE STEP CUTS THE RECURSION.  kmanip_dyn.hip's step epilogue sets KM_DONE_TRUNCATED when step_idx reaches max_episode_steps and
// KM_DONE_DIVERGED on a bad state, and with auto_reset (or a bad state) resets the env INSIDE the step and writes the new episode's
// first observation over obs_row.  obs[t + 1] after a done step is another episode's, and so is value[t + 1]: it is never read.  What
// the cut bootstraps from is 0, or the caller's timeout_value for a step that is truncated and did not diverge.
//
// k_gae: ONE LANE PER ENV COLUMN, so every load is coalesced across envs; the recurrence runs backward in time.  reward, done, value
// (and timeout_value) do not depend on the carry, only A does: the loads of a chunk of KM_GAE_CHUNK time steps are issued into
// registers before the chunk's dependent chain starts, so the chain never waits for memory more than once a chunk.  value[t + 1] of a
// chunk's last step is the value[t] the chunk after it (earlier in the loop) loaded: it is carried, not reloaded.  Each lane sums its
// rounded advantages and their squares in float64 in its loop order; the block then adds its lanes in a fixed order -- __shfl_xor
// within a wave (32, 16, 8, 4, 2, 1), then the waves through LDS, ascending -- and writes one pair to the workspace.
// k_gae_finish: thread 0 of every block sums the pairs in ascending block order (every block gets the same bits), block 0 writes
// stats, and with normalize each thread normalises one entry of adv in place.
#include "kmanip_device.hpp"

static_assert(KM_GAE_BLOCK % 64 == 0, "whole waves");

__global__ __launch_bounds__(KM_GAE_BLOCK) void k_gae(KGaeIn in, int T, int N, double* __restrict__ ws, KGaeDev out) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * KM_GAE_BLOCK + threadIdx.x;
  const bool live = e < N;
  const double gl = in.gamma * in.lambda;
  double A = 0.0, s1 = 0.0, s2 = 0.0;
  float vnext = 0.f;                                                 // value[t + 1] of the step in hand
  if (live) vnext = in.value[(size_t)T * N + e];
  for (int c = (T - 1) / KM_GAE_CHUNK; c >= 0; c--) {
    const int t0 = c * KM_GAE_CHUNK;
    double r[KM_GAE_CHUNK];
    float v[KM_GAE_CHUNK], tv[KM_GAE_CHUNK];
    uint8_t dn[KM_GAE_CHUNK];
#pragma unroll
    for (int j = 0; j < KM_GAE_CHUNK; j++) {                         // the chunk's loads: none depends on A
      r[j] = 0.0; v[j] = 0.f; tv[j] = 0.f; dn[j] = 0;
      if (live && t0 + j < T) {
        const size_t at = (size_t)(t0 + j) * N + e;
        r[j] = in.reward[at]; v[j] = in.value[at]; dn[j] = in.done[at];
        if (in.timeout_value) tv[j] = in.timeout_value[at];
      }
    }
#pragma unroll
    for (int j = KM_GAE_CHUNK - 1; j >= 0; j--) {
      if (live && t0 + j < T) {
        const bool d = dn[j] != 0;
        const bool boot = (dn[j] & KM_DONE_TRUNCATED) && !(dn[j] & KM_DONE_DIVERGED);
        const double nv = d ? (boot ? (double)tv[j] : 0.0) : (double)vnext;
        const double delta = (r[j] + in.gamma * nv) - (double)v[j];
        A = d ? delta : delta + gl * A;
        const float a = (float)A;
        const size_t at = (size_t)(t0 + j) * N + e;
        out.adv[at] = a;
        out.ret[at] = (float)(A + (double)v[j]);
        s1 = s1 + (double)a;
        s2 = s2 + (double)a * (double)a;
        vnext = v[j];
      }
    }
  }
  // ---- the block's pair: the lanes of a wave, then the waves ascending (a lane beyond N adds zeros)
  __shared__ double part[2 * (KM_GAE_BLOCK / 64)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 = s1 + __shfl_xor(s1, o, 64);
    s2 = s2 + __shfl_xor(s2, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[2 * wave] = s1; part[2 * wave + 1] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double b1 = 0.0, b2 = 0.0;
    for (int w = 0; w < KM_GAE_BLOCK / 64; w++) { b1 = b1 + part[2 * w]; b2 = b2 + part[2 * w + 1]; }
    ws[2 * (size_t)blockIdx.x] = b1;
    ws[2 * (size_t)blockIdx.x + 1] = b2;
  }
}

__global__ __launch_bounds__(256) void k_gae_finish(const double* __restrict__ ws, int nb, size_t count, int normalize, KGaeDev out) {
#pragma clang fp contract(off)
  __shared__ double ms[2];
  if (threadIdx.x == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < nb; b++) { s1 = s1 + ws[2 * (size_t)b]; s2 = s2 + ws[2 * (size_t)b + 1]; }
    const double mean = s1 / (double)count;
    const double sd = sqrt(fmax(s2 / (double)count - mean * mean, 0.0));
    ms[0] = mean; ms[1] = sd;
    if (blockIdx.x == 0 && out.stats) { out.stats[0] = mean; out.stats[1] = sd; }
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (normalize && i < count) out.adv[i] = (float)(((double)out.adv[i] - ms[0]) / (ms[1] + 1e-8));
}

void kmanip_launch_gae(const KGaeIn& in, int T, int N, double* ws, const KGaeDev& out, hipStream_t stream) {
  const int nb = (N + KM_GAE_BLOCK - 1) / KM_GAE_BLOCK;
  hipLaunchKernelGGL(k_gae, dim3(nb), dim3(KM_GAE_BLOCK), 0, stream, in, T, N, ws, out);
  if (!in.normalize && !out.stats) return;
  const size_t count = (size_t)T * N;
  const unsigned blocks = in.normalize ? (unsigned)((count + 255) / 256) : 1u;
  hipLaunchKernelGGL(k_gae_finish, dim3(blocks), dim3(256), 0, stream, ws, nb, count, in.normalize, out);
}
