// kmanip_normalize.hip -- running observation statistics and reward scaling for PPO (include/kmanip.h KObsStatsIn, KRewardScaleIn;
// DESIGN.md section 51): two reductions over a collect() buffer, each folded into a running state by Chan's merge.  Float64 throughout,
// no atomics, every sum in an order that is a function of the shape only: the same call on the same state gives the same bytes.
//
// THE SUMS ARE SHIFTED.  Both calls sum (x - c) and (x - c)^2 with c the state's mean (for an empty state the first value): a column
// at 1e3 with a spread of 1e-2 loses ten digits in sum x^2 - (sum x)^2 / R and none here.  c comes from memory the first launch only
// reads, so every lane derives it itself and no launch is spent on it.
//
// k_obs_stats: ROWS ARE CONTIGUOUS, so lane t of a block that uses L = dim floor(256 / dim) lanes owns column t % dim and row offset
// t / dim for the whole kernel, and one pass of the block reads L consecutive doubles: floor(256 / dim) whole rows, coalesced, no lane
// idle but the 256 - L at the end (13 at dim 27, 11 at 49, none at 64).  A lane keeps its two sums in registers; the loads of
// KM_OBS_STATS_UNROLL passes are issued before their dependent adds, as k_gae issues a chunk's.  A block owns a contiguous range of
// rows.  At the end the lanes of a column meet through LDS in ascending row offset and the block writes 2 dim partials.
// k_obs_stats_finish: one block; thread c < dim sums column c's partials in ascending block order, merges and writes the state and
// the two vectors.  A thread that walks the workspace itself pays one memory latency a block (measured: 116 us for 456 blocks, ten
// times k_obs_stats), so THE PARTIALS COME THROUGH LDS: all 256 lanes copy a tile of whole blocks' partials -- KM_OBS_FINISH_TILE
// doubles, 16 coalesced loads a lane, all in flight at once -- the next tile's loads are issued into registers before this tile's adds,
// and the column's thread adds from LDS, still in ascending block order.
// k_return_stats: k_gae's scheme run forward -- one lane per env, coalesced across envs, chunks of KM_GAE_CHUNK steps whose loads are
// issued before the chain; the block's pair is reduced as k_gae reduces its own.  The new carried returns and the state's moments as
// this launch read them go to the workspace: the second launch never reads the state it writes.
// k_reward_scale_finish: thread 0 of every block sums the pairs in ascending order and merges (every block gets the same bits), block
// 0 writes the state's moments and stats, thread i < N the carried return of env i, and each thread scales one entry.
#include "kmanip_device.hpp"

static_assert(KM_OBS_STATS_PASSES % KM_OBS_STATS_UNROLL == 0, "whole unrolled groups");
static_assert(KM_OBS_STATS_BLOCK >= KM_ACTOR_MAX_IN, "a pass holds at least one row, and the finish kernel one thread a column");
static_assert(KM_GAE_BLOCK % 64 == 0, "whole waves");

// A batch of R > 0 values with shifted sums (s1, s2) about c, merged into (na, ma, M2a): include/kmanip.h's definition, used by both calls
struct KMoments { double n, mean, M2; };
static __device__ __forceinline__ KMoments km_merge_moments(double na, double ma, double M2a, double R, double c, double s1, double s2) {
#pragma clang fp contract(off)
  const double mb = c + s1 / R;
  const double M2b = fmax(s2 - (s1 * s1) / R, 0.0);
  if (!(na > 0.0)) return {R, mb, M2b};
  const double n = na + R, delta = mb - ma;
  return {n, ma + (delta * R) / n, (M2a + M2b) + (((delta * delta) * na) * R) / n};
}

__global__ __launch_bounds__(KM_OBS_STATS_BLOCK) void k_obs_stats(const double* __restrict__ obs, int n_rows, int dim, int block_rows,
                                                                  const double* __restrict__ state, double* __restrict__ ws) {
#pragma clang fp contract(off)
  const int p = KM_OBS_STATS_BLOCK / dim, t = threadIdx.x;
  const bool owner = t < p * dim;
  const int col = t % dim, off = t / dim;
  const long long r0 = (long long)blockIdx.x * block_rows;
  const long long r1 = r0 + block_rows < n_rows ? r0 + block_rows : n_rows;      // this block's rows: [r0, r1)
  double s1 = 0.0, s2 = 0.0;
  if (owner) {
    const double c = state[0] > 0.0 ? state[1 + col] : obs[col];
    for (long long r = r0 + off; r < r1; r += (long long)KM_OBS_STATS_UNROLL * p) {
      double x[KM_OBS_STATS_UNROLL];
#pragma unroll
      for (int j = 0; j < KM_OBS_STATS_UNROLL; j++) {                              // the group's loads: none depends on the sums
        const long long rj = r + (long long)j * p;
        x[j] = rj < r1 ? obs[(size_t)rj * dim + col] : c;
      }
#pragma unroll
      for (int j = 0; j < KM_OBS_STATS_UNROLL; j++) {
        if (r + (long long)j * p < r1) {
          const double d = x[j] - c;
          s1 = s1 + d;
          s2 = s2 + d * d;
        }
      }
    }
  }
  // ---- the lanes of a column, ascending row offset (a lane without rows holds zeros)
  __shared__ double part[2][KM_OBS_STATS_BLOCK];
  part[0][t] = s1; part[1][t] = s2;
  __syncthreads();
  if (t < dim) {
    double b1 = 0.0, b2 = 0.0;
    for (int o = 0; o < p; o++) { b1 = b1 + part[0][o * dim + t]; b2 = b2 + part[1][o * dim + t]; }
    ws[(2 * (size_t)blockIdx.x) * dim + t] = b1;
    ws[(2 * (size_t)blockIdx.x + 1) * dim + t] = b2;
  }
}

#define KM_OBS_FINISH_TILE 4096                                                     // doubles of LDS: at least 32 blocks' partials (dim 64)
#define KM_OBS_FINISH_LOADS (KM_OBS_FINISH_TILE / KM_OBS_STATS_BLOCK)
__global__ __launch_bounds__(KM_OBS_STATS_BLOCK) void k_obs_stats_finish(const double* __restrict__ obs, int n_rows, int dim, int nb, double eps,
                                                                         const double* __restrict__ ws, double* __restrict__ state,
                                                                         double* __restrict__ obs_mean, double* __restrict__ obs_inv_std) {
#pragma clang fp contract(off)
  __shared__ double tile[KM_OBS_FINISH_TILE];
  const int c = threadIdx.x;
  const bool live = c < dim;
  const int fb = KM_OBS_FINISH_TILE / (2 * dim), per = fb * 2 * dim;               // whole blocks a tile, and their doubles
  const size_t total = 2 * (size_t)dim * nb;
  double pre[KM_OBS_FINISH_LOADS], s1 = 0.0, s2 = 0.0;
  auto fetch = [&](int k) {                                                        // tile k's share of this lane into registers
#pragma unroll
    for (int j = 0; j < KM_OBS_FINISH_LOADS; j++) {
      const int i = j * KM_OBS_STATS_BLOCK + c;
      const size_t at = (size_t)k * per + i;
      pre[j] = i < per && at < total ? ws[at] : 0.0;
    }
  };
  fetch(0);
  for (int k = 0; k * fb < nb; k++) {
#pragma unroll
    for (int j = 0; j < KM_OBS_FINISH_LOADS; j++) tile[j * KM_OBS_STATS_BLOCK + c] = pre[j];
    __syncthreads();
    fetch(k + 1);
    const int here = nb - k * fb < fb ? nb - k * fb : fb;
    if (live)
      for (int b = 0; b < here; b++) { s1 = s1 + tile[(2 * b) * dim + c]; s2 = s2 + tile[(2 * b + 1) * dim + c]; }
    __syncthreads();
  }
  const double na = state[0];
  KMoments m = {na, 0.0, 0.0};
  if (live) {
    m.mean = state[1 + c]; m.M2 = state[1 + dim + c];
    if (n_rows > 0) m = km_merge_moments(na, m.mean, m.M2, (double)n_rows, na > 0.0 ? m.mean : obs[c], s1, s2);
  }
  __syncthreads();                                                                 // every thread has read the count before it moves
  if (!live) return;
  if (n_rows > 0) {
    if (c == 0) state[0] = m.n;
    state[1 + c] = m.mean; state[1 + dim + c] = m.M2;
  }
  const bool empty = !(m.n > 0.0);
  if (obs_mean) obs_mean[c] = empty ? 0.0 : m.mean;
  if (obs_inv_std) obs_inv_std[c] = empty ? 1.0 : 1.0 / sqrt(m.M2 / m.n + eps);
}

__global__ __launch_bounds__(KM_GAE_BLOCK) void k_return_stats(KRewardScaleIn in, const double* __restrict__ state, double* __restrict__ ws) {
#pragma clang fp contract(off)
  const int T = in.T, N = in.N, nb = (N + KM_GAE_BLOCK - 1) / KM_GAE_BLOCK;
  const int e = blockIdx.x * KM_GAE_BLOCK + threadIdx.x;
  const bool live = e < N;
  const double c = state[0] > 0.0 ? state[1] : in.gamma * state[3] + in.reward[0];
  if (e == 0) { ws[0] = state[0]; ws[1] = state[1]; ws[2] = state[2]; ws[3] = c; }
  double G = live ? state[3 + e] : 0.0, s1 = 0.0, s2 = 0.0;
  for (int t0 = 0; t0 < T; t0 += KM_GAE_CHUNK) {
    double r[KM_GAE_CHUNK];
    uint8_t dn[KM_GAE_CHUNK];
#pragma unroll
    for (int j = 0; j < KM_GAE_CHUNK; j++) {                                       // the chunk's loads: none depends on G
      r[j] = 0.0; dn[j] = 0;
      if (live && t0 + j < T) { r[j] = in.reward[(size_t)(t0 + j) * N + e]; dn[j] = in.done[(size_t)(t0 + j) * N + e]; }
    }
#pragma unroll
    for (int j = 0; j < KM_GAE_CHUNK; j++) {
      if (live && t0 + j < T) {
        G = in.gamma * G + r[j];
        const double d = G - c;
        s1 = s1 + d;
        s2 = s2 + d * d;
        if (dn[j]) G = 0.0;
      }
    }
  }
  if (live) ws[4 + 2 * (size_t)nb + e] = G;
  // ---- the block's pair, as k_gae's: the lanes of a wave, then the waves ascending (a lane beyond N adds zeros)
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
    ws[4 + 2 * (size_t)blockIdx.x] = b1;
    ws[4 + 2 * (size_t)blockIdx.x + 1] = b2;
  }
}

__global__ __launch_bounds__(256) void k_reward_scale_finish(KRewardScaleIn in, const double* __restrict__ ws, double* __restrict__ state,
                                                             double* __restrict__ scaled, double* __restrict__ stats) {
#pragma clang fp contract(off)
  const int nb = (in.N + KM_GAE_BLOCK - 1) / KM_GAE_BLOCK;
  const size_t count = (size_t)in.T * in.N;
  __shared__ double sd;
  if (threadIdx.x == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < nb; b++) { s1 = s1 + ws[4 + 2 * (size_t)b]; s2 = s2 + ws[4 + 2 * (size_t)b + 1]; }
    const KMoments m = km_merge_moments(ws[0], ws[1], ws[2], (double)count, ws[3], s1, s2);
    sd = sqrt(m.M2 / m.n + in.eps);
    if (blockIdx.x == 0) {
      state[0] = m.n; state[1] = m.mean; state[2] = m.M2;
      if (stats) { stats[0] = m.mean; stats[1] = sqrt(m.M2 / m.n); }
    }
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)in.N) state[3 + i] = ws[4 + 2 * (size_t)nb + i];
  if (i < count) scaled[i] = in.reward[i] / sd;
}

size_t kmanip_obs_stats_block_rows(int n_rows, int dim) {
  const size_t q = (size_t)(KM_OBS_STATS_BLOCK / dim) * KM_OBS_STATS_PASSES, cap = q * KM_OBS_STATS_MAX_BLOCKS;
  const size_t k = ((size_t)n_rows + cap - 1) / cap;
  return q * (k > 1 ? k : 1);
}

void kmanip_launch_obs_stats(const KObsStatsIn& in, double* state, double* ws, double* obs_mean, double* obs_inv_std, hipStream_t stream) {
  int nb = 0;
  if (in.n_rows > 0) {
    const size_t rows = kmanip_obs_stats_block_rows(in.n_rows, in.dim);
    nb = (int)(((size_t)in.n_rows + rows - 1) / rows);
    hipLaunchKernelGGL(k_obs_stats, dim3(nb), dim3(KM_OBS_STATS_BLOCK), 0, stream, in.obs, in.n_rows, in.dim, (int)rows, state, ws);
  }
  hipLaunchKernelGGL(k_obs_stats_finish, dim3(1), dim3(KM_OBS_STATS_BLOCK), 0, stream, in.obs, in.n_rows, in.dim, nb, in.eps, ws, state, obs_mean, obs_inv_std);
}

void kmanip_launch_reward_scale(const KRewardScaleIn& in, double* state, double* ws, double* scaled, double* stats, hipStream_t stream) {
  const int nb = (in.N + KM_GAE_BLOCK - 1) / KM_GAE_BLOCK;
  hipLaunchKernelGGL(k_return_stats, dim3(nb), dim3(KM_GAE_BLOCK), 0, stream, in, state, ws);
  const size_t count = (size_t)in.T * in.N;
  hipLaunchKernelGGL(k_reward_scale_finish, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, in, ws, state, scaled, stats);
}
