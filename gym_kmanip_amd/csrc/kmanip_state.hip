// kmanip_state.hip -- the env state in and out of a handle on the device (include/kmanip.h: kmanip_get_state_dev,
// kmanip_set_state_dev, kmanip_copy_envs).  No step or render kernel is touched and no field of
// KDeviceState / KDeviceModel moves: the kernels here take the state's pointers in structs of their own.
//
// The state is component-major ([K][N], element (k, env) at k * N + env: what the step kernels read coalesced), the caller's
// tensors are env-major ([n][K], row j = env index[j]).  Two shapes of kernel, each ONE launch per call for every field, the
// counters, the bound sim time and the index check:
//   k_state_io<IMPORT>   state <-> tensors.  A workgroup takes a tile of KS_TILE = 64 consecutive ROWS of one field.  The state
//                        side is accessed lane = row, one component per wave instruction (64 consecutive doubles for a NULL or
//                        sorted index); the tensor side as the tile's rows * K consecutive doubles; in between the tile sits in
//                        LDS as [row][KP] with KP = K | 1.
//                        Banks (8-byte accesses): the column side puts lane j at dword 2 KP j + 2 k.  A store is served 16 lanes
//                        at a time on 32 banks, a load 32 lanes at a time on 64 banks: both are free of conflicts when
//                        KP j mod 16 (mod 32) is distinct over 16 (32) consecutive j, i.e. for every ODD KP.  The row side walks
//                        the tile in address order with a one-double gap per row where K is even (K = 16, 10, 26, 20 -> KP 17,
//                        11, 27, 21; K = 17, 27 stay): 32 lanes then span at most 32 + 3 doubles, a two-way conflict on at most
//                        3 of them.
//   k_state_gather       state -> state (between two handles, or into / out of the staging copy of a same-handle call).  Both
//                        sides are component-major: lane = destination row, stores coalesced, loads gathered by the source index
//                        (a broadcast reads one address per wave).  A thread moves KS_CPT components of its row, loads first.
// An index entry outside 0 .. range-1 is never used as an address: the entry is skipped and the handle's error counter gets one
// atomicAdd (from the workgroups of the first field / component chunk only, so that an entry counts once).
#include <hip/hip_runtime.h>

#include "kmanip_device.hpp"

#define KS_TILE 64
#define KS_KMAX 27    // nq of the 20-link models
#define KS_CPT 8      // components per thread of k_state_gather

template <bool IMPORT>
__global__ __launch_bounds__(256) void k_state_io(KStateSide st, KStateSide t, int n, KStateShape sh, unsigned long long* __restrict__ errors) {
  __shared__ double tile[KS_TILE * KS_KMAX];
  __shared__ int s_env[KS_TILE];
  const int row0 = blockIdx.x * KS_TILE, tid = threadIdx.x, fld = blockIdx.y;
  const int rows = n - row0 < KS_TILE ? n - row0 : KS_TILE;
  if (tid < KS_TILE) {
    int e = -1;
    if (tid < rows) {
      const size_t row = (size_t)row0 + tid;
      e = t.index ? t.index[row] : (int)row;
      if (e < 0 || e >= st.range) {
        e = -1;
        if (fld == 0) atomicAdd(errors, 1ull);
      } else if (fld == 0) {
        // the counters have one component: no transpose
        if (IMPORT) {
          if (t.step) {
            const int32_t s = t.step[row];
            st.step[e] = s;
            if (st.sim_time) st.sim_time[e] = s * st.control_dt;
          }
          if (t.episode) st.episode[e] = t.episode[row];
        } else {
          if (t.step) t.step[row] = st.step[e];
          if (t.episode) t.episode[row] = st.episode[e];
        }
      }
    }
    s_env[tid] = e;
  }
  double* const tf = t.f[fld];
  if (!tf) return;                      // a NULL tensor: that field is skipped (uniform over the workgroup)
  double* const sf = st.f[fld];
  const int K = sh.K[fld], KP = K | 1;
  const size_t N = (size_t)st.stride;
  double* const trow = tf + (size_t)row0 * K;
  const int wave = tid >> 6, lane = tid & 63;
  __syncthreads();
  if (IMPORT) {
    for (int i = tid; i < rows * K; i += 256) {
      const int j = i / K, k = i - j * K;
      tile[j * KP + k] = trow[i];
    }
    __syncthreads();
    const int e = s_env[lane];
    if (e >= 0)
      for (int k = wave; k < K; k += 4) sf[(size_t)k * N + e] = tile[lane * KP + k];
  } else {
    const int e = s_env[lane];
    if (e >= 0)
      for (int k = wave; k < K; k += 4) tile[lane * KP + k] = sf[(size_t)k * N + e];
    __syncthreads();
    for (int i = tid; i < rows * K; i += 256) {
      const int j = i / K, k = i - j * K;
      if (s_env[j] >= 0) trow[i] = tile[j * KP + k];
    }
  }
}

__global__ __launch_bounds__(256) void k_state_gather(KStateSide d, KStateSide s, int n, KStateShape sh, KEnvParamDefaults model,
                                                      unsigned long long* __restrict__ errors) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const bool first = blockIdx.y == 0;
  // the entry's two envs; a staged side is addressed by the row itself, its index is only checked
  const int di = d.index ? d.index[j] : j, si = s.index ? s.index[j] : j;
  if (di < 0 || di >= d.range || si < 0 || si >= s.range) {
    if (first && errors) atomicAdd(errors, 1ull);
    return;
  }
  const size_t de = d.staged ? (size_t)j : (size_t)di, se = s.staged ? (size_t)j : (size_t)si;
  const size_t Nd = (size_t)d.stride, Ns = (size_t)s.stride;
  if (first) {
    const int32_t step = s.step[se];
    d.step[de] = step;
    if (d.sim_time) d.sim_time[de] = step * d.control_dt;
    if (d.episode) d.episode[de] = s.episode[se];
  }
  const int c0 = blockIdx.y * KS_CPT;
  double v[KS_CPT];
  double* dst[KS_CPT];
#pragma unroll
  for (int u = 0; u < KS_CPT; u++) {
    int k = c0 + u, fld = 0;
    while (fld < KS_NFIELD && k >= sh.K[fld]) { k -= sh.K[fld]; fld++; }
    dst[u] = nullptr; v[u] = 0;
    if (fld < KS_NFIELD) {
      dst[u] = d.f[fld] + (size_t)k * Nd + de;
      // (the last field is the per-env parameters: a source without them stands for the compiled model's values)
      v[u] = s.f[fld] ? s.f[fld][(size_t)k * Ns + se] : model.v[k];
    }
  }
#pragma unroll
  for (int u = 0; u < KS_CPT; u++)
    if (dst[u]) *dst[u] = v[u];
}

static KStateShape io_shape(const KModelDesc& hd) {
  const int nl = hd.nlink;
  return KStateShape{{nl + 7, nl + 6, nl, nl + 6, 0}};
}

void kmanip_launch_state_io(const KModelDesc& hd, const KStateSide& state, const KStateSide& tensors, int n, bool import, unsigned long long* errors,
                            hipStream_t stream) {
  if (n <= 0) return;
  const dim3 grid((n + KS_TILE - 1) / KS_TILE, 4), block(256);
  if (import) hipLaunchKernelGGL(k_state_io<true>, grid, block, 0, stream, state, tensors, n, io_shape(hd), errors);
  else hipLaunchKernelGGL(k_state_io<false>, grid, block, 0, stream, state, tensors, n, io_shape(hd), errors);
}

void kmanip_launch_state_gather(const KModelDesc& hd, const KStateSide& dst, const KStateSide& src, int n, bool env_params,
                                const KEnvParamDefaults& model, unsigned long long* errors, hipStream_t stream) {
  if (n <= 0) return;
  KStateShape sh = io_shape(hd);
  sh.K[KS_NFIELD - 1] = env_params ? KM_EP_N : 0;
  int total = 0;
  for (int f = 0; f < KS_NFIELD; f++) total += sh.K[f];
  const dim3 grid((n + 255) / 256, (total + KS_CPT - 1) / KS_CPT), block(256);
  hipLaunchKernelGGL(k_state_gather, grid, block, 0, stream, dst, src, n, sh, model, errors);
}
