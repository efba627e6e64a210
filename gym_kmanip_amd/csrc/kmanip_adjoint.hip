// kmanip_adjoint.hip -- kmanip_adjoint (gfx950, wave64): the adjoint sweep of a rollout, gym_kmanip_amd/derivatives.py adjoint_pass, in
// ONE launch (include/kmanip.h KAdjointIn / KAdjointDev).  No simulator state is touched: the handle gives the
// size class only.
//
// One workgroup of AJ_NT = 256 threads owns one problem and up to MC = NX of its m cotangent vectors (m > MC: a workgroup per chunk of
// MC vectors, each reading the problem's Jacobians once) and runs the loop t = T-1 .. 0 inside the kernel.  In LDS, every matrix with
// an ODD row stride (LX = NX | 1, LU = NU | 1 doubles), TWO buffers of each:
//   blk [NX + NU][LX]   the step's A' then B', the caller's block as it lies in memory (rows contiguous)
//   gbk [NX][LU]        the step's gains transposed, KFeedbackIn::gain_t's block (closed loop only)
// and lamb [2][MC][NX], the vectors lam[t+1] and lam[t] in turn, and mus [MC][NU].  (52, 20): 2 * 3 816 + 2 * 1 092 + 5 408 + 1 040 =
// 16 264 doubles (130 112 B); (32, 10): 2 * 1 386 + 2 * 352 + 2 048 + 320 = 5 844 (46 752 B).
// WHAT BOUNDS IT: the kernel reads every Jacobian block ONCE from HBM -- (NX + NU) NX doubles a step, 30 KB for (52, 20), against
// 2 (NX + NU) NX m flops -- and at m = 1 nothing else is of any size: it is bound by that read and by the chain of T dependent steps.
// So the loads are whole contiguous rows (thread i takes double i, i + 256, .. of the block: a wave reads 512 consecutive bytes), and
// the block of step t - 1 is fetched into registers BEFORE the products of step t and put into the other LDS buffer after them: the
// HBM latency of a step hides behind the arithmetic of the step before, and one barrier a step suffices.
// Banks: an 8-byte read is served 32 lanes at a time on 64 four-byte banks.  A thread owns two rows j0, j0 + H of one vector; the lanes
// of a wave walk j0 (stride LX or LU doubles: odd, so 32 consecutive rows start on 32 different even banks) and read the vector's
// entry at one address, a broadcast.
// THE ORDER OF EVERY SUM (include/kmanip.h): one fma chain from 0 over k ascending, for lam continued over the actuators i ascending,
// then one add of the direct term.  No row reads another row's vector: a row's result does not depend on n, m or its place.
#include <hip/hip_runtime.h>

#include "kmanip_device.hpp"

#define AJ_NT 256

// CNT contiguous doubles of global memory into registers, thread i taking i, i + AJ_NT, ..; then into an LDS matrix of COLS columns
// and row stride LD
template <int CNT>
__device__ __forceinline__ void aj_fetch(double (&r)[(CNT + AJ_NT - 1) / AJ_NT], const double* __restrict__ src, int tid) {
#pragma unroll
  for (int s = 0; s < (CNT + AJ_NT - 1) / AJ_NT; s++) {
    const int i = tid + s * AJ_NT;
    r[s] = i < CNT ? src[i] : 0.0;
  }
}
template <int CNT, int COLS, int LD>
__device__ __forceinline__ void aj_put(double* dst, const double (&r)[(CNT + AJ_NT - 1) / AJ_NT], int tid) {
#pragma unroll
  for (int s = 0; s < (CNT + AJ_NT - 1) / AJ_NT; s++) {
    const int i = tid + s * AJ_NT;
    if (i < CNT) dst[(i / COLS) * LD + i % COLS] = r[s];
  }
}

template <int NX, int NU>
__global__ __launch_bounds__(AJ_NT) void k_adjoint(KAdjointIn in, int n, int T, int m, int chunks, KAdjointDev out) {
  constexpr int LX = NX | 1, LU = NU | 1, R = NX + NU, MC = NX;
  constexpr int BLK = R * LX, GBK = NX * LU;
  constexpr int NA = (NX * NX + AJ_NT - 1) / AJ_NT, NB = (NU * NX + AJ_NT - 1) / AJ_NT, NG = (NX * NU + AJ_NT - 1) / AJ_NT;
  static_assert(NX % 2 == 0 && NU % 2 == 0, "two rows a thread");
  __shared__ double lds[2 * BLK + 2 * GBK + 2 * MC * NX + MC * NU];
  double* const blk = lds;
  double* const gbk = blk + 2 * BLK;
  double* const lamb = gbk + 2 * GBK;
  double* const mus = lamb + 2 * MC * NX;
  const int tid = threadIdx.x, e = blockIdx.x / chunks, v0 = (blockIdx.x - e * chunks) * MC;
  if (e >= n || v0 >= m) return;
  const int mv = m - v0 < MC ? m - v0 : MC;          // this workgroup's vectors: rows row0 .. row0 + mv - 1
  const size_t eT = (size_t)e * T, row0 = (size_t)e * m + v0;
  const bool fb = in.gain_t != nullptr;
  const double* const gx = in.gx + row0 * (T + 1) * NX;
  const double* const gu = in.gu ? in.gu + row0 * T * NU : nullptr;
  double* const lo = out.lam ? out.lam + row0 * (T + 1) * NX : nullptr;
  double* const mo = out.mu ? out.mu + row0 * T * NU : nullptr;
  double ra[NA], rb[NB], rg[NG];
  // ---- the last step's block, and lam[T] = gx[T]
  aj_fetch<NX * NX>(ra, in.a_t + (eT + T - 1) * in.a_stride, tid);
  aj_fetch<NU * NX>(rb, in.b_t + (eT + T - 1) * in.b_stride, tid);
  if (fb) aj_fetch<NX * NU>(rg, in.gain_t + (eT + T - 1) * (NX * NU), tid);
  for (int i = tid; i < mv * NX; i += AJ_NT) {
    const int v = i / NX, j = i - v * NX;
    const size_t at = ((size_t)v * (T + 1) + T) * NX + j;
    const double g = gx[at];
    lamb[i] = g;
    if (lo) lo[at] = g;
  }
  aj_put<NX * NX, NX, LX>(blk, ra, tid);
  aj_put<NU * NX, NX, LX>(blk + NX * LX, rb, tid);
  if (fb) aj_put<NX * NU, NU, LU>(gbk, rg, tid);
  __syncthreads();
  int c = 0;
  for (int t = T - 1; t >= 0; t--) {
    const double* const ab = blk + c * BLK;          // A' rows 0 .. NX-1, B' rows NX .. R-1
    const double* const gb = gbk + c * GBK;
    const double* const ln = lamb + c * (MC * NX);   // lam[t+1]
    double* const lc = lamb + (1 - c) * (MC * NX);   // lam[t]
    // ---- the block of step t - 1 on its way while this step's products run
    if (t > 0) {
      aj_fetch<NX * NX>(ra, in.a_t + (eT + t - 1) * in.a_stride, tid);
      aj_fetch<NU * NX>(rb, in.b_t + (eT + t - 1) * in.b_stride, tid);
      if (fb) aj_fetch<NX * NU>(rg, in.gain_t + (eT + t - 1) * (NX * NU), tid);
    }
    if (!fb) {
      // ---- open loop: the R rows of [A' ; B'] times lam[t+1], two rows a thread
      constexpr int H = R / 2;
      for (int idx = tid; idx < H * mv; idx += AJ_NT) {
        const int v = idx / H, j0 = idx - v * H, j1 = j0 + H;
        const double *x0 = ab + j0 * LX, *x1 = ab + j1 * LX, *y = ln + v * NX;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
        for (int k = 0; k < NX; k++) {
          const double b = y[k];
          s0 = fma(x0[k], b, s0);
          s1 = fma(x1[k], b, s1);
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int j = h ? j1 : j0;
          const double s = h ? s1 : s0;
          if (j < NX) {
            const size_t at = ((size_t)v * (T + 1) + t) * NX + j;
            const double val = s + gx[at];
            lc[v * NX + j] = val;
            if (lo) lo[at] = val;
          } else {
            const size_t at = ((size_t)v * T + t) * NU + (j - NX);
            const double val = s + (gu ? gu[at] : 0.0);
            if (mo) mo[at] = val;
          }
        }
      }
    } else {
      // ---- closed loop: mu[t] = gu[t] + B' lam[t+1] first, lam[t] reads it
      constexpr int HU = NU / 2, HX = NX / 2;
      for (int idx = tid; idx < HU * mv; idx += AJ_NT) {
        const int v = idx / HU, i0 = idx - v * HU, i1 = i0 + HU;
        const double *x0 = ab + (NX + i0) * LX, *x1 = ab + (NX + i1) * LX, *y = ln + v * NX;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
        for (int k = 0; k < NX; k++) {
          const double b = y[k];
          s0 = fma(x0[k], b, s0);
          s1 = fma(x1[k], b, s1);
        }
        const size_t at0 = ((size_t)v * T + t) * NU + i0, at1 = ((size_t)v * T + t) * NU + i1;
        const double u0 = s0 + (gu ? gu[at0] : 0.0), u1 = s1 + (gu ? gu[at1] : 0.0);
        mus[v * NU + i0] = u0;
        mus[v * NU + i1] = u1;
        if (mo) { mo[at0] = u0; mo[at1] = u1; }
      }
      __syncthreads();
      for (int idx = tid; idx < HX * mv; idx += AJ_NT) {
        const int v = idx / HX, j0 = idx - v * HX, j1 = j0 + HX;
        const double *x0 = ab + j0 * LX, *x1 = ab + j1 * LX, *y = ln + v * NX;
        const double *g0 = gb + j0 * LU, *g1 = gb + j1 * LU, *u = mus + v * NU;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
        for (int k = 0; k < NX; k++) {
          const double b = y[k];
          s0 = fma(x0[k], b, s0);
          s1 = fma(x1[k], b, s1);
        }
#pragma unroll 2
        for (int i = 0; i < NU; i++) {
          const double b = u[i];
          s0 = fma(g0[i], b, s0);
          s1 = fma(g1[i], b, s1);
        }
        const size_t at0 = ((size_t)v * (T + 1) + t) * NX + j0, at1 = ((size_t)v * (T + 1) + t) * NX + j1;
        const double l0 = s0 + gx[at0], l1 = s1 + gx[at1];
        lc[v * NX + j0] = l0;
        lc[v * NX + j1] = l1;
        if (lo) { lo[at0] = l0; lo[at1] = l1; }
      }
    }
    // ---- the fetched block into the other buffer (last read one step ago, before that step's barrier)
    if (t > 0) {
      double* const nb = blk + (1 - c) * BLK;
      aj_put<NX * NX, NX, LX>(nb, ra, tid);
      aj_put<NU * NX, NX, LX>(nb + NX * LX, rb, tid);
      if (fb) aj_put<NX * NU, NU, LU>(gbk + (1 - c) * GBK, rg, tid);
    }
    __syncthreads();
    c ^= 1;
  }
}

// n > 0 problems of T > 0 steps, m > 0 vectors each; the strides resolved (never 0); the class is the handle's
void kmanip_launch_adjoint(const KModelDesc& hd, const KAdjointIn& in, int n, int T, int m, const KAdjointDev& out, hipStream_t stream) {
  if (hd.nlink <= 10) {
    const int chunks = (m + 31) / 32;
    hipLaunchKernelGGL((k_adjoint<32, 10>), dim3(n * chunks), dim3(AJ_NT), 0, stream, in, n, T, m, chunks, out);
  } else {
    const int chunks = (m + 51) / 52;
    hipLaunchKernelGGL((k_adjoint<52, 20>), dim3(n * chunks), dim3(AJ_NT), 0, stream, in, n, T, m, chunks, out);
  }
}
