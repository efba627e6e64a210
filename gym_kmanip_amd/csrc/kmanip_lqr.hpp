// kmanip_lqr.hpp -- the tile product and the staging load of the two backward-pass units, kmanip_lqr.hip (k_lqr_backward) and
// kmanip_lqr_box.hip (k_lqr_backward_box): written once, included by those two only (DESIGN.md sections 37 and 39).
#pragma once
#include <hip/hip_runtime.h>

#include "kmanip_device.hpp"

#define LQ_NT 256

// C(i, j) = init(i, j) + sum_k X(i, k) Y(k, j) for i < M, j < N, k < KD ascending; element (i, k) of X at X[i * xsi + k * xsk], (k, j) of
// Y at Y[k * ysk + j * ysj]; init may be C itself (a thread reads only the entries it writes) or NULL
template <int M, int N, int KD>
__device__ __forceinline__ void lq_mm(double* C, int ldc, const double* init, int ldi, const double* X, int xsi, int xsk, const double* Y,
                                      int ysk, int ysj, int tid) {
  static_assert(M % 2 == 0 && N % 2 == 0, "2 x 2 tiles");
  constexpr int HM = M / 2, HN = N / 2;
  for (int t = tid; t < HM * HN; t += LQ_NT) {
    const int i0 = t / HN, j0 = t - i0 * HN, i1 = i0 + HM, j1 = j0 + HN;
    const double *x0 = X + i0 * xsi, *x1 = X + i1 * xsi, *y0 = Y + j0 * ysj, *y1 = Y + j1 * ysj;
    double c00 = 0, c01 = 0, c10 = 0, c11 = 0;
#pragma unroll 4
    for (int k = 0; k < KD; k++) {
      const double a0 = x0[k * xsk], a1 = x1[k * xsk], b0 = y0[k * ysk], b1 = y1[k * ysk];
      c00 = fma(a0, b0, c00); c01 = fma(a0, b1, c01);
      c10 = fma(a1, b0, c10); c11 = fma(a1, b1, c11);
    }
    if (init) {
      c00 += init[i0 * ldi + j0]; c01 += init[i0 * ldi + j1];
      c10 += init[i1 * ldi + j0]; c11 += init[i1 * ldi + j1];
    }
    C[i0 * ldc + j0] = c00; C[i0 * ldc + j1] = c01;
    C[i1 * ldc + j0] = c10; C[i1 * ldc + j1] = c11;
  }
}

// rows x cols doubles, dense in global memory, into an LDS matrix of row stride ld
template <int ROWS, int COLS>
__device__ __forceinline__ void lq_load(double* dst, int ld, const double* __restrict__ src, int tid) {
  for (int i = tid; i < ROWS * COLS; i += LQ_NT) {
    const int r = i / COLS, c = i - r * COLS;
    dst[r * ld + c] = src[i];
  }
}
