// kmanip_lqr.hip -- kmanip_lqr_backward (gfx950, wave64): the backward pass of iLQR, gym_kmanip_amd/ilqr.py backward_pass, in ONE launch
// (include/kmanip.h KLqrIn / KLqrDev).  No simulator state is touched: the handle gives the size class only.
//
// One workgroup of LQ_NT = 256 threads (four waves, one per SIMD) owns one problem and runs the loop t = T-1 .. 0 inside the kernel
// with everything but the step's inputs in LDS.  With nx = NX, nu = NU, every matrix [rows][LX or LU] with an ODD row stride
// (LX = NX | 1, LU = NU | 1 doubles):
//   vxx [NX][LX]   Vxx of step t + 1; Qxx is accumulated over it once W and Y are formed, then the new Vxx
//   at  [NX][LX]   A transposed, the caller's block as it lies in memory        bt [NU][LX]   B transposed, likewise
//   w   [NX][LX]   W = Vxx A; after Qxx and Qux are formed its first NU rows hold H = Quu K + Qux
//   yk  [NX][LU]   Y = Vxx B; after Quu is formed the same doubles hold K [NU][LX]
//   qux [NU][LX], quu [NU][LU], lf [NU][LU] the Cholesky factor, and the vectors vx, qx, qu, kv, qk = Quu k, tmp = Quu k + Qu.
// 12 504 doubles (100 032 B) for (52, 20), 4 504 (36 032 B) for (32, 10), and the 4-byte flag of the factorisation.
// Banks: an 8-byte read is served 32 lanes at a time on 64 four-byte banks.  Every product below is a 2 x 2 register tile whose two
// columns lie N / 2 apart, so the lanes of a wave walk j (unit stride: consecutive doubles) or, where the operand is read
// transposed, i (stride LX or LU doubles: odd, so 32 consecutive rows start on 32 different even banks); the other operand is one
// address per row of tiles, a broadcast.  Each sum runs over k ascending as ONE fma chain from 0, the cost's term added last: the
// result of a problem does not depend on n, on its index or on the problems beside it.
// The factorisation is one wave's: lane i keeps row i of the lower triangle in registers, column by column, the pivot row handed
// round with __shfl; the two triangular solves run one right-hand side (Qu, then the NX columns of Qux) per thread.
// FAILURE: a pivot that is not > 0 or not finite, or an entry of the step's k or K that is not finite (a NaN in A reaches Qux, not
// Quu), stops the problem: status 1, fail_step t, and every k / gain_t / dv entry of the problem zero -- each thread zeroes exactly the addresses it wrote at the earlier steps, so the stores are ordered by the thread.
#include "kmanip_lqr.hpp"          // (LQ_NT, lq_mm, lq_load: shared with kmanip_lqr_box.hip)

template <int NX, int NU>
__global__ __launch_bounds__(LQ_NT) void k_lqr_backward(KLqrIn in, int n, int T, KLqrDev out) {
  constexpr int LX = NX | 1, LU = NU | 1;
  constexpr int YK = NX * LU > NU * LX ? NX * LU : NU * LX;
  static_assert(NU <= 64 && NX + 1 + NU <= LQ_NT, "one lane per row of Quu; one thread per right-hand side");
  __shared__ double lds[3 * NX * LX + 2 * NU * LX + YK + 2 * NU * LU + 2 * NX + 4 * NU];
  __shared__ int s_ok;
  double* const vxx = lds;
  double* const at = vxx + NX * LX;
  double* const w = at + NX * LX;
  double* const bt = w + NX * LX;
  double* const qux = bt + NU * LX;
  double* const yk = qux + NU * LX;
  double* const quu = yk + YK;
  double* const lf = quu + NU * LU;
  double* const vx = lf + NU * LU;
  double* const qx = vx + NX;
  double* const qu = qx + NX;
  double* const kv = qu + NU;
  double* const qk = kv + NU;
  double* const tmp = qk + NU;
  const int tid = threadIdx.x, e = blockIdx.x;
  if (e >= n) return;
  const size_t eT = (size_t)e * T;
  const double* const lx = in.lx + ((size_t)e * (T + 1)) * NX;
  const double* const lu = in.lu + eT * NU;
  const double* const lxx = in.lxx + (in.lxx_per_env ? (size_t)e * (T + 1) : 0) * (NX * NX);
  const double* const luu = in.luu + (in.luu_per_env ? eT : 0) * (NU * NU);
  const double reg = in.reg ? in.reg[e] : 0.0;
  double* const ko = out.k ? out.k + eT * NU : nullptr;
  double* const go = out.gain_t ? out.gain_t + eT * (NX * NU) : nullptr;
  double dv0 = 0.0, dv1 = 0.0;          // thread 0's
  // Vx = lx[T], Vxx = lxx[T]
  lq_load<NX, NX>(vxx, LX, lxx + (size_t)T * (NX * NX), tid);
  if (tid < NX) vx[tid] = lx[(size_t)T * NX + tid];
  for (int t = T - 1; t >= 0; t--) {
    // ---- the step's A' and B'
    lq_load<NX, NX>(at, LX, in.a_t + (eT + t) * in.a_stride, tid);
    lq_load<NU, NX>(bt, LX, in.b_t + (eT + t) * in.b_stride, tid);
    __syncthreads();
    // ---- W = Vxx A, Y = Vxx B; Qx = lx + A' Vx, Qu = lu + B' Vx (the last NX + NU threads: the first are the ones with a tile more)
    lq_mm<NX, NX, NX>(w, LX, nullptr, 0, vxx, LX, 1, at, 1, LX, tid);
    lq_mm<NX, NU, NX>(yk, LU, nullptr, 0, vxx, LX, 1, bt, 1, LX, tid);
    {
      const int r = LQ_NT - 1 - tid;
      if (r < NX + NU) {
        const double* row = r < NX ? at + r * LX : bt + (r - NX) * LX;
        double s = 0.0;
        for (int k = 0; k < NX; k++) s = fma(row[k], vx[k], s);
        if (r < NX) qx[r] = s + lx[(size_t)t * NX + r];
        else qu[r - NX] = s + lu[(size_t)t * NU + (r - NX)];
      }
    }
    __syncthreads();
    // ---- Qxx = lxx + A' W (over the dead Vxx), Qux = B' W, Quu = luu + B' Y
    lq_mm<NX, NX, NX>(vxx, LX, lxx + (size_t)t * (NX * NX), NX, at, LX, 1, w, LX, 1, tid);
    lq_mm<NU, NX, NX>(qux, LX, nullptr, 0, bt, LX, 1, w, LX, 1, tid);
    lq_mm<NU, NU, NX>(quu, LU, luu + (size_t)t * (NU * NU), NU, bt, LX, 1, yk, LU, 1, tid);
    __syncthreads();
    // ---- Quu + reg I = L L', the lower triangle, by the first wave: lane i holds row i
    if (tid < 64) {
      const int ir = tid < NU ? tid : 0;            // (the lanes beyond NU repeat row 0 and store nothing)
      double L[NU];
      bool ok = true;
#pragma unroll
      for (int j = 0; j < NU; j++) {
        __builtin_amdgcn_sched_barrier(0);          // (column by column: nothing of a later column is worth a register now)
        double s = j <= ir ? quu[ir * LU + j] : 0.0;
        if (j == ir) s += reg;
#pragma unroll
        for (int m = 0; m < j; m++) s = fma(-L[m], __shfl(L[m], j), s);
        const double piv = __shfl(s, j);
        ok = ok && piv > 0.0 && piv - piv == 0.0;
        const double d = sqrt(piv);
        L[j] = ir > j ? s / d : ir == j ? d : 0.0;
      }
      if (tid < NU) {
#pragma unroll
        for (int j = 0; j < NU; j++) lf[tid * LU + j] = L[j];
      }
      if (tid == 0) s_ok = ok;
    }
    __syncthreads();
    // ---- (Quu + reg I) [k | K] = -[Qu | Qux]: one right-hand side per thread, forward then back; K over the dead Y.  (After a failed
    // factorisation this runs on an unfinished factor: nothing of it is kept.)  A solution that is not finite fails the step as well.
    if (tid < NX + 1) {
      double y[NU];
#pragma unroll
      for (int i = 0; i < NU; i++) {
        __builtin_amdgcn_sched_barrier(0);          // (row by row: the factor's entries are read when they are used)
        double s = tid == 0 ? qu[i] : qux[i * LX + tid - 1];
#pragma unroll
        for (int m = 0; m < i; m++) s = fma(-lf[i * LU + m], y[m], s);
        y[i] = s / lf[i * LU + i];
      }
#pragma unroll
      for (int i = NU - 1; i >= 0; i--) {
        __builtin_amdgcn_sched_barrier(0);
        double s = y[i];
#pragma unroll
        for (int m = i + 1; m < NU; m++) s = fma(-lf[m * LU + i], y[m], s);
        y[i] = s / lf[i * LU + i];
      }
      double z = 0.0;
#pragma unroll
      for (int i = 0; i < NU; i++) {
        z += y[i] - y[i];
        if (tid == 0) kv[i] = -y[i];
        else yk[i * LX + tid - 1] = -y[i];
      }
      if (!(z == 0.0)) s_ok = 0;
    }
    __syncthreads();
    if (!s_ok) {
      // the problem stops: zeros at every address this thread wrote, and at the steps it never reached
      for (int s = 0; s < T; s++) {
        if (ko && tid < NU) ko[(size_t)s * NU + tid] = 0.0;
        if (go)
          for (int i = tid; i < NX * NU; i += LQ_NT) go[(size_t)s * (NX * NU) + i] = 0.0;
      }
      if (tid == 0) {
        if (out.dv) { out.dv[2 * (size_t)e] = 0.0; out.dv[2 * (size_t)e + 1] = 0.0; }
        if (out.status) out.status[e] = 1;
        if (out.fail_step) out.fail_step[e] = t;
      }
      return;
    }
    // ---- H = Quu K + Qux (over the dead W), qk = Quu k, tmp = qk + Qu (Quu WITHOUT reg); the step's k and K' go out
    lq_mm<NU, NX, NU>(w, LX, qux, LX, quu, LU, 1, yk, LX, 1, tid);
    {
      const int r = LQ_NT - 1 - tid;
      if (r < NU) {
        double s = 0.0;
        for (int m = 0; m < NU; m++) s = fma(quu[r * LU + m], kv[m], s);
        qk[r] = s;
        tmp[r] = s + qu[r];
      }
    }
    if (ko && tid < NU) ko[(size_t)t * NU + tid] = kv[tid];
    if (go)
      for (int i = tid; i < NX * NU; i += LQ_NT) {
        const int j = i / NU, a = i - j * NU;
        go[(size_t)t * (NX * NU) + i] = yk[a * LX + j];
      }
    __syncthreads();
    // ---- Vxx = Qxx + K' H + Qux' K; Vx = Qx + K' tmp + Qux' k; dV
    lq_mm<NX, NX, NU>(vxx, LX, vxx, LX, yk, 1, LX, w, LX, 1, tid);
    lq_mm<NX, NX, NU>(vxx, LX, vxx, LX, qux, 1, LX, yk, LX, 1, tid);
    {
      const int r = LQ_NT - 1 - tid;
      if (r < NX) {
        double s = 0.0, u = 0.0;
        for (int m = 0; m < NU; m++) s = fma(yk[m * LX + r], tmp[m], s);
        for (int m = 0; m < NU; m++) u = fma(qux[m * LX + r], kv[m], u);
        vx[r] = qx[r] + (s + u);
      }
    }
    if (tid == 0) {
      double s = 0.0, u = 0.0;
      for (int m = 0; m < NU; m++) { s = fma(kv[m], qu[m], s); u = fma(kv[m], qk[m], u); }
      dv0 += s;
      dv1 += 0.5 * u;
    }
    __syncthreads();
    // ---- Vxx = 0.5 (Vxx + Vxx'): one thread per pair
    for (int p = tid; p < NX * NX; p += LQ_NT) {
      const int i = p / NX, j = p - i * NX;
      if (i < j) {
        const double s = 0.5 * (vxx[i * LX + j] + vxx[j * LX + i]);
        vxx[i * LX + j] = s;
        vxx[j * LX + i] = s;
      }
    }
    // (the next step's first barrier stands between these stores and the reads of Vxx; at and bt are dead since the one above)
  }
  if (tid == 0) {
    if (out.dv) { out.dv[2 * (size_t)e] = dv0; out.dv[2 * (size_t)e + 1] = dv1; }
    if (out.status) out.status[e] = 0;
    if (out.fail_step) out.fail_step[e] = -1;
  }
}

// n > 0 problems of T > 0 steps; the strides resolved (never 0); the class is the handle's
void kmanip_launch_lqr_backward(const KModelDesc& hd, const KLqrIn& in, int n, int T, const KLqrDev& out, hipStream_t stream) {
  if (hd.nlink <= 10) hipLaunchKernelGGL((k_lqr_backward<32, 10>), dim3(n), dim3(LQ_NT), 0, stream, in, n, T, out);
  else hipLaunchKernelGGL((k_lqr_backward<52, 20>), dim3(n), dim3(LQ_NT), 0, stream, in, n, T, out);
}
