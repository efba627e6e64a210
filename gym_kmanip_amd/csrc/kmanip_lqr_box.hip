// kmanip_lqr_box.hip -- kmanip_lqr_backward_box (gfx950, wave64): the backward pass of control-limited DDP (Tassa, Mansard, Todorov,
// ICRA 2014), gym_kmanip_amd/ilqr.py backward_pass_box, in ONE launch (include/kmanip.h KLqrBoxIn / KLqrBoxDev).
//
// The workgroup, the LDS plan, the products and the order of every sum are k_lqr_backward's (kmanip_lqr.hip, whose header describes
// them; lq_mm and lq_load are kmanip_lqr.hpp's).  What differs is the solve of a step: in place of k = -H^-1 Qu, H = Quu + reg I, the
// FIRST WAVE solves   min_d 0.5 d'H d + Qu'd,  bl <= d <= bh,  bl = lo - u_t, bh = hi - u_t   by projected Newton steps, lane i owning
// actuator i (d_i, its bounds and its gradient entry live in the lane's registers; H and Qu are read from LDS):
//   d = clip(0, bl, bh)
//   repeat   g = Qu + H d;   c = { d_i == bl_i and g_i > 0 } u { d_i == bh_i and g_i < 0 }
//            stop (converged) if the last step was a full one that the clip left alone and c is the set it was factorised for
//            H_ff = L L' with row and column i of H replaced by the unit row for i in c (only when c changed); a bad pivot FAILS
//            stop (converged) if every actuator is in c
//            L L' s = -g on the free rows, s_i = 0 in c;   sg = s . g;   not finite FAILS, sg >= 0 stops (converged: no descent left)
//            a = 1, 0.6, 0.36 .. (at most LQ_LS trials) until  v(clip(d + a s)) - v(d) <= 0.1 a sg;   d = clip(d + a s)
// at most LQ_QP iterations: the cap, or a line search that runs out of trials, gives status 3.  Nothing here is a tolerance: the
// rule compares sets and steps, never a gradient norm, so a problem scaled by any power of two takes the same decisions.
// The unit rows keep the factorisation and the solves at their fixed NU shape: a clamped row factorises to the unit row, its
// right-hand side is zero, its solution an exact zero.  The lanes exchange d and s by __shfl; the back substitution reads the
// factor's column from LDS (lf, which the K solves need anyway).  The wave publishes status, mask and iteration count through LDS;
// every __syncthreads() stands in workgroup-uniform control flow.
// FAILURE as in k_lqr_backward (zeros everywhere, fail_step t; clamped and qp_iters zeroed with them): status 1 for a pivot of a
// free block that is not > 0 or not finite, a k or K entry that is not finite, or a row of the step's box with bl_i <= bh_i false (lo > hi, a
// NaN bound, a non-finite u: at the first step solved for the first two); status 3 for the cap.
#include "kmanip_lqr.hpp"

#define LQ_QP 100          // projected-Newton iterations per step (the paper's cap)
#define LQ_LS 100          // trials of one line search: 0.6^100 < 1e-22, the paper's smallest step

// (H x)_i for the lane's row hr of H = Quu + reg I, x_j taken from lane j.  The row is read again at every call, through an offset
// the optimiser cannot see through: hoisted out of the QP's loops the NU entries would live in registers across them.
template <int NU>
__device__ __forceinline__ double lq_hx(const double* hr, int ir, double reg, double x) {
  int o = 0;
  asm volatile("" : "+v"(o));
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < NU; j++) {
    double h = hr[o + j];
    if (j == ir) h += reg;
    s = fma(h, __shfl(x, j), s);
  }
  return s;
}

// the sum of x over the 64 lanes, the same in every lane
__device__ __forceinline__ double lq_wsum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

__device__ __forceinline__ double lq_clip(double x, double lo, double hi) { return x < lo ? lo : x > hi ? hi : x; }

template <int NX, int NU>
__global__ __launch_bounds__(LQ_NT) void k_lqr_backward_box(KLqrBoxIn bin, int n, int T, KLqrBoxDev bout) {
  constexpr int LX = NX | 1, LU = NU | 1;
  constexpr int YK = NX * LU > NU * LX ? NX * LU : NU * LX;
  static_assert(NU <= 32 && NX + 1 + NU <= LQ_NT, "one lane and one mask bit per actuator; one thread per right-hand side");
  __shared__ double lds[3 * NX * LX + 2 * NU * LX + YK + 2 * NU * LU + 2 * NX + 4 * NU];
  __shared__ int s_st, s_it;
  __shared__ unsigned s_mask;
  const KLqrIn& in = bin.lqr;
  const KLqrDev& out = bout.lqr;
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
  uint32_t* const co = bout.clamped ? bout.clamped + eT : nullptr;
  int32_t* const io = bout.qp_iters ? bout.qp_iters + eT : nullptr;
  // the first wave's lane = actuator (the lanes beyond NU repeat row 0, hold an empty box at 0 and store nothing)
  const bool act = tid < NU;
  const int ir = act ? tid : 0;
  const size_t brow = (bin.box_per_env ? (size_t)e : (size_t)0) * NU + ir;
  const double lo_i = tid < 64 ? bin.lo[brow] : 0.0, hi_i = tid < 64 ? bin.hi[brow] : 0.0;
  const double* const un = bin.u + eT * NU;
  double dv0 = 0.0, dv1 = 0.0;          // thread 0's
  // Vx = lx[T], Vxx = lxx[T]
  lq_load<NX, NX>(vxx, LX, lxx + (size_t)T * (NX * NX), tid);
  if (tid < NX) vx[tid] = lx[(size_t)T * NX + tid];
  for (int t = T - 1; t >= 0; t--) {
    // the thread's index opaque to the optimiser, once per step and again after the QP: the tile and row addresses derived from it are
    // then computed where they are used, not hoisted out of this loop and kept in registers across the QP (DESIGN.md section 3.2's
    // device; without it the (52, 20) kernel spills)
    int tp = tid; asm volatile("" : "+v"(tp));
    // ---- the step's A' and B'
    lq_load<NX, NX>(at, LX, in.a_t + (eT + t) * in.a_stride, tp);
    lq_load<NU, NX>(bt, LX, in.b_t + (eT + t) * in.b_stride, tp);
    __syncthreads();
    // ---- W = Vxx A, Y = Vxx B; Qx = lx + A' Vx, Qu = lu + B' Vx (the last NX + NU threads: the first are the ones with a tile more)
    lq_mm<NX, NX, NX>(w, LX, nullptr, 0, vxx, LX, 1, at, 1, LX, tp);
    lq_mm<NX, NU, NX>(yk, LU, nullptr, 0, vxx, LX, 1, bt, 1, LX, tp);
    {
      const int r = LQ_NT - 1 - tp;
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
    lq_mm<NX, NX, NX>(vxx, LX, lxx + (size_t)t * (NX * NX), NX, at, LX, 1, w, LX, 1, tp);
    lq_mm<NU, NX, NX>(qux, LX, nullptr, 0, bt, LX, 1, w, LX, 1, tp);
    lq_mm<NU, NU, NX>(quu, LU, luu + (size_t)t * (NU * NU), NU, bt, LX, 1, yk, LU, 1, tp);
    __syncthreads();
    // ---- the box QP of the step, by the first wave
    if (tid < 64) {
      const double* const hr = quu + ir * LU;
      const double ut = un[(size_t)t * NU + ir];
      const double bl = act ? lo_i - ut : 0.0, bh = act ? hi_i - ut : 0.0, qi = act ? qu[ir] : 0.0;
      const unsigned all = (1u << NU) - 1u;
      int st = __ballot(!(bl <= bh)) ? 1 : 0;          // (an empty or NaN box, a non-finite u)
      double d = lq_clip(0.0, bl, bh);
      double hd = lq_hx<NU>(hr, ir, reg, d);
      double v = lq_wsum(act ? d * fma(0.5, hd, qi) : 0.0);
      unsigned cm = 0u, cf = ~0u;                      // the clamped set; the one lf was factorised for (none yet)
      bool moved = true;                               // the last step was shortened or clipped (true before the first)
      int it = 0;
      double dg = 1.0;                                 // the lane's diagonal entry of the factor
      if (!st) {
#pragma nounroll
        for (;; it++) {
          const double g = qi + hd;
          cm = (unsigned)__ballot(act && ((d == bl && g > 0.0) || (d == bh && g < 0.0))) & all;
          if (!moved && cm == cf) break;
          if (it == LQ_QP) { st = 3; break; }
          if (cm != cf) {
            // H with the unit row and column at the clamped actuators = L L', the lower triangle: lane i holds row i
            const bool ci = (cm >> ir) & 1u;
            int o = 0;
            asm volatile("" : "+v"(o));              // (lq_hx's: the row is read here, not kept from an earlier pass)
            double L[NU];
            bool ok = true;
#pragma unroll
            for (int j = 0; j < NU; j++) {
              __builtin_amdgcn_sched_barrier(0);       // (column by column: nothing of a later column is worth a register now)
              double s = j <= ir ? hr[o + j] : 0.0;
              if (j == ir) s += reg;
              if (ci || ((cm >> j) & 1u)) s = j == ir ? 1.0 : 0.0;
#pragma unroll
              for (int m = 0; m < j; m++) s = fma(-L[m], __shfl(L[m], j), s);
              const double piv = __shfl(s, j);
              ok = ok && piv > 0.0 && piv - piv == 0.0;
              const double r = sqrt(piv);
              L[j] = ir > j ? s / r : ir == j ? r : 0.0;
              if (ir == j) dg = r;
            }
            if (act) {
#pragma unroll
              for (int j = 0; j < NU; j++) lf[tid * LU + j] = L[j];
            }
            KM_GSYNC();
            if (!ok) { st = 1; break; }
            cf = cm;
          }
          if (cm == all) break;
          // L L' s = -g on the free rows: forward with the lane's row of lf, back with its column; lane j's entry is final at turn j
          double b = (!act || ((cm >> ir) & 1u)) ? 0.0 : -g;
#pragma unroll
          for (int j = 0; j < NU; j++) {
            __builtin_amdgcn_sched_barrier(0);
            const double yj = __shfl(b / dg, j);
            if (ir > j) b = fma(-lf[ir * LU + j], yj, b);
            else if (ir == j) b = yj;
          }
#pragma unroll
          for (int j = NU - 1; j >= 0; j--) {
            __builtin_amdgcn_sched_barrier(0);
            const double xj = __shfl(b / dg, j);
            if (ir < j) b = fma(-lf[j * LU + ir], xj, b);
            else if (ir == j) b = xj;
          }
          const double s = act ? b : 0.0;
          // (lq_wsum's butterfly adds commute: sg, and v below, are the same bits in every lane, so the branches on them are the wave's)
          const double sg = lq_wsum(s * g);
          if (!(sg - sg == 0.0)) { st = 1; break; }
          if (!(sg < 0.0)) break;
          // the projected Armijo search
          double a = 1.0, xc = d, hc = hd, vc = v;
          bool clipped = false, found = false;
#pragma nounroll
          for (int ls = 0; ls < LQ_LS; ls++) {
            const double y = fma(a, s, d);
            xc = lq_clip(y, bl, bh);
            clipped = __ballot(act && xc != y) != 0ull;
            hc = lq_hx<NU>(hr, ir, reg, xc);
            vc = lq_wsum(act ? xc * fma(0.5, hc, qi) : 0.0);
            if ((vc - v) / (a * sg) >= 0.1) { found = true; break; }
            a *= 0.6;
          }
          if (!found) { st = 3; break; }
          moved = clipped || a != 1.0;
          d = xc; hd = hc; v = vc;
        }
      }
      if (!st && __ballot(act && !(d - d == 0.0))) st = 1;
      if (act) kv[tid] = d;
      if (tid == 0) { s_st = st; s_mask = cm; s_it = it; }
    }
    __syncthreads();
    int ts = tid; asm volatile("" : "+v"(ts));
    // ---- H_ff K_f = -Qux_f, the rows of K at the clamped actuators exact zeros: one right-hand side per thread, forward then back; K
    // over the dead Y.  (After a failed QP this runs on an unfinished factor: nothing of it is kept.)  A solution that is not finite
    // fails the step as well.
    const unsigned cmask = s_mask;
    if (ts >= 1 && ts < NX + 1) {
      const int fail0 = s_st;
      double y[NU];
#pragma unroll
      for (int i = 0; i < NU; i++) {
        __builtin_amdgcn_sched_barrier(0);          // (row by row: the factor's entries are read when they are used)
        double s = ((cmask >> i) & 1u) ? 0.0 : qux[i * LX + ts - 1];
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
        yk[i * LX + ts - 1] = ((cmask >> i) & 1u) ? 0.0 : -y[i];
      }
      if (!(z == 0.0) && !fail0) s_st = 1;
    }
    __syncthreads();
    if (s_st) {
      // the problem stops: zeros at every address this thread wrote, and at the steps it never reached
      for (int s = 0; s < T; s++) {
        if (ko && ts < NU) ko[(size_t)s * NU + ts] = 0.0;
        if (go)
          for (int i = ts; i < NX * NU; i += LQ_NT) go[(size_t)s * (NX * NU) + i] = 0.0;
        if (ts == 0) {
          if (co) co[s] = 0u;
          if (io) io[s] = 0;
        }
      }
      if (ts == 0) {
        if (out.dv) { out.dv[2 * (size_t)e] = 0.0; out.dv[2 * (size_t)e + 1] = 0.0; }
        if (out.status) out.status[e] = (uint8_t)s_st;
        if (out.fail_step) out.fail_step[e] = t;
      }
      return;
    }
    // ---- H = Quu K + Qux (over the dead W), qk = Quu k, tmp = qk + Qu (Quu WITHOUT reg); the step's k, K', mask and count go out
    lq_mm<NU, NX, NU>(w, LX, qux, LX, quu, LU, 1, yk, LX, 1, ts);
    {
      const int r = LQ_NT - 1 - ts;
      if (r < NU) {
        double s = 0.0;
        for (int m = 0; m < NU; m++) s = fma(quu[r * LU + m], kv[m], s);
        qk[r] = s;
        tmp[r] = s + qu[r];
      }
    }
    if (ko && ts < NU) ko[(size_t)t * NU + ts] = kv[ts];
    if (go)
      for (int i = ts; i < NX * NU; i += LQ_NT) {
        const int j = i / NU, a = i - j * NU;
        go[(size_t)t * (NX * NU) + i] = yk[a * LX + j];
      }
    if (ts == 0) {
      if (co) co[t] = cmask;
      if (io) io[t] = s_it;
    }
    __syncthreads();
    // ---- Vxx = Qxx + K' H + Qux' K; Vx = Qx + K' tmp + Qux' k; dV
    lq_mm<NX, NX, NU>(vxx, LX, vxx, LX, yk, 1, LX, w, LX, 1, ts);
    lq_mm<NX, NX, NU>(vxx, LX, vxx, LX, qux, 1, LX, yk, LX, 1, ts);
    {
      const int r = LQ_NT - 1 - ts;
      if (r < NX) {
        double s = 0.0, u = 0.0;
        for (int m = 0; m < NU; m++) s = fma(yk[m * LX + r], tmp[m], s);
        for (int m = 0; m < NU; m++) u = fma(qux[m * LX + r], kv[m], u);
        vx[r] = qx[r] + (s + u);
      }
    }
    if (ts == 0) {
      double s = 0.0, u = 0.0;
      for (int m = 0; m < NU; m++) { s = fma(kv[m], qu[m], s); u = fma(kv[m], qk[m], u); }
      dv0 += s;
      dv1 += 0.5 * u;
    }
    __syncthreads();
    // ---- Vxx = 0.5 (Vxx + Vxx'): one thread per pair
    for (int p = ts; p < NX * NX; p += LQ_NT) {
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
void kmanip_launch_lqr_backward_box(const KModelDesc& hd, const KLqrBoxIn& in, int n, int T, const KLqrBoxDev& out, hipStream_t stream) {
  if (hd.nlink <= 10) hipLaunchKernelGGL((k_lqr_backward_box<32, 10>), dim3(n), dim3(LQ_NT), 0, stream, in, n, T, out);
  else hipLaunchKernelGGL((k_lqr_backward_box<52, 20>), dim3(n), dim3(LQ_NT), 0, stream, in, n, T, out);
}
