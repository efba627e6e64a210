// kmanip_actor_grad_head.hpp -- what k_actor_bwd (kmanip_actor_grad.hip) and k_actor_bwd_bf16 (kmanip_actor_grad_bfloat.hip) do around
// their layers, written once so that both kernels compile the same source: the row's record and its guard, the observation read, and
// the three loss heads with their writes of row_loss, logp and status (include/kmanip.h KActorGradIn has the definition).
#pragma once
#include "kmanip_actor_layer.hpp"

// Lane (g, n) of the wave of tile blockIdx.x: its row, the row's record, and the status -- an index outside the buffer is status 2 and
// never an address.
struct AgradRow { int row, rec, status; bool live, ok; };

__device__ __forceinline__ AgradRow agrad_row(const KActorGradIn& in, int n, int lane) {
  AgradRow rw;
  rw.row = blockIdx.x * 16 + (lane & 15);
  rw.live = rw.row < n;
  rw.rec = 0; rw.status = 0;
  if (rw.live) {
    rw.rec = in.idx ? in.idx[rw.row] : rw.row;
    if (rw.rec < 0 || rw.rec >= in.n_records) rw.status = 2;
  }
  rw.ok = rw.live && rw.status == 0;
  return rw;
}

// input k of the row's record: normalised in float64, cast once; zero beyond the real inputs and in a row that is not ok
__device__ __forceinline__ float agrad_obs(const KActorGradIn& in, const AgradRow& rw, int id, int k) {
  if (!rw.ok || k >= id) return 0.f;
  double v = in.obs[(size_t)rw.rec * id + k];
  if (in.obs_mean) v = v - in.obs_mean[k];
  if (in.obs_inv_std) v = v * in.obs_inv_std[k];
  return (float)v;
}

// Lane (g, n) holds outputs 4 g .. 4 g + 3 of its row in `mean`: the head in float64, gmean rounded to float32 once.  gm: dL/dmean;
// lt: the log_std terms coef (u^2 - 1) of the PPO head; both zero in a row that is not ok.  Every lane of the wave calls it.
__device__ __forceinline__ void agrad_head(const KActorGradIn& in, const KActorGradDev& out, int od, const AgradRow& rw, int g, const f4 mean,
                                           f4& gm, f4& lt) {
#pragma clang fp contract(off)
  const int row = rw.row, rec = rw.rec;
  const bool live = rw.live, ok = rw.ok;
  gm = f4{0.f, 0.f, 0.f, 0.f}; lt = gm;
  const size_t at = (size_t)rec * od + 4 * g;
  double part = 0.0, u[4] = {0.0, 0.0, 0.0, 0.0}, isd[4] = {0.0, 0.0, 0.0, 0.0};
  if (ok) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (4 * g + c < od) {
        if (in.head == KM_AGRAD_GIVEN) gm[c] = (float)(in.scale * (double)in.g[at + c]);
        else if (in.head == KM_AGRAD_MSE) {
          const double e = (double)mean[c] - (double)in.target[at + c];
          gm[c] = (float)(in.scale * e);
          part = part + e * e;
        } else {
          const float ls = in.log_std[4 * g + c];
          const float sd = (float)exp((double)ls);                   // as k_actor: float64, rounded once
          isd[c] = 1.0 / (double)sd;
          u[c] = ((double)in.raw[at + c] - (double)mean[c]) / (double)sd;
          part = part + (((-0.5 * (u[c] * u[c])) - (double)ls) - 0.9189385332046727);
        }
      }
    }
  }
  if (in.head != KM_AGRAD_GIVEN) {                                   // (wave-uniform: every lane reaches the shuffles or none)
    // the four lane groups of a row, a fixed order: (g ^ 1) first, then (g ^ 2); every lane ends with the same bits
    part = part + __shfl_xor(part, 16, 64);
    part = part + __shfl_xor(part, 32, 64);
    double loss = 0.5 * part;
    if (in.head == KM_AGRAD_PPO_CLIP && ok) {
      const double adv = (double)in.adv[rec], rho = exp(part - in.logp_old[rec]);
      const double s = rho * adv, cl = fmin(fmax(rho, 1.0 - in.clip), 1.0 + in.clip) * adv;
      const double coef = s <= cl ? -in.scale * adv * rho : 0.0;
      loss = -fmin(s, cl);
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (4 * g + c < od) {
          gm[c] = (float)(coef * u[c] * isd[c]);
          lt[c] = (float)(coef * (u[c] * u[c] - 1.0));
        }
    }
    if (live && g == 0) {
      if (out.row_loss) out.row_loss[row] = ok ? loss : 0.0;
      if (out.logp && in.head == KM_AGRAD_PPO_CLIP) out.logp[row] = ok ? part : 0.0;
    }
  }
  if (live && g == 0 && out.status) out.status[row] = rw.status;
}
