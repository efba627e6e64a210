// kmanip_actor_head.hpp -- what k_actor (kmanip_actor.hip) and k_actor_bf16 (kmanip_actor_bfloat.hip) do around their layers, written
// once so that both kernels compile the same source: the row's env and its guard, the observation read, and the writes of the mean,
// the status and the Gaussian head (include/kmanip.h has the definition).  At the same handle state the noise and logp of the two
// kernels are therefore the same bits, and raw and act the same float32 arithmetic on each call's own mean.
#pragma once
#include "kmanip_actor_layer.hpp"

// Lane (g, n) of the wave of tile blockIdx.x: its row, the row's env, and the status -- an index outside the handle is status 2 and
// never an address.
struct ActorRow { int row, env, status; bool live, ok; };

__device__ __forceinline__ ActorRow actor_row(const KDeviceState& st, const KActorIn& in, int n, int lane) {
  ActorRow rw;
  rw.row = blockIdx.x * 16 + (lane & 15);
  rw.live = rw.row < n;
  rw.env = 0; rw.status = 0;
  if (rw.live) {
    rw.env = in.envs ? in.envs[rw.row] : rw.row;
    if (rw.env < 0 || rw.env >= st.num_envs) rw.status = 2;
  }
  rw.ok = rw.live && rw.status == 0;
  return rw;
}

// input k of the row: normalised in float64, cast once; zero beyond the real inputs and in a row that is not ok
__device__ __forceinline__ float actor_obs(const KActorIn& in, const ActorRow& rw, int id, int k) {
  if (!rw.ok || k >= id) return 0.f;
  double v = in.obs[(size_t)rw.row * id + k];
  if (in.obs_mean) v = v - in.obs_mean[k];
  if (in.obs_inv_std) v = v * in.obs_inv_std[k];
  return (float)v;
}

// Lane (g, n) holds outputs 4 g .. 4 g + 3 of its row in y: the mean, the status and the Gaussian head.  Every lane of the wave calls it.
__device__ __forceinline__ void actor_head(const KDeviceState& st, const KActorIn& in, const KActorDev& out, int od, const ActorRow& rw, int g,
                                           const f4 y) {
  const int row = rw.row, env = rw.env;
  const bool live = rw.live, ok = rw.ok;
  const f4 mean = ok ? y : f4{0.f, 0.f, 0.f, 0.f};
  if (live && out.mean) {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (4 * g + c < od) out.mean[(size_t)row * od + 4 * g + c] = mean[c];
  }
  if (live && g == 0 && out.status) out.status[row] = rw.status;
  if (!in.log_std) return;                                           // (wave-uniform: every lane reaches the shuffles below or none)
  // ---- the Gaussian head
  {
#pragma clang fp contract(off)
    f4 z = {0.f, 0.f, 0.f, 0.f}, raw = z, act = z;
    double lp = 0.0;
    if (ok) {
      const int64_t genv = st.env_id_offset + env;
      const uint32_t key[2] = {(uint32_t)st.seed, (uint32_t)(st.seed >> 32)};
      const uint32_t ctr[4] = {(uint32_t)genv, (uint32_t)((uint64_t)genv >> 32), (uint32_t)st.episode[env], KM_POL_CTR3(st.step_idx[env], g)};
      uint32_t o[4];
      philox4x32_10(ctr, key, o);
#pragma unroll
      for (int b = 0; b < 2; b++) {                                  // Box-Muller in float64 on words (0, 1), then (2, 3)
        const double u1 = ((double)(o[2 * b] >> 8) + 0.5) * (1.0 / 16777216.0), u2 = ((double)(o[2 * b + 1] >> 8) + 0.5) * (1.0 / 16777216.0);
        const double rho = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
        z[2 * b] = (float)(rho * cos(ang));
        z[2 * b + 1] = (float)(rho * sin(ang));
      }
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int j = 4 * g + c;
        if (j < od) {
          const float ls = in.log_std[j];
          const float sd = (float)exp((double)ls);                   // exp in float64, rounded once: the same float32 on every host
          const float pr = sd * z[c];
          raw[c] = mean[c] + pr;
          act[c] = fminf(fmaxf(raw[c], -1.f), 1.f);
          const double zd = (double)z[c];
          lp = lp + (((-0.5 * (zd * zd)) - (double)ls) - 0.9189385332046727);
        } else z[c] = 0.f;
      }
    }
    // the four lane groups of a row, a fixed order: (g ^ 1) first, then (g ^ 2); every lane ends with the same bits
    lp = lp + __shfl_xor(lp, 16, 64);
    lp = lp + __shfl_xor(lp, 32, 64);
    if (!live) return;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int j = 4 * g + c;
      if (j < od) {
        const size_t at = (size_t)row * od + j;
        if (out.noise) out.noise[at] = z[c];
        if (out.raw) out.raw[at] = raw[c];
        if (out.act) out.act[at] = act[c];
      }
    }
    if (g == 0 && out.logp) out.logp[row] = lp;
  }
}
