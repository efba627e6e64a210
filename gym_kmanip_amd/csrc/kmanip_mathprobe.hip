// kmanip_mathprobe.hip -- kmanip_dbg_math (include/kmanip_debug.h): the kernels' FP64 math and quaternion helpers, one function per
// launch, one row per lane.  A row's arguments are loaded, ONE function of kmanip_math.hpp / kmanip_device.hpp /
// kmanip_dyn_rows.hpp is called on them and what it returns is stored: no arithmetic of the probe's own stands between input and
// output, so that what tests/test_math_gpu.py measures is the code the kernels call (compiled with the library's flags; a kernel
// may contract an expression around an inlined call differently, inside the helpers the FMAs are spelt out or the same rule applies).
// A diagnostic: it reads no handle state and nothing in the step path calls it.
#include <hip/hip_runtime.h>

#include "kmanip_ik_coop.hpp"          // kmanip_device.hpp, kmanip_math.hpp
// quat_log_diff lives with the row entry of the per-variant query units; their prelude is only declared here (no kernel of it is
// instantiated), with the macros of the single-arm Newton variant
#define KM_VAR_NL 10
#define KM_VAR_G 16
#define KM_VAR_SOLVER 1
#include "kmanip_dyn_variant.hpp"
#include "kmanip_dyn_rows.hpp"
KM_VARIANT_END

namespace {

struct ProbeCols { int in, out; };
// indexed by KM_MATH_*
constexpr ProbeCols PROBE_COLS[KM_MATH_NFN] = {{1, 2}, {2, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {3, 4}, {4, 4}, {4, 4}, {9, 4}, {8, 3}, {8, 5}, {8, 3}};

template <int FN>
__global__ void __launch_bounds__(256) k_math_probe(int n, const double* __restrict__ in, double* __restrict__ out) {
  constexpr int IC = PROBE_COLS[FN].in, OC = PROBE_COLS[FN].out;
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= (size_t)n) return;
  real a[IC], r[OC];
#pragma unroll
  for (int i = 0; i < IC; i++) a[i] = in[row * IC + i];
  if constexpr (FN == KM_MATH_SINCOS) km_sincos(a[0], &r[0], &r[1]);
  else if constexpr (FN == KM_MATH_ATAN2) r[0] = km_atan2(a[0], a[1]);
  else if constexpr (FN == KM_MATH_SQRT) r[0] = km_sqrt(a[0]);
  else if constexpr (FN == KM_MATH_RCP) r[0] = km_rcp(a[0]);
  else if constexpr (FN == KM_MATH_FRCP) r[0] = frcp(a[0]);
  else if constexpr (FN == KM_MATH_RSQRT_NR) r[0] = rsqrt_nr(a[0]);
  else if constexpr (FN == KM_MATH_NORMALIZE3) { r[3] = normalize3_fast(a); r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; }
  else if constexpr (FN == KM_MATH_NORMALIZE4) { normalize4_fast(a); r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3]; }
  else if constexpr (FN == KM_MATH_AXIS_ANGLE) axis_angle2quat(r, a, a[3]);
  else if constexpr (FN == KM_MATH_MAT2QUAT) mat2quat(r, a);
  else if constexpr (FN == KM_MATH_SUB_QUAT) sub_quat(r, a, a + 4);
  else if constexpr (FN == KM_MATH_SUB_QUAT_SC) sub_quat_sc(r, a, a + 4, r[3], r[4]);
  else {
    static_assert(FN == KM_MATH_QUAT_LOG_DIFF, "one branch per KM_MATH_* function");
    const real qa[4] = {a[0], a[1], a[2], a[3]}, qb[4] = {a[4], a[5], a[6], a[7]};
    real rot[3];
    quat_log_diff(qa, qb, rot);
    r[0] = rot[0]; r[1] = rot[1]; r[2] = rot[2];
  }
#pragma unroll
  for (int i = 0; i < OC; i++) out[row * OC + i] = r[i];
}

template <int FN>
void launch_fn(int fn, int n, const double* in, double* out, hipStream_t stream) {
  if (fn == FN) hipLaunchKernelGGL((k_math_probe<FN>), dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, stream, n, in, out);
  else if constexpr (FN + 1 < KM_MATH_NFN) launch_fn<FN + 1>(fn, n, in, out, stream);
}

}  // namespace

bool kmanip_math_probe_cols(int fn, int* in_cols, int* out_cols) {
  if (fn < 0 || fn >= KM_MATH_NFN) return false;
  *in_cols = PROBE_COLS[fn].in; *out_cols = PROBE_COLS[fn].out;
  return true;
}

// n > 0 rows, fn one of KM_MATH_* (kmanip_api.hip checks both)
void kmanip_launch_math_probe(int fn, int n, const double* in, double* out, hipStream_t stream) {
  launch_fn<0>(fn, n, in, out, stream);
}
