/*
 * kmanip_debug.h -- diagnostic entry points of libkmanip_hip.so.  NOT part of the drop-in boundary (include/kmanip.h):
 * nothing here replaces a reference interface; the measurement tools under tools/ and tests/tools/ and one GPU test
 * (tests/test_gpu_config_sizes.py, the cost-sorted dispatch order) bind them.  They are declared here so that every
 * exported symbol of the library is declared in a header (tests/test_abi.py).
 */
#ifndef KMANIP_DEBUG_H
#define KMANIP_DEBUG_H

#include "kmanip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Product build.  With KMANIP_WAVE_CLOCKS=1 in the environment at kmanip_create: per wave slot, the s_memtime ticks its wave
 * spent in the last k_step (clk, HOST unsigned long long[num_envs]); always: the env each dispatch slot held in the LAST step
 * launch (slot_env, HOST int32[num_envs]: the order k_sort_envs chose, the SPREAD map of that launch's shape, the identity
 * otherwise) and every env's work counter of its last step (work, HOST int32[num_envs]; zero on the single-arm kernel, which ships
 * without the counters).  Any pointer may be NULL; clk needs the environment variable (an error otherwise).  Synchronous. */
KMANIP_API int kmanip_dbg_wave_clocks(KHandle h, unsigned long long* clk, int32_t* slot_env, int32_t* work);

/* The kernels' FP64 math and quaternion helpers (csrc/kmanip_math.hpp, kmanip_device.hpp, quat_log_diff of kmanip_dyn_rows.hpp), one
 * function applied to each of n rows: row i of in_dev (DEVICE double[n][in_cols]) is the function's arguments, row i of out_dev
 * (DEVICE double[n][out_cols]) its results, with no arithmetic of the probe's own in between (tests/test_math_gpu.py holds them to
 * a 50-digit reference).  fn, arguments -> results:
 *   KM_MATH_SINCOS x -> sin, cos            KM_MATH_ATAN2 y, x -> atan2          KM_MATH_SQRT / _RCP / _FRCP / _RSQRT_NR x -> f(x)
 *   KM_MATH_NORMALIZE3 v[3] -> v[3], the returned norm                         KM_MATH_NORMALIZE4 q[4] -> q[4]
 *   KM_MATH_AXIS_ANGLE axis[3], angle -> q[4]                                  KM_MATH_MAT2QUAT m[9] -> q[4]
 *   KM_MATH_SUB_QUAT qa[4], qb[4] -> res[3]   KM_MATH_SUB_QUAT_SC qa[4], qb[4] -> res[3], sn, ac   KM_MATH_QUAT_LOG_DIFF a[4], b[4] -> r[3]
 * The handle gives the device and is only read.  An unknown fn, column counts other than the function's, a NULL pointer (with
 * n > 0) or a negative n is an error (kmanip_last_error) and launches nothing; n = 0 succeeds.  Asynchronous on `stream`. */
enum {
  KM_MATH_SINCOS = 0, KM_MATH_ATAN2, KM_MATH_SQRT, KM_MATH_RCP, KM_MATH_FRCP, KM_MATH_RSQRT_NR, KM_MATH_NORMALIZE3, KM_MATH_NORMALIZE4,
  KM_MATH_AXIS_ANGLE, KM_MATH_MAT2QUAT, KM_MATH_SUB_QUAT, KM_MATH_SUB_QUAT_SC, KM_MATH_QUAT_LOG_DIFF, KM_MATH_NFN
};
KMANIP_API int kmanip_dbg_math(KHandle h, int fn, int n, const double* in_dev, int in_cols, double* out_dev, int out_cols, void* stream);

#ifdef KM_PROFILE
/* -DKM_PROFILE build only (libkmanip_hip_prof.so, `make prof`; never shipped, never timed as the product): the in-kernel
 * phase stamps' accumulators, KM_NPH slots per variant object (tools/phase_profile.py). */
KMANIP_API int kmanip_dbg_prof(unsigned long long* out, int reset);          /* single-arm Newton object */
KMANIP_API int kmanip_dbg_prof_blocks(unsigned long long* out, int nblocks);  /* its first workgroups, per env */
KMANIP_API int kmanip_dbg_prof20(unsigned long long* out, int reset);        /* two-arm Newton object */
#endif

#ifdef __cplusplus
}
#endif
#endif /* KMANIP_DEBUG_H */
