// kmanip_dyn_variant.hpp -- the build macros of one per-variant object and the device code of one step, by phase.  Included once,
// after kmanip_ik_coop.hpp, by each translation unit the Makefile compiles per (links, lanes per env[, solver]) variant:
// kmanip_dyn.hip, kmanip_forces.hip, kmanip_kinematics.hip, kmanip_inverse.hip, kmanip_forward.hip, kmanip_rollout.hip (the
// kmanip_feedback_* objects are its too, built with its own KM_VAR_FB), kmanip_transfd.hip, kmanip_paramfd.hip (KM_VAR_PAR builds only) and kmanip_sitekin.hip.  It opens the build's namespace; KM_VARIANT_END,
// after the unit's kernels and launch templates, closes it.
#pragma once
#ifndef KM_VAR_NL
#error "compile with -DKM_VAR_NL=<10|20> -DKM_VAR_G=<16|32> -DKM_VAR_SOLVER=<0|1>"
#endif
// KM_VAR_PAR=1: the per-env physics parameter build of a variant (kmanip_set_env_params).  The Makefile
// compiles a unit a second time per variant with it; those kernels live in their own namespace and are launched only while a
// handle has parameters; the default objects take none of the parameter code paths (same instruction counts, registers,
// scratch and LDS as before).
#ifndef KM_VAR_PAR
#define KM_VAR_PAR 0
#endif
// KM_VAR_FRC=1: the applied-force build (kmanip_bind_applied_force), orthogonal to KM_VAR_PAR and built by the
// same rule: a third and a fourth compilation per variant, kernels in namespaces of their own, launched only while a handle has a
// force buffer bound.  kmanip_dyn.hip (step kernels only: a reset never reads the buffer), kmanip_forces.hip, kmanip_forward.hip and
// kmanip_rollout.hip have these builds (the last two also launch them for a force the caller passes).
#ifndef KM_VAR_FRC
#define KM_VAR_FRC 0
#endif
// ---- the build's name parts: kernel names of their own, so that profiles and tools/kernel_resources.py tell the builds apart
#if KM_VAR_PAR
#define KM_EP_SFX _ep
#define KM_EP_TAG ep_
#else
#define KM_EP_SFX
#define KM_EP_TAG
#endif
#if KM_VAR_FRC
#define KM_FRC_SFX _frc
#define KM_FRC_TAG frc_
#else
#define KM_FRC_SFX
#define KM_FRC_TAG
#endif
#if KM_VAR_PAR && KM_VAR_FRC
#define KM_VARIANT_NS km_envp_frc
#elif KM_VAR_FRC
#define KM_VARIANT_NS km_frc
#elif KM_VAR_PAR
#define KM_VARIANT_NS km_envp
#endif
#define KM_PASTE_(a, b, c, d, e, f) a##b##c##d##e##f
#define KM_PASTE(a, b, c, d, e, f) KM_PASTE_(a, b, c, d, e, f)
// k_step -> k_step | k_step_ep | k_step_frc | k_step_ep_frc
#define KM_KERNEL(base) KM_PASTE(base, KM_EP_SFX, KM_FRC_SFX, , , )
// forces -> k_forces | k_forces_ep | k_frc_forces | k_frc_forces_ep ("frc" first: tools that list the k_forces kernels by name keep
// seeing the default four)
#define KM_KERNEL_FRC_FIRST(base) KM_PASTE(k_, KM_FRC_TAG, base, KM_EP_SFX, , )
// forces -> kmanip_launch_forces_[ep_][frc_]<NL>_<G>, the name kmanip_dispatch.hip declares; KM_LAUNCHER3: with _<SOLVER> after it
#define KM_LAUNCHER2(base) KM_PASTE(kmanip_launch_##base##_, KM_EP_TAG, KM_FRC_TAG, KM_VAR_NL, _, KM_VAR_G)
#define KM_LAUNCHER3(base) KM_PASTE(KM_LAUNCHER2(base), _, KM_VAR_SOLVER, , , )
#ifdef KM_VARIANT_NS
namespace KM_VARIANT_NS {
#define KM_VARIANT_END } using namespace KM_VARIANT_NS;
#else
#define KM_VARIANT_END
#endif
// tree loops over link candidates (static addresses + a mask bit each): fully unrolled for the 10-link model, where all the
// loads can be in flight together; the 20-link models sit at the 512-register limit and keep them rolled
#define KM_TREE_UNROLL(NL) NL <= 10 ? NL : 1

// Work units one Newton iteration of each kind adds to Ws::work (roughly kilo-clocks on the two-arm kernels; only their ORDER
// matters: k_sort_envs ranks the envs by them).  Two-arm kernels only: the single-arm headline launch is one residency round.
// (measured on the single-arm kernel, tests/tools/wave_times.py with -DKM_WORK_COUNTERS_ALL: wave cycles = 375 k + 308 x the
// slowest env's work units + 13.8 k x the largest IK evaluation count, R^2 0.66; the counters cost it 1.5 %, so it ships without)
#ifdef KM_WORK_COUNTERS_ALL
#define KM_WORK_COUNTERS(NL) true
#else
#define KM_WORK_COUNTERS(NL) ((NL) > 10)
#endif
#define KM_WORK_ALL 40
#define KM_WORK_ARM 14
#define KM_WORK_PLAIN 3
#define KM_WORK_CUBE 5
// the device code of one step, by phase (textual order matters: each part uses the ones before it)
#include "kmanip_dyn_ws.hpp"
#include "kmanip_dyn_tree.hpp"
#include "kmanip_dyn_constraints.hpp"
#include "kmanip_dyn_newton.hpp"
#include "kmanip_dyn_env.hpp"
