// kmanip_dispatch.hip -- host-side choice of the per-variant object: build x link-count class x solver.
#include "kmanip_device.hpp"

// the link classes (links, lanes per env), in table order: nlink <= 10 selects the first
#define KM_CLASSES(X, B) X(B, 10, 16) X(B, 20, 32)
// the builds of a per-variant translation unit, by the tag in its launchers' names, in table order (index = PAR + 2 * FRC): default,
// per-env physics parameters (KM_VAR_PAR: launched while KDeviceState::envp is set), applied force (KM_VAR_FRC: while
// KDeviceState::qfrc_applied is set), both.  A reset ignores the force, and so do kmanip_kinematics and kmanip_inverse: no force builds.
#define KM_BUILDS_PAR(X) X() X(ep_)
#define KM_BUILDS(X) KM_BUILDS_PAR(X) X(frc_) X(ep_frc_)
// the builds of kmanip_paramfd.hip, always a parameter build (index = FRC)
#define KM_BUILDS_EP(X) X(ep_) X(ep_frc_)
#define KM_NAME(kind, B, NL, G, S) kmanip_launch_##kind##_##B##NL##_##G##S

typedef void StepFn(const KDeviceModel*, const KDeviceState&, const float*, double*, double*, uint8_t*, int, int, hipStream_t);
typedef void ResetFn(const KDeviceModel*, const KDeviceState&, const uint8_t*, double*, int, hipStream_t);
typedef void ObserveFn(const KDeviceModel*, const KDeviceState&, double*, double*, hipStream_t);
typedef void PrepareFn(KDeviceModel*, hipStream_t);
typedef void ForcesFn(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
typedef void KinFn(const KDeviceModel*, const KDeviceState&, const KKinDev&, hipStream_t);
typedef void InverseFn(const KDeviceModel*, const KDeviceState&, const KInverseIn&, const KInverseDev&, hipStream_t);
typedef void ForwardFn(const KDeviceModel*, const KDeviceState&, const KForwardIn&, int, const KForcesDev&, hipStream_t);
typedef void KinRowsFn(const KDeviceModel*, const KDeviceState&, const KKinRowsIn&, int, const KKinDev&, hipStream_t);
typedef void SiteCostFn(const KDeviceModel*, const KDeviceState&, const KSiteCostIn&, int, const KSiteCostDev&, hipStream_t);
typedef void RolloutFn(const KDeviceModel*, const KDeviceState&, const KRolloutIn&, int, int, int, const KRolloutDev&, hipStream_t);
typedef void FeedbackFn(const KDeviceModel*, const KDeviceState&, const KFeedbackIn&, int, int, int, const KFeedbackDev&, hipStream_t);
typedef void BoxFbFn(const KDeviceModel*, const KDeviceState&, const KFeedbackBoxIn&, int, int, int, const KFeedbackDev&, hipStream_t);
typedef void ParamFdFn(const KDeviceModel*, const KDeviceState&, const KParamFdIn&, const KEnvParamDefaults&, int, int, int, const KParamFdDev&, hipStream_t);
typedef void TransFdFn(const KDeviceModel*, const KDeviceState&, const KTransFdIn&, int, int, int, double, double, const KTransFdDev&, hipStream_t);

// kmanip_dyn.hip: step per solver in every build, reset per solver in the parameter builds; observe and prepare are
// solver-independent, one copy per class (in the default Newton object)
#define KM_STEP_ROW(B, NL, G) {KM_NAME(step, B, NL, G, _0), KM_NAME(step, B, NL, G, _1)},
#define KM_RESET_ROW(B, NL, G) {KM_NAME(reset, B, NL, G, _0), KM_NAME(reset, B, NL, G, _1)},
// kmanip_rollout.hip: per solver in every build, like the step
#define KM_ROLLOUT_ROW(B, NL, G) {KM_NAME(rollout, B, NL, G, _0), KM_NAME(rollout, B, NL, G, _1)},
// kmanip_rollout.hip built with KM_VAR_FB (the kmanip_feedback_* objects): likewise
#define KM_FEEDBACK_ROW(B, NL, G) {KM_NAME(feedback, B, NL, G, _0), KM_NAME(feedback, B, NL, G, _1)},
// kmanip_rollout.hip built with KM_VAR_FB=2 (the kmanip_boxfb_* objects): likewise
#define KM_BOXFB_ROW(B, NL, G) {KM_NAME(boxfb, B, NL, G, _0), KM_NAME(boxfb, B, NL, G, _1)},
// kmanip_transfd.hip: likewise
#define KM_TRANSFD_ROW(B, NL, G) {KM_NAME(transfd, B, NL, G, _0), KM_NAME(transfd, B, NL, G, _1)},
// kmanip_paramfd.hip: per solver, the two parameter builds
#define KM_PARAMFD_ROW(B, NL, G) {KM_NAME(paramfd, B, NL, G, _0), KM_NAME(paramfd, B, NL, G, _1)},
#define KM_OBSERVE_ROW(B, NL, G) KM_NAME(observe, B, NL, G, _1),
#define KM_PREPARE_ROW(B, NL, G) KM_NAME(prepare, B, NL, G, _1),
// kmanip_forces.hip and kmanip_forward.hip (the Newton classes, every build), kmanip_kinematics.hip and kmanip_inverse.hip (one object per class serves both
// solvers, the parameter builds)
#define KM_FORCES_ROW(B, NL, G) KM_NAME(forces, B, NL, G, ),
#define KM_KIN_ROW(B, NL, G) KM_NAME(kinematics, B, NL, G, ),
#define KM_INVERSE_ROW(B, NL, G) KM_NAME(inverse, B, NL, G, ),
#define KM_FORWARD_ROW(B, NL, G) KM_NAME(forward, B, NL, G, ),
// kmanip_sitekin.hip: two launchers per object, one object per class, the parameter builds
#define KM_KINROWS_ROW(B, NL, G) KM_NAME(kinrows, B, NL, G, ),
#define KM_SITECOST_ROW(B, NL, G) KM_NAME(sitecost, B, NL, G, ),

#define KM_DECL_SOLVERS(Fn, kind, B, NL, G) Fn KM_NAME(kind, B, NL, G, _0), KM_NAME(kind, B, NL, G, _1);
#define KM_DECL_FRC(B, NL, G) KM_DECL_SOLVERS(StepFn, step, B, NL, G) KM_DECL_SOLVERS(RolloutFn, rollout, B, NL, G) KM_DECL_SOLVERS(FeedbackFn, feedback, B, NL, G) KM_DECL_SOLVERS(BoxFbFn, boxfb, B, NL, G) KM_DECL_SOLVERS(TransFdFn, transfd, B, NL, G) ForcesFn KM_NAME(forces, B, NL, G, ); ForwardFn KM_NAME(forward, B, NL, G, );
#define KM_DECL_PAR(B, NL, G) KM_DECL_SOLVERS(ResetFn, reset, B, NL, G) KinFn KM_NAME(kinematics, B, NL, G, ); InverseFn KM_NAME(inverse, B, NL, G, ); KinRowsFn KM_NAME(kinrows, B, NL, G, ); SiteCostFn KM_NAME(sitecost, B, NL, G, );
#define KM_DECL_ONCE(B, NL, G) ObserveFn KM_NAME(observe, B, NL, G, _1); PrepareFn KM_NAME(prepare, B, NL, G, _1);
#define KM_DECL_EP(B, NL, G) KM_DECL_SOLVERS(ParamFdFn, paramfd, B, NL, G)
#define KM_DECL_BUILD_FRC(B) KM_CLASSES(KM_DECL_FRC, B)
#define KM_DECL_BUILD_EP(B) KM_CLASSES(KM_DECL_EP, B)
#define KM_DECL_BUILD_PAR(B) KM_CLASSES(KM_DECL_PAR, B)
KM_BUILDS(KM_DECL_BUILD_FRC) KM_BUILDS_PAR(KM_DECL_BUILD_PAR) KM_BUILDS_EP(KM_DECL_BUILD_EP) KM_CLASSES(KM_DECL_ONCE, )

// the tables: [build][class][solver], [build][class] or [class]
#define KM_STEP_BUILD(B) {KM_CLASSES(KM_STEP_ROW, B)},
#define KM_RESET_BUILD(B) {KM_CLASSES(KM_RESET_ROW, B)},
#define KM_FORCES_BUILD(B) {KM_CLASSES(KM_FORCES_ROW, B)},
#define KM_KIN_BUILD(B) {KM_CLASSES(KM_KIN_ROW, B)},
#define KM_INVERSE_BUILD(B) {KM_CLASSES(KM_INVERSE_ROW, B)},
#define KM_FORWARD_BUILD(B) {KM_CLASSES(KM_FORWARD_ROW, B)},
#define KM_KINROWS_BUILD(B) {KM_CLASSES(KM_KINROWS_ROW, B)},
#define KM_SITECOST_BUILD(B) {KM_CLASSES(KM_SITECOST_ROW, B)},
#define KM_ROLLOUT_BUILD(B) {KM_CLASSES(KM_ROLLOUT_ROW, B)},
#define KM_FEEDBACK_BUILD(B) {KM_CLASSES(KM_FEEDBACK_ROW, B)},
#define KM_BOXFB_BUILD(B) {KM_CLASSES(KM_BOXFB_ROW, B)},
#define KM_TRANSFD_BUILD(B) {KM_CLASSES(KM_TRANSFD_ROW, B)},
#define KM_PARAMFD_BUILD(B) {KM_CLASSES(KM_PARAMFD_ROW, B)},
static constexpr StepFn* step_tab[4][2][2] = {KM_BUILDS(KM_STEP_BUILD)};
static constexpr ResetFn* reset_tab[2][2][2] = {KM_BUILDS_PAR(KM_RESET_BUILD)};
static constexpr ObserveFn* observe_tab[2] = {KM_CLASSES(KM_OBSERVE_ROW, )};
static constexpr PrepareFn* prepare_tab[2] = {KM_CLASSES(KM_PREPARE_ROW, )};
static constexpr ForcesFn* forces_tab[4][2] = {KM_BUILDS(KM_FORCES_BUILD)};
static constexpr KinFn* kin_tab[2][2] = {KM_BUILDS_PAR(KM_KIN_BUILD)};
static constexpr InverseFn* inverse_tab[2][2] = {KM_BUILDS_PAR(KM_INVERSE_BUILD)};
static constexpr ForwardFn* forward_tab[4][2] = {KM_BUILDS(KM_FORWARD_BUILD)};
static constexpr KinRowsFn* kinrows_tab[2][2] = {KM_BUILDS_PAR(KM_KINROWS_BUILD)};
static constexpr SiteCostFn* sitecost_tab[2][2] = {KM_BUILDS_PAR(KM_SITECOST_BUILD)};
static constexpr RolloutFn* rollout_tab[4][2][2] = {KM_BUILDS(KM_ROLLOUT_BUILD)};
static constexpr FeedbackFn* feedback_tab[4][2][2] = {KM_BUILDS(KM_FEEDBACK_BUILD)};
static constexpr BoxFbFn* boxfb_tab[4][2][2] = {KM_BUILDS(KM_BOXFB_BUILD)};
static constexpr TransFdFn* transfd_tab[4][2][2] = {KM_BUILDS(KM_TRANSFD_BUILD)};
static constexpr ParamFdFn* paramfd_tab[2][2][2] = {KM_BUILDS_EP(KM_PARAMFD_BUILD)};

static int cls(const KModelDesc& hd) { return hd.nlink <= 10 ? 0 : 1; }
static int newton(const KModelDesc& hd) { return hd.solver == KM_SOLVER_NEWTON ? 1 : 0; }
static int par(const KDeviceState& st) { return st.envp ? 1 : 0; }
static int frc(const KDeviceState& st) { return st.qfrc_applied ? 2 : 0; }
// a call over rows the caller passes (KForwardIn, KRolloutIn, KFeedbackIn): the force build iff a row can have a force -- the caller's
// rows or the handle's bound buffer
template <class In>
static int row_build(const KDeviceState& st, const In& in) { return par(st) + ((in.qfrc_applied || st.qfrc_applied) ? 2 : 0); }

void kmanip_launch_step(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const float* act, double* obs, double* reward,
                        uint8_t* done, int nchunk, int epb, hipStream_t stream) {
  step_tab[par(st) + frc(st)][cls(hd)][newton(hd)](dm, st, act, obs, reward, done, nchunk, epb, stream);
}
void kmanip_launch_reset(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const uint8_t* mask, double* obs,
                         int epb, hipStream_t stream) {
  reset_tab[par(st)][cls(hd)][newton(hd)](dm, st, mask, obs, epb, stream);
}
void kmanip_launch_observe(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, double* obs, double* reward,
                           hipStream_t stream) {
  observe_tab[cls(hd)](dm, st, obs, reward, stream);
}
void kmanip_launch_forces(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KForcesDev& out, hipStream_t stream) {
  forces_tab[par(st) + frc(st)][cls(hd)](dm, st, out, stream);
}
void kmanip_launch_kinematics(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KKinDev& out, hipStream_t stream) {
  kin_tab[par(st)][cls(hd)](dm, st, out, stream);
}
void kmanip_launch_inverse(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KInverseIn& in, const KInverseDev& out,
                           hipStream_t stream) {
  inverse_tab[par(st)][cls(hd)](dm, st, in, out, stream);
}
void kmanip_launch_forward(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KForwardIn& in, int n,
                           const KForcesDev& out, hipStream_t stream) {
  forward_tab[row_build(st, in)][cls(hd)](dm, st, in, n, out, stream);
}
void kmanip_launch_kinrows(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KKinRowsIn& in, int n,
                           const KKinDev& out, hipStream_t stream) {
  kinrows_tab[par(st)][cls(hd)](dm, st, in, n, out, stream);
}
void kmanip_launch_sitecost(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KSiteCostIn& in, int n,
                            const KSiteCostDev& out, hipStream_t stream) {
  sitecost_tab[par(st)][cls(hd)](dm, st, in, n, out, stream);
}
void kmanip_launch_rollout(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KRolloutIn& in, int n, int nstep,
                           int nsub, const KRolloutDev& out, hipStream_t stream) {
  rollout_tab[row_build(st, in)][cls(hd)][newton(hd)](dm, st, in, n, nstep, nsub, out, stream);
}
void kmanip_launch_feedback(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KFeedbackIn& in, int n, int nstep,
                            int nsub, const KFeedbackDev& out, hipStream_t stream) {
  feedback_tab[row_build(st, in)][cls(hd)][newton(hd)](dm, st, in, n, nstep, nsub, out, stream);
}
void kmanip_launch_boxfb(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KFeedbackBoxIn& in, int n, int nstep,
                         int nsub, const KFeedbackDev& out, hipStream_t stream) {
  boxfb_tab[row_build(st, in)][cls(hd)][newton(hd)](dm, st, in, n, nstep, nsub, out, stream);
}
// (the force build also for a differentiated force nobody gave: the kernel then perturbs rows of zeros)
void kmanip_launch_transfd(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KTransFdIn& in, int n, int ncol,
                           int nsub, double ch, double sh, const KTransFdDev& out, hipStream_t stream) {
  const int build = par(st) + ((in.qfrc_applied || st.qfrc_applied || (in.wrt & KM_WRT_FRC)) ? 2 : 0);
  transfd_tab[build][cls(hd)][newton(hd)](dm, st, in, n, ncol, nsub, ch, sh, out, stream);
}
// (a parameter build whatever par(st) says: the kernel takes the parameters from its arguments)
void kmanip_launch_paramfd(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KParamFdIn& in,
                           const KEnvParamDefaults& model, int n, int npar, int nsub, const KParamFdDev& out, hipStream_t stream) {
  paramfd_tab[(in.qfrc_applied || st.qfrc_applied) ? 1 : 0][cls(hd)][newton(hd)](dm, st, in, model, n, npar, nsub, out, stream);
}
void kmanip_launch_prepare_model(KDeviceModel* dm, const KModelDesc& hd, hipStream_t stream) {
  prepare_tab[cls(hd)](dm, stream);
}
