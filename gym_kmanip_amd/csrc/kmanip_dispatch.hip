// kmanip_dispatch.hip -- host-side choice of the k_step / k_reset variant (link-count class x solver).
#include "kmanip_device.hpp"

#define KM_DECL(NL, G, S)                                                                                          \
  void kmanip_launch_step_##NL##_##G##_##S(const KDeviceModel*, const KDeviceState&, const float*, double*, double*, uint8_t*, int, int, hipStream_t); \
  void kmanip_launch_reset_##NL##_##G##_##S(const KDeviceModel*, const KDeviceState&, const uint8_t*, double*, int, hipStream_t);
KM_DECL(10, 16, 0) KM_DECL(10, 16, 1) KM_DECL(20, 32, 0) KM_DECL(20, 32, 1)
#undef KM_DECL
// the per-env physics parameter builds (kmanip_dyn.hip KM_VAR_PAR): launched while KDeviceState::envp is set
#define KM_DECL(NL, G, S)                                                                                          \
  void kmanip_launch_step_ep_##NL##_##G##_##S(const KDeviceModel*, const KDeviceState&, const float*, double*, double*, uint8_t*, int, int, hipStream_t); \
  void kmanip_launch_reset_ep_##NL##_##G##_##S(const KDeviceModel*, const KDeviceState&, const uint8_t*, double*, int, hipStream_t);
KM_DECL(10, 16, 0) KM_DECL(10, 16, 1) KM_DECL(20, 32, 0) KM_DECL(20, 32, 1)
#undef KM_DECL
// the applied-force builds (kmanip_dyn.hip KM_VAR_FRC, with and without KM_VAR_PAR): launched while KDeviceState::qfrc_applied is set
#define KM_DECL(NL, G, S)                                                                                          \
  void kmanip_launch_step_frc_##NL##_##G##_##S(const KDeviceModel*, const KDeviceState&, const float*, double*, double*, uint8_t*, int, int, hipStream_t); \
  void kmanip_launch_step_ep_frc_##NL##_##G##_##S(const KDeviceModel*, const KDeviceState&, const float*, double*, double*, uint8_t*, int, int, hipStream_t);
KM_DECL(10, 16, 0) KM_DECL(10, 16, 1) KM_DECL(20, 32, 0) KM_DECL(20, 32, 1)
#undef KM_DECL
void kmanip_launch_observe_10_16_1(const KDeviceModel*, const KDeviceState&, double*, double*, hipStream_t);
void kmanip_launch_prepare_10_16_1(KDeviceModel*, hipStream_t);
void kmanip_launch_prepare_20_32_1(KDeviceModel*, hipStream_t);
void kmanip_launch_observe_20_32_1(const KDeviceModel*, const KDeviceState&, double*, double*, hipStream_t);

// kmanip_forces.hip: the Newton classes, default and per-env parameter builds
void kmanip_launch_forces_10_16(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
void kmanip_launch_forces_20_32(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
void kmanip_launch_forces_ep_10_16(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
void kmanip_launch_forces_ep_20_32(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
void kmanip_launch_forces_frc_10_16(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
void kmanip_launch_forces_frc_20_32(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
void kmanip_launch_forces_ep_frc_10_16(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);
void kmanip_launch_forces_ep_frc_20_32(const KDeviceModel*, const KDeviceState&, const KForcesDev&, hipStream_t);

// kmanip_kinematics.hip: one object per class serves both solvers, default and per-env parameter builds
void kmanip_launch_kinematics_10_16(const KDeviceModel*, const KDeviceState&, const KKinDev&, hipStream_t);
void kmanip_launch_kinematics_20_32(const KDeviceModel*, const KDeviceState&, const KKinDev&, hipStream_t);
void kmanip_launch_kinematics_ep_10_16(const KDeviceModel*, const KDeviceState&, const KKinDev&, hipStream_t);
void kmanip_launch_kinematics_ep_20_32(const KDeviceModel*, const KDeviceState&, const KKinDev&, hipStream_t);
// kmanip_inverse.hip: one object per class serves both solvers, default and per-env parameter builds
void kmanip_launch_inverse_10_16(const KDeviceModel*, const KDeviceState&, const KInverseIn&, const KInverseDev&, hipStream_t);
void kmanip_launch_inverse_20_32(const KDeviceModel*, const KDeviceState&, const KInverseIn&, const KInverseDev&, hipStream_t);
void kmanip_launch_inverse_ep_10_16(const KDeviceModel*, const KDeviceState&, const KInverseIn&, const KInverseDev&, hipStream_t);
void kmanip_launch_inverse_ep_20_32(const KDeviceModel*, const KDeviceState&, const KInverseIn&, const KInverseDev&, hipStream_t);

void kmanip_launch_step(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const float* act, double* obs, double* reward,
                        uint8_t* done, int nchunk, int epb, hipStream_t stream) {
  const bool newton = hd.solver == KM_SOLVER_NEWTON;
  if (st.qfrc_applied && st.envp) {
    if (hd.nlink <= 10) { if (newton) kmanip_launch_step_ep_frc_10_16_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_ep_frc_10_16_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
    else { if (newton) kmanip_launch_step_ep_frc_20_32_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_ep_frc_20_32_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
    return;
  }
  if (st.qfrc_applied) {
    if (hd.nlink <= 10) { if (newton) kmanip_launch_step_frc_10_16_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_frc_10_16_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
    else { if (newton) kmanip_launch_step_frc_20_32_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_frc_20_32_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
    return;
  }
  if (st.envp) {
    if (hd.nlink <= 10) { if (newton) kmanip_launch_step_ep_10_16_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_ep_10_16_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
    else { if (newton) kmanip_launch_step_ep_20_32_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_ep_20_32_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
    return;
  }
  if (hd.nlink <= 10) { if (newton) kmanip_launch_step_10_16_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_10_16_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
  else { if (newton) kmanip_launch_step_20_32_1(dm, st, act, obs, reward, done, nchunk, epb, stream); else kmanip_launch_step_20_32_0(dm, st, act, obs, reward, done, nchunk, epb, stream); }
}
void kmanip_launch_reset(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const uint8_t* mask, double* obs,
                         int epb, hipStream_t stream) {
  const bool newton = hd.solver == KM_SOLVER_NEWTON;
  if (st.envp) {
    if (hd.nlink <= 10) { if (newton) kmanip_launch_reset_ep_10_16_1(dm, st, mask, obs, epb, stream); else kmanip_launch_reset_ep_10_16_0(dm, st, mask, obs, epb, stream); }
    else { if (newton) kmanip_launch_reset_ep_20_32_1(dm, st, mask, obs, epb, stream); else kmanip_launch_reset_ep_20_32_0(dm, st, mask, obs, epb, stream); }
    return;
  }
  if (hd.nlink <= 10) { if (newton) kmanip_launch_reset_10_16_1(dm, st, mask, obs, epb, stream); else kmanip_launch_reset_10_16_0(dm, st, mask, obs, epb, stream); }
  else { if (newton) kmanip_launch_reset_20_32_1(dm, st, mask, obs, epb, stream); else kmanip_launch_reset_20_32_0(dm, st, mask, obs, epb, stream); }
}
void kmanip_launch_observe(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, double* obs, double* reward,
                           hipStream_t stream) {
  if (hd.nlink <= 10) kmanip_launch_observe_10_16_1(dm, st, obs, reward, stream);
  else kmanip_launch_observe_20_32_1(dm, st, obs, reward, stream);
}
void kmanip_launch_forces(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KForcesDev& out, hipStream_t stream) {
  if (st.qfrc_applied && st.envp) { if (hd.nlink <= 10) kmanip_launch_forces_ep_frc_10_16(dm, st, out, stream); else kmanip_launch_forces_ep_frc_20_32(dm, st, out, stream); }
  else if (st.qfrc_applied) { if (hd.nlink <= 10) kmanip_launch_forces_frc_10_16(dm, st, out, stream); else kmanip_launch_forces_frc_20_32(dm, st, out, stream); }
  else if (st.envp) { if (hd.nlink <= 10) kmanip_launch_forces_ep_10_16(dm, st, out, stream); else kmanip_launch_forces_ep_20_32(dm, st, out, stream); }
  else { if (hd.nlink <= 10) kmanip_launch_forces_10_16(dm, st, out, stream); else kmanip_launch_forces_20_32(dm, st, out, stream); }
}
void kmanip_launch_kinematics(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KKinDev& out, hipStream_t stream) {
  if (st.envp) { if (hd.nlink <= 10) kmanip_launch_kinematics_ep_10_16(dm, st, out, stream); else kmanip_launch_kinematics_ep_20_32(dm, st, out, stream); }
  else { if (hd.nlink <= 10) kmanip_launch_kinematics_10_16(dm, st, out, stream); else kmanip_launch_kinematics_20_32(dm, st, out, stream); }
}
void kmanip_launch_inverse(const KDeviceModel* dm, const KModelDesc& hd, const KDeviceState& st, const KInverseIn& in, const KInverseDev& out,
                           hipStream_t stream) {
  if (st.envp) { if (hd.nlink <= 10) kmanip_launch_inverse_ep_10_16(dm, st, in, out, stream); else kmanip_launch_inverse_ep_20_32(dm, st, in, out, stream); }
  else { if (hd.nlink <= 10) kmanip_launch_inverse_10_16(dm, st, in, out, stream); else kmanip_launch_inverse_20_32(dm, st, in, out, stream); }
}
void kmanip_launch_prepare_model(KDeviceModel* dm, const KModelDesc& hd, hipStream_t stream) {
  if (hd.nlink <= 10) kmanip_launch_prepare_10_16_1(dm, stream);
  else kmanip_launch_prepare_20_32_1(dm, stream);
}
