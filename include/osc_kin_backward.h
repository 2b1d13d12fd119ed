/*
 * osc_kin_backward.h -- backward pass of the kinematics front end: the vector-Jacobian product of
 * osc_batch_kinematics(_env) (osc_kinematics.h, osc_kin_env_params.h) with respect to qpos, qvel
 * and the per-env inertial parameters.  Together with osc_batch_solve_backward_data (osc_backward.h)
 * or osc_batch_solve_backward_env (osc_backward_env.h), which give dL/dM, dL/dC, dL/dJ and dL/db,
 * the chain  qpos, qvel (, mass_scale, com_offset, armature_scale) -> M, C, J, b, site_xpos ->
 * x, tau -> loss  is differentiable end to end in two backward launches.  Part of
 * libosc_batch.so; same return codes as osc_batch.h; additive to ABI 4.  All array pointers are
 * DEVICE pointers, fp64, env-major, 8-byte aligned; `stream` is a hipStream_t (NULL = default).
 */
#ifndef OSC_KIN_BACKWARD_H_
#define OSC_KIN_BACKWARD_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"
#include "osc_kin_env_params.h"
#include "osc_kinematics.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gradient outputs with respect to the per-env parameters, each nullable (= not computed):
 * mass_scale [nenv][nbody], com_offset [nenv][nbody][3], armature_scale [nenv][nv]. */
typedef struct {
  double* mass_scale;
  double* com_offset;
  double* armature_scale;
} osc_kin_env_grads;

/* The VJP of exactly what osc_batch_kinematics(_env) computes, in the layouts of osc_kinematics.h.
 *   qpos, qvel     [nenv][nq], [nenv][nv]: the forward call's inputs
 *   kin_params     nullable: the forward call's block (NULL fields = the model's values)
 *   grad_M [nenv][nv][nv], grad_C [nenv][nv], grad_J [nenv][6 ns][nv], grad_b [nenv][6 ns],
 *   grad_site_xpos [nenv][ns][3]: the cotangents, each nullable = zero.  All nv^2 entries of
 *                  grad_M are independent, as in osc_backward.h; the kernel forms M_ij and M_ji
 *                  from one product, so both cotangents feed it
 *   grad_qpos      [nenv][nq], nullable: with respect to the raw nq coordinates.  A free or ball
 *                  quaternion is differentiated through the kernel's own normalisation, so its four
 *                  components are orthogonal to q
 *   grad_qvel      [nenv][nv], nullable
 *   kin_grads      nullable.  A parameter gradient is with respect to the per-env array entry;
 *                  asking for the gradient of a field whose forward pointer is NULL is allowed and
 *                  is the derivative at the identity (scale 1, offset 0)
 * Stateless: no workspace; the kernel recomputes the forward from qpos, qvel and the parameters.
 * Asynchronous on `stream`; never synchronises.  No atomics: an env's gradients are bitwise
 * reproducible and do not depend on the batch around it.  A NULL output is not computed and
 * leaves the others bitwise unchanged.  An env that osc_kin_env_params.h calls invalid (a NaN or
 * non-finite parameter, a mass_scale <= 0, an armature_scale < 0) gets zeros in every gradient
 * output; every other env is bitwise unaffected.  Every joint type and every tree the forward
 * accepts is supported, up to OSC_KIN_MAX_BODIES / DOFS / SITES.
 * OSC_ERR_INVALID_ARGUMENT, all checked before any launch: a NULL kin, nenv < 0, a NULL qpos or
 * qvel, any pointer that is not 8-byte aligned, every output NULL.  nenv == 0 is OSC_OK. */
int osc_batch_kinematics_backward(const osc_kin_model* kin, int32_t nenv, const double* qpos,
                                  const double* qvel, const osc_kin_env_params* kin_params,
                                  const double* grad_M, const double* grad_C, const double* grad_J,
                                  const double* grad_b, const double* grad_site_xpos,
                                  double* grad_qpos, double* grad_qvel,
                                  const osc_kin_env_grads* kin_grads, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_KIN_BACKWARD_H_ */
