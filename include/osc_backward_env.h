/*
 * osc_backward_env.h -- backward pass of the batched OSC solve with per-environment parameters
 * (osc_env_params.h): the gradients of osc_backward.h's second entry with the env's own friction
 * and task weights read where the model's were, and dL/dtheta for the seven per-env fields -- mu,
 * the torque box u_lb / u_ub, the normal-force bounds fz_lb / fz_ub and the task weights w_pos /
 * w_rot.  Part of libosc_batch.so; same return codes as osc_batch.h; additive to ABI 4 (every
 * existing entry point is unchanged).
 *
 * Notation of osc_backward.h: y' = (u, z), w = -dx_(u,z), v = X_y w = -dx_dv, r~ = (g_u, g_z) +
 * X_y' g_dv before the projection, D = diag(2 (w_torque + w_reg) on u, 2 w_reg on z).  The (u, z)
 * block of the adjoint system's first block row, with the equality adjoint dnu = -M^-1 (g_dv -
 * H_dv v) substituted, leaves the stacked adjoint multipliers of the active box and pyramid rows
 *   G' dnu_G = rho,   rho = X_y'(H_dv v) + D w - r~        (P rho = 0 up to rounding)
 * -- the refinement step's own product with the final w and without the projector; no solve with
 * M.  With nu the forward duals, z* and fz* from x, and dL/db_W = -dnu, dL/dA = dnu x*' + nu dx':
 *   torque row j, active by osc_backward.h's rule: dL/du_ub[j] = -rho_j if its multiplier is > 0,
 *     otherwise dL/du_lb[j] = -rho_j; an inactive row or an absent bound (|v| >= infinity / 1e10)
 *     gets exactly 0
 *   contact c with mask != 0: G = the active rows the Gram-Schmidt of the projector keeps, in its
 *     order (the four pyramid rows, then the fx, fy, fz box rows; at most three, independent);
 *     G' dnu = rho_c, a dropped row has dnu = 0;
 *       dL/dmu    += sum over kept pyramid rows r of (-dnu_r fz*_c + nu_r w_fz,c)
 *       dL/dfz_ub += -dnu_fz mask_c   if the fz multiplier is > 0
 *       dL/dfz_lb += -dnu_fz mask_c   if the fz multiplier is < 0 and fz_lb mask_c != 0
 *     a contact with mask == 0 contributes nothing; the sums run over the contacts in order
 *   dL/dw_pos[s] = grad_wrow[3 s] + grad_wrow[3 s + 1] + grad_wrow[3 s + 2], added in that order;
 *     dL/dw_rot[s] likewise from row 3 ns + 3 s.
 *
 * The fz_lb convention.  With fz_lb mask_c == 0 an active lower row means fz* = 0: the contact
 * sits at the pyramid's apex, where five rows are active on three forces and the multipliers are
 * not unique.  x* is not differentiable in fz_lb there -- lowering the bound moves nothing (the
 * pyramid alone holds fz >= 0), raising it moves the optimum -- and the library returns the LEFT
 * derivative, 0; the right derivative is out of scope.  dL/dmu needs no rule: at the apex fz* = 0
 * and w_fz = 0, so every term vanishes.
 */
#ifndef OSC_BACKWARD_ENV_H_
#define OSC_BACKWARD_ENV_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"
#include "osc_env_params.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All DEVICE pointers, fp64, env-major, shapes as osc_env_params.  Each field is nullable: NULL =
 * not computed. */
typedef struct {
  double* mu;     /* [nenv]      */
  double* u_lb;   /* [nenv][nu]  */
  double* u_ub;   /* [nenv][nu]  */
  double* fz_lb;  /* [nenv]      */
  double* fz_ub;  /* [nenv]      */
  double* w_pos;  /* [nenv][ns]  */
  double* w_rot;  /* [nenv][ns]  */
} osc_env_grads;

/* After osc_batch_solve_env or osc_batch_solve_warm_env with x and duals, on the same model, batch,
 * workspace and env_params; or after osc_batch_solve_ex or its warm twin, with env_params NULL --
 * the parameter gradients are then those of the model's constants, taken env by env.
 *   env_params   the forward call's block; NULL, or a NULL field, = the model's value
 *   grads        nullable; each field nullable
 *   everything else as osc_batch_solve_backward_data (osc_backward.h)
 * Asynchronous on `stream`; never synchronises.  No atomics: an env's outputs are bitwise
 * independent of its batch.  An env whose status is not OSC_SOLVE_OK -- one the forward call marked
 * invalid included -- gets zeros in every output.  A NULL output is not computed and leaves the
 * others bitwise unchanged; with only mu and bound gradients asked for, the factorisation of M and
 * the pass over J are skipped.  With env_params NULL, every field NULL, or a block filled with the
 * model's constants, the six data outputs are bitwise those of osc_batch_solve_backward_data.
 * OSC_ERR_INVALID_ARGUMENT, all checked before any launch: whatever osc_batch_solve_backward_data
 * refuses; a model with wheel rows; a model created with refine_steps = 0; a parameter or gradient
 * pointer that is not 8-byte aligned.  nenv == 0 is OSC_OK. */
int osc_batch_solve_backward_env(const osc_model* model, int32_t nenv, const double* M,
                                 const double* J, const double* b, const double* T,
                                 const double* contact_mask, const osc_env_params* env_params,
                                 const double* x, const double* y, const int32_t* status,
                                 const double* grad_x, double* grad_M, double* grad_C,
                                 double* grad_J, double* grad_wrow, double* grad_T,
                                 double* grad_b, const osc_env_grads* grads,
                                 const void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_BACKWARD_ENV_H_ */
