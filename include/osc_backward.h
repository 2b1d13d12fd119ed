/*
 * osc_backward.h -- backward pass of the batched OSC solve: gradients of a loss L(x) with respect
 * to the task targets T and the task bias b (osc_batch_solve_backward), and with respect to the
 * dynamics inputs M, C, J and the task-row weights as well (osc_batch_solve_backward_data).  Part
 * of libosc_batch.so; same return codes as osc_batch.h.  All array pointers are DEVICE pointers,
 * env-major, fp64 unless noted; `stream` is a hipStream_t (NULL = default).
 *
 * At the optimum the active set is known, so x* = (dv, u, z) is locally an affine function of
 * f_dv = 2 J'W (b - t), the only part of the QP that T and b enter.  With y' = (u, z),
 * dv = X_y y' + X_c and the reduced Hessian Hr the forward call leaves in its workspace, the
 * vector-Jacobian product of gx = dL/dx is one equality-constrained solve per env:
 *   r = (g_u, g_z) + X_y' g_dv
 *   w = argmin 1/2 w'Hr w - r'w  over  null(G_A)        (G_A: the active rows)
 *   v = X_y w,  q = 2 W (J v),  dL/db = -q,  dL/dT = +q  (T[s][0:3] <-> task rows 3s..3s+2,
 *                                                         T[s][3:6] <-> rows 3 ns + 3s..)
 * solved as w = P K^-1 P r with P the orthogonal projector onto null(G_A) and
 * K = P Hr P + (I - P), positive definite whatever rows are active (a contact at the pyramid apex
 * has five active rows on three forces), plus one refinement step whose residual goes through the
 * factored form X_y'(H_dv (X_y w)) + D w, never through Hr.
 *
 * The active set is read off the dual solution of the forward call (osc_solve_extras.y, rows
 * [Aeq; Aineq; I_n]): a pyramid row is active iff its multiplier is > 0; an fz box row iff its
 * multiplier is != 0; a contact with mask == 0 has all three forces fixed; a torque box row iff
 * its |multiplier| is above 1e-6 x (1 + the env's largest multiplier of a one-sided row) -- the
 * torque-box duals are recovered from stationarity and carry rounding residues on inactive rows.
 * No primal slack is consulted: a weakly active row (zero multiplier) stays out.
 *
 * The dynamics inputs enter H_dv = 2 J'WJ + 2 w_reg I, f_dv = 2 J'W (b - t) and the equality rows
 * [M, -B, -Jc'] (dv, u, z) = -C.  With the working set fixed the adjoint system
 * [[H, A_W'], [A_W, 0]] [dx; dnu] = [-gx; 0] has dx_(u,z) = -w and dx_dv = -v, and since no
 * inequality or bound row touches dv its first block row gives the equality rows' adjoint with one
 * more solve with M:
 *   dnu = -M^-1 (g_dv - H_dv v)
 * and, with dv*, u*, z* from x, nu = y[0:nv] (H x + f + A'y = 0) and e = J dv* + b - t:
 *   dL/dC       = dnu
 *   dL/dM[i][k] = dnu_i dv*_k - nu_i v_k        (all nv^2 entries independent, not symmetrised)
 *   dL/dJ[r][:] = -2 W_r ((J v)_r dv*' + e_r v')   every task row r,
 *                 - z*_j dnu' + w_z,j nu'          added on contact row j (row 3 ns - 3 nc + j)
 *   dL/dw_row[r] = -2 (J v)_r e_r               (a site's w_pos / w_rot gradient: its rows' sum)
 * The bounds, the pyramid and the mask are not functions of M, C, J or W: the active-set rule is
 * the one above, and the non-unique multipliers of a contact at the pyramid apex never enter.
 */
#ifndef OSC_BACKWARD_H_
#define OSC_BACKWARD_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dL/dT and dL/db of every env from dL/dx, after osc_batch_solve_ex (or its warm twin) with x and
 * duals on the same model, batch and workspace.
 *   J, contact_mask  the forward call's inputs, [nenv][6 ns][nv] and [nenv][nc] (16-byte aligned)
 *   y                [nenv][osc_dual_rows] the forward call's duals
 *   status           [nenv] int32 the forward call's statuses
 *   grad_x           [nenv][nv + nu + 3 nc] dL/dx over the whole design vector (dv, u, z)
 *   grad_T           [nenv][ns][6], nullable
 *   grad_b           [nenv][6 ns], nullable; grad_b == -grad_T re-laid out, exactly
 *   workspace        the forward call's workspace (osc_workspace_bytes), read only: it must still
 *                    hold that call's reduced QPs
 * Asynchronous on `stream`; never synchronises.  No atomics: an env's gradients are bitwise
 * reproducible and do not depend on the batch it sits in.  An env whose status is not
 * OSC_SOLVE_OK gets all-zero gradients.  Gradients with respect to M, C, J and the weights:
 * osc_batch_solve_backward_data below.
 * OSC_ERR_INVALID_ARGUMENT: a NULL model, nenv < 0, a model with wheel rows, a NULL or misaligned
 * array, a workspace smaller than osc_workspace_bytes -- all checked before any launch.
 * nenv == 0 is OSC_OK. */
int osc_batch_solve_backward(const osc_model* model, int32_t nenv, const double* J,
                             const double* contact_mask, const double* y, const int32_t* status,
                             const double* grad_x, double* grad_T, double* grad_b,
                             const void* workspace, size_t workspace_bytes, void* stream);

/* The same, with the gradients of the dynamics inputs: after osc_batch_solve_ex (or its warm twin)
 * with x and duals on the same model, batch and workspace.
 *   M, J, b, T, contact_mask  the forward call's inputs (M, J and the mask 16-byte aligned)
 *   x, y, status              the forward call's design vectors [nenv][nv + nu + 3 nc], duals
 *                             [nenv][osc_dual_rows] and statuses
 *   grad_x                    [nenv][nv + nu + 3 nc] dL/dx
 *   grad_M [nenv][nv][nv], grad_C [nenv][nv], grad_J [nenv][6 ns][nv]   (16-byte aligned),
 *   grad_wrow [nenv][6 ns] (task rows in W's order: w_pos of every site x 3, then w_rot x 3),
 *   grad_T [nenv][ns][6], grad_b [nenv][6 ns]: every one nullable; a NULL output is not computed
 *   and leaves the others bitwise unchanged
 *   workspace                 the forward call's workspace, read only
 * grad_T and grad_b are bitwise those of osc_batch_solve_backward.  Asynchronous on `stream`, no
 * atomics, an env's outputs bitwise independent of its batch; an env whose status is not
 * OSC_SOLVE_OK gets zeros in every output.  Argument rules and return codes as
 * osc_batch_solve_backward (a model with wheel rows is refused; all checks before any launch;
 * nenv == 0 is OSC_OK).  Gradients with respect to the bounds, mu and the site weights, and the
 * backward pass of a batch solved with per-env parameters (osc_env_params.h):
 * osc_batch_solve_backward_env, osc_backward_env.h.  From joint states, the kinematics' own backward
 * pass (osc_batch_kinematics_backward, osc_kin_backward.h) takes grad_M, grad_C, grad_J and grad_b
 * on to qpos, qvel and the per-env inertial parameters.  Backward passes of the multi, host-fed
 * and wheel-row entries remain out of scope. */
int osc_batch_solve_backward_data(const osc_model* model, int32_t nenv, const double* M,
                                  const double* J, const double* b, const double* T,
                                  const double* contact_mask, const double* x, const double* y,
                                  const int32_t* status, const double* grad_x, double* grad_M,
                                  double* grad_C, double* grad_J, double* grad_wrow,
                                  double* grad_T, double* grad_b, const void* workspace,
                                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_BACKWARD_H_ */
