/*
 * osc_backward.h -- backward pass of the batched OSC solve: gradients of a loss L(x) with respect
 * to the task targets T and the task bias b.  Part of libosc_batch.so; same return codes as
 * osc_batch.h.  All array pointers are DEVICE pointers, env-major, fp64 unless noted; `stream` is
 * a hipStream_t (NULL = default).
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
 * OSC_SOLVE_OK gets all-zero gradients.  Gradients with respect to M, C, J, the weights or the
 * bounds are not provided.
 * OSC_ERR_INVALID_ARGUMENT: a NULL model, nenv < 0, a model with wheel rows, a NULL or misaligned
 * array, a workspace smaller than osc_workspace_bytes -- all checked before any launch.
 * nenv == 0 is OSC_OK. */
int osc_batch_solve_backward(const osc_model* model, int32_t nenv, const double* J,
                             const double* contact_mask, const double* y, const int32_t* status,
                             const double* grad_x, double* grad_T, double* grad_b,
                             const void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_BACKWARD_H_ */
