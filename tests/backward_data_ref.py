"""Reference adjoint of the batched OSC solve with respect to its dynamics inputs, for
tests/test_backward_data_ref.py (CPU) and tests/test_gpu_backward_data.py (GPU): dL/dM, dL/dC,
dL/dJ, the per-row weight gradient dL/dw_row, and dL/dT, dL/db, of a loss L(x) at the oracle's
optimum (include/osc_backward.h, osc_batch_solve_backward_data).

With the working set fixed, the adjoint of  min 1/2 x'Hx + f'x  s.t.  A_W x = b_W  solves
[[H, A_W'], [A_W, 0]] [dx; dnu] = [-gx; 0]  and gives (Amos & Kolter, OptNet)
    dL/dH = 1/2 (dx x*' + x* dx'),  dL/df = dx,  dL/dA = dnu x*' + nu* dx',  dL/db_W = -dnu
with nu* the forward duals in the convention H x + f + A'y = 0.

  reference_adjoint_data  the dense full-space KKT solve of backward_ref.reference_adjoint, keeping
                          dnu, then the formulas above on the FULL H and A, chained through
                          oracle/osc_qp.build_qp to M, C, J and the row weights: no reduced space
  projector_adjoint_data  numpy model of the library's formulation (csrc/osc_backward_data.hip):
                          w and v = X_y w from the projected reduced-Hessian solve, one factored
                          solve with M for the equality adjoint, rank-one products
  directional_fd_data     central differences of the oracle's own optimum along a direction of
                          C, of J, of M (a symmetric direction) or of one site's w_pos, with the
                          working sets the oracle found at theta +- h
"""
import dataclasses
import functools

import numpy as np

import backward_ref as br
from backward_ref import (NENV, active_set, contact_projector, env_args, grad_seed, inputs,
                          model_of, oracle, relayout_T, working_rows)
from osc_qp import (b_matrix, build_qp, contact_jacobian, task_targets_vector, task_weights)
from qp_exact import _kkt_solve, certified, solve_exact

OUTPUTS = ("M", "C", "J", "wrow", "T", "b")


def reference_adjoint_data(mdl, M, C, J, b, T, mask, gx, x, y):
    """dict of the six gradients (M [nv][nv], C [nv], J [6 ns][nv], wrow [6 ns], T [ns][6],
    b [6 ns]) at the optimum x with duals y, by the dense KKT solve on the working set of y."""
    nv, nu, n, s = mdl.nv, mdl.nu, mdl.n, mdl.s
    qp = build_qp(mdl, M, C, J, b, T, mask)
    rows = working_rows(qp, y)
    assert rows[:nv] == list(range(nv))          # the dynamics rows lead the working set
    AW = qp.A[rows]
    k = AW.shape[0]
    K = np.zeros((n + k, n + k))
    K[:n, :n] = qp.H
    K[:n, n:] = AW.T
    K[n:, :n] = AW
    rhs = np.concatenate([-np.asarray(gx, float), np.zeros(k)])
    sol = _kkt_solve(K, rhs)
    Kl, rhsl, soll = K.astype(np.longdouble), rhs.astype(np.longdouble), sol.astype(np.longdouble)
    for _ in range(br.KKT_REFINE):
        soll = soll + _kkt_solve(K, (rhsl - Kl @ soll).astype(np.float64)).astype(np.longdouble)
    sol = soll.astype(np.float64)
    dx, dnu = sol[:n], sol[n:]
    x, nus = np.asarray(x, float), np.asarray(y, float)[rows]
    # OptNet, full space
    gH = 0.5 * (np.outer(dx, x) + np.outer(x, dx))
    gf = dx
    gA = np.outer(dnu, x) + np.outer(nus, dx)    # rows of the working set
    gbw = -dnu
    # chain rule through build_qp: only H_dv, f_dv and the dynamics rows [M, -B, -Jc], -C move
    J = np.asarray(J, float).reshape(s, nv)
    Wd = task_weights(mdl)
    bt = np.asarray(b, float).reshape(s) - task_targets_vector(mdl, T)
    G = gH[:nv, :nv]
    gJ = 2.0 * Wd[:, None] * (J @ (G + G.T)) + 2.0 * (Wd * bt)[:, None] * gf[None, :nv]
    r0 = 3 * mdl.ns - mdl.nz
    gJ[r0:r0 + mdl.nz] -= gA[:nv, nv + nu:].T    # Aeq's z block is -Jc = -J[r0:r0 + 3 nc]'
    gw = 2.0 * np.einsum("ri,ij,rj->r", J, G, J) + 2.0 * (J @ gf[:nv]) * bt
    gb = 2.0 * Wd * (J @ gf[:nv])
    return dict(M=gA[:nv, :nv].copy(), C=-gbw[:nv], J=gJ, wrow=gw, T=relayout_T(mdl, -gb), b=gb)


@functools.lru_cache(maxsize=None)
def reference_data(batch: str, robot: str, tau_only: bool = False) -> dict:
    """name -> [NENV][...] gradients of the batch at the oracle's optimum (computed once,
    read-only)."""
    mdl, d = model_of(batch, robot), inputs(batch, robot)
    xs, ys = oracle(batch, robot)
    g = grad_seed(batch, robot, tau_only)
    out = [reference_adjoint_data(mdl, *env_args(d, e), g[e], xs[e], ys[e]) for e in range(NENV)]
    ref = {k: np.array([o[k] for o in out]) for k in OUTPUTS}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def projector_adjoint_data(mdl, M, C, J, b, T, mask, gx, x, y, refine: int = 1,
                           refine_m: int = 0):
    """numpy model of osc_batch_solve_backward_data: the first entry's w (reduced coordinates,
    projector onto the active rows' null space, `refine` steps), v = X_y w, then
      dnu = -M^-1 (g_dv - H_dv v)   by a Cholesky solve (+ refine_m refinement steps)
    and the products of DESIGN.md §3.5."""
    nv, nu, nc, ny, s = mdl.nv, mdl.nu, mdl.nc, mdl.nu + 3 * mdl.nc, mdl.s
    M = np.asarray(M, float).reshape(nv, nv)
    J = np.asarray(J, float).reshape(s, nv)
    Wd = task_weights(mdl)
    Xy = np.linalg.solve(M, np.hstack([b_matrix(mdl), contact_jacobian(mdl, J)]))
    Hd = 2.0 * (J.T * Wd) @ J + 2.0 * mdl.w_reg * np.eye(nv)
    D = np.concatenate([np.full(nu, 2.0 * (mdl.w_torque + mdl.w_reg)), np.full(3 * nc, 2.0 * mdl.w_reg)])
    Hr = Xy.T @ Hd @ Xy + np.diag(D)
    tq, normals = active_set(mdl, mask, y)
    P = np.zeros((ny, ny))
    P[:nu, :nu] = np.diag(np.where(tq, 0.0, 1.0))
    for k in range(nc):
        c = nu + 3 * k
        P[c:c + 3, c:c + 3] = contact_projector(normals[k])
    gx = np.asarray(gx, float)
    r = P @ (gx[nv:] + Xy.T @ gx[:nv])
    L = np.linalg.cholesky(P @ Hr @ P + (np.eye(ny) - P))
    solve = lambda a: P @ np.linalg.solve(L.T, np.linalg.solve(L, P @ a))
    w = solve(r)
    for _ in range(refine):
        w = w + solve(r - (Xy.T @ (Hd @ (Xy @ w)) + D * w))
    v = Xy @ w
    # the equality adjoint: one more solve with M
    LM = np.linalg.cholesky(M)
    msolve = lambda a: np.linalg.solve(LM.T, np.linalg.solve(LM, a))
    rhs = -(gx[:nv] - Hd @ v)
    dnu = msolve(rhs)
    for _ in range(refine_m):
        dnu = dnu + msolve(rhs - M @ dnu)
    x = np.asarray(x, float)
    dvs, zs, nu_ = x[:nv], x[nv + nu:], np.asarray(y, float)[:nv]
    Jv, e = J @ v, J @ dvs + np.asarray(b, float).reshape(s) - task_targets_vector(mdl, T)
    gJ = -2.0 * Wd[:, None] * (Jv[:, None] * dvs[None, :] + e[:, None] * v[None, :])
    r0 = 3 * mdl.ns - mdl.nz
    gJ[r0:r0 + mdl.nz] += -zs[:, None] * dnu[None, :] + w[nu:, None] * nu_[None, :]
    gb = -2.0 * Wd * Jv
    return dict(M=np.outer(dnu, dvs) - np.outer(nu_, v), C=dnu, J=gJ, wrow=-2.0 * Jv * e,
                T=relayout_T(mdl, -gb), b=gb)


def with_w_pos(mdl, site: int, value: float):
    w = mdl.w_pos.copy()
    w[site] = value
    return dataclasses.replace(mdl, w_pos=w)


def directional_fd_data(mdl, M, C, J, b, T, mask, gx, which, direction, h):
    """((L(theta + h d) - L(theta - h d)) / 2h, working sets at theta + h d and theta - h d) with
    L = gx . x*(theta): the oracle differentiated by itself.  which: "C", "J", "M" (direction an
    array of the input's shape, symmetric for M) or ("w_pos", site) (direction a scalar)."""
    def run(sign):
        m2, a = mdl, dict(M=np.asarray(M, float), C=np.asarray(C, float), J=np.asarray(J, float))
        if isinstance(which, tuple):
            m2 = with_w_pos(mdl, which[1], mdl.w_pos[which[1]] + sign * h * direction)
        else:
            a[which] = a[which] + sign * h * np.asarray(direction).reshape(a[which].shape)
        qp = build_qp(m2, a["M"], a["C"], a["J"], b, T, mask)
        sol = solve_exact(m2, qp, a["M"], a["C"], a["J"])
        assert certified(sol.cert, 1e-8), sol.cert
        return float(gx @ sol.x), frozenset(working_rows(qp, sol.y))
    (lp, wp), (lm, wm) = run(+1.0), run(-1.0)
    return (lp - lm) / (2.0 * h), wp, wm
