"""Reference adjoint of the batched OSC solve with respect to the per-env parameters, for
tests/test_backward_env_ref.py (CPU) and tests/test_gpu_backward_env.py (GPU): dL/dmu, dL/du_lb,
dL/du_ub, dL/dfz_lb, dL/dfz_ub, dL/dw_pos, dL/dw_rot and the six data outputs of
tests/backward_data_ref.py, of a loss L(x) at the oracle's optimum of tests/env_params_cases.py's
batch, every env on its own model (include/osc_backward_env.h).

With the working set fixed the adjoint system [[H, A_W'], [A_W, 0]] [dx; dnu] = [-gx; 0] gives
(Amos & Kolter, OptNet) dL/db_W = -dnu and dL/dA = dnu x*' + nu* dx', chained to the fields:
  a torque box row       b_W = u_ub[j] (multiplier > 0) or u_lb[j]
  an fz box row          b_W = fz_ub mask_c (multiplier > 0) or fz_lb mask_c; the fz_lb convention:
                         with fz_lb mask_c == 0 the row contributes exactly 0 (the left derivative
                         at the pyramid's apex)
  a pyramid row          A[r][fz_c] = -mu
  w_pos[s], w_rot[s]     the ordered sums of their three rows of the row-weight gradient

  reference_adjoint_env  the dense full-space KKT solve, keeping dnu
  kernel_model_env       numpy model of the library's formulation (csrc/osc_backward_env.hip): rho
                         from w and v, the Gram-Schmidt's kept rows, the <= 3 x 3 solve
  directional_fd_env     central (or one-sided) differences of the oracle's own optimum along a
                         direction of one field
"""
import functools

import numpy as np

import backward_data_ref as bd
import backward_ref as br
import env_params_cases as ec
from osc_qp import b_matrix, build_qp, contact_jacobian, task_weights
from qp_exact import _kkt_solve, certified, solve_exact

NENV = ec.NENV
ROBOTS = ec.ROBOTS
FIELDS = ec.FIELDS
OUTPUTS = bd.OUTPUTS
PYRAMID = ((1, 1), (-1, 1), (1, -1), (-1, -1))


def grad_seed(robot: str, tau_only: bool = False) -> np.ndarray:
    """gx = dL/dx of every env: random over all of x, or on the torque block alone."""
    mdl = ec.env_model(robot, ec.params(robot), 0)
    g = np.random.default_rng(9191 + ROBOTS.index(robot)).standard_normal((NENV, mdl.n))
    if tau_only:
        g[:, :mdl.nv] = 0.0
        g[:, mdl.nv + mdl.nu:] = 0.0
    return g


def site_sums(mdl, gw: np.ndarray):
    """(dL/dw_pos [ns], dL/dw_rot [ns]): the three rows of each site, added in order."""
    ns = mdl.ns
    pos = np.array([(gw[3 * s] + gw[3 * s + 1]) + gw[3 * s + 2] for s in range(ns)])
    rot = np.array([(gw[3 * ns + 3 * s] + gw[3 * ns + 3 * s + 1]) + gw[3 * ns + 3 * s + 2]
                    for s in range(ns)])
    return pos, rot


def reference_adjoint_env(mdl, M, C, J, b, T, mask, gx, x, y):
    """dict of the seven parameter gradients and the six data outputs at the optimum x with duals
    y of the env's own model `mdl`, by the dense KKT solve on the working set of y."""
    nv, nu, nc, n = mdl.nv, mdl.nu, mdl.nc, mdl.n
    out = bd.reference_adjoint_data(mdl, M, C, J, b, T, mask, gx, x, y)
    qp = build_qp(mdl, M, C, J, b, T, mask)
    rows = br.working_rows(qp, y)
    AW = qp.A[rows]
    k = AW.shape[0]
    K = np.zeros((n + k, n + k))
    K[:n, :n], K[:n, n:], K[n:, :n] = qp.H, AW.T, AW
    rhs = np.concatenate([-np.asarray(gx, float), np.zeros(k)])
    sol = _kkt_solve(K, rhs)
    Kl, rhsl, soll = K.astype(np.longdouble), rhs.astype(np.longdouble), sol.astype(np.longdouble)
    for _ in range(br.KKT_REFINE):
        soll = soll + _kkt_solve(K, (rhsl - Kl @ soll).astype(np.float64)).astype(np.longdouble)
    sol = soll.astype(np.float64)
    dx, dnu = sol[:n], sol[n:]
    x, y, mask = np.asarray(x, float), np.asarray(y, float), np.asarray(mask, float)
    g = dict(mu=0.0, u_lb=np.zeros(nu), u_ub=np.zeros(nu), fz_lb=0.0, fz_ub=0.0)
    box0 = nv + 4 * nc                      # the first row of I_n
    for p, i in enumerate(rows):
        if i < nv:
            continue
        if i < box0:                        # pyramid row of contact c: A[i][fz_c] = -mu
            fz = nv + nu + 3 * ((i - nv) // 4) + 2
            g["mu"] += -(dnu[p] * x[fz] + y[i] * dx[fz])
            continue
        j = i - box0 - nv                   # a bound on (u, z)[j]
        assert j >= 0
        if j < nu:
            g["u_ub" if y[i] > 0.0 else "u_lb"][j] += -dnu[p]
        elif (j - nu) % 3 == 2:
            m = mask[(j - nu) // 3]
            if m == 0.0:                    # (z = 0 rows of an unloaded contact: no parameter)
                continue
            if y[i] > 0.0:
                g["fz_ub"] += -dnu[p] * m
            elif mdl.z_lb[2] * m != 0.0:    # the fz_lb convention
                g["fz_lb"] += -dnu[p] * m
    g["w_pos"], g["w_rot"] = site_sums(mdl, out["wrow"])
    out.update(g)
    return out


@functools.lru_cache(maxsize=None)
def reference_env(robot: str, tau_only: bool = False) -> dict:
    """name -> [NENV][...] of the batch at the oracle's optimum (computed once, read-only)."""
    d, p = ec.inputs(robot), ec.params(robot)
    xs, ys = ec.oracle(robot)
    g = grad_seed(robot, tau_only)
    out = [reference_adjoint_env(ec.env_model(robot, p, e), *br.env_args(d, e), g[e], xs[e], ys[e])
           for e in range(NENV)]
    ref = {k: np.array([o[k] for o in out]) for k in FIELDS + OUTPUTS}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def kernel_model_env(mdl, M, C, J, b, T, mask, gx, x, y, refine: int = 1):
    """numpy model of osc_batch_solve_backward_env's parameter gradients: w with `refine` steps,
    rho = X_y'(H_dv (X_y w)) + D w - r~, per torque row -rho_j by the multiplier's sign, per
    contact the Gram-Schmidt's kept rows G and G' dnu = rho_c (least squares on <= 3 rows)."""
    nv, nu, nc, ny, s = mdl.nv, mdl.nu, mdl.nc, mdl.nu + 3 * mdl.nc, mdl.s
    M = np.asarray(M, float).reshape(nv, nv)
    J = np.asarray(J, float).reshape(s, nv)
    x, y, mask, gx = (np.asarray(a, float) for a in (x, y, mask, gx))
    Wd = task_weights(mdl)
    Xy = np.linalg.solve(M, np.hstack([b_matrix(mdl), contact_jacobian(mdl, J)]))
    Hd = 2.0 * (J.T * Wd) @ J + 2.0 * mdl.w_reg * np.eye(nv)
    D = np.concatenate([np.full(nu, 2.0 * (mdl.w_torque + mdl.w_reg)), np.full(3 * nc, 2.0 * mdl.w_reg)])
    Hr = Xy.T @ Hd @ Xy + np.diag(D)
    tq, normals = br.active_set(mdl, mask, y)
    P = np.zeros((ny, ny))
    P[:nu, :nu] = np.diag(np.where(tq, 0.0, 1.0))
    for k in range(nc):
        c = nu + 3 * k
        P[c:c + 3, c:c + 3] = br.contact_projector(normals[k])
    rt = gx[nv:] + Xy.T @ gx[:nv]
    r = P @ rt
    L = np.linalg.cholesky(P @ Hr @ P + (np.eye(ny) - P))
    solve = lambda a: P @ np.linalg.solve(L.T, np.linalg.solve(L, P @ a))
    w = solve(r)
    for _ in range(refine):
        w = w + solve(r - (Xy.T @ (Hd @ (Xy @ w)) + D * w))
    rho = Xy.T @ (Hd @ (Xy @ w)) + D * w - rt
    pyr = y[nv:nv + 4 * nc].reshape(nc, 4)
    box = y[nv + 4 * nc:]
    yu, yz = box[nv:nv + nu], box[nv + nu:].reshape(nc, 3)
    g = dict(mu=0.0, u_lb=np.zeros(nu), u_ub=np.zeros(nu), fz_lb=0.0, fz_ub=0.0)
    thr = mdl.infinity / 1e10
    for j in range(nu):
        if tq[j]:
            if yu[j] > 0.0:
                g["u_ub"][j] = -rho[j] if abs(mdl.u_ub[j]) < thr else 0.0
            else:
                g["u_lb"][j] = -rho[j] if abs(mdl.u_lb[j]) < thr else 0.0
    for c in range(nc):
        if mask[c] == 0.0:
            continue
        cand = [(np.array([sx, sy, -mdl.mu]), ("pyr", r)) for r, (sx, sy) in enumerate(PYRAMID)
                if pyr[c, r] > 0.0]
        cand += [(np.eye(3)[a], ("box", a)) for a in range(3) if yz[c, a] != 0.0]
        Q, kept = [], []
        for a, tag in cand:                 # backward_ref.contact_projector's Gram-Schmidt
            u = a.copy()
            for _ in range(2):
                for q in Q:
                    u = u - (q @ u) * q
            if len(Q) < 3 and u @ u > 1e-12 * (a @ a):
                Q.append(u / np.sqrt(u @ u))
                kept.append((a, tag))
        if not kept:
            continue
        G = np.array([a for a, _ in kept])
        dn = np.linalg.lstsq(G.T, rho[nu + 3 * c:nu + 3 * c + 3], rcond=None)[0]
        fzs, wfz = x[nv + nu + 3 * c + 2], w[nu + 3 * c + 2]
        for (a, (kind, r)), dnr in zip(kept, dn):
            if kind == "pyr":
                g["mu"] += -dnr * fzs + pyr[c, r] * wfz
            elif r == 2:
                if yz[c, 2] > 0.0:
                    g["fz_ub"] += -dnr * mask[c]
                elif mdl.z_lb[2] * mask[c] != 0.0:
                    g["fz_lb"] += -dnr * mask[c]
    return g


def perturbed(p: dict, e: int, field: str, delta) -> dict:
    """p with env e's `field` moved by delta (a scalar or an array of the field's row shape)."""
    a = p[field].copy()
    a[e] = a[e] + delta
    return dict(p, **{field: a})


def loss_at(robot: str, d: dict, p: dict, e: int, gx):
    """(gx . x*, working set, qp) of env e's oracle optimum under the parameters p."""
    mdl = ec.env_model(robot, p, e)
    args = br.env_args(d, e)
    qp = build_qp(mdl, *args)
    sol = solve_exact(mdl, qp, *args[:3])
    assert certified(sol.cert, 1e-8), sol.cert
    return float(gx @ sol.x), frozenset(br.working_rows(qp, sol.y)), qp


def directional_fd_env(robot: str, d: dict, p: dict, e: int, gx, field: str, direction, h):
    """((L(theta + h d) - L(theta - h d)) / 2h, working sets at + and -) along `direction` of env
    e's `field`: the oracle differentiated by itself."""
    lp, wp, _ = loss_at(robot, d, perturbed(p, e, field, h * direction), e, gx)
    lm, wm, _ = loss_at(robot, d, perturbed(p, e, field, -h * direction), e, gx)
    return (lp - lm) / (2.0 * h), wp, wm
