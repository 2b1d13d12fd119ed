"""CPU reference of the rollout's backward pass (include/osc_rollout_backward.h), float64, one
environment at a time, for tests/test_rollout_backward_ref.py (CPU) and
tests/test_gpu_rollout_backward.py (GPU):

  step / step_vjp      the semi-implicit Euler step in torch ops, written exactly as
                       csrc/osc_rollout.hip's quat_step and oracle/kinematics.py::integrate write
                       it, and its vector-Jacobian product by torch.autograd.  At a zero rotation
                       angle the increment is (1, r / 2): the forward's value, and the analytic
                       limit of the slope
  pd_targets / pd_vjp  oracle/producers.py::pd_base_targets in torch ops, and its VJP
  chain                K ticks of  oracle kinematics -> [PD] -> qp_exact.solve_exact -> step,  then
                       backwards tick by tick: backward_data_ref.reference_adjoint_data (or
                       backward_env_ref.reference_adjoint_env), kin_backward_ref.vjp, step_vjp and
                       pd_vjp.  At every (env, tick) it asserts what test_gpu_kin_backward's
                       chain_reference asserts: the optimum certified at 1e-8, every active
                       multiplier > 1e-4 (1 + max|y|), every inactive slack > 1e-6 (1 + |bound|)

TEST INFRASTRUCTURE ONLY.  It lives under tests/ because oracle/ is not to change."""
import numpy as np
import torch

import backward_data_ref as bd
import backward_env_ref as ber
import kin_backward_ref as kbr
import kin_env_ref as ker
import kinematics as kin
from osc_qp import build_qp
from qp_exact import _constraints, certified, solve_exact

F64 = torch.float64


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=F64, requires_grad=grad)


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz,
                        aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw])


def quat_step(q, wl):
    """normalise(q * exp(wl / 2)), as quat_step of csrc/osc_rollout.hip."""
    th = torch.sqrt((wl * wl).sum())
    if float(th.detach()) == 0.0:
        d = torch.cat([torch.ones(1, dtype=F64), 0.5 * wl])   # value (1, 0); slope 1/2: the limit
    else:
        d = torch.cat([torch.cos(0.5 * th).reshape(1), torch.sin(0.5 * th) * wl / th])
    p = quat_mul(q, d)
    return p / torch.sqrt((p * p).sum())


def step(km, qpos, qvel, qacc, dt):
    """(qpos', qvel') torch tensors: qvel' = qvel + dt qacc, qpos' = integratePos(qpos, qvel', dt)."""
    v = qvel + dt * qacc
    parts = []
    for j in km.joints:
        qa, da = j["qadr"], j["dadr"]
        if j["type"] == "free":
            parts.append(qpos[qa:qa + 3] + v[da:da + 3] * dt)
            parts.append(quat_step(qpos[qa + 3:qa + 7], v[da + 3:da + 6] * dt))
        elif j["type"] == "ball":
            parts.append(quat_step(qpos[qa:qa + 4], v[da:da + 3] * dt))
        else:
            parts.append(qpos[qa:qa + 1] + v[da:da + 1] * dt)
    return torch.cat(parts), v


def step_vjp(km, qpos, qvel, qacc, dt, gq_new, gv_new):
    """(grad_qpos, grad_qvel, grad_qacc), numpy, of one env's step."""
    q, v, a = _t(qpos, True), _t(qvel, True), _t(qacc, True)
    qn, vn = step(km, q, v, a, dt)
    loss = (qn * _t(gq_new)).sum() + (vn * _t(gv_new)).sum()
    g = torch.autograd.grad(loss, [q, v, a], allow_unused=True)
    return tuple(np.zeros_like(x.detach().numpy()) if y is None else y.numpy()
                 for x, y in zip((q, v, a), g))


def pd_targets(ns, pos, quat, lin, ang, pos_ref, quat_ref, gains):
    """(ns, 6) torch tensor: oracle/producers.py::pd_base_targets."""
    kp_l, kd_l, kp_a, kd_a = gains
    conj = torch.stack([quat[0], -quat[1], -quat[2], -quat[3]])
    rot = quat_mul(quat_ref, conj)[1:]
    row = torch.cat([kp_l * (pos_ref - pos) + kd_l * (0.0 - lin), kp_a * rot + kd_a * (0.0 - ang)])
    return torch.cat([row.reshape(1, 6), torch.zeros((ns - 1, 6), dtype=F64)])


def pd_vjp(ns, quat, pos_ref, quat_ref, gains, gT):
    """(grad_pos, grad_quat, grad_lin, grad_ang), numpy, of one env's producer call (it is linear
    in the state, so only the quaternion's reference enters)."""
    pos, lin, ang = (_t(np.zeros(3), True) for _ in range(3))
    q = _t(quat, True)
    T = pd_targets(ns, pos, q, lin, ang, _t(pos_ref), _t(quat_ref), gains)
    g = torch.autograd.grad((T * _t(gT)).sum(), [pos, q, lin, ang])
    return tuple(x.numpy() for x in g)


def assert_clean(qp, sol, where):
    """chain_reference's conditions of tests/test_gpu_kin_backward.py, at one (env, tick)."""
    assert certified(sol.cert, 1e-8), (where, sol.cert)
    ymax = 1 + np.abs(sol.y).max()
    act, slk = np.inf, np.inf
    for i, sign, bound in _constraints(qp)[1]:
        slack = bound - sign * (qp.A[i] @ sol.x)
        if sol.y[i] * sign > 0:      # this side of the row is in the working set
            assert abs(sol.y[i]) > 1e-4 * ymax, ("weakly active row", where, i, sol.y[i])
            act = min(act, abs(sol.y[i]) / ymax)
        elif sol.y[i] == 0:
            assert slack > 1e-6 * (1 + abs(bound)), ("weakly active row", where, i, slack)
            slk = min(slk, slack / (1 + abs(bound)))
    return act, slk


def chain(tree, mdl, qpos0, qvel0, mask, nticks, dt, cot, T=None, pd=None, kin_params=None,
          env=False, where=""):
    """One env: the forward rollout on the oracle and the gradient of
    sum(cot["qpos"] * qpos_hist) + sum(cot["qvel"] * qvel_hist) + sum(cot["tau"] * tau_hist).
      mdl          the env's own QP model (osc_qp.load_model, with its overrides)
      kin_params   None or dict of the env's own arrays (mass_scale [nbody], ...)
      env          True: the seven per-env parameter gradients too (backward_env_ref)
    Returns (grads, hist): grads = dict(qpos0, qvel0, T (held), the kin_params' fields, the seven
    env fields), summed over the ticks in the order K-1 .. 0; hist = dict(qpos, qvel, tau)."""
    assert (T is None) != (pd is None)
    m = kin.KinModel(tree)
    nv, nu = mdl.nv, mdl.nu
    p1 = None if kin_params is None else {k: np.asarray(v)[None] for k, v in kin_params.items()}
    qh, vh, th, ticks = [np.array(qpos0, float)], [np.array(qvel0, float)], [], []
    for t in range(nticks):
        q, v = qh[-1], vh[-1]
        if pd is not None:
            Tt = pd_targets(mdl.ns, _t(q[0:3]), _t(q[3:7]), _t(v[0:3]), _t(v[3:6]), _t(pd[0]),
                            _t(pd[1]), pd[2]).numpy()
        else:
            Tt = np.asarray(T, float)
        M, C, J, b = ker.kinematics(tree, p1, 0, q, v) if p1 is not None else \
            kin.kinematics(m, q, v)
        qp = build_qp(mdl, M, C, J, b, Tt, mask)
        sol = solve_exact(mdl, qp, M, C, J)
        assert_clean(qp, sol, (where, t))
        qn, vn = step(m, _t(q), _t(v), _t(sol.x[:nv]), dt)
        qh.append(qn.numpy())
        vh.append(vn.numpy())
        th.append(sol.x[nv:nv + nu].copy())
        ticks.append((M, C, J, b, Tt, sol))
    gq, gv = np.array(cot["qpos"][nticks], float), np.array(cot["qvel"][nticks], float)
    sums = {}

    def add(k, v):
        sums[k] = v if k not in sums else sums[k] + v

    for t in range(nticks - 1, -1, -1):
        M, C, J, b, Tt, sol = ticks[t]
        dq, dvv, da = step_vjp(m, qh[t], vh[t], sol.x[:nv], dt, gq, gv)
        gx = np.zeros(mdl.n)
        gx[:nv] = da
        gx[nv:nv + nu] = cot["tau"][t]
        fn = ber.reference_adjoint_env if env else bd.reference_adjoint_data
        g = fn(mdl, M, C, J, b, Tt, mask, gx, sol.x, sol.y)
        k = kbr.vjp(m, qh[t], vh[t], kin_params, dict(M=g["M"], C=g["C"], J=g["J"], b=g["b"]))
        gq = dq + k["qpos"]
        gv = dvv + k["qvel"]
        if pd is not None:
            gp, gqt, gl, ga = pd_vjp(mdl.ns, qh[t][3:7], pd[0], pd[1], pd[2], g["T"])
            gq[0:3] += gp
            gq[3:7] += gqt
            gv[0:3] += gl
            gv[3:6] += ga
        else:
            add("T", g["T"])
        gq = gq + cot["qpos"][t]
        gv = gv + cot["qvel"][t]
        for f in (kin_params or {}):
            add(f, k[f])
        if env:
            for f in ber.FIELDS:
                add(f, np.asarray(g[f], float))
    grads = dict(qpos0=gq, qvel0=gv, **sums)
    return grads, dict(qpos=np.array(qh), qvel=np.array(vh), tau=np.array(th).reshape(nticks, nu))
