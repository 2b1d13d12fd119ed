"""CPU reference of the scheduled rollout and its backward pass (include/osc_rollout_schedule.h),
float64, one environment at a time, for tests/test_rollout_schedule_ref.py (CPU) and
tests/test_gpu_rollout_schedule.py (GPU).  It extends tests/rollout_backward_ref.py by import:

  pd_param_vjp   the VJP of rollout_backward_ref.pd_targets with respect to pos_ref, quat_ref and
                 the four gains, by torch.autograd
  rollout        the oracle rollout (tests/rollout_ref.py's step) with per-tick targets, masks
                 and references: what the finite differences are taken of
  chain          rollout_backward_ref.chain with per-tick T, mask and references; next to grad
                 qpos0 / qvel0 it returns every tick's grad_T and the reference and gain
                 gradients, per tick and summed in the order K-1 .. 0.  It keeps
                 rollout_backward_ref.assert_clean at every (env, tick)

TEST INFRASTRUCTURE ONLY.  It lives under tests/ because oracle/ is not to change."""
import numpy as np
import torch

import backward_data_ref as bd
import kin_backward_ref as kbr
import kinematics as kin
import rollout_backward_ref as rbr
import rollout_ref
from osc_qp import build_qp
from qp_exact import solve_exact

_t = rbr._t


def pd_param_vjp(ns, pos, quat, lin, ang, pos_ref, quat_ref, gains, gT):
    """(grad_pos_ref (3), grad_quat_ref (4), grad_gains (4)), numpy, of one env's producer call."""
    pr, qr, g = _t(pos_ref, True), _t(quat_ref, True), _t(gains, True)
    T = rbr.pd_targets(ns, _t(pos), _t(quat), _t(lin), _t(ang), pr, qr, g)
    out = torch.autograd.grad((T * _t(gT)).sum(), [pr, qr, g])
    return tuple(x.numpy() for x in out)


def tick_targets(mdl, q, v, t, T=None, pd=None):
    """Tick t's targets of one env.  Held mode (pd None): T[t].  PD mode: the producer's targets of
    (q, v) under pd = (pos_refs (K, 3), quat_refs (K, 4), gains), plus T[t] when T is given."""
    if pd is None:
        return np.asarray(T[t], float)
    Tt = rollout_ref.pd_targets(mdl, q, v, (pd[0][t], pd[1][t], pd[2]))
    return Tt if T is None else Tt + np.asarray(T[t], float)


def rollout(km, mdl, qpos, qvel, masks, nticks, dt, T=None, pd=None):
    """The oracle rollout with tick t's mask masks[t] and targets tick_targets(t):
    dict(qpos (nticks + 1, nq), qvel (nticks + 1, nv), tau (nticks, nu))."""
    qh, vh, th = [np.array(qpos, float)], [np.array(qvel, float)], []
    for t in range(nticks):
        Tt = tick_targets(mdl, qh[-1], vh[-1], t, T, pd)
        q, v, tau, _ = rollout_ref.step(km, mdl, qh[-1], vh[-1], masks[t], dt, T=Tt)
        qh.append(q)
        vh.append(v)
        th.append(tau)
    return dict(qpos=np.array(qh), qvel=np.array(vh), tau=np.array(th).reshape(nticks, mdl.nu))


def chain(tree, mdl, qpos0, qvel0, masks, nticks, dt, cot, T=None, pd=None, where=""):
    """One env: the forward rollout on the oracle with per-tick inputs (as rollout above) and the
    gradient of sum(cot["qpos"] * qpos_hist) + sum(cot["qvel"] * qvel_hist) + sum(cot["tau"] *
    tau_hist).  Returns (grads, hist): grads = dict(qpos0, qvel0, T_seq (K, ns, 6): every tick's
    grad_T; in PD mode also pos_ref_seq (K, 3), quat_ref_seq (K, 4), their sums pos_ref, quat_ref
    and gains (4), each summed in the order K-1 .. 0); hist = dict(qpos, qvel, tau)."""
    assert T is not None or pd is not None
    m = kin.KinModel(tree)
    nv, nu = mdl.nv, mdl.nu
    qh, vh, th, ticks = [np.array(qpos0, float)], [np.array(qvel0, float)], [], []
    for t in range(nticks):
        q, v = qh[-1], vh[-1]
        Tt = tick_targets(mdl, q, v, t, T, pd)
        M, C, J, b = kin.kinematics(m, q, v)
        qp = build_qp(mdl, M, C, J, b, Tt, masks[t])
        sol = solve_exact(mdl, qp, M, C, J)
        rbr.assert_clean(qp, sol, (where, t))
        qn, vn = rbr.step(m, _t(q), _t(v), _t(sol.x[:nv]), dt)
        qh.append(qn.numpy())
        vh.append(vn.numpy())
        th.append(sol.x[nv:nv + nu].copy())
        ticks.append((M, C, J, b, Tt, sol))
    gq, gv = np.array(cot["qpos"][nticks], float), np.array(cot["qvel"][nticks], float)
    gT_seq = np.zeros((nticks, mdl.ns, 6))
    gpr, gqr = np.zeros((nticks, 3)), np.zeros((nticks, 4))
    sums = dict(pos_ref=np.zeros(3), quat_ref=np.zeros(4), gains=np.zeros(4))
    for t in range(nticks - 1, -1, -1):
        M, C, J, b, Tt, sol = ticks[t]
        dq, dvv, da = rbr.step_vjp(m, qh[t], vh[t], sol.x[:nv], dt, gq, gv)
        gx = np.zeros(mdl.n)
        gx[:nv] = da
        gx[nv:nv + nu] = cot["tau"][t]
        g = bd.reference_adjoint_data(mdl, M, C, J, b, Tt, masks[t], gx, sol.x, sol.y)
        k = kbr.vjp(m, qh[t], vh[t], None, dict(M=g["M"], C=g["C"], J=g["J"], b=g["b"]))
        gq = dq + k["qpos"]
        gv = dvv + k["qvel"]
        gT_seq[t] = g["T"]
        if pd is not None:
            q, v = qh[t], vh[t]
            gp, gqt, gl, ga = rbr.pd_vjp(mdl.ns, q[3:7], pd[0][t], pd[1][t], pd[2], g["T"])
            gq[0:3] += gp
            gq[3:7] += gqt
            gv[0:3] += gl
            gv[3:6] += ga
            gpr[t], gqr[t], gg = pd_param_vjp(mdl.ns, q[0:3], q[3:7], v[0:3], v[3:6], pd[0][t],
                                              pd[1][t], pd[2], g["T"])
            sums["pos_ref"] = sums["pos_ref"] + gpr[t]
            sums["quat_ref"] = sums["quat_ref"] + gqr[t]
            sums["gains"] = sums["gains"] + gg
        gq = gq + cot["qpos"][t]
        gv = gv + cot["qvel"][t]
    grads = dict(qpos0=gq, qvel0=gv, T_seq=gT_seq)
    if pd is not None:
        grads.update(pos_ref_seq=gpr, quat_ref_seq=gqr, **sums)
    return grads, dict(qpos=np.array(qh), qvel=np.array(vh), tau=np.array(th).reshape(nticks, nu))
