"""CPU reference of the closed-loop rollout (include/osc_rollout.h), one environment, built only
from existing oracle functions: kinematics.kinematics -> [producers.pd_base_targets] ->
osc_qp.build_qp -> qp_exact.solve_exact -> qvel += dt dv, kinematics.integrate with the new
velocity (MuJoCo's semi-implicit Euler step on the controller's own model).

TEST INFRASTRUCTURE ONLY.  It lives under tests/ because oracle/ is not to change."""
import numpy as np

import kinematics as kin
import producers
from osc_qp import build_qp, torque
from qp_exact import solve_exact

STANDING_GAINS = (150.0, 25.0, 50.0, 10.0)   # examples/standing.cc:143-155
DT = 0.002


def pd_targets(model, qpos, qvel, pd):
    """The PD base targets of one state; pd = (pos_ref, quat_ref, gains), free root joint."""
    pos_ref, quat_ref, gains = pd
    return producers.pd_base_targets(model.ns, qpos[0:3], qpos[3:7], qvel[0:3], qvel[3:6],
                                     pos_ref, quat_ref, gains)


def step(km, model, qpos, qvel, mask, dt, T=None, pd=None):
    """One tick from (qpos, qvel): returns (qpos', qvel', tau, dv)."""
    assert (T is None) != (pd is None)
    qpos, qvel = np.asarray(qpos, float), np.asarray(qvel, float)
    if T is None:
        T = pd_targets(model, qpos, qvel, pd)
    M, C, J, b = kin.kinematics(km, qpos, qvel)
    x = solve_exact(model, build_qp(model, M, C, J, b, T, mask), M, C, J).x
    dv = x[:model.nv].copy()
    qvel1 = qvel + dt * dv
    return kin.integrate(km, qpos, qvel1, dt), qvel1, torque(model, x), dv


def rollout(km, model, qpos, qvel, mask, nticks, dt, T=None, pd=None):
    """nticks ticks: dict(qpos (nticks + 1, nq), qvel (nticks + 1, nv), tau (nticks, nu))."""
    qh, vh, th = [np.array(qpos, float)], [np.array(qvel, float)], []
    for _ in range(nticks):
        q, v, tau, _ = step(km, model, qh[-1], vh[-1], mask, dt, T=T, pd=pd)
        qh.append(q)
        vh.append(v)
        th.append(tau)
    return dict(qpos=np.array(qh), qvel=np.array(vh), tau=np.array(th).reshape(nticks, model.nu))


def go2_case(offset=(0.01, -0.01, -0.02)):
    """The closed-loop convergence case: the shipped Go2 tree, unit base quaternion, hinge angles
    default_rng(5).uniform(-0.5, 0.5), zero velocity, all contacts on, the base reference `offset`
    away from the initial base position, the standing gains."""
    from osc_qp import load_model
    km = kin.load("unitree_go2")
    model = load_model("unitree_go2")
    qpos = np.zeros(km.nq)
    qpos[3] = 1.0
    qpos[7:] = np.random.default_rng(5).uniform(-0.5, 0.5, km.nq - 7)
    qvel = np.zeros(km.nv)
    pos_ref = qpos[0:3] + np.asarray(offset, float)
    pd = (pos_ref, np.array([1.0, 0.0, 0.0, 0.0]), STANDING_GAINS)
    return km, model, qpos, qvel, np.ones(model.nc), pd


def error_ratio(qpos_final, qpos0, pos_ref):
    """Base-position error after the rollout over its initial value."""
    return float(np.linalg.norm(qpos_final[0:3] - pos_ref) / np.linalg.norm(qpos0[0:3] - pos_ref))
