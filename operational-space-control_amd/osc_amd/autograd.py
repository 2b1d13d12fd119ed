"""torch.autograd through the batched OSC solve: gradients of (tau, x) with respect to the task
targets T and the task bias b and, with data_grads=True, the dynamics inputs M, C and J
(include/osc_backward.h).

    tau, x, status = solve_differentiable(solver, M, C, J, b, T, mask)
    loss(tau, x).backward()        # T.grad, b.grad

    tau, x, status = solve_differentiable(solver, M, C, J, b, T, mask, data_grads=True)
    loss(tau, x).backward()        # M.grad, C.grad, J.grad as well

The forward is OSCBatchSolver.solve_into with the design vector and the duals; the backward is one
launch on the forward's workspace: osc_batch_solve_backward, or osc_batch_solve_backward_data
with data_grads=True, filling only the gradients autograd asks for.  By default gradients flow to
T and b ONLY: M, C, J and mask get None (a None is not a zero), so M, C or J with requires_grad
raise instead of silently training nothing.  The mask never gets a gradient; the task weights are
model constants, not tensors (their gradient: OSCBatchSolver.backward_data_into's grad_wrow).

With per-env parameters (solver.EnvParams; include/osc_backward_env.h):

    p = EnvParams(mu=mu, fz_ub=cap, w_pos=w)     # tensors with requires_grad get a gradient
    tau, x, status = solve_differentiable_env(solver, M, C, J, b, T, mask, p)
    loss(tau, x).backward()        # mu.grad, cap.grad, w.grad, T.grad, b.grad

Through the kinematics front end (include/osc_kin_backward.h), for callers who
hold qpos / qvel on the device:

    M, C, J, b = kinematics_differentiable(kin, qpos, qvel)            # kin: a KinematicsBatch
    tau, x, status = solve_differentiable_qpos(solver, kin, qpos, qvel, T, mask,
                                               kin_params=KinEnvParams(mass_scale=s))
    loss(tau, x).backward()        # qpos.grad, qvel.grad, s.grad, T.grad: two backward launches

Through the forward dynamics of a plant (include/osc_plant_backward.h):

    qacc = forward_dynamics_differentiable(solver, kin, M, C, J, u, z, qfrc)
    loss(qacc).backward()          # M.grad, C.grad, J.grad, u.grad, z.grad, qfrc.grad: one launch
"""
from __future__ import annotations

import torch

from .kinematics import KinEnvGrads, KinEnvParams, KinematicsBatch
from .solver import EnvGrads, EnvParams, OSCBatchSolver


class _OSCSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, M, C, J, b, T, mask):
        nenv = int(M.shape[0])
        out = solver.alloc_outputs(nenv, want_x=True, want_y=True)
        with torch.cuda.device(solver.device):
            solver.solve_into(out, M, C, J, b, T, mask)
        ctx.solver, ctx.out = solver, out
        ctx.save_for_backward(J, mask)
        ctx.mark_non_differentiable(out.status)
        return out.x, out.status

    @staticmethod
    def backward(ctx, grad_x, _grad_status):
        solver, out = ctx.solver, ctx.out
        J, mask = ctx.saved_tensors
        d = solver.dims
        nenv = out.tau.shape[0]
        need_b, need_T = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        if grad_x is None or not (need_b or need_T):
            return (None,) * 7
        grad_x = grad_x.to(dtype=torch.float64).contiguous()
        opts = dict(dtype=torch.float64, device=solver.device)
        grad_T = torch.empty((nenv, d["ns"], 6), **opts) if need_T else None
        grad_b = torch.empty((nenv, d["s"]), **opts) if need_b else None
        with torch.cuda.device(solver.device):
            solver.backward_into(out, J, mask, grad_x, grad_T, grad_b)
        return None, None, None, None, grad_b, grad_T, None


class _OSCSolveData(torch.autograd.Function):
    """As _OSCSolve, differentiable with respect to M, C and J as well."""

    @staticmethod
    def forward(ctx, solver, M, C, J, b, T, mask):
        nenv = int(M.shape[0])
        out = solver.alloc_outputs(nenv, want_x=True, want_y=True)
        with torch.cuda.device(solver.device):
            solver.solve_into(out, M, C, J, b, T, mask)
        ctx.solver, ctx.out = solver, out
        ctx.save_for_backward(M, J, b, T, mask)
        ctx.mark_non_differentiable(out.status)
        return out.x, out.status

    @staticmethod
    def backward(ctx, grad_x, _grad_status):
        solver, out = ctx.solver, ctx.out
        M, J, b, T, mask = ctx.saved_tensors
        d = solver.dims
        nenv = out.tau.shape[0]
        need = dict(zip(("M", "C", "J", "b", "T"), ctx.needs_input_grad[1:6]))
        if grad_x is None or not any(need.values()):
            return (None,) * 7
        grad_x = grad_x.to(dtype=torch.float64).contiguous()
        shape = dict(M=(nenv, d["nv"], d["nv"]), C=(nenv, d["nv"]), J=(nenv, d["s"], d["nv"]),
                     b=(nenv, d["s"]), T=(nenv, d["ns"], 6))
        g = {k: (torch.empty(shape[k], dtype=torch.float64, device=solver.device) if need[k]
                 else None) for k in shape}
        with torch.cuda.device(solver.device):
            solver.backward_data_into(out, M, J, b, T, mask, grad_x, grad_M=g["M"], grad_C=g["C"],
                                      grad_J=g["J"], grad_T=g["T"], grad_b=g["b"])
        return None, g["M"], g["C"], g["J"], g["b"], g["T"], None


def solve_differentiable(solver: OSCBatchSolver, M, C, J, b, T, mask, data_grads: bool = False,
                         env_params=None):
    """(tau, x, status) of the batch, differentiable with respect to T and b, and with
    data_grads=True with respect to M, C and J as well.

    Inputs are float64 tensors on the solver's device in the C-ABI's layout (solver.prepare).  tau
    is the slice x[:, nv:nv + nu], so a loss on either reaches the same backward.  Without
    data_grads gradients flow to T and b only; M, C, J and mask get None, and M, C or J with
    requires_grad raise ValueError.  M.grad treats all nv^2 entries of M as independent (it is not
    symmetrised).  An env whose status is not 0 contributes zero gradients.  The model must have
    no wheel rows.  env_params (solver.EnvParams) is not supported here -- this function's backward
    kernels read the model's friction and weights: solve_differentiable_env takes it."""
    if env_params is not None:
        raise NotImplementedError("solve_differentiable: per-env parameters have no backward pass "
                                  "(the backward kernels read the model's mu and task weights); "
                                  "use solve_differentiable_env")
    if not data_grads:
        for name, t in (("M", M), ("C", C), ("J", J)):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise ValueError(f"solve_differentiable: no gradient with respect to {name} "
                                 "(only T and b are differentiated; pass data_grads=True)")
    M, C, J, b, T, mask = solver.prepare(M, C, J, b, T, mask)
    fn = _OSCSolveData if data_grads else _OSCSolve
    x, status = fn.apply(solver, M, C, J, b, T, mask)
    d = solver.dims
    return x[:, d["nv"]:d["nv"] + d["nu"]], x, status


class _OSCSolveEnv(torch.autograd.Function):
    """The solve with per-env parameters; the seven EnvParams fields follow the data inputs as
    explicit inputs (a tensor, or None for a field that is absent or a numpy array)."""

    @staticmethod
    def forward(ctx, solver, env_params, M, C, J, b, T, mask, *fields):
        nenv = int(M.shape[0])
        out = solver.alloc_outputs(nenv, want_x=True, want_y=True)
        with torch.cuda.device(solver.device):
            solver.solve_into(out, M, C, J, b, T, mask, env_params=env_params)
        ctx.solver, ctx.out, ctx.env_params = solver, out, env_params
        ctx.save_for_backward(M, J, b, T, mask)
        ctx.mark_non_differentiable(out.status)
        return out.x, out.status

    @staticmethod
    def backward(ctx, grad_x, _grad_status):
        solver, out = ctx.solver, ctx.out
        M, J, b, T, mask = ctx.saved_tensors
        d = solver.dims
        nenv = out.tau.shape[0]
        need = dict(zip(("M", "C", "J", "b", "T"), ctx.needs_input_grad[2:7]))
        need_p = dict(zip(EnvParams.FIELDS, ctx.needs_input_grad[8:15]))
        if grad_x is None or not (any(need.values()) or any(need_p.values())):
            return (None,) * 15
        grad_x = grad_x.to(dtype=torch.float64).contiguous()
        shape = dict(M=(nenv, d["nv"], d["nv"]), C=(nenv, d["nv"]), J=(nenv, d["s"], d["nv"]),
                     b=(nenv, d["s"]), T=(nenv, d["ns"], 6))
        g = {k: (torch.empty(shape[k], dtype=torch.float64, device=solver.device) if need[k]
                 else None) for k in shape}
        eg = EnvGrads.empty(nenv, d, solver.device, [k for k in EnvParams.FIELDS if need_p[k]])
        with torch.cuda.device(solver.device):
            solver.backward_env_into(out, M, J, b, T, mask, grad_x, env_params=ctx.env_params,
                                     grad_M=g["M"], grad_C=g["C"], grad_J=g["J"], grad_T=g["T"],
                                     grad_b=g["b"], env_grads=eg)
        return (None, None, g["M"], g["C"], g["J"], g["b"], g["T"], None,
                *(getattr(eg, k) for k in EnvParams.FIELDS))


def solve_differentiable_env(solver: OSCBatchSolver, M, C, J, b, T, mask, env_params: EnvParams,
                             data_grads: bool = False):
    """(tau, x, status) of the batch solved with per-env parameters (solver.EnvParams),
    differentiable with respect to those parameters, to T and b, and with data_grads=True to M, C
    and J as well.

    An EnvParams field that is a torch tensor with requires_grad -- float64, on the solver's
    device, ValueError otherwise -- receives a gradient; a numpy field, or a tensor without
    requires_grad, gets none (its .grad stays None).  One backward launch
    (osc_batch_solve_backward_env) fills only what autograd asks for.  The gradient with respect to
    fz_lb at a contact resting on the pyramid's apex (fz_lb x mask = 0) is the left derivative, 0
    (include/osc_backward_env.h).  Everything else as solve_differentiable."""
    if not isinstance(env_params, EnvParams):
        raise TypeError("solve_differentiable_env: env_params must be an EnvParams")
    if not data_grads:
        for name, t in (("M", M), ("C", C), ("J", J)):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise ValueError(f"solve_differentiable_env: no gradient with respect to {name} "
                                 "(pass data_grads=True)")
    M, C, J, b, T, mask = solver.prepare(M, C, J, b, T, mask)
    fields = []
    for name in EnvParams.FIELDS:
        a = getattr(env_params, name)
        if isinstance(a, torch.Tensor) and a.requires_grad:
            if a.device != solver.device:
                raise ValueError(f"solve_differentiable_env: EnvParams.{name} requires a gradient "
                                 f"and must be on {solver.device}")
            fields.append(a)
        else:
            fields.append(None)
    x, status = _OSCSolveEnv.apply(solver, env_params, M, C, J, b, T, mask, *fields)
    d = solver.dims
    return x[:, d["nv"]:d["nv"] + d["nu"]], x, status


class _Kinematics(torch.autograd.Function):
    """osc_batch_kinematics(_env); the three KinEnvParams fields follow qpos and qvel as explicit
    inputs (a tensor, or None for a field that is absent, a numpy array or needs no gradient)."""

    @staticmethod
    def forward(ctx, kin, kin_params, want_sites, qpos, qvel, *fields):
        nenv = int(qpos.shape[0])
        out = kin.alloc(nenv, want_sites)
        with torch.cuda.device(kin.device):
            kin.compute_into(out, qpos, qvel, kin_params=kin_params)
        ctx.kin, ctx.kin_params, ctx.want_sites = kin, kin_params, want_sites
        ctx.save_for_backward(qpos, qvel)
        if want_sites:
            return out.M, out.C, out.J, out.b, out.site_xpos
        return out.M, out.C, out.J, out.b

    @staticmethod
    def backward(ctx, *grads):
        kin = ctx.kin
        qpos, qvel = ctx.saved_tensors
        nenv = int(qpos.shape[0])
        need_q, need_v = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        need_p = [k for k, n in zip(KinEnvParams.FIELDS, ctx.needs_input_grad[5:8]) if n]
        if all(g is None for g in grads) or not (need_q or need_v or need_p):
            return (None,) * 8
        g = [None if t is None else t.to(dtype=torch.float64).contiguous() for t in grads]
        g += [None] * (5 - len(g))
        opts = dict(dtype=torch.float64, device=kin.device)
        gq = torch.empty((nenv, kin.nq), **opts) if need_q else None
        gv = torch.empty((nenv, kin.nv), **opts) if need_v else None
        kg = KinEnvGrads.empty(nenv, kin.nbody, kin.nv, kin.device, need_p) if need_p else None
        with torch.cuda.device(kin.device):
            kin.backward_into(qpos, qvel, grad_M=g[0], grad_C=g[1], grad_J=g[2], grad_b=g[3],
                              grad_site_xpos=g[4], grad_qpos=gq, grad_qvel=gv,
                              kin_params=ctx.kin_params, kin_grads=kg)
        return (None, None, None, gq, gv,
                *(getattr(kg, k) if kg is not None else None for k in KinEnvParams.FIELDS))


def kinematics_differentiable(kin: KinematicsBatch, qpos, qvel, kin_params=None,
                              want_sites: bool = False):
    """(M, C, J, b[, site_xpos]) of the batch (KinematicsBatch.compute_into), differentiable with
    respect to qpos (the raw nq coordinates: a quaternion's gradient is orthogonal to it), qvel
    and the fields of kin_params (a KinEnvParams) that are torch tensors with requires_grad --
    float64, on kin's device, ValueError otherwise; a numpy field, or a tensor without
    requires_grad, gets none (its .grad stays None).  The backward is one launch
    (osc_batch_kinematics_backward) that fills only what autograd asks for; an env with invalid
    parameters contributes zero gradients.  M's cotangent treats all nv^2 entries as independent."""
    if kin_params is not None and not isinstance(kin_params, KinEnvParams):
        raise TypeError("kinematics_differentiable: kin_params must be a KinEnvParams")
    nenv = int(qpos.shape[0])
    qpos = kin._dev(qpos, (nenv, kin.nq), "qpos")
    qvel = kin._dev(qvel, (nenv, kin.nv), "qvel")
    fields = []
    for name in KinEnvParams.FIELDS:
        a = getattr(kin_params, name) if kin_params is not None else None
        if isinstance(a, torch.Tensor) and a.requires_grad:
            if a.device != kin.device:
                raise ValueError(f"kinematics_differentiable: KinEnvParams.{name} requires a "
                                 f"gradient and must be on {kin.device}")
            fields.append(a)
        else:
            fields.append(None)
    return _Kinematics.apply(kin, kin_params, bool(want_sites), qpos, qvel, *fields)


def solve_differentiable_qpos(solver: OSCBatchSolver, kin: KinematicsBatch, qpos, qvel, T, mask,
                              env_params=None, kin_params=None):
    """(tau, x, status) of the joint-state tick (KinematicsBatch.solve: its forward values,
    bitwise), differentiable with respect to qpos, qvel, T and the tensor fields of kin_params
    and env_params that require a gradient: kinematics_differentiable composed with
    solve_differentiable(data_grads=True), or with solve_differentiable_env(data_grads=True) when
    env_params (a solver.EnvParams) is given.  Two backward launches."""
    M, C, J, b = kinematics_differentiable(kin, qpos, qvel, kin_params=kin_params)
    if env_params is not None:
        return solve_differentiable_env(solver, M, C, J, b, T, mask, env_params, data_grads=True)
    return solve_differentiable(solver, M, C, J, b, T, mask, data_grads=True)


class _Rollout(torch.autograd.Function):
    """KinematicsBatch.rollout with histories; qpos, qvel, the held T (or None) and the seven
    EnvParams and three KinEnvParams fields follow as explicit inputs (a tensor, or None for a
    field that is absent, a numpy array or needs no gradient)."""

    NFIXED = 9   # solver .. kin_params

    @staticmethod
    def forward(ctx, solver, kin, mask, nticks, dt, pd, warm, env_params, kin_params, qpos, qvel,
                T, *fields):
        res = kin.rollout(solver, qpos, qvel, mask, nticks, dt, T=T, pd=pd, warm=warm,
                          history=True, env_params=env_params, kin_params=kin_params)
        ctx.call = (solver, kin, mask, dt, pd, env_params, kin_params, T)
        ctx.res = res
        ctx.mark_non_differentiable(res.status_hist)
        return res.qpos_hist, res.qvel_hist, res.tau_hist, res.status_hist

    @staticmethod
    def backward(ctx, gq, gv, gt, _grad_status):
        solver, kin, mask, dt, pd, env_params, kin_params, T = ctx.call
        names = ("qpos0", "qvel0", "T") + tuple("env." + k for k in EnvParams.FIELDS) + \
            tuple("kin." + k for k in KinEnvParams.FIELDS)
        need = ctx.needs_input_grad[_Rollout.NFIXED:]
        want = tuple(n for n, w in zip(names, need) if w)
        none = (None,) * (_Rollout.NFIXED + len(names))
        if not want or all(g is None for g in (gq, gv, gt)):
            return none
        cot = [None if g is None else g.to(dtype=torch.float64).contiguous() for g in (gq, gv, gt)]
        g = kin.rollout_backward(solver, ctx.res, mask, dt, T=T, pd=pd, grad_qpos_hist=cot[0],
                                 grad_qvel_hist=cot[1], grad_tau_hist=cot[2],
                                 env_params=env_params, kin_params=kin_params, want=want)
        return none[:_Rollout.NFIXED] + tuple(g.get(n) for n in names)


class _RolloutSched(torch.autograd.Function):
    """KinematicsBatch.rollout(..., schedule=) with histories (osc_batch_rollout_sched and its
    backward, include/osc_rollout_schedule.h); qpos, qvel, the held T, schedule.T, the two PD
    references (held, or the schedule's: seq_refs), the gains and the parameter fields follow as
    explicit inputs (a tensor, or None / a plain value where no gradient is wanted)."""

    NFIXED = 11   # solver .. pd_mode

    @staticmethod
    def _call(sched_mask, seq_refs, pd_mode, T, sched_T, pos_ref, quat_ref, gains):
        from .kinematics import RolloutSchedule
        schedule = RolloutSchedule(T=sched_T, mask=sched_mask,
                                   pos_ref=pos_ref if seq_refs[0] else None,
                                   quat_ref=quat_ref if seq_refs[1] else None)
        pd = None
        if pd_mode:
            g = gains.detach().cpu().tolist() if isinstance(gains, torch.Tensor) else gains
            pd = (None if seq_refs[0] else pos_ref, None if seq_refs[1] else quat_ref, g)
        return schedule, pd

    @staticmethod
    def forward(ctx, solver, kin, mask, nticks, dt, warm, env_params, kin_params, sched_mask,
                seq_refs, pd_mode, qpos, qvel, T, sched_T, pos_ref, quat_ref, gains, *fields):
        schedule, pd = _RolloutSched._call(sched_mask, seq_refs, pd_mode, T, sched_T, pos_ref,
                                           quat_ref, gains)
        res = kin.rollout(solver, qpos, qvel, mask, nticks, dt, T=T, pd=pd, warm=warm,
                          history=True, env_params=env_params, kin_params=kin_params,
                          schedule=schedule)
        ctx.call = (solver, kin, mask, dt, pd, env_params, kin_params, T, schedule, seq_refs)
        ctx.res = res
        ctx.mark_non_differentiable(res.status_hist)
        return res.qpos_hist, res.qvel_hist, res.tau_hist, res.status_hist

    @staticmethod
    def backward(ctx, gq, gv, gt, _grad_status):
        solver, kin, mask, dt, pd, env_params, kin_params, T, schedule, seq_refs = ctx.call
        names = ("qpos0", "qvel0", "T", "T_seq", "pos_ref_seq" if seq_refs[0] else "pos_ref",
                 "quat_ref_seq" if seq_refs[1] else "quat_ref", "gains") + \
            tuple("env." + k for k in EnvParams.FIELDS) + \
            tuple("kin." + k for k in KinEnvParams.FIELDS)
        need = ctx.needs_input_grad[_RolloutSched.NFIXED:]
        want = tuple(n for n, w in zip(names, need) if w)
        none = (None,) * (_RolloutSched.NFIXED + len(names))
        if not want or all(g is None for g in (gq, gv, gt)):
            return none
        cot = [None if g is None else g.to(dtype=torch.float64).contiguous() for g in (gq, gv, gt)]
        g = kin.rollout_backward(solver, ctx.res, mask, dt, T=T, pd=pd, grad_qpos_hist=cot[0],
                                 grad_qvel_hist=cot[1], grad_tau_hist=cot[2],
                                 env_params=env_params, kin_params=kin_params, want=want,
                                 schedule=schedule)
        return none[:_RolloutSched.NFIXED] + tuple(g.get(n) for n in names)


def rollout_differentiable(solver: OSCBatchSolver, kin: KinematicsBatch, qpos, qvel, mask,
                           nticks: int, dt: float, T=None, pd=None, warm: bool = True,
                           env_params=None, kin_params=None, schedule=None, plant=None):
    """(qpos_hist, qvel_hist, tau_hist, status_hist) of the closed-loop rollout
    (KinematicsBatch.rollout(..., history=True, schedule=...): its forward values, bitwise),
    differentiable with respect to qpos, qvel, a held T and the tensor fields of env_params (a
    solver.EnvParams) and kin_params (a KinEnvParams) that require a gradient -- float64, on kin's
    device, ValueError otherwise; a numpy field, or a tensor without requires_grad, gets none.
    Without a schedule exactly one of T (held targets) and pd = (pos_ref, quat_ref, gains).
    With schedule (a kinematics.RolloutSchedule: inputs that change over the ticks) gradients also
    flow to schedule.T (every tick's target gradient: a target sequence can be optimised),
    schedule.pos_ref and schedule.quat_ref.  The held PD references get a gradient too, and so do
    the gains when they are passed as a float64 tensor of 4 on kin's device (their values are read
    on the host: one synchronisation).  dt and the mask, held or scheduled, get no gradient.
    The backward is one call (osc_batch_rollout_backward, include/osc_rollout_backward.h, or
    osc_batch_rollout_backward_sched, include/osc_rollout_schedule.h) that recomputes the ticks
    from the histories and fills only what autograd asks for; a loss may touch any slab of the
    three histories.  The gradient with respect to qpos is with respect to the raw nq
    coordinates.
    plant (a kinematics.Plant with a field set) raises NotImplementedError: gradients through the
    plant are out of scope (include/osc_plant.h), and the backward pass here is the matched
    model's."""
    if plant is not None and getattr(plant, "active", True):
        raise NotImplementedError(
            "rollout_differentiable: its backward pass is the matched model's, wrong for a plant "
            "(include/osc_plant.h, DESIGN.md §7.5); rollout_plant_differentiable differentiates "
            "through the plant")
    if env_params is not None and not isinstance(env_params, EnvParams):
        raise TypeError("rollout_differentiable: env_params must be an EnvParams")
    if kin_params is not None and not isinstance(kin_params, KinEnvParams):
        raise TypeError("rollout_differentiable: kin_params must be a KinEnvParams")
    grad_t = lambda r: isinstance(r, torch.Tensor) and r.requires_grad
    sched = schedule is not None or (pd is not None and any(grad_t(r) for r in pd))
    if sched:
        if T is not None and pd is not None:
            raise ValueError("rollout_differentiable: at most one of T and pd may be given")
        if T is None and pd is None and (schedule is None or schedule.T is None):
            raise ValueError("rollout_differentiable: one of T, pd and schedule.T must be given")
    elif (T is None) == (pd is None):
        raise ValueError("rollout_differentiable: exactly one of T and pd must be given")
    d = solver.dims
    nenv = int(qpos.shape[0])
    qpos = kin._dev(qpos, (nenv, kin.nq), "qpos")
    qvel = kin._dev(qvel, (nenv, kin.nv), "qvel")
    if T is not None:
        T = kin._dev(T, (nenv, d["ns"], 6), "T")
    fields = []
    for block, cls, label in ((env_params, EnvParams, "EnvParams"),
                              (kin_params, KinEnvParams, "KinEnvParams")):
        for name in cls.FIELDS:
            a = getattr(block, name) if block is not None else None
            if isinstance(a, torch.Tensor) and a.requires_grad:
                if a.device != kin.device:
                    raise ValueError(f"rollout_differentiable: {label}.{name} requires a gradient "
                                     f"and must be on {kin.device}")
                fields.append(a)
            else:
                fields.append(None)
    if sched:
        from .kinematics import RolloutSchedule
        sc = schedule if schedule is not None else RolloutSchedule()
        pos_ref, quat_ref, gains = pd if pd is not None else (None, None, None)
        seq_refs = (sc.pos_ref is not None, sc.quat_ref is not None)
        refs = [sc.pos_ref if seq_refs[0] else pos_ref, sc.quat_ref if seq_refs[1] else quat_ref]
        for i, r in enumerate(refs):
            if grad_t(r) and (r.dtype != torch.float64 or r.device != kin.device):
                raise ValueError("rollout_differentiable: a PD reference that requires a gradient "
                                 f"must be float64 on {kin.device}")
        if grad_t(gains) and (gains.dtype != torch.float64 or gains.device != kin.device or
                              tuple(gains.shape) != (4,)):
            raise ValueError("rollout_differentiable: gains that require a gradient must be a "
                             f"float64 tensor of 4 on {kin.device}")
        sT = sc.T
        if grad_t(sT) and (sT.dtype != torch.float64 or sT.device != kin.device):
            raise ValueError("rollout_differentiable: schedule.T requires a gradient and must be "
                             f"float64 on {kin.device}")
        return _RolloutSched.apply(solver, kin, mask, int(nticks), float(dt), bool(warm),
                                   env_params, kin_params, sc.mask, seq_refs, pd is not None,
                                   qpos, qvel, T, sT, refs[0], refs[1], gains, *fields)
    return _Rollout.apply(solver, kin, mask, int(nticks), float(dt), pd, bool(warm), env_params,
                          kin_params, qpos, qvel, T, *fields)


class _ForwardDynamics(torch.autograd.Function):
    """osc_batch_forward_dynamics and its vector-Jacobian product (include/osc_plant_backward.h)."""

    @staticmethod
    def forward(ctx, solver, kin, M, C, J, u, z, qfrc):
        nenv = int(M.shape[0])
        qacc = torch.empty((nenv, kin.nv), dtype=torch.float64, device=kin.device)
        with torch.cuda.device(kin.device):
            kin.forward_dynamics_into(solver, qacc, M, C, J, u, z, qfrc)
        ctx.solver, ctx.kin = solver, kin
        ctx.save_for_backward(M, J, z, qacc)
        return qacc

    @staticmethod
    def backward(ctx, grad_qacc):
        solver, kin = ctx.solver, ctx.kin
        M, J, z, qacc = ctx.saved_tensors
        need = dict(zip(("M", "C", "J", "u", "z", "qfrc"), ctx.needs_input_grad[2:]))
        if grad_qacc is None or not any(need.values()):
            return (None,) * 8
        d = solver.dims
        nenv, nv, nz = int(M.shape[0]), kin.nv, 3 * d["nc"]
        if z is None:          # no contact force: J did not enter the forward
            need["J"] = need["z"] = False
        opts = dict(dtype=torch.float64, device=kin.device)
        shape = dict(M=(nenv, nv, nv), C=(nenv, nv), Jc=(nenv, nz, nv), u=(nenv, d["nu"]),
                     z=(nenv, nz), qfrc=(nenv, nv))
        need["Jc"] = need.pop("J")
        out = {k: torch.empty(shape[k], **opts) if need[k] else None for k in shape}
        if not any(t is not None for t in out.values()):
            return (None,) * 8
        g = grad_qacc.to(dtype=torch.float64).contiguous()
        with torch.cuda.device(kin.device):
            kin.forward_dynamics_backward(solver, M, J if out["z"] is not None else None, z, qacc,
                                          g, **{"grad_" + k: t for k, t in out.items()})
        gJ = None
        if out["Jc"] is not None:      # the compact contact rows into a J-shaped cotangent
            r0 = 3 * d["ns"] - nz
            gJ = torch.zeros((nenv, 6 * d["ns"], nv), **opts)
            gJ[:, r0:r0 + nz] = out["Jc"]
        return (None, None, out["M"], out["C"], gJ, out["u"], out["z"], out["qfrc"])


def forward_dynamics_differentiable(solver: OSCBatchSolver, kin: KinematicsBatch, M, C, J, u,
                                    z=None, qfrc_applied=None):
    """qacc (nenv, nv) = M^-1 (B u + Jc' z + qfrc_applied - C) (KinematicsBatch.
    forward_dynamics_into: its forward values, bitwise), differentiable with respect to M, C, J, u,
    z and qfrc_applied -- float64 tensors on kin's device; z / qfrc_applied None = no contact force
    / no applied force, and J may then be None too.  The backward is one launch
    (osc_batch_forward_dynamics_backward, include/osc_plant_backward.h) that fills only what
    autograd asks for.  M's gradient treats all nv^2 entries as independent (-w qacc', not
    symmetrised); J's is zero outside the contact rows; an env whose M is not positive definite,
    or with a non-finite input, has a NaN qacc row and zero gradients."""
    nenv = int(M.shape[0])
    d = solver.dims
    u = u if u.stride(-1) == 1 else u.contiguous()
    if z is not None and z.stride(-1) != 1:
        z = z.contiguous()
    if z is None:
        J = None
    for name, t, shape in (("M", M, (nenv, kin.nv, kin.nv)), ("C", C, (nenv, kin.nv)),
                           ("J", J, (nenv, 6 * d["ns"], kin.nv)),
                           ("qfrc_applied", qfrc_applied, (nenv, kin.nv))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or
                              t.device != kin.device or tuple(t.shape) != shape):
            raise ValueError(f"forward_dynamics_differentiable: {name} must be a float64 tensor of "
                             f"shape {shape} on {kin.device}")
    cont = lambda t: None if t is None else t.contiguous()
    return _ForwardDynamics.apply(solver, kin, cont(M), cont(C), cont(J), u, z,
                                  cont(qfrc_applied))


class _RolloutPlant(torch.autograd.Function):
    """KinematicsBatch.rollout(..., plant=) with histories and rollout_plant_backward.  As
    _RolloutSched: qpos, qvel, the held T, schedule.T, the two PD references (held, or the
    schedule's: seq_refs), the gains and the seven EnvParams and three KinEnvParams fields follow
    as explicit inputs, then the plant's qfrc_applied and its three KinEnvParams fields (a tensor,
    or None / a plain value where no gradient is wanted)."""

    NFIXED = 12   # solver .. plant

    @staticmethod
    def forward(ctx, solver, kin, mask, nticks, dt, warm, env_params, kin_params, sched_mask,
                seq_refs, pd_mode, plant, qpos, qvel, T, sched_T, pos_ref, quat_ref, gains,
                *fields):
        schedule, pd = _RolloutSched._call(sched_mask, seq_refs, pd_mode, T, sched_T, pos_ref,
                                           quat_ref, gains)
        if sched_T is None and sched_mask is None and not any(seq_refs):
            schedule = None
        res = kin.rollout(solver, qpos, qvel, mask, nticks, dt, T=T, pd=pd, warm=warm,
                          history=True, env_params=env_params, kin_params=kin_params,
                          schedule=schedule, plant=plant)
        ctx.call = (solver, kin, mask, dt, pd, env_params, kin_params, T, schedule, seq_refs)
        ctx.res = res
        ctx.mark_non_differentiable(res.status_hist)
        return res.qpos_hist, res.qvel_hist, res.tau_hist, res.status_hist, res.qacc_hist

    @staticmethod
    def backward(ctx, gq, gv, gt, _grad_status, ga):
        solver, kin, mask, dt, pd, env_params, kin_params, T, schedule, seq_refs = ctx.call
        names = ("qpos0", "qvel0", "T", "T_seq", "pos_ref_seq" if seq_refs[0] else "pos_ref",
                 "quat_ref_seq" if seq_refs[1] else "quat_ref", "gains") + \
            tuple("env." + k for k in EnvParams.FIELDS) + \
            tuple("kin." + k for k in KinEnvParams.FIELDS) + ("plant.qfrc_applied",) + \
            tuple("plant.kin." + k for k in KinEnvParams.FIELDS)
        need = ctx.needs_input_grad[_RolloutPlant.NFIXED:]
        want = tuple(n for n, w in zip(names, need) if w)
        none = (None,) * (_RolloutPlant.NFIXED + len(names))
        if not want or all(g is None for g in (gq, gv, gt, ga)):
            return none
        cot = [None if g is None else g.to(dtype=torch.float64).contiguous()
               for g in (gq, gv, gt, ga)]
        g = kin.rollout_plant_backward(solver, ctx.res, mask, dt, T=T, pd=pd,
                                       grad_qpos_hist=cot[0], grad_qvel_hist=cot[1],
                                       grad_tau_hist=cot[2], grad_qacc_hist=cot[3],
                                       env_params=env_params, kin_params=kin_params, want=want,
                                       schedule=schedule)
        return none[:_RolloutPlant.NFIXED] + tuple(g.get(n) for n in names)


def rollout_plant_differentiable(solver: OSCBatchSolver, kin: KinematicsBatch, qpos, qvel, mask,
                                 nticks: int, dt: float, T=None, pd=None, warm: bool = True,
                                 env_params=None, kin_params=None, schedule=None, plant=None):
    """(qpos_hist, qvel_hist, tau_hist, status_hist, qacc_hist) of the closed-loop rollout against
    a plant (KinematicsBatch.rollout(..., history=True, plant=plant): its forward values, bitwise;
    plant a kinematics.Plant with a field set).  It carries everything rollout_differentiable
    carries -- gradients to qpos, qvel, a held T, the tensor fields of env_params and kin_params
    (the CONTROLLER's), schedule.T, schedule.pos_ref / quat_ref or the held PD references, and the
    gains when they are a float64 tensor of 4 -- and, through the plant, gradients to
    plant.qfrc_applied (held or per tick: the gradient has its shape) and the tensor fields of
    plant.kin_params.  Only float64 tensors on kin's device that require a gradient get one.  The
    backward is one call (osc_batch_rollout_plant_backward, include/osc_plant_backward.h) that
    fills only what autograd asks for; a loss may touch any slab of the four histories."""
    from .kinematics import Plant, RolloutSchedule
    if not isinstance(plant, Plant) or not plant.active:
        raise ValueError("rollout_plant_differentiable: plant must be a Plant with a field set "
                         "(rollout_differentiable is the call without one)")
    if env_params is not None and not isinstance(env_params, EnvParams):
        raise TypeError("rollout_plant_differentiable: env_params must be an EnvParams")
    for block in (kin_params, plant.kin_params):
        if block is not None and not isinstance(block, KinEnvParams):
            raise TypeError("rollout_plant_differentiable: kin_params must be a KinEnvParams")
    if T is not None and pd is not None:
        raise ValueError("rollout_plant_differentiable: at most one of T and pd may be given")
    if T is None and pd is None and (schedule is None or schedule.T is None):
        raise ValueError("rollout_plant_differentiable: one of T, pd and schedule.T must be given")
    grad_t = lambda r: isinstance(r, torch.Tensor) and r.requires_grad
    d = solver.dims
    nenv = int(qpos.shape[0])
    qpos = kin._dev(qpos, (nenv, kin.nq), "qpos")
    qvel = kin._dev(qvel, (nenv, kin.nv), "qvel")
    if T is not None:
        T = kin._dev(T, (nenv, d["ns"], 6), "T")
    sc = schedule if schedule is not None else RolloutSchedule()
    pos_ref, quat_ref, gains = pd if pd is not None else (None, None, None)
    seq_refs = (sc.pos_ref is not None, sc.quat_ref is not None)
    refs = [sc.pos_ref if seq_refs[0] else pos_ref, sc.quat_ref if seq_refs[1] else quat_ref]
    for r in refs + [sc.T]:
        if grad_t(r) and (r.dtype != torch.float64 or r.device != kin.device):
            raise ValueError("rollout_plant_differentiable: a schedule member or PD reference "
                             f"that requires a gradient must be float64 on {kin.device}")
    if grad_t(gains) and (gains.dtype != torch.float64 or gains.device != kin.device or
                          tuple(gains.shape) != (4,)):
        raise ValueError("rollout_plant_differentiable: gains that require a gradient must be a "
                         f"float64 tensor of 4 on {kin.device}")
    fields = []
    for block, cls, label in ((env_params, EnvParams, "EnvParams"),
                              (kin_params, KinEnvParams, "KinEnvParams"),
                              (plant, ("qfrc_applied",), "Plant"),
                              (plant.kin_params, KinEnvParams, "Plant.kin_params")):
        for name in (cls if isinstance(cls, tuple) else cls.FIELDS):
            a = getattr(block, name) if block is not None else None
            if grad_t(a):
                if a.device != kin.device or a.dtype != torch.float64:
                    raise ValueError(f"rollout_plant_differentiable: {label}.{name} requires a "
                                     f"gradient and must be float64 on {kin.device}")
                fields.append(a)
            else:
                fields.append(None)
    return _RolloutPlant.apply(solver, kin, mask, int(nticks), float(dt), bool(warm), env_params,
                               kin_params, sc.mask, seq_refs, pd is not None, plant, qpos, qvel,
                               T, sc.T, refs[0], refs[1], gains, *fields)
