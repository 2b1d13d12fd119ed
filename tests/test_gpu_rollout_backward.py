"""GPU tests of the rollout's backward pass (include/osc_rollout_backward.h,
csrc/osc_rollout_backward.hip; KinematicsBatch.integrate_backward_into / rollout_backward and
osc_amd.autograd.rollout_differentiable):
   1. the step's adjoint alone against the torch step's VJP (tests/rollout_backward_ref.py);
   2. the PD producer's adjoint alone against the torch VJP;
   3. the whole backward against the same GPU kernels composed by hand in a torch loop;
   4. the whole backward against the CPU chain (exact solver, reference adjoints);
   5. structure: batch independence, reproducibility, linearity, NULL outputs, tick-ordered sums;
   6. memory: guard bands (tests/guard.py) and refusals;
   7. autograd: gradcheck, what gets a gradient, the forward's values.

Error per env and output, as everywhere in the project: |g - g_ref|_inf / (1 + |g_ref|_inf).  Bars:
1e-11 for the step's and the producer's adjoints (the kinematics backward's bar); 10 x the measured
worst for the hand composition on the same x (CKPT_BAR), and the reference's own rounding
sensitivity for the free-running loop (test_whole_backward_vs_the_hand_composition); NORM_TOL =
1e-5 with backward_ref.env_errors against the CPU chain and wherever the solve's backward rounds two
ways."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import backward_ref as br
import kin_env_ref as ker
import kinematics as kin
import rollout_backward_ref as rbr
import rollout_ref
import test_rollout_backward_ref as cpu
from guard import assert_guards_intact, guarded, guarded_like
from kin_trees import mixed_tree, random_tree, slider, spherical_pendulum
from osc_amd import _lib
from osc_amd.kinematics import (KinEnvParams, KinematicsBatch, RolloutResult, load_tree,
                                random_states)
from osc_amd.solver import EnvParams, OSCBatchSolver
from osc_amd.synth import generate
from osc_qp import load_model

pytestmark = pytest.mark.gpu

TOL = 1e-11
NORM_TOL = cpu.NORM_TOL
DT = rollout_ref.DT
GO2, WALTER = "unitree_go2", "walter_sr"
NUMERICAL = _lib.SOLVE_NUMERICAL
K = 3
NBIG = 33                      # two full 16-env blocks and a one-env tail
GAINS = rollout_ref.STANDING_GAINS
OFFSET = np.array([0.01, -0.01, -0.02])

TREES = {GO2: lambda: load_tree(GO2), WALTER: lambda: load_tree(WALTER),
         "mixed_1": lambda: mixed_tree(1),                       # balls and slides
         "random_fixed": lambda: random_tree(2, free_root=False),
         "ball": spherical_pendulum, "slide": slider}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared cases are read-only)


def errors(g, ref):
    """Per env: |g - ref|_inf / (1 + |ref|_inf)."""
    g, ref = np.asarray(g).reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1)
    return np.abs(g - ref).max(axis=1) / (1 + np.abs(ref).max(axis=1))


def bitwise(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def kin_of(name):
    tree = TREES[name]()
    return tree, KinematicsBatch(tree=tree), kin.KinModel(tree)


@functools.lru_cache(maxsize=None)
def pair(robot):
    tree, kb, km = kin_of(robot)
    return tree, kb, km, OSCBatchSolver(robot), load_model(robot)


# ---- 1. the step's adjoint -----------------------------------------------------------------------

def _quats(km):
    """(qadr, dadr) of every quaternion and its three rates."""
    return [(j["qadr"] + (3 if j["type"] == "free" else 0),
             j["dadr"] + (3 if j["type"] == "free" else 0))
            for j in km.joints if j["type"] in ("free", "ball")]


@pytest.mark.parametrize("nenv", [1, 5, 17])
@pytest.mark.parametrize("name", list(TREES))
def test_step_adjoint_vs_the_torch_vjp(gpu, name, nenv):
    """osc_batch_integrate_backward against rollout_backward_ref.step_vjp with drawn cotangents,
    dt = +-0.002; a lone env, a partial block, a full 16-env block plus a tail.  In the batches of 5
    and 17 four rows are forced: all rates exactly zero (the limit branch), rates of 1e-9 (the
    series branch), status NUMERICAL and a NaN in qacc (both: cotangents passed through, grad_qacc
    zero).  Every env, grad_qpos / grad_qvel / grad_qacc within 1e-11; the quaternion blocks of
    grad_qpos orthogonal to q within the same bar; a strided grad_qacc / qacc pair out of an
    x-shaped buffer and the in-place call bitwise the packed, out-of-place one.

    Worst measured on an MI355X per tree (grad_qpos / grad_qvel / grad_qacc), over the three batch
    sizes and both signs of dt:
      Go2            1.7e-16 / 5.9e-18 / 2.7e-20
      WaLTER         2.1e-16 / 0 / 0
      mixed_tree(1)  2.6e-16 / 3.0e-18 / 1.4e-20
      fixed-base random_tree(2), slider   0 / 0 / 0   (no quaternion: one product per entry)
      spherical pendulum                  2.5e-16 / 2.0e-18 / 6.8e-21
    None exceeds 1e-13."""
    tree, kb, km = kin_of(name)
    nq, nv = km.nq, km.nv
    rows = {1: (), 5: (1, 2, 3, 4), 17: (1, 5, 15, 16)}[nenv]
    worst = np.zeros(3)
    for dt in (DT, -DT):
        qpos, qvel = random_states(tree, nenv, 21, base_pos_zero=False)
        rng = np.random.default_rng(500 + nenv)
        qacc = rng.standard_normal((nenv, nv))
        gqn, gvn = rng.standard_normal((nenv, nq)), rng.standard_normal((nenv, nv))
        status = np.zeros(nenv, np.int32)
        frozen = np.zeros(nenv, bool)
        if rows:
            r_zero, r_tiny, r_num, r_nan = rows
            u = np.array([0.6, 0.0, -0.8])
            for _, da in _quats(km):
                qvel[r_zero, da:da + 3], qacc[r_zero, da:da + 3] = 0.0, 0.0
                qvel[r_tiny, da:da + 3], qacc[r_tiny, da:da + 3] = 1e-9 * u, 0.0
            status[r_num] = NUMERICAL
            qacc[r_nan, nv // 2] = np.nan
            frozen[[r_num, r_nan]] = True
        vnew = qvel + dt * qacc
        vnew[frozen] = qvel[frozen]

        ref = [np.zeros((nenv, nq)), np.zeros((nenv, nv)), np.zeros((nenv, nv))]
        for e in range(nenv):
            if frozen[e]:
                ref[0][e], ref[1][e] = gqn[e], gvn[e]
            else:
                ref[0][e], ref[1][e], ref[2][e] = rbr.step_vjp(km, qpos[e], qvel[e], qacc[e], dt,
                                                               gqn[e], gvn[e])
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=gpu)
        gq, gv, ga = nan(nenv, nq), nan(nenv, nv), nan(nenv, nv)
        kb.integrate_backward_into(dev(qpos), dev(vnew), dev(qacc), dt, status=dev(status),
                                   grad_qpos_new=dev(gqn), grad_qvel_new=dev(gvn), grad_qpos=gq,
                                   grad_qvel=gv, grad_qacc=ga)
        # strided accelerations and their gradient, and in place on the cotangents
        xbuf, gxbuf = dev(rng.standard_normal((nenv, nv + 7))), nan(nenv, nv + 7)
        xbuf[:, :nv] = dev(qacc)
        gq2, gv2 = dev(gqn), dev(gvn)
        kb.integrate_backward_into(dev(qpos), dev(vnew), xbuf[:, :nv], dt, status=dev(status),
                                   grad_qpos_new=gq2, grad_qvel_new=gv2, grad_qpos=gq2,
                                   grad_qvel=gv2, grad_qacc=gxbuf[:, :nv])
        torch.cuda.synchronize()
        assert torch.equal(gq, gq2) and torch.equal(gv, gv2) and torch.equal(ga, gxbuf[:, :nv])
        assert torch.isnan(gxbuf[:, nv:]).all()
        got = [t.cpu().numpy() for t in (gq, gv, ga)]
        for k, (g, r) in enumerate(zip(got, ref)):
            assert np.isfinite(g).all(), k
            e = errors(g, r)
            worst[k] = max(worst[k], e.max())
            assert e.max() <= TOL, (k, dt, int(e.argmax()), e.max())
        for e in np.nonzero(frozen)[0]:
            assert bitwise(got[0][e], gqn[e]) and bitwise(got[1][e], gvn[e])
            assert (got[2][e] == 0.0).all()
        scale = 1 + np.abs(got[0]).max(axis=1)
        for qa, _ in _quats(km):
            dot = np.einsum("ei,ei->e", got[0][:, qa:qa + 4], qpos[:, qa:qa + 4])
            assert (np.abs(dot)[~frozen] <= TOL * scale[~frozen]).all(), np.abs(dot).max()
        if rows and _quats(km):     # the limit and the series rows moved their rates' gradients
            qa, da = _quats(km)[0]
            for r in (r_zero, r_tiny):
                assert np.abs(got[1][r, da:da + 3] - gvn[r, da:da + 3]).max() > 1e-5
    print(f"\nstep adjoint {name} nenv={nenv}: worst qpos {worst[0]:.2e} qvel {worst[1]:.2e} "
          f"qacc {worst[2]:.2e}")


# ---- 2. the PD producer's adjoint ------------------------------------------------------------------

def pd_backward(nenv, ns, quat, quat_ref, per_env, gT, want=(True,) * 4):
    shapes = ((nenv, 3), (nenv, 4), (nenv, 3), (nenv, 3))
    outs = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") if w else None
            for s, w in zip(shapes, want)]
    keep = [dev(quat), dev(quat_ref), dev(gT)]
    gains = (ctypes.c_double * 4)(*GAINS)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = _lib.lib().osc_pd_base_targets_backward(
        nenv, ns, ptr(keep[0]), ptr(keep[1]), int(per_env), gains, ptr(keep[2]),
        *[ptr(o) for o in outs], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("nenv", [1, 5, 67])
def test_pd_adjoint_vs_the_torch_vjp(gpu, nenv, per_env):
    """osc_pd_base_targets_backward against rollout_backward_ref.pd_vjp, shared and per-env
    quaternion references, every env and output within 1e-11.  Rows 1 .. ns-1 of the targets are
    constants: their cotangents do not reach the outputs (bitwise).  A NULL output leaves the
    others bitwise unchanged.  Worst measured on an MI355X: 2.2e-16."""
    ns = 5
    rng = np.random.default_rng(40 + nenv)
    quat = rng.standard_normal((nenv, 4))
    qr = rng.standard_normal((nenv, 4) if per_env else (4,))
    gT = rng.standard_normal((nenv, ns, 6))
    got = pd_backward(nenv, ns, quat, qr, per_env, gT)
    worst = 0.0
    for e in range(nenv):
        ref = rbr.pd_vjp(ns, quat[e], np.zeros(3), qr[e] if per_env else qr, GAINS, gT[e])
        for g, r in zip(got, ref):
            err = np.abs(g[e] - r).max() / (1 + np.abs(r).max())
            worst = max(worst, err)
            assert err <= TOL, (e, err)
    row0 = gT.copy()
    row0[:, 1:] = 0.0
    for a, b in zip(got, pd_backward(nenv, ns, quat, qr, per_env, row0)):
        assert bitwise(a, b)
    for drop in range(4):
        part = pd_backward(nenv, ns, quat, qr, per_env, gT, want=[i != drop for i in range(4)])
        assert part[drop] is None
        assert all(bitwise(a, b) for i, (a, b) in enumerate(zip(part, got)) if i != drop)
    print(f"\npd adjoint nenv={nenv} per_env={per_env}: worst {worst:.2e}")


# ---- shared cases ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(robot):
    """NBIG envs of a robot: states, held targets, a mask with every count of loaded contacts,
    mass scales, per-env PD position references, cotangents on every slab (read-only)."""
    tree, kb, km, s, mdl = pair(robot)
    seed = 7 + len(robot)
    qpos, qvel = random_states(tree, NBIG, seed, joint_range=0.5, vel_scale=0.1)
    T = generate(robot, NBIG, seed, "standing", "ones")["T"]
    rng = np.random.default_rng(seed)
    mask = (rng.uniform(size=(NBIG, mdl.nc)) < 0.7).astype(np.float64)
    mask[:, 1] = 1.0
    mask[1] = 1.0
    ms = ker.draw(tree, NBIG, seed + 1)["mass_scale"]
    pos_ref = qpos[:, 0:3] + OFFSET
    cot = cpu.draw_cotangents(K, NBIG, km.nq, km.nv, mdl.nu, seed + 2)
    c = dict(qpos=qpos, qvel=qvel, T=T, mask=mask, ms=ms, pos_ref=pos_ref,
             quat_ref=np.array([1.0, 0.0, 0.0, 0.0]), cot=cot)
    for a in list(c.values())[:-1] + list(cot.values()):
        a.setflags(write=False)
    return c


def run(robot, mode, rows, nticks=K, want=("qpos0", "qvel0"), warm=False, kin_ms=True, cot=None,
        scale=1.0):
    """Forward rollout and backward on the rows `rows` of case(robot); name -> numpy, the forward
    RolloutResult under "res"."""
    tree, kb, km, s, mdl = pair(robot)
    c = case(robot)
    cot = c["cot"] if cot is None else cot
    kw = dict(T=dev(c["T"][rows])) if mode == "held" else \
        dict(pd=(dev(c["pos_ref"][rows]), c["quat_ref"].copy(), GAINS))
    kp = KinEnvParams(mass_scale=dev(c["ms"][rows])) if kin_ms else None
    res = kb.rollout(s, dev(c["qpos"][rows]), dev(c["qvel"][rows]), dev(c["mask"][rows]), nticks, DT,
                     warm=warm, history=True, kin_params=kp, **kw)
    g = kb.rollout_backward(s, res, dev(c["mask"][rows]), DT,
                            grad_qpos_hist=dev(scale * cot["qpos"][:nticks + 1, rows]),
                            grad_qvel_hist=dev(scale * cot["qvel"][:nticks + 1, rows]),
                            grad_tau_hist=dev(scale * cot["tau"][:nticks, rows]), kin_params=kp,
                            want=want, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in g.items()}
    out["res"] = res
    return out


# ---- 3. against the same kernels composed by hand --------------------------------------------------

def qmul_b(a, b):
    aw, ax, ay, az = a.unbind(1)
    bw, bx, by, bz = b.unbind(1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw],
                       dim=1)


def quat_step_b(q, wl):
    th = wl.square().sum(dim=1, keepdim=True).sqrt()    # no zero angle in these cases
    p = qmul_b(q, torch.cat([torch.cos(0.5 * th), torch.sin(0.5 * th) * wl / th], dim=1))
    return p / p.square().sum(dim=1, keepdim=True).sqrt()


def step_b(km, qpos, qvel, dv, dt):
    """The step in torch ops on the device, a batch at a time."""
    v = qvel + dt * dv
    parts = []
    for j in km.joints:
        qa, da = j["qadr"], j["dadr"]
        if j["type"] == "free":
            parts += [qpos[:, qa:qa + 3] + v[:, da:da + 3] * dt,
                      quat_step_b(qpos[:, qa + 3:qa + 7], v[:, da + 3:da + 6] * dt)]
        elif j["type"] == "ball":
            parts.append(quat_step_b(qpos[:, qa:qa + 4], v[:, da:da + 3] * dt))
        else:
            parts.append(qpos[:, qa:qa + 1] + v[:, da:da + 1] * dt)
    return torch.cat(parts, dim=1), v


def pd_b(ns, qpos, qvel, pos_ref, quat_ref, gains):
    kp_l, kd_l, kp_a, kd_a = gains
    n = qpos.shape[0]
    q = qpos[:, 3:7]
    conj = torch.cat([q[:, :1], -q[:, 1:]], dim=1)
    rot = qmul_b(quat_ref.expand(n, 4), conj)[:, 1:]
    row = torch.cat([kp_l * (pos_ref - qpos[:, 0:3]) - kd_l * qvel[:, 0:3],
                     kp_a * rot - kd_a * qvel[:, 3:6]], dim=1)
    return torch.cat([row.reshape(n, 1, 6), torch.zeros((n, ns - 1, 6), dtype=torch.float64,
                                                        device=qpos.device)], dim=1)


def pd_t(ns, qpos, qvel, pos_ref, quat_ref, gains):
    """pd_b's graph carrying the device producer's values: bitwise the targets the rollout and
    its backward feed their solves (pos_ref per env, quat_ref shared)."""
    ref = pd_b(ns, qpos, qvel, pos_ref, quat_ref, gains)
    n = qpos.shape[0]
    parts = [t.detach().contiguous() for t in (qpos[:, 0:3], qpos[:, 3:7], qvel[:, 0:3],
                                               qvel[:, 3:6], pos_ref, quat_ref)]
    Tk = torch.empty_like(ref)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().osc_pd_base_targets(
        n, ns, *[ptr(t) for t in parts[:5]], 1, ptr(parts[5]), 0, (ctypes.c_double * 4)(*gains),
        ptr(Tk), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return Tk + (ref - ref.detach())      # Tk + 0, exactly


def hand_composition(robot, mode, rows, nticks, ulps=0):
    """K autograd nodes of solve_differentiable_qpos (cold solves), the step and the producer in
    torch ops: the loop this feature replaces.  Gradients of the loss that weighs every slab of
    the three histories with case(robot)'s cotangents.  ulps: the initial joint angles moved by
    that many units in the last place (the reference's own sensitivity to rounding)."""
    from osc_amd.autograd import solve_differentiable_qpos
    tree, kb, km, s, mdl = pair(robot)
    c = case(robot)
    q0 = c["qpos"][rows].copy()
    for _ in range(ulps):
        q0[:, 7:] = np.nextafter(q0[:, 7:], np.inf)
    q = dev(q0).requires_grad_(True)
    v = dev(c["qvel"][rows]).requires_grad_(True)
    ms = dev(c["ms"][rows]).requires_grad_(True)
    T = dev(c["T"][rows]).requires_grad_(True)
    mask = dev(c["mask"][rows])
    pos_ref, quat_ref = dev(c["pos_ref"][rows]), dev(c["quat_ref"])
    qh, vh, th = [q], [v], []
    for _ in range(nticks):
        Tt = T if mode == "held" else pd_t(mdl.ns, qh[-1], vh[-1], pos_ref, quat_ref, GAINS)
        tau, x, status = solve_differentiable_qpos(s, kb, qh[-1], vh[-1], Tt, mask,
                                                   kin_params=KinEnvParams(mass_scale=ms))
        assert (status == 0).all(), status
        qn, vn = step_b(km, qh[-1], vh[-1], x[:, :km.nv], DT)
        qh.append(qn)
        vh.append(vn)
        th.append(tau)
    cot = c["cot"]
    loss = (torch.stack(qh) * dev(cot["qpos"][:nticks + 1, rows])).sum() + \
        (torch.stack(vh) * dev(cot["qvel"][:nticks + 1, rows])).sum()
    if nticks:
        loss = loss + (torch.stack(th) * dev(cot["tau"][:nticks, rows])).sum()
    leaves = dict(qpos0=q, qvel0=v)
    if nticks:
        leaves["kin.mass_scale"] = ms
        if mode == "held":
            leaves["T"] = T
    g = torch.autograd.grad(loss, list(leaves.values()))
    return {k: t.cpu().numpy() for k, t in zip(leaves, g)}, \
        dict(qpos=torch.stack(qh).detach(), qvel=torch.stack(vh).detach())


def checkpoint_composition(robot, mode, rows, res):
    """The same composition tick by tick on the forward's own checkpoints: for t = K-1 .. 0 one
    solve_differentiable_qpos node on history slab t, the step and the producer in torch ops, and
    autograd of  g_q . qpos' + g_v . qvel' + cot_tau[t] . tau.  Every solve and every backward
    kernel then sees bitwise the x the library's backward sees."""
    from osc_amd.autograd import solve_differentiable_qpos
    tree, kb, km, s, mdl = pair(robot)
    c = case(robot)
    cot = {k: dev(a[:, rows]) for k, a in c["cot"].items()}
    mask = dev(c["mask"][rows])
    pos_ref, quat_ref = dev(c["pos_ref"][rows]), dev(c["quat_ref"])
    nticks = res.status_hist.shape[0]
    gq, gv = cot["qpos"][nticks], cot["qvel"][nticks]
    sums = {}
    for t in range(nticks - 1, -1, -1):
        q = res.qpos_hist[t].clone().requires_grad_(True)
        v = res.qvel_hist[t].clone().requires_grad_(True)
        ms = dev(c["ms"][rows]).requires_grad_(True)
        T = dev(c["T"][rows]).requires_grad_(True)
        Tt = T if mode == "held" else pd_t(mdl.ns, q, v, pos_ref, quat_ref, GAINS)
        tau, x, status = solve_differentiable_qpos(s, kb, q, v, Tt, mask,
                                                   kin_params=KinEnvParams(mass_scale=ms))
        qn, vn = step_b(km, q, v, x[:, :km.nv], DT)
        loss = (qn * gq).sum() + (vn * gv).sum() + (tau * cot["tau"][t]).sum()
        leaves = [q, v, ms] + ([T] if mode == "held" else [])
        g = torch.autograd.grad(loss, leaves)
        gq, gv = g[0] + cot["qpos"][t], g[1] + cot["qvel"][t]
        for k, t_ in zip(("kin.mass_scale", "T"), g[2:]):
            sums[k] = t_ if k not in sums else sums[k] + t_
    out = dict(qpos0=gq, qvel0=gv, **sums)
    return {k: t.cpu().numpy() for k, t in out.items()}


# 10 x the worst measured on an MI355X against the checkpointed composition: 2.98e-11 (Go2, PD
# targets, grad mass_scale; held targets: 5.5e-16, every summand bitwise the library's).  In PD mode
# the producer's adjoint rounds differently in torch, the state adjoints of the later ticks differ in
# the last place, and the solve's backward carries that through its projected solve, whose own
# rounding noise on these envs is of this size (test_linearity_in_the_cotangents: 1.4e-9).
CKPT_BAR = 3e-10


@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_whole_backward_vs_the_hand_composition(gpu, robot, mode):
    """5 envs, K = 3, a loss on every slab of the three histories: grad qpos0, qvel0, mass_scale
    (and T, held) of osc_batch_rollout_backward against the same solve and kinematics backward
    kernels composed by hand with the step and the producer in torch ops (the producer's VALUES
    from its device kernel, so that the solves see bitwise the same targets), two ways:

    checkpointed   one solve_differentiable_qpos node per tick ON THE FORWARD'S HISTORY SLABS,
                   chained by hand.  Every kernel then sees the x the library's backward sees;
                   the two sides differ in the step's and the producer's adjoints' rounding and
                   in summation order alone.  Bar: CKPT_BAR, 10 x the measured worst (Go2 held
                   1.7e-16, PD 3.0e-11; WaLTER 5.5e-16).
    the loop       the torch loop of K autograd nodes from the initial state, which this feature
                   replaces.  Its states are the torch step's, which differ from the step kernel's
                   by one rounding (histories: 1.1e-16), so its solves do NOT see the same x: each
                   cold solve ends within the solver's ~1e-11 of the optimum, wherever it started.
                   Measured worst against it (held / PD): Go2 3.6e-10 / 3.2e-11, WaLTER 4.9e-8 /
                   4.9e-8 -- a finding, not a bar: the loop's OWN gradients move by as much when
                   its initial joint angles move by one unit in the last place (Go2 2.2e-10 /
                   2.3e-11, WaLTER 1.6e-7 / 1.6e-7; the worst output is grad qpos0, WaLTER's next
                   is grad mass_scale at 6.5e-9 against 9.5e-9),
                   while the checkpointed composition, on the same x, agrees to rounding.  So the
                   loop is held to 10 x its own one-ulp sensitivity, measured in the test: the
                   reference's own error.  (WaLTER's torso rows carry zero weight, so its PD
                   targets do not reach the solve: its two modes give the same figures.)"""
    rows = slice(0, 5)
    want = ("qpos0", "qvel0", "kin.mass_scale") + (("T",) if mode == "held" else ())
    got = run(robot, mode, rows, want=want)
    ref, hist = hand_composition(robot, mode, rows, K)
    ref1, _ = hand_composition(robot, mode, rows, K, ulps=1)
    ckpt = checkpoint_composition(robot, mode, rows, got["res"])
    assert (got["res"].status_hist == 0).all()
    dq = (got["res"].qpos_hist - hist["qpos"]).abs().max()
    worst = {k: errors(got[k], ref[k]).max() for k in want}
    noise = {k: errors(ref1[k], ref[k]).max() for k in want}
    wck = {k: errors(got[k], ckpt[k]).max() for k in want}
    print(f"\nhand composition {robot} {mode}: histories differ by {dq:.2e}")
    for k in want:
        print(f"  {k}: |ref| {np.abs(ref[k]).max():.2e}  vs loop {worst[k]:.2e}  loop's own 1-ulp "
              f"noise {noise[k]:.2e}  vs checkpointed {wck[k]:.2e}")
    assert dq <= 1e-14
    for k in want:
        assert np.abs(ref[k]).max() > 1e-3, k
        assert wck[k] <= CKPT_BAR, (k, wck[k])
        assert worst[k] <= max(10 * noise[k], CKPT_BAR), (k, worst[k], noise[k])


@pytest.mark.parametrize("mode", ["held", "pd"])
def test_one_tick_and_no_tick(gpu, mode):
    """K = 1 against the hand composition (one tick from the initial state: loop and checkpoints
    coincide, the same x) within CKPT_BAR (measured 1.9e-16); K = 0: the outputs are the slab-0 cotangents, bitwise,
    and the sums are zero."""
    rows = slice(0, 5)
    want = ("qpos0", "qvel0", "kin.mass_scale") + (("T",) if mode == "held" else ())
    got = run(GO2, mode, rows, nticks=1, want=want)
    ref, _ = hand_composition(GO2, mode, rows, 1)
    for k in want:
        e = errors(got[k], ref[k]).max()
        print(f"\none tick {mode} {k}: {e:.2e}")
        assert e <= CKPT_BAR, (k, e)
    got = run(GO2, mode, rows, nticks=0, want=want)
    cot = case(GO2)["cot"]
    assert bitwise(got["qpos0"], cot["qpos"][0, rows]) and bitwise(got["qvel0"], cot["qvel"][0, rows])
    for k in want[2:]:
        assert (got[k] == 0.0).all(), k


@pytest.mark.parametrize("mode", ["held", "pd"])
def test_warm_and_cold_forward_agree(gpu, mode):
    """The backward recomputes every tick cold; a warm-started forward's histories differ from a
    cold one's by the solver's ~1e-11, the gradients within NORM_TOL (backward_ref.env_errors;
    measured worst 7.8e-10 held, 1.6e-11 PD)."""
    rows = slice(0, 5)
    want = ("qpos0", "qvel0", "kin.mass_scale")
    cold = run(GO2, mode, rows, want=want, warm=False)
    warm = run(GO2, mode, rows, want=want, warm=True)
    for k in want:
        e = br.env_errors(warm[k], cold[k])
        print(f"\nwarm vs cold {mode} {k}: {e.max():.2e}")
        assert e.max() <= NORM_TOL, (k, e.max())


# ---- 4. against the CPU chain ------------------------------------------------------------------------

def test_held_mode_vs_the_cpu_chain(gpu):
    """Go2, 5 envs, K = 3, dt 0.002, the held case of tests/test_rollout_backward_ref.py (whose
    reference is pinned to finite differences there and asserts a certified optimum and a clean
    working set at every env and tick): grad qpos0, qvel0, T and mass_scale, every env, within
    NORM_TOL by backward_ref.env_errors; the forward histories within the chain's contract.
    Measured worst on an MI355X: grad qpos0 6.1e-9, qvel0 9.8e-11, T 9.1e-11, mass_scale 9.6e-10."""
    tree, mdl, qpos, qvel, T, mask, ms = cpu.held_case()
    cot, ref = cpu.held_chain()
    _, kb, km, s, _ = pair(GO2)
    kp = KinEnvParams(mass_scale=dev(ms))
    res = kb.rollout(s, dev(qpos), dev(qvel), dev(mask), K, DT, T=dev(T), history=True,
                     kin_params=kp)
    g = kb.rollout_backward(s, res, dev(mask), DT, T=dev(T), grad_qpos_hist=dev(cot["qpos"]),
                            grad_qvel_hist=dev(cot["qvel"]), grad_tau_hist=dev(cot["tau"]),
                            kin_params=kp, want=("qpos0", "qvel0", "T", "kin.mass_scale"))
    torch.cuda.synchronize()
    assert (res.status_hist == 0).all()
    qh = np.stack([r[1]["qpos"] for r in ref], axis=1)
    assert np.abs(res.qpos_hist.cpu().numpy() - qh).max() <= NORM_TOL
    for k, rk in (("qpos0", "qpos0"), ("qvel0", "qvel0"), ("T", "T"),
                  ("kin.mass_scale", "mass_scale")):
        r = np.stack([x[0][rk] for x in ref])
        e = br.env_errors(g[k].cpu().numpy(), r)
        print(f"\nheld chain {k}: worst {e.max():.3e} (env {e.argmax()})")
        assert e.max() <= NORM_TOL, (k, int(e.argmax()), e.max())


# PD mode.  Candidates: random_states(tree, 40, 7, joint_range=0.5, vel_scale=0.1); reference: each
# env's base position + OFFSET, the identity quaternion, the standing gains.  A foot whose normal
# force is zero at tick 0 with every contact on (|fz| <= 1e-6: it rests at the pyramid's apex) is
# masked off; the first five candidates for which the CPU reference's assertions then hold at all
# K ticks are kept -- here the first five drawn.  The reference re-asserts it on every run.
PD_CANDIDATES, PD_SEED = 40, 7
PD_ENVS = [0, 1, 2, 3, 4]
PD_MASK = [[1, 0, 1, 0], [0, 1, 1, 1], [1, 0, 0, 1], [1, 0, 1, 0], [1, 0, 0, 0]]


def test_pd_mode_vs_the_cpu_chain(gpu):
    """Go2, the five PD cases above, K = 3: grad qpos0 and qvel0, every env, within NORM_TOL.
    Measured worst on an MI355X: 1.4e-13 and 3.3e-15."""
    tree, kb, km, s, mdl = pair(GO2)
    qpos, qvel = random_states(tree, PD_CANDIDATES, PD_SEED, joint_range=0.5, vel_scale=0.1)
    qpos, qvel = qpos[PD_ENVS], qvel[PD_ENVS]
    mask = np.array(PD_MASK, dtype=np.float64)
    n = len(PD_ENVS)
    quat_ref = np.array([1.0, 0.0, 0.0, 0.0])
    pos_ref = qpos[:, 0:3] + OFFSET
    cot = cpu.draw_cotangents(K, n, km.nq, km.nv, mdl.nu, 19)
    ref = [rbr.chain(tree, mdl, qpos[e], qvel[e], mask[e], K, DT, cpu.env_cot(cot, e),
                     pd=(pos_ref[e], quat_ref, GAINS), where=e)[0] for e in range(n)]
    pd = (dev(pos_ref), quat_ref, GAINS)
    res = kb.rollout(s, dev(qpos), dev(qvel), dev(mask), K, DT, pd=pd, history=True)
    g = kb.rollout_backward(s, res, dev(mask), DT, pd=pd, grad_qpos_hist=dev(cot["qpos"]),
                            grad_qvel_hist=dev(cot["qvel"]), grad_tau_hist=dev(cot["tau"]))
    torch.cuda.synchronize()
    assert (res.status_hist == 0).all()
    for k in ("qpos0", "qvel0"):
        e = br.env_errors(g[k].cpu().numpy(), np.stack([r[k] for r in ref]))
        print(f"\npd chain {k}: worst {e.max():.3e} (env {e.argmax()})")
        assert e.max() <= NORM_TOL, (k, int(e.argmax()), e.max())


# Per-env QP parameters: w_pos = the model's x uniform(0.5, 2), fz_ub = uniform(20, 60) from
# default_rng(ENV_SEED) -- the first seed from 20 on for which the CPU reference's assertions hold
# for all five envs of the held case (a cap on fz puts several envs' contacts on the cap).
ENV_SEED = 28


def test_env_parameter_gradients_vs_the_cpu_chain(gpu):
    """EnvParams(w_pos, fz_ub) on the held case: their gradients, and grad qpos0 / qvel0, against
    backward_env_ref through the CPU chain, every env, within NORM_TOL.  Measured worst on an
    MI355X: grad qpos0 1.2e-13, qvel0 5.3e-16, w_pos 5.4e-14, fz_ub 6.7e-14."""
    tree, mdl, qpos, qvel, T, mask, ms = cpu.held_case()
    cot, _ = cpu.held_chain()
    _, kb, km, s, _ = pair(GO2)
    rng = np.random.default_rng(ENV_SEED)
    w_pos = np.asarray(mdl.w_pos) * rng.uniform(0.5, 2.0, (cpu.NENV, mdl.ns))
    fz_ub = rng.uniform(20.0, 60.0, cpu.NENV)
    ref = []
    for e in range(cpu.NENV):
        me = load_model(GO2, overrides=dict(
            w_pos=[float(v) for v in w_pos[e]],
            z_ub=[float(mdl.z_ub[0]), float(mdl.z_ub[1]), float(fz_ub[e])]))
        ref.append(rbr.chain(tree, me, qpos[e], qvel[e], mask[e], K, DT, cpu.env_cot(cot, e),
                             T=T[e], env=True, where=e)[0])
    ep = EnvParams(w_pos=dev(w_pos), fz_ub=dev(fz_ub))
    res = kb.rollout(s, dev(qpos), dev(qvel), dev(mask), K, DT, T=dev(T), history=True,
                     env_params=ep)
    g = kb.rollout_backward(s, res, dev(mask), DT, T=dev(T), grad_qpos_hist=dev(cot["qpos"]),
                            grad_qvel_hist=dev(cot["qvel"]), grad_tau_hist=dev(cot["tau"]),
                            env_params=ep, want=("qpos0", "qvel0", "env.w_pos", "env.fz_ub"))
    torch.cuda.synchronize()
    assert (res.status_hist == 0).all()
    assert sum(abs(float(r["fz_ub"])) > 1e-3 for r in ref) >= 2     # the cap is felt
    for k, rk in (("qpos0", "qpos0"), ("qvel0", "qvel0"), ("env.w_pos", "w_pos"),
                  ("env.fz_ub", "fz_ub")):
        r = np.stack([np.atleast_1d(x[rk]) for x in ref])
        e = br.env_errors(g[k].cpu().numpy().reshape(r.shape), r)
        print(f"\nenv chain {k}: worst {e.max():.3e} (env {e.argmax()})")
        assert e.max() <= NORM_TOL, (k, int(e.argmax()), e.max())


# ---- 5. structure ------------------------------------------------------------------------------------

WANT_ALL = ("qpos0", "qvel0", "T", "kin.mass_scale")


@pytest.mark.parametrize("mode", ["held", "pd"])
def test_batch_independence_and_reproducibility(gpu, mode):
    """An env alone is bitwise what it is inside 33; two identical calls are bitwise equal."""
    want = WANT_ALL if mode == "held" else tuple(k for k in WANT_ALL if k != "T")
    full = run(GO2, mode, slice(0, NBIG), want=want)
    again = run(GO2, mode, slice(0, NBIG), want=want)
    for k in want:
        assert bitwise(full[k], again[k]), k
    for e in (0, 15, 16, 32):
        one = run(GO2, mode, slice(e, e + 1), want=want)
        for k in want:
            assert bitwise(one[k], full[k][e:e + 1]), (e, k)


def test_linearity_in_the_cotangents(gpu):
    """Each history's cotangent alone sums to all three together, and 2 x the cotangents give 2 x
    the gradients.  Both are held to the contract, NORM_TOL with backward_ref.env_errors, as the linearity tests of the
    solve's backward it chains (tests/test_gpu_backward_data.py, test_gpu_backward_env.py): that
    pass's projected solve is where the parts round differently.  Measured on an MI355X: the sum
    6.4e-10 (qpos0), 2.1e-11 (qvel0), 4.2e-11 (T), 1.4e-9 (mass_scale); the scaling exact."""
    rows = slice(0, 5)
    cot = case(GO2)["cot"]
    whole = run(GO2, "held", rows, want=WANT_ALL)
    parts = [run(GO2, "held", rows, want=WANT_ALL,
                 cot={k: (v if k == only else np.zeros_like(v)) for k, v in cot.items()})
             for only in cot]
    twice = run(GO2, "held", rows, want=WANT_ALL, scale=2.0)
    for k in WANT_ALL:
        e = br.env_errors(sum(p[k] for p in parts), whole[k]).max()
        print(f"\nlinearity {k}: {e:.2e}")
        assert e <= NORM_TOL, k
        e2 = br.env_errors(twice[k], 2.0 * whole[k]).max()
        print(f"scaling by 2 {k}: {e2:.2e} (bitwise: {bitwise(twice[k], 2.0 * whole[k])})")
        assert e2 <= NORM_TOL, k


def test_null_outputs_leave_the_others_unchanged(gpu):
    rows = slice(0, 5)
    full = run(GO2, "held", rows, want=WANT_ALL)
    for drop in WANT_ALL:
        part = run(GO2, "held", rows, want=tuple(k for k in WANT_ALL if k != drop))
        assert drop not in part
        for k in WANT_ALL:
            assert k == drop or bitwise(part[k], full[k]), (drop, k)
    for only in WANT_ALL:
        assert bitwise(run(GO2, "held", rows, want=(only,))[only], full[only]), only


def test_sums_are_the_tick_ordered_sums_of_one_tick_calls(gpu):
    """grad_T and grad mass_scale of the K-tick call equal, bitwise, the sum in the order K-1 .. 0
    (from zero) of K one-tick calls, each seeded with the state adjoints of the call before it;
    the state adjoints that come out of the last one are grad_qpos0 / grad_qvel0, bitwise."""
    tree, kb, km, s, mdl = pair(GO2)
    c = case(GO2)
    rows = slice(0, 5)
    whole = run(GO2, "held", rows, want=WANT_ALL)
    res = whole["res"]
    cot = {k: dev(v[:, rows]) for k, v in c["cot"].items()}
    mask, T = dev(c["mask"][rows]), dev(c["T"][rows])
    kp = KinEnvParams(mass_scale=dev(c["ms"][rows]))
    gq, gv = cot["qpos"][K], cot["qvel"][K]
    sums = {k: torch.zeros_like(dev(whole[k])) for k in ("T", "kin.mass_scale")}
    for t in range(K - 1, -1, -1):
        one = RolloutResult(None, None, None, None, qpos_hist=res.qpos_hist[t:t + 2].contiguous(),
                            qvel_hist=res.qvel_hist[t:t + 2].contiguous(),
                            tau_hist=res.tau_hist[t:t + 1].contiguous(),
                            status_hist=res.status_hist[t:t + 1].contiguous())
        g = kb.rollout_backward(s, one, mask, DT, T=T,
                                grad_qpos_hist=torch.stack([cot["qpos"][t], gq]),
                                grad_qvel_hist=torch.stack([cot["qvel"][t], gv]),
                                grad_tau_hist=cot["tau"][t:t + 1].contiguous(), kin_params=kp,
                                want=WANT_ALL)
        gq, gv = g["qpos0"], g["qvel0"]
        for k in sums:
            sums[k] = sums[k] + g[k]
    torch.cuda.synchronize()
    assert bitwise(gq.cpu().numpy(), whole["qpos0"]) and bitwise(gv.cpu().numpy(), whole["qvel0"])
    for k in sums:
        assert bitwise(sums[k].cpu().numpy(), whole[k]), k


def test_a_frozen_env_passes_its_cotangents_through(gpu):
    """An env with an invalid mass scale is NUMERICAL at every tick: its state never moves, its
    grad_qpos0 / grad_qvel0 are the sums of its slabs' cotangents in the order K .. 0, its T and
    parameter gradients are zero, and every other env is bitwise unaffected."""
    tree, kb, km, s, mdl = pair(GO2)
    c = case(GO2)
    rows = slice(0, 5)
    good = run(GO2, "held", rows, want=WANT_ALL)
    ms = c["ms"][rows].copy()
    ms[2, 3] = -1.0
    kp = KinEnvParams(mass_scale=dev(ms))
    mask, T = dev(c["mask"][rows]), dev(c["T"][rows])
    res = kb.rollout(s, dev(c["qpos"][rows]), dev(c["qvel"][rows]), mask, K, DT, T=T, warm=False,
                     history=True, kin_params=kp)
    cot = {k: v[:, rows] for k, v in c["cot"].items()}
    g = kb.rollout_backward(s, res, mask, DT, T=T, grad_qpos_hist=dev(cot["qpos"]),
                            grad_qvel_hist=dev(cot["qvel"]), grad_tau_hist=dev(cot["tau"]),
                            kin_params=kp, want=WANT_ALL)
    torch.cuda.synchronize()
    assert (res.status_hist[:, 2] == NUMERICAL).all()
    g = {k: v.cpu().numpy() for k, v in g.items()}
    for k, name in (("qpos0", "qpos"), ("qvel0", "qvel")):
        acc = cot[name][K, 2]
        for t in range(K - 1, -1, -1):
            acc = acc + cot[name][t, 2]
        assert bitwise(g[k][2], acc), k
    assert (g["T"][2] == 0.0).all() and (g["kin.mass_scale"][2] == 0.0).all()
    others = [0, 1, 3, 4]
    for k in WANT_ALL:
        assert bitwise(g[k][others], good[k][others]), k


# ---- 6. memory and refusals --------------------------------------------------------------------------

def raw_call(kb, s, a, ep=None, kp=None):
    return _lib.lib().osc_batch_rollout_backward(
        s._h, kb._h, a._nenv, ctypes.byref(a), ep, kp,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def raw_args(nenv, nticks, tensors, mode="held"):
    """osc_rollout_backward_args from a dict of device tensors named as its fields (absent =
    NULL)."""
    a = _lib.OscRolloutBackwardArgs()
    a._nenv = nenv
    a.nticks, a.dt = nticks, DT
    a.target_mode = _lib.ROLLOUT_TARGETS_HELD if mode == "held" else _lib.ROLLOUT_TARGETS_PD_BASE
    a.gains[:] = GAINS
    for k, t in tensors.items():
        if k == "workspace":
            a.workspace, a.workspace_bytes = t.data_ptr(), t.numel() * t.element_size()
        elif k in ("pos_ref_per_env", "quat_ref_per_env"):
            setattr(a, k, t)
        else:
            setattr(a, k, t.data_ptr())
    a._keep = tensors
    return a


@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("nenv", [5, 17])
def test_no_access_outside_the_arrays(gpu, nenv, mode):
    """Every input, cotangent, output and the workspace between guard bands at its exact size: the
    bands intact, the inputs unmodified, the results bitwise the ordinary call's whether the bands
    around the inputs hold 0x00 or 0xFF."""
    tree, kb, km, s, mdl = pair(GO2)
    c = case(GO2)
    rows = slice(0, nenv)
    want = ("qpos0", "qvel0", "kin.mass_scale", "env.w_pos") + (("T",) if mode == "held" else ())
    w_pos = np.asarray(mdl.w_pos) * np.random.default_rng(3).uniform(0.5, 2.0, (nenv, mdl.ns))
    ep, kp = EnvParams(w_pos=dev(w_pos)), KinEnvParams(mass_scale=dev(c["ms"][rows]))
    kw = dict(T=dev(c["T"][rows])) if mode == "held" else \
        dict(pd=(dev(c["pos_ref"][rows]), c["quat_ref"].copy(), GAINS))
    res = kb.rollout(s, dev(c["qpos"][rows]), dev(c["qvel"][rows]), dev(c["mask"][rows]), K, DT,
                     warm=False, history=True, env_params=ep, kin_params=kp, **kw)
    cot = {k: dev(v[:, rows]) for k, v in c["cot"].items()}
    ref = kb.rollout_backward(s, res, dev(c["mask"][rows]), DT, grad_qpos_hist=cot["qpos"],
                              grad_qvel_hist=cot["qvel"], grad_tau_hist=cot["tau"], env_params=ep,
                              kin_params=kp, want=want, **kw)
    torch.cuda.synchronize()
    shape = {"qpos0": (nenv, km.nq), "qvel0": (nenv, km.nv), "T": (nenv, mdl.ns, 6),
             "kin.mass_scale": (nenv, kb.nbody), "env.w_pos": (nenv, mdl.ns)}
    nbytes = kb.rollout_backward_workspace_bytes(s, nenv)
    for pad in (0x00, 0xFF):
        fill = 0xA5 if pad == 0 else 0x5A
        ins = dict(contact_mask=dev(c["mask"][rows]), qpos_hist=res.qpos_hist,
                   qvel_hist=res.qvel_hist, status_hist=res.status_hist,
                   grad_qpos_hist=cot["qpos"], grad_qvel_hist=cot["qvel"],
                   grad_tau_hist=cot["tau"], w_pos=dev(w_pos), mass_scale=dev(c["ms"][rows]))
        if mode == "held":
            ins["T"] = dev(c["T"][rows])
        else:
            ins["pos_ref"], ins["quat_ref"] = dev(c["pos_ref"][rows]), dev(c["quat_ref"])
        ins = {k: guarded_like(v, pad) for k, v in ins.items()}
        kept = {k: v.clone() for k, v in ins.items()}
        o = {k: guarded(shape[k], torch.float64, gpu, fill=fill) for k in want}
        ws = guarded((nbytes // 8,), torch.float64, gpu, fill=fill, env_bytes=nbytes // nenv)
        t = {k: v for k, v in ins.items() if k not in ("w_pos", "mass_scale")}
        t.update(grad_qpos0=o["qpos0"], grad_qvel0=o["qvel0"], workspace=ws)
        if mode == "held":
            t["grad_T"] = o["T"]
        else:
            t["pos_ref_per_env"] = 1
        a = raw_args(nenv, K, t, mode)
        eg = _lib.OscEnvGrads(w_pos=o["env.w_pos"].data_ptr())
        kg = _lib.OscKinEnvGrads(mass_scale=o["kin.mass_scale"].data_ptr())
        a.env_grads, a.kin_grads = ctypes.pointer(eg), ctypes.pointer(kg)
        cep = _lib.OscEnvParams(w_pos=ins["w_pos"].data_ptr())
        ckp = _lib.OscKinEnvParams(mass_scale=ins["mass_scale"].data_ptr())
        assert raw_call(kb, s, a, ctypes.byref(cep), ctypes.byref(ckp)) == 0
        torch.cuda.synchronize()
        for k in want:
            assert_guards_intact(o[k], k)
            assert torch.equal(o[k], ref[k]), (k, hex(pad))
        assert_guards_intact(ws, "workspace")
        for k, v in ins.items():
            assert_guards_intact(v, "input " + k)
            assert torch.equal(v, kept[k]), k


@pytest.mark.parametrize("nenv", [5, 17])
def test_step_and_pd_adjoints_stay_inside_their_arrays(gpu, nenv):
    """The two small entries alone, every array between guard bands at its exact size."""
    tree, kb, km = kin_of(GO2)
    L = _lib.lib()
    rng = np.random.default_rng(60 + nenv)
    qpos, qvel = random_states(tree, nenv, 23, base_pos_zero=False)
    qacc = rng.standard_normal((nenv, km.nv))
    src = dict(qpos=qpos, vnew=qvel + DT * qacc, qacc=qacc, gqn=rng.standard_normal(qpos.shape),
               gvn=rng.standard_normal(qvel.shape), status=np.zeros(nenv, np.int32),
               quat=qpos[:, 3:7], qr=rng.standard_normal((nenv, 4)),
               gT=rng.standard_normal((nenv, 5, 6)))
    oshape = dict(gq=(nenv, km.nq), gv=(nenv, km.nv), ga=(nenv, km.nv), bp=(nenv, 3),
                  bq=(nenv, 4), bl=(nenv, 3), ba=(nenv, 3))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gains = (ctypes.c_double * 4)(*GAINS)
    results = []
    for pad in (0x00, 0xFF):
        i = {k: guarded_like(dev(v), pad) for k, v in src.items()}
        kept = {k: v.clone() for k, v in i.items()}
        o = {k: guarded(s, torch.float64, gpu, fill=0xA5 if pad == 0 else 0x5A)
             for k, s in oshape.items()}
        assert L.osc_batch_integrate_backward(
            kb._h, nenv, DT, ptr(i["qpos"]), ptr(i["vnew"]), ptr(i["status"]), ptr(i["qacc"]), km.nv,
            ptr(i["gqn"]), ptr(i["gvn"]), ptr(o["gq"]), ptr(o["gv"]), ptr(o["ga"]), km.nv,
            stream) == 0
        assert L.osc_pd_base_targets_backward(
            nenv, 5, ptr(i["quat"]), ptr(i["qr"]), 1, gains, ptr(i["gT"]), ptr(o["bp"]),
            ptr(o["bq"]), ptr(o["bl"]), ptr(o["ba"]), stream) == 0
        torch.cuda.synchronize()
        for k, t in o.items():
            assert_guards_intact(t, k)
            assert torch.isfinite(t).all(), k
        for k, t in i.items():
            assert_guards_intact(t, "input " + k)
            assert torch.equal(t, kept[k]), k
        results.append({k: t.clone() for k, t in o.items()})
    for k in oshape:
        assert torch.equal(results[0][k], results[1][k]), k


def test_refusals_leave_the_outputs_untouched(gpu):
    """OSC_ERR_INVALID_ARGUMENT with nothing enqueued and every output untouched for: a model with
    wheel rows, PD targets on a hinge-rooted tree, a bad dt, nticks < 0, an unknown target mode, a
    missing T / reference / mask / history, grad_T asked in PD mode, every output NULL, a
    misaligned pointer, a misaligned or short workspace."""
    from test_gpu_wheels import NOSLIP_YAML
    tree, kb, km, s, mdl = pair(GO2)
    c = case(GO2)
    n = 5
    rows = slice(0, n)
    SENT = -12345.0
    res = kb.rollout(s, dev(c["qpos"][rows]), dev(c["qvel"][rows]), dev(c["mask"][rows]), K, DT,
                     T=dev(c["T"][rows]), history=True)
    full = lambda *sh: torch.full(sh, SENT, dtype=torch.float64, device=gpu)
    o = dict(grad_qpos0=full(n, km.nq), grad_qvel0=full(n, km.nv), grad_T=full(n, mdl.ns, 6))
    eg_t = full(n, mdl.ns)
    ws = torch.empty(kb.rollout_backward_workspace_bytes(s, n) // 8 + 2, dtype=torch.float64,
                     device=gpu)
    base = dict(T=dev(c["T"][rows]), contact_mask=dev(c["mask"][rows]), qpos_hist=res.qpos_hist,
                qvel_hist=res.qvel_hist, status_hist=res.status_hist,
                grad_qpos_hist=dev(c["cot"]["qpos"][:, rows]), workspace=ws, **o)
    pdk = dict(pos_ref=dev(c["pos_ref"][rows]), quat_ref=dev(c["quat_ref"]), pos_ref_per_env=1)

    def args(drop=(), mode="held", **kw):
        t = {k: v for k, v in dict(base, **kw).items() if k not in drop}
        a = raw_args(n, K, t, mode)
        return a

    def untouched():
        torch.cuda.synchronize()
        return all((t == SENT).all() for t in o.values()) and (eg_t == SENT).all()

    cases = {}
    a = args(); a.dt = 0.0; cases["dt = 0"] = a
    a = args(); a.dt = -DT; cases["dt < 0"] = a
    a = args(); a.dt = float("nan"); cases["dt NaN"] = a
    a = args(); a.nticks = -1; cases["nticks < 0"] = a
    a = args(); a.target_mode = 7; cases["unknown target mode"] = a
    for k in ("T", "contact_mask", "qpos_hist", "qvel_hist", "status_hist"):
        cases["missing " + k] = args(drop=(k,))
    cases["missing pos_ref"] = args(drop=("T", "grad_T", "pos_ref"), mode="pd", **pdk)
    cases["missing quat_ref"] = args(drop=("T", "grad_T", "quat_ref"), mode="pd", **pdk)
    cases["grad_T in PD mode"] = args(mode="pd", **pdk)
    cases["every output NULL"] = args(drop=tuple(o))
    a = args(drop=tuple(o)); eg = _lib.OscEnvGrads(); a.env_grads = ctypes.pointer(eg)
    cases["every output NULL, an empty env_grads"] = a
    for k in ("T", "qpos_hist", "grad_qpos_hist", "grad_qvel0"):
        a = args()
        setattr(a, k, getattr(a, k) + 4)
        cases["odd " + k] = a
    a = args(); a.workspace += 8; cases["misaligned workspace"] = a
    a = args(); a.workspace_bytes -= 4096; cases["short workspace"] = a
    a = args(); odd = _lib.OscEnvGrads(w_pos=eg_t.data_ptr() + 4); a.env_grads = ctypes.pointer(odd)
    cases["odd parameter gradient"] = a
    for what, a in cases.items():
        assert raw_call(kb, s, a) == 1, what
        assert untouched(), what
    a = args()
    odd_p = _lib.OscKinEnvParams(mass_scale=ws.data_ptr() + 4)
    assert raw_call(kb, s, a, kp=ctypes.byref(odd_p)) == 1 and untouched()
    assert _lib.lib().osc_batch_rollout_backward(None, kb._h, n, ctypes.byref(a), None, None,
                                                 None) == 1
    assert _lib.lib().osc_batch_rollout_backward(s._h, kb._h, n, None, None, None, None) == 1
    assert _lib.lib().osc_batch_rollout_backward(s._h, kb._h, -1, ctypes.byref(a), None, None,
                                                 None) == 1
    assert untouched()
    # a model with wheel rows; PD targets on a hinge-rooted tree of WaLTER's sizes
    _, kw_, kmw, sw, mw = pair(WALTER)
    wheels = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)
    cw = case(WALTER)
    resw = kw_.rollout(sw, dev(cw["qpos"][rows]), dev(cw["qvel"][rows]), dev(cw["mask"][rows]), 1,
                       DT, T=dev(cw["T"][rows]), history=True)
    ow = dict(grad_qpos0=full(n, kmw.nq), grad_qvel0=full(n, kmw.nv))
    tw = dict(T=dev(cw["T"][rows]), contact_mask=dev(cw["mask"][rows]), qpos_hist=resw.qpos_hist,
              qvel_hist=resw.qvel_hist, status_hist=resw.status_hist, **ow)
    assert raw_call(kw_, wheels, raw_args(n, 1, tw)) == 1
    hinged = random_tree(4, nbody=14, free_root=False, nsite=17, weld_p=0.0)
    kh = KinematicsBatch(tree=hinged)
    assert (kh.nq, kh.nv) == (14, 14)
    th = dict(contact_mask=dev(cw["mask"][rows]), qpos_hist=full(2, n, 14), qvel_hist=full(2, n, 14),
              status_hist=resw.status_hist, grad_qpos0=full(n, 14), grad_qvel0=full(n, 14),
              pos_ref=dev(cw["pos_ref"][rows]), quat_ref=dev(cw["quat_ref"]), pos_ref_per_env=1)
    assert raw_call(kh, sw, raw_args(n, 1, th, "pd")) == 1
    torch.cuda.synchronize()
    assert all((t == SENT).all() for t in ow.values())
    assert (th["grad_qpos0"] == SENT).all() and (th["grad_qvel0"] == SENT).all()
    # nenv == 0 and a good call
    a = args()
    a._nenv = 0
    assert raw_call(kb, s, a) == 0 and untouched()
    a = args()
    assert raw_call(kb, s, a) == 0
    torch.cuda.synchronize()
    assert not any((t == SENT).any() for t in o.values())


# ---- 7. autograd -------------------------------------------------------------------------------------

def test_gradcheck(gpu):
    """torch.autograd.gradcheck of rollout_differentiable on two Go2 envs of the held case, K = 2,
    with respect to qpos, qvel, T and mass_scale (eps 1e-6, atol 1e-5, as the existing ones)."""
    from osc_amd.autograd import rollout_differentiable
    tree, mdl, qpos, qvel, T, mask, ms = cpu.held_case()
    _, kb, km, s, _ = pair(GO2)
    e = [1, 4]
    leaves = [dev(a[e]).requires_grad_(True) for a in (qpos, qvel, T, ms)]
    m = dev(mask[e])

    def fn(q, v, t, scale):
        out = rollout_differentiable(s, kb, q, v, m, 2, DT, T=t, warm=False,
                                     kin_params=KinEnvParams(mass_scale=scale))
        return out[:3]

    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-5)


def test_autograd_fills_only_what_is_asked(gpu):
    from osc_amd.autograd import rollout_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    c = case(GO2)
    rows = slice(0, 5)
    cot = {k: dev(v[:, rows]) for k, v in c["cot"].items()}
    mask = dev(c["mask"][rows])
    q = dev(c["qpos"][rows]).requires_grad_(True)
    v = dev(c["qvel"][rows])
    T = dev(c["T"][rows]).requires_grad_(True)
    ms = dev(c["ms"][rows])
    w = dev(np.broadcast_to(np.asarray(mdl.w_pos), (5, mdl.ns)).copy()).requires_grad_(True)
    kp, ep = KinEnvParams(mass_scale=ms), EnvParams(w_pos=w)
    qh, vh, th, st = rollout_differentiable(s, kb, q, v, mask, K, DT, T=T, env_params=ep,
                                            kin_params=kp)
    plain = kb.rollout(s, q.detach(), v, mask, K, DT, T=T.detach(), history=True, env_params=ep,
                       kin_params=kp)
    torch.cuda.synchronize()
    for a, b in ((qh, plain.qpos_hist), (vh, plain.qvel_hist), (th, plain.tau_hist),
                 (st, plain.status_hist)):
        assert torch.equal(a.detach(), b)
    assert not st.requires_grad
    ((qh * cot["qpos"]).sum() + (vh * cot["qvel"]).sum() + (th * cot["tau"]).sum()).backward()
    assert v.grad is None and ms.grad is None
    ref = kb.rollout_backward(s, plain, mask, DT, T=T.detach(), grad_qpos_hist=cot["qpos"],
                              grad_qvel_hist=cot["qvel"], grad_tau_hist=cot["tau"], env_params=ep,
                              kin_params=kp, want=("qpos0", "T", "env.w_pos"))
    assert torch.equal(q.grad, ref["qpos0"]) and torch.equal(T.grad, ref["T"])
    assert torch.equal(w.grad, ref["env.w_pos"]) and w.grad.abs().max() > 0
    # PD targets: gradients to the state alone; a loss on the last slab only
    v2 = dev(c["qvel"][rows]).requires_grad_(True)
    pd = (dev(c["pos_ref"][rows]), c["quat_ref"].copy(), GAINS)
    qh, vh, th, st = rollout_differentiable(s, kb, q.detach(), v2, mask, K, DT, pd=pd)
    (qh[-1, :, 0:3] - pd[0]).square().sum().backward()
    assert v2.grad is not None and torch.isfinite(v2.grad).all() and v2.grad.abs().max() > 0
    with pytest.raises(ValueError):
        rollout_differentiable(s, kb, q, v, mask, K, DT, T=T, kin_params=KinEnvParams(
            mass_scale=torch.ones((5, kb.nbody), dtype=torch.float64, requires_grad=True)))
    with pytest.raises(ValueError):
        rollout_differentiable(s, kb, q, v, mask, K, DT, T=T, pd=pd)
    with pytest.raises(TypeError):
        rollout_differentiable(s, kb, q, v, mask, K, DT, T=T, kin_params=dict(mass_scale=ms))
