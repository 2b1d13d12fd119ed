"""GPU tests of the scheduled rollout (include/osc_rollout_schedule.h,
csrc/osc_rollout_schedule.hip; KinematicsBatch.rollout / rollout_backward with schedule= and
osc_amd.autograd.rollout_differentiable):
   1. the forward bitwise against the loop a user would write from the existing entries;
   2. its reductions to the plain rollout: no schedule, a schedule of identical slabs, K = 0 and 1;
   3. the backward against the same GPU kernels composed by hand in a torch loop;
   4. the backward against the CPU chain (tests/rollout_schedule_ref.py, exact solver);
   5. the producer's parameter adjoint alone against the torch VJP;
   6. structure: grad_T as the tick-ordered sum of grad_T_seq, batch independence,
      reproducibility, NULL outputs, a frozen env;
   7. guard bands (tests/guard.py) around every new input, output and both workspaces;
   8. refusals;
   9. autograd: gradcheck, what gets a gradient, the forward's values.

Errors and bars as tests/test_gpu_rollout_backward.py: |g - g_ref|_inf / (1 + |g_ref|_inf) per env
against 1e-11 for the producer's adjoint and 10 x the measured worst for the hand composition;
backward_ref.env_errors at NORM_TOL = 1e-5 against the CPU chain."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import backward_ref as br
import rollout_ref
import rollout_schedule_ref as rsr
import test_gpu_rollout_backward as tb
import test_rollout_schedule_ref as scpu
from guard import assert_guards_intact, guarded, guarded_like
from osc_amd import _lib
from osc_amd.kinematics import KinEnvParams, RolloutSchedule, random_states
from osc_amd.solver import EnvParams
from osc_amd.synth import generate

pytestmark = pytest.mark.gpu

TOL = 1e-11
NORM_TOL = scpu.NORM_TOL
# 10 x the worst measured on an MI355X against the checkpointed hand composition, the rule of
# tests/test_gpu_rollout_backward.py's CKPT_BAR: 2.00e-14 (Go2, PD targets, grad qpos0).  Per output,
# Go2 held / PD: qpos0 2.2e-16 / 2.0e-14, qvel0 7.8e-17 / 1.2e-15, T_seq 1.1e-16 / 3.0e-15,
# pos_ref_seq 5.2e-15, quat_ref_seq 1.2e-14, gains 2.3e-15; WaLTER: qpos0 4.0e-16, every other
# output bitwise (its torso rows carry no weight: the reference and gain gradients are zero).
# Smaller than that file's 3e-10 because nothing here goes through a parameter gradient of the
# solve's backward (its mass_scale), whose projected solve is where that file's noise comes from.
CKPT_BAR = 2e-13
DT = rollout_ref.DT
GO2, WALTER = "unitree_go2", "walter_sr"
GAINS = rollout_ref.STANDING_GAINS
K4 = 4            # the forward's tests
K = scpu.K        # the backward's: 3
NBIG = 33         # two full 16-env blocks and a one-env tail
NUMERICAL = _lib.SOLVE_NUMERICAL

dev, bitwise, errors, pair = tb.dev, tb.bitwise, tb.errors, tb.pair


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ---- the forward's inputs: K4 ticks, every schedule field ---------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(robot, nenv, nticks=K4):
    """Read-only arrays of a forward case: states, held T / mask / references, and a schedule of
    nticks slabs: a feed-forward, a mask that lifts contact (e mod nc) of env e at tick 1 and puts
    it back at tick 3 (every env restarts cold twice under a warm start), per-env position
    references on a ramp and a shared quaternion reference that drifts."""
    tree, kb, km, s, mdl = pair(robot)
    seed = 31
    qpos, qvel = random_states(tree, nenv, seed, base_pos_zero=False, joint_range=0.5,
                               vel_scale=0.1)
    rng = np.random.default_rng(seed)
    c = dict(qpos=qpos, qvel=qvel, T=generate(robot, nenv, seed, "standing", "ones")["T"],
             mask=np.ones((nenv, mdl.nc)),
             pos_ref=qpos[:, :3] + 0.02 * rng.standard_normal((nenv, 3)),
             quat_ref=np.array([1.0, 0.0, 0.0, 0.0]))
    c["T_seq"] = 0.05 * rng.standard_normal((nticks, nenv, mdl.ns, 6))
    m = np.ones((nticks, nenv, mdl.nc))
    m[1:3, np.arange(nenv), np.arange(nenv) % mdl.nc] = 0.0
    c["mask_seq"] = m
    ramp = (np.arange(1, nticks + 1) / max(nticks, 1))[:, None, None]
    c["pos_ref_seq"] = c["pos_ref"][None] + ramp * scpu.OFFSET
    q = np.array([[1.0, 0.01 * (t + 1), -0.005 * (t + 1), 0.002 * t] for t in range(nticks)])
    c["quat_ref_seq"] = q / np.linalg.norm(q, axis=1, keepdims=True).reshape(-1, 1) \
        if nticks else q.reshape(0, 4)
    for a in c.values():
        a.setflags(write=False)
    return c


FIELDS = {"held": (("T",), ("mask",), ("T", "mask")),
          "pd": (("T",), ("mask",), ("pos_ref",), ("quat_ref",),
                 ("T", "mask", "pos_ref", "quat_ref"))}
MODE_FIELDS = [(m, f) for m in ("held", "pd") for f in FIELDS[m]]


def schedule_of(c, fields):
    return RolloutSchedule(**{f: c[f + "_seq"] for f in fields})


def user_loop(robot, c, mode, fields, nticks, warm):
    """The loop a user would write from the existing entries: per tick the producer (PD mode) on the
    tick's references, a torch add of T_seq[t], solve_(warm_)into with the tick's mask, then
    integrate_into (tests/test_gpu_rollout.py::_user_loop with per-tick inputs)."""
    tree, kb, km, s, mdl = pair(robot)
    nenv, nv, ns = c["qpos"].shape[0], km.nv, mdl.ns
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    qp, qv = dev(c["qpos"]), dev(c["qvel"])
    out = s.alloc_outputs(nenv, want_x=True)
    wstate = s.alloc_warm_state(nenv)
    ws = torch.empty((kb.workspace_bytes(s, nenv) // 8 + 2,), dtype=torch.float64, device="cuda")
    bad = torch.zeros(nenv, dtype=torch.int32, device="cuda")
    gains = (ctypes.c_double * 4)(*GAINS)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = dict(qpos=[qp.clone()], qvel=[qv.clone()], tau=[], status=[])
    for t in range(nticks):
        md = dev(c["mask_seq"][t] if "mask" in fields else c["mask"])
        if mode == "pd":
            pref = dev(c["pos_ref_seq"][t] if "pos_ref" in fields else c["pos_ref"])
            qref = dev(c["quat_ref_seq"][t] if "quat_ref" in fields else c["quat_ref"])
            Td = torch.empty((nenv, ns, 6), dtype=torch.float64, device="cuda")
            base = [qp[:, 0:3].contiguous(), qp[:, 3:7].contiguous(), qv[:, 0:3].contiguous(),
                    qv[:, 3:6].contiguous()]
            rc = _lib.lib().osc_pd_base_targets(nenv, ns, *[p(x) for x in base], p(pref), 1,
                                                p(qref), 0, gains, p(Td), stream)
            assert rc == 0
        else:
            Td = dev(c["T"])
        if "T" in fields:
            Td = Td + dev(c["T_seq"][t])
        if warm:
            kb.solve_warm_into(s, out, wstate, qp, qv, Td, md, ws)
        else:
            kb.solve_into(s, out, qp, qv, Td, md, ws)
        h["tau"].append(out.tau.clone())
        h["status"].append(out.status.clone())
        kb.integrate_into(qp, qv, out.x[:, :nv], DT, status=out.status, bad_ticks=bad)
        h["qpos"].append(qp.clone())
        h["qvel"].append(qv.clone())
    torch.cuda.synchronize()
    return {k: torch.stack(v) for k, v in h.items()}, bad


def same_rollout(r, ref, bad=None):
    ok = torch.equal(r.qpos_hist, ref["qpos"]) and torch.equal(r.qvel_hist, ref["qvel"]) and \
        torch.equal(r.tau_hist, ref["tau"]) and torch.equal(r.status_hist, ref["status"]) and \
        torch.equal(r.qpos, ref["qpos"][-1]) and torch.equal(r.qvel, ref["qvel"][-1])
    return ok and (bad is None or torch.equal(r.bad_ticks, bad))


def as_ref(res):
    return dict(qpos=res.qpos_hist, qvel=res.qvel_hist, tau=res.tau_hist, status=res.status_hist)


def held_kw(c, mode):
    return dict(T=c["T"]) if mode == "held" else dict(pd=(c["pos_ref"], c["quat_ref"], GAINS))


# ---- 1. bitwise against the user loop ------------------------------------------------------------------

@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("mode,fields", MODE_FIELDS)
@pytest.mark.parametrize("robot,nenv", [(GO2, NBIG), (WALTER, 5)])
def test_forward_bitwise_vs_the_user_loop(gpu, robot, nenv, mode, fields, warm):
    """Four ticks of osc_batch_rollout_sched with each schedule field alone and all together, held
    and PD targets, warm and cold: histories, statuses, bad_ticks and the final state bitwise the
    user loop's.  The mask schedule flips a contact of every env at ticks 1 and 3: under a warm
    start those envs restart cold and are still bitwise.  A caller workspace and the library's
    scratch agree; the caller's arrays are not modified."""
    tree, kb, km, s, mdl = pair(robot)
    c = inputs(robot, nenv)
    kept = {k: v.copy() for k, v in c.items()}
    sch = schedule_of(c, fields)
    kw = held_kw(c, mode)
    res = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, history=True,
                     schedule=sch, **kw)
    res2 = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, history=True,
                      workspace=None, schedule=sch, **kw)
    ref, bad = user_loop(robot, c, mode, fields, K4, warm)
    torch.cuda.synchronize()
    assert all(np.array_equal(c[k], kept[k]) for k in c)
    assert same_rollout(res, ref, bad) and same_rollout(res2, ref, bad)
    assert (res.status_hist == 0).all()
    plain = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, history=True, **kw)
    if robot == GO2 or "T" in fields or "mask" in fields:   # the schedule is felt (WaLTER's torso
        assert not torch.equal(plain.qpos_hist, res.qpos_hist)   # rows carry no weight: not its
                                                                  # PD references)
    res3 = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, schedule=sch, **kw)
    torch.cuda.synchronize()
    assert torch.equal(res3.qpos, res.qpos) and torch.equal(res3.tau, res.tau)


# ---- 2. reductions to the existing entry ---------------------------------------------------------------

@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("mode", ["held", "pd"])
def test_reductions_to_the_plain_rollout(gpu, mode, warm):
    """An empty schedule is bitwise rollout(); so is a schedule of K identical slabs of the held
    values with the held arguments omitted (T, the mask, both references: pointer offsets only);
    K = 1 likewise, and K = 0 returns the input state with slab 0 written."""
    tree, kb, km, s, mdl = pair(GO2)
    for nticks in (K4, 1, 0):
        c = inputs(GO2, NBIG, nticks)
        kw = held_kw(c, mode)
        plain = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], nticks, DT, warm=warm, history=True,
                           **kw)
        empty = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], nticks, DT, warm=warm, history=True,
                           schedule=RolloutSchedule(), **kw)
        tile = lambda a: np.broadcast_to(a, (nticks,) + a.shape).copy()
        if mode == "held":
            sch = RolloutSchedule(T=tile(c["T"]), mask=tile(c["mask"]))
            same = kb.rollout(s, c["qpos"], c["qvel"], None, nticks, DT, warm=warm, history=True,
                              schedule=sch)
        else:
            sch = RolloutSchedule(mask=tile(c["mask"]), pos_ref=tile(c["pos_ref"]),
                                  quat_ref=tile(c["quat_ref"]))
            same = kb.rollout(s, c["qpos"], c["qvel"], None, nticks, DT, warm=warm, history=True,
                              pd=(None, None, GAINS), schedule=sch)
        torch.cuda.synchronize()
        for r in (empty, same):
            assert same_rollout(r, as_ref(plain), plain.bad_ticks), nticks
            assert torch.equal(r.tau, plain.tau)
        if nticks == 0:
            assert torch.equal(empty.qpos, dev(c["qpos"])) and empty.qpos_hist.shape[0] == 1


@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("robot,nenv", [(GO2, 17), (WALTER, 5)])
def test_backward_reductions_to_the_plain_backward(gpu, robot, nenv, mode):
    """The backward's reduction: osc_batch_rollout_backward and osc_batch_rollout_backward_sched
    on one forward (tb.case's inputs, K = 3, per-env mass scales, task weights and force caps),
    the second with the held mask tiled K times as its schedule and no held mask, the same
    cotangents on all three histories: every gradient the plain entry gives -- qpos0, qvel0, T
    (held targets), env.w_pos, env.fz_ub, kin.mass_scale -- bitwise equal.  17 Go2 envs are one
    full 16-env block and a one-env tail."""
    tree, kb, km, s, mdl = pair(robot)
    c = tb.case(robot)
    rows = slice(0, nenv)
    rng = np.random.default_rng(5)
    ep = EnvParams(w_pos=dev(np.asarray(mdl.w_pos) * rng.uniform(0.5, 2.0, (nenv, mdl.ns))),
                   fz_ub=dev(float(mdl.z_ub[2]) * rng.uniform(0.6, 1.2, nenv)))
    kp = KinEnvParams(mass_scale=dev(c["ms"][rows]))
    kw = dict(T=c["T"][rows]) if mode == "held" else \
        dict(pd=(c["pos_ref"][rows], c["quat_ref"], GAINS))
    mask = c["mask"][rows]
    res = kb.rollout(s, c["qpos"][rows], c["qvel"][rows], mask, K, DT, warm=False, history=True,
                     env_params=ep, kin_params=kp, **kw)
    want = ("qpos0", "qvel0", "env.w_pos", "env.fz_ub", "kin.mass_scale") + \
        (("T",) if mode == "held" else ())
    bw = dict(grad_qpos_hist=dev(c["cot"]["qpos"][:, rows]),
              grad_qvel_hist=dev(c["cot"]["qvel"][:, rows]),
              grad_tau_hist=dev(c["cot"]["tau"][:, rows]), env_params=ep, kin_params=kp,
              want=want, **kw)
    plain = kb.rollout_backward(s, res, mask, DT, **bw)
    tiled = np.broadcast_to(mask, (K,) + mask.shape).copy()
    sched = kb.rollout_backward(s, res, None, DT, schedule=RolloutSchedule(mask=tiled), **bw)
    torch.cuda.synchronize()
    assert set(plain) == set(sched) == set(want)
    for k in want:
        assert torch.isfinite(plain[k]).all(), k
        assert bitwise(plain[k].cpu().numpy(), sched[k].cpu().numpy()), k
    if robot == GO2:
        assert all(plain[k].abs().max() > 0 for k in ("qpos0", "qvel0", "kin.mass_scale"))


# ---- the backward's shared case: NBIG envs, K ticks ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def bcase(robot):
    """tests/test_gpu_rollout_backward.py's case(robot) (states, masks with every count of loaded
    contacts, per-env position references, cotangents) with a schedule on top: a feed-forward,
    the case's mask with contact 0 toggled at tick 1 and back at tick 2 (contact 1 is on in every
    env throughout), per-env position references on a ramp and a shared drifting quaternion
    reference."""
    c = dict(tb.case(robot))
    n = c["qpos"].shape[0]
    mdl = pair(robot)[4]
    rng = np.random.default_rng(77)
    c["T_seq"] = 0.05 * rng.standard_normal((K, n, mdl.ns, 6))
    m = np.broadcast_to(c["mask"], (K, n, mdl.nc)).copy()
    m[1, :, 0] = 1.0 - m[1, :, 0]          # contact 0 changes state at tick 1 and goes back at 2
    c["mask_seq"] = m
    ramp = (np.arange(1, K + 1) / K)[:, None, None]
    c["pos_ref_seq"] = c["qpos"][None, :, 0:3] + ramp * scpu.OFFSET
    c["quat_ref_seq"] = scpu.sched_case(robot)["quat_ref_seq"]
    for k in ("T_seq", "mask_seq", "pos_ref_seq"):
        c[k].setflags(write=False)
    return c


SEQ_WANT = ("qpos0", "qvel0", "T_seq", "pos_ref_seq", "quat_ref_seq", "gains")
HELD_WANT = ("qpos0", "qvel0", "T_seq", "pos_ref", "quat_ref", "gains")


def brun(robot, rows, seq=True, mode="pd", want=None, warm=False, raw=False, ms=None):
    """Forward with the schedule of bcase(robot) on `rows` and the scheduled backward.  PD targets
    with a feed-forward and a mask schedule, the references per tick (seq) or held; or held
    targets T + T_seq.  name -> numpy (raw: the library's per-env outputs, through the C entry),
    the forward RolloutResult under "res"."""
    tree, kb, km, s, mdl = pair(robot)
    c = bcase(robot)
    want = want or (SEQ_WANT if seq else HELD_WANT)
    sl = lambda a: a[:, rows]
    sch = RolloutSchedule(T=sl(c["T_seq"]), mask=sl(c["mask_seq"]))
    if mode == "pd" and seq:
        sch.pos_ref, sch.quat_ref = sl(c["pos_ref_seq"]), c["quat_ref_seq"]
        kw = dict(pd=(None, None, GAINS))
    elif mode == "pd":
        kw = dict(pd=(c["pos_ref"][rows], c["quat_ref"], GAINS))
    else:
        kw = dict(T=c["T"][rows])
    kp = None if ms is None else KinEnvParams(mass_scale=dev(ms))
    res = kb.rollout(s, c["qpos"][rows], c["qvel"][rows], None, K, DT, warm=warm, history=True,
                     schedule=sch, kin_params=kp, **kw)
    cot = {k: dev(v[:, rows]) for k, v in c["cot"].items()}
    g = kb.rollout_backward(s, res, None, DT, grad_qpos_hist=cot["qpos"],
                            grad_qvel_hist=cot["qvel"], grad_tau_hist=cot["tau"], want=want,
                            schedule=sch, kin_params=kp, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in g.items()}
    out["res"] = res
    return out


# ---- 3. against the same kernels composed by hand ----------------------------------------------------

def pd_t(ns, qpos, qvel, pos_ref, quat_ref, gains_t):
    """tb.pd_b's graph (now also through the references and a tensor of gains) carrying the device
    producer's values, as tb.pd_t."""
    ref = tb.pd_b(ns, qpos, qvel, pos_ref, quat_ref, gains_t)
    n = qpos.shape[0]
    parts = [t.detach().contiguous() for t in (qpos[:, 0:3], qpos[:, 3:7], qvel[:, 0:3],
                                               qvel[:, 3:6], pos_ref, quat_ref)]
    Tk = torch.empty_like(ref)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().osc_pd_base_targets(
        n, ns, *[ptr(t) for t in parts[:5]], 1, ptr(parts[5]), 0, (ctypes.c_double * 4)(*GAINS),
        ptr(Tk), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return Tk + (ref - ref.detach())      # Tk + 0, exactly


def checkpoint_composition(robot, rows, res, mode):
    """tb.checkpoint_composition with per-tick inputs: for t = K-1 .. 0 one
    solve_differentiable_qpos node on history slab t with the tick's mask, the producer on the
    tick's references plus T_seq[t] (a torch add), the step in torch ops; autograd of
    g_q . qpos' + g_v . qvel' + cot_tau[t] . tau with respect to the state, T_seq[t], the tick's
    references and the gains."""
    from osc_amd.autograd import solve_differentiable_qpos
    tree, kb, km, s, mdl = pair(robot)
    c = bcase(robot)
    cot = {k: dev(a[:, rows]) for k, a in c["cot"].items()}
    gq, gv = cot["qpos"][K], cot["qvel"][K]
    n = gq.shape[0]
    out = dict(T_seq=[None] * K, pos_ref_seq=[None] * K, quat_ref_seq=[None] * K,
               gains=torch.zeros(4, dtype=torch.float64, device="cuda"))
    for t in range(K - 1, -1, -1):
        q = res.qpos_hist[t].clone().requires_grad_(True)
        v = res.qvel_hist[t].clone().requires_grad_(True)
        ff = dev(c["T_seq"][t, rows]).requires_grad_(True)
        leaves = [q, v, ff]
        if mode == "pd":
            pr = dev(c["pos_ref_seq"][t, rows]).requires_grad_(True)
            qr = dev(c["quat_ref_seq"][t]).requires_grad_(True)
            gn = dev(np.array(GAINS)).requires_grad_(True)
            Tt = pd_t(mdl.ns, q, v, pr, qr, gn) + ff
            leaves += [pr, qr, gn]
        else:
            Tt = dev(c["T"][rows]) + ff
        tau, x, status = solve_differentiable_qpos(s, kb, q, v, Tt, dev(c["mask_seq"][t, rows]))
        qn, vn = tb.step_b(km, q, v, x[:, :km.nv], DT)
        loss = (qn * gq).sum() + (vn * gv).sum() + (tau * cot["tau"][t]).sum()
        g = torch.autograd.grad(loss, leaves)
        gq, gv = g[0] + cot["qpos"][t], g[1] + cot["qvel"][t]
        out["T_seq"][t] = g[2]
        if mode == "pd":
            out["pos_ref_seq"][t], out["quat_ref_seq"][t] = g[3], g[4]
            out["gains"] = out["gains"] + g[5]
    ref = dict(qpos0=gq, qvel0=gv, T_seq=torch.stack(out["T_seq"]))
    if mode == "pd":
        ref.update(pos_ref_seq=torch.stack(out["pos_ref_seq"]),
                   quat_ref_seq=torch.stack(out["quat_ref_seq"]), gains=out["gains"])
    return {k: t.cpu().numpy() for k, t in ref.items()}


@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_backward_vs_the_hand_composition(gpu, robot, mode):
    """5 envs, K = 3, a loss on every slab of the three histories, a feed-forward, a mask schedule
    and (PD) reference sequences: grad qpos0, qvel0, T_seq and (PD) pos_ref_seq, quat_ref_seq,
    gains of osc_batch_rollout_backward_sched against the checkpointed hand composition of
    tests/test_gpu_rollout_backward.py -- the same solve and kinematics backward kernels on the
    forward's history slabs, the producer and the step in torch ops.  Both sides see the same x;
    they differ in the adjoints' rounding and summation order.  Bar: CKPT_BAR above, 10 x the
    measured worst (2.0e-14), that file's rule.  Per-tick outputs are compared per tick."""
    rows = slice(0, 5)
    want = SEQ_WANT if mode == "pd" else ("qpos0", "qvel0", "T_seq")
    got = brun(robot, rows, seq=True, mode=mode, want=want)
    assert (got["res"].status_hist == 0).all()
    ref = checkpoint_composition(robot, rows, got["res"], mode)
    for k in want:
        g, r = got[k], ref[k]
        if k == "gains":
            e = np.abs(g - r).max() / (1 + np.abs(r).max())
        elif k == "quat_ref_seq":      # shared: (K, 4), one row per tick
            e = errors(g, r).max()
        elif k.endswith("_seq"):       # (K, nenv, ...): per tick and env
            e = max(errors(g[t], r[t]).max() for t in range(K))
        else:
            e = errors(g, r).max()
        print(f"\nhand composition {robot} {mode} {k}: |ref| {np.abs(r).max():.2e} err {e:.2e}")
        assert e <= CKPT_BAR, (k, e)
    if robot == GO2:
        assert all(np.abs(ref[k]).max() > 1e-3 for k in want)


# ---- 4. against the CPU chain ----------------------------------------------------------------------------

def chain_run(robot, seq, mode="pd"):
    tree, kb, km, s, mdl = pair(robot)
    c = scpu.sched_case(robot)
    sch = RolloutSchedule(T=c["ff"], mask=c["masks"])
    if mode == "held":
        kw, want = {}, ("qpos0", "qvel0", "T_seq")
    elif seq:
        sch.pos_ref, sch.quat_ref = c["pos_ref_seq"], c["quat_ref_seq"]
        kw, want = dict(pd=(None, None, GAINS)), SEQ_WANT
    else:
        kw, want = dict(pd=(c["pos_ref"], c["quat_ref"], GAINS)), HELD_WANT
    res = kb.rollout(s, c["qpos"], c["qvel"], None, K, DT, history=True, schedule=sch, **kw)
    cot = {k: dev(v) for k, v in c["cot"].items()}
    g = kb.rollout_backward(s, res, None, DT, grad_qpos_hist=cot["qpos"],
                            grad_qvel_hist=cot["qvel"], grad_tau_hist=cot["tau"], want=want,
                            schedule=sch, **kw)
    torch.cuda.synchronize()
    assert (res.status_hist == 0).all()
    return res, {k: v.cpu().numpy() for k, v in g.items()}, want


@pytest.mark.parametrize("seq", [False, True])
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_pd_schedule_vs_the_cpu_chain(gpu, robot, seq):
    """5 envs, K = 3, PD targets + feed-forward + the mask schedule of
    tests/test_rollout_schedule_ref.py (whose reference is pinned to finite differences there and
    asserts a clean working set at every env and tick): grad qpos0, qvel0, grad_T_seq per tick,
    and grad pos_ref / quat_ref / gains (held references) or pos_ref_seq / quat_ref_seq per tick
    (sequences), every env, within NORM_TOL by backward_ref.env_errors.  The shared quaternion
    reference's and the gains' gradients are sums over the envs: compared as one row.
    Measured worst on an MI355X, held references / sequences.  Go2: qpos0 6.9e-11 / 2.5e-10, qvel0
    2.5e-12 / 4.8e-12, T_seq 6.1e-11 / 6.5e-11, pos_ref 3.0e-13 / 4.1e-12, quat_ref 2.7e-11 /
    8.6e-11, gains 2.7e-11 / 2.0e-11.  WaLTER: qpos0 1.1e-7, qvel0 3.5e-11, T_seq 2.5e-9; its
    reference and gain gradients are zero on both sides (the torso rows carry no weight)."""
    res, g, want = chain_run(robot, seq)
    ref = scpu.sched_chain(robot, seq)
    qh = np.stack([r[1]["qpos"] for r in ref], axis=1)
    assert np.abs(res.qpos_hist.cpu().numpy() - qh).max() <= NORM_TOL
    for k in want:
        r = np.stack([x[0][k] for x in ref])            # (nenv, ...)
        if k in ("gains", "quat_ref"):                  # shared: the wrapper's sum over the envs
            e = br.env_errors(g[k][None], r.sum(0)[None])
        elif k == "quat_ref_seq":                       # shared, per tick: (K, 4)
            e = br.env_errors(g[k], r.sum(0))
        elif k.endswith("_seq"):                        # (K, nenv, ...) against (nenv, K, ...)
            e = np.concatenate([br.env_errors(g[k][t], r[:, t]) for t in range(K)])
        else:
            e = br.env_errors(g[k], r)
        assert np.isfinite(g[k]).all()
        if not np.abs(r).max():     # WaLTER's torso rows carry no weight: a zero reference has no
            e = np.abs(g[k]).max()  # scale for env_errors; held to NORM_TOL x 1 in absolute value
            print(f"\nchain {robot} seq={seq} {k}: the reference is zero, |g| {e:.3e}")
            assert e <= NORM_TOL, k
            continue
        print(f"\nchain {robot} seq={seq} {k}: worst {e.max():.3e}")
        assert e.max() <= NORM_TOL, (k, int(e.argmax()), e.max())


@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_held_target_sequence_vs_the_cpu_chain(gpu, robot):
    """Held mode with T omitted: tick t's targets are schedule.T[t] (a target sequence to
    optimise).  grad_T_seq per tick, grad qpos0 and qvel0 within NORM_TOL of the CPU chain.
    Measured worst on an MI355X: Go2 4.7e-10 / 1.8e-12 / 6.7e-12 (qpos0 / qvel0 / T_seq), WaLTER
    1.1e-7 / 3.5e-11 / 2.5e-9."""
    res, g, want = chain_run(robot, False, mode="held")
    ref = scpu.held_sched_chain(robot)
    for k in want:
        r = np.stack([x[0][k] for x in ref])
        e = np.concatenate([br.env_errors(g[k][t], r[:, t]) for t in range(K)]) \
            if k == "T_seq" else br.env_errors(g[k], r)
        print(f"\nheld chain {robot} {k}: worst {e.max():.3e}")
        assert e.max() <= NORM_TOL, (k, int(e.argmax()), e.max())


# ---- 5. the producer's parameter adjoint -------------------------------------------------------------

def pd_params_backward(nenv, ns, st, pr, qr, per_env, gT, want=(True,) * 3):
    shapes = ((nenv, 3), (nenv, 4), (nenv, 4))
    outs = [nan(*sh) if w else None for sh, w in zip(shapes, want)]
    keep = [dev(a) for a in (*st, pr, qr, gT)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = _lib.lib().osc_pd_base_targets_backward_params(
        nenv, ns, *[ptr(t) for t in keep[:5]], int(per_env), ptr(keep[5]), int(per_env),
        (ctypes.c_double * 4)(*GAINS), ptr(keep[6]), *[ptr(o) for o in outs],
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("nenv", [1, 5, 67])
def test_pd_parameter_adjoint_vs_the_torch_vjp(gpu, nenv, per_env):
    """osc_pd_base_targets_backward_params against rollout_schedule_ref.pd_param_vjp, shared and
    per-env references, every env and output within 1e-11; the outputs are per env either way.
    Rows 1 .. ns-1 of the cotangent do not reach the outputs (bitwise); a NULL output leaves the
    others bitwise unchanged.  Measured worst on an MI355X: 6.1e-16 (nenv 67, per-env references)."""
    ns = 5
    rng = np.random.default_rng(70 + nenv)
    st = [rng.standard_normal((nenv, w)) for w in (3, 4, 3, 3)]
    pr = rng.standard_normal((nenv, 3) if per_env else (3,))
    qr = rng.standard_normal((nenv, 4) if per_env else (4,))
    gT = rng.standard_normal((nenv, ns, 6))
    got = pd_params_backward(nenv, ns, st, pr, qr, per_env, gT)
    worst = 0.0
    for e in range(nenv):
        ref = rsr.pd_param_vjp(ns, *(a[e] for a in st), pr[e] if per_env else pr,
                               qr[e] if per_env else qr, GAINS, gT[e])
        for g, r in zip(got, ref):
            err = np.abs(g[e] - r).max() / (1 + np.abs(r).max())
            worst = max(worst, err)
            assert err <= TOL, (e, err)
    row0 = gT.copy()
    row0[:, 1:] = 0.0
    for a, b in zip(got, pd_params_backward(nenv, ns, st, pr, qr, per_env, row0)):
        assert bitwise(a, b)
    for keepers in itertools.product([True, False], repeat=3):
        if not any(keepers) or all(keepers):
            continue
        part = pd_params_backward(nenv, ns, st, pr, qr, per_env, gT, want=keepers)
        for i, w in enumerate(keepers):
            assert (part[i] is None) if not w else bitwise(part[i], got[i])
    print(f"\npd parameter adjoint nenv={nenv} per_env={per_env}: worst {worst:.2e}")


# ---- 6. structure --------------------------------------------------------------------------------------

def test_grad_T_is_the_tick_ordered_sum_of_grad_T_seq(gpu):
    """Held mode, T + T_seq: bargs->grad_T is bitwise ((0 + g[K-1]) + ...) + g[0] of grad_T_seq,
    formed in torch in that order; and grad_T_seq does not change when grad_T is not asked for."""
    rows = slice(0, NBIG)
    both = brun(GO2, rows, mode="held", want=("qpos0", "T", "T_seq"))
    acc = torch.zeros_like(dev(both["T"]))
    for t in range(K - 1, -1, -1):
        acc = acc + dev(both["T_seq"][t])
    assert bitwise(acc.cpu().numpy(), both["T"])
    assert np.abs(both["T"]).max() > 1e-3
    only = brun(GO2, rows, mode="held", want=("T_seq",))
    assert bitwise(only["T_seq"], both["T_seq"])


@pytest.mark.parametrize("seq", [False, True])
def test_batch_independence_and_reproducibility(gpu, seq):
    """An env's per-env outputs (through the C entry: before the wrapper's sums over the envs) are
    bitwise the same alone and inside 33; two identical calls are bitwise equal."""
    full = raw_backward(GO2, slice(0, NBIG), seq)
    again = raw_backward(GO2, slice(0, NBIG), seq)
    for k in full:
        assert bitwise(full[k], again[k]), k
    for e in (0, 15, 16, 32):
        one = raw_backward(GO2, slice(e, e + 1), seq)
        for k in full:
            f = full[k][:, e:e + 1] if k.endswith("_seq") else full[k][e:e + 1]
            assert bitwise(one[k], f), (e, k)


RAW_SHAPES = dict(grad_T_seq=lambda n, d: (K, n, d["ns"], 6), grad_pos_ref=lambda n, d: (n, 3),
                  grad_quat_ref=lambda n, d: (n, 4), grad_pos_ref_seq=lambda n, d: (K, n, 3),
                  grad_quat_ref_seq=lambda n, d: (K, n, 4), grad_gains=lambda n, d: (n, 4))


def raw_setup(robot, rows, seq, mode="pd", ms=None, guard_pad=None):
    """The forward through the wrapper and the C structs of the scheduled backward on bcase(robot):
    (a, sc, tensors, res).  guard_pad: every input between guard bands of that byte."""
    tree, kb, km, s, mdl = pair(robot)
    c = bcase(robot)
    n = c["qpos"][rows].shape[0]
    sl = lambda a: np.ascontiguousarray(a[:, rows])
    sch = RolloutSchedule(T=sl(c["T_seq"]), mask=sl(c["mask_seq"]))
    if mode == "pd" and seq:
        sch.pos_ref, sch.quat_ref = sl(c["pos_ref_seq"]), c["quat_ref_seq"]
        kw = dict(pd=(None, None, GAINS))
    elif mode == "pd":
        kw = dict(pd=(c["pos_ref"][rows], c["quat_ref"], GAINS))
    else:
        kw = dict(T=c["T"][rows])
    kp = None if ms is None else KinEnvParams(mass_scale=dev(ms))
    res = kb.rollout(s, c["qpos"][rows], c["qvel"][rows], None, K, DT, warm=False, history=True,
                     schedule=sch, kin_params=kp, **kw)
    torch.cuda.synchronize()
    wrap = (lambda t: t) if guard_pad is None else (lambda t: guarded_like(t, guard_pad))
    t = dict(qpos_hist=wrap(res.qpos_hist), qvel_hist=wrap(res.qvel_hist),
             status_hist=wrap(res.status_hist),
             grad_qpos_hist=wrap(dev(c["cot"]["qpos"][:, rows])),
             grad_qvel_hist=wrap(dev(c["cot"]["qvel"][:, rows])),
             grad_tau_hist=wrap(dev(c["cot"]["tau"][:, rows])))
    st = dict(T_seq=wrap(dev(sch.T)), mask_seq=wrap(dev(sch.mask)))
    if mode == "pd" and seq:
        st.update(pos_ref_seq=wrap(dev(sch.pos_ref)), quat_ref_seq=wrap(dev(sch.quat_ref)))
    elif mode == "pd":
        t.update(pos_ref=wrap(dev(c["pos_ref"][rows])), quat_ref=wrap(dev(c["quat_ref"])))
    else:
        t["T"] = wrap(dev(c["T"][rows]))
    if mode == "pd":
        t["pos_ref_per_env"] = 1
    a = tb.raw_args(n, K, t, mode)
    sc = _lib.OscRolloutSchedule(**{k: v.data_ptr() for k, v in st.items()})
    sc._keep = st
    return a, sc, dict(t, **st), res


def raw_call(robot, a, sc, sg, kp=None):
    tree, kb, km, s, mdl = pair(robot)
    return _lib.lib().osc_batch_rollout_backward_sched(
        s._h, kb._h, a._nenv, ctypes.byref(a), ctypes.byref(sc) if sc is not None else None,
        ctypes.byref(sg) if sg is not None else None, None, kp,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def raw_names(seq, mode="pd"):
    if mode == "held":
        return ("grad_T_seq",)
    return ("grad_T_seq", "grad_gains") + (("grad_pos_ref_seq", "grad_quat_ref_seq") if seq else
                                           ("grad_pos_ref", "grad_quat_ref"))


def raw_backward(robot, rows, seq, mode="pd", names=None, state=True, ms=None):
    """The library's own outputs (per env) of the scheduled backward, name -> numpy."""
    tree, kb, km, s, mdl = pair(robot)
    a, sc, t, res = raw_setup(robot, rows, seq, mode, ms=ms)
    n = a._nenv
    names = raw_names(seq, mode) if names is None else names
    o = {k: nan(*RAW_SHAPES[k](n, s.dims)) for k in names}
    if state:
        o["grad_qpos0"], o["grad_qvel0"] = nan(n, km.nq), nan(n, km.nv)
        a.grad_qpos0, a.grad_qvel0 = o["grad_qpos0"].data_ptr(), o["grad_qvel0"].data_ptr()
    sg = _lib.OscRolloutScheduleGrads(**{k: o[k].data_ptr() for k in names})
    ckp = None
    if ms is not None:
        msd = dev(ms)
        ckp = ctypes.byref(_lib.OscKinEnvParams(mass_scale=msd.data_ptr()))
    assert raw_call(robot, a, sc, sg, ckp) == 0
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    assert all(np.isfinite(v).all() for v in out.values())
    return out


@pytest.mark.parametrize("seq", [False, True])
def test_null_outputs_leave_the_others_unchanged(gpu, seq):
    """Every subset of the schedule's outputs (with and without the state gradients) gives bitwise
    what the full call gives for the outputs it keeps."""
    rows = slice(0, 5)
    full = raw_backward(GO2, rows, seq)
    names = raw_names(seq)
    for r in range(0, len(names)):
        for sub in itertools.combinations(names, r):
            for state in (True, False):
                if not sub and not state:
                    continue
                part = raw_backward(GO2, rows, seq, names=sub, state=state)
                assert set(part) == set(sub) | ({"grad_qpos0", "grad_qvel0"} if state else set())
                for k in part:
                    assert bitwise(part[k], full[k]), (sub, state, k)
    # the plain entry's outputs do not move when the schedule's are asked for next to them
    plain = raw_backward(GO2, rows, seq, names=())
    assert bitwise(plain["grad_qpos0"], full["grad_qpos0"])


def test_a_frozen_env_has_zeros_at_its_ticks(gpu):
    """An env with an invalid mass scale is NUMERICAL at every tick (tests/
    test_gpu_rollout_backward.py's way of freezing one): zeros in its slab of grad_T_seq at every
    tick and in its reference and gain gradients, its state cotangents summed; every other env
    bitwise unaffected."""
    tree, kb, km, s, mdl = pair(GO2)
    rows = slice(0, 5)
    ms = np.ones((5, kb.nbody))
    good = raw_backward(GO2, rows, False, ms=ms)
    bad = ms.copy()
    bad[2, 3] = -1.0
    got = raw_backward(GO2, rows, False, ms=bad)
    seq = raw_backward(GO2, rows, True, ms=bad)
    for k in ("grad_pos_ref", "grad_quat_ref", "grad_gains"):
        assert (got[k][2] == 0.0).all(), k
    for g in (got, seq):
        assert (g["grad_T_seq"][:, 2] == 0.0).all()
    assert (seq["grad_pos_ref_seq"][:, 2] == 0.0).all()
    assert (seq["grad_quat_ref_seq"][:, 2] == 0.0).all()
    cot = bcase(GO2)["cot"]
    acc = cot["qpos"][K, 2]
    for t in range(K - 1, -1, -1):
        acc = acc + cot["qpos"][t, 2]
    assert bitwise(got["grad_qpos0"][2], acc)
    others = [0, 1, 3, 4]
    for k in got:
        sel = (lambda a: a[:, others]) if k.endswith("_seq") else (lambda a: a[others])
        assert bitwise(sel(got[k]), sel(good[k])), k
        assert np.abs(sel(good[k])).max() > 0


# ---- 7. guard bands --------------------------------------------------------------------------------------

@pytest.mark.parametrize("seq", [False, True])
@pytest.mark.parametrize("nenv", [5, 17])
def test_backward_stays_inside_its_arrays(gpu, nenv, seq):
    """Every input, sequence, cotangent, new output and the workspace between guard bands at its
    exact size: the bands intact, the inputs unmodified, the results bitwise the ordinary call's
    whether the bands around the inputs hold 0x00 or 0xFF."""
    tree, kb, km, s, mdl = pair(GO2)
    rows = slice(0, nenv)
    ref = raw_backward(GO2, rows, seq)
    nbytes = kb.rollout_backward_workspace_bytes(s, nenv)
    for pad in (0x00, 0xFF):
        fill = 0xA5 if pad == 0 else 0x5A
        a, sc, ins, res = raw_setup(GO2, rows, seq, guard_pad=pad)
        ins = {k: v for k, v in ins.items() if isinstance(v, torch.Tensor)}
        kept = {k: v.clone() for k, v in ins.items()}
        names = raw_names(seq)
        o = {k: guarded(RAW_SHAPES[k](nenv, s.dims), torch.float64, gpu, fill=fill) for k in names}
        o["grad_qpos0"] = guarded((nenv, km.nq), torch.float64, gpu, fill=fill)
        o["grad_qvel0"] = guarded((nenv, km.nv), torch.float64, gpu, fill=fill)
        a.grad_qpos0, a.grad_qvel0 = o["grad_qpos0"].data_ptr(), o["grad_qvel0"].data_ptr()
        ws = guarded((nbytes // 8,), torch.float64, gpu, fill=fill, env_bytes=nbytes // nenv)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        sg = _lib.OscRolloutScheduleGrads(**{k: o[k].data_ptr() for k in names})
        assert raw_call(GO2, a, sc, sg) == 0
        torch.cuda.synchronize()
        for k, t in o.items():
            assert_guards_intact(t, k)
            assert bitwise(t.cpu().numpy(), ref[k]), (k, hex(pad))
        assert_guards_intact(ws, "workspace")
        for k, v in ins.items():
            assert_guards_intact(v, "input " + k)
            assert torch.equal(v, kept[k]), k


@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("nenv", [5, 17])
def test_forward_stays_inside_its_arrays(gpu, nenv, mode):
    """osc_batch_rollout_sched through the C entry with every sequence, the state, the histories
    and the workspace between guard bands; results bitwise the wrapper's."""
    tree, kb, km, s, mdl = pair(GO2)
    c = inputs(GO2, NBIG)
    rows = slice(0, nenv)
    fields = FIELDS[mode][-1]
    sub = {k: (v[:, rows] if k.endswith("_seq") and v.ndim > 2 else
               v if k.endswith("_seq") or v.ndim == 1 else v[rows]) for k, v in c.items()}
    ref = kb.rollout(s, sub["qpos"], sub["qvel"], None, K4, DT, warm=True, history=True,
                     schedule=schedule_of(sub, fields),
                     **(dict(T=sub["T"]) if mode == "held" else dict(pd=(None, None, GAINS))))
    torch.cuda.synchronize()
    nbytes = kb.rollout_workspace_bytes(s, nenv, K4)
    for pad in (0x00, 0xFF):
        fill = 0xA5 if pad == 0 else 0x5A
        seqs = {f + "_seq": guarded_like(dev(np.ascontiguousarray(sub[f + "_seq"])), pad)
                for f in fields}
        kept = {k: v.clone() for k, v in seqs.items()}
        qp, qv = guarded_like(dev(sub["qpos"]), pad), guarded_like(dev(sub["qvel"]), pad)
        o = dict(qpos_hist=guarded((K4 + 1, nenv, km.nq), torch.float64, gpu, fill=fill),
                 qvel_hist=guarded((K4 + 1, nenv, km.nv), torch.float64, gpu, fill=fill),
                 tau_hist=guarded((K4, nenv, mdl.nu), torch.float64, gpu, fill=fill),
                 status_hist=guarded((K4, nenv), torch.int32, gpu, fill=fill),
                 tau=guarded((nenv, mdl.nu), torch.float64, gpu, fill=fill),
                 bad_ticks=guarded((nenv,), torch.int32, gpu, fill=fill))
        ws = guarded((nbytes // 8,), torch.float64, gpu, fill=fill, env_bytes=nbytes // nenv)
        a = _lib.OscRolloutArgs()
        a.nticks, a.dt, a.flags = K4, DT, _lib.ROLLOUT_WARM
        a.qpos, a.qvel = qp.data_ptr(), qv.data_ptr()
        for k, t in o.items():
            setattr(a, k, t.data_ptr())
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        Td = guarded_like(dev(sub["T"]), pad)
        if mode == "held":
            a.target_mode, a.T = _lib.ROLLOUT_TARGETS_HELD, Td.data_ptr()
        else:
            a.target_mode, a.pos_ref_per_env = _lib.ROLLOUT_TARGETS_PD_BASE, 1
            a.gains[:] = GAINS
        sc = _lib.OscRolloutSchedule(**{k: v.data_ptr() for k, v in seqs.items()})
        rc = _lib.lib().osc_batch_rollout_sched(
            s._h, kb._h, nenv, ctypes.byref(a), ctypes.byref(sc), None, None,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        for k, t in o.items():
            assert_guards_intact(t, k)
        for k, t in dict(seqs, qpos=qp, qvel=qv, T=Td, workspace=ws).items():
            assert_guards_intact(t, k)
        assert all(torch.equal(seqs[k], kept[k]) for k in seqs) and torch.equal(Td, dev(sub["T"]))
        assert torch.equal(o["qpos_hist"], ref.qpos_hist) and torch.equal(qp, ref.qpos)
        assert torch.equal(o["tau_hist"], ref.tau_hist) and torch.equal(o["tau"], ref.tau)
        assert torch.equal(o["status_hist"], ref.status_hist)


@pytest.mark.parametrize("nenv", [5, 17])
def test_pd_parameter_adjoint_stays_inside_its_arrays(gpu, nenv):
    rng = np.random.default_rng(90 + nenv)
    src = [rng.standard_normal((nenv, w)) for w in (3, 4, 3, 3, 3, 4)] + \
        [rng.standard_normal((nenv, 5, 6))]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    results = []
    for pad in (0x00, 0xFF):
        i = [guarded_like(dev(a), pad) for a in src]
        kept = [t.clone() for t in i]
        o = [guarded(sh, torch.float64, gpu, fill=0xA5 if pad == 0 else 0x5A)
             for sh in ((nenv, 3), (nenv, 4), (nenv, 4))]
        rc = _lib.lib().osc_pd_base_targets_backward_params(
            nenv, 5, *[ptr(t) for t in i[:5]], 1, ptr(i[5]), 1, (ctypes.c_double * 4)(*GAINS),
            ptr(i[6]), *[ptr(t) for t in o],
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        for k, t in enumerate(o):
            assert_guards_intact(t, f"output {k}")
            assert torch.isfinite(t).all()
        for k, (t, b) in enumerate(zip(i, kept)):
            assert_guards_intact(t, f"input {k}")
            assert torch.equal(t, b)
        results.append([t.clone() for t in o])
    assert all(torch.equal(a, b) for a, b in zip(*results))


# ---- 8. refusals -----------------------------------------------------------------------------------------

def test_backward_refusals_leave_the_outputs_untouched(gpu):
    """Every new argument error of osc_batch_rollout_backward_sched returns 1 with nothing
    enqueued: outputs pre-filled with NaN stay NaN."""
    tree, kb, km, s, mdl = pair(GO2)
    rows, n = slice(0, 5), 5
    outs = {k: nan(*f(n, s.dims)) for k, f in RAW_SHAPES.items()}
    outs["grad_qpos0"] = nan(n, km.nq)

    def untouched():
        torch.cuda.synchronize()
        return all(torch.isnan(t).all() for t in outs.values())

    def setup(seq, mode="pd"):
        a, sc, t, res = raw_setup(GO2, rows, seq, mode)
        a.grad_qpos0 = outs["grad_qpos0"].data_ptr()
        return a, sc

    def grads(*names):
        return _lib.OscRolloutScheduleGrads(**{k: outs[k].data_ptr() for k in names})

    cases = []
    a, sc = setup(False)      # held references
    cases += [("grad_pos_ref_seq without pos_ref_seq", a, sc, grads("grad_pos_ref_seq")),
              ("grad_quat_ref_seq without quat_ref_seq", a, sc, grads("grad_quat_ref_seq"))]
    a, sc = setup(True)       # reference sequences
    cases += [("grad_pos_ref with pos_ref_seq", a, sc, grads("grad_pos_ref")),
              ("grad_quat_ref with quat_ref_seq", a, sc, grads("grad_quat_ref"))]
    for k in ("grad_T_seq", "grad_gains", "grad_pos_ref_seq", "grad_quat_ref_seq"):
        g = grads(k)
        setattr(g, k, getattr(g, k) + 4)
        cases.append(("odd " + k, a, sc, g))
    for k in ("T_seq", "mask_seq", "pos_ref_seq", "quat_ref_seq"):
        a2, sc2 = setup(True)
        setattr(sc2, k, getattr(sc2, k) + 4)
        cases.append(("odd " + k, a2, sc2, grads("grad_T_seq")))
    a2, sc2 = setup(True)
    sc2.mask_seq = None       # and no held mask either
    cases.append(("no mask at all", a2, sc2, grads("grad_T_seq")))
    a2, sc2 = setup(True)
    sc2.pos_ref_seq = None    # and no held reference either
    cases.append(("no position reference at all", a2, sc2, grads("grad_T_seq")))
    a2, sc2 = setup(True)
    a2.grad_qpos0 = None
    cases.append(("every output NULL", a2, sc2, grads()))
    a, sc = setup(False, "held")
    for k in ("grad_pos_ref", "grad_quat_ref", "grad_gains"):
        cases.append((k + " in held mode", a, sc, grads(k)))
    a2, sc2 = setup(False, "held")
    sc2.pos_ref_seq = outs["grad_pos_ref_seq"].data_ptr()
    cases.append(("a reference sequence in held mode", a2, sc2, grads("grad_T_seq")))
    a2, sc2 = setup(False, "held")
    a2.T, sc2.T_seq = None, None
    cases.append(("no targets at all", a2, sc2, grads("grad_T_seq")))
    for what, a, sc, sg in cases:
        assert raw_call(GO2, a, sc, sg) == 1, what
        assert untouched(), what
    # good calls: PD mode may ask for grad_T_seq without a T_seq; every output is then written
    a, sc = setup(True)
    sc.T_seq = None
    sg = grads("grad_T_seq", "grad_pos_ref_seq", "grad_quat_ref_seq", "grad_gains")
    assert raw_call(GO2, a, sc, sg) == 0
    torch.cuda.synchronize()
    for k in ("grad_T_seq", "grad_pos_ref_seq", "grad_quat_ref_seq", "grad_gains", "grad_qpos0"):
        assert torch.isfinite(outs[k]).all(), k


def test_forward_refusals_enqueue_nothing(gpu):
    """osc_batch_rollout_sched: a reference sequence in held mode, a misaligned sequence, and a
    missing T / mask / reference with no sequence in its place return 1; the state and the
    histories (pre-filled with NaN) stay as they are."""
    tree, kb, km, s, mdl = pair(GO2)
    n = 5
    c = inputs(GO2, NBIG)
    qp, qv = dev(c["qpos"][:n]), dev(c["qvel"][:n])
    q0 = qp.clone()
    hist = nan(K4 + 1, n, km.nq)
    seqs = dict(T_seq=dev(c["T_seq"][:, :n]), mask_seq=dev(c["mask_seq"][:, :n]),
                pos_ref_seq=dev(c["pos_ref_seq"][:, :n]), quat_ref_seq=dev(c["quat_ref_seq"]))
    held = dict(T=dev(c["T"][:n]), contact_mask=dev(c["mask"][:n]), pos_ref=dev(c["pos_ref"][:n]),
                quat_ref=dev(c["quat_ref"]))

    def call(mode, use, drop=(), odd=None):
        a = _lib.OscRolloutArgs()
        a.nticks, a.dt, a.flags = K4, DT, 0
        a.qpos, a.qvel, a.qpos_hist = qp.data_ptr(), qv.data_ptr(), hist.data_ptr()
        a.target_mode = _lib.ROLLOUT_TARGETS_HELD if mode == "held" else \
            _lib.ROLLOUT_TARGETS_PD_BASE
        a.pos_ref_per_env = 1
        a.gains[:] = GAINS
        for k, t in held.items():
            if k not in drop and (mode == "pd" or k not in ("pos_ref", "quat_ref")) and \
                    (mode == "held" or k != "T"):
                setattr(a, k, t.data_ptr())
        sc = _lib.OscRolloutSchedule(**{k: seqs[k].data_ptr() + (4 if k == odd else 0)
                                        for k in use})
        return _lib.lib().osc_batch_rollout_sched(
            s._h, kb._h, n, ctypes.byref(a), ctypes.byref(sc), None, None,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call("held", ("pos_ref_seq",)) == 1 and call("held", ("quat_ref_seq",)) == 1
    for k in seqs:
        assert call("pd", tuple(seqs), odd=k) == 1, k
    assert call("held", ("mask_seq",), drop=("T",)) == 1
    assert call("held", ("T_seq",), drop=("contact_mask",)) == 1
    assert call("pd", ("T_seq",), drop=("pos_ref",)) == 1
    assert call("pd", ("pos_ref_seq",), drop=("quat_ref",)) == 1
    torch.cuda.synchronize()
    assert torch.isnan(hist).all() and torch.equal(qp, q0)
    assert call("pd", tuple(seqs), drop=tuple(held)) == 0      # the sequences stand in for all
    torch.cuda.synchronize()
    assert torch.isfinite(hist).all() and not torch.equal(qp, q0)


# ---- 9. autograd -----------------------------------------------------------------------------------------

def test_gradcheck(gpu):
    """torch.autograd.gradcheck of rollout_differentiable on two Go2 envs of the chain case, K = 2,
    PD targets with a feed-forward and the mask schedule, with respect to schedule.T, the held
    per-env pos_ref and the gains (eps 1e-6, atol 1e-5, as tests/test_gpu_rollout_backward.py)."""
    from osc_amd.autograd import rollout_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    c = scpu.sched_case(GO2)
    e = [1, 4]
    q, v = dev(c["qpos"][e]), dev(c["qvel"][e])
    masks = dev(c["masks"][:2, e])
    leaves = [dev(c["ff"][:2, e]).requires_grad_(True), dev(c["pos_ref"][e]).requires_grad_(True),
              dev(np.array(GAINS)).requires_grad_(True)]

    def fn(ff, pos_ref, gains):
        out = rollout_differentiable(s, kb, q, v, None, 2, DT, pd=(pos_ref, c["quat_ref"], gains),
                                     warm=False, schedule=RolloutSchedule(T=ff, mask=masks))
        return out[:3]

    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-5)


def test_autograd_fills_only_what_is_asked(gpu):
    """Forward values bitwise rollout(..., history=True, schedule=...); gradients to schedule.T,
    schedule.pos_ref, the held quat_ref and the gains bitwise rollout_backward's; inputs without
    requires_grad get None; the default call is unchanged."""
    from osc_amd.autograd import rollout_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    c = bcase(GO2)
    rows = slice(0, 5)
    cot = {k: dev(v[:, rows]) for k, v in c["cot"].items()}
    q, v = dev(c["qpos"][rows]), dev(c["qvel"][rows]).requires_grad_(True)
    ff = dev(c["T_seq"][:, rows]).requires_grad_(True)
    prs = dev(c["pos_ref_seq"][:, rows]).requires_grad_(True)
    qr = dev(c["quat_ref"]).requires_grad_(True)
    gains = dev(np.array(GAINS)).requires_grad_(True)
    masks = dev(c["mask_seq"][:, rows])
    sch = RolloutSchedule(T=ff, mask=masks, pos_ref=prs)
    qh, vh, th, st = rollout_differentiable(s, kb, q, v, None, K, DT, pd=(None, qr, gains),
                                            schedule=sch)
    dsch = RolloutSchedule(T=ff.detach(), mask=masks, pos_ref=prs.detach())
    pd = (None, qr.detach(), GAINS)
    plain = kb.rollout(s, q, v.detach(), None, K, DT, pd=pd, history=True, schedule=dsch)
    torch.cuda.synchronize()
    for a, b in ((qh, plain.qpos_hist), (vh, plain.qvel_hist), (th, plain.tau_hist),
                 (st, plain.status_hist)):
        assert torch.equal(a.detach(), b)
    assert not st.requires_grad
    ((qh * cot["qpos"]).sum() + (vh * cot["qvel"]).sum() + (th * cot["tau"]).sum()).backward()
    ref = kb.rollout_backward(s, plain, None, DT, pd=pd, grad_qpos_hist=cot["qpos"],
                              grad_qvel_hist=cot["qvel"], grad_tau_hist=cot["tau"], schedule=dsch,
                              want=("qvel0", "T_seq", "pos_ref_seq", "quat_ref", "gains"))
    assert q.grad is None and masks.grad is None
    assert torch.equal(v.grad, ref["qvel0"]) and torch.equal(ff.grad, ref["T_seq"])
    assert torch.equal(prs.grad, ref["pos_ref_seq"]) and prs.grad.shape == prs.shape
    assert torch.equal(qr.grad, ref["quat_ref"]) and qr.grad.shape == (4,)
    assert torch.equal(gains.grad, ref["gains"]) and gains.grad.shape == (4,)
    assert all(t.grad.abs().max() > 0 for t in (ff, prs, qr, gains))
    # only schedule.T asks: nothing else is filled
    ff2 = dev(c["T_seq"][:, rows]).requires_grad_(True)
    qr2, g2 = dev(c["quat_ref"]), dev(np.array(GAINS))
    out = rollout_differentiable(s, kb, q, v.detach(), None, K, DT, pd=(None, qr2, g2),
                                 schedule=RolloutSchedule(T=ff2, mask=masks, pos_ref=prs.detach()))
    (out[0] * cot["qpos"]).sum().backward()
    assert qr2.grad is None and g2.grad is None and ff2.grad is not None
    # the held references of a call without a schedule get their gradient too
    pr = dev(c["pos_ref"][rows]).requires_grad_(True)
    out = rollout_differentiable(s, kb, q, v.detach(), dev(c["mask"][rows]), K, DT,
                                 pd=(pr, c["quat_ref"], GAINS))
    held = kb.rollout(s, q, v.detach(), dev(c["mask"][rows]), K, DT,
                      pd=(pr.detach(), c["quat_ref"], GAINS), history=True)
    assert torch.equal(out[0].detach(), held.qpos_hist)
    (out[0][-1, :, 0:3] - pr.detach()).square().sum().backward()
    assert pr.grad.shape == pr.shape and pr.grad.abs().max() > 0
