"""GPU tests of the closed-loop rollout (include/osc_rollout.h, csrc/osc_rollout.hip):
  1. the step kernel (osc_batch_integrate) against oracle/kinematics.py::integrate;
  2. osc_batch_rollout bitwise against the loop a user would write from the existing entries;
  3. one-step consistency along the GPU's own trajectory against the oracle chain;
  4. the Go2 closed loop converging on the GPU as it does on the oracle.
Stated tolerances are in each test's docstring."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kin_trees
import kinematics as kin
import rollout_ref
from osc_amd import _lib
from osc_amd.kinematics import KinematicsBatch, load_tree, random_states
from osc_amd.synth import generate
from osc_qp import load_model
from test_gpu_joint_states import CONTRACT          # the oracle chain's contract, 1e-5
from test_gpu_wheels import NOSLIP_YAML, _rel_errors

pytestmark = pytest.mark.gpu

DT = rollout_ref.DT
OK, NUMERICAL, UNREFINED = _lib.SOLVE_OK, _lib.SOLVE_NUMERICAL, _lib.SOLVE_UNREFINED

TREES = {
    "unitree_go2": lambda: load_tree("unitree_go2"),
    "walter_sr": lambda: load_tree("walter_sr"),
    "random_free_root": lambda: kin_trees.random_tree(1),                      # welded body 7
    "random_hinge_root": lambda: kin_trees.random_tree(2, free_root=False),   # welded body 5
    "chain": lambda: kin_trees.chain_tree(3),
    "free_body": kin_trees.free_body,
    "mixed_ball_slide": lambda: kin_trees.mixed_tree(1),                       # 3 balls, 3 slides
    "ball": kin_trees.spherical_pendulum,
    "slide": kin_trees.slider,
}
_kb, _pairs = {}, {}


def _kin(name):
    if name not in _kb:
        tree = TREES[name]()
        _kb[name] = (tree, KinematicsBatch(tree=tree), kin.KinModel(tree))
    return _kb[name]


def _pair(robot):
    from osc_amd.solver import OSCBatchSolver
    if robot not in _pairs:
        tree, kb, km = _kin(robot)
        _pairs[robot] = (tree, kb, km, OSCBatchSolver(robot), load_model(robot))
    return _pairs[robot]


def _exact_fma(v, dt, a):
    """round(v + dt a) of the exact sum, entrywise: what one fma gives."""
    f = np.frompyfunc(lambda x, y: float(Fraction(x) + Fraction(dt) * Fraction(y)), 2, 1)
    return f(v, a).astype(np.float64)


def _rate_dofs(km):
    """First angular-rate dof of every quaternion joint."""
    return [j["dadr"] + (3 if j["type"] == "free" else 0) for j in km.joints
            if j["type"] in ("free", "ball")]


def _quat_adrs(km):
    return [j["qadr"] + (3 if j["type"] == "free" else 0) for j in km.joints
            if j["type"] in ("free", "ball")]


@pytest.mark.parametrize("nenv", [1, 5, 67])
@pytest.mark.parametrize("name", list(TREES))
def test_step_kernel_vs_oracle(gpu, name, nenv):
    """osc_batch_integrate against kinematics.integrate, dt = +-0.002, random qacc, states with
    base_pos_zero=False.  In the batches of 5 and 67 envs (a batch of one has no room for them)
    four rows are forced -- at 67 spread over four of the kernel's 16-env blocks: zero angular
    velocity and acceleration (the identity increment), a rotation angle of 1e-12 per step, status
    OSC_SOLVE_NUMERICAL, a NaN in qacc.
      * qvel' within 1 ulp of qvel + dt qacc -- the reference is the exact sum rounded once;
      * qpos' within 1e-13 absolute of the oracle (a few dozen roundings of O(1) quantities and one
        sincos);  every output quaternion | |q| - 1 | <= 4e-16;
      * the NUMERICAL and NaN rows bitwise unchanged and counted once in bad_ticks, no other row
        counted;
      * a strided qacc out of a larger x-shaped buffer gives bitwise the packed copy's result."""
    tree, kb, km = _kin(name)
    nq, nv = km.nq, km.nv
    assert (kb.nq, kb.nv) == (nq, nv)
    rows = {1: (), 5: (1, 2, 3, 4), 67: (1, 20, 40, 66)}[nenv]
    rates, quats = _rate_dofs(km), _quat_adrs(km)
    for dt in (DT, -DT):
        qpos, qvel = random_states(tree, nenv, 11, base_pos_zero=False)
        rng = np.random.default_rng(100 + nenv)
        qacc = rng.standard_normal((nenv, nv))
        status = np.zeros(nenv, np.int32)
        if rows:
            r_zero, r_tiny, r_num, r_nan = rows
            u = np.array([0.6, 0.0, -0.8])
            for da in rates:
                qvel[r_zero, da:da + 3] = 0.0
                qacc[r_zero, da:da + 3] = 0.0
                qvel[r_tiny, da:da + 3] = u * (1e-12 / abs(dt))
                qacc[r_tiny, da:da + 3] = 0.0
            status[r_num] = NUMERICAL
            qacc[r_nan, nv // 2] = np.nan
        frozen = np.zeros(nenv, bool)
        for r in rows[2:]:
            frozen[r] = True

        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
        qp, qv, bad = dev(qpos), dev(qvel), torch.zeros(nenv, dtype=torch.int32, device=gpu)
        kb.integrate_into(qp, qv, dev(qacc), dt, status=dev(status), bad_ticks=bad)
        xbuf = dev(rng.standard_normal((nenv, nv + 7)))
        xbuf[:, :nv] = dev(qacc)
        qp2, qv2, bad2 = dev(qpos), dev(qvel), torch.zeros(nenv, dtype=torch.int32, device=gpu)
        kb.integrate_into(qp2, qv2, xbuf[:, :nv], dt, status=dev(status), bad_ticks=bad2)
        torch.cuda.synchronize()
        assert torch.equal(qp, qp2) and torch.equal(qv, qv2) and torch.equal(bad, bad2)
        gq, gv = qp.cpu().numpy(), qv.cpu().numpy()

        assert np.array_equal(gq[frozen], qpos[frozen]) and np.array_equal(gv[frozen], qvel[frozen])
        assert np.array_equal(bad.cpu().numpy(), frozen.astype(np.int32))
        live = ~frozen
        vref = _exact_fma(qvel[live], dt, qacc[live])
        ulps = np.abs(gv[live] - vref) / np.spacing(np.abs(vref))
        assert ulps.max() <= 1.0, ulps.max()
        worst = 0.0
        for e in np.nonzero(live)[0]:
            ref = kin.integrate(km, qpos[e], gv[e], dt)
            worst = max(worst, np.abs(gq[e] - ref).max())
        assert worst <= 1e-13, worst
        assert np.isfinite(gq[live]).all()   # the zero-angle row too: no 0 / 0
        for qa in quats:
            nrm = np.linalg.norm(gq[:, qa:qa + 4], axis=1)
            assert np.abs(nrm - 1.0).max() <= 4e-16, np.abs(nrm - 1.0).max()


def test_not_ok_status_is_counted_but_still_steps(gpu):
    """bad_ticks counts every status that is not OSC_SOLVE_OK; only OSC_SOLVE_NUMERICAL (or a
    non-finite qacc) freezes the env."""
    tree, kb, km = _kin("unitree_go2")
    qpos, qvel = random_states(tree, 3, 5, base_pos_zero=False)
    qacc = np.random.default_rng(1).standard_normal((3, km.nv))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    qp, qv, bad = dev(qpos), dev(qvel), torch.full((3,), 2, dtype=torch.int32, device=gpu)
    st = dev(np.array([OK, UNREFINED, _lib.SOLVE_MAX_ITER], np.int32))
    kb.integrate_into(qp, qv, dev(qacc), DT, status=st, bad_ticks=bad)
    a, b = dev(qpos), dev(qvel)
    kb.integrate_into(a, b, dev(qacc), DT)
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [2, 3, 3]
    assert torch.equal(qp, a) and torch.equal(qv, b) and not torch.equal(qp, dev(qpos))


def _inputs(robot, nenv, seed=31):
    tree, kb, km, solver, model = _pair(robot)
    qpos, qvel = random_states(tree, nenv, seed, base_pos_zero=False, joint_range=0.5,
                               vel_scale=0.1)
    T = generate(robot, nenv, seed, "standing", "ones")["T"]
    mask = np.ones((nenv, model.nc))
    rng = np.random.default_rng(seed)
    pos_ref = qpos[:, :3] + 0.02 * rng.standard_normal((nenv, 3))     # per env
    pd = (pos_ref, np.array([1.0, 0.0, 0.0, 0.0]), rollout_ref.STANDING_GAINS)   # quat shared
    return qpos, qvel, T, mask, pd


def _user_loop(robot, qpos, qvel, mask, nticks, dt, T, pd, warm, gpu):
    """The loop a user would write from the existing entries plus integrate_into."""
    tree, kb, km, solver, model = _pair(robot)
    nenv, nv, ns = qpos.shape[0], km.nv, model.ns
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    qp, qv, md = dev(qpos), dev(qvel), dev(mask)
    out = solver.alloc_outputs(nenv, want_x=True)
    wstate = solver.alloc_warm_state(nenv)
    ws = torch.empty((kb.workspace_bytes(solver, nenv) // 8 + 2,), dtype=torch.float64, device=gpu)
    bad = torch.zeros(nenv, dtype=torch.int32, device=gpu)
    if pd is None:
        Td = dev(T)
    else:
        Td = torch.empty((nenv, ns, 6), dtype=torch.float64, device=gpu)
        pref, qref = dev(pd[0]), dev(pd[1])
        gains = (ctypes.c_double * 4)(*pd[2])
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    h = dict(qpos=[qp.clone()], qvel=[qv.clone()], tau=[], status=[])
    for _ in range(nticks):
        if pd is not None:
            base = [qp[:, 0:3].contiguous(), qp[:, 3:7].contiguous(), qv[:, 0:3].contiguous(),
                    qv[:, 3:6].contiguous()]
            rc = _lib.lib().osc_pd_base_targets(nenv, ns, *[p(t) for t in base], p(pref),
                                                int(pref.dim() == 2), p(qref),
                                                int(qref.dim() == 2), gains, p(Td), stream)
            assert rc == 0
        if warm:
            kb.solve_warm_into(solver, out, wstate, qp, qv, Td, md, ws)
        else:
            kb.solve_into(solver, out, qp, qv, Td, md, ws)
        h["tau"].append(out.tau.clone())
        h["status"].append(out.status.clone())
        kb.integrate_into(qp, qv, out.x[:, :nv], dt, status=out.status, bad_ticks=bad)
        h["qpos"].append(qp.clone())
        h["qvel"].append(qv.clone())
    torch.cuda.synchronize()
    return {k: torch.stack(v) for k, v in h.items()}, bad


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("robot,nenv", [("unitree_go2", 33), ("walter_sr", 5)])
def test_rollout_bitwise_vs_user_loop(gpu, robot, nenv, mode, warm):
    """Four ticks of osc_batch_rollout: qpos_hist, qvel_hist, tau_hist, status_hist, bad_ticks and
    the final state bitwise those of a Python loop over osc_pd_base_targets (PD mode, on the base
    state sliced out of qpos / qvel), solve_warm_into / solve_into with x and integrate_into with
    x[:, :nv]; a caller workspace and the library's own scratch agree bitwise; the caller's
    arrays are not modified."""
    tree, kb, km, solver, model = _pair(robot)
    qpos, qvel, T, mask, pd = _inputs(robot, nenv)
    q0, v0 = qpos.copy(), qvel.copy()
    kw = dict(T=T) if mode == "held" else dict(pd=pd)
    res = kb.rollout(solver, qpos, qvel, mask, 4, DT, warm=warm, history=True, **kw)
    res2 = kb.rollout(solver, qpos, qvel, mask, 4, DT, warm=warm, history=True, workspace=None,
                      **kw)
    ref, bad = _user_loop(robot, qpos, qvel, mask, 4, DT, kw.get("T"), kw.get("pd"), warm, gpu)
    torch.cuda.synchronize()
    assert np.array_equal(qpos, q0) and np.array_equal(qvel, v0)
    for r in (res, res2):
        assert torch.equal(r.qpos_hist, ref["qpos"]) and torch.equal(r.qvel_hist, ref["qvel"])
        assert torch.equal(r.tau_hist, ref["tau"]) and torch.equal(r.status_hist, ref["status"])
        assert torch.equal(r.qpos, ref["qpos"][-1]) and torch.equal(r.qvel, ref["qvel"][-1])
        assert torch.equal(r.tau, ref["tau"][-1]) and torch.equal(r.bad_ticks, bad)
    assert (res.status_hist == OK).all() and not torch.equal(res.qpos_hist[0], res.qpos_hist[4])
    # without histories: the same final state
    res3 = kb.rollout(solver, qpos, qvel, mask, 4, DT, warm=warm, **kw)
    torch.cuda.synchronize()
    assert torch.equal(res3.qpos, res.qpos) and torch.equal(res3.qvel, res.qvel)
    assert torch.equal(res3.tau, res.tau) and res3.qpos_hist is None


def test_rollout_zero_ticks(gpu):
    """nticks = 0 returns the input state and writes slab 0 of the histories only."""
    tree, kb, km, solver, model = _pair("unitree_go2")
    qpos, qvel, T, mask, pd = _inputs("unitree_go2", 7)
    for kw in (dict(T=T), dict(pd=pd)):
        for ws in ("alloc", None):
            res = kb.rollout(solver, qpos, qvel, mask, 0, DT, history=True, workspace=ws, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(res.qpos.cpu().numpy(), qpos)
            assert np.array_equal(res.qvel.cpu().numpy(), qvel)
            assert res.qpos_hist.shape[0] == 1 and res.tau_hist.shape[0] == 0
            assert np.array_equal(res.qpos_hist[0].cpu().numpy(), qpos)
            assert np.array_equal(res.qvel_hist[0].cpu().numpy(), qvel)
            assert (res.bad_ticks == 0).all() and (res.tau == 0).all()


def test_rollout_refusals(gpu):
    """OSC_ERR_INVALID_ARGUMENT, before anything is enqueued, for: a model with wheel rows, PD-base
    targets on a hinge-rooted tree, nticks < 0, dt <= 0, a too small or misaligned workspace, both
    or neither of T and pd."""
    from osc_amd.solver import OSCBatchSolver
    tree, kb, km, solver, model = _pair("walter_sr")
    qpos, qvel, T, mask, pd = _inputs("walter_sr", 3)

    def refused(fn):
        with pytest.raises(_lib.OSCError) as e:
            fn()
        assert e.value.code == 1
    wheels = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)       # same nv / ns as walter_sr
    assert wheels.wheels
    refused(lambda: kb.rollout(wheels, qpos, qvel, mask, 2, DT, T=T))
    refused(lambda: kb.rollout_workspace_bytes(wheels, 3, 2))
    # a hinge-rooted tree with WaLTER's nv and site count: the pair itself is accepted
    hinged = kin_trees.random_tree(4, nbody=14, free_root=False, nsite=17, weld_p=0.0)
    kh = KinematicsBatch(tree=hinged)
    assert (kh.nv, kh.ns) == (14, 17) and kh.rollout_workspace_bytes(solver, 3, 2) > 0
    qh, vh = random_states(hinged, 3, 1)
    pdh = (np.zeros(3), pd[1], pd[2])
    refused(lambda: kh.rollout(solver, qh, vh, mask, 2, DT, pd=pdh))
    refused(lambda: kh.rollout(solver, qh, vh, mask, 0, DT, pd=pdh))
    refused(lambda: kb.rollout(solver, qpos, qvel, mask, -1, DT, T=T))
    refused(lambda: kb.rollout(solver, qpos, qvel, mask, 2, 0.0, T=T))
    refused(lambda: kb.rollout(solver, qpos, qvel, mask, 2, -DT, T=T))
    refused(lambda: kb.rollout(solver, qpos, qvel, mask, 2, float("nan"), T=T))
    refused(lambda: kb.rollout_workspace_bytes(solver, 3, -1))
    need = kb.rollout_workspace_bytes(solver, 3, 2)
    small = torch.empty((need // 8 - 1,), dtype=torch.float64, device=gpu)
    refused(lambda: kb.rollout(solver, qpos, qvel, mask, 2, DT, T=T, workspace=small))
    odd = torch.empty((need // 8 + 2,), dtype=torch.float64, device=gpu)[1:]   # 8 mod 16
    refused(lambda: kb.rollout(solver, qpos, qvel, mask, 2, DT, T=T, workspace=odd))
    with pytest.raises(ValueError):
        kb.rollout(solver, qpos, qvel, mask, 2, DT)
    with pytest.raises(ValueError):
        kb.rollout(solver, qpos, qvel, mask, 2, DT, T=T, pd=pd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("robot,nenv,mode", [("unitree_go2", 4, "pd"), ("walter_sr", 2, "held")])
def test_one_step_consistency_vs_oracle(gpu, robot, nenv, mode):
    """Five ticks; from every (qpos_k, qvel_k) of the GPU's own history one oracle tick
    (rollout_ref.step).  The GPU's implied acceleration (qvel_{k+1} - qvel_k) / dt against the
    oracle's dv normwise within the chain contract tests/test_gpu_joint_states.py applies to this
    same oracle chain (CONTRACT, 1e-5); qpos_{k+1} within 1e-13 of kinematics.integrate(qpos_k,
    qvel_{k+1} of the GPU, dt).  One step at a time from the GPU's states: nothing compounds."""
    tree, kb, km, solver, model = _pair(robot)
    qpos, qvel, T, mask, pd = _inputs(robot, nenv, seed=41)
    kw = dict(T=T) if mode == "held" else dict(pd=pd)
    res = kb.rollout(solver, qpos, qvel, mask, 5, DT, history=True, **kw)
    torch.cuda.synchronize()
    qh, vh = res.qpos_hist.cpu().numpy(), res.qvel_hist.cpu().numpy()
    assert (res.status_hist == OK).all() and (res.bad_ticks == 0).all()
    worst_a = worst_q = 0.0
    for k in range(5):
        for e in range(nenv):
            one = dict(T=T[e]) if mode == "held" else dict(pd=(pd[0][e], pd[1], pd[2]))
            _, _, _, dv = rollout_ref.step(km, model, qh[k, e], vh[k, e], mask[e], DT, **one)
            nw, _ = _rel_errors((vh[k + 1, e] - vh[k, e]) / DT, dv)
            worst_a = max(worst_a, float(nw))
            ref = kin.integrate(km, qh[k, e], vh[k + 1, e], DT)
            worst_q = max(worst_q, np.abs(qh[k + 1, e] - ref).max())
    print(f"\n{robot} one-step consistency: implied acceleration vs oracle dv worst normwise "
          f"{worst_a:.2e}, qpos vs oracle integrate worst {worst_q:.2e}")
    assert worst_a <= CONTRACT, worst_a
    assert worst_q <= 1e-13, worst_q


GO2_OFFSETS = [(0.01, -0.01, -0.02),      # the CPU test's case
               (-0.015, 0.01, 0.015),     # |.| 0.0235 m; oracle ratio 0.0033 after 300 ticks
               (0.0, 0.02, -0.01)]        # |.| 0.0224 m; oracle ratio 0.0023


def test_go2_closed_loop_on_the_gpu(gpu):
    """Go2, 3 envs, 300 warm ticks in PD mode, dt 0.002: env 0 is tests/test_rollout_ref.py's
    case, envs 1 and 2 the same pose with two other reference offsets.  Precondition on the inputs
    (checked, not measured): the oracle rollout of every env has r_ref <= 0.03.  Then every
    status OK, bad_ticks zero, all states finite, quaternions unit, and each env's base-position
    error ratio r_gpu <= 2 r_ref (the margin forgives the slow tail's wobble, 0.0065 / 0.0030 /
    0.0023 at 250 / 300 / 350 ticks; a loop that fails to close sits at >= 0.3)."""
    tree, kb, km, solver, model = _pair("unitree_go2")
    cases = [rollout_ref.go2_case(o) for o in GO2_OFFSETS]
    r_ref = []
    for _, _, q0, v0, m, pd in cases:
        h = rollout_ref.rollout(km, model, q0, v0, m, 300, DT, pd=pd)
        r_ref.append(rollout_ref.error_ratio(h["qpos"][300], q0, pd[0]))
    assert max(r_ref) <= 0.03, r_ref
    qpos = np.array([c[2] for c in cases])
    qvel = np.array([c[3] for c in cases])
    mask = np.array([c[4] for c in cases])
    pos_ref = np.array([c[5][0] for c in cases])
    pd = (pos_ref, cases[0][5][1], cases[0][5][2])
    res = kb.rollout(solver, qpos, qvel, mask, 300, DT, pd=pd, warm=True, history=True)
    torch.cuda.synchronize()
    qh, vh = res.qpos_hist.cpu().numpy(), res.qvel_hist.cpu().numpy()
    assert (res.status_hist == OK).all() and (res.bad_ticks == 0).all()
    assert np.isfinite(qh).all() and np.isfinite(vh).all() and torch.isfinite(res.tau_hist).all()
    assert np.abs(np.linalg.norm(qh[:, :, 3:7], axis=2) - 1.0).max() <= 4e-16
    r_gpu = [rollout_ref.error_ratio(qh[300, e], qpos[e], pos_ref[e]) for e in range(3)]
    print(f"\nGo2 closed loop, 300 ticks: r_ref {np.round(r_ref, 5)}, r_gpu {np.round(r_gpu, 5)}, "
          f"max |tau| {res.tau_hist.abs().max().item():.2f} N m")
    for rg, rr in zip(r_gpu, r_ref):
        assert rg <= 2.0 * rr, (r_gpu, r_ref)
