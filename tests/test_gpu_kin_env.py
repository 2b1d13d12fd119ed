"""GPU tests of the per-env inertial parameters and of the joint-state tick and rollout with per-env
parameters (include/osc_kin_env_params.h; osc_amd.kinematics.KinEnvParams):
   1. parity of osc_batch_kinematics_env against the oracle on each env's own tree
      (tests/kin_env_ref.py), each field alone and all three;
   2. off is off: no block, an all-None block, identity values; J, b, site_xpos never move;
   3. an env of the batch is bitwise its one-env call (first row, last row of a wave, the tail);
   4. the base-z bias at rest is the scaled total weight;
   5. an invalid env is NUMERICAL with NaN outputs, the others untouched;
   6. the tick is bitwise the user's kinematics-env call followed by the solve(-env);
   7. the tick against the exact optimum of the oracle chain;
   8. the rollout is bitwise the user's loop; an invalid env stays frozen;
   9. refusals leave nothing enqueued;
  10. no access outside the parameter arrays and the outputs (tests/guard.py).

Tolerances.  Kinematics: per env and output max |gpu - oracle| <= 1e-12 (1 + max |oracle|), the
kinematics tolerance (tests/test_gpu_kinematics.py); M exactly symmetric.  Torques against the
exact optimum: the contract tests/test_gpu_env_params.py holds its own oracle comparison to
(test_gpu_descriptors._within_contract: tau normwise and elementwise above the 1 % floor, and x
normwise, <= 1e-5).  Everything else is bitwise."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import env_params_cases as ec
import kin_env_ref as ker
import kinematics as kin
import rollout_ref
from guard import assert_guards_intact, guarded, guarded_like
from kin_trees import chain_tree, mixed_tree, random_tree
from osc_amd import _lib
from osc_amd.kinematics import KinEnvParams, KinematicsBatch, KinOutputs, load_tree, random_states

pytestmark = pytest.mark.gpu

TOL = 1e-12
NENV = 37          # nine full wavefronts + a ragged tail row
GO2, WALTER = "unitree_go2", "walter_sr"
NUMERICAL = _lib.SOLVE_NUMERICAL
FIELDS = KinEnvParams.FIELDS
FIELD_SETS = [(f,) for f in FIELDS] + [FIELDS]
OUT = ("M", "C", "J", "b", "site_xpos")
DT = rollout_ref.DT

TREES = {GO2: lambda: load_tree(GO2), WALTER: lambda: load_tree(WALTER),
         "random_free": lambda: random_tree(5), "chain16": lambda: chain_tree(7),
         "slide_ball_fixed": lambda: mixed_tree(3, free_root=False)}


@functools.lru_cache(maxsize=None)
def setup(name):
    """(tree, KinematicsBatch, states, drawn parameters) of a tree, shared by the tests."""
    tree = TREES[name]()
    kb = KinematicsBatch(tree=tree)
    assert kb.nbody == len(tree["bodies"])
    qpos, qvel = random_states(tree, NENV, 100 + len(name), base_pos_zero=(name != "random_free"))
    return tree, kb, qpos, qvel, ker.draw(tree, NENV, 500 + len(name))


@functools.lru_cache(maxsize=None)
def solver(robot):
    from osc_amd.solver import OSCBatchSolver
    return OSCBatchSolver(robot)


def block(p, fields=FIELDS, rows=slice(None)):
    return KinEnvParams(**{k: torch.from_numpy(np.ascontiguousarray(p[k][rows])).cuda()
                           for k in fields})


def env_block(p, rows=slice(None)):
    from osc_amd.solver import EnvParams
    return EnvParams(**{k: torch.from_numpy(np.ascontiguousarray(p[k][rows])).cuda() for k in p})


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def same(a, b):
    """bitwise equality (NaNs and signed zeros included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                              b.contiguous().view(torch.uint8))


def compute(kb, qpos, qvel, kin_params=None):
    out = kb.compute(qpos, qvel, kin_params=kin_params)
    torch.cuda.synchronize()
    return out


# ---- 1. parity ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fields", FIELD_SETS, ids=["mass", "com", "armature", "all"])
@pytest.mark.parametrize("name", list(TREES))
def test_parity_with_the_oracle_on_each_envs_tree(gpu, name, fields):
    tree, kb, qpos, qvel, p = setup(name)
    assert (p["armature_scale"] == 0.0).any() and p["mass_scale"].min() >= 0.5
    out = compute(kb, qpos, qvel, block(p, fields))
    got = {k: getattr(out, k).cpu().numpy() for k in OUT}
    worst = dict.fromkeys(OUT[:4], 0.0)
    for e in range(NENV):
        ref = dict(zip(OUT[:4], ker.kinematics(tree, p, e, qpos[e], qvel[e], fields)))
        for k, r in ref.items():
            err = np.abs(got[k][e] - r).max() / (1 + np.abs(r).max())
            worst[k] = max(worst[k], err)
            assert err <= TOL, (k, e, err)
        assert np.array_equal(got["M"][e], got["M"][e].T), e
    print(f"\n{name} {fields}: worst scaled error " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- 2. off is off -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(TREES))
def test_off_is_off(gpu, name):
    tree, kb, qpos, qvel, p = setup(name)
    ref = compute(kb, qpos, qvel)
    for what, kp in (("None", None), ("all-None block", KinEnvParams())):
        out = compute(kb, qpos, qvel, kp)
        for k in OUT:
            assert same(getattr(out, k), getattr(ref, k)), (what, k)
    ident = compute(kb, qpos, qvel, block(ker.identity(tree, NENV)))
    for k in ("M", "C"):      # (a zero's sign may differ: not bitwise)
        g, r = getattr(ident, k).cpu().numpy(), getattr(ref, k).cpu().numpy()
        for e in range(NENV):
            assert np.abs(g[e] - r[e]).max() <= TOL * (1 + np.abs(r[e]).max()), (k, e)
    for fields in FIELD_SETS:
        out = compute(kb, qpos, qvel, block(p, fields))
        for k in ("J", "b", "site_xpos"):
            assert same(getattr(out, k), getattr(ref, k)), (fields, k)
        assert not same(out.M, ref.M), fields


# ---- 3. row independence -----------------------------------------------------------------------

@pytest.mark.parametrize("name", [GO2, "chain16"])
def test_an_env_of_the_batch_is_bitwise_its_one_env_call(gpu, name):
    tree, kb, qpos, qvel, p = setup(name)
    full = compute(kb, qpos, qvel, block(p))
    for e in (0, 3, 35, 36):
        one = compute(kb, qpos[e:e + 1], qvel[e:e + 1], block(p, rows=slice(e, e + 1)))
        for k in OUT:
            assert same(getattr(one, k), getattr(full, k)[e:e + 1]), (e, k)


# ---- 4. total mass -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", [GO2, "random_free"])
def test_base_z_bias_at_rest_is_the_scaled_total_weight(gpu, name):
    tree, kb, qpos, qvel, p = setup(name)
    out = compute(kb, qpos, np.zeros_like(qvel), block(p))
    mass = np.array([b["mass"] for b in tree["bodies"]])
    np.testing.assert_allclose(out.C[:, 2].cpu().numpy(), 9.81 * (p["mass_scale"] * mass).sum(1),
                               rtol=1e-13)


# ---- 5. invalid env ----------------------------------------------------------------------------

def _tick_inputs(robot, nenv, seed):
    tree = load_tree(robot)
    qpos, qvel = random_states(tree, nenv, seed, joint_range=0.5)
    d = solver(robot).dims
    rng = np.random.default_rng(seed)
    T = np.zeros((nenv, d["ns"], 6))
    T[:, 0, :] = 10.0 * rng.standard_normal((nenv, 6))
    mask = (rng.uniform(size=(nenv, d["nc"])) < 0.75).astype(np.float64)
    return tree, qpos, qvel, T, mask


INVALID = {"mass NaN": ("mass_scale", (5, 2), np.nan), "mass 0": ("mass_scale", (5, 0), 0.0),
           "mass -1": ("mass_scale", (5, 12), -1.0), "com +inf": ("com_offset", (5, 4, 1), np.inf),
           "armature -0.5": ("armature_scale", (5, 17), -0.5)}


@pytest.mark.parametrize("what", list(INVALID))
def test_invalid_env_is_numerical_and_the_others_untouched(gpu, what):
    tree, qpos, qvel, T, mask = _tick_inputs(GO2, NENV, 9)
    kb, s = setup(GO2)[1], solver(GO2)
    p = ker.draw(tree, NENV, 77)
    field, idx, value = INVALID[what]
    bad = {k: v.copy() for k, v in p.items()}
    bad[field][idx] = value
    good_k, bad_k = compute(kb, qpos, qvel, block(p)), compute(kb, qpos, qvel, block(bad))
    assert torch.isnan(bad_k.M[5]).all() and torch.isnan(bad_k.C[5]).all()
    others = [e for e in range(NENV) if e != 5]
    for k in OUT:
        rows = others if k in ("M", "C") else slice(None)     # J, b, site_xpos: env 5 as well
        assert same(getattr(bad_k, k)[rows], getattr(good_k, k)[rows]), k
    good = kb.solve(s, qpos, qvel, T, mask, want_x=True, kin_params=block(p))
    res = kb.solve(s, qpos, qvel, T, mask, want_x=True, kin_params=block(bad))
    torch.cuda.synchronize()
    assert res.status[5].item() == NUMERICAL and torch.isnan(res.tau[5]).all()
    assert (good.status == 0).all()
    for k in ("tau", "x", "status", "iters"):
        assert same(getattr(res, k)[others], getattr(good, k)[others]), k


# ---- 6. tick composition -----------------------------------------------------------------------

@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("robot,nenv", [(GO2, 33), (WALTER, 5)])
def test_tick_is_bitwise_kinematics_env_then_the_solve(gpu, robot, nenv, warm):
    """Three ticks of a small joint-space walk.  solve_into / solve_warm_into with (both blocks),
    (kin_params only), (an all-None kin block) against compute_into(kin_params) followed by
    solver.solve_into / solve_warm_into with the same env_params, and the last against today's
    solve_into as well: tau, x, status, iters and the warm state bitwise."""
    from osc_amd.solver import EnvParams
    tree, qpos, qvel, T, mask = _tick_inputs(robot, nenv, 5)
    kb, s = KinematicsBatch(tree=tree), solver(robot)
    K = block(ker.draw(tree, nenv, 31))
    E = env_block(ec.draw_params(robot, np.random.default_rng(32), nenv))
    Td, md = dev(T), dev(mask)
    ws = torch.empty((kb.env_workspace_bytes(s, nenv) // 8 + 2,), dtype=torch.float64, device=gpu)
    kk = kb.alloc(nenv)
    for what, ep, kp in (("both", E, K), ("kin only", None, K), ("off", None, KinEnvParams()),
                         ("env only", E, None), ("all-None blocks", EnvParams(), KinEnvParams())):
        oa, ob, oc = (s.alloc_outputs(nenv, want_x=True) for _ in range(3))
        wa, wb, wc = (s.alloc_warm_state(nenv) for _ in range(3))
        for t in range(3):
            qp, qv = dev(qpos + 0.01 * t), dev(qvel)
            kb.compute_into(kk, qp, qv, kin_params=kp)
            if warm:
                kb.solve_warm_into(s, oa, wa, qp, qv, Td, md, ws, env_params=ep, kin_params=kp)
                s.solve_warm_into(ob, wb, kk.M, kk.C, kk.J, kk.b, Td, md, env_params=ep)
            else:
                kb.solve_into(s, oa, qp, qv, Td, md, ws, env_params=ep, kin_params=kp)
                s.solve_into(ob, kk.M, kk.C, kk.J, kk.b, Td, md, env_params=ep)
            torch.cuda.synchronize()
            for k in ("tau", "x", "status", "iters"):
                assert same(getattr(oa, k), getattr(ob, k)), (what, t, k)
            assert not warm or same(wa, wb), (what, t)
            assert (oa.status == 0).all(), (what, t, oa.status)
            if what in ("off", "all-None blocks"):
                if warm:
                    kb.solve_warm_into(s, oc, wc, qp, qv, Td, md, ws)
                else:
                    kb.solve_into(s, oc, qp, qv, Td, md, ws)
                torch.cuda.synchronize()
                for k in ("tau", "x", "status", "iters"):
                    assert same(getattr(oa, k), getattr(oc, k)), (what, "today's entry", t, k)
                assert not warm or same(wa, wc), (what, t)


# ---- 7. end to end against the oracle -----------------------------------------------------------

def test_tick_against_the_exact_optimum_of_the_oracle_chain(gpu):
    """Go2, 8 envs, both blocks: env e's tau and x against qp_exact.solve_exact (certified to
    1e-8) on the QP of its own model (tests/env_params_cases.env_model) built from the oracle's
    M, C, J, b of its own tree (tests/kin_env_ref.py)."""
    import desc_variants as dv
    from osc_qp import load_model
    from test_gpu_descriptors import _within_contract
    nenv = 8
    tree, qpos, qvel, T, mask = _tick_inputs(GO2, nenv, 9)
    kb, s = setup(GO2)[1], solver(GO2)
    kp = ker.draw(tree, nenv, 41)
    ep = ec.draw_params(GO2, np.random.default_rng(42), nenv)
    res = kb.solve(s, qpos, qvel, T, mask, want_x=True, env_params=env_block(ep),
                   kin_params=block(kp))
    torch.cuda.synchronize()
    assert (res.status == 0).all(), res.status
    xo = []
    for e in range(nenv):
        M, C, J, b = ker.kinematics(tree, kp, e, qpos[e], qvel[e])
        d = dict(M=M[None], C=C[None], J=J[None], b=b[None], T=T[e:e + 1], mask=mask[e:e + 1])
        xo.append(dv.solve_oracle(ec.env_model(GO2, ep, e), d)[0][0])
    nw, el, ok = _within_contract(res.tau.cpu().numpy(), res.x.cpu().numpy(), np.array(xo),
                                  load_model(GO2))
    print(f"\nworst normwise {nw.max():.2e}, elementwise {el.max():.2e}")
    assert ok.all(), (nw, el)


# ---- 8. rollout --------------------------------------------------------------------------------

def _rollout_inputs(nenv, seed=31):
    from osc_amd.synth import generate
    tree = load_tree(GO2)
    qpos, qvel = random_states(tree, nenv, seed, base_pos_zero=False, joint_range=0.5,
                               vel_scale=0.1)
    T = generate(GO2, nenv, seed, "standing", "ones")["T"]
    mask = np.ones((nenv, solver(GO2).dims["nc"]))
    rng = np.random.default_rng(seed)
    pos_ref = qpos[:, :3] + 0.02 * rng.standard_normal((nenv, 3))
    pd = (pos_ref, np.array([1.0, 0.0, 0.0, 0.0]), rollout_ref.STANDING_GAINS)
    return tree, qpos, qvel, T, mask, pd


def _user_loop(kb, s, qpos, qvel, mask, nticks, T, pd, warm, ep, kp):
    """compute_into(kin_params) -> [osc_pd_base_targets] -> solver.solve(_warm)_into(env_params)
    -> integrate_into, from the entries a user has."""
    nenv, nv, ns = qpos.shape[0], kb.nv, s.dims["ns"]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    qp, qv, md = dev(qpos), dev(qvel), dev(mask)
    out, wstate, kk = s.alloc_outputs(nenv, want_x=True), s.alloc_warm_state(nenv), kb.alloc(nenv)
    bad = torch.zeros(nenv, dtype=torch.int32, device=qp.device)
    if pd is None:
        Td = dev(T)
    else:
        Td = torch.empty((nenv, ns, 6), dtype=torch.float64, device=qp.device)
        pref, qref = dev(pd[0]), dev(pd[1])
        gains = (ctypes.c_double * 4)(*pd[2])
    stream = ctypes.c_void_p(torch.cuda.current_stream(qp.device).cuda_stream)
    h = dict(qpos=[qp.clone()], qvel=[qv.clone()], tau=[], status=[])
    for _ in range(nticks):
        if pd is not None:
            base = [qp[:, 0:3].contiguous(), qp[:, 3:7].contiguous(), qv[:, 0:3].contiguous(),
                    qv[:, 3:6].contiguous()]
            rc = _lib.lib().osc_pd_base_targets(nenv, ns, *[p(t) for t in base], p(pref),
                                                int(pref.dim() == 2), p(qref),
                                                int(qref.dim() == 2), gains, p(Td), stream)
            assert rc == 0
        kb.compute_into(kk, qp, qv, kin_params=kp)
        if warm:
            s.solve_warm_into(out, wstate, kk.M, kk.C, kk.J, kk.b, Td, md, env_params=ep)
        else:
            s.solve_into(out, kk.M, kk.C, kk.J, kk.b, Td, md, env_params=ep)
        h["tau"].append(out.tau.clone())
        h["status"].append(out.status.clone())
        kb.integrate_into(qp, qv, out.x[:, :nv], DT, status=out.status, bad_ticks=bad)
        h["qpos"].append(qp.clone())
        h["qvel"].append(qv.clone())
    torch.cuda.synchronize()
    return {k: torch.stack(v) for k, v in h.items()}, bad


def _assert_rollouts_equal(r, ref, bad, where, rows=slice(None)):
    for a, b in ((r.qpos_hist, ref["qpos"]), (r.qvel_hist, ref["qvel"]), (r.tau_hist, ref["tau"]),
                 (r.status_hist, ref["status"])):
        assert same(a[:, rows], b[:, rows]), where
    assert same(r.qpos[rows], ref["qpos"][-1][rows]) and same(r.qvel[rows], ref["qvel"][-1][rows])
    assert same(r.tau[rows], ref["tau"][-1][rows]) and same(r.bad_ticks[rows], bad[rows]), where


@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("mode", ["held", "pd"])
def test_rollout_is_bitwise_the_user_loop(gpu, mode, warm):
    from osc_amd.solver import EnvParams
    nenv, nticks = 33, 3
    tree, qpos, qvel, T, mask, pd = _rollout_inputs(nenv)
    kb, s = setup(GO2)[1], solver(GO2)
    K = block(ker.draw(tree, nenv, 51))
    E = env_block(ec.draw_params(GO2, np.random.default_rng(52), nenv))
    kw = dict(T=T) if mode == "held" else dict(pd=pd)
    res = kb.rollout(s, qpos, qvel, mask, nticks, DT, warm=warm, history=True, env_params=E,
                     kin_params=K, **kw)
    res2 = kb.rollout(s, qpos, qvel, mask, nticks, DT, warm=warm, history=True, workspace=None,
                      env_params=E, kin_params=K, **kw)
    ref, bad = _user_loop(kb, s, qpos, qvel, mask, nticks, kw.get("T"), kw.get("pd"), warm, E, K)
    torch.cuda.synchronize()
    for r in (res, res2):
        _assert_rollouts_equal(r, ref, bad, (mode, warm))
    assert (res.status_hist == 0).all() and not same(res.qpos_hist[0], res.qpos_hist[nticks])
    # both blocks off: today's rollout
    today = kb.rollout(s, qpos, qvel, mask, nticks, DT, warm=warm, history=True, **kw)
    off = kb.rollout(s, qpos, qvel, mask, nticks, DT, warm=warm, history=True,
                     env_params=EnvParams(), kin_params=KinEnvParams(), **kw)
    torch.cuda.synchronize()
    _assert_rollouts_equal(off, dict(qpos=today.qpos_hist, qvel=today.qvel_hist,
                                     tau=today.tau_hist, status=today.status_hist),
                           today.bad_ticks, "off")
    assert not same(today.qpos, res.qpos)


@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
def test_rollout_freezes_an_env_with_an_invalid_mass_scale(gpu, warm):
    nenv, nticks = 33, 3
    tree, qpos, qvel, T, mask, pd = _rollout_inputs(nenv)
    kb, s = setup(GO2)[1], solver(GO2)
    p = ker.draw(tree, nenv, 51)
    E = env_block(ec.draw_params(GO2, np.random.default_rng(52), nenv))
    bad = {k: v.copy() for k, v in p.items()}
    bad["mass_scale"][7, 3] = -1.0
    run = lambda q: kb.rollout(s, qpos, qvel, mask, nticks, DT, T=T, warm=warm, history=True,
                               env_params=E, kin_params=block(q))
    good, res = run(p), run(bad)
    torch.cuda.synchronize()
    assert same(res.qpos[7], dev(qpos[7])) and same(res.qvel[7], dev(qvel[7]))
    assert res.bad_ticks[7].item() == nticks and (res.status_hist[:, 7] == NUMERICAL).all()
    others = [e for e in range(nenv) if e != 7]
    assert (res.bad_ticks[others] == 0).all()
    _assert_rollouts_equal(res, dict(qpos=good.qpos_hist, qvel=good.qvel_hist, tau=good.tau_hist,
                                     status=good.status_hist), good.bad_ticks, "others", others)


# ---- 9. refusals -------------------------------------------------------------------------------

def test_refusals_leave_nothing_enqueued(gpu):
    """OSC_ERR_INVALID_ARGUMENT from the three entries, every output and the workspace still
    holding their sentinel afterwards: a wheel-row model with env_params, a parameter pointer at an
    odd multiple of 4 bytes (either block), a kin / model pair of different robots, a workspace one
    byte short of osc_qpos_env_workspace_bytes."""
    from osc_amd.solver import OSCBatchSolver
    from test_gpu_wheels import NOSLIP_YAML
    L = _lib.lib()
    nenv = 5
    tree, qpos, qvel, T, mask = _tick_inputs(WALTER, nenv, 3)
    kw, kg = KinematicsBatch(tree=tree), setup(GO2)[1]
    sw, wheels = solver(WALTER), OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)
    assert wheels.wheels and (kw.nv, kw.ns) == (wheels.dims["nv"], wheels.dims["ns"])
    d = sw.dims
    SENT = -12345.0
    f64 = lambda *shape: torch.full(shape, SENT, dtype=torch.float64, device=gpu)
    i32 = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=gpu)
    need = kw.env_workspace_bytes(sw, nenv)
    assert need % 8 == 0
    outs = dict(tau=f64(nenv, d["nu"]), x=f64(nenv, d["n"]), status=i32(nenv), iters=i32(nenv),
                ws=f64(need // 8), M=f64(nenv, kw.nv, kw.nv), C=f64(nenv, kw.nv),
                J=f64(nenv, 6 * kw.ns, kw.nv), b=f64(nenv, 6 * kw.ns), qp=dev(qpos), qv=dev(qvel))
    before = {k: v.clone() for k, v in outs.items()}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    Td, md = dev(T), dev(mask)
    p = ker.draw(tree, nenv, 3)
    ms, mu = dev(p["mass_scale"]), dev(np.full(nenv, 0.6))
    kin_ok = _lib.OscKinEnvParams(mass_scale=ms.data_ptr())
    kin_odd = _lib.OscKinEnvParams(armature_scale=ms.data_ptr() + 4)
    env_ok = _lib.OscEnvParams(mu=mu.data_ptr())
    env_odd = _lib.OscEnvParams(mu=mu.data_ptr() + 4)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def tick(model, kb, ep, kp, ws_bytes=need, warm=None):
        return L.osc_batch_solve_qpos_env(
            model._h, kb._h, nenv, ptr(outs["qp"]), ptr(outs["qv"]), ptr(Td), ptr(md),
            ctypes.byref(ep) if ep else None, ctypes.byref(kp) if kp else None, None,
            ptr(outs["tau"]), ptr(outs["x"]), ptr(outs["status"]), ptr(outs["iters"]),
            ptr(warm) if warm is not None else None,
            ctypes.c_size_t(0 if warm is None else warm.numel() * 8), ptr(outs["ws"]),
            ctypes.c_size_t(ws_bytes), stream)

    def rollout(model, kb, ep, kp):
        a = _lib.OscRolloutArgs()
        a.nticks, a.dt, a.flags, a.target_mode = 2, DT, 0, _lib.ROLLOUT_TARGETS_HELD
        a.T, a.contact_mask = Td.data_ptr(), md.data_ptr()
        a.qpos, a.qvel, a.tau = outs["qp"].data_ptr(), outs["qv"].data_ptr(), outs["tau"].data_ptr()
        return L.osc_batch_rollout_env(model._h, kb._h, nenv, ctypes.byref(a),
                                       ctypes.byref(ep) if ep else None,
                                       ctypes.byref(kp) if kp else None, stream)

    def kinematics(kp):
        return L.osc_batch_kinematics_env(kw._h, nenv, ptr(outs["qp"]), ptr(outs["qv"]),
                                          ctypes.byref(kp), ptr(outs["M"]), ptr(outs["C"]),
                                          ptr(outs["J"]), ptr(outs["b"]), None, stream)

    warm = sw.alloc_warm_state(nenv)
    calls = {"wheel rows + env_params": lambda: tick(wheels, kw, env_ok, kin_ok),
             "wheel rows + env_params, warm": lambda: tick(wheels, kw, env_ok, kin_ok, warm=warm),
             "wheel rows + env_params, rollout": lambda: rollout(wheels, kw, env_ok, kin_ok),
             "odd kin pointer": lambda: tick(sw, kw, env_ok, kin_odd),
             "odd kin pointer, no env block": lambda: tick(sw, kw, None, kin_odd),
             "odd env pointer": lambda: tick(sw, kw, env_odd, kin_ok),
             "odd kin pointer, kinematics": lambda: kinematics(kin_odd),
             "odd kin pointer, rollout": lambda: rollout(sw, kw, env_ok, kin_odd),
             "odd env pointer, rollout": lambda: rollout(sw, kw, env_odd, kin_ok),
             "pair mismatch": lambda: tick(sw, kg, env_ok, kin_ok),
             "pair mismatch, rollout": lambda: rollout(sw, kg, env_ok, kin_ok),
             "workspace one byte short": lambda: tick(sw, kw, env_ok, kin_ok, ws_bytes=need - 1),
             "workspace one byte short, kin only": lambda: tick(sw, kw, None, kin_ok,
                                                                ws_bytes=need - 1)}
    sz = ctypes.c_size_t(0)
    assert L.osc_qpos_env_workspace_bytes(sw._h, kg._h, nenv, ctypes.byref(sz)) == 1
    assert L.osc_rollout_env_workspace_bytes(wheels._h, kw._h, nenv, 2, ctypes.byref(sz)) == 1
    for what, call in calls.items():
        assert call() == 1, what
        torch.cuda.synchronize()
        for k, v in outs.items():
            assert same(v, before[k]), (what, k)
    # the same arguments, nothing wrong with them: accepted, and the outputs are written
    assert tick(sw, kw, env_ok, kin_ok) == 0
    torch.cuda.synchronize()
    assert not (outs["tau"] == SENT).any() and not (outs["status"] == -77).any()


# ---- 10. memory bounds -------------------------------------------------------------------------

@pytest.mark.parametrize("nenv", [1, NENV])
@pytest.mark.parametrize("name", [GO2, "chain16"])
def test_no_access_outside_the_parameter_arrays_and_the_outputs(gpu, name, nenv):
    """The three parameter arrays, qpos, qvel and the five outputs each between guard bands at
    their exact sizes: the bands are intact after osc_batch_kinematics_env, the inputs unmodified,
    and the results are bitwise the ordinary call's whether the bands around the inputs hold 0x00
    or 0xFF -- so nothing outside the arrays is read (the tail rows read the clamped env)."""
    tree, kb, qpos, qvel, p = setup(name)
    rows = slice(0, nenv)
    ref = compute(kb, qpos[rows], qvel[rows], block(p, rows=rows))
    nv, s6 = kb.nv, 6 * kb.ns
    for pad in (0x00, 0xFF):
        fill = 0xA5 if pad == 0 else 0x5A
        ins = {k: guarded_like(dev(v[rows]), pad) for k, v in
               dict(p, qpos=qpos, qvel=qvel).items()}
        kept = {k: v.clone() for k, v in ins.items()}
        out = KinOutputs(*[guarded(shape, torch.float64, gpu, fill=fill) for shape in
                           ((nenv, nv, nv), (nenv, nv), (nenv, s6, nv), (nenv, s6),
                            (nenv, kb.ns, 3))])
        kp = KinEnvParams(**{k: ins[k] for k in FIELDS})
        c, keep = kp.to_device(nenv, kb.nbody, kb.nv, gpu)
        assert [t.data_ptr() for t in keep] == [ins[k].data_ptr() for k in FIELDS]
        kb.compute_into(out, ins["qpos"], ins["qvel"], kin_params=kp)
        torch.cuda.synchronize()
        for k in OUT:
            assert_guards_intact(getattr(out, k), k)
            assert same(getattr(out, k), getattr(ref, k)), (k, hex(pad))
        for k, t in ins.items():
            assert_guards_intact(t, "input " + k)
            assert same(t, kept[k]), k
