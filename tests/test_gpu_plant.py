"""GPU tests of the forward dynamics and of the rollout against a mismatched plant
(include/osc_plant.h, csrc/osc_forward_dynamics.hip, csrc/osc_rollout.hip; KinematicsBatch.
forward_dynamics(_into) and rollout(..., plant=)):
   4. the forward dynamics against the refined float64 reference (tests/plant_ref.py), at a bar
      of ten times the error of the numpy model of the kernel's LDL' on the same inputs;
   5. its bitwise properties: NULL z / qfrc, batch independence, a NaN row for a bad env, guard bands;
   6. no plant: plant=None and Plant() are bitwise rollout();
   7. the plant rollout bitwise against the loop a user would write from the entries;
   8. against the CPU chain of tests/plant_ref.py;
   9. the behaviour: an unknown payload sags, a known one does not;
  10. an env with invalid plant parameters stays frozen;
  11. argument errors enqueue nothing; the backward pass refuses a plant result."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import backward_ref as br
import kin_env_ref as ker
import plant_ref as pr
import rollout_ref
import test_gpu_rollout_backward as tb
import test_gpu_rollout_schedule as ts
from guard import assert_guards_intact, guarded, guarded_like
from osc_amd import _lib
from osc_amd.kinematics import KinEnvParams, Plant, RolloutSchedule
from osc_amd.solver import EnvParams

pytestmark = pytest.mark.gpu

GO2, WALTER = pr.GO2, pr.WALTER
DT = rollout_ref.DT
GAINS = rollout_ref.STANDING_GAINS
NORM_TOL = 1e-5       # the rollout chains' contract (tests/test_gpu_rollout_backward.py)
# 10 x the worst env_errors measured on an MI355X against the CPU chain (test 8), the rule of
# 2.74e-13 (WaLTER, qacc)
CHAIN_BAR = 3e-12
K4 = ts.K4
NBIG = ts.NBIG

dev, bitwise, pair = tb.dev, tb.bitwise, tb.pair


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ---- 4. forward dynamics against the reference --------------------------------------------------------

def fd_run(robot, rows, z=True, qfrc=True, M=None):
    """forward_dynamics_into on the oracle's M, C, J of plant_ref.fd_case(robot)[rows] -> numpy."""
    tree, kb, km, s, mdl = pair(robot)
    c = pr.fd_case(robot)
    n = len(c["u"][rows])
    qacc = ts.nan(n, km.nv)
    kb.forward_dynamics_into(s, qacc, dev(c["M"][rows] if M is None else M), dev(c["C"][rows]),
                             dev(c["J"][rows]), dev(c["u"][rows]),
                             dev(c["z"][rows]) if z else None,
                             dev(c["qfrc"][rows]) if qfrc else None)
    torch.cuda.synchronize()
    return qacc.cpu().numpy()


@functools.lru_cache(maxsize=None)
def fd_full(robot):
    return fd_run(robot, slice(0, 67))


@pytest.mark.parametrize("nenv", [1, 5, 67])
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_forward_dynamics_vs_the_reference(gpu, robot, nenv):
    """Go2 (NV 18: both column slots live) and WaLTER (NV 14 padded to 17, 24 contact rows); a lone
    DPP row, a partial second wavefront, 16 full wavefronts plus 3 envs.  Every env's
    |qacc - ref|_inf / max(|ref|_inf, 1) against the refined reference within 10 x the worst error
    of plant_ref.ldl_model on the same inputs (Go2 1.02e-15, WaLTER 7.8e-16), capped at 1e-10.
    Measured worst on an MI355X: Go2 1.73e-15, WaLTER 1.71e-15 (both at 67 envs)."""
    c = pr.fd_case(robot)
    got = fd_run(robot, slice(0, nenv))
    err = np.array([pr.fd_error(got[e], c["ref"][e]) for e in range(nenv)])
    bar = pr.fd_bar(robot)
    print(f"\nforward dynamics {robot} nenv={nenv}: worst {err.max():.2e}, model "
          f"{c['model_err'].max():.2e}, bar {bar:.2e}")
    assert np.isfinite(got).all()
    assert err.max() <= bar, (int(err.argmax()), err.max())


@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_forward_dynamics_wrapper_is_compute_then_the_entry(gpu, robot):
    """forward_dynamics(qpos, qvel, tau, z, qfrc, kin_params) is bitwise compute(kin_params=) then
    forward_dynamics_into, with u and z strided views of an x-shaped buffer; on the GPU's own M, C
    it is within cond(M) x the kinematics' rounding of the reference (1e-9)."""
    tree, kb, km, s, mdl = pair(robot)
    c = pr.fd_case(robot)
    n, nv, nu = 67, mdl.nv, mdl.nu
    kp = KinEnvParams(**{k: dev(c[k]) for k in KinEnvParams.FIELDS})
    got = kb.forward_dynamics(s, c["qpos"], c["qvel"], c["u"], c["z"], c["qfrc"], kin_params=kp)
    k = kb.compute(c["qpos"], c["qvel"], want_sites=False, kin_params=kp)
    x = ts.nan(n, nv + nu + 3 * mdl.nc)
    x[:, nv:nv + nu], x[:, nv + nu:] = dev(c["u"]), dev(c["z"])
    qacc = ts.nan(n, nv)
    kb.forward_dynamics_into(s, qacc, k.M, k.C, k.J, x[:, nv:nv + nu], x[:, nv + nu:],
                             dev(c["qfrc"]))
    torch.cuda.synchronize()
    assert torch.equal(got, qacc)
    err = max(pr.fd_error(got[e].cpu().numpy(), c["ref"][e]) for e in range(n))
    print(f"\nforward dynamics on the GPU's own kinematics, {robot}: worst {err:.2e}")
    assert err <= 1e-9


# ---- 5. bitwise properties ---------------------------------------------------------------------------------

@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_null_inputs_are_zero_arrays(gpu, robot):
    tree, kb, km, s, mdl = pair(robot)
    c = pr.fd_case(robot)
    n, rows = 67, slice(0, 67)
    M, C, J, u = (dev(c[k]) for k in ("M", "C", "J", "u"))
    z, f = dev(c["z"]), dev(c["qfrc"])
    z0, f0 = torch.zeros_like(z), torch.zeros_like(f)
    run = lambda J_, z_, f_: kb.forward_dynamics_into(s, ts.nan(n, km.nv), M, C, J_, u, z_, f_)
    assert torch.equal(run(J, None, f), run(J, z0, f))
    assert torch.equal(run(None, None, f), run(J, z0, f))       # without z, J is not read
    assert torch.equal(run(J, z, None), run(J, z, f0))
    assert torch.equal(run(None, None, None), run(J, z0, f0))
    assert not torch.equal(run(J, z, f), run(J, z0, f))
    assert bitwise(run(J, z, f).cpu().numpy(), fd_full(robot))


@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_an_envs_result_does_not_depend_on_its_batch(gpu, robot):
    full = fd_full(robot)
    assert bitwise(fd_run(robot, slice(0, 5)), full[0:5])
    assert bitwise(fd_run(robot, slice(0, 1)), full[0:1])
    assert bitwise(fd_run(robot, slice(64, 67)), full[64:67])
    assert bitwise(fd_run(robot, slice(0, 67)), full)


@pytest.mark.parametrize("what", ["nan", "negated diagonal", "nan in u", "inf in qfrc"])
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_a_bad_env_has_a_nan_row_and_the_others_do_not_move(gpu, robot, what):
    """Env 21 (a middle row of its wavefront) with a NaN in M, an M with a negated diagonal entry
    (a pivot <= 0), or a non-finite input: its whole qacc row is NaN, the other 66 are bitwise the
    clean batch's."""
    tree, kb, km, s, mdl = pair(robot)
    c = pr.fd_case(robot)
    full = fd_full(robot)
    e = 21
    t = {k: dev(c[k]) for k in ("M", "C", "J", "u", "z", "qfrc")}
    if what == "nan":
        t["M"][e, 3, 7] = float("nan")
        t["M"][e, 7, 3] = float("nan")
    elif what == "negated diagonal":
        t["M"][e, mdl.nv - 2, mdl.nv - 2] *= -1.0
    elif what == "nan in u":
        t["u"][e, 1] = float("nan")
    else:
        t["qfrc"][e, 0] = float("inf")
    got = kb.forward_dynamics_into(s, ts.nan(67, km.nv), t["M"], t["C"], t["J"], t["u"], t["z"],
                                   t["qfrc"]).cpu().numpy()
    assert np.isnan(got[e]).all()
    others = np.arange(67) != e
    assert bitwise(got[others], full[others])


@pytest.mark.parametrize("nenv", [1, 5, 67])
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_forward_dynamics_stays_inside_its_arrays(gpu, robot, nenv):
    """Every input and qacc between guard bands at its exact size (tests/guard.py), the inputs at
    the weakest alignment the entry allows (8 bytes): the bands intact, the inputs unmodified, the
    result bitwise the ordinary call's whether the bands around the inputs hold 0x00 or 0xFF."""
    tree, kb, km, s, mdl = pair(robot)
    c = pr.fd_case(robot)
    rows = slice(0, nenv)
    ref = fd_full(robot)[rows]
    for pad in (0x00, 0xFF):
        fill = 0xA5 if pad == 0 else 0x5A
        i = {k: guarded_like(dev(c[k][rows]), pad, offset_bytes=8)
             for k in ("M", "C", "J", "u", "z", "qfrc")}
        kept = {k: v.clone() for k, v in i.items()}
        qacc = guarded((nenv, km.nv), torch.float64, gpu, fill=fill, offset_bytes=8)
        kb.forward_dynamics_into(s, qacc, i["M"], i["C"], i["J"], i["u"], i["z"], i["qfrc"])
        torch.cuda.synchronize()
        assert_guards_intact(qacc, "qacc")
        for k, v in i.items():
            assert_guards_intact(v, k)
            assert torch.equal(v, kept[k]), k
        assert bitwise(qacc.cpu().numpy(), ref), hex(pad)


# ---- 6. no plant ------------------------------------------------------------------------------------------

def small_env_params(nenv, mdl):
    rng = np.random.default_rng(5)
    return EnvParams(mu=dev(rng.uniform(0.4, 1.0, nenv)), fz_ub=dev(rng.uniform(60.0, 90.0, nenv)))


def drawn_kin_params(tree, nenv, seed):
    p = ker.draw(tree, nenv, seed)
    return KinEnvParams(**{k: dev(p[k]) for k in KinEnvParams.FIELDS})


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("sched", [False, True])
@pytest.mark.parametrize("mode", ["held", "pd"])
def test_no_plant_is_bitwise_the_rollout(gpu, mode, sched, blocks):
    """plant=None and Plant() (osc_batch_rollout_plant with an all-NULL plant, and with a NULL one
    through the C entry) against rollout(): K = 4, 1, 0; held and PD targets; with and without a
    schedule, env_params and kin_params: every history, the final state, tau and bad_ticks."""
    tree, kb, km, s, mdl = pair(GO2)
    for nticks in (K4, 1, 0):
        c = ts.inputs(GO2, NBIG, nticks)
        kw = ts.held_kw(c, mode)
        if sched:
            kw["schedule"] = ts.schedule_of(c, ts.FIELDS[mode][-1])
        if blocks:
            kw.update(env_params=small_env_params(NBIG, mdl),
                      kin_params=drawn_kin_params(tree, NBIG, 3))
        run = lambda **p: kb.rollout(s, c["qpos"], c["qvel"], c["mask"], nticks, DT, warm=True,
                                     history=True, **kw, **p)
        plain, none, empty = run(), run(plant=None), run(plant=Plant())
        torch.cuda.synchronize()
        for r in (none, empty):
            assert ts.same_rollout(r, ts.as_ref(plain), plain.bad_ticks), nticks
            assert torch.equal(r.tau, plain.tau)
            assert r.qacc_hist is None and r.plant is None


def test_a_null_plant_through_the_c_entry(gpu):
    tree, kb, km, s, mdl = pair(GO2)
    c = ts.inputs(GO2, NBIG)
    plain = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, T=c["T"], history=True)
    qp, qv = dev(c["qpos"]), dev(c["qvel"])
    T, mask = dev(c["T"]), dev(c["mask"])
    hist = ts.nan(K4 + 1, NBIG, km.nq)
    a = _lib.OscRolloutArgs()
    a.nticks, a.dt, a.flags = K4, DT, _lib.ROLLOUT_WARM
    a.target_mode, a.T, a.contact_mask = _lib.ROLLOUT_TARGETS_HELD, T.data_ptr(), mask.data_ptr()
    a.qpos, a.qvel, a.qpos_hist = qp.data_ptr(), qv.data_ptr(), hist.data_ptr()
    nbytes = kb.rollout_workspace_bytes(s, NBIG, K4)          # the plain size is enough: no plant
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    rc = _lib.lib().osc_batch_rollout_plant(s._h, kb._h, NBIG, ctypes.byref(a), None, None, None,
                                            None, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(hist, plain.qpos_hist) and torch.equal(qp, plain.qpos)


# ---- 7. the user loop, bitwise ----------------------------------------------------------------------------

def plant_case(robot, nenv, nticks=K4):
    """ts.inputs(robot, nenv) with a plant on top: drawn plant parameters (seed 41), a held applied
    force and a per-tick one with a 30 N push along x at tick 1."""
    tree = pair(robot)[0]
    c = dict(ts.inputs(robot, nenv, nticks))
    nv = pair(robot)[2].nv
    rng = np.random.default_rng(43)
    c["plant_kp"] = ker.draw(tree, nenv, 41)
    c["qfrc"] = rng.uniform(-3, 3, (nenv, nv))
    c["qfrc_seq"] = rng.uniform(-3, 3, (nticks, nenv, nv))
    if nticks > 1:
        c["qfrc_seq"][1, :, 0] += 30.0
    return c


def user_loop(robot, c, mode, fields, nticks, warm, plant_kp=None, qfrc=None, qfrc_seq=None,
              ctrl_kp=None, ctrl_ep=None):
    """The loop a user would write: per tick the targets (ts.user_loop), solve_(warm_)into with
    the CONTROLLER's parameters, compute_into with the PLANT's (the controller's when it has none),
    forward_dynamics_into on the solve's u and z, integrate_into."""
    tree, kb, km, s, mdl = pair(robot)
    nenv, nv, nu, ns = c["qpos"].shape[0], km.nv, mdl.nu, mdl.ns
    qp, qv = dev(c["qpos"]), dev(c["qvel"])
    out = s.alloc_outputs(nenv, want_x=True)
    wstate = s.alloc_warm_state(nenv)
    ws = torch.empty((kb.workspace_bytes(s, nenv) // 8 + 2,), dtype=torch.float64, device="cuda")
    bad = torch.zeros(nenv, dtype=torch.int32, device="cuda")
    kout = kb.alloc(nenv)
    gains = (ctypes.c_double * 4)(*GAINS)
    kw = dict(env_params=ctrl_ep, kin_params=ctrl_kp)
    pk = plant_kp if plant_kp is not None else ctrl_kp
    h = dict(qpos=[qp.clone()], qvel=[qv.clone()], tau=[], status=[], qacc=[])
    for t in range(nticks):
        md = dev(c["mask_seq"][t] if "mask" in fields else c["mask"])
        if mode == "pd":
            pref = dev(c["pos_ref_seq"][t] if "pos_ref" in fields else c["pos_ref"])
            qref = dev(c["quat_ref_seq"][t] if "quat_ref" in fields else c["quat_ref"])
            Td = torch.empty((nenv, ns, 6), dtype=torch.float64, device="cuda")
            base = [qp[:, 0:3].contiguous(), qp[:, 3:7].contiguous(), qv[:, 0:3].contiguous(),
                    qv[:, 3:6].contiguous()]
            rc = _lib.lib().osc_pd_base_targets(nenv, ns, *[ptr(x) for x in base], ptr(pref), 1,
                                                ptr(qref), 0, gains, ptr(Td), stream())
            assert rc == 0
        else:
            Td = dev(c["T"])
        if "T" in fields:
            Td = Td + dev(c["T_seq"][t])
        if warm:
            kb.solve_warm_into(s, out, wstate, qp, qv, Td, md, ws, **kw)
        else:
            kb.solve_into(s, out, qp, qv, Td, md, ws, **kw)
        h["tau"].append(out.tau.clone())
        h["status"].append(out.status.clone())
        kb.compute_into(kout, qp, qv, kin_params=pk)
        f = qfrc_seq[t] if qfrc_seq is not None else qfrc
        qacc = torch.empty((nenv, nv), dtype=torch.float64, device="cuda")
        kb.forward_dynamics_into(s, qacc, kout.M, kout.C, kout.J, out.x[:, nv:nv + nu],
                                 out.x[:, nv + nu:], f)
        h["qacc"].append(qacc)
        kb.integrate_into(qp, qv, qacc, DT, status=out.status, bad_ticks=bad)
        h["qpos"].append(qp.clone())
        h["qvel"].append(qv.clone())
    torch.cuda.synchronize()
    return {k: torch.stack(v) for k, v in h.items()}, bad


def same_plant_rollout(r, ref, bad):
    return ts.same_rollout(r, ref, bad) and torch.equal(r.qacc_hist, ref["qacc"])


PLANT_CASES = ("kin", "held", "seq", "all")


def plant_of(c, what):
    """(Plant, the user loop's keywords) of one case."""
    kp = KinEnvParams(**{k: dev(c["plant_kp"][k]) for k in KinEnvParams.FIELDS})
    held, seq = dev(c["qfrc"]), dev(c["qfrc_seq"])
    if what == "kin":
        return Plant(kin_params=kp), dict(plant_kp=kp)
    if what == "held":
        return Plant(qfrc_applied=held), dict(qfrc=held)
    if what == "seq":
        return Plant(qfrc_applied=seq), dict(qfrc_seq=seq)
    return Plant(kin_params=kp, qfrc_applied=seq), dict(plant_kp=kp, qfrc_seq=seq)


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("what", PLANT_CASES)
@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("robot,nenv", [(GO2, NBIG), (WALTER, 5)])
def test_plant_rollout_bitwise_vs_the_user_loop(gpu, robot, nenv, mode, what, warm):
    """Four ticks against a plant -- its parameters alone, a held applied force, a per-tick one,
    all together -- held and PD targets, warm and cold: every history, qacc_hist, the statuses,
    bad_ticks and the final state bitwise the user loop's; a caller workspace and the library's
    scratch agree; the plant is felt."""
    tree, kb, km, s, mdl = pair(robot)
    c = plant_case(robot, nenv)
    plant, lkw = plant_of(c, what)
    kw = ts.held_kw(c, mode)
    run = lambda **p: kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm,
                                 history=True, plant=plant, **kw, **p)
    res, res2 = run(), run(workspace=None)
    ref, bad = user_loop(robot, c, mode, (), K4, warm, **lkw)
    torch.cuda.synchronize()
    assert same_plant_rollout(res, ref, bad) and same_plant_rollout(res2, ref, bad)
    assert (res.status_hist == 0).all() and torch.isfinite(res.qacc_hist).all()
    assert res.plant is plant
    plain = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, history=True, **kw)
    assert not torch.equal(plain.qpos_hist, res.qpos_hist)
    nohist = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, plant=plant, **kw)
    torch.cuda.synchronize()
    assert torch.equal(nohist.qpos, res.qpos) and torch.equal(nohist.tau, res.tau)
    assert nohist.qacc_hist is None


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("mode", ["held", "pd"])
@pytest.mark.parametrize("robot,nenv", [(GO2, NBIG), (WALTER, 5)])
def test_plant_rollout_with_everything_bitwise_vs_the_user_loop(gpu, robot, nenv, mode, warm):
    """All together once more under a controller with its own kin_params and env_params and a
    RolloutSchedule of every field (the mask flips a contact at ticks 1 and 3)."""
    tree, kb, km, s, mdl = pair(robot)
    c = plant_case(robot, nenv)
    plant, lkw = plant_of(c, "all")
    fields = ts.FIELDS[mode][-1]
    ctrl_kp, ctrl_ep = drawn_kin_params(tree, nenv, 3), small_env_params(nenv, mdl)
    res = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, history=True,
                     plant=plant, schedule=ts.schedule_of(c, fields), env_params=ctrl_ep,
                     kin_params=ctrl_kp, **ts.held_kw(c, mode))
    ref, bad = user_loop(robot, c, mode, fields, K4, warm, ctrl_kp=ctrl_kp, ctrl_ep=ctrl_ep, **lkw)
    assert same_plant_rollout(res, ref, bad)
    # the controller's parameters with a plant that has none of its own: the tick's M, C
    held = dev(c["qfrc"])
    res = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, warm=warm, history=True,
                     plant=Plant(qfrc_applied=held), kin_params=ctrl_kp, **ts.held_kw(c, mode))
    ref, bad = user_loop(robot, c, mode, (), K4, warm, ctrl_kp=ctrl_kp, qfrc=held)
    assert same_plant_rollout(res, ref, bad)


# ---- 8. against the CPU chain -----------------------------------------------------------------------------

@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_plant_rollout_vs_the_cpu_chain(gpu, robot):
    """5 envs, K = 3, held targets, the plant's parameters drawn (the controller keeps the
    model's), a held applied force plus a 30 N push at tick 1: qpos, qvel, tau and qacc histories,
    every tick and env, by backward_ref.env_errors within the rollout chains' 1e-5 contract and
    within CHAIN_BAR, ten times the worst measured on an MI355X; the reference
    (plant_ref.chain_case) asserts a certified optimum at every env and tick.
    Measured worst: Go2 qpos 1.8e-16, qvel 1.2e-14, tau 2.3e-14, qacc 2.3e-14; WaLTER qpos 2.1e-16,
    qvel 1.8e-13, tau 2.5e-13, qacc 2.7e-13."""
    tree, kb, km, s, mdl = pair(robot)
    c = pr.chain_case(robot)
    K = c["qfrc_seq"].shape[0]
    kp = KinEnvParams(**{k: dev(c[k]) for k in KinEnvParams.FIELDS})
    res = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K, DT, T=c["T"], warm=False,
                     history=True, plant=Plant(kin_params=kp, qfrc_applied=c["qfrc_seq"]))
    torch.cuda.synchronize()
    assert (res.status_hist == 0).all() and (res.bad_ticks == 0).all()
    got = dict(qpos=res.qpos_hist, qvel=res.qvel_hist, tau=res.tau_hist, qacc=res.qacc_hist)
    for k, g in got.items():
        g, r = g.cpu().numpy(), c["ref_" + k]
        first = 1 if k in ("qpos", "qvel") else 0        # slab 0 is the input
        e = np.concatenate([br.env_errors(g[t], r[t]) for t in range(first, len(r))])
        print(f"\nplant chain {robot} {k}: worst {e.max():.3e}")
        assert e.max() <= NORM_TOL, (k, e.max())
        assert e.max() <= CHAIN_BAR, (k, e.max())


# ---- 9. behaviour -----------------------------------------------------------------------------------------

def test_an_unknown_payload_sags_on_the_gpu(gpu):
    """rollout_ref.go2_case three times in one batch, K = 100: env 0 matched, env 1 the trunk
    1.5 x heavier in the plant only, env 2 in the controller's model too.  Env 1's base ends more
    than 5 mm below its reference, envs 0 and 2 more than 5 mm above and converging (the CPU
    reference's figures, tests/test_plant_ref.py: -0.00745, +0.00646, +0.00646).  Without a plant
    env 1 cannot be told apart from env 0."""
    tree, kb, km, s, mdl = pair(GO2)
    _, _, qpos, qvel, mask, pd = rollout_ref.go2_case()
    rep = lambda a: np.tile(np.asarray(a, float), (3, 1))
    ctrl, plant = np.ones((3, kb.nbody)), np.ones((3, kb.nbody))
    plant[1, 0] = plant[2, 0] = ctrl[2, 0] = pr.TRUNK_SCALE
    res = kb.rollout(s, rep(qpos), rep(qvel), rep(mask), 100, DT, pd=pd, warm=True,
                     kin_params=KinEnvParams(mass_scale=dev(ctrl)),
                     plant=Plant(kin_params=KinEnvParams(mass_scale=dev(plant))))
    torch.cuda.synchronize()
    assert (res.bad_ticks == 0).all()
    ez = res.qpos[:, 2].cpu().numpy() - pd[0][2]
    print(f"\nz error after 100 ticks (matched, plant 1.5 x, both 1.5 x): {ez}")
    assert ez[1] < -0.005 and ez[0] > 0.005 and ez[2] > 0.005


def test_a_push_moves_the_base_on_the_gpu(gpu):
    tree, kb, km, s, mdl = pair(GO2)
    _, _, qpos, qvel, mask, pd = rollout_ref.go2_case()
    run = lambda f: kb.rollout(s, qpos[None], qvel[None], mask[None], 100, DT, pd=pd,
                               plant=Plant(qfrc_applied=f)).qpos[0, 0].item()
    seq = pr.go2_push_seq(100, km.nv)[:, None, :]
    dx = run(seq) - run(np.zeros_like(seq))
    print(f"\nfinal base x, push against no push: {dx:.3e}")
    assert abs(dx) > 5e-4


# ---- 10. frozen envs --------------------------------------------------------------------------------------

@pytest.mark.parametrize("warm", [True, False])
def test_invalid_plant_parameters_freeze_the_env(gpu, warm):
    """mass_scale <= 0 on one body of env 2 of the PLANT (the controller's model is fine, its
    solves are OK): env 2's state is unchanged, bad_ticks = K, no NaN in any state; every other env
    is bitwise the run without it."""
    tree, kb, km, s, mdl = pair(GO2)
    c = plant_case(GO2, 5)
    ms = np.array(c["plant_kp"]["mass_scale"])
    good = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, T=c["T"], warm=warm,
                      history=True, plant=Plant(kin_params=KinEnvParams(mass_scale=dev(ms))))
    ms[2, 3] = -1.0
    got = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, T=c["T"], warm=warm,
                     history=True, plant=Plant(kin_params=KinEnvParams(mass_scale=dev(ms))))
    torch.cuda.synchronize()
    assert got.bad_ticks.tolist() == [0, 0, K4, 0, 0]
    assert (got.status_hist == 0).all()                      # the controller's solve is fine
    assert torch.equal(got.qpos[2], dev(c["qpos"][2])) and torch.equal(got.qvel[2], dev(c["qvel"][2]))
    assert torch.isnan(got.qacc_hist[:, 2]).all()
    assert torch.isfinite(got.qpos_hist).all() and torch.isfinite(got.qvel_hist).all()
    o = [0, 1, 3, 4]
    for k in ("qpos_hist", "qvel_hist", "tau_hist", "qacc_hist"):
        assert torch.equal(getattr(got, k)[:, o], getattr(good, k)[:, o]), k


# ---- 11. argument errors, guard bands of the rollout ------------------------------------------------------

def raw_plant_call(robot, c, nenv, plant, ws, nbytes, hist):
    tree, kb, km, s, mdl = pair(robot)
    qp, qv = dev(c["qpos"][:nenv]), dev(c["qvel"][:nenv])
    T, mask = dev(c["T"][:nenv]), dev(c["mask"][:nenv])
    a = _lib.OscRolloutArgs()
    a.nticks, a.dt, a.flags = K4, DT, _lib.ROLLOUT_WARM
    a.target_mode, a.T, a.contact_mask = _lib.ROLLOUT_TARGETS_HELD, T.data_ptr(), mask.data_ptr()
    a.qpos, a.qvel, a.qpos_hist = qp.data_ptr(), qv.data_ptr(), hist.data_ptr()
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    rc = _lib.lib().osc_batch_rollout_plant(s._h, kb._h, nenv, ctypes.byref(a), None, None, None,
                                            ctypes.byref(plant), stream())
    torch.cuda.synchronize()
    return rc, qp


@pytest.mark.parametrize("nenv", [5, 17])
def test_plant_rollout_stays_inside_its_arrays(gpu, nenv):
    """osc_batch_rollout_plant through the C entry with the plant's parameters, the per-tick
    applied force, qacc_hist and the workspace (at exactly osc_rollout_plant_workspace_bytes)
    between guard bands: the bands intact, the inputs unmodified, results bitwise the wrapper's."""
    tree, kb, km, s, mdl = pair(GO2)
    c = plant_case(GO2, NBIG)
    kp = {k: c["plant_kp"][k][:nenv] for k in KinEnvParams.FIELDS}
    ref = kb.rollout(s, c["qpos"][:nenv], c["qvel"][:nenv], c["mask"][:nenv], K4, DT,
                     T=c["T"][:nenv], history=True,
                     plant=Plant(kin_params=KinEnvParams(**{k: dev(v) for k, v in kp.items()}),
                                 qfrc_applied=c["qfrc_seq"][:, :nenv]))
    nbytes = kb.rollout_workspace_bytes(s, nenv, K4, plant=True)
    assert nbytes > kb.rollout_workspace_bytes(s, nenv, K4)
    for pad in (0x00, 0xFF):
        fill = 0xA5 if pad == 0 else 0x5A
        i = {k: guarded_like(dev(v), pad) for k, v in kp.items()}
        i["qfrc_seq"] = guarded_like(dev(np.ascontiguousarray(c["qfrc_seq"][:, :nenv])), pad)
        kept = {k: v.clone() for k, v in i.items()}
        qh = guarded((K4, nenv, km.nv), torch.float64, gpu, fill=fill)
        hist = guarded((K4 + 1, nenv, km.nq), torch.float64, gpu, fill=fill)
        ws = guarded((nbytes // 8,), torch.float64, gpu, fill=fill, env_bytes=nbytes // nenv)
        ck = _lib.OscKinEnvParams(**{k: i[k].data_ptr() for k in kp})
        pl = _lib.OscRolloutPlant(kin_params=ctypes.pointer(ck),
                                  qfrc_applied_seq=i["qfrc_seq"].data_ptr(),
                                  qacc_hist=qh.data_ptr())
        rc, qp = raw_plant_call(GO2, c, nenv, pl, ws, nbytes, hist)
        assert rc == 0
        for k, t in dict(i, qacc_hist=qh, qpos_hist=hist, workspace=ws).items():
            assert_guards_intact(t, k)
        assert all(torch.equal(i[k], kept[k]) for k in i)
        assert torch.equal(qh, ref.qacc_hist) and torch.equal(hist, ref.qpos_hist)
        assert torch.equal(qp, ref.qpos)


def test_refusals_enqueue_nothing(gpu):
    """A misaligned qfrc / qfrc_seq / qacc_hist / plant parameter pointer, a workspace one byte
    short of osc_rollout_plant_workspace_bytes and a wheel-row model each return 1; the state
    and the history (pre-filled with NaN) stay as they are.  The forward dynamics' own refusals
    leave qacc untouched."""
    tree, kb, km, s, mdl = pair(GO2)
    n = 5
    c = plant_case(GO2, NBIG)
    f = dev(c["qfrc"][:n])
    fs = dev(np.ascontiguousarray(c["qfrc_seq"][:, :n]))
    qh = ts.nan(K4, n, km.nv)
    hist = ts.nan(K4 + 1, n, km.nq)
    nbytes = kb.rollout_workspace_bytes(s, n, K4, plant=True)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    ck = _lib.OscKinEnvParams(mass_scale=dev(np.ones((n, kb.nbody))).data_ptr() + 4)
    P = _lib.OscRolloutPlant
    bad = [("odd qfrc", P(qfrc_applied=f.data_ptr() + 4), nbytes),
           ("odd qfrc_seq", P(qfrc_applied_seq=fs.data_ptr() + 4), nbytes),
           ("odd qacc_hist", P(qfrc_applied=f.data_ptr(), qacc_hist=qh.data_ptr() + 4), nbytes),
           ("odd plant mass_scale", P(kin_params=ctypes.pointer(ck)), nbytes),
           ("short workspace", P(qfrc_applied=f.data_ptr(), qacc_hist=qh.data_ptr()), nbytes - 1),
           ("the plain rollout's workspace", P(qfrc_applied=f.data_ptr()),
            kb.rollout_workspace_bytes(s, n, K4))]
    for what, pl, nb in bad:
        rc, qp = raw_plant_call(GO2, c, n, pl, ws, nb, hist)
        assert rc == 1, what
        assert torch.isnan(hist).all() and torch.isnan(qh).all(), what
        assert torch.equal(qp, dev(c["qpos"][:n])), what
    rc, qp = raw_plant_call(GO2, c, n, P(qfrc_applied=f.data_ptr(), qacc_hist=qh.data_ptr()), ws,
                            nbytes, hist)
    assert rc == 0 and torch.isfinite(hist).all() and torch.isfinite(qh).all()

    # a wheel-row model: refused by the rollout and by the forward dynamics
    from osc_amd.solver import OSCBatchSolver
    from test_gpu_wheels import NOSLIP_YAML
    sw = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)       # same nv / ns as walter_sr
    assert sw.wheels
    tw, kw_, kmw, _, mw = pair(WALTER)
    cw = pr.fd_case(WALTER)
    qacc = ts.nan(n, kmw.nv)
    with pytest.raises(_lib.OSCError):
        kw_.forward_dynamics_into(sw, qacc, dev(cw["M"][:n]), dev(cw["C"][:n]), dev(cw["J"][:n]),
                                  dev(cw["u"][:n]), dev(cw["z"][:n]), None)
    nb = ctypes.c_size_t()
    assert _lib.lib().osc_rollout_plant_workspace_bytes(sw._h, kw_._h, n, K4,
                                                        ctypes.byref(nb)) == 1
    # the forward dynamics: strides shorter than a row, z without J, misaligned pointers
    M, C, J, u, z = (dev(c_[:n]) for c_ in (cw["M"], cw["C"], cw["J"], cw["u"], cw["z"]))
    _, _, _, sW, _ = pair(WALTER)
    L, nu, nz = _lib.lib(), mw.nu, 3 * mw.nc
    call = lambda **k: L.osc_batch_forward_dynamics(
        sW._h, k.get("n", n), ptr(M), ptr(C), k.get("J", ptr(J)), k.get("u", ptr(u)),
        k.get("us", nu), k.get("z", ptr(z)), k.get("zs", nz), k.get("f", None),
        k.get("q", ptr(qacc)), stream())
    assert call(us=nu - 1) == 1 and call(zs=nz - 1) == 1 and call(J=None) == 1
    assert call(n=-1) == 1 and call(u=None) == 1 and call(q=None) == 1
    for k, t in (("J", J), ("u", u), ("z", z), ("q", qacc), ("f", u)):
        assert call(**{k: ctypes.c_void_p(t.data_ptr() + 4)}) == 1, k
    torch.cuda.synchronize()
    assert torch.isnan(qacc).all()
    assert call(n=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(qacc).all()


def test_the_backward_pass_refuses_a_plant_result(gpu):
    from osc_amd.autograd import rollout_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    c = plant_case(GO2, 5)
    plant = Plant(qfrc_applied=dev(c["qfrc"]))
    res = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, T=c["T"], history=True,
                     plant=plant)
    with pytest.raises(NotImplementedError, match="osc_plant.h"):
        kb.rollout_backward(s, res, c["mask"], DT, T=c["T"],
                            grad_qpos_hist=torch.ones_like(res.qpos_hist))
    with pytest.raises(NotImplementedError, match="osc_plant.h"):
        rollout_differentiable(s, kb, dev(c["qpos"]), dev(c["qvel"]), dev(c["mask"]), K4, DT,
                               T=dev(c["T"]), plant=plant)
    # an empty Plant() is no plant: the backward pass runs as before
    res = kb.rollout(s, c["qpos"], c["qvel"], c["mask"], K4, DT, T=c["T"], history=True,
                     plant=Plant())
    g = kb.rollout_backward(s, res, c["mask"], DT, T=c["T"],
                            grad_qpos_hist=torch.ones_like(res.qpos_hist))
    torch.cuda.synchronize()
    assert torch.isfinite(g["qpos0"]).all()
