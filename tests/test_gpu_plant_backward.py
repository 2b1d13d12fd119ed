"""GPU tests of the forward dynamics' vector-Jacobian product (include/osc_plant_backward.h,
csrc/osc_forward_dynamics_backward.hip; KinematicsBatch.forward_dynamics_backward and
autograd.forward_dynamics_differentiable):
   1. every output against the float64 closed form on the refined w (tests/plant_backward_ref.py),
      at a bar of ten times the error of the numpy model of the kernel's LDL' on the same inputs;
   2. its bitwise properties: z = None, batch independence, every NULL output, a repeated call,
      strided rows;
   3. a bad env has zeros in every output and its wave-mates do not move;
   4. guard bands around every input and output, the strided ones included;
   5. argument errors launch nothing;
   6. autograd: gradcheck, and only what is asked for is filled;
and of the rollout's backward through a plant (osc_batch_rollout_plant_backward; KinematicsBatch.
rollout_plant_backward, autograd.rollout_plant_differentiable):
   7. a result without a plant: bitwise rollout_backward;
   8. against the same kernels composed by hand, tick by tick on the forward's checkpoints;
   9. against the CPU chain (tests/plant_backward_ref.py) and central differences of GPU rollouts;
  10. its bitwise properties: the held force's sum, batch independence, scaling, NULL outputs;
  11. an env with invalid plant parameters; guard bands; refusals; autograd; the behaviour."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import backward_ref as br
import kin_env_ref as ker
import plant_backward_ref as pbr
import plant_ref as pr
import rollout_ref
import test_gpu_rollout_backward as tb
from guard import assert_guards_intact, guarded, guarded_like
from osc_amd import _lib
from osc_amd.kinematics import KinEnvParams, Plant, RolloutResult, RolloutSchedule
from osc_amd.solver import EnvParams

pytestmark = pytest.mark.gpu

GO2, WALTER = pr.GO2, pr.WALTER
ROBOTS = [GO2, WALTER]
OUT = pbr.OUTPUTS
N = 67
BAD = 21                  # a middle row of its wavefront

dev, bitwise, pair = tb.dev, tb.bitwise, tb.pair


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def shapes(mdl, n):
    nv, nu, nz = mdl.nv, mdl.nu, 3 * mdl.nc
    return dict(M=(n, nv, nv), C=(n, nv), Jc=(n, nz, nv), u=(n, nu), z=(n, nz), qfrc=(n, nv))


def inputs(robot, rows):
    c = pbr.bw_case(robot)
    return {k: dev(c[k][rows]) for k in ("M", "J", "z", "qacc", "g")}


def run(robot, rows=slice(0, N), want=OUT, t=None, z=True):
    """forward_dynamics_backward on bw_case(robot)[rows] (or the device tensors t) -> name -> numpy
    of the outputs in `want`, each NaN-filled before the call."""
    tree, kb, km, s, mdl = pair(robot)
    t = inputs(robot, rows) if t is None else t
    n = int(t["qacc"].shape[0])
    if not z:
        want = tuple(k for k in want if k not in ("Jc", "z"))
    out = {k: nan(*shapes(mdl, n)[k]) for k in want}
    kb.forward_dynamics_backward(s, t["M"], t["J"] if z else None, t["z"] if z else None,
                                 t["qacc"], t["g"], **{"grad_" + k: v for k, v in out.items()})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def full(robot):
    return run(robot)


# ---- 1. against the reference ---------------------------------------------------------------------------

@pytest.mark.parametrize("nenv", [1, 5, N])
@pytest.mark.parametrize("robot", ROBOTS)
def test_every_output_vs_the_closed_form(gpu, robot, nenv):
    """Go2 (NV 18: both column slots live, 12 contact rows) and WaLTER (NV 14 padded to 17, 24
    contact rows: two per lane); a lone DPP row, a partial second wavefront, 16 full wavefronts
    plus 3 envs.  Every env's |got - ref|_inf / max(|ref|_inf, 1) of every output against the
    closed form on the refined w within 10 x the worst error of plant_ref.ldl_model's w on the same
    inputs (Go2 1.19e-15, WaLTER 9.96e-16), capped at 1e-10.
    Measured worst on an MI355X at 67 envs, M / C / Jc / u / z / qfrc:
      Go2     1.59e-15 / 1.58e-15 / 1.56e-15 / 1.58e-15 / 1.51e-15 / 1.58e-15
      WaLTER  1.52e-15 / 1.52e-15 / 1.57e-15 / 1.52e-15 / 1.48e-15 / 1.52e-15"""
    c = pbr.bw_case(robot)
    got = run(robot, slice(0, nenv))
    bar = pbr.bw_bar(robot)
    worst = {}
    for k in OUT:
        assert np.isfinite(got[k]).all(), k
        err = pbr.out_errors(got[k], c["grads"][k][:nenv])
        worst[k] = float(err.max())
    print(f"\nforward dynamics backward {robot} nenv={nenv}: worst "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f", model {c['bw_model_err'].max():.2e}, bar {bar:.2e}")
    for k in OUT:
        assert worst[k] <= bar, (k, worst[k], bar)


# ---- 2. bitwise properties --------------------------------------------------------------------------------

@pytest.mark.parametrize("robot", ROBOTS)
def test_no_contact_force_is_a_zero_contact_force(gpu, robot):
    """z = None (and then J = None) against z = 0 with J given: the four outputs that remain are
    bitwise the same, and with z = 0 the contact-row gradient is zero while Jc w is not."""
    t = inputs(robot, slice(0, N))
    none = run(robot, t=t, z=False)
    t0 = dict(t, z=torch.zeros_like(t["z"]))
    zero = run(robot, t=t0)
    assert sorted(none) == ["C", "M", "qfrc", "u"]
    for k in none:
        assert bitwise(none[k], zero[k]) and bitwise(none[k], full(robot)[k]), k
    assert not zero["Jc"].any()
    assert bitwise(zero["z"], full(robot)["z"])
    # J is read for grad_z alone: without that output it may be absent
    tree, kb, km, s, mdl = pair(robot)
    gJc = nan(*shapes(mdl, N)["Jc"])
    kb.forward_dynamics_backward(s, t["M"], None, t["z"], t["qacc"], t["g"], grad_Jc=gJc)
    assert bitwise(gJc.cpu().numpy(), full(robot)["Jc"])


@pytest.mark.parametrize("robot", ROBOTS)
def test_an_envs_result_does_not_depend_on_its_batch(gpu, robot):
    f = full(robot)
    for rows in (slice(0, 5), slice(64, 67), slice(0, 1)):
        got = run(robot, rows)
        for k in OUT:
            assert bitwise(got[k], f[k][rows]), (k, rows)


@pytest.mark.parametrize("robot", ROBOTS)
def test_a_null_output_leaves_the_others_unchanged(gpu, robot):
    """Each output alone, and all but each: bitwise the values of the call with all six; and a
    repeated call gives the same bits."""
    f = full(robot)
    again = run(robot)
    for k in OUT:
        assert bitwise(again[k], f[k]), k
        alone = run(robot, want=(k,))
        assert list(alone) == [k] and bitwise(alone[k], f[k]), k
        rest = run(robot, want=tuple(o for o in OUT if o != k))
        assert k not in rest
        for o in rest:
            assert bitwise(rest[o], f[o]), (k, o)


@pytest.mark.parametrize("robot", ROBOTS)
def test_strided_rows_are_the_dense_call(gpu, robot):
    """z, grad_qacc, grad_u and grad_z as views of x-shaped buffers (the rollout's layout): bitwise
    the dense call, and the buffers' other columns are left alone."""
    tree, kb, km, s, mdl = pair(robot)
    nv, nu, nz = mdl.nv, mdl.nu, 3 * mdl.nc
    nx = nv + nu + nz
    t = inputs(robot, slice(0, N))
    xin, gin, gout = nan(N, nx), nan(N, nx + 3), nan(N, nx)
    xin[:, nv + nu:] = t["z"]
    gin[:, 3:3 + nv] = t["g"]
    sh = shapes(mdl, N)
    out = {k: nan(*sh[k]) for k in ("M", "C", "Jc", "qfrc")}
    kb.forward_dynamics_backward(s, t["M"], t["J"], xin[:, nv + nu:], t["qacc"], gin[:, 3:3 + nv],
                                 grad_u=gout[:, nv:nv + nu], grad_z=gout[:, nv + nu:],
                                 **{"grad_" + k: v for k, v in out.items()})
    torch.cuda.synchronize()
    f = full(robot)
    for k, v in out.items():
        assert bitwise(v.cpu().numpy(), f[k]), k
    assert bitwise(gout[:, nv:nv + nu].cpu().numpy(), f["u"])
    assert bitwise(gout[:, nv + nu:].cpu().numpy(), f["z"])
    assert torch.isnan(gout[:, :nv]).all()


# ---- 3. a bad env --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["nan in M", "negated diagonal", "nan in qacc", "inf in grad_qacc",
                                  "nan in z", "inf in a contact row of J"])
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_bad_env_has_zeros_and_the_others_do_not_move(gpu, robot, what):
    """Env 21 with a NaN in M, an M with a negated diagonal entry (a pivot <= 0), or a non-finite
    entry in qacc, grad_qacc, z or a contact row of J: every output of that env is zero (no NaN),
    the other 66 are bitwise the clean batch's."""
    tree, kb, km, s, mdl = pair(robot)
    t = inputs(robot, slice(0, N))
    e = BAD
    if what == "nan in M":
        t["M"][e, 3, 7] = float("nan")
        t["M"][e, 7, 3] = float("nan")
    elif what == "negated diagonal":
        t["M"][e, mdl.nv - 2, mdl.nv - 2] *= -1.0
    elif what == "nan in qacc":
        t["qacc"][e, 1] = float("nan")
    elif what == "inf in grad_qacc":
        t["g"][e, mdl.nv - 1] = float("inf")
    elif what == "nan in z":
        t["z"][e, 3 * mdl.nc - 1] = float("nan")
    else:
        t["J"][e, 3 * mdl.ns - 2, 4] = float("inf")
    got = run(robot, t=t)
    others = np.arange(N) != e
    f = full(robot)
    for k in OUT:
        assert not got[k][e].any() and np.isfinite(got[k][e]).all(), k
        assert bitwise(got[k][others], f[k][others]), k


# ---- 4. guard bands -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nenv", [1, 5, N])
@pytest.mark.parametrize("robot", ROBOTS)
def test_the_kernel_stays_inside_its_arrays(gpu, robot, nenv):
    """Every input and output between guard bands at its exact size (tests/guard.py) and at the
    weakest alignment the entry allows (8 bytes); z, grad_qacc, grad_u and grad_z once dense and
    once as the LAST columns of a strided buffer, so that a row overrun of the last env leaves the
    payload.  The bands intact, the inputs unmodified, the results bitwise the ordinary call's
    whether the bands around the inputs hold 0x00 or 0xFF."""
    tree, kb, km, s, mdl = pair(robot)
    nv, nu, nz = mdl.nv, mdl.nu, 3 * mdl.nc
    rows = slice(0, nenv)
    f = {k: v[rows] for k, v in full(robot).items()}
    src = inputs(robot, rows)
    sh = shapes(mdl, nenv)
    for strided in (False, True):
        for pad in (0x00, 0xFF):
            fill = 0xA5 if pad == 0 else 0x5A
            i = {k: guarded_like(src[k], pad, offset_bytes=8) for k in ("M", "J", "qacc")}
            out = {k: guarded(sh[k], torch.float64, gpu, fill=fill, offset_bytes=8)
                   for k in ("M", "C", "Jc", "qfrc")}
            if strided:
                hz = guarded_like(torch.cat([src["g"], src["z"]], 1), pad, offset_bytes=8)
                hg = guarded_like(torch.cat([src["z"], src["g"]], 1), pad, offset_bytes=8)
                i.update(hz=hz, hg=hg)
                z, g = hz[:, nv:], hg[:, nz:]
                ho = guarded((nenv, nv + nu + nz), torch.float64, gpu, fill=fill, offset_bytes=8)
                hu = guarded((nenv, nz + nu), torch.float64, gpu, fill=fill, offset_bytes=8)
                out.update(ho=ho, hu=hu)
                gz, gu = ho[:, nv + nu:], hu[:, nz:]
            else:
                i["z"] = z = guarded_like(src["z"], pad, offset_bytes=8)
                i["g"] = g = guarded_like(src["g"], pad, offset_bytes=8)
                out["z"] = gz = guarded(sh["z"], torch.float64, gpu, fill=fill, offset_bytes=8)
                out["u"] = gu = guarded(sh["u"], torch.float64, gpu, fill=fill, offset_bytes=8)
            kept = {k: v.clone() for k, v in i.items()}
            kb.forward_dynamics_backward(s, i["M"], i["J"], z, i["qacc"], g, grad_M=out["M"],
                                         grad_C=out["C"], grad_Jc=out["Jc"], grad_u=gu, grad_z=gz,
                                         grad_qfrc=out["qfrc"])
            torch.cuda.synchronize()
            for k, v in list(i.items()) + list(out.items()):
                assert_guards_intact(v, k)
            for k, v in i.items():
                assert torch.equal(v, kept[k]), k
            for k in ("M", "C", "Jc", "qfrc"):
                assert bitwise(out[k].cpu().numpy(), f[k]), (k, strided, hex(pad))
            assert bitwise(gu.cpu().numpy(), f["u"]) and bitwise(gz.cpu().numpy(), f["z"])
            if strided:     # the holders' other columns still hold the fill
                byte = lambda v: v.contiguous().view(torch.uint8)
                assert (byte(ho[:, :nv + nu]) == fill).all() and (byte(hu[:, :nz]) == fill).all()


# ---- 5. argument errors -------------------------------------------------------------------------------------

def test_refusals_launch_nothing(gpu):
    """Every refusal of include/osc_plant_backward.h returns OSC_ERR_INVALID_ARGUMENT and leaves the
    outputs untouched; the same call without the fault runs.  A wheel-row model is refused."""
    tree, kb, km, s, mdl = pair(WALTER)
    n, nv, nu, nz = 5, mdl.nv, mdl.nu, 3 * mdl.nc
    t = inputs(WALTER, slice(0, n))
    sh = shapes(mdl, n)
    out = {k: nan(*sh[k]) for k in OUT}
    L = _lib.lib()
    order = ("model", "n", "M", "J", "z", "zs", "qacc", "g", "gs", "oM", "oC", "oJc", "ou", "ous",
             "oz", "ozs", "of")
    base = dict(model=s._h, n=n, M=ptr(t["M"]), J=ptr(t["J"]), z=ptr(t["z"]), zs=nz,
                qacc=ptr(t["qacc"]), g=ptr(t["g"]), gs=nv, oM=ptr(out["M"]), oC=ptr(out["C"]),
                oJc=ptr(out["Jc"]), ou=ptr(out["u"]), ous=nu, oz=ptr(out["z"]), ozs=nz,
                of=ptr(out["qfrc"]))
    call = lambda **k: L.osc_batch_forward_dynamics_backward(
        *[dict(base, **k)[a] for a in order], stream())
    off = lambda x: ctypes.c_void_p(x.data_ptr() + 4)
    bad = [dict(model=None), dict(n=-1), dict(M=None), dict(qacc=None), dict(g=None),
           dict(z=None),                               # J, grad_Jc, grad_z still given
           dict(z=None, oJc=None, oz=None),            # J still given
           dict(z=None, J=None, oz=None), dict(z=None, J=None, oJc=None),
           dict(J=None),                               # grad_z needs J
           dict(zs=nz - 1), dict(gs=nv - 1), dict(ous=nu - 1), dict(ozs=nz - 1),
           dict(oM=None, oC=None, oJc=None, ou=None, oz=None, of=None)]
    bad += [dict(**{a: off(x)}) for a, x in
            (("M", t["M"]), ("J", t["J"]), ("z", t["z"]), ("qacc", t["qacc"]), ("g", t["g"]),
             ("oM", out["M"]), ("oC", out["C"]), ("oJc", out["Jc"]), ("ou", out["u"]),
             ("oz", out["z"]), ("of", out["qfrc"]))]
    for k in bad:
        assert call(**k) == 1, k
    from osc_amd.solver import OSCBatchSolver
    from test_gpu_wheels import NOSLIP_YAML
    sw = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)       # same nv / ns as walter_sr
    assert sw.wheels and call(model=sw._h) == 1
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.isnan(v).all(), k
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in out.values())
    assert call() == 0 and call(z=None, J=None, oJc=None, oz=None) == 0
    torch.cuda.synchronize()
    f = full(WALTER)
    for k, v in out.items():
        assert bitwise(v.cpu().numpy(), f[k][:n]), k
    # the Python wrapper refuses the same before the library does
    with pytest.raises(ValueError):
        kb.forward_dynamics_backward(s, t["M"], t["J"], t["z"], t["qacc"], t["g"])
    with pytest.raises(ValueError):
        kb.forward_dynamics_backward(s, t["M"], t["J"], None, t["qacc"], t["g"], grad_C=out["C"])
    with pytest.raises(ValueError):
        kb.forward_dynamics_backward(s, t["M"], None, t["z"], t["qacc"], t["g"], grad_z=out["z"])


# ---- 6. autograd --------------------------------------------------------------------------------------------

def ad_inputs(robot, n):
    c = pbr.bw_case(robot)
    return {k: dev(c[k][:n]).requires_grad_(True) for k in ("M", "C", "J", "u", "z", "qfrc")}


@pytest.mark.parametrize("robot", ROBOTS)
def test_gradcheck(gpu, robot):
    """torch.autograd.gradcheck of forward_dynamics_differentiable at 2 envs, all six inputs.  M
    enters as (A + A') / 2: the kernel's factorisation takes M as symmetric, so only symmetric
    perturbations are the function's, and grad_M = -w qacc' is its gradient for those.
    Tolerances, with eps = 1e-6: the central difference's rounding is at most |qacc| cond(M)
    2.2e-16 / eps ~ 1e3 x 1.4e3 x 2.2e-10 = 3e-4, so atol = 1e-3; its truncation is relative,
    (eps / min M_ii)^2 ~ (1e-6 / 1e-3)^2 at the very worst, so rtol = 1e-5 with margin (the
    function is linear in everything but M).  The gradients' entries reach 1e5."""
    from osc_amd.autograd import forward_dynamics_differentiable
    tree, kb, km, s, mdl = pair(robot)
    i = ad_inputs(robot, 2)
    tol = dict(eps=1e-6, atol=1e-3, rtol=1e-5, nondet_tol=0.0)
    f = lambda A, C, J, u, z, q: forward_dynamics_differentiable(
        s, kb, 0.5 * (A + A.transpose(1, 2)), C, J, u, z, q)
    assert torch.autograd.gradcheck(f, tuple(i.values()), **tol)
    g = lambda A, C, u, q: forward_dynamics_differentiable(
        s, kb, 0.5 * (A + A.transpose(1, 2)), C, None, u, None, q)
    assert torch.autograd.gradcheck(g, (i["M"], i["C"], i["u"], i["qfrc"]), **tol)


def test_autograd_fills_only_what_is_asked_for(gpu):
    """The forward is forward_dynamics_into, bitwise; the backward's gradients are the primitive's
    (J's zero off the contact rows); an input without requires_grad gets none; a bad env has a NaN
    qacc row and zero gradients."""
    from osc_amd.autograd import forward_dynamics_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    n, nv = 5, mdl.nv
    c = pbr.bw_case(GO2)
    i = ad_inputs(GO2, n)
    qacc = forward_dynamics_differentiable(s, kb, *i.values())
    plain = kb.forward_dynamics_into(s, nan(n, nv), *(v.detach() for v in i.values()))
    assert torch.equal(qacc.detach(), plain)
    g = dev(c["g"][:n])
    qacc.backward(g)
    ref = kb.forward_dynamics_backward(
        s, i["M"].detach(), i["J"].detach(), i["z"].detach(), plain, g,
        **{"grad_" + k: nan(*shapes(mdl, n)[k]) for k in OUT})
    for k in ("M", "C", "u", "z", "qfrc"):
        assert torch.equal(i[k].grad, ref[k]), k
    rows = pbr.contact_rows(mdl)
    assert torch.equal(i["J"].grad[:, rows], ref["Jc"])
    assert not i["J"].grad[:, :rows.start].any() and not i["J"].grad[:, rows.stop:].any()
    # only qfrc asks: the others stay None
    j = {k: dev(c[k][:n]) for k in ("M", "C", "J", "u", "z", "qfrc")}
    j["qfrc"].requires_grad_(True)
    j["M"][2, 4, 4] *= -1.0                                   # env 2: not positive definite
    q2 = forward_dynamics_differentiable(s, kb, *j.values())
    assert torch.isnan(q2[2]).all() and torch.isfinite(q2[[0, 1, 3, 4]]).all()
    q2.backward(g)
    assert all(j[k].grad is None for k in ("M", "C", "J", "u", "z"))
    assert not j["qfrc"].grad[2].any()
    keep = [0, 1, 3, 4]
    assert torch.equal(j["qfrc"].grad[keep], ref["qfrc"][keep])


# ---- the rollout's backward through a plant: shared cases ----------------------------------------------

K = tb.K
DT = tb.DT
GAINS = tb.GAINS
CKPT_BAR = tb.CKPT_BAR          # 3e-10: the bar of the existing test of the same construction
NORM_TOL = 1e-5                 # the project's contract for a gradient
ROWS = slice(0, 5)
WHAT = ("kin", "held", "seq", "all")
FIELDS = KinEnvParams.FIELDS


@functools.lru_cache(maxsize=None)
def pcase(robot, nenv=5):
    """tb.case(robot)'s first envs with a plant on top: drawn plant parameters (seed 41), a held
    applied force, a per-tick one with a 30 N push along x at tick 1, a cotangent on qacc_hist."""
    tree, kb, km, s, mdl = pair(robot)
    c = tb.case(robot)
    rng = np.random.default_rng(43)
    p = dict(plant_kp=ker.draw(tree, nenv, 41), qfrc=rng.uniform(-3, 3, (nenv, km.nv)),
             qfrc_seq=rng.uniform(-3, 3, (K, nenv, km.nv)),
             cot_qacc=rng.standard_normal((K, nenv, km.nv)))
    p["qfrc_seq"][1, :, 0] += 30.0
    return dict(c, **p)


def plant_of(c, what, rows=ROWS, nticks=K, grad=False):
    """The Plant of one case: its parameters alone, a held force, a per-tick one, all three."""
    kp = f = None
    if what in ("kin", "all"):
        kp = KinEnvParams(**{k: dev(c["plant_kp"][k][rows]).requires_grad_(grad) for k in FIELDS})
    if what == "held":
        f = dev(c["qfrc"][rows]).requires_grad_(grad)
    elif what in ("seq", "all"):
        f = dev(c["qfrc_seq"][:nticks, rows]).requires_grad_(grad)
    return Plant(kin_params=kp, qfrc_applied=f)


def plant_want(what, mode):
    w = ("qpos0", "qvel0", "kin.mass_scale") + (("T",) if mode == "held" else ())
    if what != "kin":
        w += ("plant.qfrc_applied",)
    if what in ("kin", "all"):
        w += tuple("plant.kin." + k for k in FIELDS)
    return w


def held_kw(c, mode, rows):
    return dict(T=dev(c["T"][rows])) if mode == "held" else \
        dict(pd=(dev(c["pos_ref"][rows]), c["quat_ref"].copy(), GAINS))


def cots(c, rows, nticks, scale=1.0):
    return dict(grad_qpos_hist=dev(scale * c["cot"]["qpos"][:nticks + 1, rows]),
                grad_qvel_hist=dev(scale * c["cot"]["qvel"][:nticks + 1, rows]),
                grad_tau_hist=dev(scale * c["cot"]["tau"][:nticks, rows]),
                grad_qacc_hist=dev(scale * c["cot_qacc"][:nticks, rows]))


def prun(robot, mode, what, rows=ROWS, nticks=K, want=None, scale=1.0, plant=None, **extra):
    """The forward rollout against plant_of(what) (cold solves, the controller on its own
    mass_scale) and rollout_plant_backward; name -> numpy, the RolloutResult under "res"."""
    tree, kb, km, s, mdl = pair(robot)
    c = pcase(robot)
    plant = plant_of(c, what, rows, nticks) if plant is None else plant
    kw = dict(held_kw(c, mode, rows), kin_params=KinEnvParams(mass_scale=dev(c["ms"][rows])))
    kw.update(extra)
    mask = dev(c["mask"][rows])
    res = kb.rollout(s, dev(c["qpos"][rows]), dev(c["qvel"][rows]), mask, nticks, DT, warm=False,
                     history=True, plant=plant, **kw)
    g = kb.rollout_plant_backward(s, res, mask, DT, want=want or plant_want(what, mode),
                                  **cots(c, rows, nticks, scale), **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in g.items()}
    out["res"] = res
    return out


# ---- 7. no plant ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [False, True])
@pytest.mark.parametrize("mode", ["held", "pd"])
def test_a_result_without_a_plant_is_bitwise_rollout_backward(gpu, mode, sched):
    """rollout_plant_backward of a rollout without a plant passes a NULL plant: the launches of
    osc_batch_rollout_backward(_sched), K = 3, 1, 0, held and PD, plain and scheduled."""
    tree, kb, km, s, mdl = pair(GO2)
    c = pcase(GO2)
    mask = dev(c["mask"][ROWS])
    for nticks in (K, 1, 0):
        kw = dict(held_kw(c, mode, ROWS), kin_params=KinEnvParams(mass_scale=dev(c["ms"][ROWS])))
        want = ("qpos0", "qvel0", "kin.mass_scale") + (("T",) if mode == "held" else ())
        if sched:
            rng = np.random.default_rng(3)
            kw["schedule"] = RolloutSchedule(T=dev(0.1 * rng.standard_normal(
                (nticks, 5, mdl.ns, 6))))
            want += ("T_seq",)
        res = kb.rollout(s, dev(c["qpos"][ROWS]), dev(c["qvel"][ROWS]), mask, nticks, DT,
                         warm=False, history=True, **kw)
        cot = cots(c, ROWS, nticks)
        cot.pop("grad_qacc_hist")
        a = kb.rollout_backward(s, res, mask, DT, want=want, **cot, **kw)
        b = kb.rollout_plant_backward(s, res, mask, DT, want=want, **cot, **kw)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(a[k], b[k]), (nticks, k)


# ---- 8. the hand composition --------------------------------------------------------------------------------

def composition(robot, mode, what, res, plant, env_params=None, sched_T=None):
    """Tick by tick on the forward's checkpoints, t = K-1 .. 0: one solve_differentiable_qpos node
    with the CONTROLLER's parameters, kinematics_differentiable with the PLANT's,
    forward_dynamics_differentiable on the solve's u and z, the step and the producer in torch
    ops, and autograd of g_q . qpos' + g_v . qvel' + cot_tau[t] . tau + cot_qacc[t] . qacc: the
    public entries this feature chains, the new one and the two kinematics backwards among them."""
    from osc_amd.autograd import (forward_dynamics_differentiable, kinematics_differentiable,
                                  solve_differentiable_qpos)
    tree, kb, km, s, mdl = pair(robot)
    c = pcase(robot)
    nv, nu = km.nv, mdl.nu
    cot = {k: dev(a[:, ROWS]) for k, a in c["cot"].items()}
    cq = dev(c["cot_qacc"][:, ROWS])
    mask = dev(c["mask"][ROWS])
    pos_ref, quat_ref = dev(c["pos_ref"][ROWS]), dev(c["quat_ref"])
    gq, gv = cot["qpos"][K], cot["qvel"][K]
    sums, slabs = {}, {}
    for t in range(K - 1, -1, -1):
        q = res.qpos_hist[t].clone().requires_grad_(True)
        v = res.qvel_hist[t].clone().requires_grad_(True)
        ms = dev(c["ms"][ROWS]).requires_grad_(True)
        T = dev(c["T"][ROWS]).requires_grad_(True)
        Tt = T if mode == "held" else tb.pd_t(mdl.ns, q, v, pos_ref, quat_ref, GAINS)
        if sched_T is not None:
            Tt = Tt + sched_T[t]
        tau, x, status = solve_differentiable_qpos(s, kb, q, v, Tt, mask, env_params=env_params,
                                                   kin_params=KinEnvParams(mass_scale=ms))
        leaves = {"qpos0": q, "qvel0": v, "kin.mass_scale": ms}
        if mode == "held":
            leaves["T"] = T
        if plant.kin_params is not None:
            pk = {k: getattr(plant.kin_params, k).detach().clone().requires_grad_(True)
                  for k in FIELDS}
            leaves.update({"plant.kin." + k: a for k, a in pk.items()})
            pkp = KinEnvParams(**pk)
        else:
            pkp = KinEnvParams(mass_scale=ms)
        Mp, Cp, J, _ = kinematics_differentiable(kb, q, v, kin_params=pkp)
        f = plant.qfrc_applied
        if f is not None:
            f = (f[t] if f.dim() == 3 else f).detach().clone().requires_grad_(True)
            leaves["plant.qfrc_applied"] = f
        qacc = forward_dynamics_differentiable(s, kb, Mp, Cp, J, x[:, nv:nv + nu],
                                               x[:, nv + nu:], f)
        qn, vn = tb.step_b(km, q, v, qacc, DT)
        loss = (qn * gq).sum() + (vn * gv).sum() + (tau * cot["tau"][t]).sum() + \
            (qacc * cq[t]).sum()
        g = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
        gq, gv = g.pop("qpos0") + cot["qpos"][t], g.pop("qvel0") + cot["qvel"][t]
        for k, a in g.items():
            if k == "plant.qfrc_applied" and plant.qfrc_applied.dim() == 3:
                slabs[t] = a
            else:
                sums[k] = a if k not in sums else sums[k] + a
    if slabs:
        sums["plant.qfrc_applied"] = torch.stack([slabs[t] for t in range(K)])
    out = dict(qpos0=gq, qvel0=gv, **sums)
    return {k: a.cpu().numpy() for k, a in out.items()}


def compare(got, ref, want, bar, label):
    worst = {}
    for k in want:
        r = ref[k].reshape(5, -1) if ref[k].shape[0] == 5 else np.moveaxis(ref[k], 1, 0).reshape(5, -1)
        g = got[k].reshape(5, -1) if got[k].shape[0] == 5 else np.moveaxis(got[k], 1, 0).reshape(5, -1)
        worst[k] = float(br.env_errors(g, r).max())
    print(f"\n{label}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in want:
        assert np.isfinite(got[k]).all() and np.abs(ref[k]).max() > 0, k
        assert worst[k] <= bar, (k, worst[k])
    return worst


@pytest.mark.parametrize("what", WHAT)
@pytest.mark.parametrize("mode", ["held", "pd"])
def test_vs_the_hand_composition(gpu, mode, what):
    """Go2, 5 envs, K = 3, a loss on every slab of the four histories; plant parameters alone, a
    held force, a per-tick force, all three; held and PD targets: every gradient within CKPT_BAR
    (backward_ref.env_errors) of the composition of the public entries on the same checkpoints."""
    want = plant_want(what, mode)
    got = prun(GO2, mode, what, want=want)
    assert (got["res"].status_hist == 0).all()
    ref = composition(GO2, mode, what, got["res"], plant_of(pcase(GO2), what))
    compare(got, ref, want, CKPT_BAR, f"plant composition go2 {mode} {what}")


def test_walter_and_everything_vs_the_hand_composition(gpu):
    """WaLTER, all three plant fields; and Go2 once more under the controller's kin_params,
    env_params and a schedule (T_seq added to the held targets).  Every (env, tick) of both is
    OK (asserted), so no gradient is the zero a failed solve would give; WaLTER's parameter, target
    and force gradients come out bitwise the composition's (error 0): the same kernels on the same
    bits, summed in the same order."""
    want = plant_want("all", "held")
    got = prun(WALTER, "held", "all", want=want)
    assert (got["res"].status_hist == 0).all() and (got["res"].bad_ticks == 0).all()
    ref = composition(WALTER, "held", "all", got["res"], plant_of(pcase(WALTER), "all"))
    compare(got, ref, want, CKPT_BAR, "plant composition walter held all")
    tree, kb, km, s, mdl = pair(GO2)
    rng = np.random.default_rng(5)
    ep = EnvParams(mu=dev(rng.uniform(0.4, 1.0, 5)), fz_ub=dev(rng.uniform(60.0, 90.0, 5)))
    sT = dev(0.1 * rng.standard_normal((K, 5, mdl.ns, 6)))
    got = prun(GO2, "held", "all", want=want, env_params=ep, schedule=RolloutSchedule(T=sT))
    assert (got["res"].status_hist == 0).all()
    ref = composition(GO2, "held", "all", got["res"], plant_of(pcase(GO2), "all"), env_params=ep,
                      sched_T=sT)
    compare(got, ref, want, CKPT_BAR, "plant composition go2 held all, env_params + schedule")


# ---- 9. the CPU chain -----------------------------------------------------------------------------------------

def test_vs_the_cpu_chain(gpu):
    """plant_backward_ref.chain_case -- Go2, 5 envs, K = 3, HELD_MASK, the controller on its own
    mass_scale, the plant's three fields drawn, a held force with a 30 N push at tick 1, cotangents
    on every slab of the four histories; the reference asserts a clean, certified optimum at every
    env and tick and is itself pinned to finite differences on the CPU: qpos0, qvel0, T, the
    controller's mass_scale, the per-tick force and the plant's mass_scale, com_offset and
    armature_scale by backward_ref.env_errors within the 1e-5 contract.
    Measured worst on an MI355X: qpos0 1.92e-9, qvel0 1.28e-10, T 3.96e-11, kin.mass_scale
    2.56e-10, plant.qfrc_applied 1.00e-11, plant.kin.mass_scale 2.08e-11, com_offset 1.16e-11,
    armature_scale 7.15e-11."""
    tree, kb, km, s, mdl = pair(GO2)
    c = pbr.chain_case()
    ref = pbr.chain_grads(c)
    mask, T = dev(c["mask"]), dev(c["T"])
    kp = KinEnvParams(mass_scale=dev(c["ms"]))
    plant = Plant(kin_params=KinEnvParams(**{k: dev(c["plant_" + k]) for k in FIELDS}),
                  qfrc_applied=dev(c["qfrc_seq"]))
    res = kb.rollout(s, dev(c["qpos"]), dev(c["qvel"]), mask, pbr.CHAIN_K, DT, T=T, warm=False,
                     history=True, kin_params=kp, plant=plant)
    want = ("qpos0", "qvel0", "T", "kin.mass_scale", "plant.qfrc_applied") + \
        tuple("plant.kin." + k for k in FIELDS)
    g = kb.rollout_plant_backward(s, res, mask, DT, T=T, kin_params=kp, want=want,
                                  **{"grad_" + k + "_hist": dev(c["cot_" + k])
                                     for k in ("qpos", "qvel", "tau", "qacc")})
    torch.cuda.synchronize()
    assert (res.status_hist == 0).all() and (res.bad_ticks == 0).all()
    for k, h in (("qpos", res.qpos_hist), ("qacc", res.qacc_hist)):
        r = np.stack([o[1][k] for o in c["out"]], axis=1)
        assert np.abs(h.cpu().numpy() - r).max() <= 1e-9 * (1 + np.abs(r).max()), k
    got = {k: v.cpu().numpy() for k, v in g.items()}
    compare(got, ref, want, NORM_TOL, "plant backward vs the CPU chain")


# ---- 9b. central differences of GPU forward rollouts -------------------------------------------------------

def test_vs_central_differences_of_the_forward(gpu):
    """Go2, 5 envs, K = 3, all three plant fields: <gradient, direction> against the Richardson
    central difference of the loss sum(cotangent . history) over two pairs of GPU forward rollouts
    (cold solves) along drawn directions in the per-tick force, the plant's mass_scale and
    com_offset and in qvel0, per env.  Bar: the project's 1e-5, relative to max(|d|, 1).  The cold
    solves end within ~1e-11 of their optimum, so the difference quotient carries ~1e-11 / h."""
    tree, kb, km, s, mdl = pair(GO2)
    c = pcase(GO2)
    want = plant_want("all", "held")
    got = prun(GO2, "held", "all", want=want)
    mask = dev(c["mask"][ROWS])
    kw = dict(held_kw(c, "held", ROWS), kin_params=KinEnvParams(mass_scale=dev(c["ms"][ROWS])))
    cot = cots(c, ROWS, K)
    base = dict(qvel=c["qvel"][ROWS], qfrc=c["qfrc_seq"][:, ROWS],
                mass_scale=c["plant_kp"]["mass_scale"][ROWS],
                com_offset=c["plant_kp"]["com_offset"][ROWS])

    def loss(**over):
        a = dict(base, **over)
        kp = KinEnvParams(mass_scale=dev(a["mass_scale"]), com_offset=dev(a["com_offset"]),
                          armature_scale=dev(c["plant_kp"]["armature_scale"][ROWS]))
        r = kb.rollout(s, dev(c["qpos"][ROWS]), dev(a["qvel"]), mask, K, DT, warm=False,
                       history=True, plant=Plant(kin_params=kp, qfrc_applied=dev(a["qfrc"])), **kw)
        per = lambda h, g: (h * g).reshape(h.shape[0], 5, -1).sum(dim=(0, 2))
        return (per(r.qpos_hist, cot["grad_qpos_hist"]) + per(r.qvel_hist, cot["grad_qvel_hist"]) +
                per(r.tau_hist, cot["grad_tau_hist"]) +
                per(r.qacc_hist, cot["grad_qacc_hist"])).cpu().numpy()

    rng = np.random.default_rng(9)
    names = dict(qvel="qvel0", qfrc="plant.qfrc_applied", mass_scale="plant.kin.mass_scale",
                 com_offset="plant.kin.com_offset")
    for k, h in (("qfrc", 0.1), ("qvel", 1e-3), ("mass_scale", 1e-3), ("com_offset", 1e-3)):
        dx = rng.standard_normal(base[k].shape)
        d = lambda s_: (loss(**{k: base[k] + s_ * dx}) - loss(**{k: base[k] - s_ * dx})) / (2 * s_)
        num = (4 * d(h / 2) - d(h)) / 3
        g = got[names[k]]
        ana = (g * dx).sum(axis=(0, 2) if k == "qfrc" else tuple(range(1, g.ndim)))
        rel = np.abs(num - ana) / np.maximum(np.abs(num), 1.0)
        print(f"\ncentral differences, {k}: worst {rel.max():.2e} (|d| <= {np.abs(num).max():.2e})")
        assert rel.max() <= NORM_TOL, (k, num, ana)


# ---- 10. bitwise properties ---------------------------------------------------------------------------------

def test_the_held_force_gradient_is_the_tick_ordered_sum(gpu):
    """grad_qfrc_applied of a held force equals, bitwise, the sum in the order K-1 .. 0 (from zero)
    of the gradients of K one-tick calls, each seeded with the state adjoints of the call before
    it; the plant's parameter gradients likewise; the state adjoints of the last are grad_qpos0 /
    grad_qvel0."""
    tree, kb, km, s, mdl = pair(GO2)
    c = pcase(GO2)
    plant = Plant(kin_params=plant_of(c, "kin").kin_params, qfrc_applied=dev(c["qfrc"][ROWS]))
    want = ("qpos0", "qvel0", "plant.qfrc_applied") + tuple("plant.kin." + k for k in FIELDS)
    whole = prun(GO2, "held", None, want=want, plant=plant)
    res = whole["res"]
    ct = cots(c, ROWS, K)
    mask, T = dev(c["mask"][ROWS]), dev(c["T"][ROWS])
    kp = KinEnvParams(mass_scale=dev(c["ms"][ROWS]))
    gq, gv = ct["grad_qpos_hist"][K], ct["grad_qvel_hist"][K]
    sums = {k: torch.zeros_like(dev(whole[k])) for k in want[2:]}
    for t in range(K - 1, -1, -1):
        one = RolloutResult(None, None, None, None, qpos_hist=res.qpos_hist[t:t + 2].contiguous(),
                            qvel_hist=res.qvel_hist[t:t + 2].contiguous(),
                            tau_hist=res.tau_hist[t:t + 1].contiguous(),
                            status_hist=res.status_hist[t:t + 1].contiguous(), plant=plant)
        g = kb.rollout_plant_backward(
            s, one, mask, DT, T=T, kin_params=kp, want=want,
            grad_qpos_hist=torch.stack([ct["grad_qpos_hist"][t], gq]),
            grad_qvel_hist=torch.stack([ct["grad_qvel_hist"][t], gv]),
            grad_tau_hist=ct["grad_tau_hist"][t:t + 1].contiguous(),
            grad_qacc_hist=ct["grad_qacc_hist"][t:t + 1].contiguous())
        gq, gv = g["qpos0"], g["qvel0"]
        for k in sums:
            sums[k] = sums[k] + g[k]
    torch.cuda.synchronize()
    assert bitwise(gq.cpu().numpy(), whole["qpos0"]) and bitwise(gv.cpu().numpy(), whole["qvel0"])
    for k in sums:
        assert bitwise(sums[k].cpu().numpy(), whole[k]), k


def test_batch_independence_scaling_and_null_outputs(gpu):
    """An env alone is bitwise what it is inside 5, and a repeated call gives the same bits; 2 x
    the cotangents give 2 x the gradients, bitwise; each output alone, and all but each, is
    bitwise the call with all of them."""
    want = plant_want("all", "held")
    full = prun(GO2, "held", "all", want=want)
    again = prun(GO2, "held", "all", want=want)
    twice = prun(GO2, "held", "all", want=want, scale=2.0)
    env = lambda a, e: a[:, e:e + 1] if a.ndim == 3 and a.shape[0] == K and a.shape[1] == 5 \
        else a[e:e + 1]
    for k in want:
        assert bitwise(again[k], full[k]), k
        assert bitwise(twice[k], 2.0 * full[k]), k
    for e in (0, 3):
        one = prun(GO2, "held", "all", rows=slice(e, e + 1), want=want)
        for k in want:
            assert bitwise(one[k], env(full[k], e)), (e, k)
    for k in want:
        assert bitwise(prun(GO2, "held", "all", want=(k,))[k], full[k]), k
        rest = prun(GO2, "held", "all", want=tuple(o for o in want if o != k))
        for o in want:
            assert o == k or bitwise(rest[o], full[o]), (k, o)


# ---- 11. frozen envs, memory, refusals, autograd, behaviour -----------------------------------------------

def test_invalid_plant_parameters_pass_the_cotangents_through(gpu):
    """mass_scale <= 0 on one body of env 2 of the PLANT: the env never moved, its grad_qpos0 /
    grad_qvel0 are the sums of its slabs' cotangents in the order K .. 0, every other gradient of
    it is zero, nothing is NaN, and the other envs are bitwise the run without it."""
    c = pcase(GO2)
    want = plant_want("all", "held")
    good = prun(GO2, "held", "all", want=want)
    plant = plant_of(c, "all")
    plant.kin_params.mass_scale[2, 3] = -1.0
    got = prun(GO2, "held", "all", want=want, plant=plant)
    assert got["res"].bad_ticks.tolist() == [0, 0, K, 0, 0]
    for k, name in (("qpos0", "qpos"), ("qvel0", "qvel")):
        acc = c["cot"][name][K, 2]
        for t in range(K - 1, -1, -1):
            acc = acc + c["cot"][name][t, 2]
        assert bitwise(got[k][2], acc), k
    o = [0, 1, 3, 4]
    for k in want:
        assert np.isfinite(got[k]).all(), k
        per_tick = got[k].ndim == 3 and got[k].shape[:2] == (K, 5)
        mine = got[k][:, 2] if per_tick else got[k][2]
        if k not in ("qpos0", "qvel0"):
            assert not mine.any(), k
        a, b = (got[k][:, o], good[k][:, o]) if per_tick else (got[k][o], good[k][o])
        assert bitwise(a, b), k


def raw_plant_backward(robot, res, c, pl, ws, nbytes, out, cot):
    tree, kb, km, s, mdl = pair(robot)
    a = _lib.OscRolloutBackwardArgs()
    a.nticks, a.dt, a.target_mode = K, DT, _lib.ROLLOUT_TARGETS_HELD
    T, mask = dev(c["T"][ROWS]), dev(c["mask"][ROWS])
    a.T, a.contact_mask = T.data_ptr(), mask.data_ptr()
    a.qpos_hist, a.qvel_hist = res.qpos_hist.data_ptr(), res.qvel_hist.data_ptr()
    a.status_hist = res.status_hist.data_ptr()
    a.grad_qpos_hist = cot["grad_qpos_hist"].data_ptr()
    a.grad_qvel_hist = cot["grad_qvel_hist"].data_ptr()
    a.grad_tau_hist = cot["grad_tau_hist"].data_ptr()
    a.grad_qpos0 = out.data_ptr() if out is not None else None
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    rc = _lib.lib().osc_batch_rollout_plant_backward(s._h, kb._h, 5, ctypes.byref(a), None, None,
                                                     None, None, ctypes.byref(pl), stream())
    torch.cuda.synchronize()
    return rc


def test_the_c_entry_stays_inside_its_arrays_and_refuses(gpu):
    """osc_batch_rollout_plant_backward through the C entry with the plant's parameters, its
    gradients, the per-tick force, its gradient, grad_qacc_hist and the workspace (at exactly
    osc_rollout_plant_backward_workspace_bytes) between guard bands: the bands intact, the results
    bitwise the wrapper's.  Then the refusals, each with the outputs untouched."""
    tree, kb, km, s, mdl = pair(GO2)
    c = pcase(GO2)
    ref = prun(GO2, "held", "all", kin_params=None,
               want=("qpos0", "plant.qfrc_applied") + tuple("plant.kin." + k for k in FIELDS))
    res = ref["res"]
    cot = cots(c, ROWS, K)
    nbytes = kb.rollout_plant_backward_workspace_bytes(s, 5)
    assert nbytes > kb.rollout_backward_workspace_bytes(s, 5)
    i = {k: guarded_like(dev(c["plant_kp"][k][ROWS]), 0xFF) for k in FIELDS}
    i["seq"] = guarded_like(dev(np.ascontiguousarray(c["qfrc_seq"][:, ROWS])), 0xFF)
    i["gah"] = guarded_like(cot["grad_qacc_hist"], 0xFF)
    shp = dict(mass_scale=(5, kb.nbody), com_offset=(5, kb.nbody, 3), armature_scale=(5, km.nv))
    o = {k: guarded(shp[k], torch.float64, gpu) for k in FIELDS}
    o["gseq"] = guarded((K, 5, km.nv), torch.float64, gpu)
    o["gq0"] = guarded((5, km.nq), torch.float64, gpu)
    ws = guarded((nbytes // 8,), torch.float64, gpu, env_bytes=nbytes // 5)
    ck = _lib.OscKinEnvParams(**{k: i[k].data_ptr() for k in FIELDS})
    cg = _lib.OscKinEnvGrads(**{k: o[k].data_ptr() for k in FIELDS})
    P = _lib.OscRolloutPlantBackward
    full = dict(kin_params=ctypes.pointer(ck), qfrc_applied_seq=i["seq"].data_ptr(),
                grad_qacc_hist=i["gah"].data_ptr(), grad_qfrc_applied_seq=o["gseq"].data_ptr(),
                kin_grads=ctypes.pointer(cg))
    assert raw_plant_backward(GO2, res, c, P(**full), ws, nbytes, o["gq0"], cot) == 0
    for k, t in dict(i, workspace=ws, **{"out " + k: v for k, v in o.items()}).items():
        assert_guards_intact(t, k)
    assert bitwise(o["gq0"].cpu().numpy(), ref["qpos0"])
    assert bitwise(o["gseq"].cpu().numpy(), ref["plant.qfrc_applied"])
    for k in FIELDS:
        assert bitwise(o[k].cpu().numpy(), ref["plant.kin." + k]), k
    # ---- refusals ----
    out, held = nan(5, km.nq), nan(5, km.nv)
    odd = lambda t: t.data_ptr() + 4
    cko = _lib.OscKinEnvParams(mass_scale=odd(i["mass_scale"]))
    cgo = _lib.OscKinEnvGrads(mass_scale=odd(o["mass_scale"]))
    bad = [("held gradient of a per-tick force", dict(full, grad_qfrc_applied=held.data_ptr(),
                                                       grad_qfrc_applied_seq=None), nbytes),
           ("per-tick gradient of a held force", dict(full, qfrc_applied_seq=None,
                                                      qfrc_applied=i["seq"].data_ptr()), nbytes),
           ("kin_grads without kin_params", dict(full, kin_params=None), nbytes),
           ("odd qfrc_seq", dict(full, qfrc_applied_seq=odd(i["seq"])), nbytes),
           ("odd grad_qacc_hist", dict(full, grad_qacc_hist=odd(i["gah"])), nbytes),
           ("odd grad_qfrc_applied_seq", dict(full, grad_qfrc_applied_seq=odd(o["gseq"])), nbytes),
           ("odd plant mass_scale", dict(full, kin_params=ctypes.pointer(cko), kin_grads=None),
            nbytes),
           ("odd plant grad mass_scale", dict(full, kin_grads=ctypes.pointer(cgo)), nbytes),
           ("short workspace", full, nbytes - 1),
           ("the plain backward's workspace", full, kb.rollout_backward_workspace_bytes(s, 5))]
    for label, fields, nb in bad:
        assert raw_plant_backward(GO2, res, c, P(**fields), ws, nb, out, cot) == 1, label
        assert torch.isnan(out).all() and torch.isnan(held).all(), label
    # every output NULL, the plant's among them
    assert raw_plant_backward(GO2, res, c, P(qfrc_applied_seq=i["seq"].data_ptr()), ws, nbytes,
                              None, cot) == 1
    # a held gradient with no held force is the gradient at zero: accepted
    assert raw_plant_backward(GO2, res, c, P(grad_qfrc_applied=held.data_ptr()), ws, nbytes, None,
                              cot) == 0
    assert torch.isfinite(held).all()


def test_autograd_through_the_plant(gpu):
    """rollout_plant_differentiable: the forward's histories are rollout(..., plant=)'s, bitwise;
    the gradients are rollout_plant_backward's, bitwise; only what requires a gradient gets one;
    rollout_differentiable and rollout_backward still refuse a plant."""
    from osc_amd.autograd import rollout_differentiable, rollout_plant_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    c = pcase(GO2)
    ref = prun(GO2, "held", "all", kin_params=None,
               want=("qvel0", "plant.qfrc_applied", "plant.kin.mass_scale"))
    plant = plant_of(c, "all")
    plant.qfrc_applied.requires_grad_(True)
    plant.kin_params.mass_scale.requires_grad_(True)
    qv = dev(c["qvel"][ROWS]).requires_grad_(True)
    qp, mask, T = dev(c["qpos"][ROWS]), dev(c["mask"][ROWS]), dev(c["T"][ROWS])
    hq, hv, ht, hs, ha = rollout_plant_differentiable(s, kb, qp, qv, mask, K, DT, T=T, warm=False,
                                                      plant=plant)
    res = ref["res"]
    assert torch.equal(hq, res.qpos_hist) and torch.equal(ha, res.qacc_hist)
    ct = cots(c, ROWS, K)
    loss = (hq * ct["grad_qpos_hist"]).sum() + (hv * ct["grad_qvel_hist"]).sum() + \
        (ht * ct["grad_tau_hist"]).sum() + (ha * ct["grad_qacc_hist"]).sum()
    loss.backward()
    assert bitwise(qv.grad.cpu().numpy(), ref["qvel0"])
    assert bitwise(plant.qfrc_applied.grad.cpu().numpy(), ref["plant.qfrc_applied"])
    assert bitwise(plant.kin_params.mass_scale.grad.cpu().numpy(), ref["plant.kin.mass_scale"])
    assert qp.grad is None and T.grad is None and plant.kin_params.com_offset.grad is None
    with pytest.raises(NotImplementedError, match="osc_plant.h"):
        rollout_differentiable(s, kb, qp, qv.detach(), mask, K, DT, T=T, plant=plant_of(c, "held"))
    with pytest.raises(NotImplementedError, match="osc_plant.h"):
        kb.rollout_backward(s, res, mask, DT, T=T, grad_qpos_hist=ct["grad_qpos_hist"])


def test_autograd_carries_the_schedule_the_references_and_the_gains(gpu):
    """PD targets with a feed-forward schedule.T, against a plant: the gradients of schedule.T, the
    held PD references, the gains (a tensor of 4) and the plant's force from
    rollout_plant_differentiable are, bitwise, rollout_plant_backward's by name -- what
    rollout_differentiable carries, through the plant."""
    from osc_amd.autograd import rollout_plant_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    c = pcase(GO2)
    rng = np.random.default_rng(6)
    mk = lambda a: dev(a).requires_grad_(True)
    sT = mk(0.1 * rng.standard_normal((K, 5, mdl.ns, 6)))
    pos_ref, quat_ref = mk(c["pos_ref"][ROWS]), mk(c["quat_ref"])
    gains = mk(np.array(GAINS))
    f = mk(c["qfrc"][ROWS])
    qp, qv, mask = dev(c["qpos"][ROWS]), dev(c["qvel"][ROWS]), dev(c["mask"][ROWS])
    hist = rollout_plant_differentiable(s, kb, qp, qv, mask, K, DT, pd=(pos_ref, quat_ref, gains),
                                        warm=False, schedule=RolloutSchedule(T=sT),
                                        plant=Plant(qfrc_applied=f))
    ct = cots(c, ROWS, K)
    cot = [ct["grad_qpos_hist"], ct["grad_qvel_hist"], ct["grad_tau_hist"], None,
           ct["grad_qacc_hist"]]
    sum((h * g).sum() for h, g in zip(hist, cot) if g is not None).backward()
    pd = (pos_ref.detach(), quat_ref.detach(), GAINS)
    sched = RolloutSchedule(T=sT.detach())
    res = kb.rollout(s, qp, qv, mask, K, DT, pd=pd, warm=False, history=True, schedule=sched,
                     plant=Plant(qfrc_applied=f.detach()))
    assert torch.equal(res.qpos_hist, hist[0]) and torch.equal(res.qacc_hist, hist[4])
    want = ("T_seq", "pos_ref", "quat_ref", "gains", "plant.qfrc_applied")
    ref = kb.rollout_plant_backward(s, res, mask, DT, pd=pd, schedule=sched, want=want, **ct)
    torch.cuda.synchronize()
    for k, t in zip(want, (sT, pos_ref, quat_ref, gains, f)):
        assert t.grad is not None and t.grad.abs().max() > 0, k
        assert torch.equal(t.grad, ref[k]), k
    assert qp.grad is None


def test_identifying_a_payload(gpu):
    """rollout_ref.go2_case, K = 20: the logged data come from a plant whose trunk is 1.5 x heavier;
    the loss is the squared base-height history error of a plant at 1.0 x.  Its gradient with
    respect to the trunk's mass_scale is negative (a heavier trunk sags towards the log) and matches
    the central difference of two GPU forward rollouts (h = 1e-3) within ten times the disagreement
    of the same comparison on the CPU chain (plant_backward_ref.behaviour_case: 1.15e-6, the
    difference's truncation), 1e-5 at most; it also equals the CPU chain's gradient to 1e-5."""
    from osc_amd.autograd import rollout_plant_differentiable
    tree, kb, km, s, mdl = pair(GO2)
    _, _, qpos, qvel, mask, pd = rollout_ref.go2_case()
    n, KB = 1, pbr.BEHAVIOUR_K
    cpu = pbr.behaviour_case()
    qp, qv, mk = dev(qpos[None]), dev(qvel[None]), dev(mask[None])

    def heights(scale, grad=False):
        ms = torch.ones((n, kb.nbody), dtype=torch.float64, device="cuda")
        ms[:, 0] = scale
        ms.requires_grad_(grad)
        plant = Plant(kin_params=KinEnvParams(mass_scale=ms))
        if grad:
            h = rollout_plant_differentiable(s, kb, qp, qv, mk, KB, DT, pd=pd, warm=False,
                                             plant=plant)[0]
        else:
            h = kb.rollout(s, qp, qv, mk, KB, DT, pd=pd, warm=False, history=True,
                           plant=plant).qpos_hist
        return h[:, :, 2], ms

    log, _ = heights(pr.TRUNK_SCALE)
    z, ms = heights(1.0, grad=True)
    loss = ((z - log) ** 2).sum()
    loss.backward()
    g = ms.grad[0, 0].item()
    L = lambda sc: float(((heights(sc)[0] - log) ** 2).sum())
    h = pbr.BEHAVIOUR_H
    num = (L(1.0 + h) - L(1.0 - h)) / (2 * h)
    bar = pbr.behaviour_bar()
    print(f"\npayload identification: dL/d trunk mass_scale {g:.6e}, central difference {num:.6e}"
          f" (disagreement {abs(g - num) / abs(num):.2e}, bar {bar:.2e}), CPU chain "
          f"{cpu['grad']:.6e} (CPU disagreement {cpu['disagreement']:.2e})")
    assert g < 0
    assert abs(g - num) <= bar * abs(num)
    assert abs(g - cpu["grad"]) <= NORM_TOL * abs(cpu["grad"])
