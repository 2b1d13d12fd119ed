"""GPU tests of the backward pass with per-env parameters (include/osc_backward_env.h,
osc_batch_solve_backward_env; csrc/osc_backward_env.hip; osc_amd.solver.EnvGrads,
osc_amd.autograd.solve_differentiable_env): the gradients of the seven per-env fields and the six
data outputs against the reference adjoint built from each env's own oracle model
(tests/backward_env_ref.py, pinned by the oracle's own differences in
tests/test_backward_env_ref.py), on tests/env_params_cases.py's 61-env batch (a partial last
wavefront; tumbling, fractional mask, one-sided torque boxes on every seventh env, fz_lb in
{0, 5}) of Go2 and WaLTER Sr.  Every env is compared.

Error per env and output: |g - g_ref|_inf / max(|g_ref|_inf, 1e-6 x the batch's largest
|g_ref|_inf) (backward_ref.env_errors).  The bar is the contract, NORM_TOL = 1e-5
(tests/test_gpu_parity.py), as tests/test_gpu_backward_data.py.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import backward_env_ref as be
import backward_ref as br
import env_params_cases as ec
from osc_amd import _lib
from test_gpu_parity import NORM_TOL

pytestmark = pytest.mark.gpu

GO2, WALTER = be.ROBOTS
FIELDS, OUTPUTS = be.FIELDS, be.OUTPUTS
ALL = FIELDS + OUTPUTS
NUMERICAL = _lib.SOLVE_NUMERICAL


@functools.lru_cache(maxsize=None)
def solver(robot):
    from osc_amd.solver import OSCBatchSolver
    return OSCBatchSolver(robot)


def block(p, rows=slice(None)):
    from osc_amd.solver import EnvParams
    return EnvParams(**{k: torch.as_tensor(np.ascontiguousarray(p[k][rows])).cuda() for k in FIELDS})


def forward(robot, p="drawn", rows=slice(None), d=None, warm=False):
    """(device inputs, SolveResult with x, y and the workspace, the EnvParams block or None) of the
    batch's rows; p: "drawn" (env_params_cases.params), None (no block) or a dict of arrays."""
    s = solver(robot)
    p = ec.params(robot) if isinstance(p, str) else p
    d = {k: v[rows] for k, v in (d or ec.inputs(robot)).items()}
    blk = None if p is None else block(p, rows)
    args = s.prepare(**d)
    out = s.alloc_outputs(args[0].shape[0], want_x=True, want_y=True)
    if warm:
        state = s.alloc_warm_state(args[0].shape[0])
        for _ in range(2):                  # the second tick starts from the first's solution
            s.solve_warm_into(out, state, *args, env_params=blk)
    else:
        s.solve_into(out, *args, env_params=blk)
    torch.cuda.synchronize()
    return args, out, blk


@functools.lru_cache(maxsize=None)
def solved(robot, p="drawn"):
    """The whole batch's forward solve, shared by the tests (left unchanged)."""
    return forward(robot, p)


def shapes(s, n):
    from osc_amd.solver import EnvParams
    d = s.dims
    sh = dict(M=(n, d["nv"], d["nv"]), C=(n, d["nv"]), J=(n, d["s"], d["nv"]), wrow=(n, d["s"]),
              T=(n, d["ns"], 6), b=(n, d["s"]))
    sh.update(EnvParams().shapes(n, d))
    return sh


def backward(robot, fwd, gx, want=ALL, blk="forward"):
    """name -> gradient as numpy for the outputs in `want` (the others are passed as NULL), from
    gx (numpy, one row per env of the forward solve).  Outputs start as NaN.  blk: the EnvParams
    of the backward call (default: the forward call's)."""
    from osc_amd.solver import EnvGrads
    s = solver(robot)
    (M, C, J, b, T, mask), out, fblk = fwd
    n = out.tau.shape[0]
    g = torch.from_numpy(np.ascontiguousarray(gx)).to(s.device)
    sh = shapes(s, n)
    o = {k: torch.full(sh[k], float("nan"), dtype=torch.float64, device=s.device) for k in want}
    eg = EnvGrads(**{k: o[k] for k in FIELDS if k in o})
    s.backward_env_into(out, M, J, b, T, mask, g, env_params=fblk if isinstance(blk, str) else blk,
                        grad_M=o.get("M"), grad_C=o.get("C"), grad_J=o.get("J"),
                        grad_wrow=o.get("wrow"), grad_T=o.get("T"), grad_b=o.get("b"),
                        env_grads=eg)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def backward_data(robot, fwd, gx):
    s = solver(robot)
    (M, C, J, b, T, mask), out, _ = fwd
    g = torch.from_numpy(np.ascontiguousarray(gx)).to(s.device)
    sh = shapes(s, out.tau.shape[0])
    o = {k: torch.full(sh[k], float("nan"), dtype=torch.float64, device=s.device) for k in OUTPUTS}
    s.backward_data_into(out, M, J, b, T, mask, g, grad_M=o["M"], grad_C=o["C"], grad_J=o["J"],
                         grad_wrow=o["wrow"], grad_T=o["T"], grad_b=o["b"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def bitwise(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_against_reference(gpu, robot):
    """Every env of the batch, gx random over all of x and gx on tau alone: status OK, and all
    seven parameter gradients and the six data outputs within the contract of the reference
    adjoint.

    Worst errors measured on an MI355X, gx over all of x / on tau alone:
      Go2     mu 3.5e-13 / 5.9e-13  u_lb 4.4e-14 / 3.2e-14  u_ub 4.1e-13 / 2.6e-14  fz_lb 5.5e-13 / 1.6e-14
              fz_ub 1.4e-12 / 2.1e-13  w_pos 7.2e-14 / 1.9e-13  w_rot 9.9e-14 / 7.7e-14
              M 7.3e-14 / 5.7e-14  C 4.2e-14 / 6.8e-14  J 7.5e-14 / 1.4e-13  wrow 5.9e-14 / 7.2e-14  b 4.5e-14 / 5.1e-14
      WaLTER  mu 5.2e-12 / 7.6e-13  u_lb 4.4e-12 / 6.9e-13  u_ub 1.4e-12 / 4.4e-13  fz_lb 2.0e-13 / 9.3e-14
              fz_ub 3.2e-12 / 5.0e-12  w_pos 7.0e-14 / 4.3e-14  w_rot 9.5e-14 / 3.4e-14
              M 6.6e-12 / 1.2e-12  C 8.8e-12 / 9.9e-13  J 2.8e-12 / 9.3e-13  wrow 5.5e-14 / 3.7e-14  b 1.4e-13 / 1.9e-13
    (dL/dT is dL/db's numbers; the numpy model of the formulation, tests/test_backward_env_ref.py,
    lands at the same order)"""
    fwd = solved(robot)
    assert (fwd[1].status.cpu().numpy() == 0).all()
    for tau_only in (False, True):
        got = backward(robot, fwd, be.grad_seed(robot, tau_only))
        ref = be.reference_env(robot, tau_only)
        errs = {k: br.env_errors(got[k], ref[k]) for k in ALL}
        print(f"\nbackward_env {robot} tau_only={tau_only}: " +
              "  ".join(f"{k} {errs[k].max():.3e} (env {errs[k].argmax()})" for k in ALL))
        for k in ALL:
            assert np.isfinite(got[k]).all(), k
        for k in ALL:
            assert errs[k].max() <= NORM_TOL, (tau_only, k, int(errs[k].argmax()), errs[k].max())


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_after_a_warm_solve(gpu, robot):
    """After osc_batch_solve_warm_env (two ticks on the same inputs, the second warm-started):
    within the contract of the same reference."""
    fwd = forward(robot, warm=True)
    assert (fwd[1].status.cpu().numpy() == 0).all()
    got = backward(robot, fwd, be.grad_seed(robot))
    ref = be.reference_env(robot)
    errs = {k: br.env_errors(got[k], ref[k]) for k in ALL}
    print(f"\nbackward_env after warm {robot}: " +
          "  ".join(f"{k} {errs[k].max():.3e}" for k in ALL))
    for k in ALL:
        assert errs[k].max() <= NORM_TOL, (k, int(errs[k].argmax()), errs[k].max())


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_model_constants_are_bitwise_backward_data(gpu, robot):
    """After the forward call without a block: the six data outputs with env_params=None and with
    a block of the model's constants are bitwise osc_batch_solve_backward_data's, and the seven
    parameter gradients of the two calls are bitwise each other's."""
    fwd = solved(robot, None)
    consts = block(ec.model_constants(robot))
    for tau_only in (False, True):
        gx = br.grad_seed("tumbling", robot, tau_only)
        want = backward_data(robot, fwd, gx)
        none, cst = backward(robot, fwd, gx, blk=None), backward(robot, fwd, gx, blk=consts)
        for k in OUTPUTS:
            assert bitwise(none[k], want[k]), (tau_only, "None", k)
            assert bitwise(cst[k], want[k]), (tau_only, "constants", k)
        for k in FIELDS:
            assert np.isfinite(none[k]).all() and bitwise(none[k], cst[k]), (tau_only, k)
        assert np.abs(none["mu"]).max() > 0.0     # (the shipped WaLTER box is never active)


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_structure(gpu, robot):
    """Exact zeros and exact sums: an inactive torque row and an absent bound get 0; no joint has
    a gradient on both bounds; an env whose mask is all zero has 0 in mu, fz_lb and fz_ub; an env
    with fz_lb = 0 has grad fz_lb = 0 (the convention); grad w_pos / w_rot are the ordered
    three-row sums of grad_wrow."""
    s, p = solver(robot), ec.params(robot)
    fwd = solved(robot)
    got = backward(robot, fwd, be.grad_seed(robot))
    nv, nu, nc, ns = (s.dims[k] for k in ("nv", "nu", "nc", "ns"))
    y = fwd[1].y.cpu().numpy()
    mask = ec.inputs(robot)["mask"]
    inf = ec.env_model(robot, p, 0).infinity / 1e10
    active = np.zeros((ec.NENV, nu), bool)
    for e in range(ec.NENV):
        active[e] = br.active_set(ec.env_model(robot, p, e), mask[e], y[e])[0]
    yu = y[:, nv + 4 * nc + nv:nv + 4 * nc + nv + nu]
    assert active.any() and (~active).any()
    assert (got["u_lb"][~active] == 0.0).all() and (got["u_ub"][~active] == 0.0).all()
    assert (got["u_lb"][np.abs(p["u_lb"]) >= inf] == 0.0).all()
    assert (got["u_ub"][np.abs(p["u_ub"]) >= inf] == 0.0).all()
    assert (got["u_lb"][yu > 0.0] == 0.0).all() and (got["u_ub"][yu <= 0.0] == 0.0).all()
    assert not ((got["u_lb"] != 0.0) & (got["u_ub"] != 0.0)).any()
    assert (got["u_lb"] != 0.0).any() and (got["u_ub"] != 0.0).any()
    assert (got["fz_lb"][p["fz_lb"] == 0.0] == 0.0).all()
    assert (got["fz_lb"] != 0.0).any() and (got["fz_ub"] != 0.0).any()
    for e in range(ec.NENV):
        pos, rot = be.site_sums(ec.env_model(robot, p, e), got["wrow"][e])
        assert bitwise(got["w_pos"][e], pos) and bitwise(got["w_rot"][e], rot), e
    # an env in the air: rows 0-4 of the batch with env 2's mask cleared
    d = {k: v[:5].copy() for k, v in ec.inputs(robot).items()}
    d["mask"][2] = 0.0
    air = forward(robot, rows=slice(0, 5), d=dict(d))
    assert int(air[1].status[2]) == 0
    g = backward(robot, air, be.grad_seed(robot)[:5])
    for k in ("mu", "fz_lb", "fz_ub"):
        assert g[k][2] == 0.0, k


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_linearity(gpu, robot):
    """The map is linear in gx to the contract: two calls' sum against one call on the summed
    seed, per output."""
    fwd = solved(robot)
    g1, g2 = be.grad_seed(robot), be.grad_seed(robot, True)[::-1].copy()
    a, b, ab = (backward(robot, fwd, g) for g in (g1, g2, g1 + g2))
    for k in ALL:
        err = br.env_errors(a[k] + b[k], ab[k])
        print(f"\nlinearity {robot} {k}: worst {err.max():.3e}")
        assert err.max() <= NORM_TOL, k


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_batch_independence(gpu, robot):
    """Envs 0-4 solved and differentiated alone (a batch of 5), and env 0 alone (a batch of 1),
    are bitwise what they are inside the 61-env batch."""
    gx = be.grad_seed(robot)
    full = backward(robot, solved(robot), gx)
    for n in (5, 1):
        part = backward(robot, forward(robot, rows=slice(0, n)), gx[:n])
        for k in ALL:
            assert bitwise(part[k], full[k][:n]), (n, k)


@pytest.mark.parametrize("robot", be.ROBOTS)
@pytest.mark.parametrize("how", ["nan_input", "invalid_parameter"])
def test_bad_env_isolation(gpu, robot, how):
    """One env of a wavefront with a NaN in M, or with an invalid parameter (u_lb >= u_ub on one
    joint): its status is OSC_SOLVE_NUMERICAL and every output of it is exactly zero; the other
    60 envs are bitwise those of the clean batch."""
    bad = 6
    gx = be.grad_seed(robot)
    clean = backward(robot, solved(robot), gx)
    d, p = ec.inputs(robot), ec.params(robot)
    if how == "nan_input":
        d = dict(d, M=d["M"].copy())
        d["M"][bad, 1, 1] = np.nan
    else:
        p = dict(p, u_lb=p["u_lb"].copy())
        p["u_lb"][bad, 1] = p["u_ub"][bad, 1]
    fwd = forward(robot, p, d=d)
    assert int(fwd[1].status[bad]) == NUMERICAL
    got = backward(robot, fwd, gx)
    keep = np.arange(ec.NENV) != bad
    for k in ALL:
        assert (got[k][bad] == 0.0).all(), k
        assert bitwise(got[k][keep], clean[k][keep]), k


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_null_outputs(gpu, robot):
    """Each of the thirteen outputs left NULL leaves the others bitwise unchanged; the parameter
    gradients alone (no solve with M, no pass over J) and the data outputs alone are bitwise what
    they are among all thirteen."""
    fwd, gx = solved(robot), be.grad_seed(robot)
    full = backward(robot, fwd, gx)
    for drop in ALL:
        part = backward(robot, fwd, gx, want=tuple(k for k in ALL if k != drop))
        assert drop not in part
        for k in part:
            assert bitwise(part[k], full[k]), (drop, k)
    for group in (("mu", "u_lb", "u_ub", "fz_lb", "fz_ub"), OUTPUTS, ("w_pos",), ("mu",)):
        part = backward(robot, fwd, gx, want=group)
        for k in group:
            assert bitwise(part[k], full[k]), (group, k)


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_autograd(gpu, robot):
    """(tau^2 + x . c).backward() through solve_differentiable_env with every field a tensor that
    requires grad: each .grad, T.grad and b.grad bitwise backward_env_into's on the same dL/dx;
    fields without requires_grad (tensor or numpy) stay None; data_grads=True adds M, C, J;
    solve_differentiable(..., env_params=...) still raises."""
    from osc_amd.autograd import solve_differentiable, solve_differentiable_env
    from osc_amd.solver import EnvParams
    s, p = solver(robot), ec.params(robot)
    d = s.dims
    c = torch.from_numpy(be.grad_seed(robot)).to(s.device)

    def run(fields, data_grads, numpy_fields=()):
        M, C, J, b, T, mask = (t.clone() for t in s.prepare(**ec.inputs(robot)))
        for t in (T, b) + ((M, C, J) if data_grads else ()):
            t.requires_grad_(True)
        t = {k: (p[k] if k in numpy_fields else torch.from_numpy(p[k]).to(s.device)) for k in FIELDS}
        for k in fields:
            t[k].requires_grad_(True)
        tau, x, status = solve_differentiable_env(s, M, C, J, b, T, mask, EnvParams(**t),
                                                  data_grads=data_grads)
        assert (status == 0).all() and not status.requires_grad
        (tau.square().sum() + (x * c).sum()).backward()
        gx = c.cpu().numpy().copy()
        gx[:, d["nv"]:d["nv"] + d["nu"]] += 2.0 * tau.detach().cpu().numpy()
        return t, dict(M=M, C=C, J=J, b=b, T=T, mask=mask), gx

    t, data, gx = run(FIELDS, False)
    ref = backward(robot, solved(robot), gx)
    for k in FIELDS:
        assert t[k].grad is not None and bitwise(t[k].grad.cpu().numpy(), ref[k]), k
    for k in ("T", "b"):
        assert bitwise(data[k].grad.cpu().numpy(), ref[k]), k
    assert data["M"].grad is None and data["mask"].grad is None
    t, data, gx = run(("mu", "w_pos"), True, numpy_fields=("fz_ub", "u_lb"))
    for k in FIELDS:
        if k in ("mu", "w_pos"):
            assert bitwise(t[k].grad.cpu().numpy(), ref[k]), k
        else:
            assert getattr(t[k], "grad", None) is None, k
    for k in ("M", "C", "J", "T", "b"):
        assert bitwise(data[k].grad.cpu().numpy(), ref[k]), k
    args = s.prepare(**ec.inputs(robot))
    with pytest.raises(ValueError):
        solve_differentiable_env(s, args[0].clone().requires_grad_(True), *args[1:], block(p))
    with pytest.raises(NotImplementedError):
        solve_differentiable(s, *args, env_params=block(p))


def test_argument_errors(gpu):
    """Refused before any launch: a model with wheel rows, a model created with refine_steps = 0,
    a misaligned parameter or gradient pointer, whatever osc_batch_solve_backward_data refuses, a
    workspace one byte short; EnvGrads of a wrong shape raise ValueError on the host; nenv == 0
    and no output at all are OSC_OK."""
    from osc_amd.solver import EnvGrads, OSCBatchSolver
    L, INVALID = _lib.lib(), 1
    robot = GO2
    s = solver(robot)
    (M, C, J, b, T, mask), out, blk = solved(robot)
    n = ec.NENV
    gx = torch.zeros((n, s.dims["n"]), dtype=torch.float64, device=s.device)
    gM = torch.zeros((n, s.dims["nv"], s.dims["nv"]), dtype=torch.float64, device=s.device)
    gmu = torch.zeros(n + 1, dtype=torch.float64, device=s.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    wsb = out.workspace.numel() * 8

    def call(h=s._h, nenv=n, M=p(M), J=p(J), b=p(b), T=p(T), mask=p(mask), x=p(out.x), y=p(out.y),
             st=p(out.status), g=p(gx), oM=p(gM), ws=p(out.workspace), nb=wsb, mu=blk.mu.data_ptr(),
             gmu_=gmu.data_ptr()):
        ep, eg = _lib.OscEnvParams(), _lib.OscEnvGrads()
        ep.mu, eg.mu = mu, gmu_
        return L.osc_batch_solve_backward_env(h, nenv, M, J, b, T, mask, ctypes.byref(ep), x, y,
                                              st, g, oM, None, None, None, None, None,
                                              ctypes.byref(eg), ws, ctypes.c_size_t(nb), None)

    assert call() == 0
    assert call(nenv=0) == 0
    assert call(oM=None, gmu_=None) == 0
    assert call(nenv=-1) == INVALID
    for name in ("M", "J", "b", "T", "mask", "x", "y", "st", "g", "ws"):
        assert call(**{name: None}) == INVALID, name
    assert call(J=ctypes.c_void_p(J.data_ptr() + 8)) == INVALID
    assert call(oM=ctypes.c_void_p(gM.data_ptr() + 8)) == INVALID
    assert call(mu=blk.mu.data_ptr() + 4) == INVALID
    assert call(gmu_=gmu.data_ptr() + 4) == INVALID
    assert call(gmu_=gmu.data_ptr() + 8) == 0             # (8-byte aligned: taken)
    need = ctypes.c_size_t()
    assert L.osc_workspace_bytes(s._h, n, ctypes.byref(need)) == 0
    assert call(nb=need.value - 1) == INVALID
    from test_gpu_wheels import NOSLIP_YAML
    wheels = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)   # the wheel no-slip rows switched on
    assert wheels.wheels
    assert call(h=wheels._h) == INVALID and call(h=wheels._h, nenv=0) == INVALID
    unrefined = OSCBatchSolver(robot, tuning={"refine_steps": 0})
    assert call(h=unrefined._h) == INVALID and call(h=unrefined._h, nenv=0) == INVALID
    torch.cuda.synchronize()
    before = gM.clone()
    for bad in (dict(mu=torch.zeros(n + 1, dtype=torch.float64, device=s.device)),
                dict(u_ub=torch.zeros((n, s.dims["nu"] + 1), dtype=torch.float64, device=s.device)),
                dict(w_rot=torch.zeros((n, s.dims["ns"]), dtype=torch.float32, device=s.device)),
                dict(fz_lb=torch.zeros(n, dtype=torch.float64))):
        with pytest.raises(ValueError):
            s.backward_env_into(out, M, J, b, T, mask, gx, env_params=blk, grad_M=gM,
                                env_grads=EnvGrads(**bad))
    torch.cuda.synchronize()
    assert torch.equal(gM, before)
