"""GPU tests of the backward pass with respect to the dynamics inputs (include/osc_backward.h,
osc_batch_solve_backward_data; csrc/osc_backward_data.hip; osc_amd/autograd.py): dL/dM, dL/dC,
dL/dJ, the per-row weight gradient and dL/dT, dL/db against the reference adjoint built from the
oracle (tests/backward_data_ref.py, pinned by the oracle's own differences in
tests/test_backward_data_ref.py), on the 61-env batches (a partial last wavefront) of
tests/backward_ref.py -- Go2 and WaLTER Sr standing and tumbling, and the `tight` and `absent`
descriptors -- and on batches of 1 and 5 envs.  Every env is compared.

Error per env and output: |g - g_ref|_inf / max(|g_ref|_inf, 1e-6 x the batch's largest
|g_ref|_inf) (backward_ref.env_errors).  Contract: 1e-5 (NORM_TOL of tests/test_gpu_parity.py).
ACHIEVED below is 10 x the worst error measured on an MI355X against the reference, per robot and
output; the bar is the smaller of it and the contract.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import backward_data_ref as bd
import backward_ref as br
import desc_variants as dv
from osc_amd import _lib
from test_gpu_parity import NORM_TOL

pytestmark = pytest.mark.gpu

GO2, WALTER = br.ROBOTS
CASES = [(b, r) for r in br.ROBOTS for b in br.BATCHES]
IDS = [f"{b}-{r}" for b, r in CASES]
NUMERICAL = _lib.SOLVE_NUMERICAL
OUTPUTS = bd.OUTPUTS
# robot -> output -> 10 x the worst error measured over its batches and both seeds
# (test_against_reference's docstring)
ACHIEVED = {
    GO2: dict(M=9.9e-9, C=9.7e-9, J=9.6e-9, wrow=1.8e-11, T=8.7e-11, b=8.7e-11),
    WALTER: dict(M=9.1e-6, C=9.1e-6, J=8.2e-6, wrow=4.6e-8, T=4.3e-8, b=4.3e-8),
}


def bar(robot, k):
    return min(ACHIEVED[robot][k], NORM_TOL)


@functools.lru_cache(maxsize=None)
def solver(batch, robot):
    from osc_amd.solver import OSCBatchSolver
    if batch in br.SHIPPED:
        return OSCBatchSolver(robot)
    return OSCBatchSolver(robot, desc_overrides=dv.overrides(batch, robot))


def forward(batch, robot, envs=None, poison=None):
    """Device inputs and the forward solve (x, duals, workspace) of the batch, or of its envs
    `envs`; poison = an env whose M gets a NaN."""
    s = solver(batch, robot)
    d = {k: (v if envs is None else v[envs]) for k, v in br.inputs(batch, robot).items()}
    if poison is not None:
        d = dict(d, M=d["M"].copy())
        d["M"][poison, 1, 1] = np.nan
    args = s.prepare(**d)
    out = s.alloc_outputs(args[0].shape[0], want_x=True, want_y=True)
    s.solve_into(out, *args)
    torch.cuda.synchronize()
    return args, out


@functools.lru_cache(maxsize=None)
def solved(batch, robot):
    """The whole batch's forward solve, shared by the tests (left unchanged)."""
    return forward(batch, robot)


def shapes(s, n):
    d = s.dims
    return dict(M=(n, d["nv"], d["nv"]), C=(n, d["nv"]), J=(n, d["s"], d["nv"]), wrow=(n, d["s"]),
                T=(n, d["ns"], 6), b=(n, d["s"]))


def backward_data(batch, robot, fwd, gx, want=OUTPUTS):
    """name -> gradient as numpy for the outputs in `want` (the others are passed as NULL), from
    gx (numpy, one row per env of the forward solve).  Outputs start as NaN."""
    s = solver(batch, robot)
    (M, C, J, b, T, mask), out = fwd
    n = out.tau.shape[0]
    g = torch.from_numpy(np.ascontiguousarray(gx)).to(s.device)
    sh = shapes(s, n)
    o = {k: torch.full(sh[k], float("nan"), dtype=torch.float64, device=s.device) for k in want}
    s.backward_data_into(out, M, J, b, T, mask, g, grad_M=o.get("M"), grad_C=o.get("C"),
                         grad_J=o.get("J"), grad_wrow=o.get("wrow"), grad_T=o.get("T"),
                         grad_b=o.get("b"))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def backward_first(batch, robot, fwd, gx):
    """(grad_T, grad_b) of the first entry, osc_batch_solve_backward."""
    s = solver(batch, robot)
    args, out = fwd
    n, d = out.tau.shape[0], s.dims
    g = torch.from_numpy(np.ascontiguousarray(gx)).to(s.device)
    gT = torch.full((n, d["ns"], 6), float("nan"), dtype=torch.float64, device=s.device)
    gb = torch.full((n, d["s"]), float("nan"), dtype=torch.float64, device=s.device)
    s.backward_into(out, args[2], args[5], g, gT, gb)
    torch.cuda.synchronize()
    return gT.cpu().numpy(), gb.cpu().numpy()


def bitwise(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_against_reference(gpu, batch, robot):
    """Every env of the batch, gx random over all of x and gx on tau alone: status OK and every
    output within min(ACHIEVED, the contract) of the reference adjoint.

    Worst errors measured on an MI355X, gx over all of x / on tau alone (ACHIEVED holds 10 x the
    worst of each robot and output; dL/dT is dL/db's numbers, and both are the first entry's):
      Go2     standing  M 2.8e-11 / 1.4e-11  C 2.1e-11 / 9.6e-12  J 9.1e-12 / 6.4e-12  wrow 1.6e-13 / 1.7e-13  b 4.6e-13 / 2.7e-13
              tumbling  M 1.8e-11 / 1.8e-11  C 1.5e-11 / 8.6e-12  J 1.9e-11 / 1.3e-11  wrow 8.1e-14 / 4.2e-14  b 1.7e-13 / 2.5e-13
              tight     M 5.4e-14 / 7.2e-14  C 3.3e-14 / 3.5e-14  J 2.6e-13 / 4.2e-14  wrow 7.8e-14 / 7.4e-14  b 4.2e-14 / 2.8e-14
              absent    M 8.5e-10 / 9.8e-10  C 7.9e-10 / 9.6e-10  J 1.7e-10 / 9.6e-10  wrow 7.3e-13 / 1.7e-12  b 2.2e-12 / 8.7e-12
      WaLTER  standing  M 9.0e-7 / 2.0e-7    C 9.0e-7 / 2.0e-7    J 8.2e-7 / 3.6e-7    wrow 4.6e-9 / 2.4e-9    b 4.2e-9 / 4.1e-9
              tumbling  M 2.0e-7 / 1.4e-7    C 2.0e-7 / 1.4e-7    J 2.9e-7 / 2.7e-7    wrow 7.4e-10 / 7.2e-10  b 1.5e-9 / 7.1e-10
              tight     M 7.6e-14 / 2.7e-14  C 5.6e-14 / 2.4e-14  J 1.0e-13 / 2.8e-14  wrow 1.1e-13 / 2.5e-14  b 1.1e-13 / 1.7e-14
              absent    M 7.8e-7 / 2.5e-7    C 7.8e-7 / 2.5e-7    J 2.9e-7 / 2.4e-7    wrow 9.0e-10 / 6.3e-10  b 2.6e-9 / 1.1e-9
    (the numpy model of the kernel, tests/test_backward_data_ref.py, lands at the same figures:
    WaLTER's dL/dM and dL/dC carry the error of v, the conditioning of its 32-column reduced
    Hessian, amplified by the solve with M -- a tenth of the contract)"""
    fwd = solved(batch, robot)
    assert (fwd[1].status.cpu().numpy() == 0).all()
    for tau_only in (False, True):
        got = backward_data(batch, robot, fwd, br.grad_seed(batch, robot, tau_only))
        ref = bd.reference_data(batch, robot, tau_only)
        errs = {k: br.env_errors(got[k], ref[k]) for k in OUTPUTS}
        print(f"\nbackward_data {batch} {robot} tau_only={tau_only}: " +
              "  ".join(f"{k} {errs[k].max():.3e} (env {errs[k].argmax()})" for k in OUTPUTS))
        for k in OUTPUTS:
            assert np.isfinite(got[k]).all(), k
        for k in OUTPUTS:
            assert errs[k].max() <= NORM_TOL, (tau_only, k, int(errs[k].argmax()), errs[k].max())
            assert errs[k].max() <= bar(robot, k), (tau_only, k, int(errs[k].argmax()), errs[k].max())


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_grad_T_and_b_are_the_first_entrys(gpu, batch, robot):
    """grad_T and grad_b of the new entry are bitwise osc_batch_solve_backward's."""
    fwd = solved(batch, robot)
    for tau_only in (False, True):
        gx = br.grad_seed(batch, robot, tau_only)
        got = backward_data(batch, robot, fwd, gx)
        T1, b1 = backward_first(batch, robot, fwd, gx)
        assert bitwise(got["T"], T1) and bitwise(got["b"], b1), tau_only


@pytest.mark.parametrize("batch,robot", [("tumbling", GO2), ("tight", WALTER)])
def test_linearity(gpu, batch, robot):
    """The map is linear in gx to the achieved bar: two calls' sum against one call on the summed
    seed, per output (measured: 1.9e-11 Go2 tumbling, dL/dM; 7.2e-15 WaLTER `tight`)."""
    fwd = solved(batch, robot)
    g1, g2 = br.grad_seed(batch, robot), br.grad_seed(batch, robot, True)[::-1].copy()
    a, b, ab = (backward_data(batch, robot, fwd, g) for g in (g1, g2, g1 + g2))
    for k in OUTPUTS:
        err = br.env_errors(a[k] + b[k], ab[k])
        print(f"\nlinearity {batch} {robot} {k}: worst {err.max():.3e}")
        assert err.max() <= bar(robot, k), k


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_batch_independence(gpu, robot):
    """Envs 0-4 solved and differentiated alone (a batch of 5), and env 0 alone (a batch of 1),
    are bitwise what they are inside the 61-env batch."""
    batch = "tumbling"
    gx = br.grad_seed(batch, robot)
    full = backward_data(batch, robot, solved(batch, robot), gx)
    for n in (5, 1):
        part = backward_data(batch, robot, forward(batch, robot, envs=np.arange(n)), gx[:n])
        for k in OUTPUTS:
            assert bitwise(part[k], full[k][:n]), (n, k)


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_nan_isolation(gpu, robot):
    """One env of a wavefront with a NaN in M: its status is OSC_SOLVE_NUMERICAL and every output
    of it is exactly zero; the other 60 envs are bitwise those of the clean batch."""
    batch, bad = "standing", 6
    gx = br.grad_seed(batch, robot)
    clean = backward_data(batch, robot, solved(batch, robot), gx)
    fwd = forward(batch, robot, poison=bad)
    assert int(fwd[1].status[bad]) == NUMERICAL
    got = backward_data(batch, robot, fwd, gx)
    keep = np.arange(br.NENV) != bad
    for k in OUTPUTS:
        assert (got[k][bad] == 0.0).all(), k
        assert bitwise(got[k][keep], clean[k][keep]), k


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_null_outputs(gpu, robot):
    """Each nullable output left NULL leaves the others bitwise unchanged; one output alone is
    bitwise what it is among all six."""
    batch = "tumbling"
    fwd, gx = solved(batch, robot), br.grad_seed(batch, robot)
    full = backward_data(batch, robot, fwd, gx)
    for drop in OUTPUTS:
        part = backward_data(batch, robot, fwd, gx, want=tuple(k for k in OUTPUTS if k != drop))
        assert drop not in part
        for k in part:
            assert bitwise(part[k], full[k]), (drop, k)
    for only in OUTPUTS:
        assert bitwise(backward_data(batch, robot, fwd, gx, want=(only,))[only], full[only]), only


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_autograd(gpu, robot):
    """(tau^2 + x . c).backward() through solve_differentiable(data_grads=True): M.grad, C.grad and
    J.grad bitwise backward_data_into's on the same dL/dx (T.grad and b.grad too); only the
    gradients asked for are there; data_grads=False with M.requires_grad still raises."""
    from osc_amd.autograd import solve_differentiable
    batch = "tumbling"
    s = solver(batch, robot)
    M, C, J, b, T, mask = (t.clone() for t in s.prepare(**br.inputs(batch, robot)))
    for t in (M, C, J, T):
        t.requires_grad_(True)
    c = torch.from_numpy(br.grad_seed(batch, robot)).to(s.device)
    tau, x, status = solve_differentiable(s, M, C, J, b, T, mask, data_grads=True)
    assert (status == 0).all() and not status.requires_grad
    (tau.square().sum() + (x * c).sum()).backward()
    assert b.grad is None and mask.grad is None
    d = s.dims
    gx = c.cpu().numpy().copy()
    gx[:, d["nv"]:d["nv"] + d["nu"]] += 2.0 * tau.detach().cpu().numpy()
    ref = backward_data(batch, robot, solved(batch, robot), gx)
    for k, t in (("M", M), ("C", C), ("J", J), ("T", T)):
        assert t.grad is not None and bitwise(t.grad.cpu().numpy(), ref[k]), k
    with pytest.raises(ValueError):
        solve_differentiable(s, M, C.detach(), J.detach(), b, T, mask)
    with pytest.raises(ValueError):
        solve_differentiable(s, M, C.detach(), J.detach(), b, T, mask, data_grads=False)


def test_argument_errors(gpu):
    """Refused before any launch: a model with wheel rows, nenv < 0, a NULL or misaligned array,
    a workspace one byte short; nenv == 0 and no output at all are OSC_OK."""
    from osc_amd.solver import OSCBatchSolver
    L, INVALID = _lib.lib(), 1
    batch, robot = "standing", GO2
    s = solver(batch, robot)
    (M, C, J, b, T, mask), out = solved(batch, robot)
    n = br.NENV
    gx = torch.zeros((n, s.dims["n"]), dtype=torch.float64, device=s.device)
    gM = torch.zeros((n, s.dims["nv"], s.dims["nv"]), dtype=torch.float64, device=s.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    wsb = out.workspace.numel() * 8

    def call(h=s._h, nenv=n, M=p(M), J=p(J), b=p(b), T=p(T), mask=p(mask), x=p(out.x), y=p(out.y),
             st=p(out.status), g=p(gx), oM=p(gM), ws=p(out.workspace), nb=wsb):
        return L.osc_batch_solve_backward_data(h, nenv, M, J, b, T, mask, x, y, st, g, oM, None,
                                               None, None, None, None, ws, ctypes.c_size_t(nb),
                                               None)

    assert call() == 0
    assert call(nenv=0) == 0
    assert call(oM=None) == 0
    assert call(nenv=-1) == INVALID
    for name in ("M", "J", "b", "T", "mask", "x", "y", "st", "g", "ws"):
        assert call(**{name: None}) == INVALID, name
    assert call(J=ctypes.c_void_p(J.data_ptr() + 8)) == INVALID
    assert call(M=ctypes.c_void_p(M.data_ptr() + 8)) == INVALID
    assert call(oM=ctypes.c_void_p(gM.data_ptr() + 8)) == INVALID
    need = ctypes.c_size_t()
    assert L.osc_workspace_bytes(s._h, n, ctypes.byref(need)) == 0
    assert call(nb=need.value - 1) == INVALID
    from test_gpu_wheels import NOSLIP_YAML
    wheels = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)   # the wheel no-slip rows switched on
    assert wheels.wheels
    assert call(h=wheels._h) == INVALID and call(h=wheels._h, nenv=0) == INVALID
    torch.cuda.synchronize()
