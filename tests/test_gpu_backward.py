"""GPU tests of the backward pass of the batched solve (include/osc_backward.h,
csrc/osc_backward.hip, osc_amd/autograd.py): dL/dT and dL/db against the reference adjoint built
from the oracle (tests/backward_ref.py, pinned by the oracle's own differences in
tests/test_backward_ref.py), on 61-env batches (a partial last wavefront) of Go2 and WaLTER Sr --
the shipped models standing and tumbling, and the `tight` and `absent` descriptors of
tests/desc_variants.py -- and on batches of 1 and 5 envs.  No env is left out
(test_backward_ref.EXCLUDED is empty).

Error per env: |g - g_ref|_inf / max(|g_ref|_inf, 1e-6 x the batch's largest |g_ref|_inf).
Contract: 1e-5 (NORM_TOL of tests/test_gpu_parity.py).  ACHIEVED below is 10 x the worst error
measured on an MI355X against the reference, never looser than the contract.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import backward_ref as br
import desc_variants as dv
from osc_amd import _lib
from test_backward_ref import EXCLUDED
from test_gpu_parity import NORM_TOL

pytestmark = pytest.mark.gpu

GO2, WALTER = br.ROBOTS
CASES = [(b, r) for r in br.ROBOTS for b in br.BATCHES]
IDS = [f"{b}-{r}" for b, r in CASES]
NUMERICAL = _lib.SOLVE_NUMERICAL
# robot -> 10 x the worst error measured over its batches and both seeds
# (test_against_reference's docstring)
ACHIEVED = {GO2: 8.7e-11, WALTER: 4.3e-8}


def bar(robot):
    return min(ACHIEVED[robot], NORM_TOL)


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


def backward(batch, robot, fwd, gx):
    """(grad_T, grad_b) as numpy, from gx (numpy, one row per env of the forward solve)."""
    s = solver(batch, robot)
    args, out = fwd
    n, d = out.tau.shape[0], s.dims
    g = torch.from_numpy(np.ascontiguousarray(gx)).to(s.device)
    gT = torch.full((n, d["ns"], 6), float("nan"), dtype=torch.float64, device=s.device)
    gb = torch.full((n, d["s"]), float("nan"), dtype=torch.float64, device=s.device)
    s.backward_into(out, args[2], args[5], g, gT, gb)
    torch.cuda.synchronize()
    return gT.cpu().numpy(), gb.cpu().numpy()


def relayout(gT):
    n = gT.shape[0]
    return np.concatenate([gT[:, :, :3].reshape(n, -1), gT[:, :, 3:].reshape(n, -1)], axis=1)


def bitwise(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_against_reference(gpu, batch, robot):
    """Every env of the batch, gx random over all of x and gx on tau alone: status OK, grad_T and
    grad_b within ACHIEVED (and the contract) of the reference adjoint.

    Worst errors measured on an MI355X (grad_b; grad_T is the same numbers re-laid out), gx over
    all of x / on tau alone; ACHIEVED holds 10 x the worst of each robot:
      Go2     standing 4.6e-13 / 2.7e-13   tumbling 1.7e-13 / 2.5e-13
              tight    4.2e-14 / 2.8e-14   absent   2.2e-12 / 8.7e-12
      WaLTER  standing 4.2e-9 / 4.1e-9     tumbling 1.5e-9 / 7.1e-10
              tight    1.1e-13 / 1.7e-14   absent   2.6e-9 / 1.1e-9
    (the numpy model of the kernel, tests/test_backward_ref.py, lands at the same figures: the
    error is the conditioning of WaLTER's 32-column reduced Hessian, not the kernel's schedule)"""
    assert not EXCLUDED
    fwd = solved(batch, robot)
    assert (fwd[1].status.cpu().numpy() == 0).all()
    for tau_only in (False, True):
        gT, gb = backward(batch, robot, fwd, br.grad_seed(batch, robot, tau_only))
        rT, rb = br.reference(batch, robot, tau_only)
        eb, eT = br.env_errors(gb, rb), br.env_errors(gT, rT)
        print(f"\nbackward {batch} {robot} tau_only={tau_only}: worst grad_b {eb.max():.3e} "
              f"(env {eb.argmax()}), grad_T {eT.max():.3e}; median {np.median(eb):.1e}; "
              f"{int((np.abs(rb).max(axis=1) <= 1e-12 * np.abs(rb).max()).sum())} envs with a zero "
              f"reference")
        assert np.isfinite(gT).all() and np.isfinite(gb).all()
        assert max(eb.max(), eT.max()) <= NORM_TOL, (tau_only, int(eb.argmax()), eb.max())
        assert max(eb.max(), eT.max()) <= bar(robot), (tau_only, int(eb.argmax()), eb.max())


@pytest.mark.parametrize("batch,robot", [("tumbling", GO2), ("tight", WALTER)])
def test_linear_identity(gpu, batch, robot):
    """grad_b == -grad_T re-laid out, bitwise; the map is linear in gx to rounding: two calls'
    sum against one call on the summed seed, each within the achieved bar of the exact map, so
    their difference within three bars."""
    fwd = solved(batch, robot)
    g1, g2 = br.grad_seed(batch, robot), br.grad_seed(batch, robot, True)[::-1].copy()
    T1, b1 = backward(batch, robot, fwd, g1)
    T2, b2 = backward(batch, robot, fwd, g2)
    T12, b12 = backward(batch, robot, fwd, g1 + g2)
    for T, b in ((T1, b1), (T2, b2), (T12, b12)):
        assert bitwise(b, -relayout(T))
    err = br.env_errors(b1 + b2, b12)
    print(f"\nlinearity {batch} {robot}: worst {err.max():.3e}")
    assert err.max() <= 3.0 * bar(robot)


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_batch_independence(gpu, robot):
    """Envs 0-4 solved and differentiated alone (a batch of 5), and env 0 alone (a batch of 1),
    are bitwise what they are inside the 61-env batch -- and so within the bar of the reference."""
    batch = "tumbling"
    gx = br.grad_seed(batch, robot)
    T, b = backward(batch, robot, solved(batch, robot), gx)
    for n in (5, 1):
        Tn, bn = backward(batch, robot, forward(batch, robot, envs=np.arange(n)), gx[:n])
        assert bitwise(Tn, T[:n]) and bitwise(bn, b[:n]), n


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_nan_isolation(gpu, robot):
    """One env of a wavefront with a NaN in M: its status is OSC_SOLVE_NUMERICAL and its gradients
    are exactly zero; the other 60 envs are bitwise those of the clean batch."""
    batch, bad = "standing", 6
    gx = br.grad_seed(batch, robot)
    T, b = backward(batch, robot, solved(batch, robot), gx)
    fwd = forward(batch, robot, poison=bad)
    assert int(fwd[1].status[bad]) == NUMERICAL
    Tp, bp = backward(batch, robot, fwd, gx)
    assert (Tp[bad] == 0.0).all() and (bp[bad] == 0.0).all()
    keep = np.arange(br.NENV) != bad
    assert bitwise(Tp[keep], T[keep]) and bitwise(bp[keep], b[keep])


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_masked_contacts(gpu, robot):
    """A contact with mask == 0 has all three forces fixed: dL/dT does not change, bitwise, when
    grad_x's entries on the masked forces do."""
    batch = "tumbling"
    mdl = br.model_of(batch, robot)
    gx = br.grad_seed(batch, robot)
    off = np.repeat(br.inputs(batch, robot)["mask"] == 0, 3, axis=1)
    assert off.any() and not off.all()
    g2 = gx.copy()
    g2[:, mdl.nv + mdl.nu:][off] = 7.5 - 3.0 * g2[:, mdl.nv + mdl.nu:][off]
    fwd = solved(batch, robot)
    T, _ = backward(batch, robot, fwd, gx)
    T2, _ = backward(batch, robot, fwd, g2)
    assert np.abs(T).max() > 0.0 and bitwise(T, T2)


@pytest.mark.parametrize("robot", br.ROBOTS)
def test_autograd(gpu, robot):
    """(tau^2 + x . c).backward() through solve_differentiable: T.grad bitwise backward_into's
    result on the same dL/dx; b.grad present; M.grad None; an M with requires_grad raises."""
    from osc_amd.autograd import solve_differentiable
    batch = "tumbling"
    s = solver(batch, robot)
    M, C, J, b, T, mask = s.prepare(**br.inputs(batch, robot))
    T = T.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    c = torch.from_numpy(br.grad_seed(batch, robot)).to(s.device)
    tau, x, status = solve_differentiable(s, M, C, J, b, T, mask)
    assert (status == 0).all() and not status.requires_grad
    (tau.square().sum() + (x * c).sum()).backward()
    assert T.grad is not None and b.grad is not None and M.grad is None
    d = s.dims
    gx = c.cpu().numpy().copy()
    gx[:, d["nv"]:d["nv"] + d["nu"]] += 2.0 * tau.detach().cpu().numpy()
    Tg, bg = backward(batch, robot, solved(batch, robot), gx)
    assert bitwise(T.grad.cpu().numpy(), Tg) and bitwise(b.grad.cpu().numpy(), bg)
    with pytest.raises(ValueError):
        solve_differentiable(s, M.clone().requires_grad_(True), C, J, b, T, mask)


def test_argument_errors(gpu):
    """Refused before any launch: a model with wheel rows, nenv < 0, a NULL or misaligned array,
    a workspace one byte short; nenv == 0 is OSC_OK."""
    from osc_amd.solver import OSCBatchSolver
    L, INVALID = _lib.lib(), 1
    batch, robot = "standing", GO2
    s = solver(batch, robot)
    args, out = solved(batch, robot)
    n = br.NENV
    gx = torch.zeros((n, s.dims["n"]), dtype=torch.float64, device=s.device)
    gT = torch.zeros((n, s.dims["ns"], 6), dtype=torch.float64, device=s.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    wsb = out.workspace.numel() * 8

    def call(h=s._h, nenv=n, J=p(args[2]), mask=p(args[5]), y=p(out.y), st=p(out.status),
             g=p(gx), T=p(gT), ws=p(out.workspace), nb=wsb):
        return L.osc_batch_solve_backward(h, nenv, J, mask, y, st, g, T, None, ws,
                                          ctypes.c_size_t(nb), None)

    assert call() == 0
    assert call(nenv=0) == 0
    assert call(nenv=-1) == INVALID
    assert call(J=None) == INVALID and call(y=None) == INVALID and call(ws=None) == INVALID
    assert call(J=ctypes.c_void_p(args[2].data_ptr() + 8)) == INVALID
    need = ctypes.c_size_t()
    assert L.osc_workspace_bytes(s._h, n, ctypes.byref(need)) == 0
    assert call(nb=need.value - 1) == INVALID
    from test_gpu_wheels import NOSLIP_YAML
    wheels = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)   # the wheel no-slip rows switched on
    assert wheels.wheels
    assert call(h=wheels._h) == INVALID and call(h=wheels._h, nenv=0) == INVALID
    torch.cuda.synchronize()
