"""GPU tests of model descriptors other than the three shipped YAML files (tests/desc_variants.py:
tight, absent, lifted), through OSCBatchSolver(desc_overrides=...), against the exact CPU
oracle of the same model.  The kernels read friction, weights, bounds and the infinity threshold
at run time (DevParams); these models make every row kind active (the fz cap and WaLTER's torque
bounds included), absent (one-sided and unbounded torques, unbounded fz, a threshold other than
the shipped one) or lifted (a non-zero fz lower bound), with a mask of 0 / 0.5 / 1 scaling the fz
bounds.  tests/test_desc_variants.py (CPU) holds the precondition: how many rows of each kind are
active at the oracle's optimum of these very batches.

Wheel-row models are out of scope: their oracle needs a phase-1 LP for its start and their
statuses have their own rules (tests/test_gpu_wheels.py).

Tolerances: the contract and the KKT bars are those of tests/test_gpu_parity.py and
tests/test_gpu_wheels.py, imported from there.  ACHIEVED below is 10 x the worst error measured
on an MI355X against the oracle (the margin covers the last-bit changes a re-schedule of the
kernels is allowed), never looser than the contract.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import desc_variants as dv
from osc_amd.synth import SEED_BASE, generate, random_walk
from osc_qp import b_matrix
from test_gpu_parity import ELEM_TOL, NORM_TOL, _rel_errors
from test_gpu_stages import check_reduced_qp
from test_gpu_wheels import _batched_qp, _certify, _kkt

pytestmark = pytest.mark.gpu

GO2, WALTER = "unitree_go2", "walter_sr"
ONE_WAVE, TWO_WAVE, UNREFINED = (("small_batch_max", 100000000),), (("small_batch_max", 0),), \
    (("refine_steps", 0),)
# (model, refinement on): (normwise, elementwise above the 1 % floor) = 10 x the worst measured
# over the model's parity cases, both robots (see test_parity_every_env's docstring)
ACHIEVED = {("tight", True): (5.75e-12, 4.03e-11), ("absent", True): (2.46e-10, 3.06e-10),
            ("lifted", True): (5.52e-12, 4.11e-11), ("tight", False): (1.92e-9, 5.59e-9)}


@functools.lru_cache(maxsize=None)
def solver(name, robot, tuning=()):
    from osc_amd.solver import OSCBatchSolver
    return OSCBatchSolver(robot, tuning=dict(tuning), desc_overrides=dv.overrides(name, robot))


@functools.lru_cache(maxsize=None)
def solved(name, robot, tuning=(), want_y=True):
    """One solve of the variant's batch, shared by the tests that compare it (left unchanged)."""
    s = solver(name, robot, tuning)
    res = s.solve(**dv.inputs(name, robot), want_x=True, want_y=want_y)
    torch.cuda.synchronize()
    return res


def _np(t):
    return t.cpu().numpy()


def _x_error(x, xo):
    return (np.abs(x - xo) / np.maximum(np.abs(xo).max(axis=1, keepdims=True), 1.0)).max(axis=1)


def _within_contract(tau, x, xo, mdl):
    """Per env: tau normwise and elementwise above the floor, x normwise, all within the contract
    (a NaN is outside it)."""
    nw, el = _rel_errors(tau, xo[:, mdl.nv:mdl.nv + mdl.nu])
    return nw, el, (nw <= NORM_TOL) & (el <= ELEM_TOL) & (_x_error(x, xo) <= NORM_TOL)


def _feasible(mdl, d, x, tol=1e-7):
    """x within the variant's own bounds to tol, its dynamics residual within the bound of
    test_gpu_parity.test_full_size_properties, masked contacts exactly zero."""
    nv, nu, nc = mdl.nv, mdl.nu, mdl.nc
    dvv, u, z = x[:, :nv], x[:, nv:nv + nu], x[:, nv + nu:]
    Jc = np.transpose(d["J"][:, 3 * mdl.ns - mdl.nz:3 * mdl.ns, :], (0, 2, 1))
    res = np.einsum("eij,ej->ei", d["M"], dvv) + d["C"] - u @ b_matrix(mdl).T - \
        np.einsum("eij,ej->ei", Jc, z)
    assert (np.abs(res).max(axis=1) / (1.0 + np.abs(d["C"]).max(axis=1))).max() <= 1e-8
    assert ((u >= mdl.u_lb - tol) & (u <= mdl.u_ub + tol)).all()
    zz = z.reshape(-1, nc, 3)
    m = d["mask"]
    assert (zz[m == 0] == 0.0).all()
    assert (np.abs(zz[:, :, 0]) + np.abs(zz[:, :, 1]) <= mdl.mu * zz[:, :, 2] + tol).all()
    on = m != 0
    assert (zz[:, :, 2][on] >= (mdl.z_lb[2] * m)[on] - tol).all()
    assert (zz[:, :, 2][on] <= (mdl.z_ub[2] * m)[on] + tol).all()


def _no_dual_on_absent_rows(mdl, mask, y):
    """Rows over A = [Aeq; Aineq; I_n].  Exactly zero on every side the model has no row for:
    the pyramid rows' lower side, the dv box, fx / fy, and a torque or fz side at or above the
    threshold (infinity / 1e10, include/osc_batch.h)."""
    nv, nu, nc, n = mdl.nv, mdl.nu, mdl.nc, mdl.n
    thr = mdl.infinity * 1e-10
    pyr = y[:, nv:nv + 4 * nc]
    box = y[:, nv + 4 * nc:]
    assert (pyr >= 0.0).all()
    assert (box[:, :nv] == 0.0).all()
    ub = box[:, nv:nv + nu]
    assert (ub[:, np.abs(mdl.u_ub) >= thr] <= 0.0).all()
    assert (ub[:, np.abs(mdl.u_lb) >= thr] >= 0.0).all()
    zb = box[:, nv + nu:].reshape(-1, nc, 3)
    on = mask != 0
    assert (zb[:, :, :2][on] == 0.0).all()
    if abs(mdl.z_ub[2]) >= thr:
        assert (zb[:, :, 2][on] <= 0.0).all()
    if abs(mdl.z_lb[2]) >= thr:
        assert (zb[:, :, 2][on] >= 0.0).all()


def test_unknown_descriptor_field_refused(gpu):
    from osc_amd.solver import OSCBatchSolver
    with pytest.raises(KeyError):
        OSCBatchSolver(GO2, desc_overrides={"friction": 0.5})
    with pytest.raises(ValueError):
        OSCBatchSolver(GO2, desc_overrides={"z_lb": [0.0] * 4})


PARITY = [(n, GO2, t) for n in dv.NAMES for t in (ONE_WAVE, TWO_WAVE)] + \
    [(n, WALTER, ()) for n in dv.NAMES] + [("tight", GO2, UNREFINED), ("tight", WALTER, UNREFINED)]


@pytest.mark.parametrize("name,robot,tuning", PARITY,
                         ids=[f"{n}-{r}-{'-'.join(f'{k}{v}' for k, v in t) or 'default'}"
                              for n, r, t in PARITY])
def test_parity_every_env(gpu, name, robot, tuning):
    """Every env of the 61-env batch: status OK; tau within the contract of test_gpu_parity.py
    (normwise and elementwise above the 1 % floor <= 1e-5) of the oracle's certified optimum and x
    normwise within it; masked contacts exactly 0; x feasible for the variant's own bounds to
    1e-7 and on the dynamics to 1e-8; the KKT certificate of (x, y) at the bars of
    test_gpu_wheels.py; no dual on a row the model switches off.  (refine_steps 0: the interior
    point alone to mu <= 1e-12; the library exports duals only with the refinement, so the
    certificate and the dual rows are checked on the refined cases.)

    Worst errors measured on an MI355X, normwise / elementwise above the floor (Go2 one-wave and
    two-wave are bitwise equal); ACHIEVED holds 10 x the worst of each model:
      tight   Go2 5.75e-13 / 4.03e-12   WaLTER 5.80e-14 / 2.40e-13   (iterations <= 31 / 37)
      absent  Go2 2.37e-13 / 9.92e-13   WaLTER 2.46e-11 / 3.06e-11   (<= 13 / 15)
      lifted  Go2 5.52e-13 / 4.11e-12   WaLTER 1.16e-13 / 5.40e-13   (<= 30 / 31)
      tight, refine_steps 0   Go2 1.92e-10 / 5.59e-10   WaLTER 2.81e-11 / 1.16e-10
    Before the re-centre of the interior point kept off iterates with large multipliers
    (osc_ipm.hpp, kRecentreLamMax) 2 / 27 tight and 1 / 3 lifted envs (Go2 / WaLTER) came back
    OSC_SOLVE_MAX_ITER, and the absent model's one-sided torques carried duals of 1e-9..1e-8
    (scaled) on their absent side (osc_dual.hip)."""
    mdl, d = dv.model(name, robot), dv.inputs(name, robot)
    xo, _ = dv.oracle(name, robot)
    refined = tuning != UNREFINED     # (the duals come from the refinement: none without it)
    res = solved(name, robot, tuning, refined)
    st = _np(res.status)
    assert (st == 0).all(), np.bincount(st)
    tau, x = _np(res.tau), _np(res.x)
    nw, el, ok = _within_contract(tau, x, xo, mdl)
    print(f"\n{name} {robot} {dict(tuning)}: worst normwise {nw.max():.2e} (env {int(nw.argmax())}), "
          f"elementwise {el.max():.2e}, x normwise {_x_error(x, xo).max():.2e}, "
          f"iters max {int(res.iters.max())}")
    assert ok.all(), (nw.max(), el.max(), _x_error(x, xo).max(), np.nonzero(~ok)[0])
    _feasible(mdl, d, x)
    if refined:
        args = solver(name, robot, tuning).prepare(**d)
        _certify(_kkt(*_batched_qp(mdl, *args), res.x, res.y), (name, robot))
        _no_dual_on_absent_rows(mdl, d["mask"], _np(res.y))
    norm_ach, elem_ach = ACHIEVED[name, refined]
    assert norm_ach <= NORM_TOL and elem_ach <= ELEM_TOL
    assert nw.max() <= norm_ach and el.max() <= elem_ach, (nw.max(), el.max())


@pytest.mark.parametrize("name", ["tight", "absent"])
def test_one_wave_and_two_wave_bitwise_equal(gpu, name):
    a, b = solved(name, GO2, ONE_WAVE), solved(name, GO2, TWO_WAVE)
    for k in ("tau", "x", "y", "status", "iters"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("robot", dv.ROBOTS)
def test_split_entries_bitwise_the_fused_solve(gpu, robot):
    s, d = solver("tight", robot), dv.inputs("tight", robot)
    args = s.prepare(**d)
    split = s.alloc_outputs(dv.NENV, want_x=True)
    s.assemble_into(split, *args)
    s.solve_assembled_into(split, args[5])
    torch.cuda.synchronize()
    fused = solved("tight", robot, (), False)
    for k in ("tau", "x", "status", "iters"):
        assert torch.equal(getattr(fused, k), getattr(split, k)), k


@pytest.mark.parametrize("robot", dv.ROBOTS)
def test_duals_leave_primal_unchanged(gpu, robot):
    a, b = solved("tight", robot, (), True), solved("tight", robot, (), False)
    for k in ("tau", "x", "status", "iters"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("robot", dv.ROBOTS)
def test_warm_ticks_vs_oracle(gpu, robot):
    """The cold first tick, then three ticks of the 1 % random walk through solve_warm_into: each
    within the contract of the oracle's optimum of that tick's own inputs, every status OK."""
    s, mdl = solver("tight", robot), dv.model("tight", robot)
    d = dv.inputs("tight", robot)
    rng = np.random.default_rng(11)
    warm = s.alloc_warm_state(dv.NENV)
    out = s.alloc_outputs(dv.NENV, want_x=True)
    for tick in range(4):
        xo = dv.oracle("tight", robot)[0] if tick == 0 else dv.solve_oracle(mdl, d)[0]
        s.solve_warm_into(out, warm, *s.prepare(**d))
        torch.cuda.synchronize()
        st = _np(out.status)
        assert (st == 0).all(), (tick, np.bincount(st))
        nw, el, ok = _within_contract(_np(out.tau), _np(out.x), xo, mdl)
        print(f"\ntight {robot} warm tick {tick}: normwise {nw.max():.2e}, elementwise "
              f"{el.max():.2e}, mean iters {float(out.iters.float().mean()):.1f}")
        assert ok.all(), (tick, nw.max(), el.max(), np.nonzero(~ok)[0])
        d = random_walk(d, rng)


def test_pair_kernel_bitwise_the_solo_solves(gpu):
    """osc_batch_solve_multi with a WaLTER and a Go2 job of one resident wavefront each: the
    two-model grid, two descriptors' parameters side by side."""
    from osc_amd.solver import solve_multi_into
    jobs = []
    for robot in (WALTER, GO2):
        s = solver("tight", robot)
        jobs.append((s, s.alloc_outputs(dv.NENV, want_x=True), s.prepare(**dv.inputs("tight", robot))))
    solve_multi_into(jobs)
    torch.cuda.synchronize()
    for (s, o, _) in jobs:
        r = solved("tight", s.robot, (), False)
        for k in ("tau", "x", "status", "iters"):
            assert torch.equal(getattr(o, k), getattr(r, k)), (s.robot, k)


@pytest.mark.parametrize("robot", dv.ROBOTS)
def test_reduced_qp_uses_the_descriptor(gpu, robot):
    """The assembly kernel's weights, w_torque and w_reg: the checker of
    test_gpu_stages.test_reduced_qp_consistent_with_oracle_qp on the tight model."""
    check_reduced_qp(gpu, solver("tight", robot), dv.model("tight", robot), dv.inputs("tight", robot))


def test_compaction_bitwise_equal_on_tight(gpu):
    """Lockstep compaction with torque bounds and the fz cap in the active set: WaLTER tight,
    20,480 envs, the default park iteration against none (test_gpu_stages's shape; no oracle)."""
    inp = generate(WALTER, 20480, SEED_BASE + 34, "tumbling", "bernoulli")
    inp["mask"] = dv.fractional_mask(inp["mask"])
    outs = []
    for tuning in ((), (("park_it", 0),)):
        s = solver("tight", WALTER, tuning)
        o = s.alloc_outputs(20480, want_x=True)
        s.solve_into(o, *s.prepare(**inp))
        torch.cuda.synchronize()
        outs.append(o)
    it = _np(outs[1].iters)
    assert (it > 16).any() and (it <= 16).any()   # both passes ran
    print(f"\nstatuses {np.bincount(_np(outs[1].status), minlength=4)}, iters max {int(it.max())}")
    for k in ("tau", "x", "status", "iters"):
        assert torch.equal(getattr(outs[0], k), getattr(outs[1], k)), k
