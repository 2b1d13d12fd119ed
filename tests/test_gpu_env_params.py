"""GPU tests of the per-env parameters (include/osc_env_params.h, osc_amd.solver.EnvParams): friction,
torque box, fz bounds and task weights per env next to the usual inputs, through the _env entry
points and their kernels (osc_setup_env_kernel, osc_ipm_env_kernel, osc_refine_env_kernel,
osc_dual_env_kernel).  tests/env_params_cases.py holds the 61-env batch, the draw and each env's
oracle; tests/test_env_params_ref.py (CPU) holds the precondition.

Tolerances: the contract and the KKT bars are those of tests/test_gpu_parity.py and
tests/test_gpu_wheels.py, imported from there.  ACHIEVED below is 10 x the worst error measured on
an MI355X against the oracle, never looser than the contract (as tests/test_gpu_descriptors.py).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import desc_variants as dv
import env_params_cases as ec
from test_gpu_descriptors import _feasible, _no_dual_on_absent_rows, _np, _within_contract, _x_error
from test_gpu_parity import ELEM_TOL, NORM_TOL
from test_gpu_wheels import _batched_qp, _certify, _kkt

pytestmark = pytest.mark.gpu

GO2, WALTER = "unitree_go2", "walter_sr"
ONE_WAVE, TWO_WAVE = (("small_batch_max", 100000000),), (("small_batch_max", 0),)
CASES = [(GO2, ONE_WAVE), (GO2, TWO_WAVE), (WALTER, ())]
CASE_IDS = ["go2-one-wave", "go2-two-wave", "walter"]
KEYS = ("tau", "x", "y", "status", "iters")
NUMERICAL = 2
# robot: (normwise, elementwise above the 1 % floor) = 10 x the worst measured over the parity
# and warm-tick cases (see test_parity_every_env's docstring)
ACHIEVED = {GO2: (1.98e-11, 1.71e-10), WALTER: (2.16e-12, 4.17e-11)}


@functools.lru_cache(maxsize=None)
def solver(robot, tuning=(), overrides=None):
    from osc_amd.solver import OSCBatchSolver
    return OSCBatchSolver(robot, tuning=dict(tuning),
                          desc_overrides=dict(overrides) if overrides else None)


def env_block(p, fields=ec.FIELDS, rows=slice(None)):
    """EnvParams of the named fields of p (device tensors), the others None."""
    from osc_amd.solver import EnvParams
    return EnvParams(**{k: torch.as_tensor(np.ascontiguousarray(p[k][rows])).cuda() for k in fields})


def solve(robot, tuning, d, p=None, fields=ec.FIELDS, rows=slice(None), want_y=True, s=None):
    s = s or solver(robot, tuning)
    d = {k: v[rows] for k, v in d.items()}
    res = s.solve(**d, want_x=True, want_y=want_y,
                  env_params=None if p is None else env_block(p, fields, rows))
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def solved(robot, tuning=(), want_y=True):
    """The drawn batch with its drawn parameters, shared by the tests that compare it."""
    return solve(robot, tuning, ec.inputs(robot), ec.params(robot), want_y=want_y)


def assert_bitwise(a, b, where, keys=KEYS, rows_a=slice(None), rows_b=slice(None)):
    for k in keys:
        ta, tb = getattr(a, k)[rows_a], getattr(b, k)[rows_b]
        assert torch.equal(ta, tb), (where, k, int((ta != tb).reshape(ta.shape[0], -1).any(1).sum()))


@pytest.mark.parametrize("robot,tuning", CASES, ids=CASE_IDS)
def test_model_constants_per_env_are_bitwise_the_existing_entry(gpu, robot, tuning):
    """EnvParams filled with the model's own constants -- each field alone, all together, and an
    all-None block -- against solve() without it: tau, x, y, status, iters torch.equal."""
    d, p = ec.inputs(robot), ec.model_constants(robot)
    ref = solve(robot, tuning, d)
    for fields in [(f,) for f in ec.FIELDS] + [ec.FIELDS, ()]:
        assert_bitwise(solve(robot, tuning, d, p, fields), ref, fields)


def _three_descriptors(robot):
    """The shipped descriptor and two that differ from it only in the seven per-env fields."""
    seven = ("mu", "u_lb", "u_ub", "z_lb", "z_ub", "w_pos", "w_rot")
    tight, lifted = dv.overrides("tight", robot), dv.overrides("lifted", robot)
    return [{}, {k: tight[k] for k in seven}, {k: lifted[k] for k in seven if k in lifted}]


@pytest.mark.parametrize("robot,tuning", CASES, ids=CASE_IDS)
def test_mixed_batch_is_bitwise_the_per_model_solves(gpu, robot, tuning):
    """Env e takes descriptor e % 3; each env's outputs are bitwise its row of the solve of the
    whole batch by OSCBatchSolver(desc_overrides=<its descriptor>)."""
    from osc_qp import load_model
    d = ec.inputs(robot)
    descs = _three_descriptors(robot)
    models = [load_model(robot, overrides=o) for o in descs]
    p = {k: [] for k in ec.FIELDS}
    for e in range(ec.NENV):
        m = models[e % 3]
        for k, v in dict(mu=m.mu, u_lb=m.u_lb, u_ub=m.u_ub, fz_lb=m.z_lb[2], fz_ub=m.z_ub[2],
                         w_pos=m.w_pos, w_rot=m.w_rot).items():
            p[k].append(v)
    p = {k: np.array(v, dtype=np.float64) for k, v in p.items()}
    mixed = solve(robot, tuning, d, p)
    for k, o in enumerate(descs):
        key = tuple((n, tuple(v) if isinstance(v, list) else v) for n, v in o.items())
        per_model = solve(robot, tuning, d, s=solver(robot, tuning, key))
        rows = slice(k, None, 3)
        assert_bitwise(mixed, per_model, (robot, k), rows_a=rows, rows_b=rows)


def _per_env_kkt(robot, args, p, res):
    qps = []
    for e in range(ec.NENV):
        qps.append(_batched_qp(ec.env_model(robot, p, e), *[a[e:e + 1] for a in args]))
    return _kkt(*[torch.cat([q[i] for q in qps]) for i in range(5)], res.x, res.y)


def _check_against_oracle(robot, d, p, res, xo, where, duals=True):
    from osc_qp import load_model
    base = load_model(robot)
    st = _np(res.status)
    assert (st == 0).all(), (where, np.bincount(st))
    tau, x = _np(res.tau), _np(res.x)
    nw, el, ok = _within_contract(tau, x, xo, base)
    print(f"\n{where}: worst normwise {nw.max():.2e} (env {int(nw.argmax())}), elementwise "
          f"{el.max():.2e}, x normwise {_x_error(x, xo).max():.2e}, iters max "
          f"{int(res.iters.max())}, mean {float(res.iters.float().mean()):.1f}")
    assert ok.all(), (where, nw.max(), el.max(), _x_error(x, xo).max(), np.nonzero(~ok)[0])
    for e in range(x.shape[0]):      # each env feasible for its own bounds (1e-7), mask zeros exact
        _feasible(ec.env_model(robot, p, e), {k: v[e:e + 1] for k, v in d.items()}, x[e:e + 1])
    if duals:
        y = _np(res.y)
        for e in range(x.shape[0]):
            _no_dual_on_absent_rows(ec.env_model(robot, p, e), d["mask"][e:e + 1], y[e:e + 1])
    norm_ach, elem_ach = ACHIEVED[robot]
    assert norm_ach <= NORM_TOL and elem_ach <= ELEM_TOL
    assert nw.max() <= norm_ach and el.max() <= elem_ach, (where, nw.max(), el.max())


@pytest.mark.parametrize("robot,tuning", CASES, ids=CASE_IDS)
def test_parity_every_env(gpu, robot, tuning):
    """The drawn batch, every env against the oracle's certified optimum of ITS OWN model: status
    OK; tau within the contract of test_gpu_parity.py (normwise and elementwise above the 1 %
    floor <= 1e-5) and x normwise within it; masked contacts exactly 0; x feasible for the env's
    own bounds to 1e-7; the KKT certificate of (x, y) at the bars of test_gpu_wheels.py with each
    env's QP built from its own model; no dual on a side the env switches off.

    Worst errors measured on an MI355X, normwise / elementwise above the floor (Go2 one-wave and
    two-wave are bitwise equal); ACHIEVED holds 10 x the worst of each robot, warm ticks included:
      Go2     cold 1.98e-12 / 1.71e-11 (iterations <= 31), warm ticks 1-3 <= 1.24e-12 / 8.72e-12
      WaLTER  cold 1.36e-13 / 8.97e-13 (iterations <= 36), warm ticks 1-3 <= 2.16e-13 / 4.17e-12"""
    d, p = ec.inputs(robot), ec.params(robot)
    res = solved(robot, tuning)
    _check_against_oracle(robot, d, p, res, ec.oracle(robot)[0], f"{robot} {dict(tuning)}")
    args = solver(robot, tuning).prepare(**d)
    _certify(_per_env_kkt(robot, args, p, res), (robot, tuning))


def test_one_wave_and_two_wave_bitwise_equal(gpu):
    assert_bitwise(solved(GO2, ONE_WAVE), solved(GO2, TWO_WAVE), "go2")


@pytest.mark.parametrize("robot,tuning", CASES, ids=CASE_IDS)
def test_split_entries_bitwise_the_fused_solve(gpu, robot, tuning):
    """assemble_into + solve_assembled_into with env_params against the fused call; and the fused
    call with and without the duals."""
    s, blk = solver(robot, tuning), env_block(ec.params(robot))
    args = s.prepare(**ec.inputs(robot))
    split = s.alloc_outputs(ec.NENV, want_x=True)
    s.assemble_into(split, *args, env_params=blk)
    s.solve_assembled_into(split, args[5], env_params=blk)
    torch.cuda.synchronize()
    fused = solved(robot, tuning, False)
    primal = ("tau", "x", "status", "iters")
    assert_bitwise(split, fused, "split", primal)
    assert_bitwise(solved(robot, tuning, True), fused, "duals", primal)


@pytest.mark.parametrize("robot,tuning", CASES, ids=CASE_IDS)
def test_warm_ticks_vs_oracle(gpu, robot, tuning):
    """One cold tick, then three ticks of the 1 % random walk through solve_warm_into with mu and
    the torque boxes redrawn at every tick (same finite / absent pattern): every status OK, every
    tick within the contract of that tick's oracle (each env's own model)."""
    s = solver(robot, tuning)
    warm = s.alloc_warm_state(ec.NENV)
    out = s.alloc_outputs(ec.NENV, want_x=True)
    for tick, (d, p, xo) in enumerate(ec.warm_ticks(robot)):
        s.solve_warm_into(out, warm, *s.prepare(**d), env_params=env_block(p))
        torch.cuda.synchronize()
        _check_against_oracle(robot, d, p, out, xo, f"{robot} {dict(tuning)} warm tick {tick}", False)


@pytest.mark.parametrize("robot,tuning", CASES, ids=CASE_IDS)
def test_envs_are_independent(gpu, robot, tuning):
    """Envs 0-4 alone (a partial wavefront) and env 0 alone are bitwise their rows of the batch."""
    d, p, full = ec.inputs(robot), ec.params(robot), solved(robot, tuning)
    for n in (5, 1):
        part = solve(robot, tuning, d, p, rows=slice(0, n))
        assert part.tau.shape[0] == n
        assert_bitwise(part, full, (robot, n), rows_b=slice(0, n))


@pytest.mark.parametrize("what", ["u_lb>u_ub", "mu=nan", "w_pos=nan"])
@pytest.mark.parametrize("robot,tuning", CASES, ids=CASE_IDS)
def test_invalid_env_is_numerical_and_the_others_untouched(gpu, robot, tuning, what):
    """One env with an invalid parameter: it returns OSC_SOLVE_NUMERICAL with NaN outputs (an
    input-validation path: the call completes normally); the other 60 are bitwise the clean
    batch's."""
    bad = 17
    p = {k: v.copy() for k, v in ec.params(robot).items()}
    if what == "u_lb>u_ub":
        p["u_lb"][bad, 2] = p["u_ub"][bad, 2] + 1.0
    elif what == "mu=nan":
        p["mu"][bad] = np.nan
    else:
        p["w_pos"][bad, 1] = np.nan
    res, clean = solve(robot, tuning, ec.inputs(robot), p), solved(robot, tuning)
    assert int(res.status[bad]) == NUMERICAL
    assert torch.isnan(res.tau[bad]).all()
    others = torch.arange(ec.NENV, device=res.tau.device) != bad
    assert (res.status[others] == 0).all()
    assert_bitwise(res, clean, (robot, what), rows_a=others, rows_b=others)


def test_refusals(gpu):
    from osc_amd import _lib
    from osc_amd.autograd import solve_differentiable
    from osc_amd.solver import EnvParams, OSCBatchSolver, tick_multi_into
    blk = env_block(ec.params(WALTER))
    d = ec.inputs(WALTER)
    from test_gpu_wheels import NOSLIP_YAML
    wheels = OSCBatchSolver("walter_sr_wheels", NOSLIP_YAML)
    assert wheels.wheels
    for s in (wheels, OSCBatchSolver(WALTER, tuning={"refine_steps": 0})):
        args = s.prepare(**d)
        out = s.alloc_outputs(ec.NENV, want_x=True)
        warm = s.alloc_warm_state(ec.NENV)
        calls = [lambda: s.solve_into(out, *args, env_params=blk),
                 lambda: s.solve_warm_into(out, warm, *args, env_params=blk),
                 lambda: s.assemble_into(out, *args, env_params=blk),
                 lambda: s.solve_assembled_into(out, args[5], env_params=blk),
                 lambda: s.solve_assembled_warm_into(out, warm, args[5], env_params=blk)]
        for call in calls:
            with pytest.raises(_lib.OSCError) as err:
                call()
            assert err.value.code == 1          # OSC_ERR_INVALID_ARGUMENT
    s = solver(WALTER)
    with pytest.raises(NotImplementedError):
        solve_differentiable(s, *s.prepare(**d), env_params=blk)
    with pytest.raises(NotImplementedError):
        tick_multi_into([], env_params=blk)
    with pytest.raises(ValueError):           # a wrong shape: before any launch
        s.solve(**d, env_params=EnvParams(mu=torch.ones(ec.NENV + 1, dtype=torch.float64)))
