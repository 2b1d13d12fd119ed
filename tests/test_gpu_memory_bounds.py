"""Guard-band tests: where the kernels touch memory (tests/guard.py holds the helper).

Every case hands the entry point its outputs and caller-supplied scratch as guarded payloads of
EXACTLY the byte size the ABI reports, synchronises, and checks three properties:

  guards         no guard byte around any output, scratch buffer or input changed (no store lands
                 outside the caller's arrays), every input is bitwise what it was, and every
                 output is bitwise the same call's made the ordinary way (alloc_outputs /
                 kb.alloc tensors, a freshly created solver);
  dirty scratch  the call runs three times, its whole workspace payload holding 0x00 bytes, 0xFF
                 bytes (NaN as a double, -1 as an int32) and the contents a solve of another
                 batch of the same size left behind: the outputs are bitwise the same;
  dirty inputs   the inputs sit once between 0x00 and once between 0xFF guards (a load past the
                 last env's rows that reaches arithmetic shows up as a difference).
The three runs of a case are (inputs between 0x00, workspace 0x00), (0xFF, 0xFF) and (0x00,
left-over contents).  Solve entries at nenv <= 5 are also held to the exact oracle
(tests/test_gpu_parity.py's NORM_ACH / ELEM_ACH, tests/test_gpu_wheels.py's WHEEL_* with wheel rows).
Batches: nenv in {1, 3, 4, 5, 61} -- a lone env, a partial wavefront, exactly one, one plus one
env, the usual ragged batch -- generate(robot, nenv, SEED_BASE + 9400, "tumbling", "bernoulli"),
joint states from random_states.

Entry points covered (G = guards, S = dirty scratch, I = dirty inputs):
  osc_batch_solve / _solve_ex (cold; duals; NULL x / status / iters)          G S I   Go2, WaLTER,
  osc_batch_assemble(_ex) + osc_batch_solve_assembled                         G S I   wheel rows;
  osc_batch_solve_warm(_ex), two ticks, warm state exactly                    G S I   one-wave and
      osc_warm_state_bytes                                                            two-wave
  osc_batch_solve_env, osc_batch_solve_warm_env                               G S I   kernels
  lockstep compaction (park area, slot list, counter), 16,387 / 16,390 envs   G S I
  osc_batch_solve_multi, osc_batch_tick_multi (cold, warm, joint states)      G S I
  osc_batch_kinematics (with / without site_xpos), osc_batch_kinematics_pair,
      osc_state_to_qpos, osc_tumbling_targets, osc_contact_mask_from_contacts G   I   (no scratch)
  osc_batch_solve_qpos(_warm), workspace exactly osc_qpos_workspace_bytes     G S I
  osc_batch_integrate (with / without status and bad_ticks)                   G   I
  osc_batch_rollout, 3 ticks with histories, osc_rollout_workspace_bytes      G S I
  osc_batch_solve_backward, _backward_data, _backward_env, every gradient
      together and each alone, one env poisoned (NaN in M)                    G   I   (workspace:
                                                                                      read only)
  alignment contract at nenv = 5: outputs at the weakest alignment the headers state, refusal of
  each misaligned 16-byte pointer and of each buffer 16 bytes too small, outputs untouched.

Two cases show on the device that these checks can fail (tests/test_guard_helper.py shows it on
the host): an output one env short of the batch puts a kernel's own store into its back guard,
an input one env short makes the results follow the guard's fill.

Left out on purpose: the host-fed entries (csrc/osc_host_feed.cpp own their pinned buffers: there
is nothing of the caller's to guard) and the stream-ordered scratch path (workspace = NULL: the
library's own hipMallocAsync block cannot be guarded from outside).  What a guard cannot see: a
stray access further from the array than the guard's length (tests/guard.py states the rule).

Every integer in the workspace tail is written before it is read -- the reading the dirty-scratch
runs rest on (a garbage slot index would be an out-of-bounds access, so this was read first):
  status scratch (int32 per env after the reduced QPs; used when the caller's status is NULL and
      the call is warm, has wheel rows or fuses the refinement: launch_t, csrc/osc_api.hip): every
      valid env's entry is STORED by the first interior-point pass (ipm_block's output section,
      `if (gstatus) gstatus[env] = st`, csrc/osc_ipm.hpp; with compaction by the park pass for the
      envs that finish in it and by the resume pass for the parked ones).  It is only READ by the
      fix-up pass (`redo = ... gstatus[env] != OSC_SOLVE_OK`, same file), which runs after that
      store -- in the same launch behind a workgroup fence (osc_ipm_kernel, flags & 4) or in a
      later launch -- and by osc_gi_kernel (csrc/osc_gi.hip, `if (gstatus[env] == OSC_SOLVE_OK)
      return`), launched after the interior point (launch_gi).  osc_refine_kernel takes the env's
      status from the W_SOL hand-off block of the reduced QP, which the interior point wrote, and
      only stores to gstatus.  The dual kernels (csrc/osc_dual_body.hpp) do not touch it.
  counter (*PA.count): zeroed by hipMemsetAsync in launch_ipm before the park pass, incremented
      by the park pass's atomicAdd, read by the resume pass (`cnt = *PA.count`).
  slot list (PA.list): entry `slot` is stored by the park pass (`PA.list[slot] = env`) for every
      slot the counter handed out; the resume pass reads entries below the counter only
      (`PA.list[valid ? env_raw : cnt - 1]`, a wave past the counter returns before that).
  park area: slot `slot`'s doubles are stored by the park pass next to the list entry and read by
      the resume pass's resume_state() for slots below the counter.
  Spare rows of a ragged wavefront start `done` (`done = !valid`), so they never take a slot.
The warm state is not dirtied: its contract is zero-filled or valid.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import env_params_cases as ec
from guard import assert_guards_intact, guard_damage, guarded, guarded_like
from osc_amd import _lib
from osc_amd.synth import (SEED_BASE, WALTER_WHEEL_DOFS, WHEEL_RADIUS, generate,
                           wheel_directions)
from osc_qp import WheelRows, build_qp, load_model, torque
from qp_exact import solve_exact
from rollout_ref import DT
from test_gpu_parity import ELEM_ACH, NORM_ACH, _rel_errors
from test_gpu_wheels import NOSLIP_YAML, WHEEL_ELEM, WHEEL_NORM
from test_producers import _tumbling_state

pytestmark = pytest.mark.gpu

GO2, WALTER, WHEELS = "unitree_go2", "walter_sr", "walter_sr_wheels"
NENVS = (1, 3, 4, 5, 61)
SEED = SEED_BASE + 9400
ONE_WAVE, TWO_WAVE = 100000000, 0
INVALID = 1                      # OSC_ERR_INVALID_ARGUMENT
NAMES = ("M", "C", "J", "b", "T", "mask")
FIELDS = ("tau", "x", "y", "status", "iters")
F64, I32 = torch.float64, torch.int32
# the three runs of a case: (fill around the inputs, workspace contents)
RUNS = ((0x00, 0x00), (0xFF, 0xFF), (0x00, "left"))


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """These tests are built so that no overrun within a guard's reach leaves its allocation; should
    the device report an error all the same, nothing further is launched on it."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, no further test is run: {e}", returncode=3)


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------

def same(a, b):
    """bitwise equality (NaNs and signed zeros included)"""
    return (a.shape == b.shape and a.dtype == b.dtype and
            torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))


def assert_same(got, ref, what):
    assert same(got, ref), f"{what}: not bitwise the ordinary call's"


class Tracker:
    """The guarded tensors of one run: inputs (copied between guards of `pad`), outputs and
    in/out buffers (guards 0xA5 / 0x5A: neither byte pattern is a result)."""

    def __init__(self, device, pad):
        self.dev, self.pad = device, pad
        self.fill = 0xA5 if pad == 0 else 0x5A
        self.ins, self.outs = [], []

    def _dev(self, src):
        if isinstance(src, np.ndarray):
            src = torch.from_numpy(np.ascontiguousarray(src))
        return src.to(self.dev)

    def inp(self, name, src, off=0):
        if src is None:
            return None
        t = guarded_like(self._dev(src), self.pad, offset_bytes=off)
        assert t.data_ptr() % 16 == off
        self.ins.append((name, t, t.clone()))
        return t

    def out(self, name, shape, dtype, off=0, env_bytes=None, zero=False):
        t = guarded(shape, dtype, self.dev, fill=self.fill, offset_bytes=off, env_bytes=env_bytes)
        assert t.data_ptr() % 16 == off
        if zero:
            t.zero_()
        self.outs.append((name, t))
        return t

    def inout(self, name, src):
        t = guarded_like(self._dev(src), self.fill)
        self.outs.append((name, t))
        return t

    def check(self):
        torch.cuda.synchronize()
        for name, t in self.outs:
            assert_guards_intact(t, name)
        for name, t, before in self.ins:
            assert_guards_intact(t, "input " + name)
            assert same(t, before), f"input {name} was modified"

    def untouched(self):
        """after a refused call: no byte of any output allocation, payload included, changed"""
        torch.cuda.synchronize()
        for name, t in self.outs:
            assert bool((t._guard.base == t._guard.fill).all()), f"{name} written by a refused call"
        for name, t, before in self.ins:
            assert same(t, before), f"input {name} was modified"


def set_bytes(t, mode, left=None):
    """the whole payload of a scratch buffer: one byte value, or a copy of `left`"""
    if isinstance(mode, str):
        assert left.numel() == t.numel()
        t.copy_(left)
    else:
        t.reshape(-1).view(torch.uint8).fill_(mode)


def new_solver(robot, sbm=None, **tuning):
    from osc_amd.solver import OSCBatchSolver
    if sbm is not None:
        tuning["small_batch_max"] = sbm
    if robot == WHEELS:
        return OSCBatchSolver(WHEELS, NOSLIP_YAML, tuning=tuning or None)
    return OSCBatchSolver(robot, tuning=tuning or None)


@functools.lru_cache(maxsize=None)
def kin(robot):
    from osc_amd.kinematics import KinematicsBatch
    return KinematicsBatch(robot)


def _wheel():
    return WheelRows(dof=np.array(WALTER_WHEEL_DOFS), radius=np.full(8, WHEEL_RADIUS))


@functools.lru_cache(maxsize=None)
def batch(robot, nenv, k=0, scenario="tumbling", seed=None):
    """(inputs dict, wheel directions or None), left unchanged by the tests"""
    seed = SEED + 100 * k if seed is None else seed + k
    d = generate(robot, nenv, seed, scenario, "bernoulli")
    wd = None
    if robot == WHEELS:
        wd = wheel_directions(WHEELS, d, _wheel().dof, _wheel().radius, seed + 1)
    return d, wd


@functools.lru_cache(maxsize=None)
def states(robot, nenv, k=0):
    from osc_amd.kinematics import load_tree, random_states
    return random_states(load_tree(robot), nenv, SEED + 7 + 100 * k)


@functools.lru_cache(maxsize=None)
def env_draw(robot, nenv):
    return ec.draw_params(robot, np.random.default_rng(SEED + 3), nenv)


def env_block(robot, nenv, tr=None):
    from osc_amd.solver import EnvParams
    p = env_draw(robot, nenv)
    put = (lambda k: torch.from_numpy(p[k]).cuda()) if tr is None else \
          (lambda k: tr.inp("env_params." + k, p[k]))
    return EnvParams(**{k: put(k) for k in ec.FIELDS})


@functools.lru_cache(maxsize=None)
def oracle_tau(robot, nenv, env=False):
    d, wd = batch(robot, nenv)
    ref = []
    for e in range(nenv):
        args = [d[k][e] for k in NAMES]
        if env:
            model = ec.env_model(robot, env_draw(robot, nenv), e)
            qp = build_qp(model, *args)
        elif robot == WHEELS:
            model = load_model(WHEELS)
            qp = build_qp(model, *args, _wheel(), wd[e])
        else:
            model = load_model(robot)
            qp = build_qp(model, *args)
        ref.append(torque(model, solve_exact(model, qp, *args[:3]).x))
    return np.array(ref)


def check_oracle(robot, nenv, shot, env=False, where=""):
    if nenv > 5:
        return
    assert (shot["status"].cpu().numpy() == 0).all(), (where, shot["status"])
    nw, el = _rel_errors(shot["tau"].cpu().numpy(), oracle_tau(robot, nenv, env))
    print(f"\n{where} {robot} nenv={nenv}: vs oracle normwise {nw.max():.2e} elementwise {el.max():.2e}")
    norm, elem = (WHEEL_NORM, WHEEL_ELEM) if robot == WHEELS else (NORM_ACH, ELEM_ACH)
    assert nw.max() <= norm and el.max() <= elem, (where, nw.max(), el.max())


def size_of(fn, *args):
    nb = ctypes.c_size_t()
    assert fn(*args, ctypes.byref(nb)) == 0
    return nb.value


def ws_bytes(s, nenv):
    return size_of(_lib.lib().osc_workspace_bytes, s._h, nenv)


def warm_bytes(s, nenv):
    return size_of(_lib.lib().osc_warm_state_bytes, s._h, nenv)


def exact_buffer(tr, name, nbytes, nenv, off=0, zero=False):
    """a guarded float64 buffer of exactly `nbytes` (never rounded up)"""
    assert nbytes % 8 == 0 and nbytes > 0
    return tr.out(name, (nbytes // 8,), F64, off=off, env_bytes=-(-nbytes // nenv), zero=zero)


def guarded_result(tr, s, nenv, want_y=False, offs=None, null=(), ws=True, tag=""):
    """SolveResult whose every tensor is a guarded payload; the workspace exactly
    osc_workspace_bytes.  offs: name -> payload offset (8 / 4); null: outputs passed as NULL."""
    from osc_amd.solver import SolveResult
    offs, d = offs or {}, s.dims
    mk = lambda n, shape, dt: None if n in null else tr.out(tag + n, shape, dt, off=offs.get(n, 0))
    nb = ws_bytes(s, nenv)
    assert nb % 16 == 0
    return SolveResult(
        tau=mk("tau", (nenv, d["nu"]), F64), x=mk("x", (nenv, d["n"]), F64),
        status=mk("status", (nenv,), I32), iters=mk("iters", (nenv,), I32),
        workspace=exact_buffer(tr, tag + "workspace", nb, nenv, off=offs.get("workspace", 0))
        if ws else None,
        y=mk("y", (nenv, s.dual_rows), F64) if want_y else None)


def shot_of(out, **extra):
    torch.cuda.synchronize()
    sh = {k: getattr(out, k).clone() for k in FIELDS if getattr(out, k) is not None}
    sh.update({k: v.clone() for k, v in extra.items() if v is not None})
    return sh


def compare_shots(got, ref, where):
    assert len(got) == len(ref)
    for tick, (g, r) in enumerate(zip(got, ref)):
        for k in g:
            assert_same(g[k], r[k], f"{where} tick {tick} {k}")


# ---------------------------------------------------------------------------------------------
# solve family
# ---------------------------------------------------------------------------------------------

def run_solve(kind, s, out, a, wd=None, ep=None, warm=None):
    """One case's launches -> the outputs after each tick (clones)."""
    if kind == "cold":
        s.solve_into(out, *a, wheel_dir=wd, env_params=ep)
        return [shot_of(out)]
    if kind == "split":
        s.assemble_into(out, *a, wheel_dir=wd, env_params=ep)
        s.solve_assembled_into(out, a[5], env_params=ep)
        return [shot_of(out)]
    assert kind == "warm"
    shots = []
    for _ in range(2):           # the second tick starts from the first's solution
        s.solve_warm_into(out, warm, *a, wheel_dir=wd, env_params=ep)
        shots.append(shot_of(out, warm=warm))
    return shots


def leftover_workspace(s, robot, nenv):
    """the workspace a solve of another batch of the same size leaves behind"""
    d, wd = batch(robot, nenv, 1)
    o = s.alloc_outputs(nenv, want_x=True)
    s.solve_into(o, *s.prepare(**d), wheel_dir=None if wd is None else torch.from_numpy(wd).cuda())
    torch.cuda.synchronize()
    return o.workspace


def check_solve(robot, nenv, sbm, kind, want_y=False, env=False, offs=None, null=(), oracle=True):
    d, wd_np = batch(robot, nenv)
    s0 = new_solver(robot, sbm)                       # the ordinary call: a fresh solver,
    a0 = s0.prepare(**d)                              # unguarded tensors
    wd0 = None if wd_np is None else torch.from_numpy(wd_np).cuda()
    o0 = s0.alloc_outputs(nenv, want_x=True, want_y=want_y)
    ref = run_solve(kind, s0, o0, a0, wd0, env_block(robot, nenv) if env else None,
                    s0.alloc_warm_state(nenv) if kind == "warm" else None)
    left = leftover_workspace(s0, robot, nenv)
    s = new_solver(robot, sbm)
    where = f"{kind}{' env' if env else ''}{' y' if want_y else ''} sbm={sbm}"
    for pad, wsmode in RUNS:
        tr = Tracker(s.device, pad)
        a = tuple(tr.inp(n, t) for n, t in zip(NAMES, a0))
        wd = tr.inp("wheel_dir", wd0)
        ep = env_block(robot, nenv, tr) if env else None
        out = guarded_result(tr, s, nenv, want_y, offs, null)
        set_bytes(out.workspace, wsmode, left)
        warm = None
        if kind == "warm":
            warm = exact_buffer(tr, "warm_state", warm_bytes(s, nenv), nenv,
                                off=(offs or {}).get("warm_state", 0), zero=True)
        got = run_solve(kind, s, out, a, wd, ep, warm)
        tr.check()
        compare_shots(got, ref, f"{where} inputs in {pad:#04x} workspace {wsmode}")
    if oracle:
        for tick, r in enumerate(ref):
            check_oracle(robot, nenv, r, env, f"{where} tick {tick}")


SOLVE_CASES = [(r, n, sbm) for r in (GO2, WALTER) for n in NENVS for sbm in (ONE_WAVE, TWO_WAVE)] + \
              [(WHEELS, n, ONE_WAVE) for n in NENVS]     # (wheel rows: the one-wave kernel only)
PLAIN_CASES = [c for c in SOLVE_CASES if c[0] != WHEELS]


@pytest.mark.parametrize("robot,nenv,sbm", SOLVE_CASES)
def test_cold_solve(gpu, robot, nenv, sbm):
    check_solve(robot, nenv, sbm, "cold")


@pytest.mark.parametrize("robot,nenv,sbm", SOLVE_CASES)
def test_assemble_then_solve_assembled(gpu, robot, nenv, sbm):
    check_solve(robot, nenv, sbm, "split")


@pytest.mark.parametrize("robot,nenv,sbm", SOLVE_CASES)
def test_two_warm_ticks(gpu, robot, nenv, sbm):
    """sbm = 0 without wheel rows: the warm pass, osc_refine_kernel, then the fix-up launch."""
    check_solve(robot, nenv, sbm, "warm")


@pytest.mark.parametrize("robot,nenv,sbm", SOLVE_CASES)
def test_cold_solve_with_duals(gpu, robot, nenv, sbm):
    check_solve(robot, nenv, sbm, "cold", want_y=True)


@pytest.mark.parametrize("kind", ["cold", "split", "warm"])
@pytest.mark.parametrize("robot,nenv,sbm", PLAIN_CASES)
def test_env_entries(gpu, robot, nenv, sbm, kind):
    check_solve(robot, nenv, sbm, kind, env=True)


@pytest.mark.parametrize("null", [("x",), ("status",), ("iters",), ("x", "status", "iters")],
                         ids=lambda n: "no_" + "_".join(n))
@pytest.mark.parametrize("kind", ["cold", "warm"])
@pytest.mark.parametrize("robot,nenv,sbm", SOLVE_CASES)
def test_nullable_outputs(gpu, robot, nenv, sbm, kind, null):
    """x, status, iters NULL in turn and together: tau (and whatever else is returned) bitwise
    unchanged.  status = NULL sends the fix-up pass (and the wheel rows' fallback) to the status
    scratch at the end of the workspace."""
    check_solve(robot, nenv, sbm, kind, null=null, oracle=False)


@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_guards_see_a_kernel_store_past_the_payload(gpu, robot):
    """The detector end to end, on the device: x and status payloads ONE ENV SHORT of the batch
    the call is told about, so the kernel's (legitimate) stores for the last env land at the
    start of the back guards -- inside the same allocations, as everywhere in this file.
    assert_guards_intact reports exactly that env's row."""
    nenv = 5
    s = new_solver(robot)
    a = s.prepare(**batch(robot, nenv)[0])
    tr = Tracker(s.device, 0x00)
    out = guarded_result(tr, s, nenv, null=("x", "status"))
    out.x = tr.out("x", (nenv - 1, s.dims["n"]), F64)
    out.status = tr.out("status", (nenv - 1,), I32)
    s.solve_into(out, *a)
    torch.cuda.synchronize()
    row = s.dims["n"] * 8
    first, last = guard_damage(out.x)           # (a byte of x that happens to be 0xA5: unseen)
    assert 4 * row <= first < 4 * row + 8 and 5 * row - 8 <= last < 5 * row, (first, last, row)
    assert guard_damage(out.status) == (16, 19)     # status 0 = four 0x00 bytes
    with pytest.raises(AssertionError, match=r"x: guard bytes changed"):
        assert_guards_intact(out.x, "x")
    for k in ("tau", "iters", "workspace"):
        assert_guards_intact(getattr(out, k), k)


@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_input_surroundings_show_in_the_results_when_read(gpu, robot):
    """The same for the input side: T one env short, so the last env's targets are read from the
    back guard (inside T's allocation).  Its torques then differ between 0x00 and 0xFF guards --
    what the dirty-surroundings comparison of every case above would see -- and the other envs'
    do not."""
    nenv = 5
    s = new_solver(robot)
    a = s.prepare(**batch(robot, nenv)[0])
    taus = []
    for pad in (0x00, 0xFF):
        tr = Tracker(s.device, pad)
        out = guarded_result(tr, s, nenv)
        s.solve_into(out, *a[:4], tr.inp("T", a[4][:nenv - 1]), a[5])
        tr.check()
        taus.append(out.tau.clone())
    assert same(taus[0][:nenv - 1], taus[1][:nenv - 1])
    assert not same(taus[0][nenv - 1], taus[1][nenv - 1])


# ---------------------------------------------------------------------------------------------
# lockstep compaction: the park area, slot list and counter only exist here
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("robot,nenv,park", [(WALTER, 16387, None), (GO2, 16390, 12)])
def test_compaction(gpu, robot, nenv, park):
    """tests/test_gpu_stages.py's two ragged compaction batches under guards: bitwise the
    park_it = 0 result whatever the park area, slot list and counter held before."""
    tune = {} if park is None else {"park_it": park}
    d = generate(robot, nenv, SEED_BASE + 34, "standing", "bernoulli")
    s0 = new_solver(robot, park_it=0)
    a0 = s0.prepare(**d)
    o0 = s0.alloc_outputs(nenv, want_x=True)
    s0.solve_into(o0, *a0)
    ref = [shot_of(o0)]
    it = ref[0]["iters"].cpu().numpy()
    assert (it > (park or 16)).any() and (it <= (park or 16)).any()     # both passes have work
    s1 = new_solver(robot, **tune)                      # left-over: another batch, compaction on
    o1 = s1.alloc_outputs(nenv, want_x=True)
    s1.solve_into(o1, *s1.prepare(**generate(robot, nenv, SEED + 1, "standing", "bernoulli")))
    torch.cuda.synchronize()
    lay = ws_bytes(s1, nenv)
    assert lay > size_of(_lib.lib().osc_workspace_env_bytes, s1._h) * nenv + 4 * nenv   # (park area)
    s = new_solver(robot, **tune)
    for pad, wsmode in RUNS:
        tr = Tracker(s.device, pad)
        a = tuple(tr.inp(n, t) for n, t in zip(NAMES, a0))
        out = guarded_result(tr, s, nenv)
        set_bytes(out.workspace, wsmode, o1.workspace)
        s.solve_into(out, *a)
        got = [shot_of(out)]
        tr.check()
        compare_shots(got, ref, f"compaction inputs in {pad:#04x} workspace {wsmode}")
        del tr, a, out


# ---------------------------------------------------------------------------------------------
# two-model calls: a partial wavefront on both sides of the model boundary in the shared grid
# ---------------------------------------------------------------------------------------------

PAIRS = [(5, 3), (1, 61)]          # (WaLTER envs, Go2 envs)


def qpos_ws_bytes(s, robot, nenv):
    return kin(robot).workspace_bytes(s, nenv)


@pytest.mark.parametrize("api", ["solve_multi", "tick_cold", "tick_warm", "tick_joint_states"])
@pytest.mark.parametrize("nw,ng", PAIRS)
def test_two_model_calls(gpu, nw, ng, api):
    from osc_amd.solver import TickJob, solve_multi_into, tick_multi_into
    robots, n = (WALTER, GO2), {WALTER: nw, GO2: ng}
    joint = api == "tick_joint_states"
    ticks = 2 if api == "tick_warm" else 1

    def inputs_of(s, r, put):
        d, _ = batch(r, n[r])
        a = s.prepare(**d)
        if not joint:
            return tuple(put(nm, t) for nm, t in zip(NAMES, a))
        qp, qv = states(r, n[r])
        return (put("qpos", torch.from_numpy(qp).cuda()), put("qvel", torch.from_numpy(qv).cuda()),
                put("T", a[4]), put("mask", a[5]))

    def launch(sol, outs, ins, warm, wss):
        shots = []
        for _ in range(ticks):
            if api == "solve_multi":
                solve_multi_into([(sol[r], outs[r], ins[r]) for r in robots])
            else:
                tick_multi_into([TickJob(sol[r], outs[r], ins[r], kin=kin(r) if joint else None,
                                         warm=warm[r], workspace=wss[r]) for r in robots])
            torch.cuda.synchronize()
            shots.append({f"{r}.{k}": v for r in robots
                          for k, v in shot_of(outs[r], warm=warm[r]).items()})
        return shots

    s0 = {r: new_solver(r) for r in robots}
    o0 = {r: s0[r].alloc_outputs(n[r], want_x=True) for r in robots}
    w0 = {r: s0[r].alloc_warm_state(n[r]) if api == "tick_warm" else None for r in robots}
    q0 = {r: torch.empty(qpos_ws_bytes(s0[r], r, n[r]) // 8, dtype=F64, device="cuda") if joint
          else None for r in robots}
    ref = launch(s0, o0, {r: inputs_of(s0[r], r, lambda nm, t: t) for r in robots}, w0, q0)
    # left-over workspaces: a solve of another batch of the same size
    left = {}
    for r in robots:
        if joint:
            left[r] = torch.empty_like(q0[r])
            q1, v1 = (torch.from_numpy(a).cuda() for a in states(r, n[r], 1))
            kin(r).solve_into(s0[r], s0[r].alloc_outputs(n[r]), q1, v1,
                              *s0[r].prepare(**batch(r, n[r], 1)[0])[4:], left[r])
            torch.cuda.synchronize()
        else:
            left[r] = leftover_workspace(s0[r], r, n[r])
    s = {r: new_solver(r) for r in robots}
    for pad, wsmode in RUNS:
        tr = Tracker(s[GO2].device, pad)
        ins = {r: inputs_of(s[r], r, lambda nm, t, r=r: tr.inp(f"{r}.{nm}", t)) for r in robots}
        outs = {r: guarded_result(tr, s[r], n[r], ws=not joint, tag=r + ".") for r in robots}
        warm = {r: exact_buffer(tr, r + ".warm_state", warm_bytes(s[r], n[r]), n[r], zero=True)
                if api == "tick_warm" else None for r in robots}
        wss = {r: exact_buffer(tr, r + ".qpos_workspace", qpos_ws_bytes(s[r], r, n[r]), n[r])
               if joint else None for r in robots}
        for r in robots:
            set_bytes(wss[r] if joint else outs[r].workspace, wsmode, left[r])
        got = launch(s, outs, ins, warm, wss)
        tr.check()
        compare_shots(got, ref, f"{api} inputs in {pad:#04x} workspace {wsmode}")
    if not joint:
        for r in robots:
            last = {k.split(".", 1)[1]: v for k, v in ref[-1].items() if k.startswith(r + ".")}
            check_oracle(r, n[r], last, where=api)


# ---------------------------------------------------------------------------------------------
# kinematics front end
# ---------------------------------------------------------------------------------------------

def guarded_kin_outputs(tr, kb, nenv, sites, tag=""):
    from osc_amd.kinematics import KinOutputs
    nv, s6 = kb.nv, 6 * kb.ns
    return KinOutputs(tr.out(tag + "M", (nenv, nv, nv), F64), tr.out(tag + "C", (nenv, nv), F64),
                      tr.out(tag + "J", (nenv, s6, nv), F64), tr.out(tag + "b", (nenv, s6), F64),
                      tr.out(tag + "site_xpos", (nenv, kb.ns, 3), F64) if sites else None)


KIN_FIELDS = ("M", "C", "J", "b", "site_xpos")


def kin_shot(o, tag=""):
    torch.cuda.synchronize()
    return {tag + k: getattr(o, k).clone() for k in KIN_FIELDS if getattr(o, k) is not None}


@pytest.mark.parametrize("sites", [False, True], ids=["no_site_xpos", "site_xpos"])
@pytest.mark.parametrize("nenv", NENVS)
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_kinematics(gpu, robot, nenv, sites):
    """osc_batch_kinematics (Go2: nq = 19 is odd, every second env's qpos row is only 8-byte
    aligned)."""
    kb = kin(robot)
    qp, qv = (torch.from_numpy(a).cuda() for a in states(robot, nenv))
    ref = [kin_shot(kb.compute_into(kb.alloc(nenv, sites), qp, qv))]
    for pad in (0x00, 0xFF):
        tr = Tracker(kb.device, pad)
        out = guarded_kin_outputs(tr, kb, nenv, sites)
        kb.compute_into(out, tr.inp("qpos", qp), tr.inp("qvel", qv))
        got = [kin_shot(out)]
        tr.check()
        compare_shots(got, ref, f"kinematics inputs in {pad:#04x}")


@pytest.mark.parametrize("nw,ng", PAIRS)
def test_kinematics_pair(gpu, nw, ng):
    from osc_amd.kinematics import kinematics_pair_into
    n = {WALTER: nw, GO2: ng}
    st = {r: tuple(torch.from_numpy(a).cuda() for a in states(r, n[r])) for r in n}
    o0 = {r: kin(r).alloc(n[r]) for r in n}
    kinematics_pair_into(kin(WALTER), o0[WALTER], *st[WALTER], kin(GO2), o0[GO2], *st[GO2])
    ref = [{**kin_shot(o0[WALTER], "w."), **kin_shot(o0[GO2], "g.")}]
    for r in n:                                 # (documented: each model's are compute_into's)
        solo = kin_shot(kin(r).compute_into(kin(r).alloc(n[r]), *st[r]), "w." if r == WALTER else "g.")
        for k, v in solo.items():
            assert_same(ref[0][k], v, "pair vs solo " + k)
    for pad in (0x00, 0xFF):
        tr = Tracker(kin(GO2).device, pad)
        out = {r: guarded_kin_outputs(tr, kin(r), n[r], False, r + ".") for r in n}
        gi = {r: tuple(tr.inp(f"{r}.{nm}", t) for nm, t in zip(("qpos", "qvel"), st[r])) for r in n}
        kinematics_pair_into(kin(WALTER), out[WALTER], *gi[WALTER], kin(GO2), out[GO2], *gi[GO2])
        got = [{**kin_shot(out[WALTER], "w."), **kin_shot(out[GO2], "g.")}]
        tr.check()
        compare_shots(got, ref, f"kinematics pair inputs in {pad:#04x}")


@pytest.mark.parametrize("nenv", NENVS)
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_state_to_qpos(gpu, robot, nenv):
    kb = kin(robot)
    nu = kb.nq - 7
    rng = np.random.default_rng(SEED + 11)
    src = [rng.standard_normal((nenv, k)) for k in (4, 3, 3, nu, nu)]
    names = ("body_rotation", "linear_body_velocity", "angular_body_velocity", "motor_position",
             "motor_velocity")
    q0, v0 = kb.state_to_qpos(*src)
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for pad in (0x00, 0xFF):
        tr = Tracker(kb.device, pad)
        ins = [tr.inp(nm, a) for nm, a in zip(names, src)]
        qpos, qvel = tr.out("qpos", (nenv, kb.nq), F64), tr.out("qvel", (nenv, kb.nv), F64)
        rc = _lib.lib().osc_state_to_qpos(nenv, nu, *[p(t) for t in ins], p(qpos), p(qvel),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        tr.check()
        assert_same(qpos, q0, "qpos")
        assert_same(qvel, v0, "qvel")


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("robot,nenv,sbm", PLAIN_CASES)
def test_solve_from_joint_states(gpu, robot, nenv, sbm, warm):
    """kb.solve_into / kb.solve_warm_into (two ticks), the workspace exactly
    osc_qpos_workspace_bytes: [M | C | J | b | the solve's workspace]."""
    kb = kin(robot)
    d, _ = batch(robot, nenv)
    qp, qv = (torch.from_numpy(a).cuda() for a in states(robot, nenv))

    def launch(s, out, ins, wst, ws):
        shots = []
        for _ in range(2 if warm else 1):
            if warm:
                kb.solve_warm_into(s, out, wst, *ins, ws)
            else:
                kb.solve_into(s, out, *ins, ws)
            shots.append(shot_of(out, warm=wst))
        return shots

    s0 = new_solver(robot, sbm)
    T0, m0 = s0.prepare(**d)[4:]
    nb = kb.workspace_bytes(s0, nenv)
    ws0 = torch.empty(nb // 8, dtype=F64, device="cuda")
    ref = launch(s0, s0.alloc_outputs(nenv, want_x=True), (qp, qv, T0, m0),
                 s0.alloc_warm_state(nenv) if warm else None, ws0)
    left = torch.empty_like(ws0)                # another batch's left-overs
    q1, v1 = (torch.from_numpy(a).cuda() for a in states(robot, nenv, 1))
    kb.solve_into(s0, s0.alloc_outputs(nenv), q1, v1, *s0.prepare(**batch(robot, nenv, 1)[0])[4:], left)
    torch.cuda.synchronize()
    s = new_solver(robot, sbm)
    for pad, wsmode in RUNS:
        tr = Tracker(s.device, pad)
        ins = tuple(tr.inp(nm, t) for nm, t in zip(("qpos", "qvel", "T", "mask"), (qp, qv, T0, m0)))
        out = guarded_result(tr, s, nenv, ws=False)
        ws = exact_buffer(tr, "qpos_workspace", nb, nenv)
        set_bytes(ws, wsmode, left)
        wst = exact_buffer(tr, "warm_state", warm_bytes(s, nenv), nenv, zero=True) if warm else None
        got = launch(s, out, ins, wst, ws)
        tr.check()
        compare_shots(got, ref, f"qpos solve inputs in {pad:#04x} workspace {wsmode}")


# ---------------------------------------------------------------------------------------------
# producers (tests/test_producers.py's inputs at the tail-logic batch sizes)
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nenv", NENVS)
def test_tumbling_targets(gpu, nenv):
    from osc_amd.producers import tumbling_params, tumbling_targets_into
    rng = np.random.default_rng(9)
    st = [_tumbling_state(rng) for _ in range(nenv)]
    t0 = rng.uniform(0, 1, nenv)
    t = t0 + rng.uniform(0.002, 0.5, nenv)
    src = [np.stack([s[i] for s in st]) for i in range(3)] + [t, t0] + \
          [np.stack([s[i] for s in st]) for i in (3, 4)]
    names = ("qpos", "qvel", "site_xpos", "t", "t0", "init_qpos", "init_site_xpos")
    params = tumbling_params(torso_lin_kp=2.0, torso_lin_kv=0.3, torso_ang_kp=3.0, torso_ang_kv=0.5)
    ref = torch.empty((nenv, 17, 6), dtype=F64, device=gpu)
    tumbling_targets_into(ref, *[torch.from_numpy(a).to(gpu) for a in src], params)
    torch.cuda.synchronize()
    for pad in (0x00, 0xFF):
        tr = Tracker(gpu, pad)
        out = tr.out("T", (nenv, 17, 6), F64)
        tumbling_targets_into(out, *[tr.inp(nm, a) for nm, a in zip(names, src)], params)
        tr.check()
        assert_same(out, ref, f"tumbling targets inputs in {pad:#04x}")


@pytest.mark.parametrize("nenv", NENVS)
def test_contact_mask(gpu, nenv):
    from osc_amd.producers import contact_mask_into
    rng = np.random.default_rng(6)
    nc, max_con, ngeom = 8, 12, 30
    g2s = np.full(ngeom, -1, dtype=np.int32)
    g2s[rng.choice(ngeom, nc, replace=False)] = np.arange(nc)
    ncon = rng.integers(-1, max_con + 3, nenv).astype(np.int32)      # includes out-of-range
    pairs = rng.integers(-1, ngeom + 2, (nenv, max_con, 2)).astype(np.int32)
    ref = torch.empty((nenv, nc), dtype=F64, device=gpu)
    contact_mask_into(ref, *[torch.from_numpy(a).to(gpu) for a in (ncon, pairs, g2s)])
    torch.cuda.synchronize()
    for pad in (0x00, 0xFF):
        tr = Tracker(gpu, pad)
        out = tr.out("mask", (nenv, nc), F64)
        contact_mask_into(out, tr.inp("ncon", ncon), tr.inp("geom_pairs", pairs),
                          tr.inp("geom_to_site", g2s))
        tr.check()
        assert_same(out, ref, f"contact mask inputs in {pad:#04x}")


# ---------------------------------------------------------------------------------------------
# rollout
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extras", [False, True], ids=["plain", "status_bad_ticks"])
@pytest.mark.parametrize("nenv", NENVS)
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_integrate(gpu, robot, nenv, extras):
    kb = kin(robot)
    qp, qv = states(robot, nenv)
    rng = np.random.default_rng(SEED + 13)
    qacc = rng.standard_normal((nenv, kb.nv))
    status = np.zeros(nenv, dtype=np.int32)
    status[nenv // 2] = _lib.SOLVE_NUMERICAL          # one frozen env
    status[0] = _lib.SOLVE_MAX_ITER if nenv > 1 else status[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    r_qp, r_qv, r_bad = dev(qp), dev(qv), torch.zeros(nenv, dtype=I32, device=gpu)
    kb.integrate_into(r_qp, r_qv, dev(qacc), DT, status=dev(status) if extras else None,
                      bad_ticks=r_bad if extras else None)
    torch.cuda.synchronize()
    for pad in (0x00, 0xFF):
        tr = Tracker(gpu, pad)
        g_qp, g_qv = tr.inout("qpos", qp), tr.inout("qvel", qv)
        bad = tr.inout("bad_ticks", np.zeros(nenv, dtype=np.int32)) if extras else None
        kb.integrate_into(g_qp, g_qv, tr.inp("qacc", qacc), DT,
                          status=tr.inp("status", status) if extras else None, bad_ticks=bad)
        tr.check()
        assert_same(g_qp, r_qp, "qpos")
        assert_same(g_qv, r_qv, "qvel")
        if extras:
            assert_same(bad, r_bad, "bad_ticks")


HIST = ("qpos_hist", "qvel_hist", "tau_hist", "status_hist")


def rollout_raw(kb, s, nenv, nticks, T, mask, qpos, qvel, tau, bad, hist, ws, ws_nbytes):
    a = _lib.OscRolloutArgs()
    a.nticks, a.dt, a.flags = nticks, DT, _lib.ROLLOUT_WARM
    a.target_mode, a.T = _lib.ROLLOUT_TARGETS_HELD, T.data_ptr()
    a.contact_mask, a.qpos, a.qvel = mask.data_ptr(), qpos.data_ptr(), qvel.data_ptr()
    a.tau, a.bad_ticks = tau.data_ptr(), bad.data_ptr()
    for k in HIST:
        setattr(a, k, hist[k].data_ptr())
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_nbytes
    return _lib.lib().osc_batch_rollout(s._h, kb._h, nenv, ctypes.byref(a),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def guarded_rollout(tr, kb, s, nenv, nticks, qp, qv):
    d = s.dims
    hist = dict(qpos_hist=tr.out("qpos_hist", (nticks + 1, nenv, kb.nq), F64),
                qvel_hist=tr.out("qvel_hist", (nticks + 1, nenv, kb.nv), F64),
                tau_hist=tr.out("tau_hist", (nticks, nenv, d["nu"]), F64),
                status_hist=tr.out("status_hist", (nticks, nenv), I32))
    return (tr.inout("qpos", qp), tr.inout("qvel", qv), tr.out("tau", (nenv, d["nu"]), F64),
            tr.out("bad_ticks", (nenv,), I32), hist)


@pytest.mark.parametrize("nenv", NENVS)
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_rollout(gpu, robot, nenv):
    """osc_batch_rollout, 3 warm ticks with every history, held targets; final state, tau,
    bad_ticks and the histories guarded, the workspace exactly osc_rollout_workspace_bytes."""
    kb, nticks = kin(robot), 3
    d, _ = batch(robot, nenv)
    qp, qv = states(robot, nenv)
    s0 = new_solver(robot)
    ref = kb.rollout(s0, qp, qv, d["mask"], nticks, DT, T=d["T"], history=True)
    torch.cuda.synchronize()
    other = kb.rollout(s0, *states(robot, nenv, 1), batch(robot, nenv, 1)[0]["mask"], nticks, DT,
                       T=batch(robot, nenv, 1)[0]["T"])
    torch.cuda.synchronize()
    left = other._keep[-1]
    s = new_solver(robot)
    nb = kb.rollout_workspace_bytes(s, nenv, nticks)
    assert left.numel() * 8 == nb
    for pad, wsmode in RUNS:
        tr = Tracker(gpu, pad)
        qpos, qvel, tau, bad, hist = guarded_rollout(tr, kb, s, nenv, nticks, qp, qv)
        ws = exact_buffer(tr, "rollout_workspace", nb, nenv)
        set_bytes(ws, wsmode, left)
        rc = rollout_raw(kb, s, nenv, nticks, tr.inp("T", d["T"]), tr.inp("mask", d["mask"]), qpos,
                         qvel, tau, bad, hist, ws, nb)
        assert rc == 0
        tr.check()
        where = f"rollout inputs in {pad:#04x} workspace {wsmode}"
        for k, t in dict(qpos=qpos, qvel=qvel, tau=tau, bad_ticks=bad, **hist).items():
            assert_same(t, getattr(ref, k), f"{where} {k}")


# ---------------------------------------------------------------------------------------------
# backward passes
# ---------------------------------------------------------------------------------------------

DATA = ("M", "C", "J", "wrow", "T", "b")
BACKWARD_COMBOS = {
    "backward": [("T", "b"), ("T",), ("b",)],
    "backward_data": [DATA] + [(k,) for k in DATA],
    "backward_env": [DATA + ec.FIELDS] + [(k,) for k in DATA + ec.FIELDS],
}


def grad_shapes(s, n):
    from osc_amd.solver import EnvParams
    d = s.dims
    sh = dict(M=(n, d["nv"], d["nv"]), C=(n, d["nv"]), J=(n, d["s"], d["nv"]), wrow=(n, d["s"]),
              T=(n, d["ns"], 6), b=(n, d["s"]))
    sh.update(EnvParams().shapes(n, d))
    return sh


def run_backward(api, s, out, a, gx, g, ep=None, b=None, T=None):
    """one backward launch; g: name -> gradient tensor (absent = NULL)"""
    from osc_amd.solver import EnvGrads
    M, _, J, b0, T0, mask = a
    b, T = b0 if b is None else b, T0 if T is None else T
    data = dict(grad_M=g.get("M"), grad_C=g.get("C"), grad_J=g.get("J"), grad_wrow=g.get("wrow"),
                grad_T=g.get("T"), grad_b=g.get("b"))
    if api == "backward":
        s.backward_into(out, J, mask, gx, g.get("T"), g.get("b"))
    elif api == "backward_data":
        s.backward_data_into(out, M, J, b, T, mask, gx, **data)
    else:
        s.backward_env_into(out, M, J, b, T, mask, gx, env_params=ep, **data,
                            env_grads=EnvGrads(**{k: g[k] for k in ec.FIELDS if k in g}))


def poisoned(robot, nenv):
    """(inputs with a NaN in one env's M, that env or None): an env with a wave-mate after it
    where the batch allows, the wavefront's last where it is exactly full"""
    d = dict(batch(robot, nenv)[0])
    bad = None if nenv == 1 else nenv - 1 if nenv == 4 else nenv - 2
    if bad is not None:
        d["M"] = d["M"].copy()
        d["M"][bad, 1, 1] = np.nan
    return d, bad


@pytest.mark.parametrize("api", list(BACKWARD_COMBOS))
@pytest.mark.parametrize("nenv", NENVS)
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_backward(gpu, robot, nenv, api):
    """After a guarded forward solve with x and duals (the _env entry for backward_env): every
    gradient together and each alone, the others NULL.  The forward's x, y, status, workspace
    and inputs stay as they were; the poisoned env's gradient rows are exact zeros."""
    env = api == "backward_env"
    d, bad = poisoned(robot, nenv)
    s0 = new_solver(robot)
    a0 = s0.prepare(**d)
    o0 = s0.alloc_outputs(nenv, want_x=True, want_y=True)
    ep0 = env_block(robot, nenv) if env else None
    s0.solve_into(o0, *a0, env_params=ep0)
    fwd_ref = [shot_of(o0)]
    if bad is not None:
        assert int(o0.status[bad]) == _lib.SOLVE_NUMERICAL
    gx0 = torch.from_numpy(np.random.default_rng(SEED + 17).standard_normal((nenv, s0.dims["n"]))).cuda()
    sh = grad_shapes(s0, nenv)
    refs = []
    for combo in BACKWARD_COMBOS[api]:
        g = {k: torch.full(sh[k], float("nan"), dtype=F64, device=gpu) for k in combo}
        run_backward(api, s0, o0, a0, gx0, g, ep0)
        torch.cuda.synchronize()
        refs.append(g)
        for k, t in g.items():
            assert not torch.isnan(t).any(), (combo, k)        # every row written
            if bad is not None:
                assert not t[bad].any(), (combo, k, "poisoned env's rows")
    s = new_solver(robot)
    for pad in (0x00, 0xFF):
        tr = Tracker(gpu, pad)
        a = tuple(tr.inp(n, t) for n, t in zip(NAMES, a0))
        ep = env_block(robot, nenv, tr) if env else None
        gx = tr.inp("grad_x", gx0)
        out = guarded_result(tr, s, nenv, want_y=True)
        set_bytes(out.workspace, pad)
        s.solve_into(out, *a, env_params=ep)
        fwd = [shot_of(out, workspace=out.workspace)]
        tr.check()
        compare_shots([{k: v for k, v in fwd[0].items() if k != "workspace"}], fwd_ref, "forward")
        for combo, ref in zip(BACKWARD_COMBOS[api], refs):
            tg = Tracker(gpu, pad)
            g = {k: tg.out("grad_" + k, sh[k], F64) for k in combo}
            run_backward(api, s, out, a, gx, g, ep)
            tg.check()
            tr.check()
            for k in combo:
                assert_same(g[k], ref[k], f"{api} {combo} grad_{k} inputs in {pad:#04x}")
            now = shot_of(out, workspace=out.workspace)     # the forward's results: read only
            for k, v in now.items():
                assert_same(v, fwd[0][k], f"{api} {combo}: forward {k} after the backward pass")


# ---------------------------------------------------------------------------------------------
# alignment contract (nenv = 5)
# ---------------------------------------------------------------------------------------------

WEAK = dict(tau=8, x=8, y=8, status=4, iters=4, warm_state=8)


WEAK_KINDS = dict(cold=("cold", False, False), split=("split", False, False),
                  warm=("warm", False, False), duals=("cold", True, False),
                  env_cold=("cold", False, True), env_warm=("warm", False, True))
WEAK_CASES = [(r, sbm, k) for r, sbm in ((GO2, ONE_WAVE), (GO2, TWO_WAVE), (WALTER, ONE_WAVE),
                                         (WALTER, TWO_WAVE), (WHEELS, ONE_WAVE))
              for k in WEAK_KINDS if not (r == WHEELS and k.startswith("env"))]   # (no _env entry
#                                                                       takes a wheel-row model)


@pytest.mark.parametrize("robot,sbm,case", WEAK_CASES)
def test_outputs_at_weakest_alignment(gpu, robot, sbm, case):
    """tau, x, y (and the warm state of the single-model entries) at 8-byte but not 16-byte
    addresses, status and iters at 4-byte but not 8-byte ones: bitwise the aligned call."""
    kind, want_y, env = WEAK_KINDS[case]
    check_solve(robot, 5, sbm, kind, want_y=want_y, env=env, offs=WEAK)


@pytest.mark.parametrize("api", list(BACKWARD_COMBOS))
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_backward_at_weakest_alignment(gpu, robot, api):
    """b, T, x, y, grad_x, grad_wrow, grad_T, grad_b at 8-byte but not 16-byte addresses
    (include/osc_backward.h asks 16 bytes of M, J, the mask, the workspace and grad_M / C / J
    only): bitwise the aligned call."""
    nenv, env = 5, api == "backward_env"
    d, _ = batch(robot, nenv)
    s = new_solver(robot)
    a0 = s.prepare(**d)
    gx0 = torch.from_numpy(np.random.default_rng(SEED + 19).standard_normal((nenv, s.dims["n"]))).cuda()
    sh = grad_shapes(s, nenv)
    combo = BACKWARD_COMBOS[api][0]
    o0 = s.alloc_outputs(nenv, want_x=True, want_y=True)
    ep0 = env_block(robot, nenv) if env else None
    s.solve_into(o0, *a0, env_params=ep0)
    ref = {k: torch.full(sh[k], float("nan"), dtype=F64, device=gpu) for k in combo}
    run_backward(api, s, o0, a0, gx0, ref, ep0)
    torch.cuda.synchronize()
    tr = Tracker(gpu, 0xFF)
    a = tuple(tr.inp(n, t) for n, t in zip(NAMES, a0))
    ep = env_block(robot, nenv, tr) if env else None
    out = guarded_result(tr, s, nenv, want_y=True, offs=dict(x=8, y=8, status=4))
    s.solve_into(out, *a, env_params=ep)
    g = {k: tr.out("grad_" + k, sh[k], F64, off=0 if k in ("M", "C", "J") else 8) for k in combo}
    run_backward(api, s, out, a, tr.inp("grad_x", gx0, off=8), g, ep,
                 b=tr.inp("b8", a0[3], off=8), T=tr.inp("T8", a0[4], off=8))
    tr.check()
    for k in combo:
        assert_same(g[k], ref[k], f"{api} grad_{k}")


def refused(call):
    with pytest.raises(_lib.OSCError) as e:
        call()
    assert e.value.code == INVALID, e.value


@pytest.mark.parametrize("robot", [GO2, WALTER, WHEELS])
def test_misaligned_inputs_refused(gpu, robot):
    """Each pointer the solve entries check for 16 bytes, 8 bytes off: OSC_ERR_INVALID_ARGUMENT
    and no byte of any output written."""
    nenv = 5
    d, wd_np = batch(robot, nenv)
    s = new_solver(robot)
    a0 = s.prepare(**d)
    wheels = robot == WHEELS
    wd0 = torch.from_numpy(wd_np).cuda() if wheels else None
    entries = {"cold": NAMES, "warm": NAMES, "assemble": NAMES, "solve_assembled": ("mask",)}
    if not wheels:
        entries.update({"env_cold": NAMES, "env_warm": NAMES})
    for entry, names in entries.items():
        for bad in names + ("workspace",) + (("wheel_dir",) if wheels and entry != "solve_assembled"
                                             else ()):
            tr = Tracker(s.device, 0x00)
            a = tuple(tr.inp(n, t, off=8 if n == bad else 0) for n, t in zip(NAMES, a0))
            wd = tr.inp("wheel_dir", wd0, off=8 if bad == "wheel_dir" else 0)
            ep = env_block(robot, nenv, tr) if entry.startswith("env") else None
            out = guarded_result(tr, s, nenv, offs={"workspace": 8 if bad == "workspace" else 0})
            warm = exact_buffer(tr, "warm_state", warm_bytes(s, nenv), nenv) \
                if entry.endswith("warm") else None
            if warm is not None:
                warm._guard.base.fill_(0)          # (a valid -- zero -- state; sentinel 0)
                warm._guard.fill = 0
            if entry in ("cold", "env_cold"):
                call = lambda: s.solve_into(out, *a, wheel_dir=wd, env_params=ep)
            elif entry in ("warm", "env_warm"):
                call = lambda: s.solve_warm_into(out, warm, *a, wheel_dir=wd, env_params=ep)
            elif entry == "assemble":
                call = lambda: s.assemble_into(out, *a, wheel_dir=wd)
            else:
                call = lambda: s.solve_assembled_into(out, a[5])
            refused(call)
            tr.untouched()


@pytest.mark.parametrize("api", list(BACKWARD_COMBOS))
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_backward_misaligned_inputs_refused(gpu, robot, api):
    """The backward entries' 16-byte pointers (M, J, the mask, the workspace, grad_M / C / J), 8
    bytes off: refused, no gradient written."""
    nenv, env = 5, api == "backward_env"
    d, _ = batch(robot, nenv)
    s = new_solver(robot)
    a0 = s.prepare(**d)
    o0 = s.alloc_outputs(nenv, want_x=True, want_y=True)
    ep = env_block(robot, nenv) if env else None
    s.solve_into(o0, *a0, env_params=ep)
    torch.cuda.synchronize()
    gx = torch.zeros((nenv, s.dims["n"]), dtype=F64, device=gpu)
    sh = grad_shapes(s, nenv)
    combo = BACKWARD_COMBOS[api][0]
    cases = ("J", "mask", "workspace") if api == "backward" else \
            ("M", "J", "mask", "workspace", "grad_M", "grad_C", "grad_J")
    for bad in cases:
        from osc_amd.solver import SolveResult
        tr = Tracker(gpu, 0x00)
        a = tuple(tr.inp(n, t, off=8 if n == bad else 0) for n, t in zip(NAMES, a0))
        ws = o0.workspace
        if bad == "workspace":
            ws = tr.inp("workspace", o0.workspace, off=8)
        out = SolveResult(o0.tau, o0.x, o0.status, o0.iters, ws, o0.y)
        g = {k: tr.out("grad_" + k, sh[k], F64, off=8 if "grad_" + k == bad else 0) for k in combo}
        refused(lambda: run_backward(api, s, out, a, gx, g, ep))
        tr.untouched()


@pytest.mark.parametrize("robot", [GO2, WALTER, WHEELS])
def test_undersized_buffers_refused(gpu, robot):
    """A workspace or warm state one 16-byte unit below the reported size is refused by every
    single-model solve entry (tests/test_gpu_tick_multi.py holds the mixed tick's), outputs
    untouched -- with the exact-size cases above: the reported sizes are sufficient, exactly."""
    from osc_amd.solver import solve_multi_into
    nenv = 5
    d, wd_np = batch(robot, nenv)
    s = new_solver(robot)
    a = s.prepare(**d)
    wheels = robot == WHEELS
    wd = torch.from_numpy(wd_np).cuda() if wheels else None
    entries = ["cold", "warm", "assemble", "solve_assembled", "warm_state", "multi"] + \
              ([] if wheels else ["env_cold", "env_warm", "env_warm_state"])
    for entry in entries:
        tr = Tracker(s.device, 0x00)
        out = guarded_result(tr, s, nenv, ws=False)
        short_ws = not entry.endswith("warm_state")
        out.workspace = exact_buffer(tr, "workspace", ws_bytes(s, nenv) - (16 if short_ws else 0), nenv)
        ep = env_block(robot, nenv) if entry.startswith("env") else None
        warm = None
        if "warm" in entry:
            warm = exact_buffer(tr, "warm_state", warm_bytes(s, nenv) - (0 if short_ws else 16), nenv)
            warm._guard.base.fill_(0)
            warm._guard.fill = 0
        if entry in ("cold", "env_cold"):
            call = lambda: s.solve_into(out, *a, wheel_dir=wd, env_params=ep)
        elif "warm" in entry:
            call = lambda: s.solve_warm_into(out, warm, *a, wheel_dir=wd, env_params=ep)
        elif entry == "assemble":
            call = lambda: s.assemble_into(out, *a, wheel_dir=wd)
        elif entry == "multi":
            call = lambda: solve_multi_into([(s, out, a) + ((wd,) if wheels else ())])
        else:
            call = lambda: s.solve_assembled_into(out, a[5])
        refused(call)
        tr.untouched()


@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_undersized_joint_state_and_rollout_workspaces_refused(gpu, robot):
    nenv, nticks = 5, 3
    kb, s = kin(robot), new_solver(robot)
    d, _ = batch(robot, nenv)
    qp, qv = states(robot, nenv)
    T, mask = s.prepare(**d)[4:]
    for warm in (False, True):
        tr = Tracker(gpu, 0x00)
        out = guarded_result(tr, s, nenv, ws=False)
        ws = exact_buffer(tr, "qpos_workspace", kb.workspace_bytes(s, nenv) - 16, nenv)
        ins = (tr.inp("qpos", qp), tr.inp("qvel", qv), T, mask)
        if warm:
            refused(lambda: kb.solve_warm_into(s, out, s.alloc_warm_state(nenv), *ins, ws))
        else:
            refused(lambda: kb.solve_into(s, out, *ins, ws))
        tr.untouched()
    nb = kb.rollout_workspace_bytes(s, nenv, nticks)
    for short, off in ((16, 0), (0, 8)):            # too small; misaligned
        tr = Tracker(gpu, 0x00)
        qpos, qvel, tau, bad, hist = guarded_rollout(tr, kb, s, nenv, nticks, qp, qv)
        before = (qpos.clone(), qvel.clone())
        ws = tr.out("rollout_workspace", ((nb - short) // 8,), F64, off=off, env_bytes=nb // nenv)
        rc = rollout_raw(kb, s, nenv, nticks, T, mask, qpos, qvel, tau, bad, hist, ws, nb - short)
        assert rc == INVALID
        torch.cuda.synchronize()
        assert same(qpos, before[0]) and same(qvel, before[1])
        for name, t in tr.outs:
            if name not in ("qpos", "qvel"):
                assert bool((t._guard.base == t._guard.fill).all()), name
            assert_guards_intact(t, name)
