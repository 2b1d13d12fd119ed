"""osc_batch_tick_multi (include/osc_mixed.h): the mixed-robot tick -- a WaLTER Sr job and a Go2 job
in two-model grids -- warm-started, from joint states, or both.  Per job the results must be
BITWISE those of the matching single-model call (osc_batch_solve / _warm / _qpos / _qpos_warm): the
grids run the same per-env arithmetic.

Sizes are the smallest at which the block arithmetic can go wrong: the interior point and the
kinematics hold 4 envs per wavefront, the assembly one env per block; (7, 5), (1, 1) and (4, 9)
(WaLTER, Go2) cover partial last waves on both models and the model boundary inside the grid, and
each is run with either model listed first (the call puts WaLTER's wavefronts first itself)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from osc_amd import _lib
from osc_amd.synth import SEED_BASE, generate, random_walk

pytestmark = pytest.mark.gpu

W, G = "walter_sr", "unitree_go2"
SIZES = [(7, 5), (1, 1), (4, 9)]
NORM_TOL = 1e-9          # the bound of tests/test_gpu_mixed.py
KEYS = ("M", "C", "J", "b", "T", "mask")

_cache = {}


def solver(robot):
    from osc_amd.solver import OSCBatchSolver
    if ("s", robot) not in _cache:
        _cache["s", robot] = OSCBatchSolver(robot)
    return _cache["s", robot]


def kin(robot):
    from osc_amd.kinematics import KinematicsBatch, load_tree
    if ("k", robot) not in _cache:
        _cache["k", robot] = KinematicsBatch(tree=load_tree(robot))
    return _cache["k", robot]


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def poison(out):
    out.tau.fill_(float("nan"))
    out.status.fill_(-1)
    out.iters.fill_(-1)
    if out.x is not None:
        out.x.fill_(float("nan"))


def is_poisoned(out):
    return bool(torch.isnan(out.tau).all()) and bool((out.status == -1).all()) and \
        bool((out.iters == -1).all())


def bits(t):
    """float64 tensors compared as bit patterns (a NaN equals itself)."""
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_same(a, b, where):
    for name in ("tau", "x", "status", "iters"):
        u, v = getattr(a, name), getattr(b, name)
        assert torch.equal(bits(u), bits(v)), (where, name)


def order(pair, first):
    """The two jobs (WaLTER's, Go2's) in the order of the case."""
    return list(pair) if first == W else list(pair)[::-1]


def qp_ticks(robot, n, seed, nticks, flip_at=None):
    """nticks batches of a 1 % random walk; at tick flip_at the contact mask of a few envs is
    inverted (a contact-mode switch: those envs restart cold)."""
    data = [generate(robot, n, SEED_BASE + seed, "tumbling", "bernoulli")]
    rng = np.random.default_rng(SEED_BASE + seed + 1)
    for k in range(1, nticks):
        d = random_walk(data[-1], rng)
        if k == flip_at:
            for e in {0, n // 2, n - 1}:
                d["mask"][e] = 1.0 - d["mask"][e]
        data.append(d)
    return data


def joint_states(robot, n, seed, nticks):
    from osc_amd.kinematics import load_tree, random_states
    q0, v0 = random_states(load_tree(robot), n, SEED_BASE + seed, joint_range=0.5)
    d = generate(robot, n, SEED_BASE + seed + 1, "tumbling", "bernoulli")
    T, mask = dev(d["T"]), dev(d["mask"])
    return [(dev(q0), dev(v0 * (1.0 + 0.01 * k)), T, mask) for k in range(nticks)]


def qpos_ws(robot, n):
    nb = kin(robot).workspace_bytes(solver(robot), n)
    return torch.empty((nb // 8 + 2,), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("first", [W, G])
@pytest.mark.parametrize("nw,ng", SIZES)
def test_warm_qp_bitwise_solo(gpu, nw, ng, first):
    from osc_amd.solver import TickJob, tick_multi_into
    nt = 4
    sizes = {W: nw, G: ng}
    data = {r: qp_ticks(r, sizes[r], 700 + 10 * i, nt, flip_at=2) for i, r in enumerate((W, G))}
    s = {r: solver(r) for r in (W, G)}
    out = {r: s[r].alloc_outputs(sizes[r], want_x=True) for r in (W, G)}
    ref = {r: s[r].alloc_outputs(sizes[r], want_x=True) for r in (W, G)}
    warm = {r: s[r].alloc_warm_state(sizes[r]) for r in (W, G)}
    warm_ref = {r: s[r].alloc_warm_state(sizes[r]) for r in (W, G)}
    iters = []
    for k in range(nt):
        inputs = {r: s[r].prepare(**data[r][k]) for r in (W, G)}
        for r in (W, G):
            poison(out[r])
            s[r].solve_warm_into(ref[r], warm_ref[r], *inputs[r])
        tick_multi_into(order([TickJob(s[r], out[r], inputs[r], warm=warm[r]) for r in (W, G)],
                              first))
        torch.cuda.synchronize()
        for r in (W, G):
            assert_same(out[r], ref[r], (r, k))
        iters.append(np.concatenate([out[r].iters.cpu().numpy() for r in (W, G)]))
    for r in (W, G):
        assert torch.equal(bits(warm[r]), bits(warm_ref[r])), r
    print("mean iterations per tick:", [float(i.mean()) for i in iters])
    assert iters[3].mean() < iters[0].mean()     # warm ticks take fewer iterations


def test_warm_fixup_rescues_stalled_envs(gpu):
    """The census's stalled and formerly unrefined envs (tests/golden/*_joint_states.npz) through
    the warm entry, twice with identical inputs: the warm grids run the cold fix-up pass too."""
    from osc_amd.solver import TickJob, tick_multi_into
    gdir = os.path.join(os.path.dirname(__file__), "golden")
    sets = {G: ("go2_stalled_joint_states.npz", "go2_unrefined_joint_states.npz"),
            W: ("walter_stalled_joint_states.npz",)}
    jobs, refs, solo = [], {}, {}
    for r in (W, G):
        gs = [np.load(os.path.join(gdir, f)) for f in sets[r]]
        d = {k: np.concatenate([g[k] for g in gs]) for k in KEYS + ("tau",)}
        s, n = solver(r), d["M"].shape[0]
        inputs = s.prepare(*(d[k] for k in KEYS))
        jobs.append(TickJob(s, s.alloc_outputs(n, want_x=True), inputs, warm=s.alloc_warm_state(n)))
        refs[r] = d["tau"]
        solo[r] = (s.alloc_outputs(n, want_x=True), s.alloc_warm_state(n))
    for tick in range(2):
        for j in jobs:
            poison(j.out)
            o, w = solo[j.solver.robot]
            j.solver.solve_warm_into(o, w, *j.inputs)
        tick_multi_into(jobs)
        torch.cuda.synchronize()
        for j in jobs:
            r = j.solver.robot
            st = j.out.status.cpu().numpy()
            assert (st == 0).all(), (r, tick, st)
            assert_same(j.out, solo[r][0], (r, tick))
            got = j.out.tau.cpu().numpy()
            err = np.abs(got - refs[r]).max(axis=1) / np.maximum(np.abs(refs[r]).max(axis=1), 1.0)
            print(r, "tick", tick, "max normwise error vs fixture", err.max())
            assert err.max() <= NORM_TOL, (r, tick, err.max())


@pytest.mark.parametrize("first", [W, G])
@pytest.mark.parametrize("nw,ng", SIZES)
@pytest.mark.parametrize("warm", [False, True])
def test_joint_states_bitwise_solo(gpu, warm, nw, ng, first):
    from osc_amd.solver import TickJob, tick_multi_into
    sizes = {W: nw, G: ng}
    nt = 3 if warm else 1
    states = {r: joint_states(r, sizes[r], 720 + 10 * i, nt) for i, r in enumerate((W, G))}
    s = {r: solver(r) for r in (W, G)}
    out = {r: s[r].alloc_outputs(sizes[r], want_x=True) for r in (W, G)}
    ref = {r: s[r].alloc_outputs(sizes[r], want_x=True) for r in (W, G)}
    ws = {r: qpos_ws(r, sizes[r]) for r in (W, G)}
    ws_ref = {r: qpos_ws(r, sizes[r]) for r in (W, G)}
    wst = {r: s[r].alloc_warm_state(sizes[r]) if warm else None for r in (W, G)}
    wst_ref = {r: s[r].alloc_warm_state(sizes[r]) if warm else None for r in (W, G)}
    for k in range(nt):
        for r in (W, G):
            poison(out[r])
            if warm:
                kin(r).solve_warm_into(s[r], ref[r], wst_ref[r], *states[r][k], ws_ref[r])
            else:
                kin(r).solve_into(s[r], ref[r], *states[r][k], ws_ref[r])
        tick_multi_into(order([TickJob(s[r], out[r], states[r][k], kin=kin(r), warm=wst[r],
                                       workspace=ws[r]) for r in (W, G)], first))
        torch.cuda.synchronize()
        for r in (W, G):
            assert_same(out[r], ref[r], (r, k))
            assert (out[r].status == 0).all(), (r, k)
    if warm:
        for r in (W, G):
            assert torch.equal(bits(wst[r]), bits(wst_ref[r])), r


@pytest.mark.parametrize("nw,ng", SIZES + [(0, 6), (3, 0)])
def test_pair_kinematics_bitwise_compute(gpu, nw, ng):
    """The two-model kinematics grid called directly: M, C, J, b are kb.compute's, either model
    first (and one model's envs alone when the other has none)."""
    from osc_amd.kinematics import kinematics_pair_into
    sizes = {W: nw, G: ng}
    st = {r: joint_states(r, max(sizes[r], 1), 740 + i, 1)[0] for i, r in enumerate((W, G))}
    ref = {r: kin(r).compute_into(kin(r).alloc(max(sizes[r], 1)), st[r][0], st[r][1])
           for r in (W, G)}
    for a, b in ((W, G), (G, W)):
        got = {r: kin(r).alloc(sizes[r]) for r in (W, G)}
        for r in (W, G):
            for t in (got[r].M, got[r].C, got[r].J, got[r].b):
                t.fill_(float("nan"))
        kinematics_pair_into(kin(a), got[a], st[a][0], st[a][1], kin(b), got[b], st[b][0], st[b][1])
        torch.cuda.synchronize()
        for r in (W, G):
            for name in ("M", "C", "J", "b"):
                u, v = getattr(got[r], name), getattr(ref[r], name)[:sizes[r]]
                assert torch.equal(bits(u), bits(v.contiguous())), (a, r, name)


@pytest.mark.parametrize("first", [W, G])
def test_mixed_forms_bitwise_solo(gpu, first):
    """A WaLTER warm joint-state job next to a Go2 cold QP job: WaLTER's kinematics runs alone,
    then both share the assembly grid and the interior-point grid."""
    from osc_amd.solver import TickJob, tick_multi_into
    nw, ng, nt = 7, 5, 3
    sw, sg = solver(W), solver(G)
    states = joint_states(W, nw, 760, nt)
    data = qp_ticks(G, ng, 770, nt)
    out_w, ref_w = sw.alloc_outputs(nw, want_x=True), sw.alloc_outputs(nw, want_x=True)
    out_g, ref_g = sg.alloc_outputs(ng, want_x=True), sg.alloc_outputs(ng, want_x=True)
    ws, ws_ref = qpos_ws(W, nw), qpos_ws(W, nw)
    wst, wst_ref = sw.alloc_warm_state(nw), sw.alloc_warm_state(nw)
    for k in range(nt):
        inputs = sg.prepare(**data[k])
        poison(out_w)
        poison(out_g)
        kin(W).solve_warm_into(sw, ref_w, wst_ref, *states[k], ws_ref)
        sg.solve_into(ref_g, *inputs)
        tick_multi_into(order([TickJob(sw, out_w, states[k], kin=kin(W), warm=wst, workspace=ws),
                               TickJob(sg, out_g, inputs)], first))
        torch.cuda.synchronize()
        assert_same(out_w, ref_w, (W, k))
        assert_same(out_g, ref_g, (G, k))
    assert torch.equal(bits(wst), bits(wst_ref))


def _warm_qp_jobs(spec, seed):
    """[(robot, nenv)] -> warm QP TickJobs and, per job, the solo reference (outputs, warm)."""
    from osc_amd.solver import TickJob
    jobs, solo = [], []
    for i, (r, n) in enumerate(spec):
        s = solver(r)
        inputs = s.prepare(**generate(r, n, SEED_BASE + seed + i, "tumbling", "bernoulli"))
        jobs.append(TickJob(s, s.alloc_outputs(n, want_x=True), inputs, warm=s.alloc_warm_state(n)))
        solo.append((s.alloc_outputs(n, want_x=True), s.alloc_warm_state(n)))
    return jobs, solo


@pytest.mark.parametrize("spec", [[(G, 6), (G, 3)], [(W, 5)], [(W, 5), (G, 0)], [(G, 4100), (W, 8)]],
                         ids=["go2+go2", "one-job", "zero-env-job", "go2-past-small-batch"])
def test_fallbacks_bitwise_solo(gpu, spec):
    """Anything but an eligible {WaLTER, Go2} pair runs job after job through the single-model
    entries: same model twice, one job, a zero-env job, Go2 past one wavefront per SIMD."""
    from osc_amd.solver import tick_multi_into
    jobs, solo = _warm_qp_jobs(spec, 780)
    for tick in range(2):
        for j, (o, w) in zip(jobs, solo):
            poison(j.out)
            if j.out.tau.shape[0]:
                j.solver.solve_warm_into(o, w, *j.inputs)
        tick_multi_into(jobs)
        torch.cuda.synchronize()
        for j, (o, w) in zip(jobs, solo):
            if j.out.tau.shape[0]:
                assert_same(j.out, o, (j.solver.robot, tick))
                assert torch.equal(bits(j.warm), bits(w))


def test_refusals_launch_nothing(gpu):
    """Each bad job is refused with OSC_ERR_INVALID_ARGUMENT before anything is launched: the good
    job listed before it keeps its poisoned outputs."""
    from osc_amd.robots import config_path
    from osc_amd.solver import OSCBatchSolver, TickJob, tick_multi_into
    nw, ng = 7, 5
    sw, sg = solver(W), solver(G)
    good_inputs = sw.prepare(**generate(W, nw, SEED_BASE + 790, "tumbling", "bernoulli"))
    d = generate(G, ng, SEED_BASE + 791, "tumbling", "bernoulli")
    inputs = sg.prepare(**d)
    states = joint_states(G, ng, 792, 1)[0]

    def good():
        return TickJob(sw, sw.alloc_outputs(nw), good_inputs, warm=sw.alloc_warm_state(nw))

    def bad_jobs():
        out = lambda: sg.alloc_outputs(ng)
        noslip = OSCBatchSolver("walter_sr_wheels", os.path.join(
            os.path.dirname(config_path("walter_sr_wheels")), "walter_sr_wheels_noslip_config.yaml"))
        wheel_in = noslip.prepare(**generate(W, nw, SEED_BASE + 793, "tumbling", "bernoulli"))
        yield "wheel-row model", TickJob(noslip, noslip.alloc_outputs(nw), wheel_in)
        yield "kin of another robot", TickJob(sg, out(), states, kin=kin(W), workspace=qpos_ws(G, ng))
        yield "warm buffer too small", TickJob(sg, out(), inputs, warm=sg.alloc_warm_state(ng)[:-2])
        M8 = torch.empty((inputs[0].numel() + 1,), dtype=torch.float64, device="cuda")[1:]
        yield "misaligned M", TickJob(sg, out(), (M8.view_as(inputs[0]),) + tuple(inputs[1:]))
        w8 = torch.zeros((sg.alloc_warm_state(ng).numel() + 1,), dtype=torch.float64,
                         device="cuda")[1:]
        yield "misaligned warm state", TickJob(sg, out(), inputs, warm=w8)
        small = out()
        small.workspace = small.workspace[:16]
        yield "workspace too small", TickJob(sg, small, inputs)
        yield "joint-state workspace too small", TickJob(sg, out(), states, kin=kin(G))
        if torch.cuda.device_count() > 1:        # a job whose model lives on another device
            other = OSCBatchSolver(G, device=1)
            yield "model on another device", TickJob(other, out(), inputs)

    seen = []
    for name, bad in bad_jobs():
        g = good()
        poison(g.out)
        poison(bad.out)
        with pytest.raises(_lib.OSCError) as e:
            tick_multi_into([g, bad])
        torch.cuda.synchronize()
        assert e.value.code == 1, name
        assert is_poisoned(g.out) and is_poisoned(bad.out), name
        assert not bool(g.warm.any()), name       # (nor its warm state written)
        seen.append(name)
    assert len(seen) >= 7
    assert _lib.lib().osc_batch_tick_multi(None, 1, None) == 1
    assert _lib.lib().osc_batch_tick_multi(None, 0, None) == 0
    jobs = (_lib.OscTickJob * 1)()
    assert _lib.lib().osc_batch_tick_multi(jobs, 1, ctypes.c_void_p(0)) == 1    # NULL model
