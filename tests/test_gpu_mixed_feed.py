"""The two-model host feed (include/osc_mixed.h, MixedHostFeed): a WaLTER Sr part and a Go2 part in
one pinned block, one H2D and one D2H copy per tick, the solve osc_batch_tick_multi.  Every tick
and part must be BITWISE tick_multi_into on the same inputs resident on the device: the feed
moves bytes, it changes no arithmetic."""
import ctypes
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from osc_amd import _lib
from osc_amd.synth import SEED_BASE, generate, random_walk

pytestmark = pytest.mark.gpu

W, G = "walter_sr", "unitree_go2"
NT = 5
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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=torch.float64)


def _inputs(form, robot, n, seed):
    """NT ticks of host inputs for one part: dicts keyed as MixedHostFeed.inputs()."""
    d = generate(robot, n, SEED_BASE + seed, "standing", "ones")
    if form == "qp":
        ticks, rng = [d], np.random.default_rng(SEED_BASE + seed + 1)
        for _ in range(1, NT):
            ticks.append(random_walk(ticks[-1], rng))
        return ticks
    from osc_amd.kinematics import load_tree, random_states
    q0, v0 = random_states(load_tree(robot), n, SEED_BASE + seed + 2, joint_range=0.5)
    rng = np.random.default_rng(SEED_BASE + seed + 3)
    ticks = []
    for k in range(NT):
        q = q0.copy()
        q[:, 7:] += 0.01 * k * rng.standard_normal(q[:, 7:].shape)
        ticks.append({"qpos": q, "qvel": v0 * (1 + 0.01 * k), "T": d["T"], "mask": d["mask"]})
    return ticks


def _reference(form, warm, sizes, data):
    """tick_multi_into, tick after tick, on the same inputs resident on the device."""
    from osc_amd.solver import TickJob, tick_multi_into
    robots = (W, G)
    out = [solver(r).alloc_outputs(n) for r, n in zip(robots, sizes)]
    wst = [solver(r).alloc_warm_state(n) if warm else None for r, n in zip(robots, sizes)]
    ws = [None, None]
    if form != "qp":
        ws = [torch.empty((kin(r).workspace_bytes(solver(r), n) // 8 + 2,), dtype=torch.float64,
                          device="cuda") for r, n in zip(robots, sizes)]
    keys = ("M", "C", "J", "b", "T", "mask") if form == "qp" else ("qpos", "qvel", "T", "mask")
    ref = []
    for k in range(NT):
        jobs = [TickJob(solver(r), out[i], tuple(dev(data[i][k][key]) for key in keys),
                        kin=kin(r) if form != "qp" else None, warm=wst[i], workspace=ws[i])
                for i, r in enumerate(robots)]
        tick_multi_into(jobs)
        torch.cuda.synchronize()
        ref.append([(o.tau.cpu().numpy(), o.status.cpu().numpy(), o.iters.cpu().numpy())
                    for o in out])
    return ref


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("sizes", [(7, 5), (33, 18)])
@pytest.mark.parametrize("form,warm", [("qp", False), ("qp", True), ("joint_states", True)])
def test_mixed_feed_bitwise_tick_multi(gpu, form, warm, sizes, depth):
    from osc_amd.host_feed import MixedHostFeed
    key = (form, warm, sizes)
    if key not in _cache:                          # inputs and reference: once per form and size
        data = [_inputs(form, r, n, 800 + 10 * i) for i, (r, n) in enumerate(zip((W, G), sizes))]
        _cache[key] = (data, _reference(form, warm, sizes, data))
    data, ref = _cache[key]
    parts = [(solver(r), n) + ((kin(r),) if form != "qp" else ()) for r, n in zip((W, G), sizes)]
    feed = MixedHostFeed(parts, form=form, depth=depth, warm=warm)
    got = {}
    for k in range(NT + depth - 1):
        if k < NT:
            for p in range(2):
                v = feed.inputs(k, p)
                for name, a in data[p][k].items():
                    v[name][...] = a
            feed.submit(k)
        j = k - depth + 1
        if j >= 0:
            got[j] = [tuple(a.copy() for a in feed.wait(j, p)) for p in range(2)]
            t = feed.timing(j)
            assert t["h2d_ms"] > 0 and t["solve_ms"] > 0 and t["d2h_ms"] > 0 and \
                t["latency_ms"] > 0, (j, t)
            if form != "qp":
                assert t["kin_ms"] > 0, (j, t)
    for k in range(NT):
        for p in range(2):
            for a, b, name in zip(got[k][p], ref[k][p], ("tau", "status", "iters")):
                assert np.array_equal(a, b), (k, p, name)
            assert (got[k][p][1] == 0).all(), (k, p)
    feed.close()


def test_mixed_feed_argument_errors(gpu):
    from osc_amd.host_feed import HostFeed, MixedHostFeed
    L = _lib.lib()
    sw, sg = solver(W), solver(G)
    with pytest.raises(_lib.OSCError) as e:                     # three parts
        MixedHostFeed([(sw, 4), (sg, 4), (sg, 4)])
    assert e.value.code == 1
    with pytest.raises(_lib.OSCError) as e:                     # kin in QP form
        MixedHostFeed([(sw, 4, kin(W)), (sg, 4)], form="qp")
    assert e.value.code == 1
    with pytest.raises(_lib.OSCError) as e:                     # joint states without a kin
        MixedHostFeed([(sw, 4, kin(W)), (sg, 4)], form="joint_states")
    assert e.value.code == 1
    with pytest.raises(_lib.OSCError) as e:                     # the other robot's kin
        MixedHostFeed([(sw, 4, kin(G)), (sg, 4, kin(G))], form="joint_states")
    assert e.value.code == 1
    feed = MixedHostFeed([(sw, 4), (sg, 3)], depth=2)
    i, o = _lib.OscFeedInputs(), _lib.OscFeedOutputs()
    h = feed._owner.h
    for part in (-1, 2):                                        # a part index out of range
        assert L.osc_host_feed_inputs_part(h, 0, part, ctypes.byref(i)) == 1
        with pytest.raises(_lib.OSCError):
            feed.inputs(0, part)
    assert L.osc_host_feed_inputs(h, 0, ctypes.byref(i)) == 1   # plain inputs on a two-part feed
    feed.inputs(0, 0)
    feed.submit(0)
    assert L.osc_host_feed_wait(h, 0, ctypes.byref(o)) == 1     # plain wait likewise
    assert L.osc_host_feed_wait_part(h, 0, 2, ctypes.byref(o)) == 1
    assert L.osc_host_feed_wait_part(h, 1, 0, ctypes.byref(o)) == 1   # not submitted
    feed.wait(0, 1)                            # all-zero inputs: a defined QP (M = 0 -> NUMERICAL)
    feed.close()
    one = MixedHostFeed([(sg, 5)], depth=1)                     # one part: the plain calls work
    assert L.osc_host_feed_inputs(one._owner.h, 0, ctypes.byref(i)) == 0
    one.close()
    single = HostFeed(sg, 5, "qp", depth=1)                     # and _part(0) on a single feed
    assert L.osc_host_feed_inputs_part(single._h, 0, 0, ctypes.byref(i)) == 0
    assert L.osc_host_feed_inputs_part(single._h, 0, 1, ctypes.byref(i)) == 1
    single.close()


def test_views_outlive_the_feed_object(gpu):
    """A view handed out by the feed keeps the native feed (its pinned memory) alive after the
    MixedHostFeed object is gone."""
    from osc_amd.host_feed import MixedHostFeed
    sizes = (7, 5)
    data = [_inputs("qp", r, n, 840 + 10 * i) for i, (r, n) in enumerate(zip((W, G), sizes))]
    feed = MixedHostFeed([(solver(W), sizes[0]), (solver(G), sizes[1])], depth=1)
    for p in range(2):
        v = feed.inputs(0, p)
        for name, a in data[p][0].items():
            v[name][...] = a
    feed.submit(0)
    tau, status, _ = feed.wait(0, 1)
    kept_in = feed.inputs(1, 0)["M"]
    expect, first_m = tau.copy(), kept_in.copy()
    del feed, v
    gc.collect()
    filler = [torch.empty((1 << 16,), device="cuda") for _ in range(4)]    # reuse freed memory
    noise = [np.full((1 << 14,), 7.0) for _ in range(16)]
    assert np.array_equal(tau, expect) and (status == 0).all()
    assert np.array_equal(kept_in, first_m)
    del filler, noise
