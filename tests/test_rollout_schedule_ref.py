"""CPU tests of the scheduled rollout (include/osc_rollout_schedule.h): the reference the GPU tests
compare against (tests/rollout_schedule_ref.py), the cases they share, and the library's boundary.

  * the reference's gradients with respect to pos_ref, quat_ref and the gains equal
    Richardson-extrapolated central differences, (4 D(5e-5) - D(1e-4)) / 3, of the ORACLE rollout
    over every entry, within 1e-7 (1 + max |g|): the construction and the bar of
    tests/test_kin_backward_ref.py;
  * its per-tick grad_T equals the same differences along drawn directions within NORM_TOL, the
    bar tests/test_rollout_backward_ref.py holds grad_T to;
  * every case the GPU tests run against the chain passes rollout_backward_ref.assert_clean at
    every (env, tick): a certified optimum and a clean working set.  The cases (seeds, mask
    schedules) were chosen on the CPU so that the reference alone is clean;
  * the header's declarations are the exported symbols, the bindings' layouts are the header's,
    the ABI version stays 4, and the refusals that need no device come back without one."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kinematics as kin
import rollout_ref
import rollout_schedule_ref as rsr
import test_rollout_backward_ref as cpu
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_rollout_schedule.h")
NORM_TOL = cpu.NORM_TOL
FD_TOL = 1e-7       # tests/test_kin_backward_ref.py FD_TOL, the same construction
GO2, WALTER = "unitree_go2", "walter_sr"
DT = rollout_ref.DT
K = 3
NENV = 5
GAINS = rollout_ref.STANDING_GAINS
OFFSET = np.array([0.01, -0.01, -0.02])

# The chain cases: random_states(tree, NENV, SEED[robot], joint_range=0.5, vel_scale=0.1), the
# feed-forward and the references of sched_case below, and a mask schedule MASKS[robot][t][e] (env
# e's mask at tick t).  The schedules were searched on the CPU reference, over every tick-0 mask and
# every single loaded contact lifted at tick 1 and put back at tick 2 (a swing phase), for the first
# one that is clean at all three ticks in all three uses of the case (PD with held references, PD
# with the reference sequences, held targets); an env for which no lift is clean keeps one mask
# (Go2 envs 0 and 2).  Under OSC_ROLLOUT_WARM the envs that flip restart cold twice.
SEED = {GO2: 7, WALTER: 7}
_GO2_0 = [[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 1], [0, 1, 1, 1]]
_GO2_1 = [[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 1, 0, 1]]
_WALTER_0 = [[1, 0, 1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1], [1, 1, 1, 0, 1, 1, 1, 1],
             [1, 1, 1, 1, 1, 1, 1, 1], [1, 0, 1, 0, 0, 0, 0, 0]]
_WALTER_1 = [[0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1], [0, 1, 1, 0, 1, 1, 1, 1],
             [0, 1, 1, 1, 1, 1, 1, 1], [0, 0, 1, 0, 0, 0, 0, 0]]
MASKS = {GO2: [_GO2_0, _GO2_1, _GO2_0], WALTER: [_WALTER_0, _WALTER_1, _WALTER_0]}
FF_SCALE = 0.05     # the feed-forward's size, next to PD targets of ~1


@functools.lru_cache(maxsize=None)
def sched_case(robot):
    """dict of the chain case of a robot (read-only arrays): tree, mdl, qpos, qvel (NENV, .),
    masks (K, NENV, nc), ff (K, NENV, ns, 6) the feed-forward, pos_ref_seq (K, NENV, 3) per env: a
    ramp towards the initial base position + OFFSET, quat_ref_seq (K, 4) shared: a small drift off
    the identity, and the held references pos_ref (NENV, 3), quat_ref (4,)."""
    from osc_amd.kinematics import random_states
    from osc_qp import load_model
    tree = kin.load(robot).d
    mdl = load_model(robot)
    qpos, qvel = random_states(tree, NENV, SEED[robot], joint_range=0.5, vel_scale=0.1)
    rng = np.random.default_rng(SEED[robot] + 50)
    masks = np.array(MASKS[robot], dtype=np.float64)
    ff = FF_SCALE * rng.standard_normal((K, NENV, mdl.ns, 6))
    ramp = (np.arange(1, K + 1) / K)[:, None, None]
    pos_ref_seq = qpos[None, :, 0:3] + ramp * OFFSET
    quat_ref_seq = np.array([[1.0, 0.01 * (t + 1), -0.005 * (t + 1), 0.002 * t] for t in range(K)])
    quat_ref_seq /= np.linalg.norm(quat_ref_seq, axis=1, keepdims=True)
    c = dict(qpos=qpos, qvel=qvel, masks=masks, ff=ff, pos_ref_seq=pos_ref_seq,
             quat_ref_seq=quat_ref_seq, pos_ref=qpos[:, 0:3] + OFFSET,
             quat_ref=np.array([1.0, 0.0, 0.0, 0.0]))
    for a in c.values():
        a.setflags(write=False)
    c.update(tree=tree, mdl=mdl, cot=cpu.draw_cotangents(K, NENV, qpos.shape[1], qvel.shape[1],
                                                         mdl.nu, SEED[robot] + 60))
    return c


def env_pd(c, e, seq):
    """Env e's (pos_refs (K, 3), quat_refs (K, 4), gains): the sequences, or the held references
    repeated over the ticks."""
    if seq:
        return c["pos_ref_seq"][:, e], c["quat_ref_seq"], GAINS
    return np.tile(c["pos_ref"][e], (K, 1)), np.tile(c["quat_ref"], (K, 1)), GAINS


@functools.lru_cache(maxsize=None)
def sched_chain(robot, seq):
    """The chain reference on sched_case(robot), PD targets + feed-forward + mask schedule, with
    the reference sequences (seq) or the held references: per env (grads, hist).  Its cleanliness
    assertions run inside, at every (env, tick)."""
    c = sched_case(robot)
    return [rsr.chain(c["tree"], c["mdl"], c["qpos"][e], c["qvel"][e], c["masks"][:, e], K, DT,
                      cpu.env_cot(c["cot"], e), T=c["ff"][:, e], pd=env_pd(c, e, seq),
                      where=(robot, e)) for e in range(NENV)]


@functools.lru_cache(maxsize=None)
def held_sched_chain(robot):
    """Held mode on the same case: tick t's targets are ff[t] alone (a target sequence)."""
    c = sched_case(robot)
    return [rsr.chain(c["tree"], c["mdl"], c["qpos"][e], c["qvel"][e], c["masks"][:, e], K, DT,
                      cpu.env_cot(c["cot"], e), T=c["ff"][:, e], where=(robot, "held", e))
            for e in range(NENV)]


@pytest.mark.parametrize("seq", [False, True])
@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_the_gpu_cases_are_clean_on_the_reference(robot, seq):
    """Every (env, tick) of the cases tests/test_gpu_rollout_schedule.py compares against the chain
    passes assert_clean (it runs inside the chain); at least three envs of each robot lift a
    contact at tick 1 and put it back at tick 2."""
    out = sched_chain(robot, seq)
    assert len(out) == NENV
    c = sched_case(robot)
    flips = (c["masks"][0] != c["masks"][1]).any(axis=1)
    assert flips.sum() >= 3 and (c["masks"][0] == c["masks"][2]).all()
    for g, _ in out:
        assert all(np.isfinite(v).all() for v in g.values())
    if robot == GO2:      # the references and gains are felt (WaLTER's torso rows carry no weight)
        for k in ("pos_ref", "quat_ref", "gains"):
            assert max(np.abs(g[k]).max() for g, _ in out) > 1e-3, k


@pytest.mark.parametrize("robot", [GO2, WALTER])
def test_the_held_gpu_cases_are_clean_on_the_reference(robot):
    out = held_sched_chain(robot)
    assert max(np.abs(g["T_seq"]).max() for g, _ in out) > 1e-3


def test_chain_forward_equals_the_scheduled_oracle_rollout():
    c = sched_case(GO2)
    km = kin.KinModel(c["tree"])
    for e in (0, 3):
        got = sched_chain(GO2, True)[e][1]
        ref = rsr.rollout(km, c["mdl"], c["qpos"][e], c["qvel"][e], c["masks"][:, e], K, DT,
                          T=c["ff"][:, e], pd=env_pd(c, e, True))
        for k in ("qpos", "qvel", "tau"):
            assert np.abs(got[k] - ref[k]).max() <= 1e-9 * (1 + np.abs(ref[k]).max()), (e, k)


@pytest.mark.parametrize("e", range(NENV))
def test_reference_and_gain_gradients_equal_finite_differences(e):
    """Go2, held references: every entry of grad pos_ref, quat_ref and gains against
    (4 D(5e-5) - D(1e-4)) / 3 of the scheduled oracle rollout's loss, within 1e-7 (1 + max |g|) per
    input.  Printed per input; measured worst over the five envs: 6.7e-9 on max |g| = 95."""
    c = sched_case(GO2)
    g = sched_chain(GO2, False)[e][0]
    km = kin.KinModel(c["tree"])
    cot = cpu.env_cot(c["cot"], e)
    x0 = dict(pos_ref=c["pos_ref"][e].copy(), quat_ref=c["quat_ref"].copy(),
              gains=np.array(GAINS, float))

    def loss(x):
        pd = (np.tile(x["pos_ref"], (K, 1)), np.tile(x["quat_ref"], (K, 1)), tuple(x["gains"]))
        r = rsr.rollout(km, c["mdl"], c["qpos"][e], c["qvel"][e], c["masks"][:, e], K, DT,
                        T=c["ff"][:, e], pd=pd)
        return sum((cot[k] * r[k]).sum() for k in ("qpos", "qvel", "tau"))

    def D(k, i, h):
        xp = {n: v.copy() for n, v in x0.items()}
        xm = {n: v.copy() for n, v in x0.items()}
        xp[k][i] += h
        xm[k][i] -= h
        return (loss(xp) - loss(xm)) / (2 * h)

    for k in x0:
        fd = np.array([(4 * D(k, i, 5e-5) - D(k, i, 1e-4)) / 3 for i in range(len(x0[k]))])
        err, scale = np.abs(g[k] - fd).max(), np.abs(fd).max()
        print(f"env {e} {k}: max |g| {scale:.3e} err {err:.3e}")
        assert err <= FD_TOL * (1 + scale), (k, err, scale)


def test_sequence_gradients_equal_finite_differences():
    """Go2 env 1, the reference sequences and the feed-forward: tick t's grad pos_ref_seq /
    quat_ref_seq entry by entry as above (the same bar), and grad_T_seq along two drawn directions
    per tick within NORM_TOL (1 + |fd|), as tests/test_rollout_backward_ref.py holds grad T."""
    e = 1
    c = sched_case(GO2)
    g = sched_chain(GO2, True)[e][0]
    km = kin.KinModel(c["tree"])
    cot = cpu.env_cot(c["cot"], e)
    x0 = dict(pos_ref_seq=c["pos_ref_seq"][:, e].copy(), quat_ref_seq=c["quat_ref_seq"].copy(),
              T_seq=c["ff"][:, e].copy())

    def loss(x):
        r = rsr.rollout(km, c["mdl"], c["qpos"][e], c["qvel"][e], c["masks"][:, e], K, DT,
                        T=x["T_seq"], pd=(x["pos_ref_seq"], x["quat_ref_seq"], GAINS))
        return sum((cot[k] * r[k]).sum() for k in ("qpos", "qvel", "tau"))

    def D(k, d, h):
        return (loss(dict(x0, **{k: x0[k] + h * d})) - loss(dict(x0, **{k: x0[k] - h * d}))) / (2 * h)

    for k in ("pos_ref_seq", "quat_ref_seq"):
        fd = np.zeros(x0[k].shape)
        for idx in np.ndindex(*x0[k].shape):
            d = np.zeros(x0[k].shape)
            d[idx] = 1.0
            fd[idx] = (4 * D(k, d, 5e-5) - D(k, d, 1e-4)) / 3
        err, scale = np.abs(g[k] - fd).max(), np.abs(fd).max()
        print(f"{k}: max |g| {scale:.3e} err {err:.3e}")
        assert err <= FD_TOL * (1 + scale), (k, err, scale)
    rng = np.random.default_rng(11)
    for t in range(K):
        for _ in range(2):
            d = np.zeros(x0["T_seq"].shape)
            d[t] = rng.standard_normal(d[t].shape)
            fd = (4 * D("T_seq", d, 5e-4) - D("T_seq", d, 1e-3)) / 3
            got = float((g["T_seq"] * d).sum())
            print(f"T_seq tick {t}: g.d {got:+.6e} fd {fd:+.6e}")
            assert abs(got - fd) <= NORM_TOL * (1 + abs(fd)), (t, got, fd)


def test_held_references_are_the_sums_of_the_sequence_gradients():
    """With K identical reference slabs the held gradients are the tick-ordered sums of the per-tick
    ones (the reference's own bookkeeping, which the GPU test relies on)."""
    for g, _ in sched_chain(GO2, False):
        for k in ("pos_ref", "quat_ref"):
            acc = np.zeros_like(g[k])
            for t in range(K - 1, -1, -1):
                acc = acc + g[k + "_seq"][t]
            assert np.array_equal(acc, g[k])


# ---- the library's boundary -----------------------------------------------------------------------------

def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.ROLLOUT_SCHEDULE_SYMBOLS)
    assert len(declared) == 3
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS) |
                           set(_lib.ENV_PARAMS_SYMBOLS) | set(_lib.BACKWARD_ENV_SYMBOLS) |
                           set(_lib.KIN_ENV_SYMBOLS) | set(_lib.KIN_BACKWARD_SYMBOLS) |
                           set(_lib.ROLLOUT_BACKWARD_SYMBOLS))
    assert L.osc_abi_version() == 4            # purely additive: no ABI bump
    for struct, cls, size in (("osc_rollout_schedule", _lib.OscRolloutSchedule, 32),
                              ("osc_rollout_schedule_grads", _lib.OscRolloutScheduleGrads, 48)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(\w+)(?:\[\d+\])?;", body)
        assert fields == [n for n, _ in cls._fields_], struct
        assert ctypes.sizeof(cls) == size, struct      # the unit's static_assert
    # the two argument blocks the schedule rides on keep their layouts
    assert ctypes.sizeof(_lib.OscRolloutArgs) == 184
    assert ctypes.sizeof(_lib.OscRolloutBackwardArgs) == 208
    unit = open(os.path.join(REPO, "operational-space-control_amd", "csrc",
                             "osc_rollout_schedule.hip")).read()
    for struct, size in (("osc_rollout_schedule", 32), ("osc_rollout_schedule_grads", 48)):
        assert re.search(r"sizeof\(%s\) == %d" % (struct, size), unit), struct


def test_refusals_come_back_without_a_device():
    """The producer's parameter adjoint checks its arguments before it reads an array (a host buffer
    stands in for the device arrays); the two rollout entries refuse NULL handles first."""
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    vp = ctypes.c_void_p
    gains = (ctypes.c_double * 4)(*GAINS)
    good = dict(nenv=4, ns=5, p=vp(a), q=vp(a + 8), v=vp(a + 16), w=vp(a + 24), pr=vp(a + 32),
                ppe=0, qr=vp(a + 40), qpe=0, gains=gains, gT=vp(a + 48), gp=vp(a + 56), gq=None,
                gg=None)

    def call(**kw):
        c = dict(good, **kw)
        return L.osc_pd_base_targets_backward_params(
            c["nenv"], c["ns"], c["p"], c["q"], c["v"], c["w"], c["pr"], c["ppe"], c["qr"],
            c["qpe"], c["gains"], c["gT"], c["gp"], c["gq"], c["gg"], None)

    assert call(nenv=-1) == 1 and call(ns=0) == 1 and call(gains=None) == 1
    assert call(gp=None) == 1                              # every output NULL
    for k in ("p", "q", "v", "w", "pr", "qr", "gT", "gp", "gq", "gg"):
        assert call(**{k: vp(a + 100)}) == 1, k            # not 8-byte aligned
    for k in ("p", "q", "v", "w", "pr", "qr", "gT"):
        assert call(**{k: None}) == 1, k                   # a missing input
    assert call(nenv=0) == 0                               # an empty batch
    sc, sg = _lib.OscRolloutSchedule(), _lib.OscRolloutScheduleGrads()
    ra, ba = _lib.OscRolloutArgs(), _lib.OscRolloutBackwardArgs()
    assert L.osc_batch_rollout_sched(None, None, 4, ctypes.byref(ra), ctypes.byref(sc), None,
                                     None, None) == 1
    assert L.osc_batch_rollout_sched(None, None, 4, None, None, None, None, None) == 1
    assert L.osc_batch_rollout_backward_sched(None, None, 4, ctypes.byref(ba), ctypes.byref(sc),
                                              ctypes.byref(sg), None, None, None) == 1
