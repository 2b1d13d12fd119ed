"""CPU tests of the rollout's backward pass (include/osc_rollout_backward.h): the reference the GPU
tests compare against (tests/rollout_backward_ref.py) and the library's boundary.

  * the torch step and PD producer equal oracle/kinematics.py::integrate and
    oracle/producers.py::pd_base_targets in value, to 1e-14;
  * the step's VJP has the stated limit at a zero rotation angle and is continuous into it;
  * the chain reference's gradients equal Richardson-extrapolated central differences,
    (4 D(h/2) - D(h)) / 3, of tests/rollout_ref.py::rollout along three drawn directions per input
    (qpos0 tangent, qvel0, held T, mass_scale), on the held Go2 case at K = 3, within NORM_TOL
    (1e-5, the project's chain contract);
  * the header's declarations are the exported symbols, the bindings' layout is the header's, the
    ABI version stays 4, and every refusal that needs no device comes back without one."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kin_env_ref as ker
import kinematics as kin
import producers
import rollout_backward_ref as rbr
import rollout_ref
from kin_trees import mixed_tree, random_tree, slider, spherical_pendulum
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_rollout_backward.h")
NORM_TOL = 1e-5     # tests/test_gpu_parity.py NORM_TOL, restated: that module needs a GPU build
GO2 = "unitree_go2"
DT = rollout_ref.DT
K = 3

# the held case of the issue: Go2, 5 envs, the masks of tests/test_gpu_kin_backward.py's chain
HELD_SEED = 7
HELD_MASK = [[0, 1, 1, 0], [1, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 1], [1, 1, 1, 1]]
NENV = 5


def trees():
    return {GO2: kin.load(GO2).d, "walter_sr": kin.load("walter_sr").d, "mixed_1": mixed_tree(1),
            "random_fixed": random_tree(2, free_root=False), "ball": spherical_pendulum(),
            "slide": slider()}


@functools.lru_cache(maxsize=None)
def held_case():
    """(tree, model, qpos, qvel, T, mask, mass_scale) of the held case."""
    from osc_amd.kinematics import random_states
    from osc_amd.synth import generate
    from osc_qp import load_model
    tree = kin.load(GO2).d
    qpos, qvel = random_states(tree, NENV, HELD_SEED, joint_range=0.5, vel_scale=0.1)
    T = generate(GO2, NENV, HELD_SEED, "standing", "ones")["T"]
    ms = ker.draw(tree, NENV, HELD_SEED + 1)["mass_scale"]
    return tree, load_model(GO2), qpos, qvel, T, np.array(HELD_MASK, dtype=np.float64), ms


def draw_cotangents(nticks, nenv, nq, nv, nu, seed):
    rng = np.random.default_rng(seed)
    return dict(qpos=rng.standard_normal((nticks + 1, nenv, nq)),
                qvel=rng.standard_normal((nticks + 1, nenv, nv)),
                tau=0.1 * rng.standard_normal((nticks, nenv, nu)))


def env_cot(cot, e):
    return {k: v[:, e] for k, v in cot.items()}


@pytest.mark.parametrize("name", list(trees()))
def test_step_equals_the_oracle(name):
    m = kin.KinModel(trees()[name])
    rng = np.random.default_rng(3)
    for dt in (DT, -DT):
        for zero in (False, True):
            qpos, qvel = kin.random_state(m, rng, base_pos_zero=False)
            qacc = rng.standard_normal(m.nv)
            if zero:
                qvel[:], qacc[:] = 0.0, 0.0
            qn, vn = rbr.step(m, rbr._t(qpos), rbr._t(qvel), rbr._t(qacc), dt)
            v_ref = qvel + dt * qacc
            assert np.abs(vn.numpy() - v_ref).max() <= 1e-14
            assert np.abs(qn.numpy() - kin.integrate(m, qpos, v_ref, dt)).max() <= 1e-14


def test_pd_producer_equals_the_oracle():
    rng = np.random.default_rng(4)
    for _ in range(5):
        pos, lin, ang, pref = (rng.standard_normal(3) for _ in range(4))
        q, qr = rng.standard_normal(4), rng.standard_normal(4)
        gains = tuple(rng.uniform(1, 100, 4))
        got = rbr.pd_targets(7, *(rbr._t(a) for a in (pos, q, lin, ang, pref, qr)), gains).numpy()
        ref = producers.pd_base_targets(7, pos, q, lin, ang, pref, qr, gains)
        assert np.abs(got - ref).max() <= 1e-14 * (1 + np.abs(ref).max())
        assert (got[1:] == 0).all()


def test_step_vjp_at_and_near_a_zero_angle():
    """At zero rates the increment's vector part has slope dt / 2 (not 0), and rates of 1e-9 give
    the same gradients to 1e-9: the VJP is continuous into the limit."""
    m = kin.KinModel(spherical_pendulum())
    rng = np.random.default_rng(6)
    qpos, _ = kin.random_state(m, rng)
    gq, gv = rng.standard_normal(m.nq), rng.standard_normal(m.nv)
    z = np.zeros(m.nv)
    g0 = rbr.step_vjp(m, qpos, z, z, DT, gq, gv)
    g1 = rbr.step_vjp(m, qpos, 1e-9 * rng.standard_normal(m.nv), z, DT, gq, gv)
    for a, b in zip(g0, g1):
        assert np.abs(a - b).max() <= 1e-9
    # q' = q (1, w dt / 2) to first order: d q' / d w = (dt / 2) q (0, e_k), and q is unit
    for k in range(3):
        e = np.zeros(4)
        e[1 + k] = 1.0
        col = 0.5 * DT * producers.quat_mul(qpos, e)
        assert abs((g0[1][k] - gv[k]) - gq @ col) <= 1e-15
    assert np.abs(g0[1] - gv).max() > 1e-5


@functools.lru_cache(maxsize=None)
def held_chain():
    """The chain reference on the held case with drawn cotangents on every slab: per env
    (grads, hist).  Its cleanliness assertions run inside."""
    tree, mdl, qpos, qvel, T, mask, ms = held_case()
    cot = draw_cotangents(K, NENV, qpos.shape[1], qvel.shape[1], mdl.nu, 17)
    out = [rbr.chain(tree, mdl, qpos[e], qvel[e], mask[e], K, DT, env_cot(cot, e), T=T[e],
                     kin_params=dict(mass_scale=ms[e]), where=e) for e in range(NENV)]
    return cot, out


def test_chain_forward_equals_the_rollout_reference():
    tree, mdl, qpos, qvel, T, mask, ms = held_case()
    cot, out = held_chain()
    for e in (0, 3):
        km = ker.env_model(tree, mass_scale=ms[e])
        ref = rollout_ref.rollout(km, mdl, qpos[e], qvel[e], mask[e], K, DT, T=T[e])
        for k in ("qpos", "qvel", "tau"):
            assert np.abs(out[e][1][k] - ref[k]).max() <= 1e-9 * (1 + np.abs(ref[k]).max()), (e, k)


@pytest.mark.parametrize("e", range(NENV))
def test_chain_equals_finite_differences_of_the_rollout(e):
    """Directional derivatives along three drawn directions per input against (4 D(h/2) - D(h)) / 3
    of the oracle rollout's loss, |g.d - fd| <= NORM_TOL (1 + |fd|).  Measured worst over the five
    envs and twelve directions: 7e-11 (printed per direction)."""
    tree, mdl, qpos, qvel, T, mask, ms = held_case()
    cot, out = held_chain()
    g = out[e][0]
    c = env_cot(cot, e)
    rng = np.random.default_rng(100 + e)

    def loss(q0, v0, Te, mse):
        km = ker.env_model(tree, mass_scale=mse)
        r = rollout_ref.rollout(km, mdl, q0, v0, mask[e], K, DT, T=Te)
        return sum((c[k] * r[k]).sum() for k in ("qpos", "qvel", "tau"))

    x0 = dict(qpos0=qpos[e], qvel0=qvel[e], T=T[e], mass_scale=ms[e])
    worst = 0.0
    for name, h in (("qpos0", 1e-4), ("qvel0", 1e-4), ("T", 1e-3), ("mass_scale", 1e-4)):
        for _ in range(3):
            d = rng.standard_normal(x0[name].shape)
            if name == "qpos0":   # a tangent direction: orthogonal to the base quaternion
                d[3:7] -= qpos[e][3:7] * (d[3:7] @ qpos[e][3:7])
            d /= np.abs(d).max()

            def D(step):
                xp = dict(x0, **{name: x0[name] + step * d})
                xm = dict(x0, **{name: x0[name] - step * d})
                return (loss(xp["qpos0"], xp["qvel0"], xp["T"], xp["mass_scale"]) -
                        loss(xm["qpos0"], xm["qvel0"], xm["T"], xm["mass_scale"])) / (2 * step)

            fd = (4 * D(h / 2) - D(h)) / 3
            got = float((g[name] * d).sum())
            err = abs(got - fd) / (1 + abs(fd))
            worst = max(worst, err)
            print(f"env {e} {name}: g.d {got:+.6e} fd {fd:+.6e} err {err:.2e}")
            assert err <= NORM_TOL, (name, got, fd)
    print(f"env {e}: worst {worst:.2e}")


def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.ROLLOUT_BACKWARD_SYMBOLS)
    assert len(declared) == 4
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS) |
                           set(_lib.ENV_PARAMS_SYMBOLS) | set(_lib.BACKWARD_ENV_SYMBOLS) |
                           set(_lib.KIN_ENV_SYMBOLS) | set(_lib.KIN_BACKWARD_SYMBOLS))
    assert L.osc_abi_version() == 4
    body = re.search(r"typedef struct \{(.*?)\} osc_rollout_backward_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)(?:\[\d+\])?;", body)
    assert fields == [n for n, _ in _lib.OscRolloutBackwardArgs._fields_]
    assert ctypes.sizeof(_lib.OscRolloutBackwardArgs) == 208   # the unit's static_assert


def test_refusals_come_back_without_a_device():
    """The step's and the producer's adjoints check their arguments before they read the model or
    an array: a host buffer stands in for the handle and the device arrays."""
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    vp = ctypes.c_void_p
    good = dict(kin=vp(a), nenv=4, dt=DT, qpos=vp(a + 8), qvn=vp(a + 16), status=None,
                qacc=vp(a + 24), stride=18, gqn=vp(a + 32), gvn=vp(a + 40), gq=vp(a + 48),
                gv=vp(a + 56), ga=None, gstride=18)

    def step(**kw):
        c = dict(good, **kw)
        return L.osc_batch_integrate_backward(c["kin"], c["nenv"], c["dt"], c["qpos"], c["qvn"],
                                              c["status"], c["qacc"], c["stride"], c["gqn"],
                                              c["gvn"], c["gq"], c["gv"], c["ga"], c["gstride"],
                                              None)

    assert step(kin=None) == 1 and step(nenv=-1) == 1
    assert step(dt=float("nan")) == 1 and step(dt=float("inf")) == 1
    assert step(gq=None, gv=None, ga=None) == 1            # every output NULL
    for k in ("qpos", "qvn", "qacc", "gqn", "gvn", "gq", "gv", "ga"):
        assert step(**{k: vp(a + 100)}) == 1, k            # not 8-byte aligned
    assert step(status=vp(a + 2)) == 1
    assert step(nenv=0) == 0                               # an empty batch

    gains = (ctypes.c_double * 4)(150.0, 25.0, 50.0, 10.0)
    pgood = dict(nenv=4, ns=5, q=None, qr=vp(a), per=0, gains=gains, gT=vp(a + 8), gp=vp(a + 16),
                 gq=None, gl=None, ga=None)

    def pd(**kw):
        c = dict(pgood, **kw)
        return L.osc_pd_base_targets_backward(c["nenv"], c["ns"], c["q"], c["qr"], c["per"],
                                              c["gains"], c["gT"], c["gp"], c["gq"], c["gl"],
                                              c["ga"], None)

    assert pd(nenv=-1) == 1 and pd(ns=0) == 1 and pd(gains=None) == 1
    assert pd(gp=None) == 1                                # every output NULL
    for k in ("q", "qr", "gT", "gp", "gq", "gl", "ga"):
        assert pd(**{k: vp(a + 100)}) == 1, k
    assert pd(nenv=0) == 0

    # the rollout's backward refuses NULL handles and NULL sizes' pointers before anything else
    nb = ctypes.c_size_t()
    assert L.osc_rollout_backward_workspace_bytes(None, None, 4, ctypes.byref(nb)) == 1
    assert L.osc_batch_rollout_backward(None, None, 4, None, None, None, None) == 1
