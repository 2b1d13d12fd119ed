"""CPU tests of the kinematics' backward pass (include/osc_kin_backward.h): the reference the GPU
tests compare against (tests/kin_backward_ref.py, a torch restatement of oracle/kinematics.py
differentiated by autograd) and the library's boundary.

  * the restatement's forward is the oracle's within the kinematics bar 1e-12 (1 + max |ref|);
  * its gradient of sum(G . outputs), G standard normal, is the Richardson-extrapolated central
    difference of the ORACLE, (4 D(5e-5) - D(1e-4)) / 3, over every qpos, qvel and parameter entry,
    within 1e-7 (1 + max |g|) -- that estimate is self-consistent to 6e-10 on |g| ~ 8 (Go2) and
    1e-9 on |g| ~ 11 (WaLTER), which leaves about 1000x;
  * properties of the oracle's gradient that the kernel must share: no gradient with respect to a
    free root's position without grad_site_xpos, quaternion blocks orthogonal to q;
  * the header's declarations are the exported symbols, the ABI version stays 4, and every
    refusal comes back without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import kin_backward_ref as kbr
import kin_env_ref as ker
import kinematics as kin
from kin_trees import chain_tree, mixed_tree, random_tree
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_kin_backward.h")
FWD_TOL = 1e-12
FD_TOL = 1e-7


def trees():
    return {"unitree_go2": kin.load("unitree_go2").d, "walter_sr": kin.load("walter_sr").d,
            "random_1": random_tree(1), "random_fixed": random_tree(4, free_root=False),
            "chain": chain_tree(2), "mixed_3": mixed_tree(3)}


NAMES = list(trees())


def _case(name, seed=3):
    tree = trees()[name]
    m = kin.KinModel(tree)
    qpos, qvel = kin.random_state(m, np.random.default_rng(seed), base_pos_zero=False)
    p = {k: v[0] for k, v in ker.draw(tree, 1, seed + 10).items()}
    return tree, m, qpos, qvel, p


def _oracle(tree, qpos, qvel, p):
    """The oracle's five outputs under per-env parameters; the armature scale is applied per dof on
    the model (env_tree takes it per joint only)."""
    m = ker.env_model(tree, mass_scale=p["mass_scale"], com_offset=p["com_offset"])
    m.armature = m.armature * p["armature_scale"]
    return dict(zip(kbr.OUTPUTS, (*kin.kinematics(m, qpos, qvel), kin.site_positions(m, qpos))))


@pytest.mark.parametrize("name", NAMES)
def test_forward_equals_the_oracle(name):
    tree, m, qpos, qvel, p = _case(name)
    import torch
    for params in (None, p):
        pt = None if params is None else {k: kbr._t(v) for k, v in params.items()}
        got = kbr.forward(m, kbr._t(qpos), kbr._t(qvel), pt)
        ref = _oracle(tree, qpos, qvel, params or {k: v[0] for k, v in
                                                   ker.identity(tree, 1).items()})
        for k, g in zip(kbr.OUTPUTS, got):
            assert isinstance(g, torch.Tensor) and g.dtype == torch.float64
            err = np.abs(g.numpy() - ref[k]).max()
            assert err <= FWD_TOL * (1 + np.abs(ref[k]).max()), (k, err)


@pytest.mark.parametrize("name", NAMES)
def test_gradient_equals_finite_differences_of_the_oracle(name):
    tree, m, qpos, qvel, p = _case(name)
    G = {k: v[0] for k, v in kbr.draw_cotangents(m, 1, 7).items()}
    got = kbr.vjp(m, qpos, qvel, p, G)
    x0 = dict(qpos=qpos, qvel=qvel, **p)

    def loss(x):
        o = _oracle(tree, x["qpos"], x["qvel"], x)
        return sum((G[k] * o[k]).sum() for k in kbr.OUTPUTS)

    def D(k, idx, h):
        xp = {n: v.copy() for n, v in x0.items()}
        xm = {n: v.copy() for n, v in x0.items()}
        xp[k][idx] += h
        xm[k][idx] -= h
        return (loss(xp) - loss(xm)) / (2 * h)

    for k in kbr.INPUTS:
        fd = np.zeros(x0[k].shape)
        for idx in np.ndindex(*x0[k].shape):
            fd[idx] = (4 * D(k, idx, 5e-5) - D(k, idx, 1e-4)) / 3
        err, scale = np.abs(got[k] - fd).max(), np.abs(fd).max()
        print(f"{name} {k}: max |g| {scale:.3e} err {err:.3e}")
        assert err <= FD_TOL * (1 + scale), (k, err, scale)


@pytest.mark.parametrize("name", ["unitree_go2", "walter_sr", "random_1", "mixed_3"])
def test_translation_and_quaternion_properties(name):
    tree, m, qpos, qvel, p = _case(name, seed=5)
    G = {k: v[0] for k, v in kbr.draw_cotangents(m, 1, 9).items()}
    G["site_xpos"] = None
    g = kbr.vjp(m, qpos, qvel, p, G)
    scale = 1 + np.abs(g["qpos"]).max()
    for j in m.joints:
        qa = j["qadr"]
        if j["type"] == "free":
            assert np.abs(g["qpos"][qa:qa + 3]).max() <= 1e-11 * scale
            assert abs(g["qpos"][qa + 3:qa + 7] @ qpos[qa + 3:qa + 7]) <= 1e-11 * scale
        elif j["type"] == "ball":
            assert abs(g["qpos"][qa:qa + 4] @ qpos[qa:qa + 4]) <= 1e-11 * scale


def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.KIN_BACKWARD_SYMBOLS) == {"osc_batch_kinematics_backward"}
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS) |
                           set(_lib.ENV_PARAMS_SYMBOLS) | set(_lib.BACKWARD_ENV_SYMBOLS) |
                           set(_lib.KIN_ENV_SYMBOLS))
    assert L.osc_abi_version() == 4
    body = re.search(r"typedef struct \{(.*?)\} osc_kin_env_grads;", text, re.S).group(1)
    fields = re.findall(r"double\*\s+(\w+);", body)
    assert fields == [n for n, _ in _lib.OscKinEnvGrads._fields_]
    assert fields == ["mass_scale", "com_offset", "armature_scale"]


def test_refusals_come_back_without_a_device():
    """The argument checks read neither the model nor the arrays: a host buffer stands in for the
    handle and for the device arrays."""
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    vp = ctypes.c_void_p
    good = dict(kin=vp(a), nenv=4, qpos=vp(a + 8), qvel=vp(a + 16), kp=None, gM=vp(a + 24),
                gC=None, gJ=None, gb=None, gx=None, gq=vp(a + 32), gv=vp(a + 40), kg=None)

    def call(**kw):
        c = dict(good, **kw)
        return L.osc_batch_kinematics_backward(c["kin"], c["nenv"], c["qpos"], c["qvel"], c["kp"],
                                               c["gM"], c["gC"], c["gJ"], c["gb"], c["gx"],
                                               c["gq"], c["gv"], c["kg"], None)

    assert call(kin=None) == 1
    assert call(nenv=-1) == 1
    assert call(qpos=None) == 1 and call(qvel=None) == 1
    for k in ("qpos", "qvel", "gM", "gC", "gJ", "gb", "gx", "gq", "gv"):
        assert call(**{k: vp(a + 100)}) == 1, k          # not 8-byte aligned
    for field in ("mass_scale", "com_offset", "armature_scale"):
        p = _lib.OscKinEnvParams()
        setattr(p, field, a + 4)
        assert call(kp=ctypes.byref(p)) == 1, field
        g = _lib.OscKinEnvGrads()
        setattr(g, field, a + 4)
        assert call(kg=ctypes.byref(g)) == 1, field
    assert call(gq=None, gv=None) == 1                   # every output NULL
    assert call(gq=None, gv=None, kg=ctypes.byref(_lib.OscKinEnvGrads())) == 1
    assert call(nenv=0) == 0                             # an empty batch
