"""CPU tests of the per-env inertial parameters (include/osc_kin_env_params.h,
osc_amd.kinematics.KinEnvParams): the library's boundary -- the header's declarations are the
exported symbols, the ABI version is unchanged, argument errors come back without a device,
KinEnvParams refuses wrong shapes and dtypes -- and the reference tests/test_gpu_kin_env.py
compares against (tests/kin_env_ref.py): identity parameters give the oracle itself, a uniform
scale of every mass and armature scales M and C, and J and b ignore the parameters.

Tolerance of the scaling identity: 1e-12 * (1 + max |ref|), the kinematics tolerance (TOL in
tests/test_gpu_kinematics.py); both sides are the same oracle on trees whose inertial fields
differ by one rounding each, M and C are linear in them."""
import ctypes
import os
import re

import numpy as np
import pytest

import kin_env_ref as ker
import kinematics as kin
from kin_trees import random_tree
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_kin_env_params.h")
TOL = 1e-12


def _trees():
    return {"unitree_go2": kin.load("unitree_go2").d, "random_free": random_tree(5)}


def _state(m, seed):
    return kin.random_state(m, np.random.default_rng(seed), base_pos_zero=False)


def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", open(HEADER).read(),
                              re.M))
    assert declared == set(_lib.KIN_ENV_SYMBOLS) and len(declared) == 6
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS) |
                           set(_lib.ENV_PARAMS_SYMBOLS) | set(_lib.BACKWARD_ENV_SYMBOLS))
    assert L.osc_abi_version() == 4          # additive: ABI 4 callers are untouched


def test_struct_has_the_header_fields_in_order():
    body = re.search(r"typedef struct \{(.*?)\} osc_kin_env_params;", open(HEADER).read(),
                     re.S).group(1)
    fields = re.findall(r"const double\*\s+(\w+);", body)
    assert fields == [n for n, _ in _lib.OscKinEnvParams._fields_]
    assert fields == ["mass_scale", "com_offset", "armature_scale"]
    assert ctypes.sizeof(_lib.OscKinEnvParams) == 3 * ctypes.sizeof(ctypes.c_void_p)


def test_null_handles_are_refused_without_a_device():
    L = _lib.lib()
    nb, sz = ctypes.c_int32(-7), ctypes.c_size_t(123)
    assert L.osc_kin_model_nbody(None, ctypes.byref(nb)) == 1 and nb.value == -7
    assert L.osc_qpos_env_workspace_bytes(None, None, 4, ctypes.byref(sz)) == 1
    assert L.osc_rollout_env_workspace_bytes(None, None, 4, 2, ctypes.byref(sz)) == 1
    assert sz.value == 123
    p = _lib.OscKinEnvParams()
    assert L.osc_batch_kinematics_env(None, 4, None, None, ctypes.byref(p), None, None, None,
                                      None, None, None) == 1
    assert L.osc_batch_solve_qpos_env(None, None, 4, None, None, None, None, None, ctypes.byref(p),
                                      None, None, None, None, None, None, 0, None, 0, None) == 1
    a = _lib.OscRolloutArgs()
    assert L.osc_batch_rollout_env(None, None, 4, ctypes.byref(a), None, ctypes.byref(p),
                                   None) == 1


def test_kin_env_params_checks_types_and_shapes():
    torch = pytest.importorskip("torch")
    from osc_amd.kinematics import KinEnvParams
    with pytest.raises(TypeError):
        KinEnvParams(mass_scale=[[1.0]])
    with pytest.raises(ValueError):
        KinEnvParams(mass_scale=np.ones((3, 13), dtype=np.float32))
    with pytest.raises(ValueError):
        KinEnvParams(armature_scale=torch.ones((3, 18), dtype=torch.float32))
    p = KinEnvParams(mass_scale=np.ones((3, 13)), com_offset=np.zeros((3, 13, 3)),
                     armature_scale=np.ones((3, 18)))
    c, keep = p.to_device(3, 13, 18, "cpu")
    assert len(keep) == 3 and c.mass_scale == keep[0].data_ptr()
    for bad in (dict(mass_scale=np.ones((3, 12))), dict(com_offset=np.zeros((3, 13))),
                dict(armature_scale=np.ones((4, 18)))):
        with pytest.raises(ValueError):
            KinEnvParams(**bad).to_device(3, 13, 18, "cpu")
    c, keep = KinEnvParams().to_device(3, 13, 18, "cpu")
    assert keep == [] and c.mass_scale is None and c.com_offset is None


@pytest.mark.parametrize("name", ["unitree_go2", "random_free"])
def test_identity_parameters_give_the_oracle_exactly(name):
    tree = _trees()[name]
    m = kin.KinModel(tree)
    p = ker.identity(tree, 2)
    assert p["mass_scale"].shape == (2, m.nbody) and p["armature_scale"].shape == (2, m.nv)
    qpos, qvel = _state(m, 3)
    ref = kin.kinematics(m, qpos, qvel)
    for got, want in zip(ker.kinematics(tree, p, 1, qpos, qvel), ref):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("s", [0.5, 1.7])
@pytest.mark.parametrize("name", ["unitree_go2", "random_free"])
def test_uniform_scale_scales_m_and_c(name, s):
    """Every mass_scale = s and every armature_scale = s: M = s M0 and C = s C0."""
    tree = _trees()[name]
    m = kin.KinModel(tree)
    qpos, qvel = _state(m, 11)
    M0, C0, J0, b0 = kin.kinematics(m, qpos, qvel)
    M, C, J, b = kin.kinematics(ker.env_model(tree, mass_scale=np.full(m.nbody, s),
                                              armature_scale=np.full(m.nv, s)), qpos, qvel)
    for got, ref in ((M, s * M0), (C, s * C0)):
        assert np.abs(got - ref).max() <= TOL * (1 + np.abs(ref).max())
    assert np.array_equal(J, J0) and np.array_equal(b, b0)


@pytest.mark.parametrize("name", ["unitree_go2", "random_free"])
def test_j_and_b_ignore_the_parameters_and_m_c_do_not(name):
    tree = _trees()[name]
    m = kin.KinModel(tree)
    p = ker.draw(tree, 3, 21)
    assert (p["mass_scale"] >= 0.5).all() and (p["mass_scale"] <= 2.0).all()
    assert (np.linalg.norm(p["com_offset"], axis=2) <= 0.05 * (1 + 1e-15)).all()
    assert (p["armature_scale"] >= 0.0).all() and (p["armature_scale"] <= 3.0).all()
    assert (p["armature_scale"] == 0.0).any()
    qpos, qvel = _state(m, 5)
    M0, C0, J0, b0 = kin.kinematics(m, qpos, qvel)
    for fields in (("mass_scale",), ("com_offset",), ("armature_scale",), tuple(p)):
        M, C, J, b = ker.kinematics(tree, p, 2, qpos, qvel, fields)
        assert np.array_equal(J, J0) and np.array_equal(b, b0), fields
        assert not np.array_equal(M, M0), fields
        assert np.array_equal(M, M.T) or np.abs(M - M.T).max() <= TOL * (1 + np.abs(M).max())
        if fields != ("armature_scale",):
            assert not np.array_equal(C, C0), fields


def test_armature_scale_must_be_constant_over_a_joints_dofs():
    tree = _trees()["random_free"]
    a = np.ones(kin.KinModel(tree).nv)
    a[1] = 2.0          # inside the free joint's six dofs
    with pytest.raises(ValueError):
        ker.env_tree(tree, armature_scale=a)
